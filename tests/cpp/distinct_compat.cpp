// Source-compatibility check of cudf::distinct, distinct_indices, stable_distinct (include/cudf/stream_compaction.hpp) and
// cudf::distinct_count (include/cudf/reduction/distinct_count.hpp), written the way the reference's distinct_tests.cpp,
// stable_distinct_tests.cpp and distinct_count_tests.cpp call them (InputWithNullsEqual, InputWithNaNsUnequal, EmptyKeys,
// TableWithNull), plus an out-of-range key. Only the stream type differs (hipStream_t through cudf::stream_ref).
#include <cudf/reduction/distinct_count.hpp>
#include <cudf/stream_compaction.hpp>
#include <cudf/table/table.hpp>
#include <cudf/utilities/error.hpp>

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <memory>
#include <stdexcept>
#include <vector>

#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) {                                                                   \
      std::fprintf(stderr, "FAILED %s at %s:%d\n", #cond, __FILE__, __LINE__);       \
      return 1;                                                                      \
    }                                                                                \
  } while (0)

template <typename T>
struct dev_vec {
  T* p{};
  size_t n;
  explicit dev_vec(std::vector<T> const& h) : n{h.size()}
  {
    (void)hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T));
    (void)hipMemcpy(p, h.data(), n * sizeof(T), hipMemcpyHostToDevice);
  }
  ~dev_vec() { (void)hipFree(p); }
};

template <typename T>
std::vector<T> to_host(cudf::column_view const& c)
{
  std::vector<T> h(c.size());
  (void)hipMemcpy(h.data(), c.head<T>() + c.offset(), h.size() * sizeof(T), hipMemcpyDeviceToHost);
  return h;
}

int main()
{
  auto const stream = cudf::get_default_stream();
  using cudf::duplicate_keep_option;
  // InputWithNullsEqual (distinct_tests.cpp:437-476): col {0..6}, keys {20, null, null, 19, 21, 19, 22}
  dev_vec<int32_t> col{{0, 1, 2, 3, 4, 5, 6}}, keys{{20, 0, 0, 19, 21, 19, 22}};
  dev_vec<uint32_t> mask{{0b1111001u}};
  cudf::column_view cc{cudf::data_type{cudf::type_id::INT32}, 7, col.p, nullptr, 0};
  cudf::column_view kc{cudf::data_type{cudf::type_id::INT32}, 7, keys.p, mask.p, 2};
  cudf::table_view const input{{cc, kc}};
  {
    std::unique_ptr<cudf::table> first =
      cudf::stable_distinct(input, {1}, duplicate_keep_option::KEEP_FIRST, cudf::null_equality::EQUAL, cudf::nan_equality::ALL_EQUAL,
                            stream, cudf::get_current_device_resource_ref());
    CHECK((to_host<int32_t>(first->view().column(0)) == std::vector<int32_t>{0, 1, 3, 4, 6}));
    auto last = cudf::stable_distinct(input, {1}, duplicate_keep_option::KEEP_LAST);
    CHECK((to_host<int32_t>(last->view().column(0)) == std::vector<int32_t>{0, 2, 4, 5, 6}));
    auto none = cudf::distinct(input, {1}, duplicate_keep_option::KEEP_NONE, cudf::null_equality::EQUAL);
    CHECK((to_host<int32_t>(none->view().column(0)) == std::vector<int32_t>{0, 4, 6}));
    CHECK(none->view().column(1).null_count() == 0);
    std::unique_ptr<cudf::column> idx = cudf::distinct_indices(input.select({1}), duplicate_keep_option::KEEP_FIRST);
    CHECK((to_host<int32_t>(idx->view()) == std::vector<int32_t>{0, 1, 3, 4, 6}));
    auto any = cudf::distinct(input, {1});
    CHECK(any->num_rows() == 5);
  }
  // InputWithNaNsUnequal (:563-602)
  dev_vec<float> fk{{20.f, NAN, NAN, 19.f, 21.f, 19.f, 22.f, 20.f}};
  dev_vec<int32_t> fcol{{0, 1, 2, 3, 4, 5, 6, 7}};
  cudf::column_view fkc{cudf::data_type{cudf::type_id::FLOAT32}, 8, fk.p, nullptr, 0};
  cudf::column_view fcc{cudf::data_type{cudf::type_id::INT32}, 8, fcol.p, nullptr, 0};
  cudf::table_view const finput{{fcc, fkc}};
  {
    auto none = cudf::stable_distinct(finput, {1}, duplicate_keep_option::KEEP_NONE, cudf::null_equality::UNEQUAL, cudf::nan_equality::UNEQUAL);
    CHECK((to_host<int32_t>(none->view().column(0)) == std::vector<int32_t>{1, 2, 4, 6}));
  }
  // EmptyKeys (:130-139): an empty table of the input's schema
  CHECK(cudf::distinct(input, {}, duplicate_keep_option::KEEP_ANY)->num_rows() == 0);
  // a key outside the table
  bool threw = false;
  try {
    (void)cudf::distinct(input, {2});
  } catch (std::out_of_range const&) {
    threw = true;
  }
  CHECK(threw);
  // distinct_count (distinct_count_tests.cpp TableWithNull :249-261; a column with nulls and NaN)
  dev_vec<int32_t> a{{5, 4, 3, 5, 8, 1, 4, 5, 0, 9, -1}}, b{{2, 2, 2, -1, 2, 1, 2, 0, 0, 9, -1}};
  dev_vec<uint32_t> am{{0b01011111111u}}, bm{{0b01001110111u}};
  cudf::column_view ac{cudf::data_type{cudf::type_id::INT32}, 11, a.p, am.p, 2};
  cudf::column_view bc{cudf::data_type{cudf::type_id::INT32}, 11, b.p, bm.p, 3};
  CHECK(cudf::distinct_count(cudf::table_view{{ac, bc}}, cudf::null_equality::EQUAL) == 8);
  CHECK(cudf::distinct_count(cudf::table_view{{ac, bc}}, cudf::null_equality::UNEQUAL, stream) == 10);
  dev_vec<uint32_t> nm{{0b10111u}};
  dev_vec<float> nv{{1.f, 3.f, NAN, 70.f, 31.f}};
  cudf::column_view nc{cudf::data_type{cudf::type_id::FLOAT32}, 5, nv.p, nm.p, 1};
  CHECK(cudf::distinct_count(nc, cudf::null_policy::EXCLUDE, cudf::nan_policy::NAN_IS_NULL) == 3);  // NansAsNullWithIgnoreNull
  CHECK(cudf::distinct_count(nc, cudf::null_policy::INCLUDE, cudf::nan_policy::NAN_IS_NULL, stream) == 4);
  std::printf("distinct_compat OK\n");
  return 0;
}
