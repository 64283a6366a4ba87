// Source-compatibility check of cudf::sorted_order, sort_by_key and is_sorted (include/cudf/sorting.hpp), written the way the
// reference's sort_test.cpp and is_sorted_tests.cpp call them (WithNullMin's table with the strings column as code points,
// ValueKeysSizeMismatch, MismatchInColumnOrderSize). Only the stream type differs (hipStream_t through cudf::stream_ref).
#include <cudf/sorting.hpp>
#include <cudf/table/table.hpp>
#include <cudf/utilities/error.hpp>

#include <hip/hip_runtime.h>

#include <cstdio>
#include <memory>
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
  // WithNullMin (sort_test.cpp:86-116): row 2 is null in every column
  dev_vec<int32_t> c1{{5, 4, 3, 5, 8}}, c2{{'d', 'e', 0, 'd', 'k'}}, c3{{10, 40, 70, 5, 2}};
  dev_vec<int64_t> pay{{100, 101, 102, 103, 104}};
  dev_vec<uint32_t> mask{{0b11011u}};
  cudf::column_view k1{cudf::data_type{cudf::type_id::INT32}, 5, c1.p, mask.p, 1};
  cudf::column_view k2{cudf::data_type{cudf::type_id::INT32}, 5, c2.p, mask.p, 1};
  cudf::column_view k3{cudf::data_type{cudf::type_id::INT32}, 5, c3.p, mask.p, 1};
  cudf::column_view pc{cudf::data_type{cudf::type_id::INT64}, 5, pay.p, nullptr, 0};
  cudf::table_view const keys{{k1, k2, k3}};
  std::vector<cudf::order> const column_order{cudf::order::ASCENDING, cudf::order::ASCENDING, cudf::order::DESCENDING};
  {
    std::unique_ptr<cudf::column> got = cudf::sorted_order(keys, column_order);
    CHECK(got->type().id() == cudf::type_id::INT32 && got->null_count() == 0);
    CHECK((to_host<int32_t>(got->view()) == std::vector<int32_t>{2, 1, 0, 3, 4}));
    auto stable = cudf::stable_sorted_order(keys, column_order, {}, stream, cudf::get_current_device_resource_ref());
    CHECK((to_host<int32_t>(stable->view()) == std::vector<int32_t>{2, 1, 0, 3, 4}));
    // defaulted arguments: all ascending, nulls before
    std::unique_ptr<cudf::table> by_key = cudf::sort_by_key(cudf::table_view{{pc}}, keys);
    CHECK((to_host<int64_t>(by_key->view().column(0)) == std::vector<int64_t>{102, 101, 103, 100, 104}));
    auto sorted = cudf::sort(keys, column_order);
    CHECK(sorted->num_columns() == 3 && sorted->num_rows() == 5);
    CHECK(sorted->view().column(0).null_count() == 1);
    CHECK(cudf::is_sorted(sorted->view(), column_order, {}));
    CHECK(!cudf::is_sorted(keys, column_order, {}, stream));
    CHECK(cudf::is_sorted(cudf::stable_sort_by_key(keys, keys)->view(), {}, {}));
    CHECK(cudf::stable_sort(keys)->num_rows() == 5);
  }
  // ValueKeysSizeMismatch, MismatchInColumnOrderSize, MismatchInNullPrecedenceSize
  int threw = 0;
  try {
    (void)cudf::sort_by_key(cudf::table_view{{pc}}, cudf::table_view{{cudf::column_view{cudf::data_type{cudf::type_id::INT32}, 4, c1.p, nullptr, 0}}});
  } catch (cudf::logic_error const&) {
    ++threw;
  }
  try {
    (void)cudf::sorted_order(keys, {cudf::order::ASCENDING, cudf::order::DESCENDING});
  } catch (cudf::logic_error const&) {
    ++threw;
  }
  try {
    (void)cudf::is_sorted(keys, {}, {cudf::null_order::AFTER, cudf::null_order::BEFORE});
  } catch (cudf::logic_error const&) {
    ++threw;
  }
  CHECK(threw == 3);
  std::printf("sorting_compat OK\n");
  return 0;
}
