// Source-compatibility check of cudf::drop_nulls, drop_nans, apply_boolean_mask, apply_deletion_mask, unique
// (include/cudf/stream_compaction.hpp) and cudf::unique_count (include/cudf/reduction/unique_count.hpp), written the way the
// reference's stream_compaction tests call them: every signature with its defaulted arguments, one known answer each, and the
// exception types. Only the stream type differs (hipStream_t through cudf::stream_ref).
#include <cudf/reduction/unique_count.hpp>
#include <cudf/stream_compaction.hpp>
#include <cudf/table/table.hpp>
#include <cudf/utilities/error.hpp>

#include <hip/hip_runtime.h>

#include <algorithm>
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
  [[nodiscard]] cudf::column_view view(cudf::type_id id, uint32_t const* mask = nullptr, cudf::size_type nulls = 0) const
  {
    return cudf::column_view{cudf::data_type{id}, static_cast<cudf::size_type>(n), p, mask, nulls};
  }
};

template <typename T>
std::vector<T> to_host(cudf::column_view const& c)
{
  std::vector<T> h(c.size());
  (void)hipMemcpy(h.data(), c.head<T>() + c.offset(), h.size() * sizeof(T), hipMemcpyDeviceToHost);
  return h;
}

uint32_t mask_word(cudf::column_view const& c)
{
  uint32_t w = 0;
  (void)hipMemcpy(&w, c.null_mask(), sizeof(w), hipMemcpyDeviceToHost);
  return w;
}

int main()
{
  using cudf::type_id;
  auto const stream = cudf::get_default_stream();
  auto const mr     = cudf::get_current_device_resource_ref();
  // rows 0..5; the int32 column is null in rows 2 and 5 (bits 0b011011), the float column holds NaN in rows 1 and 2
  dev_vec<int32_t> a{{10, 40, 70, 5, 2, 10}};
  dev_vec<uint32_t> a_mask{{0b011011u}};
  dev_vec<float> f{{1.f, NAN, NAN, 4.f, 5.f, 6.f}};
  dev_vec<int64_t> pay{{100, 101, 102, 103, 104, 105}};
  cudf::table_view const t{{a.view(type_id::INT32, a_mask.p, 2), f.view(type_id::FLOAT32), pay.view(type_id::INT64)}};
  {  // apply_boolean_mask / apply_deletion_mask: a null mask element drops the row in both
    dev_vec<uint8_t> m{{1, 0, 1, 0, 1, 1}};
    dev_vec<uint32_t> m_mask{{0b011111u}};
    std::unique_ptr<cudf::table> kept = cudf::apply_boolean_mask(t, m.view(type_id::BOOL8, m_mask.p, 1));
    CHECK(kept->num_columns() == 3 && kept->num_rows() == 3);
    CHECK((to_host<int64_t>(kept->view().column(2)) == std::vector<int64_t>{100, 102, 104}));
    CHECK(kept->view().column(0).nullable() && kept->view().column(0).null_count() == 1 && mask_word(kept->view().column(0)) == 0b101u);
    CHECK(!kept->view().column(1).nullable() && !kept->view().column(2).nullable());
    auto deleted = cudf::apply_deletion_mask(t, m.view(type_id::BOOL8, m_mask.p, 1), stream, mr);
    CHECK((to_host<int64_t>(deleted->view().column(2)) == std::vector<int64_t>{101, 103}));
    dev_vec<uint8_t> none{{}};
    CHECK(cudf::apply_boolean_mask(t, none.view(type_id::BOOL8))->num_rows() == 0);
  }
  {  // drop_nulls / drop_nans, with and without a threshold
    std::unique_ptr<cudf::table> d = cudf::drop_nulls(t, {0, 1});
    CHECK((to_host<int64_t>(d->view().column(2)) == std::vector<int64_t>{100, 101, 103, 104}));
    CHECK(d->view().column(0).nullable() && d->view().column(0).null_count() == 0 && mask_word(d->view().column(0)) == 0b1111u);
    CHECK(cudf::drop_nulls(t, {0, 1}, 1)->num_rows() == 6);
    CHECK(cudf::drop_nulls(t, {0, 1}, 2, stream, mr)->num_rows() == 4);
    CHECK(cudf::drop_nulls(t, {0}, stream, mr)->num_rows() == 4);
    CHECK(cudf::drop_nulls(t, {1, 2}, 7)->num_rows() == 6);  // no key has a null: a copy, whatever the threshold
    auto n = cudf::drop_nans(t, {1});
    CHECK((to_host<int64_t>(n->view().column(2)) == std::vector<int64_t>{100, 103, 104, 105}));
    CHECK(cudf::drop_nans(t, {1}, 0)->num_rows() == 6);
    CHECK(cudf::drop_nans(t, {1}, 1, stream, mr)->num_rows() == 4);
    CHECK(cudf::drop_nans(t, {}, stream, mr)->num_rows() == 6);
  }
  {  // unique / unique_count on a sorted key
    dev_vec<int32_t> k{{1, 1, 2, 3, 3, 3}};
    cudf::table_view const s{{k.view(type_id::INT32), pay.view(type_id::INT64)}};
    std::unique_ptr<cudf::table> first = cudf::unique(s, {0}, cudf::duplicate_keep_option::KEEP_FIRST);
    CHECK((to_host<int64_t>(first->view().column(1)) == std::vector<int64_t>{100, 102, 103}));
    auto any = cudf::unique(s, {0}, cudf::duplicate_keep_option::KEEP_ANY, cudf::null_equality::UNEQUAL);
    CHECK((to_host<int64_t>(any->view().column(1)) == std::vector<int64_t>{100, 102, 103}));
    auto last = cudf::unique(s, {0}, cudf::duplicate_keep_option::KEEP_LAST, cudf::null_equality::EQUAL, stream, mr);
    CHECK((to_host<int64_t>(last->view().column(1)) == std::vector<int64_t>{101, 102, 105}));
    CHECK((to_host<int64_t>(cudf::unique(s, {0}, cudf::duplicate_keep_option::KEEP_NONE)->view().column(1)) == std::vector<int64_t>{102}));
    CHECK(cudf::unique(s, {}, cudf::duplicate_keep_option::KEEP_FIRST)->num_rows() == 0);
    cudf::size_type const rows = cudf::unique_count(cudf::table_view{{k.view(type_id::INT32)}});
    CHECK(rows == 3 && cudf::unique_count(s, cudf::null_equality::UNEQUAL, stream) == 6);
    CHECK(cudf::unique_count(k.view(type_id::INT32), cudf::null_policy::INCLUDE, cudf::nan_policy::NAN_IS_VALID) == 3);
    // {10, 40, null, 5, 2, null}: a null never counts under EXCLUDE; NaN, NaN is one run, or none when NaN is null
    CHECK(cudf::unique_count(a.view(type_id::INT32, a_mask.p, 2), cudf::null_policy::EXCLUDE, cudf::nan_policy::NAN_IS_VALID, stream) == 4);
    CHECK(cudf::unique_count(f.view(type_id::FLOAT32), cudf::null_policy::INCLUDE, cudf::nan_policy::NAN_IS_VALID) == 5);
    CHECK(cudf::unique_count(f.view(type_id::FLOAT32), cudf::null_policy::EXCLUDE, cudf::nan_policy::NAN_IS_NULL) == 4);
  }
  {  // the rejected inputs
    int threw = 0;
    auto const expect_logic_error = [&](auto&& fn) {
      try {
        fn();
      } catch (cudf::logic_error const&) {
        ++threw;
      }
    };
    dev_vec<uint8_t> five{{1, 1, 1, 1, 1}};
    expect_logic_error([&] { (void)cudf::apply_boolean_mask(t, five.view(type_id::BOOL8)); });
    expect_logic_error([&] { (void)cudf::apply_deletion_mask(t, five.view(type_id::BOOL8)); });
    expect_logic_error([&] { (void)cudf::apply_boolean_mask(t, a.view(type_id::INT32)); });
    expect_logic_error([&] { (void)cudf::drop_nans(t, {1, 0}); });
    CHECK(threw == 4);
    auto const expect_out_of_range = [&](auto&& fn) {
      try {
        fn();
      } catch (std::out_of_range const&) {
        ++threw;
      }
    };
    expect_out_of_range([&] { (void)cudf::drop_nulls(t, {0, 3}); });
    expect_out_of_range([&] { (void)cudf::drop_nans(t, {3}, 1); });
    expect_out_of_range([&] { (void)cudf::unique(t, {-1}, cudf::duplicate_keep_option::KEEP_FIRST); });
    CHECK(threw == 7);
  }
  std::printf("copy_if_compat OK\n");
  return 0;
}
