// Source-compatibility check of cudf::lower_bound, upper_bound (include/cudf/search.hpp) and cudf::merge (include/cudf/merge.hpp),
// written the way the reference's search_test.cpp and merge_test.cpp call them: the two examples of search.hpp, a nullable needle
// against a haystack without a mask, a two-table merge with a payload, the N-way form and the rejected inputs. Only the stream type
// differs (hipStream_t through cudf::stream_ref).
#include <cudf/merge.hpp>
#include <cudf/search.hpp>
#include <cudf/sorting.hpp>
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

int main()
{
  using cudf::type_id;
  auto const stream = cudf::get_default_stream();
  auto const asc    = cudf::order::ASCENDING;
  auto const before = cudf::null_order::BEFORE;
  {  // the single-column example of search.hpp
    dev_vec<int32_t> hay{{10, 20, 20, 30, 50}}, needle{{20}};
    cudf::table_view const h{{hay.view(type_id::INT32)}}, n{{needle.view(type_id::INT32)}};
    std::unique_ptr<cudf::column> lo = cudf::lower_bound(h, n, {asc}, {before});
    CHECK(lo->type().id() == type_id::INT32 && lo->null_count() == 0 && lo->size() == 1);
    CHECK((to_host<int32_t>(lo->view()) == std::vector<int32_t>{1}));
    auto up = cudf::upper_bound(h, n, {asc}, {before}, stream, cudf::get_current_device_resource_ref());
    CHECK((to_host<int32_t>(up->view()) == std::vector<int32_t>{3}));
    // a null needle against a haystack without a mask, nulls before and after
    dev_vec<uint32_t> null_mask{{0u}};
    cudf::table_view const nn{{needle.view(type_id::INT32, null_mask.p, 1)}};
    CHECK((to_host<int32_t>(cudf::upper_bound(h, nn, {}, {})->view()) == std::vector<int32_t>{0}));
    CHECK((to_host<int32_t>(cudf::lower_bound(h, nn, {asc}, {cudf::null_order::AFTER})->view()) == std::vector<int32_t>{5}));
  }
  {  // the multi-column example
    dev_vec<int32_t> h0{{10, 20, 20, 20, 20}}, n0{{20}};
    dev_vec<float> h1{{5.0f, .5f, .5f, .7f, .7f}}, n1{{.7f}};
    dev_vec<int8_t> h2{{90, 77, 78, 61, 61}}, n2{{61}};
    cudf::table_view const h{{h0.view(type_id::INT32), h1.view(type_id::FLOAT32), h2.view(type_id::INT8)}};
    cudf::table_view const n{{n0.view(type_id::INT32), n1.view(type_id::FLOAT32), n2.view(type_id::INT8)}};
    std::vector<cudf::order> const orders(3, asc);
    std::vector<cudf::null_order> const nulls(3, before);
    CHECK((to_host<int32_t>(cudf::lower_bound(h, n, orders, nulls)->view()) == std::vector<int32_t>{3}));
    CHECK((to_host<int32_t>(cudf::upper_bound(h, n, orders, nulls)->view()) == std::vector<int32_t>{5}));
  }
  {  // merge: keys with ties inside and across the tables, a payload that tells the rows apart
    dev_vec<int32_t> ka{{1, 1, 3, 7}}, kb{{0, 1, 3, 3, 9}}, kc{{2}};
    dev_vec<int64_t> pa{{100, 101, 102, 103}}, pb{{200, 201, 202, 203, 204}}, pc{{300}};
    cudf::table_view const a{{ka.view(type_id::INT32), pa.view(type_id::INT64)}};
    cudf::table_view const b{{kb.view(type_id::INT32), pb.view(type_id::INT64)}};
    cudf::table_view const c{{kc.view(type_id::INT32), pc.view(type_id::INT64)}};
    std::unique_ptr<cudf::table> two = cudf::merge({a, b}, {0}, {asc});
    CHECK(two->num_columns() == 2 && two->num_rows() == 9);
    CHECK((to_host<int32_t>(two->view().column(0)) == std::vector<int32_t>{0, 1, 1, 1, 3, 3, 3, 7, 9}));
    auto pay = to_host<int64_t>(two->view().column(1));
    auto const pos = [&](int64_t v) { return std::find(pay.begin(), pay.end(), v) - pay.begin(); };
    CHECK(pos(100) < pos(101) && pos(202) < pos(203));  // rows of one table keep their order
    std::sort(pay.begin(), pay.end());
    CHECK((pay == std::vector<int64_t>{100, 101, 102, 103, 200, 201, 202, 203, 204}));
    auto three = cudf::merge({a, b, c}, {0}, {asc}, {before}, stream, cudf::get_current_device_resource_ref());
    CHECK(three->num_rows() == 10 && cudf::is_sorted(three->view().select({0}), {asc}, {}));
    CHECK(cudf::merge({}, {0}, {asc})->num_columns() == 0);
    CHECK(cudf::merge({a}, {0}, {asc})->num_rows() == 4);
    // the rejected inputs
    int threw = 0;
    auto const expect_logic_error = [&](auto&& f) {
      try {
        f();
      } catch (cudf::logic_error const&) {
        ++threw;
      }
    };
    expect_logic_error([&] { (void)cudf::merge({a, cudf::table_view{{ka.view(type_id::INT32)}}}, {0}, {asc}); });
    expect_logic_error([&] { (void)cudf::merge({a, cudf::table_view{{ka.view(type_id::INT32), ka.view(type_id::INT32)}}}, {0}, {asc}); });
    expect_logic_error([&] { (void)cudf::merge({a, b}, {}, {asc}); });
    expect_logic_error([&] { (void)cudf::merge({a, b}, {0, 1, 0}, {asc, asc, asc}); });
    expect_logic_error([&] { (void)cudf::merge({a, b}, {0}, {}); });
    expect_logic_error([&] { (void)cudf::merge({a, b}, {0}, {asc}, {before, before}); });
    expect_logic_error([&] { (void)cudf::merge({a, b}, {2}, {asc}); });
    expect_logic_error([&] { (void)cudf::merge({a, b}, {1, 1}, {asc, asc}); });
    expect_logic_error([&] { (void)cudf::lower_bound(a, b, {asc}, {}); });
    expect_logic_error([&] { (void)cudf::upper_bound(a, b, {}, {before}); });
    CHECK(threw == 10);
    try {
      (void)cudf::lower_bound(a, cudf::table_view{{ka.view(type_id::INT32)}}, {}, {});
    } catch (std::invalid_argument const&) {
      ++threw;
    }
    try {
      (void)cudf::upper_bound(a, cudf::table_view{{ka.view(type_id::INT32), ka.view(type_id::INT32)}}, {}, {});
    } catch (std::invalid_argument const&) {
      ++threw;
    }
    CHECK(threw == 12);
  }
  std::printf("search_merge_compat OK\n");
  return 0;
}
