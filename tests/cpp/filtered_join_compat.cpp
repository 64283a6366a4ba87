// Source-compatibility check of cudf::filtered_join (include/cudf/join/filtered_join.hpp), written the way the reference's
// semi_anti_join_tests.cpp uses the class: built on the right (filter) table, probed by semi_join / anti_join, whose
// device_uvector results serve as gather maps (TestSimple, AntiJoinEmptyTables, InvalidLoadFactor), plus the contract's null
// rule and the rejected probes. Only the stream type differs (hipStream_t through cudf::stream_ref).
#include <cudf/join/filtered_join.hpp>
#include <cudf/table/table.hpp>
#include <cudf/utilities/error.hpp>

#include <hip/hip_runtime.h>

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

std::vector<cudf::size_type> to_host(rmm::device_uvector<cudf::size_type> const& v)
{
  std::vector<cudf::size_type> h(v.size());
  (void)hipMemcpy(h.data(), v.data(), h.size() * sizeof(cudf::size_type), hipMemcpyDeviceToHost);
  return h;
}

int main()
{
  auto const stream = cudf::get_default_stream();
  // TestSimple (semi_anti_join_tests.cpp:117-134): left {0, 1, 2}, right {0, 1, 3}
  dev_vec<int32_t> l{{0, 1, 2}}, r{{0, 1, 3}};
  cudf::column_view lc{cudf::data_type{cudf::type_id::INT32}, 3, l.p, nullptr, 0};
  cudf::column_view rc{cudf::data_type{cudf::type_id::INT32}, 3, r.p, nullptr, 0};
  cudf::table_view const left{{lc}}, right{{rc}};
  {
    cudf::filtered_join obj(right, cudf::null_equality::EQUAL, stream);
    std::unique_ptr<rmm::device_uvector<cudf::size_type>> semi = obj.semi_join(left, stream, cudf::get_current_device_resource_ref());
    auto anti = obj.anti_join(left);
    CHECK((to_host(*semi) == std::vector<cudf::size_type>{0, 1}));
    CHECK((to_host(*anti) == std::vector<cudf::size_type>{2}));
    // probed again: same answer
    CHECK((to_host(*obj.semi_join(left, stream)) == std::vector<cudf::size_type>{0, 1}));
  }
  // the load-factor constructor, and an invalid load factor (InvalidLoadFactor, :520-532)
  {
    cudf::filtered_join obj(right, cudf::null_equality::UNEQUAL, 0.25, stream);
    CHECK((to_host(*obj.anti_join(left, stream)) == std::vector<cudf::size_type>{2}));
    for (double lf : {-0.1, 0.0, 1.1}) {
      bool threw = false;
      try {
        cudf::filtered_join bad(right, cudf::null_equality::EQUAL, lf, stream);
      } catch (std::invalid_argument const&) {
        threw = true;
      }
      CHECK(threw);
    }
  }
  // AntiJoinEmptyTables (:358-389): an empty right table keeps every left row; an empty left table yields nothing
  {
    cudf::table empty{};
    cudf::filtered_join obj(empty.view(), cudf::null_equality::EQUAL, stream);
    CHECK((to_host(*obj.anti_join(left, stream)) == std::vector<cudf::size_type>{0, 1, 2}));
    CHECK(obj.semi_join(left, stream)->size() == 0);
    cudf::filtered_join full(right, cudf::null_equality::EQUAL, stream);
    CHECK(full.anti_join(empty.view(), stream)->size() == 0 && full.semi_join(empty.view(), stream)->size() == 0);
  }
  // nulls: left {1, null, 3}, right {null, 3}: EQUAL -> semi {1, 2}; UNEQUAL -> semi {2}, anti {0, 1}
  {
    dev_vec<int32_t> lv{{1, 0, 3}}, rv{{0, 3}};
    dev_vec<cudf::bitmask_type> lm{{0b101u}}, rm{{0b10u}};
    cudf::column_view lcn{cudf::data_type{cudf::type_id::INT32}, 3, lv.p, lm.p, 1};
    cudf::column_view rcn{cudf::data_type{cudf::type_id::INT32}, 2, rv.p, rm.p, 1};
    cudf::filtered_join eq(cudf::table_view{{rcn}}, cudf::null_equality::EQUAL, stream);
    cudf::filtered_join ne(cudf::table_view{{rcn}}, cudf::null_equality::UNEQUAL, stream);
    CHECK((to_host(*eq.semi_join(cudf::table_view{{lcn}}, stream)) == std::vector<cudf::size_type>{1, 2}));
    CHECK((to_host(*ne.semi_join(cudf::table_view{{lcn}}, stream)) == std::vector<cudf::size_type>{2}));
    CHECK((to_host(*ne.anti_join(cudf::table_view{{lcn}}, stream)) == std::vector<cudf::size_type>{0, 1}));
  }
  // rejected probes: column count -> std::invalid_argument, column type -> cudf::data_type_error
  {
    cudf::filtered_join obj(right, cudf::null_equality::EQUAL, stream);
    bool count_threw = false, type_threw = false;
    try {
      (void)obj.semi_join(cudf::table_view{{lc, lc}}, stream);
    } catch (std::invalid_argument const&) {
      count_threw = true;
    }
    dev_vec<int64_t> l64{{0, 1, 2}};
    cudf::column_view l64c{cudf::data_type{cudf::type_id::INT64}, 3, l64.p, nullptr, 0};
    try {
      (void)obj.anti_join(cudf::table_view{{l64c}}, stream);
    } catch (cudf::data_type_error const&) {
      type_threw = true;
    }
    CHECK(count_threw && type_threw);
  }
  CHECK(hipDeviceSynchronize() == hipSuccess);
  std::printf("filtered_join_compat OK\n");
  return 0;
}
