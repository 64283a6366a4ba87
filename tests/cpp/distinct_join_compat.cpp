// Source-compatibility check of cudf::distinct_hash_join (include/cudf/join/distinct_hash_join.hpp), written the way the
// reference's distinct_join_tests.cpp uses the class: built on the right table with every constructor arity, probed by inner_join
// (a pair of device_uvectors) and left_join (one device_uvector that is a gather map), with default and explicit stream and memory
// resource (PrimitiveLeftJoinWithNulls, EmptyRightTable*, InvalidLoadFactor), plus the contract's throwing cases. Only the stream
// type differs (hipStream_t through cudf::stream_ref).
#include <cudf/join/distinct_hash_join.hpp>
#include <cudf/table/table.hpp>
#include <cudf/utilities/error.hpp>

#include <hip/hip_runtime.h>

#include <cstdio>
#include <memory>
#include <stdexcept>
#include <type_traits>
#include <utility>
#include <vector>

#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) {                                                                   \
      std::fprintf(stderr, "FAILED %s at %s:%d\n", #cond, __FILE__, __LINE__);       \
      return 1;                                                                      \
    }                                                                                \
  } while (0)

static_assert(!std::is_copy_constructible_v<cudf::distinct_hash_join> && !std::is_move_constructible_v<cudf::distinct_hash_join>);
static_assert(!std::is_copy_assignable_v<cudf::distinct_hash_join> && !std::is_move_assignable_v<cudf::distinct_hash_join>);
static_assert(!std::is_default_constructible_v<cudf::distinct_hash_join>);

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

using indices = std::vector<cudf::size_type>;

indices to_host(rmm::device_uvector<cudf::size_type> const& v)
{
  indices h(v.size());
  (void)hipMemcpy(h.data(), v.data(), h.size() * sizeof(cudf::size_type), hipMemcpyDeviceToHost);
  return h;
}

int main()
{
  auto const stream      = cudf::get_default_stream();
  auto const mr          = cudf::get_current_device_resource_ref();
  constexpr auto NoMatch = cudf::JoinNoMatch;
  // PrimitiveLeftJoinWithNulls (distinct_join_tests.cpp:614-649): 5 rows of two INT32 columns, a null in the left table
  dev_vec<int32_t> l0{{3, 1, 2, 0, 2}}, l1{{1, 1, -1, 4, 0}}, r0{{2, 2, 0, 4, 3}}, r1{{1, 0, 1, 2, 1}};
  dev_vec<cudf::bitmask_type> l1m{{0b11011u}};
  cudf::data_type const i32{cudf::type_id::INT32};
  cudf::column_view lc0{i32, 5, l0.p, nullptr, 0}, lc1{i32, 5, l1.p, l1m.p, 1}, rc0{i32, 5, r0.p, nullptr, 0}, rc1{i32, 5, r1.p, nullptr, 0};
  cudf::table_view const left{{lc0, lc1}}, right{{rc0, rc1}};
  indices const gold_left_join{4, NoMatch, NoMatch, NoMatch, 1}, gold_l{0, 4}, gold_r{4, 1};
  {
    // every constructor arity
    cudf::distinct_hash_join a1{right};
    cudf::distinct_hash_join a2{right, cudf::null_equality::EQUAL};
    cudf::distinct_hash_join a3{right, cudf::null_equality::UNEQUAL, 0.5};
    cudf::distinct_hash_join a4(right, cudf::null_equality::EQUAL, 1.0, stream);
    cudf::distinct_hash_join a5(right, cudf::null_equality::EQUAL, 0.25, stream, mr);
    for (cudf::distinct_hash_join const* obj : {&a1, &a2, &a3, &a4, &a5}) {
      // default stream and mr, then explicit ones
      std::unique_ptr<rmm::device_uvector<cudf::size_type>> lj = obj->left_join(left);
      CHECK(to_host(*lj) == gold_left_join);
      CHECK(to_host(*obj->left_join(left, stream)) == gold_left_join);
      CHECK(to_host(*obj->left_join(left, stream, mr)) == gold_left_join);
      std::pair<std::unique_ptr<rmm::device_uvector<cudf::size_type>>, std::unique_ptr<rmm::device_uvector<cudf::size_type>>> ij =
        obj->inner_join(left);
      CHECK(to_host(*ij.first) == gold_l && to_host(*ij.second) == gold_r);
      auto [li, ri] = obj->inner_join(left, stream, mr);
      CHECK(to_host(*li) == gold_l && to_host(*ri) == gold_r);
      CHECK(to_host(*obj->inner_join(left, stream).first) == gold_l);
    }
  }
  // nulls: left {1, null, 3}, right {null, 3}: EQUAL -> {NoMatch, 0, 1}; UNEQUAL -> {NoMatch, NoMatch, 1}
  {
    dev_vec<int32_t> lv{{1, 0, 3}}, rv{{0, 3}};
    dev_vec<cudf::bitmask_type> lm{{0b101u}}, rm{{0b10u}};
    cudf::column_view lcn{i32, 3, lv.p, lm.p, 1}, rcn{i32, 2, rv.p, rm.p, 1};
    cudf::distinct_hash_join eq{cudf::table_view{{rcn}}, cudf::null_equality::EQUAL};
    cudf::distinct_hash_join ne{cudf::table_view{{rcn}}, cudf::null_equality::UNEQUAL};
    CHECK((to_host(*eq.left_join(cudf::table_view{{lcn}})) == indices{NoMatch, 0, 1}));
    CHECK((to_host(*ne.left_join(cudf::table_view{{lcn}})) == indices{NoMatch, NoMatch, 1}));
    CHECK((to_host(*ne.inner_join(cudf::table_view{{lcn}}).first) == indices{2}));
  }
  // EmptyRightTable* / EmptyLeftTable* (:409-503): no right rows -> no pairs, every left row JoinNoMatch; no left rows -> empty
  {
    cudf::column_view e0{i32, 0, nullptr, nullptr, 0};
    cudf::table_view const none{{e0, e0}};
    cudf::distinct_hash_join obj{none};
    CHECK(obj.inner_join(left).first->size() == 0 && obj.inner_join(left).second->size() == 0);
    CHECK((to_host(*obj.left_join(left)) == indices(5, NoMatch)));
    cudf::distinct_hash_join full{right};
    CHECK(full.inner_join(none).first->size() == 0 && full.left_join(none)->size() == 0);
  }
  // the three throwing cases: a right table without columns (cudf::logic_error), a load factor outside (0, 1]
  // (std::invalid_argument; InvalidLoadFactor, :713-734), a probe of another shape (std::invalid_argument / cudf::data_type_error)
  {
    bool no_columns_threw = false;
    try {
      cudf::table empty{};
      cudf::distinct_hash_join bad{empty.view()};
    } catch (cudf::logic_error const&) {
      no_columns_threw = true;
    }
    CHECK(no_columns_threw);
    for (double lf : {-0.1, 0.0, 1.1}) {
      bool threw = false;
      try {
        cudf::distinct_hash_join bad(right, cudf::null_equality::EQUAL, lf);
      } catch (std::invalid_argument const&) {
        threw = true;
      }
      CHECK(threw);
    }
    cudf::distinct_hash_join obj{right};
    bool count_threw = false, type_threw = false;
    try {
      (void)obj.inner_join(cudf::table_view{{lc0}});
    } catch (std::invalid_argument const&) {
      count_threw = true;
    }
    dev_vec<int64_t> l64{{0, 1, 2, 3, 4}};
    cudf::column_view l64c{cudf::data_type{cudf::type_id::INT64}, 5, l64.p, nullptr, 0};
    try {
      (void)obj.left_join(cudf::table_view{{lc0, l64c}});
    } catch (cudf::data_type_error const&) {
      type_threw = true;
    }
    CHECK(count_threw && type_threw);
  }
  CHECK(hipDeviceSynchronize() == hipSuccess);
  std::printf("distinct_join_compat OK\n");
  return 0;
}
