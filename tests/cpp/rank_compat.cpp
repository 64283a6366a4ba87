// Source-compatibility check of cudf::rank (include/cudf/sorting.hpp), written the way the reference's rank_test.cpp calls it: the
// three documented examples of the reference header (cpp/include/cudf/sorting.hpp:171-201) for every rank_method. Only the stream
// type differs (hipStream_t through cudf::stream_ref).
#include <cudf/sorting.hpp>
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

// the ranks as doubles, -1 under a null
std::vector<double> ranks_of(cudf::column const& c)
{
  std::vector<double> out;
  if (c.type().id() == cudf::type_id::FLOAT64) {
    out = to_host<double>(c.view());
  } else {
    for (auto v : to_host<int32_t>(c.view())) out.push_back(v);
  }
  if (c.nullable()) {
    std::vector<uint32_t> m((c.size() + 31) / 32);
    (void)hipMemcpy(m.data(), c.view().null_mask(), m.size() * sizeof(uint32_t), hipMemcpyDeviceToHost);
    for (int i = 0; i < c.size(); ++i)
      if (!((m[i / 32] >> (i % 32)) & 1u)) out[i] = -1;
  }
  return out;
}

int main()
{
  using cudf::rank_method;
  auto const stream = cudf::get_default_stream();
  dev_vec<int32_t> data{{3, 4, 5, 4, 1, 2}};
  dev_vec<uint32_t> mask{{0b111011u}};  // row 2 is null
  cudf::column_view const plain{cudf::data_type{cudf::type_id::INT32}, 6, data.p, nullptr, 0};
  cudf::column_view const with_null{cudf::data_type{cudf::type_id::INT32}, 6, data.p, mask.p, 1};
  std::vector<rank_method> const methods{rank_method::FIRST, rank_method::AVERAGE, rank_method::MIN, rank_method::MAX,
                                         rank_method::DENSE};
  using rows = std::vector<std::vector<double>>;
  // "Using default order::ASCENDING"
  rows const no_nulls{{3, 4, 6, 5, 1, 2}, {3, 4.5, 6, 4.5, 1, 2}, {3, 4, 6, 4, 1, 2}, {3, 5, 6, 5, 1, 2}, {3, 4, 5, 4, 1, 2}};
  // "For null_policy::INCLUDE, null_order::BEFORE"
  rows const include_before{{4, 5, 1, 6, 2, 3}, {4, 5.5, 1, 5.5, 2, 3}, {4, 5, 1, 5, 2, 3}, {4, 6, 1, 6, 2, 3}, {4, 5, 1, 5, 2, 3}};
  // "For null_policy::EXCLUDE (null_order::AFTER only)"
  rows const exclude_after{{3, 4, -1, 5, 1, 2}, {3, 4.5, -1, 4.5, 1, 2}, {3, 4, -1, 4, 1, 2}, {3, 5, -1, 5, 1, 2}, {3, 4, -1, 4, 1, 2}};
  for (std::size_t m = 0; m < methods.size(); ++m) {
    std::unique_ptr<cudf::column> got =
      cudf::rank(plain, methods[m], cudf::order::ASCENDING, cudf::null_policy::EXCLUDE, cudf::null_order::AFTER, false);
    CHECK(got->type().id() == (methods[m] == rank_method::AVERAGE ? cudf::type_id::FLOAT64 : cudf::type_id::INT32));
    CHECK(got->size() == 6 && !got->nullable() && got->null_count() == 0);
    CHECK(ranks_of(*got) == no_nulls[m]);
    got = cudf::rank(with_null, methods[m], cudf::order::ASCENDING, cudf::null_policy::INCLUDE, cudf::null_order::BEFORE, false,
                     stream, cudf::get_current_device_resource_ref());
    CHECK(!got->nullable() && ranks_of(*got) == include_before[m]);
    got = cudf::rank(with_null, methods[m], cudf::order::ASCENDING, cudf::null_policy::EXCLUDE, cudf::null_order::AFTER, false, stream);
    CHECK(got->nullable() && got->null_count() == 1 && ranks_of(*got) == exclude_after[m]);
  }
  // percentage: FLOAT64 for every method; DENSE divides by the number of distinct values
  auto const pct = cudf::rank(plain, rank_method::DENSE, cudf::order::ASCENDING, cudf::null_policy::INCLUDE, cudf::null_order::AFTER, true);
  CHECK(pct->type().id() == cudf::type_id::FLOAT64);
  CHECK((ranks_of(*pct) == std::vector<double>{3 / 5.0, 4 / 5.0, 5 / 5.0, 4 / 5.0, 1 / 5.0, 2 / 5.0}));
  // an empty column gives an empty column of the output type
  cudf::column_view const empty{cudf::data_type{cudf::type_id::INT64}, 0, nullptr, nullptr, 0};
  CHECK(cudf::rank(empty, rank_method::MIN, cudf::order::DESCENDING, cudf::null_policy::INCLUDE, cudf::null_order::AFTER, true)->type().id() ==
        cudf::type_id::FLOAT64);
  CHECK(cudf::rank(empty, rank_method::MAX, cudf::order::ASCENDING, cudf::null_policy::EXCLUDE, cudf::null_order::AFTER, false)->size() == 0);
  std::printf("rank_compat OK\n");
  return 0;
}
