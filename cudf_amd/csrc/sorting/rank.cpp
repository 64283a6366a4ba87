// SPDX-License-Identifier: Apache-2.0
// Host side of cudf::rank (include/cudf/sorting.hpp): the one-column plan of sorting_impl.hpp, its stable radix sort on the
// pair_sorter of groupby/radix_sort.hpp, and one streaming pass over the sorted words (rank_kernels.hip). Reference counterpart:
// cpp/src/sort/rank.cu:253-353, which runs transform, inclusive_scan, reduce_by_key, scatter and transform over the sorted order
// (rank.cu:58-150). The model: DESIGN.md section 4, "Ranking".
#include "sorting_impl.hpp"
#include "../common/profiler.hpp"
#include "../groupby/radix_sort.hpp"

#include <cudf/copying.hpp>
#include <cudf/null_mask.hpp>
#include <cudf/sorting.hpp>
#include <cudf/utilities/error.hpp>

#include <tuple>

namespace cudf {
namespace detail {
namespace sorting {
namespace {

// The sorted words and the order of `p`'s column, then the kernels of `method`. `count`: the rows that take part (rank.cu:339-340).
template <typename OUT>
void rank_into(packed_plan const& p, int64_t n, rank_method method, bool percentage, int64_t count, OUT* out, hipStream_t s)
{
  cudf::groupby::detail::scratch tmp{s, get_current_device_resource_ref(), {}};
  cudf::groupby::detail::pair_sorter sorter(n, tmp, s);
  for (int w = 0; w < p.nwords; ++w) sorter.sort_by_packed(p.word(w));
  uint32_t const* order = sorter.finish();
  auto const divisor    = static_cast<double>(count);
  if (method == rank_method::FIRST) return launch_rank_first(order, out, n, percentage, divisor, s);

  // sorter.words() are those of the last word sorted by. A nullable 8-byte column has two: the null-bit word is in front and the
  // value word is made again, in the final order.
  rank_words words{sorter.words(), nullptr};
  if (p.nwords == 2) {
    auto* value_words = tmp.alloc<uint64_t>(static_cast<std::size_t>(n));
    launch_fill_packed_words(p.word(0), order, value_words, tmp.alloc<uint64_t>(2), n, s);  // (its OR / AND is not read)
    words = {value_words, sorter.words()};
  }
  if (method != rank_method::DENSE) return launch_rank_ties(words, order, out, n, method, percentage, divisor, s);

  int64_t const tiles = (n + RANK_TILE - 1) / RANK_TILE;
  auto* counts        = tmp.alloc<uint32_t>(static_cast<std::size_t>(tiles) + 1);
  uint32_t* q_heads   = counts + tiles;
  launch_rank_dense_count(words, n, counts, count - 1, q_heads, s);
  cudf::groupby::detail::exclusive_scan(counts, counts, tiles, nullptr, tmp, s);
  launch_rank_dense_apply(words, order, out, n, counts, percentage, count - 1, q_heads, s);
}

}  // namespace
}  // namespace sorting
}  // namespace detail

std::unique_ptr<column> rank(column_view const& input, rank_method method, order column_order, null_policy null_handling,
                             null_order null_precedence, bool percentage, stream_ref stream, rmm::device_async_resource_ref mr)
{
  CUDF_FUNC_RANGE();
  namespace ds = detail::sorting;
  CUDF_EXPECTS(method == rank_method::FIRST || method == rank_method::AVERAGE || method == rank_method::MIN ||
                 method == rank_method::MAX || method == rank_method::DENSE,
               "Unexpected rank_method for rank()");  // rank.cu:313
  table_view const keys{std::vector<column_view>{input}};
  ds::check_orders(keys, {column_order}, {null_precedence});
  // (throws for a column that is not fixed-width, for an empty one too)
  auto const p = ds::make_plan(keys, {column_order}, {null_precedence});
  // rank.cu:262-264
  bool const as_double = percentage || method == rank_method::AVERAGE;
  data_type const type{as_double ? type_id::FLOAT64 : type_id::INT32};
  int64_t const n = input.size();
  if (n == 0) return make_empty_column(type);
  hipStream_t const s = stream.value();

  // rank.cu:265-276: EXCLUDE keeps the input's validity (na_option = keep); bitmask_and of the one column is its copy from bit 0
  rmm::device_buffer mask{};
  size_type nulls = 0;
  if (null_handling == null_policy::EXCLUDE && input.nullable()) std::tie(mask, nulls) = bitmask_and(keys, stream, mr);
  int64_t const count = n - nulls;  // rank.cu:339-340

  rmm::device_buffer data{static_cast<std::size_t>(n) * (as_double ? sizeof(double) : sizeof(int32_t)), s, mr};
  if (as_double) {
    ds::rank_into(p, n, method, percentage, count, static_cast<double*>(data.data()), s);
  } else {
    ds::rank_into(p, n, method, false, count, static_cast<int32_t*>(data.data()), s);
  }
  return std::make_unique<column>(type, static_cast<size_type>(n), std::move(data), std::move(mask), nulls);
}

}  // namespace cudf
