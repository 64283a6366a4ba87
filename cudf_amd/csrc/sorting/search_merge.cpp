// SPDX-License-Identifier: Apache-2.0
// Host side of cudf::lower_bound / upper_bound (include/cudf/search.hpp) and cudf::merge (include/cudf/merge.hpp): the joint plan of
// two key tables, the bound search, and the merge as two searches and a two-source gather. Reference counterparts:
// cpp/src/search/search_ordered.cu, cpp/src/merge/merge.cu. The model: DESIGN.md section 4, "Search and merge".
#include "sorting_impl.hpp"
#include "../common/profiler.hpp"

#include <cudf/merge.hpp>
#include <cudf/null_mask.hpp>
#include <cudf/search.hpp>
#include <cudf/utilities/error.hpp>

#include <algorithm>
#include <limits>
#include <utility>

namespace cudf {
namespace detail {
namespace sorting {
namespace {

bool same_types(table_view const& a, table_view const& b)
{
  if (a.num_columns() != b.num_columns()) return false;
  for (size_type c = 0; c < a.num_columns(); ++c)
    if (a.column(c).type() != b.column(c).type()) return false;
  return true;
}

// The joint plan: two tables compare word for word only if their words have one layout, and make_plan gives a column a null bit
// only if it has a mask. So a column gets the bit if EITHER side has nulls; the plans then differ in plan_field::col alone, and
// the side without a mask reads as all valid. In device memory: [0] reads `haystack`, [1] reads `needles`.
struct joint_plans {
  rmm::device_buffer plans;
  int nwords;
  [[nodiscard]] packed_plan const* data() const { return static_cast<packed_plan const*>(plans.data()); }
};

joint_plans make_joint_plans(table_view const& haystack, table_view const& needles, std::vector<order> const& column_order,
                             std::vector<null_order> const& null_precedence, hipStream_t s)
{
  uint32_t either = 0;
  for (size_type c = 0; c < haystack.num_columns() && c < 32; ++c)
    if (haystack.column(c).has_nulls() || needles.column(c).has_nulls()) either |= 1u << c;
  packed_plan const ph = make_plan(haystack, column_order, null_precedence, either);
  packed_plan const pn = make_plan(needles, column_order, null_precedence, either);
  joint_plans out{rmm::device_buffer{2 * sizeof(packed_plan), s, get_current_device_resource_ref()}, ph.nwords};
  launch_store_plans(ph, pn, static_cast<packed_plan*>(out.plans.data()), s);
  return out;
}

std::unique_ptr<column> bound(table_view const& haystack, table_view const& needles, std::vector<order> const& column_order,
                              std::vector<null_order> const& null_precedence, bool upper, stream_ref stream,
                              rmm::device_async_resource_ref mr)
{
  check_orders(haystack, column_order, null_precedence);  // (before every shortcut)
  CUDF_EXPECTS(haystack.num_columns() == needles.num_columns(), "Mismatched number of columns.", std::invalid_argument);
  CUDF_EXPECTS(same_types(haystack, needles), "Mismatched column types.", std::invalid_argument);
  hipStream_t const s = stream.value();
  int64_t const n     = needles.num_rows();
  // the plans are made before the shortcuts, so a key table beyond the device tables' limits throws for empty tables too
  packed_plan const probe = make_plan(haystack, column_order, null_precedence);
  (void)make_plan(needles, column_order, null_precedence);
  if (n == 0) return make_empty_column(data_type{type_id::INT32});
  rmm::device_uvector<size_type> out(static_cast<std::size_t>(n), s, mr);
  if (haystack.num_rows() == 0 || probe.nwords == 0) {
    // no haystack rows (a table without columns has none either): no row is less, and none is less or equal
    CUDF_HIP_TRY(hipMemsetAsync(out.data(), 0, static_cast<std::size_t>(n) * sizeof(size_type), s));
  } else {
    auto const plans = make_joint_plans(haystack, needles, column_order, null_precedence, s);
    launch_bound_search(plans.data(), plans.nwords, haystack.num_rows(), n, upper, out.data(), s);
  }
  return std::make_unique<column>(std::move(out), rmm::device_buffer{}, 0);
}

// Two non-empty tables a (left) and b (right), sorted on key_cols: row i of a lands at i + lower_bound(b, a[i]) and row j of b at
// j + upper_bound(a, b[j]). Each map is monotone inside its table (the stability promise), the two are disjoint, and together they
// are a permutation of [0, |a| + |b|) with a's rows before b's among equals.
std::unique_ptr<table> merge_two(table_view const& a, table_view const& b, std::vector<size_type> const& key_cols,
                                 std::vector<order> const& column_order, std::vector<null_order> const& null_precedence,
                                 stream_ref stream, rmm::device_async_resource_ref mr)
{
  hipStream_t const s = stream.value();
  auto const tmp      = get_current_device_resource_ref();
  int64_t const na = a.num_rows(), nb = b.num_rows(), n = na + nb;
  table_view const ka = a.select(key_cols), kb = b.select(key_cols);

  // If a or b is not sorted the two maps can collide and leave slots of `order` unwritten. Every slot therefore holds a valid
  // tagged index before the position kernels run: 0 is (side a, row 0), and a has a row 0 because merge() sends only non-empty
  // tables here. Whatever the inputs hold, the gather reads inside them.
  rmm::device_uvector<uint32_t> order(static_cast<std::size_t>(n), s, tmp);
  CUDF_HIP_TRY(hipMemsetAsync(order.data(), 0, static_cast<std::size_t>(n) * sizeof(uint32_t), s));
  {
    auto const plans = make_joint_plans(kb, ka, column_order, null_precedence, s);  // haystack b, needles a
    launch_merge_positions(plans.data(), plans.nwords, nb, na, false, 0u, order.data(), s);
  }
  {
    auto const plans = make_joint_plans(ka, kb, column_order, null_precedence, s);  // haystack a, needles b
    launch_merge_positions(plans.data(), plans.nwords, na, nb, true, MERGE_SIDE_B, order.data(), s);
  }

  std::vector<std::unique_ptr<column>> out_cols;
  for (auto const& col : a) {
    auto const w = size_of(col.type());
    CUDF_EXPECTS(w >= 1 && w <= 8, "merge: only fixed-width columns of at most 8 bytes.");
    out_cols.push_back(std::make_unique<column>(col.type(), static_cast<size_type>(n),
                                                rmm::device_buffer{static_cast<std::size_t>(n) * w, s, mr}, rmm::device_buffer{}, 0));
  }
  for (size_type first = 0; first < a.num_columns(); first += MERGE_COLS) {
    merge_cols g{};
    g.ncols = std::min<int32_t>(MERGE_COLS, a.num_columns() - first);
    for (int c = 0; c < g.ncols; ++c) {
      g.a[c]   = make_device_column(a.column(first + c));
      g.b[c]   = make_device_column(b.column(first + c));
      g.out[c] = out_cols[static_cast<std::size_t>(first + c)]->mutable_view().head();
    }
    launch_merge_gather(g, order.data(), n, s);
  }
  // validity: an output column is nullable if either input's column is; the null counts come down in one copy
  std::vector<size_type> nullable_cols;
  for (size_type c = 0; c < a.num_columns(); ++c)
    if (a.column(c).nullable() || b.column(c).nullable()) nullable_cols.push_back(c);
  if (!nullable_cols.empty()) {
    rmm::device_uvector<int32_t> counts(nullable_cols.size(), s, tmp);
    CUDF_HIP_TRY(hipMemsetAsync(counts.data(), 0, nullable_cols.size() * sizeof(int32_t), s));
    std::vector<rmm::device_buffer> masks;
    for (std::size_t k = 0; k < nullable_cols.size(); ++k) {
      size_type const c = nullable_cols[k];
      masks.push_back(create_null_mask(static_cast<size_type>(n), mask_state::UNINITIALIZED, stream, mr));
      launch_merge_mask(make_device_column(a.column(c)), make_device_column(b.column(c)), order.data(), n,
                        static_cast<bitmask_type*>(masks.back().data()), counts.data() + k, s);
    }
    std::vector<int32_t> h(nullable_cols.size());
    CUDF_HIP_TRY(hipMemcpyAsync(h.data(), counts.data(), h.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    CUDF_HIP_TRY(hipStreamSynchronize(s));
    for (std::size_t k = 0; k < nullable_cols.size(); ++k)
      out_cols[static_cast<std::size_t>(nullable_cols[k])]->set_null_mask(std::move(masks[k]), h[k]);
  }
  return std::make_unique<table>(std::move(out_cols));
}

}  // namespace
}  // namespace sorting
}  // namespace detail

std::unique_ptr<column> lower_bound(table_view const& haystack, table_view const& needles, std::vector<order> const& column_order,
                                    std::vector<null_order> const& null_precedence, stream_ref stream, rmm::device_async_resource_ref mr)
{
  CUDF_FUNC_RANGE();
  return detail::sorting::bound(haystack, needles, column_order, null_precedence, false, stream, mr);
}

std::unique_ptr<column> upper_bound(table_view const& haystack, table_view const& needles, std::vector<order> const& column_order,
                                    std::vector<null_order> const& null_precedence, stream_ref stream, rmm::device_async_resource_ref mr)
{
  CUDF_FUNC_RANGE();
  return detail::sorting::bound(haystack, needles, column_order, null_precedence, true, stream, mr);
}

std::unique_ptr<table> merge(std::vector<table_view> const& tables_to_merge, std::vector<size_type> const& key_cols,
                             std::vector<order> const& column_order, std::vector<null_order> const& null_precedence, stream_ref stream,
                             rmm::device_async_resource_ref mr)
{
  CUDF_FUNC_RANGE();
  if (tables_to_merge.empty()) return std::make_unique<table>(std::vector<std::unique_ptr<column>>{});
  // every check comes before the shortcuts (reference merge.cu:608-635)
  auto const& first = tables_to_merge.front();
  auto const ncols  = first.num_columns();
  for (auto const& t : tables_to_merge) CUDF_EXPECTS(t.num_columns() == ncols, "Mismatched number of columns");
  for (auto const& t : tables_to_merge) CUDF_EXPECTS(detail::sorting::same_types(first, t), "Mismatched column types");
  CUDF_EXPECTS(!key_cols.empty(), "Empty key_cols");
  CUDF_EXPECTS(key_cols.size() <= static_cast<std::size_t>(ncols), "Too many values in key_cols");
  CUDF_EXPECTS(key_cols.size() == column_order.size(), "Mismatched size between key_cols and column_order");
  CUDF_EXPECTS(null_precedence.empty() || null_precedence.size() == key_cols.size(),
               "Mismatched size between key_cols and null_precedence");
  std::size_t total = 0;
  for (auto const& t : tables_to_merge) total += static_cast<std::size_t>(t.num_rows());
  CUDF_EXPECTS(total <= static_cast<std::size_t>(std::numeric_limits<size_type>::max()), "Total number of merged rows exceeds row limit");
  std::vector<bool> seen(static_cast<std::size_t>(ncols), false);
  for (auto const k : key_cols) {
    CUDF_EXPECTS(k >= 0 && k < ncols, "A key column index is outside the table");
    CUDF_EXPECTS(!seen[static_cast<std::size_t>(k)], "A key column index repeats");
    seen[static_cast<std::size_t>(k)] = true;
  }
  // (throws for key columns beyond the device tables' limits, for empty tables too)
  (void)detail::sorting::make_plan(first.select(key_cols), column_order, null_precedence);
  for (auto const& col : first)
    CUDF_EXPECTS(size_of(col.type()) >= 1 && size_of(col.type()) <= 8, "merge: only fixed-width columns of at most 8 bytes.");

  // the non-empty tables; an intermediate result is owned by its entry
  std::vector<std::pair<table_view, std::unique_ptr<table>>> queue;
  for (auto const& t : tables_to_merge)
    if (t.num_rows() > 0) queue.emplace_back(t, nullptr);
  if (queue.size() == 1) return std::make_unique<table>(queue.front().first, stream, mr);
  if (queue.empty()) return empty_like(first);

  // merge the two tables with the fewest rows and put the result back, until one is left; only the last merge uses mr
  auto const take_smallest = [&] {
    auto it  = std::min_element(queue.begin(), queue.end(),
                                [](auto const& x, auto const& y) { return x.first.num_rows() < y.first.num_rows(); });
    auto out = std::move(*it);
    queue.erase(it);
    return out;
  };
  while (queue.size() > 1) {
    auto const left  = take_smallest();
    auto const right = take_smallest();
    auto merged      = detail::sorting::merge_two(left.first, right.first, key_cols, column_order, null_precedence, stream,
                                                  queue.empty() ? mr : get_current_device_resource_ref());
    // (the inputs of this round are freed in stream order, after the kernels that read them)
    auto const view = merged->view();
    queue.emplace_back(view, std::move(merged));
  }
  return std::move(queue.front().second);
}

}  // namespace cudf
