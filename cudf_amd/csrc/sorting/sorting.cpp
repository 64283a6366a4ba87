// SPDX-License-Identifier: Apache-2.0
// Host side of cudf::sorted_order, sort, sort_by_key, their stable_ forms and is_sorted (include/cudf/sorting.hpp): the planner
// that packs the key columns into radix words (layout: sorting_impl.hpp), the sort of the words on the pair_sorter of
// groupby/radix_sort.hpp and the gather. Reference counterparts: cpp/src/sort/{sort_impl.cuh,sort.cu,stable_sort.cu,is_sorted.cu}.
// The model: DESIGN.md section 4, "Sorting".
#include "sorting_impl.hpp"
#include "../common/profiler.hpp"
#include "../groupby/radix_sort.hpp"

#include <cudf/copying.hpp>
#include <cudf/sorting.hpp>
#include <cudf/utilities/error.hpp>

namespace cudf {
namespace detail {
namespace sorting {
// The sizes are checked before the trivial cases, so a wrong length is an error for an empty table too.
void check_orders(table_view const& keys, std::vector<order> const& column_order, std::vector<null_order> const& null_precedence)
{
  CUDF_EXPECTS(column_order.empty() || static_cast<std::size_t>(keys.num_columns()) == column_order.size(),
               "Mismatch between number of columns and column order.");
  CUDF_EXPECTS(null_precedence.empty() || static_cast<std::size_t>(keys.num_columns()) == null_precedence.size(),
               "Mismatch between number of columns and null_precedence size.");
}

// The words of `keys`, least significant first (sorting_impl.hpp, "Layout"); a forced null bit keeps the column's mask nullptr.
packed_plan make_plan(table_view const& keys, std::vector<order> const& column_order, std::vector<null_order> const& null_precedence,
                      uint32_t force_null_bit)
{
  device_table const d = make_device_table(keys);  // (throws beyond MAX_COLS or for a column that is not fixed-width)
  packed_plan p{};
  int used = 0;  // bits taken in the current word
  int nf   = 0;
  auto const close_word = [&] {
    if (nf > p.begin[p.nwords]) p.begin[++p.nwords] = nf;
    used = 0;
  };
  for (int c = d.ncols - 1; c >= 0; --c) {
    bool const descending = !column_order.empty() && column_order[c] == order::DESCENDING;
    bool const before     = null_precedence.empty() || null_precedence[c] == null_order::BEFORE;
    int const vbits       = d.col[c].cls == CLS_BOOL ? 1 : 8 * d.col[c].width;
    int const nbit        = d.col[c].mask != nullptr || ((force_null_bit >> c) & 1u) ? 1 : 0;
    plan_field f{};
    f.col        = d.col[c];
    f.invert     = descending ? 1 : 0;
    f.null_first = before != descending ? 1 : 0;
    if (vbits + nbit > 64) {  // 64 value bits in a word of their own, the null bit lowest in the next
      close_word();
      f.shift = 0, f.vbits = 64, f.null_pos = -1;
      p.f[nf++] = f;
      close_word();
      f.vbits = 0, f.null_pos = 0;
      p.f[nf++] = f;
      used      = 1;
      continue;
    }
    if (used + vbits + nbit > 64) close_word();
    f.shift    = used;
    f.vbits    = vbits;
    f.null_pos = nbit ? used + vbits : -1;
    p.f[nf++]  = f;
    used += vbits + nbit;
  }
  close_word();
  return p;
}

namespace {

std::unique_ptr<column> order_of(table_view const& keys, std::vector<order> const& column_order,
                                 std::vector<null_order> const& null_precedence, stream_ref stream, rmm::device_async_resource_ref mr)
{
  check_orders(keys, column_order, null_precedence);
  packed_plan const p = make_plan(keys, column_order, null_precedence);
  int64_t const n     = keys.num_rows();
  if (n == 0) return make_empty_column(data_type{type_id::INT32});
  hipStream_t const s = stream.value();
  rmm::device_uvector<size_type> out(static_cast<std::size_t>(n), s, mr);
  if (p.nwords == 0) {  // no key columns: the identity order
    cudf::groupby::detail::iota(reinterpret_cast<uint32_t*>(out.data()), n, s);
  } else {
    cudf::groupby::detail::scratch tmp{s, get_current_device_resource_ref(), {}};
    cudf::groupby::detail::pair_sorter sorter(n, tmp, s);
    for (int w = 0; w < p.nwords; ++w) sorter.sort_by_packed(p.word(w));
    CUDF_HIP_TRY(hipMemcpyAsync(out.data(), sorter.finish(), static_cast<std::size_t>(n) * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
  }
  return std::make_unique<column>(std::move(out), rmm::device_buffer{}, 0);
}

std::unique_ptr<table> by_key(table_view const& values, table_view const& keys, std::vector<order> const& column_order,
                              std::vector<null_order> const& null_precedence, stream_ref stream, rmm::device_async_resource_ref mr)
{
  CUDF_EXPECTS(values.num_rows() == keys.num_rows(), "Mismatch in number of rows for values and keys");
  auto const idx = order_of(keys, column_order, null_precedence, stream, get_current_device_resource_ref());
  if (values.num_rows() == 0) return empty_like(values);
  return cudf::gather(values, idx->view(), out_of_bounds_policy::DONT_CHECK, stream, mr);
}

}  // namespace
}  // namespace sorting
}  // namespace detail

std::unique_ptr<column> sorted_order(table_view const& input, std::vector<order> const& column_order,
                                     std::vector<null_order> const& null_precedence, stream_ref stream, rmm::device_async_resource_ref mr)
{
  CUDF_FUNC_RANGE();
  return detail::sorting::order_of(input, column_order, null_precedence, stream, mr);
}

// The radix sort is stable, so the stable_ names run what the plain ones run.
std::unique_ptr<column> stable_sorted_order(table_view const& input, std::vector<order> const& column_order,
                                            std::vector<null_order> const& null_precedence, stream_ref stream,
                                            rmm::device_async_resource_ref mr)
{
  CUDF_FUNC_RANGE();
  return detail::sorting::order_of(input, column_order, null_precedence, stream, mr);
}

std::unique_ptr<table> sort(table_view const& input, std::vector<order> const& column_order, std::vector<null_order> const& null_precedence,
                            stream_ref stream, rmm::device_async_resource_ref mr)
{
  CUDF_FUNC_RANGE();
  return detail::sorting::by_key(input, input, column_order, null_precedence, stream, mr);
}

std::unique_ptr<table> stable_sort(table_view const& input, std::vector<order> const& column_order,
                                   std::vector<null_order> const& null_precedence, stream_ref stream, rmm::device_async_resource_ref mr)
{
  CUDF_FUNC_RANGE();
  return detail::sorting::by_key(input, input, column_order, null_precedence, stream, mr);
}

std::unique_ptr<table> sort_by_key(table_view const& values, table_view const& keys, std::vector<order> const& column_order,
                                   std::vector<null_order> const& null_precedence, stream_ref stream, rmm::device_async_resource_ref mr)
{
  CUDF_FUNC_RANGE();
  return detail::sorting::by_key(values, keys, column_order, null_precedence, stream, mr);
}

std::unique_ptr<table> stable_sort_by_key(table_view const& values, table_view const& keys, std::vector<order> const& column_order,
                                          std::vector<null_order> const& null_precedence, stream_ref stream,
                                          rmm::device_async_resource_ref mr)
{
  CUDF_FUNC_RANGE();
  return detail::sorting::by_key(values, keys, column_order, null_precedence, stream, mr);
}

bool is_sorted(table_view const& in, std::vector<order> const& column_order, std::vector<null_order> const& null_precedence,
               stream_ref stream)
{
  CUDF_FUNC_RANGE();
  detail::sorting::check_orders(in, column_order, null_precedence);
  auto const p = detail::sorting::make_plan(in, column_order, null_precedence);
  if (p.nwords == 0 || in.num_rows() <= 1) return true;
  hipStream_t const s = stream.value();
  // {flag, plan} go up in one copy; the one read-back brings the flag down
  struct {
    uint32_t flag[2];
    detail::sorting::packed_plan plan;
  } const h{{0, 0}, p};
  rmm::device_buffer d{sizeof(h), s, get_current_device_resource_ref()};
  CUDF_HIP_TRY(hipMemcpyAsync(d.data(), &h, sizeof(h), hipMemcpyHostToDevice, s));
  auto* flag = static_cast<uint32_t*>(d.data());
  detail::sorting::launch_is_sorted(reinterpret_cast<detail::sorting::packed_plan const*>(flag + 2), in.num_rows(), flag, s);
  uint32_t out = 0;
  CUDF_HIP_TRY(hipMemcpyAsync(&out, flag, sizeof(out), hipMemcpyDeviceToHost, s));
  CUDF_HIP_TRY(hipStreamSynchronize(s));  // (`h` stays alive until both copies are done)
  return out == 0;
}

}  // namespace cudf
