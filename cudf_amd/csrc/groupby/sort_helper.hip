// SPDX-License-Identifier: Apache-2.0
// The reference's sort_groupby_helper (cpp/include/cudf/detail/groupby/sort_helper.hpp, cpp/src/groupby/sort/sort_helper.cu) on
// the radix sort of radix_sort.hpp:
//   keys   -> order-preserving words, one key column at a time from the last to the first (nulls after, as sort_helper.cu:93-111)
//   order  -> group boundaries (adjacent rows unequal) -> labels and offsets (sort_helper.cu:121-160)
//   values -> a second sort by (label, null, value) for the callers that read order statistics (sort_helper.cu:205-225)
#include "sort_helper.hpp"
#include "../common/profiler.hpp"

#include <cudf/utilities/error.hpp>

#include <algorithm>

namespace cudf::groupby::detail {
namespace {
using cudf::detail::col_is_valid;
using cudf::detail::device_column;
using cudf::detail::device_table;
using cudf::detail::gload;
using cudf::detail::gstore;
namespace prof = cudf::detail::prof;

__global__ void __launch_bounds__(256) k_boundaries(device_table keys, uint32_t const* order, int64_t nk, uint32_t* flags)
{
  int64_t const i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= nk) return;
  uint32_t f = 1;
  if (i > 0) f = cudf::detail::rows_equal(keys, gload(order + i - 1), keys, gload(order + i), true) ? 0u : 1u;
  gstore(flags + i, f);
}

// one key column without nulls: its sorted words are still in the sorter's front buffer
__global__ void __launch_bounds__(256) k_boundaries_of_words(uint64_t const* words, int64_t nk, uint32_t* flags)
{
  int64_t const i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i < nk) gstore(flags + i, (i == 0 || gload(words + i) != gload(words + i - 1)) ? 1u : 0u);
}

// labels[i] = (number of boundaries at or before i) - 1; offsets[label] = i at a boundary; first_row[label] = order[i]
__global__ void __launch_bounds__(256) k_labels(uint32_t const* flags, uint32_t const* before, uint32_t const* order, int64_t nk,
                                                int32_t* labels, int32_t* offsets, int32_t* first_row)
{
  int64_t const i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= nk) return;
  uint32_t const f = gload(flags + i);
  int32_t const g  = static_cast<int32_t>(gload(before + i) + f) - 1;
  gstore(labels + i, g);
  if (f) {
    gstore(offsets + g, static_cast<int32_t>(i));
    gstore(first_row + g, static_cast<int32_t>(gload(order + i)));
  }
}

// first_row[label] = the smallest row of the group: where the key order is not the input order inside a group (a values column sorted
// ahead of the keys), the group's key is still that of its first row in input order, as the reference's stable sort returns it.
// A group's positions are adjacent, so the lanes of a wave reduce per group and the last lane of each group's stretch adds its minimum.
__global__ void __launch_bounds__(256) k_first_rows_min(int32_t const* labels, uint32_t const* order, int64_t nk, int32_t* first_row)
{
  int64_t const i   = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  int const lane    = threadIdx.x & 63;
  bool const active = i < nk;
  int32_t const g   = active ? gload(labels + i) : -1;
  int32_t row       = active ? static_cast<int32_t>(gload(order + i)) : 0x7fffffff;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    int32_t const og = __shfl_up(g, o, 64);
    int32_t const orow = __shfl_up(row, o, 64);
    if (lane >= o && og == g && orow < row) row = orow;
  }
  int32_t const next = __shfl_down(g, 1, 64);
  if (active && (lane == 63 || next != g)) atomicMin(first_row + g, row);
}

__global__ void __launch_bounds__(256) k_valid_flags(device_column col, uint32_t const* order, int64_t nk, uint32_t* flags)
{
  int64_t const i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i < nk) gstore(flags + i, col_is_valid(col, gload(order + i)) ? 1u : 0u);
}

// vrow[i] = order[q[i]]: the row behind position i of the (label, null, value) order
__global__ void __launch_bounds__(256) k_compose(uint32_t const* order, uint32_t const* q, int64_t nk, uint32_t* vrow)
{
  int64_t const i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i < nk) gstore(vrow + i, gload(order + gload(q + i)));
}

__global__ void __launch_bounds__(256) k_count_runs(device_table keys, int64_t n, unsigned long long* out)
{
  unsigned long long mine = 0;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * 256)
    mine += (i == 0 || !cudf::detail::rows_equal(keys, i - 1, keys, i, true)) ? 1u : 0u;
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(out, mine);
}

// sorts by one column, nulls after its values: the value words, then (a column with nulls) the null flags
void sort_by_column(pair_sorter& sorter, device_column const& col, bool has_nulls)
{
  fill_args fa{};
  fa.col    = col;
  fa.source = WORD_VALUE;
  sorter.sort_by(fa);
  if (has_nulls) {
    fa.source = WORD_NULL_FLAG;
    sorter.sort_by(fa);
  }
}
}  // namespace

helper::helper(table_view const& k, hipStream_t stream)
  : keys{k}, dkeys{cudf::detail::make_device_table(k)}, keep{stream, get_current_device_resource_ref(), {}}, s{stream}
{
}

// inner_values: a values column whose order INSIDE the groups is wanted and nobody needs the rows of a group in their original
// order (no NTH_ELEMENT in the call): its words are sorted first, the key columns after them - one sort yields the groups AND that
// column's (key, null, value) order, instead of a key sort plus a second sort by (label, null, value): 11 instead of 14 passes and
// one gather instead of two at 100M rows on 1M groups.
void helper::build(bool exclude_null_keys, bool presorted, column_view const* inner_values)
{
  n = keys.num_rows();
  bool const keys_have_nulls = std::any_of(keys.begin(), keys.end(), [](auto const& c) { return c.has_nulls(); });
  // pre-sorted keys with nulls to drop are sorted like any others (reference sort_helper.cu:51-54)
  if (presorted && exclude_null_keys && keys_have_nulls) presorted = false;
  order = keep.alloc<uint32_t>(static_cast<std::size_t>(n));
  nk    = n;
  scratch tmp{s, get_current_device_resource_ref(), {}};
  auto* flags       = tmp.alloc<uint32_t>(static_cast<std::size_t>(n));
  bool flags_filled = false;
  if (presorted) {  // the rows as they lie: no sorter, no scratch for one
    iota(order, n, s);
    identity_order = true;
  } else {
    scratch sort_tmp{s, get_current_device_resource_ref(), {}};
    pair_sorter sorter{n, sort_tmp, s};
    if (inner_values != nullptr) {
      sort_by_column(sorter, cudf::detail::make_device_column(*inner_values), inner_values->has_nulls());
      _value_orders_in_key_order = key_of(*inner_values, false, false);
    }
    for (int c = dkeys.ncols - 1; c >= 0; --c) sort_by_column(sorter, dkeys.col[c], keys.column(c).has_nulls());
    if (exclude_null_keys && keys_have_nulls) {  // rows with a null in any key column to the back, then off the end
      fill_args fa{};
      fa.keys   = dkeys;
      fa.source = WORD_ANY_NULL;
      nk        = n - sorter.sort_by(fa);
    }
    CUDF_HIP_TRY(hipMemcpyAsync(order, sorter.finish(), static_cast<std::size_t>(n) * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    if (dkeys.ncols == 1 && !keys_have_nulls) {
      prof::scope p_{"sort_boundaries", s};
      hipLaunchKernelGGL(k_boundaries_of_words, dim3(blocks_of(n)), dim3(256), 0, s, sorter.words(), n, flags);
      flags_filled = true;
    }
    CUDF_HIP_TRY(hipGetLastError());
  }
  if (nk == 0) {
    G = 0;
    return;
  }
  labels       = keep.alloc<int32_t>(static_cast<std::size_t>(nk));
  auto* before = tmp.alloc<uint32_t>(static_cast<std::size_t>(nk) + 1);
  if (!flags_filled) {
    prof::scope p_{"sort_boundaries", s};
    hipLaunchKernelGGL(k_boundaries, dim3(blocks_of(nk)), dim3(256), 0, s, dkeys, order, nk, flags);
  }
  exclusive_scan(flags, before, nk, before + nk, tmp, s);
  uint32_t h_groups = 0;
  CUDF_HIP_TRY(hipMemcpyAsync(&h_groups, before + nk, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  CUDF_HIP_TRY(hipStreamSynchronize(s));
  G         = static_cast<int32_t>(h_groups);
  offsets   = keep.alloc<int32_t>(static_cast<std::size_t>(G) + 1);
  first_row = keep.alloc<int32_t>(static_cast<std::size_t>(G));
  hipLaunchKernelGGL(k_labels, dim3(blocks_of(nk)), dim3(256), 0, s, flags, before, order, nk, labels, offsets, first_row);
  fill_i32(offsets + G, 1, static_cast<int32_t>(nk), s);
  // equal keys of these classes may differ in their bits (-0.0 and 0.0, the NaNs, the non-zero bools): which row represents the group
  // shows in the unique keys
  bool const equal_keys_may_differ = std::any_of(dkeys.col, dkeys.col + dkeys.ncols, [](auto const& c) {
    return c.cls == cudf::detail::CLS_F32 || c.cls == cudf::detail::CLS_F64 || c.cls == cudf::detail::CLS_BOOL;
  });
  if (_value_orders_in_key_order.has_value() && equal_keys_may_differ) {
    prof::scope p_{"sort_first_rows", s};
    hipLaunchKernelGGL(k_first_rows_min, dim3(blocks_of(nk)), dim3(256), 0, s, labels, order, nk, first_row);
  }
  CUDF_HIP_TRY(hipGetLastError());
}

// rows in (label, null, value) order (reference sort_helper.cu:205-225 sorted_values): vrow[i] for i in the group's range
uint32_t* helper::value_order(column_view const& values, bool descending, bool nulls_first)
{
  auto const key = key_of(values, descending, nulls_first);
  if (_value_orders_in_key_order == key) return order;  // (build() sorted this column's words before the keys)
  if (auto it = _value_orders.find(key); it != _value_orders.end()) return it->second;
  auto* vrow = keep.alloc<uint32_t>(static_cast<std::size_t>(nk));
  {
    auto const col = cudf::detail::make_device_column(values);
    scratch tmp{s, get_current_device_resource_ref(), {}};
    pair_sorter sorter{nk, tmp, s};
    fill_args fa{};
    fa.col    = col;
    fa.order  = order;
    fa.source = WORD_VALUE;
    fa.invert = descending;
    sorter.sort_by(fa);
    fa.labels      = labels;
    fa.source      = WORD_LABEL_NULL;
    fa.nulls_first = nulls_first;
    sorter.sort_by(fa);
    hipLaunchKernelGGL(k_compose, dim3(blocks_of(nk)), dim3(256), 0, s, order, sorter.finish(), nk, vrow);
    CUDF_HIP_TRY(hipGetLastError());
  }
  _value_orders.emplace(key, vrow);
  return vrow;
}

// valid rows of `values` before each position of the key order (nk + 1 entries), and per group
uint32_t* helper::valid_before(column_view const& values, scratch& tmp, uint32_t** flags_out)
{
  auto* flags  = tmp.alloc<uint32_t>(static_cast<std::size_t>(nk));
  auto* before = tmp.alloc<uint32_t>(static_cast<std::size_t>(nk) + 1);
  hipLaunchKernelGGL(k_valid_flags, dim3(blocks_of(nk)), dim3(256), 0, s, cudf::detail::make_device_column(values), order, nk, flags);
  exclusive_scan(flags, before, nk, before + nk, tmp, s);
  if (flags_out) *flags_out = flags;
  return before;
}

// the number of runs of equal adjacent key rows (nulls equal nulls): one coalesced pass over the key columns
int64_t count_key_runs(table_view const& keys, stream_ref stream)
{
  int64_t const n = keys.num_rows();
  if (n == 0) return 0;
  hipStream_t const s = stream.value();
  rmm::device_buffer d{sizeof(unsigned long long), s, get_current_device_resource_ref()};
  CUDF_HIP_TRY(hipMemsetAsync(d.data(), 0, sizeof(unsigned long long), s));
  {
    prof::scope p_{"sort_boundaries", s};
    hipLaunchKernelGGL(k_count_runs, dim3(static_cast<unsigned>(std::min<int64_t>((n + 255) / 256, 256 * 32))), dim3(256), 0, s,
                       cudf::detail::make_device_table(keys), n, static_cast<unsigned long long*>(d.data()));
  }
  CUDF_HIP_TRY(hipGetLastError());
  unsigned long long h = 0;
  CUDF_HIP_TRY(hipMemcpyAsync(&h, d.data(), sizeof(h), hipMemcpyDeviceToHost, s));
  CUDF_HIP_TRY(hipStreamSynchronize(s));
  return static_cast<int64_t>(h);
}

}  // namespace cudf::groupby::detail
