// SPDX-License-Identifier: Apache-2.0
// Device side of cudf::lower_bound / upper_bound / merge (include/cudf/search.hpp, merge.hpp): a binary search of every needle row
// in a sorted haystack, the rows compared as the packed words of sorting_impl.hpp compare (row_word of sorting_device.hpp, from the
// most significant word down, as k_is_sorted does), and the two-source gather that materialises a merge. The two tables are read
// through two plans of one layout (search_merge.cpp, "joint plan"). The model: DESIGN.md section 4, "Search and merge".
#include "sorting_device.hpp"
#include "../common/profiler.hpp"

#include <cudf/utilities/error.hpp>

namespace cudf::detail::sorting {
namespace {
namespace prof = cudf::detail::prof;

__global__ void k_store_plans(packed_plan hay, packed_plan* dst) { *dst = hay; }

// The number of haystack rows less than (upper: less than or equal to) needle row i. plans[0] reads the haystack, plans[1] the
// needles; both are read from global memory, because their fields are indexed by the word and a kernel argument indexed that way
// would be copied to scratch (k_is_sorted). NW > 0: the layout has NW words and the needle's are made once, before the loop, and
// kept in registers (the loops over them are unrolled, so the array is never indexed by a variable). NW == 0: any number of words,
// the needle's word is made again at each comparison that reaches it - no array, so no scratch either.
// Every probe reads row mid with lo <= mid < hi <= haystack_rows, whatever the haystack holds: an unsorted haystack gives some
// position in [0, haystack_rows] and no read outside the columns.
template <int NW>
__device__ __forceinline__ uint32_t bound_of(packed_plan const* plans, int nwords, uint32_t haystack_rows, uint32_t i, bool upper)
{
  packed_plan const& ph = plans[0];
  packed_plan const& pn = plans[1];
  uint64_t nw[NW > 0 ? NW : 1];
  if constexpr (NW > 0) {
#pragma unroll
    for (int k = 0; k < NW; ++k) {  // k = 0: the most significant word
      int const b = pn.begin[NW - 1 - k];
      nw[k]       = row_word(pn.f + b, pn.begin[NW - k] - b, i);
    }
  }
  uint32_t lo = 0, hi = haystack_rows;
  while (lo < hi) {
    uint32_t const mid = lo + ((hi - lo) >> 1);
    bool right         = upper;  // the rows tie: an upper bound lies to the right of them, a lower bound does not
    if constexpr (NW > 0) {
#pragma unroll
      for (int k = 0; k < NW; ++k) {
        int const b      = ph.begin[NW - 1 - k];
        uint64_t const x = row_word(ph.f + b, ph.begin[NW - k] - b, mid);
        if (x != nw[k]) {
          right = x < nw[k];
          break;
        }
      }
    } else {
      for (int w = nwords - 1; w >= 0; --w) {
        int const b      = ph.begin[w];
        int const nf     = ph.begin[w + 1] - b;
        uint64_t const x = row_word(ph.f + b, nf, mid);
        uint64_t const y = row_word(pn.f + b, nf, i);
        if (x != y) {
          right = x < y;
          break;
        }
      }
    }
    if (right) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// one thread per needle row; adjacent lanes take adjacent needles, so sorted needles walk neighbouring haystack rows
template <int NW>
__global__ void __launch_bounds__(256) k_bound_search(packed_plan const* plans, int nwords, uint32_t haystack_rows, int64_t n, int upper,
                                                      int32_t* out)
{
  int64_t const i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  gstore(out + i, static_cast<int32_t>(bound_of<NW>(plans, nwords, haystack_rows, static_cast<uint32_t>(i), upper != 0)));
}

// the same search; row i of this side lands at i + bound (bound <= haystack_rows, so the position is below haystack_rows + n)
template <int NW>
__global__ void __launch_bounds__(256) k_merge_positions(packed_plan const* plans, int nwords, uint32_t haystack_rows, int64_t n,
                                                         int upper, uint32_t tag, uint32_t* order)
{
  int64_t const i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  uint32_t const pos = static_cast<uint32_t>(i) + bound_of<NW>(plans, nwords, haystack_rows, static_cast<uint32_t>(i), upper != 0);
  gstore(order + pos, tag | static_cast<uint32_t>(i));
}

// The two-source sibling of k_gather_multi (partition/hash_partition.hip): R rows per thread, the order entries first, then every
// column's R random loads back to back, then the stores. Column c of the two sides has one type, so only head and offset differ.
__global__ void __launch_bounds__(256) k_merge_gather(merge_cols g, uint32_t const* order, int64_t n)
{
  constexpr int R    = 4;
  int64_t const base = static_cast<int64_t>(blockIdx.x) * 256 * R + threadIdx.x;
  uint32_t t[R];
#pragma unroll
  for (int k = 0; k < R; ++k) {
    int64_t const i = base + static_cast<int64_t>(k) * 256;
    t[k]            = i < n ? gload(order + i) : 0;  // (past the end: side A, row 0 - loaded, never stored)
  }
#pragma unroll
  for (int c = 0; c < MERGE_COLS; ++c) {
    if (c >= g.ncols) break;
    device_column const a = g.a[c], b = g.b[c];
    uint64_t v[R];
#pragma unroll
    for (int k = 0; k < R; ++k) {
      bool const side_b = (t[k] & MERGE_SIDE_B) != 0;
      device_column src = a;
      src.head          = side_b ? b.head : a.head;
      src.offset        = side_b ? b.offset : a.offset;
      v[k]              = col_load_bits(src, t[k] & ~MERGE_SIDE_B);
    }
#pragma unroll
    for (int k = 0; k < R; ++k) {
      int64_t const i = base + static_cast<int64_t>(k) * 256;
      if (i >= n) continue;
      switch (a.width) {
        case 1: gstore(static_cast<uint8_t*>(g.out[c]) + i, static_cast<uint8_t>(v[k])); break;
        case 2: gstore(static_cast<uint16_t*>(g.out[c]) + i, static_cast<uint16_t>(v[k])); break;
        case 4: gstore(static_cast<uint32_t*>(g.out[c]) + i, static_cast<uint32_t>(v[k])); break;
        default: gstore(static_cast<uint64_t*>(g.out[c]) + i, v[k]);
      }
    }
  }
}

// out_mask bit i = validity of the element order[i] names, built by wave ballot as k_gather_mask builds it; a side without a mask
// is all valid. Counts the nulls.
__global__ void __launch_bounds__(256) k_merge_mask(device_column a, device_column b, uint32_t const* order, int64_t n,
                                                    bitmask_type* out_mask, int32_t* null_count)
{
  int64_t const i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  bool valid      = false;
  if (i < n) {
    uint32_t const t = gload(order + i);
    valid            = (t & MERGE_SIDE_B) ? col_is_valid(b, t & ~MERGE_SIDE_B) : col_is_valid(a, t);
  }
  unsigned long long const ballot = __ballot(valid);
  unsigned long long const live   = __ballot(i < n);
  int const lane                  = threadIdx.x & 63;
  if (i < n && (lane & 31) == 0) gstore(out_mask + (i >> 5), static_cast<uint32_t>(ballot >> (lane & 32)));
  int const nulls = __popcll(live & ~ballot);
  if (lane == 0 && nulls) atomicAdd(null_count, nulls);
}

unsigned blocks_of(int64_t n, int per_block) { return static_cast<unsigned>((n + per_block - 1) / per_block); }
}  // namespace

void launch_store_plans(packed_plan const& haystack, packed_plan const& needles, packed_plan* plans, hipStream_t s)
{
  // (each plan goes up as a kernel argument and is stored by the kernel: stream-ordered, and nothing on the host has to outlive it)
  hipLaunchKernelGGL(k_store_plans, dim3(1), dim3(1), 0, s, haystack, plans);
  hipLaunchKernelGGL(k_store_plans, dim3(1), dim3(1), 0, s, needles, plans + 1);
  CUDF_HIP_TRY(hipGetLastError());
}

void launch_bound_search(packed_plan const* plans, int nwords, int64_t haystack_rows, int64_t needle_rows, bool upper, int32_t* out,
                         hipStream_t s)
{
  if (needle_rows <= 0) return;
  auto const h = static_cast<uint32_t>(haystack_rows);
  dim3 const grid(blocks_of(needle_rows, 256));
  prof::scope p_{"bound_search", s};
  switch (nwords) {
    case 1: hipLaunchKernelGGL(k_bound_search<1>, grid, dim3(256), 0, s, plans, nwords, h, needle_rows, upper ? 1 : 0, out); break;
    case 2: hipLaunchKernelGGL(k_bound_search<2>, grid, dim3(256), 0, s, plans, nwords, h, needle_rows, upper ? 1 : 0, out); break;
    case 3: hipLaunchKernelGGL(k_bound_search<3>, grid, dim3(256), 0, s, plans, nwords, h, needle_rows, upper ? 1 : 0, out); break;
    case 4: hipLaunchKernelGGL(k_bound_search<4>, grid, dim3(256), 0, s, plans, nwords, h, needle_rows, upper ? 1 : 0, out); break;
    default: hipLaunchKernelGGL(k_bound_search<0>, grid, dim3(256), 0, s, plans, nwords, h, needle_rows, upper ? 1 : 0, out);
  }
  CUDF_HIP_TRY(hipGetLastError());
}

void launch_merge_positions(packed_plan const* plans, int nwords, int64_t haystack_rows, int64_t needle_rows, bool upper, uint32_t tag,
                            uint32_t* order, hipStream_t s)
{
  if (needle_rows <= 0) return;
  auto const h = static_cast<uint32_t>(haystack_rows);
  dim3 const grid(blocks_of(needle_rows, 256));
  prof::scope p_{"merge_positions", s};
  switch (nwords) {
    case 1: hipLaunchKernelGGL(k_merge_positions<1>, grid, dim3(256), 0, s, plans, nwords, h, needle_rows, upper ? 1 : 0, tag, order); break;
    case 2: hipLaunchKernelGGL(k_merge_positions<2>, grid, dim3(256), 0, s, plans, nwords, h, needle_rows, upper ? 1 : 0, tag, order); break;
    case 3: hipLaunchKernelGGL(k_merge_positions<3>, grid, dim3(256), 0, s, plans, nwords, h, needle_rows, upper ? 1 : 0, tag, order); break;
    case 4: hipLaunchKernelGGL(k_merge_positions<4>, grid, dim3(256), 0, s, plans, nwords, h, needle_rows, upper ? 1 : 0, tag, order); break;
    default: hipLaunchKernelGGL(k_merge_positions<0>, grid, dim3(256), 0, s, plans, nwords, h, needle_rows, upper ? 1 : 0, tag, order);
  }
  CUDF_HIP_TRY(hipGetLastError());
}

void launch_merge_gather(merge_cols const& g, uint32_t const* order, int64_t n, hipStream_t s)
{
  if (n <= 0) return;
  prof::scope p_{"merge_gather", s};
  hipLaunchKernelGGL(k_merge_gather, dim3(blocks_of(n, 1024)), dim3(256), 0, s, g, order, n);
  CUDF_HIP_TRY(hipGetLastError());
}

void launch_merge_mask(device_column const& a, device_column const& b, uint32_t const* order, int64_t n, bitmask_type* out_mask,
                       int32_t* null_count, hipStream_t s)
{
  if (n <= 0) return;
  prof::scope p_{"merge_mask", s};
  hipLaunchKernelGGL(k_merge_mask, dim3(blocks_of(n, 256)), dim3(256), 0, s, a, b, order, n, out_mask, null_count);
  CUDF_HIP_TRY(hipGetLastError());
}

}  // namespace cudf::detail::sorting
