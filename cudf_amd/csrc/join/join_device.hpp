// SPDX-License-Identifier: Apache-2.0
// Device code the join's kernel units share (open_table_kernels.hip, dense_table_kernels.hip, pair_kernels.hip, radix_kernels.hip,
// dense_part_kernels.hip): the argument upload, the wave-level append to a workgroup's output range, the tail of a count pass and
// the workgroup scan step.
#pragma once
#include "engine.hpp"

#include <cudf/join/join.hpp>

#include <algorithm>

namespace cudf::detail::join {
namespace {

// one thread copies a launcher's argument struct to device memory, in stream order before the kernels that read it
template <typename T>
__global__ void k_store_args(T v, T* dst) { *dst = v; }

inline unsigned grid_for(int64_t n)
{
  int64_t const blocks = (n + 255) / 256;
  return static_cast<unsigned>(std::max<int64_t>(1, std::min<int64_t>(blocks, 256 * 16)));
}

// Wave-level append: the lanes with `want` take consecutive positions from a workgroup-local LDS cursor (64-lane ballot + popcount
// prefix, one LDS atomic per wave and call). Every lane of the wave calls it; the position returned means something to the lanes
// with `want` only.
__device__ __forceinline__ unsigned long long wave_reserve(bool want, unsigned long long* lds_cursor, int lane)
{
  unsigned long long const ballot = __ballot(want);
  if (ballot == 0) return 0;
  int const lead = __ffsll(static_cast<long long>(ballot)) - 1;
  int const rank = __popcll(ballot & ((1ull << lane) - 1));
  unsigned long long base = 0;
  if (lane == lead) base = atomicAdd(lds_cursor, static_cast<unsigned long long>(__popcll(ballot)));
  return __shfl(base, lead) + rank;
}
// a retrieve pass's pair {prow, brow} of the lanes with `want`: appended at the workgroup's cursor; a full join (kind 2) notes the build row
__device__ __forceinline__ void wave_emit_pair(join_args const& a, int kind, bool want, size_type prow, size_type brow, unsigned long long* lds_cursor,
                                               int lane)
{
  uint64_t const o = wave_reserve(want, lds_cursor, lane);
  if (!want) return;
  if (o < a.out_capacity) {
    gstore(a.out_probe + o, prow);
    gstore(a.out_build + o, brow);
  }
  if (kind == 2 && brow != JoinNoMatch) gstore(a.build_matched + brow, uint8_t{1});
}

// One probe row's results of a count pass: its match cache word, its optional row count, and the pairs it will emit.
__device__ __forceinline__ unsigned int count_row(join_args const& a, int kind, int64_t j, uint32_t cache, unsigned int cnt)
{
  gstore(a.match_cache + j, cache);
  unsigned int const emitted = (cnt == 0 && kind != 0) ? 1u : cnt;  // left/full joins emit lonely probe rows once
  if (a.row_counts != nullptr) gstore(a.row_counts + j, static_cast<size_type>(emitted));
  return emitted;
}
// end of a count pass: the lanes' pair counts summed into *lds_total (zeroed, a barrier ago) and stored as the workgroup's count
__device__ __forceinline__ void count_block_total(unsigned long long local_count, unsigned long long* lds_total, unsigned long long* block_counts)
{
  for (int o = 32; o > 0; o >>= 1) local_count += __shfl_down(local_count, o);
  if ((threadIdx.x & 63) == 0 && local_count) atomicAdd(lds_total, local_count);
  __syncthreads();
  if (threadIdx.x == 0) block_counts[blockIdx.x] = *lds_total;
}

// Exclusive prefix of x over a workgroup of 1024 threads: shuffle ladder inside each wave, the 16 wave totals through LDS
// (wave_tot: 16 words). Holds one barrier; a caller that loops puts another one before the next call.
template <typename T>
__device__ __forceinline__ T block_exclusive_scan(T x, T* wave_tot)
{
  int const lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T inc = x;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    T const t = __shfl_up(inc, o);
    if (lane >= o) inc += t;
  }
  if (lane == 63) wave_tot[wave] = inc;
  __syncthreads();
  T off = inc - x;
  for (int w = 0; w < wave; ++w) off += wave_tot[w];
  return off;
}

}  // namespace
}  // namespace cudf::detail::join
