// SPDX-License-Identifier: Apache-2.0
// Device helpers of the open-addressing set of distinct rows and of the small-range integer forms, shared by the kernels of
// cudf::filtered_join (filtered_join_kernels.hip), cudf::distinct (stream_compaction/distinct_kernels.hip) and
// cudf::distinct_hash_join (distinct_join_kernels.hip): key loads, the slot sequence and the ordered compaction of a mask. The slot
// layouts themselves are described in filtered_join_impl.hpp (set_args) and distinct_join_impl.hpp (table_args).
#pragma once
#include "../common/device_table.hpp"

#include <hip/hip_runtime.h>
#include <cstdint>

namespace cudf::detail::fjoin {

// element i of an integer column widened to 64 bits: sign-extended (SIGNED) or zero-extended
template <int W, bool SIGNED>
__device__ __forceinline__ uint64_t load_int(device_column const& c, int64_t i)
{
  int64_t const e = static_cast<int64_t>(c.offset) + i;
  if constexpr (W == 1) {
    uint8_t const v = gload(static_cast<uint8_t const*>(c.head) + e);
    return SIGNED ? static_cast<uint64_t>(static_cast<int64_t>(static_cast<int8_t>(v))) : v;
  } else if constexpr (W == 2) {
    uint16_t const v = gload(static_cast<uint16_t const*>(c.head) + e);
    return SIGNED ? static_cast<uint64_t>(static_cast<int64_t>(static_cast<int16_t>(v))) : v;
  } else if constexpr (W == 4) {
    uint32_t const v = gload(static_cast<uint32_t const*>(c.head) + e);
    return SIGNED ? static_cast<uint64_t>(static_cast<int64_t>(static_cast<int32_t>(v))) : v;
  } else {
    return gload(static_cast<uint64_t const*>(c.head) + e);
  }
}

// element i of a 4- or 8-byte column as raw bits, zero-extended
template <int W>
__device__ __forceinline__ uint64_t load_bits(device_column const& c, int64_t i)
{
  int64_t const e = static_cast<int64_t>(c.offset) + i;
  if constexpr (W == 4) return gload(static_cast<uint32_t const*>(c.head) + e);
  else return gload(static_cast<uint64_t const*>(c.head) + e);
}

// first slot of a row hash's probe sequence; 64-bit, so capacities beyond 2^32 slots are addressed
__device__ __forceinline__ uint64_t home_slot(uint32_t h, uint64_t capacity) { return __umul64hi(mix64(h), capacity); }
__device__ __forceinline__ uint64_t next_slot(uint64_t s, uint64_t capacity) { return s + 1 == capacity ? 0 : s + 1; }

// Ordered compaction of one wave's chunk, rows [wave * chunk, + chunk) of `nrows`: the wave streams the mask words of its chunk, 64
// at a time (one per lane), and calls emit(position, row) in the lane of every set bit, position = the chunk's offset (counts,
// scanned) plus the bits before the row: the words' exclusive prefix over the wave, then each word's bits below the lane (mbcnt).
// No atomics; positions ascend with the rows.
template <typename Emit>
__device__ __forceinline__ void compact_chunk(uint64_t const* mask, unsigned long long const* counts, int64_t wave, int64_t chunk,
                                              int64_t nrows, Emit const& emit)
{
  int const lane      = threadIdx.x & 63;
  int64_t const begin = wave * chunk;
  int64_t const end   = nrows < begin + chunk ? nrows : begin + chunk;
  if (begin >= end) return;
  uint64_t base       = gload(counts + wave);
  int64_t const w_end = (end + 63) >> 6;
  for (int64_t w0 = begin >> 6; w0 < w_end; w0 += 64) {
    uint64_t const word = w0 + lane < w_end ? gload(mask + w0 + lane) : 0;
    uint32_t const c    = __popcll(word);
    uint32_t inc        = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      uint32_t const t = __shfl_up(inc, o);
      if (lane >= o) inc += t;
    }
    uint32_t const exc   = inc - c;
    uint32_t const total = __shfl(inc, 63);
    int const nw         = static_cast<int>(w_end - w0 < 64 ? w_end - w0 : 64);
    for (int k = 0; k < nw; ++k) {
      uint64_t const wk = __shfl(word, k);
      if (wk == 0) continue;  // (uniform)
      uint32_t const at   = __shfl(exc, k);
      uint32_t const rank = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(wk >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(wk), 0u));
      if ((wk >> lane) & 1) emit(base + at + rank, (w0 + k) * 64 + lane);
    }
    base += total;
  }
}

}  // namespace cudf::detail::fjoin
