// SPDX-License-Identifier: Apache-2.0
// Device helpers of the open-addressing set of distinct rows and of the small-range integer forms, shared by the kernels of
// cudf::filtered_join (filtered_join_kernels.hip) and of cudf::distinct (stream_compaction/distinct_kernels.hip): key loads and the
// slot sequence. The slot layout itself is described in filtered_join_impl.hpp (set_args).
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

}  // namespace cudf::detail::fjoin
