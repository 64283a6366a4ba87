// SPDX-License-Identifier: Apache-2.0
// Device side of cudf::sorted_order and cudf::is_sorted: the packed radix words of sorting_impl.hpp. row_word()
// (sorting_device.hpp) makes one word of one row from the plan's fields; k_fill_packed_words writes it for every position of the
// sorter's payload and k_is_sorted compares the words of adjacent rows. The sort itself is the pair_sorter of
// groupby/radix_sort.hpp.
#include "sorting_device.hpp"
#include "../common/profiler.hpp"

#include <cudf/utilities/error.hpp>

#include <algorithm>

namespace cudf::detail::sorting {
namespace {
namespace prof = cudf::detail::prof;

__global__ void __launch_bounds__(256) k_fill_packed_words(plan_word pw, uint32_t const* payload, uint64_t* words, uint64_t* or_and, int64_t n)
{
  uint64_t vor = 0, vand = ~0ull;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * 256) {
    uint32_t const row = payload ? gload(payload + i) : static_cast<uint32_t>(i);
    uint64_t const w   = row_word(pw.f, pw.nfields, row);
    gstore(words + i, w);
    vor |= w;
    vand &= w;
  }
  for (int o = 32; o > 0; o >>= 1) {
    vor |= __shfl_xor(vor, o, 64);
    vand &= __shfl_xor(vand, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicOr(reinterpret_cast<unsigned long long*>(or_and), static_cast<unsigned long long>(vor));
    atomicAnd(reinterpret_cast<unsigned long long*>(or_and + 1), static_cast<unsigned long long>(vand));
  }
}

constexpr int IS_ITEMS = 4;
constexpr int IS_TILE  = 256 * IS_ITEMS;  // adjacent pairs per workgroup and tile

// pair j = rows (j, j + 1). A workgroup walks tiles of pairs and leaves at the first tile it reaches after some pair was found
// out of order. The plan of all words is read from global memory: its fields are indexed by the word, and a kernel argument
// indexed that way would be copied to scratch.
__global__ void __launch_bounds__(256) k_is_sorted(packed_plan const* plan, int64_t n, uint32_t* flag)
{
  packed_plan const& p = *plan;
  int64_t const pairs = n - 1;
  int64_t const tiles = (pairs + IS_TILE - 1) / IS_TILE;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    if (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return;
    bool greater = false;
    for (int k = 0; k < IS_ITEMS; ++k) {
      int64_t const j = t * IS_TILE + k * 256 + threadIdx.x;
      if (j >= pairs) continue;
      for (int w = p.nwords - 1; w >= 0; --w) {  // from the most significant word down
        int const b      = p.begin[w];
        int const nf     = p.begin[w + 1] - b;
        uint64_t const x = row_word(p.f + b, nf, static_cast<uint32_t>(j));
        uint64_t const y = row_word(p.f + b, nf, static_cast<uint32_t>(j + 1));
        if (x != y) {
          greater |= x > y;
          break;
        }
      }
    }
    if (greater) __hip_atomic_store(flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
}  // namespace

void launch_fill_packed_words(plan_word const& w, uint32_t const* payload, uint64_t* words, uint64_t* or_and, int64_t n, hipStream_t s)
{
  if (n <= 0) return;
  auto const grid = static_cast<unsigned>(std::min<int64_t>((n + 255) / 256, 256 * 16));
  prof::scope p_{"sort_pack_words", s};
  hipLaunchKernelGGL(k_fill_packed_words, dim3(grid), dim3(256), 0, s, w, payload, words, or_and, n);
  CUDF_HIP_TRY(hipGetLastError());
}

void launch_is_sorted(packed_plan const* p, int64_t n, uint32_t* flag, hipStream_t s)
{
  if (n <= 1) return;
  int64_t const tiles = (n - 1 + IS_TILE - 1) / IS_TILE;
  prof::scope p_{"is_sorted", s};
  hipLaunchKernelGGL(k_is_sorted, dim3(static_cast<unsigned>(std::min<int64_t>(tiles, 256 * 8))), dim3(256), 0, s, p, n, flag);
  CUDF_HIP_TRY(hipGetLastError());
}

}  // namespace cudf::detail::sorting
