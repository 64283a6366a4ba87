// SPDX-License-Identifier: Apache-2.0
// Device side of cudf::rank (include/cudf/sorting.hpp; reference cpp/src/sort/rank.cu:58-353): the rank of every sorted position
// from the sorted packed words of sorting_impl.hpp, scattered through the order. Two rows tie exactly when their words are equal,
// so position i starts a run ("is a head") when i == 0 or its words differ from those of position i - 1.
//
// A workgroup walks tiles of RANK_TILE sorted positions and never waits for another workgroup: the heads of a tile are one
// ballot per 64 positions (one load to the left of the tile for its first position), the run that enters the tile from the left
// finds its true first position with a lower bound over the words before the tile, the run that leaves it to the right its true
// end with an upper bound over the words after it (one load to the right of the tile tells whether one does), and wave 0 does
// those at most two searches. Inside the tile the first and the last position of the run of every position come from the head
// bits: the highest head at or below the position and the lowest head above it, looked up in the position's own 64-bit ballot
// or, if that has none, in a forward max-scan / backward min-scan over the ballots that wave 0 makes with shuffles.
//
// FIRST reads no words (k_rank_first). MIN, MAX and AVERAGE are k_rank_ties. DENSE counts the heads of every tile
// (k_rank_dense_count), the host scans the counts (exclusive_scan of groupby/radix_sort.hpp) and k_rank_dense_apply adds the
// heads inside the tile. The percentage divisor of DENSE, the dense rank of sorted position count - 1 (rank.cu:341-349), is
// tile_base[that position's tile] + the heads of that tile up to the position; the count kernel leaves the second term in device
// memory and the apply kernel adds the two.
#include "sorting_device.hpp"
#include "../common/profiler.hpp"

#include <cudf/utilities/error.hpp>

#include <algorithm>
#include <type_traits>

namespace cudf::detail::sorting {
namespace {
namespace prof = cudf::detail::prof;

constexpr int RANK_ITEMS = RANK_TILE / 256;  // per thread and tile: position base + k * 256 + thread
constexpr int RANK_WORDS = RANK_TILE / 64;   // ballots per tile: ballot k * 4 + wave holds positions k * 256 + wave * 64 + lane
static_assert(RANK_TILE % 256 == 0);
static_assert(RANK_WORDS <= 64, "wave 0 scans the ballots of a tile with one lane each");

// the words of one sorted position, least significant first (NW == 2: the value word, then the null-bit word)
template <int NW>
struct rank_key {
  uint64_t w[NW];
};

template <int NW>
__device__ __forceinline__ rank_key<NW> load_key(uint64_t const* w0, uint64_t const* w1, int64_t i)
{
  rank_key<NW> k;
  k.w[0] = gload(w0 + i);
  if constexpr (NW == 2) k.w[1] = gload(w1 + i);
  return k;
}

template <int NW>
__device__ __forceinline__ bool key_equal(rank_key<NW> const& a, rank_key<NW> const& b)
{
  if constexpr (NW == 2) return a.w[0] == b.w[0] && a.w[1] == b.w[1];
  return a.w[0] == b.w[0];
}

// the order the words were sorted in: the last word is the most significant
template <int NW>
__device__ __forceinline__ bool key_less(rank_key<NW> const& a, rank_key<NW> const& b)
{
  if constexpr (NW == 2) return a.w[1] < b.w[1] || (a.w[1] == b.w[1] && a.w[0] < b.w[0]);
  return a.w[0] < b.w[0];
}

template <int NW>
__device__ __forceinline__ rank_key<NW> shuffle_up_one(rank_key<NW> const& k)
{
  rank_key<NW> out;
#pragma unroll
  for (int i = 0; i < NW; ++i) out.w[i] = __shfl_up(k.w[i], 1, 64);
  return out;
}

// One wave, every lane with the same arguments: the first position in [lo, hi) whose words are not less than `key` (UPPER:
// greater than `key`), hi if there is none. A 64-ary search: every step probes the last position of 64 equal chunks and keeps
// the one chunk that can hold the answer, so 2^31 positions take six steps. Every probe is inside [lo, hi).
template <int NW, bool UPPER>
__device__ int64_t wave_bound(uint64_t const* w0, uint64_t const* w1, rank_key<NW> const& key, int64_t lo, int64_t hi, int lane)
{
  while (lo < hi) {
    int64_t const step = (hi - lo + 63) / 64;
    int64_t const pos  = lo + (lane + 1) * step - 1;
    bool before        = false;  // the answer is beyond pos
    if (pos < hi) {
      rank_key<NW> const x = load_key<NW>(w0, w1, pos);
      before               = UPPER ? !key_less<NW>(key, x) : key_less<NW>(x, key);
    }
    int const c = __popcll(__ballot(before));  // (sorted words: the lanes below c)
    hi          = std::min<int64_t>(lo + (c + 1) * step - 1, hi);
    lo          = std::min<int64_t>(lo + c * step, hi);
  }
  return lo;
}

// the head ballots of the tile at `base` into heads[RANK_WORDS] (callers synchronise); n > base
template <int NW>
__device__ __forceinline__ void tile_heads(uint64_t const* w0, uint64_t const* w1, int64_t base, int64_t n, uint64_t* heads)
{
  int const lane = threadIdx.x & 63;
  int const wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < RANK_ITEMS; ++k) {
    int64_t const p = base + k * 256 + threadIdx.x;
    // (positions leave a wave from its top lane: the lane below a live lane is live, and lane 0 reads its neighbour from memory)
    rank_key<NW> const cur = load_key<NW>(w0, w1, std::min<int64_t>(p, n - 1));
    rank_key<NW> prev      = shuffle_up_one<NW>(cur);
    if (lane == 0 && p > 0 && p < n) prev = load_key<NW>(w0, w1, p - 1);
    bool const head  = p < n && (p == 0 || !key_equal<NW>(cur, prev));
    uint64_t const b = __ballot(head);
    if (lane == 0) heads[k * 4 + wave] = b;
  }
}

// OUT(rank) or, for a percentage, rank / divisor in double (rank.cu:336-351)
template <typename OUT>
__device__ __forceinline__ OUT finish_rank(OUT r, bool percentage, double divisor)
{
  if constexpr (std::is_same_v<OUT, double>) {
    if (percentage) return r / divisor;
  }
  return r;
}

// rank.cu:152-163: the stable order has no ties
template <typename OUT>
__global__ void __launch_bounds__(256) k_rank_first(uint32_t const* order, OUT* out, int64_t n, bool percentage, double divisor)
{
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * 256)
    gstore(out + gload(order + i), finish_rank<OUT>(static_cast<OUT>(i + 1), percentage, divisor));
}

// method: rank_method MIN, MAX or AVERAGE (rank.cu:179-249). out[order[i]] = first position of i's run + 1, last position + 1,
// or first + 1 + (length - 1) / 2.0
template <typename OUT, int NW>
__global__ void __launch_bounds__(256) k_rank_ties(uint64_t const* w0, uint64_t const* w1, uint32_t const* order, OUT* out, int64_t n,
                                                   int32_t method, bool percentage, double divisor)
{
  __shared__ uint64_t heads[RANK_WORDS];
  __shared__ int32_t last_before[RANK_WORDS];  // the highest head of the ballots before this one, in tile positions; -1: none
  __shared__ int32_t first_after[RANK_WORDS];  // the lowest head of the ballots after this one; RANK_TILE: none
  __shared__ int64_t edge[2];                  // first position of the run at the tile's first position; end of the run at its last
  int const lane      = threadIdx.x & 63;
  int const wave      = threadIdx.x >> 6;
  int64_t const tiles = (n + RANK_TILE - 1) / RANK_TILE;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    int64_t const base = t * RANK_TILE;
    int64_t const last = std::min<int64_t>(base + RANK_TILE, n) - 1;  // the tile's last position
    uint32_t row[RANK_ITEMS];
#pragma unroll
    for (int k = 0; k < RANK_ITEMS; ++k) {
      int64_t const p = base + k * 256 + threadIdx.x;
      row[k]          = p < n ? gload(order + p) : 0u;
    }
    tile_heads<NW>(w0, w1, base, n, heads);
    __syncthreads();
    if (wave == 0) {
      uint64_t const hw = lane < RANK_WORDS ? heads[lane] : 0;
      int32_t hi_head   = hw ? 64 * lane + 63 - __builtin_clzll(hw) : -1;
      int32_t lo_head   = hw ? 64 * lane + __builtin_ctzll(hw) : RANK_TILE;
      for (int o = 1; o < 64; o <<= 1) {
        int32_t const up   = __shfl_up(hi_head, o, 64);
        int32_t const down = __shfl_down(lo_head, o, 64);
        if (lane >= o) hi_head = std::max(hi_head, up);
        if (lane + o < 64) lo_head = std::min(lo_head, down);
      }
      int32_t const before = __shfl_up(hi_head, 1, 64);
      int32_t const after  = __shfl_down(lo_head, 1, 64);
      if (lane < RANK_WORDS) {
        last_before[lane] = lane == 0 ? -1 : before;
        first_after[lane] = lane == 63 ? RANK_TILE : after;
      }
      int64_t run_first = base, run_end = last + 1;
      if (base > 0 && (heads[0] & 1ull) == 0)  // the run of position base - 1 goes on: the words in [0, base - 1) hold its start
        run_first = wave_bound<NW, false>(w0, w1, load_key<NW>(w0, w1, base), 0, base - 1, lane);
      if (last + 1 < n) {
        rank_key<NW> const k = load_key<NW>(w0, w1, last);
        if (key_equal<NW>(k, load_key<NW>(w0, w1, last + 1))) run_end = wave_bound<NW, true>(w0, w1, k, last + 2, n, lane);
      }
      if (lane == 0) edge[0] = run_first, edge[1] = run_end;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < RANK_ITEMS; ++k) {
      int64_t const p = base + k * 256 + threadIdx.x;
      if (p >= n) continue;
      int const j          = k * 4 + wave;  // p's ballot; its bit is `lane`
      uint64_t const hw    = heads[j];
      uint64_t const below = hw & (~0ull >> (63 - lane));
      uint64_t const above = lane < 63 ? hw & (~0ull << (lane + 1)) : 0;
      int64_t first, end;  // p's run is [first, end)
      if (below) {
        first = base + 64 * j + 63 - __builtin_clzll(below);
      } else {
        first = last_before[j] >= 0 ? base + last_before[j] : edge[0];
      }
      if (above) {
        end = base + 64 * j + __builtin_ctzll(above);
      } else {
        end = first_after[j] < RANK_TILE ? base + first_after[j] : edge[1];
      }
      OUT r;
      if (method == static_cast<int32_t>(rank_method::MIN)) {
        r = static_cast<OUT>(first + 1);
      } else if (method == static_cast<int32_t>(rank_method::MAX)) {
        r = static_cast<OUT>(end);
      } else {  // rank.cu:244-247
        r = static_cast<OUT>(static_cast<double>(first + 1) + (static_cast<double>(end - first) - 1) / 2.0);
      }
      gstore(out + row[k], finish_rank<OUT>(r, percentage, divisor));
    }
    __syncthreads();  // (the next tile writes heads and edge)
  }
}

// counts[t] = the heads of tile t. The workgroup that has tile q_tile also writes *q_heads = the heads of that tile at tile
// positions <= q_local (q_local < 0: none).
template <int NW>
__global__ void __launch_bounds__(256) k_rank_dense_count(uint64_t const* w0, uint64_t const* w1, int64_t n, uint32_t* counts,
                                                          int64_t q_tile, int32_t q_local, uint32_t* q_heads)
{
  __shared__ uint64_t heads[RANK_WORDS];
  int const lane      = threadIdx.x & 63;
  int64_t const tiles = (n + RANK_TILE - 1) / RANK_TILE;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    tile_heads<NW>(w0, w1, t * RANK_TILE, n, heads);
    __syncthreads();
    if (threadIdx.x < 64) {
      uint64_t const hw = lane < RANK_WORDS ? heads[lane] : 0;
      // the part of this ballot at or below q_local
      int const q_bits    = q_local - 64 * lane;
      uint64_t const upto = q_bits < 0 ? 0 : q_bits >= 63 ? hw : hw & (~0ull >> (63 - q_bits));
      uint32_t all = __popcll(hw), part = __popcll(upto);
      for (int o = 32; o > 0; o >>= 1) {
        all += __shfl_xor(all, o, 64);
        part += __shfl_xor(part, o, 64);
      }
      if (lane == 0) {
        gstore(counts + t, all);
        if (t == q_tile) gstore(q_heads, part);
      }
    }
    __syncthreads();
  }
}

// rank.cu:57-97,165-177: out[order[i]] = the heads in [0, i]; tile_base: the exclusive scan of the counts. A percentage divides by
// tile_base[q_tile] + *q_heads.
template <typename OUT, int NW>
__global__ void __launch_bounds__(256) k_rank_dense_apply(uint64_t const* w0, uint64_t const* w1, uint32_t const* order, OUT* out,
                                                          int64_t n, uint32_t const* tile_base, bool percentage, int64_t q_tile,
                                                          uint32_t const* q_heads)
{
  __shared__ uint64_t heads[RANK_WORDS];
  __shared__ uint32_t heads_before[RANK_WORDS];  // the heads of the ballots before this one
  int const lane      = threadIdx.x & 63;
  int const wave      = threadIdx.x >> 6;
  int64_t const tiles = (n + RANK_TILE - 1) / RANK_TILE;
  double divisor      = 1.0;
  if (percentage) divisor = static_cast<double>(gload(tile_base + q_tile) + gload(q_heads));
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    int64_t const base = t * RANK_TILE;
    uint32_t row[RANK_ITEMS];
#pragma unroll
    for (int k = 0; k < RANK_ITEMS; ++k) {
      int64_t const p = base + k * 256 + threadIdx.x;
      row[k]          = p < n ? gload(order + p) : 0u;
    }
    uint32_t const before_tile = gload(tile_base + t);
    tile_heads<NW>(w0, w1, base, n, heads);
    __syncthreads();
    if (wave == 0) {
      uint32_t const mine = lane < RANK_WORDS ? __popcll(heads[lane]) : 0;
      uint32_t incl       = mine;
      for (int o = 1; o < 64; o <<= 1) {
        uint32_t const up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
      }
      if (lane < RANK_WORDS) heads_before[lane] = incl - mine;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < RANK_ITEMS; ++k) {
      int64_t const p = base + k * 256 + threadIdx.x;
      if (p >= n) continue;
      int const j          = k * 4 + wave;
      uint32_t const dense = before_tile + heads_before[j] + __popcll(heads[j] & (~0ull >> (63 - lane)));
      gstore(out + row[k], finish_rank<OUT>(static_cast<OUT>(dense), percentage, divisor));
    }
    __syncthreads();
  }
}

unsigned tile_grid(int64_t n)
{
  return static_cast<unsigned>(std::min<int64_t>((n + RANK_TILE - 1) / RANK_TILE, 256 * 16));
}
}  // namespace

template <typename OUT>
void launch_rank_first(uint32_t const* order, OUT* out, int64_t n, bool percentage, double divisor, hipStream_t s)
{
  if (n <= 0) return;
  auto const grid = static_cast<unsigned>(std::min<int64_t>((n + 255) / 256, 256 * 16));
  prof::scope p_{"rank_first", s};
  hipLaunchKernelGGL(k_rank_first<OUT>, dim3(grid), dim3(256), 0, s, order, out, n, percentage, divisor);
  CUDF_HIP_TRY(hipGetLastError());
}

template <typename OUT>
void launch_rank_ties(rank_words const& w, uint32_t const* order, OUT* out, int64_t n, rank_method method, bool percentage,
                      double divisor, hipStream_t s)
{
  if (n <= 0) return;
  auto const m = static_cast<int32_t>(method);
  prof::scope p_{"rank_ties", s};
  if (w.hi != nullptr) {
    hipLaunchKernelGGL((k_rank_ties<OUT, 2>), dim3(tile_grid(n)), dim3(256), 0, s, w.lo, w.hi, order, out, n, m, percentage, divisor);
  } else {
    hipLaunchKernelGGL((k_rank_ties<OUT, 1>), dim3(tile_grid(n)), dim3(256), 0, s, w.lo, w.hi, order, out, n, m, percentage, divisor);
  }
  CUDF_HIP_TRY(hipGetLastError());
}

void launch_rank_dense_count(rank_words const& w, int64_t n, uint32_t* counts, int64_t q, uint32_t* q_heads, hipStream_t s)
{
  if (n <= 0) return;
  int64_t const q_tile  = q < 0 ? 0 : q / RANK_TILE;
  int32_t const q_local = q < 0 ? -1 : static_cast<int32_t>(q % RANK_TILE);
  prof::scope p_{"rank_dense_count", s};
  if (w.hi != nullptr) {
    hipLaunchKernelGGL(k_rank_dense_count<2>, dim3(tile_grid(n)), dim3(256), 0, s, w.lo, w.hi, n, counts, q_tile, q_local, q_heads);
  } else {
    hipLaunchKernelGGL(k_rank_dense_count<1>, dim3(tile_grid(n)), dim3(256), 0, s, w.lo, w.hi, n, counts, q_tile, q_local, q_heads);
  }
  CUDF_HIP_TRY(hipGetLastError());
}

template <typename OUT>
void launch_rank_dense_apply(rank_words const& w, uint32_t const* order, OUT* out, int64_t n, uint32_t const* tile_base,
                             bool percentage, int64_t q, uint32_t const* q_heads, hipStream_t s)
{
  if (n <= 0) return;
  int64_t const q_tile = q < 0 ? 0 : q / RANK_TILE;
  prof::scope p_{"rank_dense_apply", s};
  if (w.hi != nullptr) {
    hipLaunchKernelGGL((k_rank_dense_apply<OUT, 2>), dim3(tile_grid(n)), dim3(256), 0, s, w.lo, w.hi, order, out, n, tile_base,
                       percentage, q_tile, q_heads);
  } else {
    hipLaunchKernelGGL((k_rank_dense_apply<OUT, 1>), dim3(tile_grid(n)), dim3(256), 0, s, w.lo, w.hi, order, out, n, tile_base,
                       percentage, q_tile, q_heads);
  }
  CUDF_HIP_TRY(hipGetLastError());
}

template void launch_rank_first<int32_t>(uint32_t const*, int32_t*, int64_t, bool, double, hipStream_t);
template void launch_rank_first<double>(uint32_t const*, double*, int64_t, bool, double, hipStream_t);
template void launch_rank_ties<int32_t>(rank_words const&, uint32_t const*, int32_t*, int64_t, rank_method, bool, double, hipStream_t);
template void launch_rank_ties<double>(rank_words const&, uint32_t const*, double*, int64_t, rank_method, bool, double, hipStream_t);
template void launch_rank_dense_apply<int32_t>(rank_words const&, uint32_t const*, int32_t*, int64_t, uint32_t const*, bool, int64_t,
                                               uint32_t const*, hipStream_t);
template void launch_rank_dense_apply<double>(rank_words const&, uint32_t const*, double*, int64_t, uint32_t const*, bool, int64_t,
                                              uint32_t const*, hipStream_t);

}  // namespace cudf::detail::sorting
