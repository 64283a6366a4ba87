// SPDX-License-Identifier: Apache-2.0
// The stable LSD radix sort of (64-bit word, 32-bit payload) pairs and the device-wide uint32 exclusive scan (radix_sort.hpp).
// Nothing here knows of groups; the one place that reads columns is k_fill_words, which makes the words a pass sorts by.
#include "sort_helper.hpp"
#include "../common/profiler.hpp"
#include "../sorting/sorting_impl.hpp"

#include <cudf/utilities/error.hpp>

#include <optional>

namespace cudf::groupby::detail {
namespace {
using cudf::detail::col_is_valid;
using cudf::detail::gload;
using cudf::detail::gstore;
namespace prof = cudf::detail::prof;

constexpr int RS_THREADS = 256;
constexpr int RS_WAVES   = RS_THREADS / 64;
constexpr int RS_ITEMS   = 16;                     // keys per thread
constexpr int RS_TILE    = RS_THREADS * RS_ITEMS;  // keys per workgroup

__device__ __forceinline__ uint64_t wave_or(uint64_t v)
{
  for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ uint64_t wave_and(uint64_t v)
{
  for (int o = 32; o > 0; o >>= 1) v &= __shfl_xor(v, o, 64);
  return v;
}

// words[i] = the word of a's source for the payload at position i (radix_sort.hpp word_source); OR / AND of all words into or_and
__global__ void __launch_bounds__(256) k_fill_words(fill_args a)
{
  uint64_t vor = 0, vand = ~0ull;
  uint32_t ones = 0;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < a.n; i += static_cast<int64_t>(gridDim.x) * 256) {
    uint32_t const p = a.payload ? gload(a.payload + i) : static_cast<uint32_t>(i);
    auto const row   = [&] { return a.order ? gload(a.order + p) : p; };  // (a gather: looked up only where a source reads the row)
    uint64_t w;
    if (a.source == WORD_VALUE) {
      uint32_t const r = row();
      w                = col_is_valid(a.col, r) ? sortable_word(a.col, r) : 0;
      if (a.invert) w = ~w;
    } else if (a.source == WORD_NULL_FLAG) {
      w = col_is_valid(a.col, row()) ? 0 : 1;
    } else if (a.source == WORD_ANY_NULL) {
      w = cudf::detail::row_has_null(a.keys, row()) ? 1 : 0;
      ones += static_cast<uint32_t>(w);
    } else {
      bool const valid = a.col.mask == nullptr || col_is_valid(a.col, row());  // no mask: the row is not looked up at all
      w                = (static_cast<uint64_t>(static_cast<uint32_t>(gload(a.labels + p))) << 1) | (valid != a.nulls_first ? 0 : 1);
    }
    gstore(a.words + i, w);
    vor |= w;
    vand &= w;
  }
  vor  = wave_or(vor);
  vand = wave_and(vand);
  if ((threadIdx.x & 63) == 0) {
    atomicOr(reinterpret_cast<unsigned long long*>(a.or_and), static_cast<unsigned long long>(vor));
    atomicAnd(reinterpret_cast<unsigned long long*>(a.or_and + 1), static_cast<unsigned long long>(vand));
  }
  if (a.ones != nullptr) {
    for (int o = 32; o > 0; o >>= 1) ones += __shfl_xor(ones, o, 64);
    if ((threadIdx.x & 63) == 0 && ones) atomicAdd(a.ones, ones);
  }
}

__global__ void __launch_bounds__(256) k_iota(uint32_t* out, int64_t n)
{
  int64_t const i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i < n) gstore(out + i, static_cast<uint32_t>(i));
}

__global__ void k_init_or_and(uint64_t* or_and, uint32_t* ones)
{
  or_and[0] = 0;
  or_and[1] = ~0ull;
  if (ones) *ones = 0;
}

__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v, int lane)
{
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    uint32_t const t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// exclusive prefix of `v` over the workgroup's threads; `total` = the workgroup's sum
template <int THREADS>
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t& total, uint32_t* wave_sums /* THREADS / 64 + 1 */)
{
  int const lane     = threadIdx.x & 63;
  int const w        = threadIdx.x >> 6;
  uint32_t const inc = wave_inclusive_scan(v, lane);
  __syncthreads();  // wave_sums may still be read from the previous use
  if (lane == 63) wave_sums[w] = inc;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (int i = 0; i < THREADS / 64; ++i) {
    uint32_t const s = wave_sums[i];
    if (i < w) before += s;
    all += s;
  }
  total = all;
  return before + inc - v;
}

// ---------------------------------------------------------------------------------------------------------
// radix pass. Lanes of one wave that hold the same digit find each other with eight ballots (one per digit bit); the lowest such lane
// updates the wave's counter for the digit, so no two lanes of a wave ever touch one counter and a run of equal keys costs what a
// random one does.
__device__ __forceinline__ uint64_t digit_peers(uint32_t d, bool active)
{
  uint64_t m = __ballot(active);
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    bool const bit    = (d >> b) & 1u;
    uint64_t const bb = __ballot(bit);
    m &= bit ? bb : ~bb;
  }
  return m;
}
__device__ __forceinline__ uint32_t lanes_below(uint64_t m, int lane) { return __popcll(m & ((1ull << lane) - 1ull)); }

// hist[d * nblocks + b] = number of keys of workgroup b's tile whose digit is d
__global__ void __launch_bounds__(RS_THREADS) k_radix_hist(uint64_t const* keys, int64_t n, int shift, uint32_t* hist, uint32_t nblocks)
{
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  int const lane     = threadIdx.x & 63;
  int64_t const base = static_cast<int64_t>(blockIdx.x) * RS_TILE + (threadIdx.x >> 6) * (64 * RS_ITEMS);
#pragma unroll 4
  for (int r = 0; r < RS_ITEMS; ++r) {
    int64_t const i    = base + r * 64 + lane;
    bool const active  = i < n;
    uint32_t const d   = active ? static_cast<uint32_t>(gload(keys + i) >> shift) & 255u : 0u;
    uint64_t const m   = digit_peers(d, active);
    if (active && lanes_below(m, lane) == 0) atomicAdd(&h[d], static_cast<uint32_t>(__popcll(m)));
  }
  __syncthreads();
  hist[static_cast<size_t>(threadIdx.x) * nblocks + blockIdx.x] = h[threadIdx.x];
}

// stable scatter of one tile: element order inside the tile is (wave, round, lane). The tile is first put in digit order inside
// LDS, then written out: consecutive lanes then write consecutive addresses inside each digit's run (16 elements on average)
// instead of 64 lanes writing to 64 runs.
__global__ void __launch_bounds__(RS_THREADS) k_radix_scatter(uint64_t const* kin, uint32_t const* pin, uint64_t* kout, uint32_t* pout,
                                                              int64_t n, int shift, uint32_t const* bases, uint32_t nblocks)
{
  __shared__ uint32_t cnt[RS_WAVES][256];
  __shared__ uint32_t delta[256];  // global position of a digit's run minus its position inside the tile
  __shared__ uint32_t ws[RS_THREADS / 64 + 1];
  __shared__ uint64_t skey[RS_TILE];
  __shared__ uint32_t spay[RS_TILE];
  for (int i = threadIdx.x; i < RS_WAVES * 256; i += RS_THREADS) (&cnt[0][0])[i] = 0;
  __syncthreads();
  int const lane          = threadIdx.x & 63;
  int const w             = threadIdx.x >> 6;
  int64_t const tile_base = static_cast<int64_t>(blockIdx.x) * RS_TILE;
  int64_t const base      = tile_base + w * (64 * RS_ITEMS);
  uint64_t key[RS_ITEMS];
  uint32_t pay[RS_ITEMS];
  uint32_t loc[RS_ITEMS];  // digit << 16 | rank among the wave's keys of that digit
#pragma unroll
  for (int r = 0; r < RS_ITEMS; ++r) {
    int64_t const i = base + r * 64 + lane;
    key[r]          = i < n ? gload(kin + i) : 0;
    pay[r]          = i < n ? (pin ? gload(pin + i) : static_cast<uint32_t>(i)) : 0;
  }
#pragma unroll
  for (int r = 0; r < RS_ITEMS; ++r) {
    bool const active   = base + r * 64 + lane < n;
    uint32_t const d    = static_cast<uint32_t>(key[r] >> shift) & 255u;
    uint64_t const m    = digit_peers(d, active);
    uint32_t const rank = lanes_below(m, lane);
    uint32_t const seen = cnt[w][d];
    __builtin_amdgcn_wave_barrier();
    if (active && rank == 0) cnt[w][d] = seen + static_cast<uint32_t>(__popcll(m));
    __builtin_amdgcn_wave_barrier();
    loc[r] = (d << 16) | (seen + rank);
  }
  __syncthreads();
  {
    uint32_t const d = threadIdx.x;
    uint32_t c[RS_WAVES];
    uint32_t all = 0;
#pragma unroll
    for (int ww = 0; ww < RS_WAVES; ++ww) {
      c[ww] = cnt[ww][d];
      all += c[ww];
    }
    uint32_t total;
    uint32_t start = block_exclusive_scan<RS_THREADS>(all, total, ws);  // the digit's run inside the tile
    delta[d]       = gload(bases + static_cast<size_t>(d) * nblocks + blockIdx.x) - start;
#pragma unroll
    for (int ww = 0; ww < RS_WAVES; ++ww) {
      cnt[ww][d] = start;
      start += c[ww];
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < RS_ITEMS; ++r) {
    if (base + r * 64 + lane < n) {
      uint32_t const at = cnt[w][loc[r] >> 16] + (loc[r] & 0xffffu);
      skey[at]          = key[r];
      spay[at]          = pay[r];
    }
  }
  __syncthreads();
  int const live = static_cast<int>(n - tile_base < RS_TILE ? n - tile_base : RS_TILE);
#pragma unroll
  for (int r = 0; r < RS_ITEMS; ++r) {
    int const at = r * RS_THREADS + threadIdx.x;
    if (at < live) {
      uint64_t const k   = skey[at];
      uint32_t const pos = delta[static_cast<uint32_t>(k >> shift) & 255u] + static_cast<uint32_t>(at);
      gstore(kout + pos, k);
      gstore(pout + pos, spay[at]);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// exclusive scan of uint32 (counts of at most 2^31 in total): tile sums -> scan of the tile sums -> tiles again with their base
constexpr int SC_THREADS = 256;
constexpr int SC_ITEMS   = 16;
constexpr int SC_TILE    = SC_THREADS * SC_ITEMS;

__global__ void __launch_bounds__(SC_THREADS) k_scan_tile_sums(uint32_t const* in, int64_t n, uint32_t* tile_sums)
{
  __shared__ uint32_t ws[SC_THREADS / 64 + 1];
  int64_t const base = static_cast<int64_t>(blockIdx.x) * SC_TILE;
  uint32_t v         = 0;
#pragma unroll
  for (int r = 0; r < SC_ITEMS; ++r) {
    int64_t const i = base + r * SC_THREADS + threadIdx.x;
    if (i < n) v += gload(in + i);
  }
  uint32_t total;
  block_exclusive_scan<SC_THREADS>(v, total, ws);
  if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

// in place, one workgroup; total (optional) receives the sum of everything
__global__ void __launch_bounds__(1024) k_scan_spine(uint32_t* sums, int64_t count, uint32_t* total_out)
{
  __shared__ uint32_t ws[1024 / 64 + 1];
  uint32_t carry = 0;
  for (int64_t first = 0; first < count; first += 1024) {
    int64_t const i  = first + threadIdx.x;
    uint32_t const v = i < count ? sums[i] : 0;
    uint32_t total;
    uint32_t const ex = block_exclusive_scan<1024>(v, total, ws);
    if (i < count) sums[i] = carry + ex;
    carry += total;
  }
  if (total_out != nullptr && threadIdx.x == 0) *total_out = carry;
}

__global__ void __launch_bounds__(SC_THREADS) k_scan_apply(uint32_t const* in, uint32_t* out, int64_t n, uint32_t const* tile_bases)
{
  __shared__ uint32_t ws[SC_THREADS / 64 + 1];
  int64_t const first = static_cast<int64_t>(blockIdx.x) * SC_TILE + static_cast<int64_t>(threadIdx.x) * SC_ITEMS;
  uint32_t v[SC_ITEMS];
  uint32_t sum = 0;
#pragma unroll
  for (int k = 0; k < SC_ITEMS; ++k) {
    v[k] = first + k < n ? gload(in + first + k) : 0;
    sum += v[k];
  }
  uint32_t total;
  uint32_t run = gload(tile_bases + blockIdx.x) + block_exclusive_scan<SC_THREADS>(sum, total, ws);
#pragma unroll
  for (int k = 0; k < SC_ITEMS; ++k) {
    if (first + k < n) gstore(out + first + k, run);
    run += v[k];
  }
}

unsigned fill_grid(int64_t n) { return static_cast<unsigned>(std::min<int64_t>((n + 255) / 256, 256 * 16)); }
}  // namespace

void exclusive_scan(uint32_t const* in, uint32_t* out, int64_t n, uint32_t* total, scratch& sc, hipStream_t s)
{
  if (n <= 0) {
    if (total) CUDF_HIP_TRY(hipMemsetAsync(total, 0, sizeof(uint32_t), s));
    return;
  }
  int64_t const tiles = (n + SC_TILE - 1) / SC_TILE;
  auto* sums          = sc.alloc<uint32_t>(static_cast<std::size_t>(tiles));
  prof::scope p_{"sort_scan", s};
  hipLaunchKernelGGL(k_scan_tile_sums, dim3(static_cast<unsigned>(tiles)), dim3(SC_THREADS), 0, s, in, n, sums);
  hipLaunchKernelGGL(k_scan_spine, dim3(1), dim3(1024), 0, s, sums, tiles, total);
  hipLaunchKernelGGL(k_scan_apply, dim3(static_cast<unsigned>(tiles)), dim3(SC_THREADS), 0, s, in, out, n, sums);
  CUDF_HIP_TRY(hipGetLastError());
}

void iota(uint32_t* out, int64_t n, hipStream_t s) { hipLaunchKernelGGL(k_iota, dim3(blocks_of(n)), dim3(256), 0, s, out, n); }

pair_sorter::pair_sorter(int64_t n, scratch& sc, hipStream_t s) : _n{n}, _sc{sc}, _s{s}
{
  _nblocks = static_cast<uint32_t>((n + RS_TILE - 1) / RS_TILE);
  for (int i = 0; i < 2; ++i) {
    _k[i] = sc.alloc<uint64_t>(static_cast<std::size_t>(n));
    _p[i] = sc.alloc<uint32_t>(static_cast<std::size_t>(n));
  }
  _hist   = sc.alloc<uint32_t>(static_cast<std::size_t>(_nblocks) * 256);
  _or_and = sc.alloc<uint64_t>(2);
  _ones   = sc.alloc<uint32_t>(1);
}

uint32_t pair_sorter::sort_by(fill_args fa)
{
  fa.n       = _n;
  fa.or_and  = _or_and;
  fa.ones    = fa.source == WORD_ANY_NULL ? _ones : nullptr;
  reset_reduction();
  fa.payload = payload();
  fa.words   = _k[_cur];
  {
    std::optional<prof::scope> p_;  // the profile counts the fills of value and label words, not those of the null flags
    if (fa.source == WORD_VALUE || fa.source == WORD_LABEL_NULL) p_.emplace("sort_words", _s);
    hipLaunchKernelGGL(k_fill_words, dim3(fill_grid(_n)), dim3(256), 0, _s, fa);
  }
  return sort_filled();
}

void pair_sorter::sort_by_packed(cudf::detail::sorting::plan_word const& w)
{
  reset_reduction();
  cudf::detail::sorting::launch_fill_packed_words(w, payload(), _k[_cur], _or_and, _n, _s);
  sort_filled();
}

void pair_sorter::reset_reduction() { hipLaunchKernelGGL(k_init_or_and, dim3(1), dim3(1), 0, _s, _or_and, _ones); }

// reads back the OR / AND of the words just filled and sorts by the digits that differ
uint32_t pair_sorter::sort_filled()
{
  struct {
    uint64_t or_and[2];
    uint32_t ones;
  } h{};
  CUDF_HIP_TRY(hipMemcpyAsync(h.or_and, _or_and, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, _s));
  CUDF_HIP_TRY(hipMemcpyAsync(&h.ones, _ones, sizeof(uint32_t), hipMemcpyDeviceToHost, _s));
  CUDF_HIP_TRY(hipStreamSynchronize(_s));
  uint64_t const differ = h.or_and[0] ^ h.or_and[1];
  for (int b = 0; b < 8; ++b)
    if ((differ >> (8 * b)) & 0xffu) pass(8 * b);
  return h.ones;
}

uint32_t* pair_sorter::finish()
{
  if (_identity) {
    iota(_p[_cur], _n, _s);
    _identity = false;
  }
  return _p[_cur];
}

void pair_sorter::pass(int shift)
{
  {
    prof::scope p_{"sort_hist", _s};
    hipLaunchKernelGGL(k_radix_hist, dim3(_nblocks), dim3(RS_THREADS), 0, _s, _k[_cur], _n, shift, _hist, _nblocks);
  }
  exclusive_scan(_hist, _hist, static_cast<int64_t>(_nblocks) * 256, nullptr, _sc, _s);
  {
    prof::scope p_{"sort_scatter", _s};
    hipLaunchKernelGGL(k_radix_scatter, dim3(_nblocks), dim3(RS_THREADS), 0, _s, _k[_cur], payload(), _k[_cur ^ 1], _p[_cur ^ 1], _n, shift,
                       _hist, _nblocks);
  }
  CUDF_HIP_TRY(hipGetLastError());
  _cur ^= 1;
  _identity = false;
}

}  // namespace cudf::groupby::detail
