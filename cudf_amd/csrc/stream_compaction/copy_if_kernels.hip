// SPDX-License-Identifier: Apache-2.0
// Kernels of cudf::apply_boolean_mask, apply_deletion_mask, drop_nulls, drop_nans, unique and unique_count: the selection passes
// and the two compaction passes. Arguments, layout and the model: copy_if_impl.hpp; DESIGN.md section 4, "Filtering rows".
#include "copy_if_impl.hpp"
#include "../common/profiler.hpp"
#include "../common/row_set.hpp"

namespace cudf::detail::copy_if {
namespace {
using namespace cudf::detail::rowset;

constexpr int THREADS = 256;  // 4 waves per workgroup, a chunk per wave, in every kernel of this file

__device__ __forceinline__ int64_t wave_of_block() { return static_cast<int64_t>(blockIdx.x) * (THREADS / 64) + (threadIdx.x >> 6); }

// 64 bits of a bitmask from bit `bit` on. Words beyond `last_word` (the word of the column's last row) are not read: they count as
// zero, and the caller masks or ignores the bits of rows that do not exist.
__device__ __forceinline__ uint64_t funnel64(bitmask_type const* m, int64_t bit, int64_t last_word)
{
  int64_t const i   = bit >> 5;
  int const sh      = static_cast<int>(bit & 31);
  uint64_t const w0 = i <= last_word ? gload(m + i) : 0u;
  uint64_t const w1 = i + 1 <= last_word ? gload(m + i + 1) : 0u;
  uint64_t const lo = w0 | (w1 << 32);
  if (sh == 0) return lo;
  uint64_t const w2 = i + 2 <= last_word ? gload(m + i + 2) : 0u;
  return (lo >> sh) | (w2 << (64 - sh));
}

__device__ __forceinline__ bool bits_are_nan(uint64_t bits, int32_t cls)
{
  if (cls == CLS_F32) return (static_cast<uint32_t>(bits) & 0x7fffffffu) > 0x7f800000u;
  if (cls == CLS_F64) return (bits & 0x7fffffffffffffffull) > 0x7ff0000000000000ull;
  return false;
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ------------------------------------------------------------------ pass 1: a row per lane
template <bool DELETION>
__global__ void __launch_bounds__(THREADS) k_select_bool(bool_args a)
{
  probe_chunk<8, true>(
    a, wave_of_block(), [&](int64_t r) { return key{load_int<1, false>(a.m, r), col_is_valid(a.m, r)}; },
    [&](key k, int64_t) { return k.valid && (DELETION ? k.v == 0 : k.v != 0); });
}

__global__ void __launch_bounds__(THREADS) k_select_valid_count(valid_args a)
{
  probe_chunk<2, true>(
    a, wave_of_block(), [](int64_t) { return no_key{}; },
    [&](no_key, int64_t r) {
      int32_t n = 0;
      for (int k = 0; k < a.nkeys; ++k) {
        int64_t const b = a.key[k].offset + r;
        n += (gload(a.key[k].mask + (b >> 5)) >> (b & 31)) & 1u;
      }
      return n >= a.need;
    });
}

__global__ void __launch_bounds__(THREADS) k_select_nan(nan_args a)
{
  probe_chunk<2, true>(
    a, wave_of_block(), [](int64_t) { return no_key{}; },
    [&](no_key, int64_t r) {
      int32_t n = 0;
      for (int c = 0; c < a.keys.ncols; ++c) {
        device_column const& col = a.keys.col[c];
        n += !col_is_valid(col, r) || !bits_are_nan(col_load_bits(col, r), col.cls);
      }
      return n >= a.need;
    });
}

template <int KEEP>
__global__ void __launch_bounds__(THREADS) k_select_unique(unique_args a)
{
  probe_chunk<1, true>(
    a, wave_of_block(), [](int64_t) { return no_key{}; },
    [&](no_key, int64_t r) {
      bool const eq = a.nulls_equal != 0;
      bool q        = true;
      if constexpr (KEEP != static_cast<int>(keep::last)) q = q && (r == 0 || !rows_equal(a.keys, r, a.keys, r - 1, eq));
      if constexpr (KEEP != static_cast<int>(keep::first)) q = q && (r == a.nrows - 1 || !rows_equal(a.keys, r, a.keys, r + 1, eq));
      return q;
    });
}

// reference cpp/src/reductions/unique_count_column.cu, rule for rule (nan_is_null is 0 for a column that is not floating point:
// the rule it switches then agrees with the comparison)
__global__ void __launch_bounds__(THREADS) k_select_unique_column(unique_column_args a)
{
  probe_chunk<1, true>(
    a, wave_of_block(), [](int64_t) { return no_key{}; },
    [&](no_key, int64_t r) {
      device_column const& c = a.keys.col[0];
      bool const is_null     = !col_is_valid(c, r);
      bool const is_nan      = a.nan_is_null != 0 && bits_are_nan(col_load_bits(c, r), c.cls);
      if (a.count_nulls == 0 && (is_null || is_nan)) return false;
      if (r == 0) return true;
      if (a.count_nulls != 0 && a.nan_is_null != 0 && (is_nan || is_null))
        return !(bits_are_nan(col_load_bits(c, r - 1), c.cls) || !col_is_valid(c, r - 1));
      return !rows_equal(a.keys, r, a.keys, r - 1, true);
    });
}

// ------------------------------------------------------------------ pass 1: 64 rows per lane
// drop_nulls when every nullable key must be valid: a lane ANDs the 64 validity bits of each key for its word of the selection.
__global__ void __launch_bounds__(THREADS) k_select_valid_words(valid_args a)
{
  int const lane       = threadIdx.x & 63;
  int64_t const wave   = wave_of_block();
  int64_t const begin  = wave * a.chunk;  // (a multiple of 512: a word never spans two chunks)
  int64_t const end    = a.nrows < begin + a.chunk ? a.nrows : begin + a.chunk;
  unsigned long long n = 0;
  int64_t const w_end  = (end + 63) >> 6;
  for (int64_t w = (begin >> 6) + lane; begin < end && w < w_end; w += 64) {
    uint64_t v = ~uint64_t{0};
    for (int k = 0; k < a.nkeys; ++k) v &= funnel64(a.key[k].mask, a.key[k].offset + w * 64, (a.key[k].offset + a.nrows - 1) >> 5);
    int64_t const left = a.nrows - w * 64;
    if (left < 64) v &= (uint64_t{1} << left) - 1;
    gstore(a.mask + w, v);
    n += __popcll(v);
  }
  n = wave_sum(n);
  if (lane == 0 && wave < a.nwaves) gstore(a.counts + wave, n);
}

// ------------------------------------------------------------------ pass 2a: the fused compaction copy
template <int W>
__device__ __forceinline__ uint64_t load_w(void const* p, int64_t i)
{
  if constexpr (W == 1) return gload(static_cast<uint8_t const*>(p) + i);
  else if constexpr (W == 2) return gload(static_cast<uint16_t const*>(p) + i);
  else if constexpr (W == 4) return gload(static_cast<uint32_t const*>(p) + i);
  else return gload(static_cast<uint64_t const*>(p) + i);
}
__device__ __forceinline__ uint64_t load_width(void const* p, int64_t i, int64_t width)
{
  switch (width) {
    case 1: return load_w<1>(p, i);
    case 2: return load_w<2>(p, i);
    case 4: return load_w<4>(p, i);
    default: return load_w<8>(p, i);
  }
}
__device__ __forceinline__ void store_width(void* p, uint64_t i, int64_t width, uint64_t v)
{
  switch (width) {
    case 1: gstore(static_cast<uint8_t*>(p) + i, static_cast<uint8_t>(v)); break;
    case 2: gstore(static_cast<uint16_t*>(p) + i, static_cast<uint16_t>(v)); break;
    case 4: gstore(static_cast<uint32_t*>(p) + i, static_cast<uint32_t>(v)); break;
    default: gstore(static_cast<uint64_t*>(p) + i, v);
  }
}

// A wave per chunk. The batch's columns are read from device memory once, into scalar registers (the loop over them is unrolled:
// no indexed copy of them exists); every set bit then loads its row's element of each column, back to back, and stores them at
// the row's position. A zero selection word costs nothing (compact_chunk skips it).
__global__ void __launch_bounds__(THREADS) k_copy_if_data(data_args const* __restrict__ p)
{
  data_args const& a = *p;
  int const ncols    = a.ncols;
  uint64_t const cap = a.out_rows;
  data_col col[DATA_COLS];
#pragma unroll
  for (int c = 0; c < DATA_COLS; ++c) col[c] = a.col[c < ncols ? c : 0];
  compact_chunk(a.mask, a.counts, wave_of_block(), a.chunk, a.nrows, [&](uint64_t o, int64_t row) {
    if (o >= cap) return;
    uint64_t v[DATA_COLS];
#pragma unroll
    for (int c = 0; c < DATA_COLS; ++c)
      if (c < ncols) v[c] = load_width(col[c].src, row, col[c].width);
#pragma unroll
    for (int c = 0; c < DATA_COLS; ++c)
      if (c < ncols) store_width(col[c].dst, o, col[c].width, v[c]);
  });
}

// ------------------------------------------------------------------ pass 2b: the bitmask compaction
// The bits of x at the set positions of m, packed low: the parallel-suffix compress of Hacker's Delight (7-4), 64 bits wide. Six
// rounds without a branch, so the lanes of a wave stay together whatever their words hold; a loop over the set bits takes up to 64
// dependent rounds for the wave as soon as one lane's word is dense.
__device__ __forceinline__ uint64_t compress64(uint64_t x, uint64_t m)
{
  x &= m;
  uint64_t mk = ~m << 1;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    uint64_t mp = mk ^ (mk << 1);
    mp ^= mp << 2;
    mp ^= mp << 4;
    mp ^= mp << 8;
    mp ^= mp << 16;
    mp ^= mp << 32;
    uint64_t const mv = mp & m;
    m                 = (m ^ mv) | (mv >> (1 << i));
    uint64_t const t  = x & mv;
    x                 = (x ^ t) | (t >> (1 << i));
    mk &= ~mp;
  }
  return x;
}

// orders the wave's LDS traffic before the call against its LDS traffic after it (the staging area is private to the wave)
__device__ __forceinline__ void wave_lds_sync()
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// relaxed device-scope atomics on global addresses (global_atomic_*: a flat atomic would also wait on the LDS counter)
__device__ __forceinline__ void global_or(uint32_t* p, uint32_t v)
{
  (void)__hip_atomic_fetch_or((CUDF_AMD_GLOBAL_AS uint32_t*)(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void global_add(unsigned long long* p, unsigned long long v)
{
  (void)__hip_atomic_fetch_add((CUDF_AMD_GLOBAL_AS unsigned long long*)(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

constexpr int STAGE_WORDS = 130;  // 64 x 64 bits, up to 31 bits of misalignment in front, one spill word

// A wave per chunk, 64 selection words at a time: lane k holds word k and the number of set bits before it (the arithmetic of
// compact_chunk). Per nullable column it extracts the validity bits of its rows at the set positions, ORs them into the stage at
// (base + bits before) - 32 * floor(base / 32), and the wave writes the staged words out: the first and the last word of the range
// belong in part to the neighbouring wave or to the previous and next round, so they go with a global atomicOr into the zero-filled
// output; the words between are this round's alone and go with plain stores.
__global__ void __launch_bounds__(THREADS) k_copy_if_validity(validity_args const* __restrict__ p)
{
  __shared__ uint32_t s_stage[THREADS / 64][STAGE_WORDS];
  validity_args const& a = *p;
  int const lane         = threadIdx.x & 63;
  uint32_t* const stage  = s_stage[threadIdx.x >> 6];
  int64_t const wave     = wave_of_block();
  int64_t const begin    = wave * a.chunk;
  int64_t const end      = a.nrows < begin + a.chunk ? a.nrows : begin + a.chunk;
  if (begin >= end) return;  // (no workgroup barrier below)
  for (int j = lane; j < STAGE_WORDS; j += 64) stage[j] = 0;
  wave_lds_sync();
  int const ncols          = a.ncols;
  int64_t const out_words  = static_cast<int64_t>((a.out_rows + 31) >> 5);
  uint64_t base            = gload(a.counts + wave);
  int64_t const w_end      = (end + 63) >> 6;
  for (int64_t w0 = begin >> 6; w0 < w_end; w0 += 64) {
    uint64_t const sel = w0 + lane < w_end ? gload(a.mask + w0 + lane) : 0;
    uint32_t const c   = __popcll(sel);
    uint32_t inc       = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      uint32_t const t = __shfl_up(inc, o);
      if (lane >= o) inc += t;
    }
    uint32_t const total = __shfl(inc, 63);
    if (total == 0) continue;  // (uniform)
    uint32_t const at    = static_cast<uint32_t>(base & 31) + (inc - c);  // the lane's first bit in the stage
    int const nwords     = static_cast<int>((static_cast<uint32_t>(base & 31) + total + 31) >> 5);  // <= 129
    int64_t const first  = static_cast<int64_t>(base >> 5);
    for (int k = 0; k < ncols; ++k) {
      validity_col const col = a.col[k];
      uint64_t bits          = 0;
      if (sel != 0) {
        uint64_t const val = funnel64(col.src, col.offset + (w0 + lane) * 64, (col.offset + a.nrows - 1) >> 5);
        bits               = sel == ~uint64_t{0} ? val : compress64(val, sel);
      }
      if (bits != 0) {  // (only words that receive a bit are touched: at most bit 31 + 4096 of the stage, word 128)
        uint32_t const i  = at >> 5;
        uint32_t const sh = at & 31;
        uint64_t const lo = bits << sh;
        uint32_t const p0 = static_cast<uint32_t>(lo), p1 = static_cast<uint32_t>(lo >> 32);
        uint32_t const p2 = sh != 0 ? static_cast<uint32_t>(bits >> (64 - sh)) : 0u;
        if (p0 != 0) atomicOr(stage + i, p0);
        if (p1 != 0) atomicOr(stage + i + 1, p1);
        if (p2 != 0) atomicOr(stage + i + 2, p2);
      }
      wave_lds_sync();  // the ORs before the read-back
      uint32_t nvalid = 0;
      for (int j = lane; j < nwords; j += 64) {
        uint32_t const v = stage[j];
        stage[j]         = 0;
        nvalid += __popc(v);
        if (first + j >= out_words) continue;  // (never: the range ends below out_rows)
        if (j == 0 || j == nwords - 1) {
          if (v != 0) global_or(col.dst + first + j, v);
        } else {
          gstore(col.dst + first + j, v);
        }
      }
      wave_lds_sync();  // the cleared words before the next column's ORs
      nvalid = wave_sum(nvalid);
      if (lane == 0 && nvalid != 0) global_add(col.valid, static_cast<unsigned long long>(nvalid));
    }
    base += total;
  }
}

template <typename T>
__global__ void k_store(T v, T* dst)
{
  *dst = v;
}

dim3 grid_of(int32_t nwaves) { return dim3(static_cast<unsigned>((nwaves + THREADS / 64 - 1) / (THREADS / 64))); }

}  // namespace

void launch_select_bool(bool_args const& a, bool deletion, hipStream_t stream)
{
  cudf::detail::prof::scope prof_{"copy_if_select_bool", stream};
  if (deletion) hipLaunchKernelGGL(k_select_bool<true>, grid_of(a.nwaves), dim3(THREADS), 0, stream, a);
  else hipLaunchKernelGGL(k_select_bool<false>, grid_of(a.nwaves), dim3(THREADS), 0, stream, a);
  CUDF_HIP_TRY(hipGetLastError());
}

void launch_select_valid_words(valid_args const& a, hipStream_t stream)
{
  CUDF_EXPECTS(a.chunk % 512 == 0 && a.need == a.nkeys, "copy_if: the word-wise selection takes whole words and every key");
  cudf::detail::prof::scope prof_{"copy_if_select_valid_words", stream};
  hipLaunchKernelGGL(k_select_valid_words, grid_of(a.nwaves), dim3(THREADS), 0, stream, a);
  CUDF_HIP_TRY(hipGetLastError());
}

void launch_select_valid_count(valid_args const& a, hipStream_t stream)
{
  cudf::detail::prof::scope prof_{"copy_if_select_valid_count", stream};
  hipLaunchKernelGGL(k_select_valid_count, grid_of(a.nwaves), dim3(THREADS), 0, stream, a);
  CUDF_HIP_TRY(hipGetLastError());
}

void launch_select_nan(nan_args const& a, hipStream_t stream)
{
  cudf::detail::prof::scope prof_{"copy_if_select_nan", stream};
  hipLaunchKernelGGL(k_select_nan, grid_of(a.nwaves), dim3(THREADS), 0, stream, a);
  CUDF_HIP_TRY(hipGetLastError());
}

void launch_select_unique(unique_args const& a, keep k, hipStream_t stream)
{
  cudf::detail::prof::scope prof_{"copy_if_select_unique", stream};
  switch (k) {
    case keep::first: hipLaunchKernelGGL(k_select_unique<0>, grid_of(a.nwaves), dim3(THREADS), 0, stream, a); break;
    case keep::last: hipLaunchKernelGGL(k_select_unique<1>, grid_of(a.nwaves), dim3(THREADS), 0, stream, a); break;
    case keep::none: hipLaunchKernelGGL(k_select_unique<2>, grid_of(a.nwaves), dim3(THREADS), 0, stream, a); break;
  }
  CUDF_HIP_TRY(hipGetLastError());
}

void launch_select_unique_column(unique_column_args const& a, hipStream_t stream)
{
  cudf::detail::prof::scope prof_{"copy_if_select_unique_column", stream};
  hipLaunchKernelGGL(k_select_unique_column, grid_of(a.nwaves), dim3(THREADS), 0, stream, a);
  CUDF_HIP_TRY(hipGetLastError());
}

void launch_copy_if_data(data_args const& a, data_args* d_args, hipStream_t stream)
{
  CUDF_EXPECTS(a.ncols >= 1 && a.ncols <= DATA_COLS, "copy_if: a data batch holds 1 to 4 columns");
  hipLaunchKernelGGL(k_store<data_args>, dim3(1), dim3(1), 0, stream, a, d_args);
  cudf::detail::prof::scope prof_{"copy_if_data", stream};
  hipLaunchKernelGGL(k_copy_if_data, grid_of(a.nwaves), dim3(THREADS), 0, stream, d_args);
  CUDF_HIP_TRY(hipGetLastError());
}

void launch_copy_if_validity(validity_args const& a, validity_args* d_args, hipStream_t stream)
{
  CUDF_EXPECTS(a.ncols >= 1 && a.ncols <= VALIDITY_COLS, "copy_if: a validity batch holds 1 to 16 columns");
  hipLaunchKernelGGL(k_store<validity_args>, dim3(1), dim3(1), 0, stream, a, d_args);
  cudf::detail::prof::scope prof_{"copy_if_validity", stream};
  hipLaunchKernelGGL(k_copy_if_validity, grid_of(a.nwaves), dim3(THREADS), 0, stream, d_args);
  CUDF_HIP_TRY(hipGetLastError());
}

}  // namespace cudf::detail::copy_if
