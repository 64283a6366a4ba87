// SPDX-License-Identifier: Apache-2.0
// gfx950 kernels of cudf::distinct (distinct_impl.hpp): the dense and set builds that leave one state word per set of equal rows,
// the sweep of those words into one bit per surviving row, and the per-chunk counts of that mask for the ordered compaction
// (rowset::compaction). Replaces the reference's cuco::static_set / static_map with a reduction of row indices per key and the copy_if that
// follows (cpp/src/stream_compaction/distinct_helpers.cu, distinct.cu, stable_distinct.cu; reductions/distinct_count.cu).
#include "distinct_impl.hpp"
#include "../common/profiler.hpp"
#include "../common/row_set.hpp"

namespace cudf::detail::distinct {
namespace {

using namespace rowset;

constexpr int THREADS     = 256;
constexpr int LDS_THREADS = 1024;
// `range` state words of LDS (launch_dense_build allocates exactly range words), within the 64 KiB of dynamic LDS a kernel gets
// without opting in
constexpr uint64_t LDS_ENTRIES_MAX = 16383;

constexpr int ANY = static_cast<int>(mode::any), FIRST = static_cast<int>(mode::first), LAST = static_cast<int>(mode::last),
              NONE = static_cast<int>(mode::none), COUNT = static_cast<int>(mode::count);

// The value a row contributes to a state word. Every mode but KEEP_NONE keeps the SMALLEST value (atomicMin, STATE_EMPTY is the
// largest): the row itself, or for KEEP_LAST 0x7fffffff - row, so that the last row has the smallest value.
template <int MODE>
__device__ __forceinline__ uint32_t encode(int64_t row)
{
  return MODE == LAST ? 0x7fffffffu - static_cast<uint32_t>(row) : static_cast<uint32_t>(row);
}
template <int MODE>
__device__ __forceinline__ uint32_t decode(uint32_t v)
{
  return MODE == LAST ? 0x7fffffffu - v : v;
}

// Folds v (an encoded row, or STATE_MULTI from a partial KEEP_NONE word) into state word *p, in LDS or HBM. True when *p was empty.
template <int MODE>
__device__ __forceinline__ bool apply(uint32_t* p, uint32_t v)
{
  if constexpr (MODE == NONE) {
    if (v == STATE_MULTI) return atomicExch(p, STATE_MULTI) == STATE_EMPTY;
    uint32_t const old = atomicCAS(p, STATE_EMPTY, v);
    if (old == STATE_EMPTY) return true;
    if (old != STATE_MULTI) atomicExch(p, STATE_MULTI);  // a second row: MULTI absorbs every later write
    return false;
  } else {
    return atomicMin(p, v) == STATE_EMPTY;
  }
}

// apply() on a word in HBM. Words only move towards the rule's answer (smaller, or MULTI), so when a read, stale or not, already
// shows a value the update could not improve, the atomic is skipped: most rows of a repeated key pay a read, not an atomic.
template <int MODE>
__device__ __forceinline__ bool apply_global(uint32_t* p, uint32_t v)
{
  uint32_t const cur = gload(p);
  if (MODE == NONE ? cur == STATE_MULTI : cur <= v) return false;  // (cur <= v < STATE_EMPTY: not empty)
  return apply<MODE>(p, v);
}

// The same fold of two partial words held in registers.
template <int MODE>
__device__ __forceinline__ uint32_t combine(uint32_t acc, uint32_t v)
{
  if (v == STATE_EMPTY) return acc;
  if (acc == STATE_EMPTY) return v;
  return MODE == NONE ? STATE_MULTI : (v < acc ? v : acc);
}

// The wave's partial word of the 64 rows [base, base + 64) whose bits are set in b.
template <int MODE>
__device__ __forceinline__ uint32_t wave_word(uint64_t b, int64_t base)
{
  if (b == 0) return STATE_EMPTY;
  if (MODE == NONE && __popcll(b) > 1) return STATE_MULTI;
  return MODE == LAST ? encode<MODE>(base + 63 - __clzll(b)) : encode<MODE>(base + __ffsll(static_cast<long long>(b)) - 1);
}

// The rows that bypass the table mark themselves (b: the wave's ballot of them; this lane's row is base + lane).
__device__ __forceinline__ void bypass_bits(build_args const& a, uint64_t b, int64_t base, int lane, unsigned& cnt)
{
  if (b == 0) return;
  if (a.flags != nullptr && ((b >> lane) & 1)) gstore(a.flags + base + lane, uint8_t{1});
  if (lane == 0) cnt += __popcll(b);
}

// End of a build kernel: the wave's partial words of the two special keys, its count and its NaN flag.
template <int MODE>
__device__ __forceinline__ void finish_wave(build_args const& a, uint32_t const sp[2], unsigned cnt, bool nan_seen, int lane)
{
  for (int k = 0; k < 2; ++k)
    if (sp[k] != STATE_EMPTY && lane == 0 && apply_global<MODE>(a.special + k, sp[k])) ++cnt;
  if (MODE == COUNT) {
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0 && cnt != 0) atomicAdd(a.counter, static_cast<unsigned long long>(cnt));
  }
  if (__any(nan_seen) && lane == 0) atomicOr(a.counter + 1, 1ull);
}

__device__ __forceinline__ bool is_nan_bits(uint64_t bits, int32_t cls)
{
  if (cls == CLS_F32) return (static_cast<uint32_t>(bits) & 0x7fffffffu) > 0x7f800000u;
  if (cls == CLS_F64) return (bits & 0x7fffffffffffffffull) > 0x7ff0000000000000ull;
  return false;
}

__device__ __forceinline__ bool row_has_nan(device_table const& t, int64_t i)
{
  for (int c = 0; c < t.ncols; ++c) {
    int32_t const cls = t.col[c].cls;
    if ((cls == CLS_F32 || cls == CLS_F64) && col_is_valid(t.col[c], i) && is_nan_bits(col_load_bits(t.col[c], i), cls)) return true;
  }
  return false;
}

// Rows are taken in 64-row groups, one group per wave and iteration (base is wave-uniform, so ballots see every lane).
#define DISTINCT_ROW_LOOP(a)                                                                                   \
  int const lane       = threadIdx.x & 63;                                                                     \
  int64_t const stride = static_cast<int64_t>(gridDim.x) * blockDim.x;                                        \
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * blockDim.x + (threadIdx.x - lane); base < (a).nrows; \
       base += stride)

// ------------------------------------------------------------------ dense
// LDS: the workgroup reduces its rows into an LDS copy of the range first, then merges the words it touched into HBM.
template <int W, bool SIGNED, int MODE, bool LDS>
__global__ void __launch_bounds__(LDS ? LDS_THREADS : THREADS) k_dense_build(build_args a)
{
  extern __shared__ uint32_t s_state[];
  if constexpr (LDS) {
    for (uint64_t e = threadIdx.x; e < a.range; e += blockDim.x) s_state[e] = STATE_EMPTY;
    __syncthreads();
  }
  device_column const& c = a.keys.col[0];
  uint32_t sp[2]         = {STATE_EMPTY, STATE_EMPTY};
  unsigned cnt           = 0;
  DISTINCT_ROW_LOOP(a)
  {
    int64_t const i   = base + lane;
    bool const active = i < a.nrows;
    bool const valid  = active && col_is_valid(c, i);
    if (valid) {
      uint64_t const off = load_int<W, SIGNED>(c, i) - a.lo;  // < range: lo and range cover every valid key
      if constexpr (LDS) apply<MODE>(s_state + off, encode<MODE>(i));
      else if constexpr (MODE == ANY) {
        // any row of the set serves: store into an empty word, no atomic (racing stores leave one of their rows)
        if (gload(a.state + off) == STATE_EMPTY) gstore(a.state + off, encode<MODE>(i));
      } else if (apply_global<MODE>(a.state + off, encode<MODE>(i)) && MODE == COUNT) ++cnt;
    }
    uint64_t const nulls = __ballot(active && !valid);
    if (a.nulls_equal) sp[0] = combine<MODE>(sp[0], wave_word<MODE>(nulls, base));
    else bypass_bits(a, nulls, base, lane, cnt);
  }
  if constexpr (LDS) {
    __syncthreads();
    for (uint64_t e = threadIdx.x; e < a.range; e += blockDim.x) {
      uint32_t const v = s_state[e];
      if (v != STATE_EMPTY && apply_global<MODE>(a.state + e, v) && MODE == COUNT) ++cnt;
    }
  }
  finish_wave<MODE>(a, sp, cnt, false, threadIdx.x & 63);
}

// ------------------------------------------------------------------ set, inline key
template <int W, int MODE>
__global__ void __launch_bounds__(THREADS) k_set_build_inline(build_args a)
{
  device_column const& c = a.keys.col[0];
  uint32_t sp[2]         = {STATE_EMPTY, STATE_EMPTY};
  unsigned cnt           = 0;
  bool nan_seen          = false;
  DISTINCT_ROW_LOOP(a)
  {
    int64_t const i     = base + lane;
    bool const active   = i < a.nrows;
    bool const valid    = active && col_is_valid(c, i);
    uint64_t const raw  = valid ? load_bits<W>(c, i) : 0;
    bool const nan      = valid && is_nan_bits(raw, c.cls);
    uint64_t const key  = normalize_key_bits(raw, c.cls);
    nan_seen |= nan;
    bool const bypass   = (active && !valid && !a.nulls_equal) || (nan && !a.nans_equal);
    bool const sentinel = valid && !bypass && key == EMPTY;  // (8-byte keys only) the one value a slot cannot hold
    if (valid && !bypass && !sentinel) {
      auto const got = claim(a.slots, a.slot_stride, a.capacity, home_slot(murmur3_32_bits(key, W, 0), a.capacity), key,
                             [&](uint64_t cur) { return cur == key; });
      if constexpr (MODE == COUNT) {
        cnt += got.inserted ? 1u : 0u;
      } else {
        // the record's two words: st[0] is written once, by the row whose CAS inserted the key (a plain store); st[1] folds the
        // other rows. A row that already sees a better st[0] does nothing (st[0] never changes once written).
        uint32_t* const st = a.state + got.slot * a.state_stride;
        uint32_t const v   = encode<MODE>(i);
        if (got.inserted) gstore(st, v);
        else if constexpr (MODE == NONE) {
          if (gload(st + 1) != STATE_MULTI) gstore(st + 1, STATE_MULTI);  // a second row: every store writes the same value
        } else if constexpr (MODE != ANY) {
          if (gload(st) > v) apply_global<MODE>(st + 1, v);
        }
      }
    }
    uint64_t const nulls = __ballot(active && !valid && a.nulls_equal);
    sp[0]                = combine<MODE>(sp[0], wave_word<MODE>(nulls, base));
    sp[1]                = combine<MODE>(sp[1], wave_word<MODE>(__ballot(sentinel), base));
    bypass_bits(a, __ballot(bypass), base, lane, cnt);
  }
  finish_wave<MODE>(a, sp, cnt, nan_seen, lane);
}

// ------------------------------------------------------------------ set, {row hash | row} slots
// The slot's row is the state: equal rows have equal hashes, so a 64-bit min / max over {hash | row} changes only the row.
template <int MODE>
__global__ void __launch_bounds__(THREADS) k_set_build_rows(build_args a)
{
  uint32_t const sp[2] = {STATE_EMPTY, STATE_EMPTY};
  unsigned cnt         = 0;
  bool nan_seen        = false;
  bool const eq        = a.nulls_equal != 0;
  DISTINCT_ROW_LOOP(a)
  {
    int64_t const i   = base + lane;
    bool const active = i < a.nrows;
    bool bypass       = false;
    if (active) {
      bool const nan = row_has_nan(a.keys, i);
      nan_seen |= nan;
      bypass = (!eq && row_has_null(a.keys, i)) || (nan && !a.nans_equal);
      if (!bypass) {
        uint32_t const h     = row_hash(a.keys, i, 0);
        uint64_t const entry = (static_cast<uint64_t>(h) << 32) | static_cast<uint32_t>(i);
        auto const got       = claim(a.slots, 1, a.capacity, home_slot(h, a.capacity), entry, [&](uint64_t cur) {
          return (cur >> 32) == h && rows_equal(a.keys, static_cast<uint32_t>(cur) & 0x7fffffffu, a.keys, i, eq);  // (less ROW_MULTI)
        });
        auto* const p        = reinterpret_cast<unsigned long long*>(a.slots + got.slot);
        if (got.inserted) {
          if (MODE == COUNT) ++cnt;
        } else if constexpr (MODE == FIRST) atomicMin(p, static_cast<unsigned long long>(entry));
        else if constexpr (MODE == LAST) atomicMax(p, static_cast<unsigned long long>(entry));
        else if constexpr (MODE == NONE) {
          if (!(got.cur & ROW_MULTI)) atomicOr(p, static_cast<unsigned long long>(ROW_MULTI));
        }
      }
    }
    bypass_bits(a, __ballot(bypass), base, lane, cnt);
  }
  finish_wave<MODE>(a, sp, cnt, nan_seen, lane);
}

// ------------------------------------------------------------------ sweep: survivors -> flag bytes
// A surviving row is named by one state word (or slot) only, so a plain byte store marks it; no atomic.
__device__ __forceinline__ void set_bit(uint8_t* flags, uint32_t row) { gstore(flags + row, uint8_t{1}); }

template <int MODE, bool ROW_SLOTS>
__global__ void __launch_bounds__(THREADS) k_sweep(build_args a, uint64_t entries)
{
  uint64_t const stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
  for (uint64_t e = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < entries; e += stride) {
    if constexpr (ROW_SLOTS) {
      uint64_t const cur = gload(a.slots + e);
      if (cur == EMPTY || (MODE == NONE && (cur & ROW_MULTI))) continue;
      set_bit(a.flags, static_cast<uint32_t>(cur) & 0x7fffffffu);
    } else {
      uint32_t v = gload(a.state + e * a.state_stride);
      if (a.slot_stride == 2) {  // an inline record: {inserting row's word, the other rows' word}
        uint32_t const w = gload(a.state + e * a.state_stride + 1);
        v                = MODE == NONE ? (w == STATE_EMPTY ? v : STATE_MULTI) : (w < v ? w : v);
      }
      if (v <= 0x7fffffffu) set_bit(a.flags, decode<MODE>(v));  // (STATE_EMPTY, STATE_MULTI: no survivor)
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < 2) {
    uint32_t const v = gload(a.special + threadIdx.x);
    if (v <= 0x7fffffffu) set_bit(a.flags, decode<MODE>(v));
  }
}

// ------------------------------------------------------------------ pack: flag bytes -> mask words + per-chunk counts
// One wave per chunk (a multiple of 512 rows, so a mask word never spans two chunks): 8 rows per lane per step, read as one 8-byte
// word (chunks start at multiples of 512 bytes), so a step covers 512 rows; the ballot of each byte position is a mask word.
__global__ void __launch_bounds__(THREADS) k_pack(uint8_t const* flags, uint64_t* mask, int64_t nrows, int64_t chunk, int32_t nwaves,
                                                  unsigned long long* counts)
{
  int const lane     = threadIdx.x & 63;
  int64_t const wave = static_cast<int64_t>(blockIdx.x) * (THREADS / 64) + (threadIdx.x >> 6);
  if (wave >= nwaves) return;
  int64_t const begin = wave * chunk;
  int64_t const end   = nrows < begin + chunk ? nrows : begin + chunk;
  unsigned long long n = 0;
  for (int64_t r0 = begin; r0 < end; r0 += 512) {
    int64_t const r = r0 + 8 * lane;  // this lane's 8 rows
    uint64_t bytes  = 0;
    if (r + 8 <= end) bytes = gload(reinterpret_cast<uint64_t const*>(flags + r));
    else
      for (int j = 0; j < 8 && r + j < end; ++j) bytes |= static_cast<uint64_t>(gload(flags + r + j)) << (8 * j);
    // rows r0 + 64 * k + lane for k = 0..7 are byte (lane & 7) of lane 8 * k + (lane >> 3)
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      uint64_t const src = __shfl(bytes, 8 * k + (lane >> 3));
      uint64_t const m   = __ballot(((src >> (8 * (lane & 7))) & 0xff) != 0 && r0 + 64 * k + lane < end);
      if (r0 + 64 * k < end) {
        if (lane == 0) gstore(mask + ((r0 + 64 * k) >> 6), m);
        n += __popcll(m);
      }
    }
  }
  if (lane == 0) gstore(counts + wave, n);
}

template <typename F>
void dispatch_mode(int32_t m, F&& f)
{
  switch (m) {
    case ANY: return f.template operator()<ANY>();
    case FIRST: return f.template operator()<FIRST>();
    case LAST: return f.template operator()<LAST>();
    case NONE: return f.template operator()<NONE>();
    case COUNT: return f.template operator()<COUNT>();
    default: CUDF_FAIL("distinct: unknown keep mode");
  }
}

}  // namespace

uint64_t lds_entries_max() { return LDS_ENTRIES_MAX; }

void launch_dense_build(build_args const& a, uint64_t lds_entries, hipStream_t stream)
{
  device_column const& c = a.keys.col[0];
  bool const lds         = lds_entries > 0;
  CUDF_EXPECTS(!lds || (a.range <= lds_entries && a.range <= LDS_ENTRIES_MAX), "distinct: range exceeds the LDS build");
  cudf::detail::prof::scope prof_{lds ? "distinct_dense_lds_build" : "distinct_dense_build", stream};
  dispatch_int(c.width, c.cls == CLS_SINT, [&]<int W, bool S>() {
    dispatch_mode(a.mode, [&]<int M>() {
      if (lds) {
        // enough rows per workgroup that the merge of its words (at most `range`) stays small against its rows
        int64_t const per_block = std::max<int64_t>(16 * static_cast<int64_t>(a.range), 16 * LDS_THREADS);
        auto const grid = static_cast<unsigned>(std::clamp<int64_t>((a.nrows + per_block - 1) / per_block, 1, 1024));
        hipLaunchKernelGGL((k_dense_build<W, S, M, true>), dim3(grid), dim3(LDS_THREADS),
                           static_cast<std::size_t>(std::max<uint64_t>(a.range, 1)) * sizeof(uint32_t), stream, a);
      } else {
        hipLaunchKernelGGL((k_dense_build<W, S, M, false>), dim3(grid_for(a.nrows, THREADS)), dim3(THREADS), 0, stream, a);
      }
    });
  });
  CUDF_HIP_TRY(hipGetLastError());
}

void launch_set_build(build_args const& a, hipStream_t stream)
{
  unsigned const grid = grid_for(a.nrows, THREADS);
  if (a.inline_key) {
    cudf::detail::prof::scope prof_{"distinct_set_build_inline", stream};
    dispatch_mode(a.mode, [&]<int M>() {
      if (a.keys.col[0].width == 4) hipLaunchKernelGGL((k_set_build_inline<4, M>), dim3(grid), dim3(THREADS), 0, stream, a);
      else hipLaunchKernelGGL((k_set_build_inline<8, M>), dim3(grid), dim3(THREADS), 0, stream, a);
    });
  } else {
    cudf::detail::prof::scope prof_{"distinct_set_build_rows", stream};
    dispatch_mode(a.mode, [&]<int M>() { hipLaunchKernelGGL((k_set_build_rows<M>), dim3(grid), dim3(THREADS), 0, stream, a); });
  }
  CUDF_HIP_TRY(hipGetLastError());
}

void launch_sweep(build_args const& a, hipStream_t stream)
{
  CUDF_EXPECTS(a.mode != COUNT && a.flags != nullptr, "distinct: the sweep needs a keep mode and the flag bytes");
  cudf::detail::prof::scope prof_{"distinct_sweep", stream};
  bool const row_slots   = a.slots != nullptr && !a.inline_key;
  uint64_t const entries = a.slots != nullptr ? a.capacity : a.range;
  dispatch_mode(a.mode, [&]<int M>() {
    if constexpr (M != COUNT) {
      if (row_slots) hipLaunchKernelGGL((k_sweep<M, true>), dim3(grid_for(static_cast<int64_t>(entries), THREADS)), dim3(THREADS), 0, stream, a, entries);
      else hipLaunchKernelGGL((k_sweep<M, false>), dim3(grid_for(static_cast<int64_t>(entries), THREADS)), dim3(THREADS), 0, stream, a, entries);
    }
  });
  CUDF_HIP_TRY(hipGetLastError());
}

void launch_pack(uint8_t const* flags, uint64_t* mask, int64_t nrows, int64_t chunk, int32_t nwaves, unsigned long long* counts,
                 hipStream_t stream)
{
  CUDF_EXPECTS(chunk % 512 == 0, "distinct: pack chunks are whole 512-row steps");
  cudf::detail::prof::scope prof_{"distinct_pack", stream};
  hipLaunchKernelGGL(k_pack, dim3((nwaves + THREADS / 64 - 1) / (THREADS / 64)), dim3(THREADS), 0, stream, flags, mask, nrows, chunk,
                     nwaves, counts);
  CUDF_HIP_TRY(hipGetLastError());
}

}  // namespace cudf::detail::distinct
