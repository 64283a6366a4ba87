// SPDX-License-Identifier: Apache-2.0
// groupby::scan and groupby::replace_nulls on the sort-based groupby (reference cpp/src/groupby/groupby.cu scan / replace_nulls,
// sort/scan.cpp, group_scan_util.cuh, group_rank_scan.cu, group_replace_nulls.cu). The rows are put in group order by the sort
// helper (sort_helper.hpp) and every scan kind is answered by one segmented inclusive scan core:
//   k_seg_tile_carry  per tile of 2048 positions: does it hold a group boundary, and the aggregate of its trailing segment
//   k_seg_spine       one workgroup: segmented scan of those tile carries (each thread walks a run of tiles, then a block scan)
//   k_seg_apply       every tile again, scanned with the carry that flows into it
// No workgroup waits on another (no decoupled look-back), so a scan cannot hang behind a workgroup that is not resident. One
// pass serves all the scan kinds of a request (up to SG_KINDS at a time): each grouped value is read once and one result per kind
// is written. The values are gathered into group order once per request, and not at all when the key order is the identity.
// RANK scans run-start / run-end / valid words of the (label, value) order with the same core and scatter the ranks back into
// group order; replace_nulls scans the position of the last valid row, forward (PRECEDING) or backward (FOLLOWING), and gathers.
#include "sort_helper.hpp"
#include "../common/profiler.hpp"

#include <cudf/copying.hpp>
#include <cudf/groupby.hpp>
#include <cudf/null_mask.hpp>
#include <cudf/utilities/error.hpp>

#include <hip/hip_runtime.h>

#include <algorithm>

namespace cudf::groupby::detail {
namespace {
using cudf::detail::CLS_BOOL;
using cudf::detail::CLS_F32;
using cudf::detail::CLS_F64;
using cudf::detail::CLS_NONE;
using cudf::detail::CLS_SINT;
using cudf::detail::col_is_valid;
using cudf::detail::col_load_bits;
using cudf::detail::device_column;
using cudf::detail::gload;
using cudf::detail::gstore;
namespace prof = cudf::detail::prof;

constexpr int SG_THREADS = 256;
constexpr int SG_ITEMS   = 8;                        // consecutive positions per thread
constexpr int SG_TILE    = SG_THREADS * SG_ITEMS;    // positions per workgroup
constexpr int SG_SPINE   = 1024;                     // threads of the spine workgroup
constexpr int SG_KINDS   = 8;                        // scan kinds per fused pass

// the associative operator of a kind; every state is 64 bits
enum scan_op : int32_t { OP_ADD_I, OP_ADD_F32, OP_ADD_F64, OP_MUL_I, OP_MUL_F32, OP_MUL_F64, OP_MIN_U, OP_MAX_U };
// what a position contributes
enum scan_lift : int32_t {
  LIFT_INT,        // the value sign- or zero-extended to 64 bits (integer SUM / PRODUCT wrap as two's complement)
  LIFT_BITS,       // the value's bits (float SUM / PRODUCT)
  LIFT_ORDERED,    // order-preserving word of the value (MIN / MAX)
  LIFT_ONE,        // 1 (COUNT_ALL)
  LIFT_VALID,      // 1 for a valid value (COUNT_VALID)
  LIFT_VALID_POS,  // scan position + 1 of a valid value, else 0 (replace_nulls)
  LIFT_BIT0_POS,   // scan position + 1 where bit 0 of the word is set, else 0 (RANK: run starts)
  LIFT_BIT1_POS,   // the same for bit 1 (RANK: run ends, scanned backward)
  LIFT_BIT0,       // bit 0 of the word (RANK DENSE)
  LIFT_BIT2        // bit 2 of the word (RANK: valid values)
};

struct scan_kind {
  int32_t op;
  int32_t lift;   // LIFT_ORDERED results are decoded back to the value
  int32_t width;  // bytes per output element
  void* out;      // one element per position, indexed like the input
};

struct scan_src {
  device_column col;          // the values, read at the position itself when bits == nullptr (rows already in group order)
  uint64_t const* bits;       // the values gathered into group order, or one word per position (RANK)
  bitmask_type const* valid;  // validity per position; nullptr: every position valid
  int32_t const* labels;      // group of each position
  int64_t n;
  int32_t backward;           // scan from the last position to the first
  int32_t read_values;        // some kind reads the value (or word) of a position
  int32_t nkinds;
  scan_kind kind[SG_KINDS];
};

template <int OP>
__device__ __forceinline__ uint64_t identity_of()
{
  if constexpr (OP == OP_ADD_F32) return 0x80000000ull;  // -0.0f: -0 + x == x for every x, -0 included
  else if constexpr (OP == OP_ADD_F64) return 0x8000000000000000ull;
  else if constexpr (OP == OP_MUL_I) return 1;
  else if constexpr (OP == OP_MUL_F32) return 0x3f800000ull;
  else if constexpr (OP == OP_MUL_F64) return 0x3ff0000000000000ull;
  else if constexpr (OP == OP_MIN_U) return ~0ull;
  else return 0;
}

template <int OP>
__device__ __forceinline__ uint64_t op_of(uint64_t a, uint64_t b)
{
  if constexpr (OP == OP_ADD_I) return a + b;
  else if constexpr (OP == OP_ADD_F32)
    return __float_as_uint(__uint_as_float(static_cast<uint32_t>(a)) + __uint_as_float(static_cast<uint32_t>(b)));
  else if constexpr (OP == OP_ADD_F64)
    return static_cast<uint64_t>(__double_as_longlong(__longlong_as_double(static_cast<long long>(a)) + __longlong_as_double(static_cast<long long>(b))));
  else if constexpr (OP == OP_MUL_I) return a * b;
  else if constexpr (OP == OP_MUL_F32)
    return __float_as_uint(__uint_as_float(static_cast<uint32_t>(a)) * __uint_as_float(static_cast<uint32_t>(b)));
  else if constexpr (OP == OP_MUL_F64)
    return static_cast<uint64_t>(__double_as_longlong(__longlong_as_double(static_cast<long long>(a)) * __longlong_as_double(static_cast<long long>(b))));
  else if constexpr (OP == OP_MIN_U) return a < b ? a : b;
  else return a > b ? a : b;
}

// order-preserving word for MIN / MAX: signed integers with the sign bit flipped, floats by sign-magnitude with every NaN made the
// canonical quiet NaN (above +inf). Unlike the key words of the sort, -0 stays below +0, so the word is reversible.
__device__ __forceinline__ uint64_t ordered_word(uint64_t raw, int32_t cls, int32_t width)
{
  switch (cls) {
    case CLS_SINT: {
      int const sh = 64 - 8 * width;
      return static_cast<uint64_t>(static_cast<int64_t>(raw << sh) >> sh) ^ 0x8000000000000000ull;
    }
    case CLS_BOOL: return raw != 0;
    case CLS_F32: {
      uint32_t b = static_cast<uint32_t>(raw);
      if ((b & 0x7fffffffu) > 0x7f800000u) b = 0x7fc00000u;
      return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
    }
    case CLS_F64: {
      uint64_t b = raw;
      if ((b & 0x7fffffffffffffffull) > 0x7ff0000000000000ull) b = 0x7ff8000000000000ull;
      return b ^ ((b >> 63) ? 0xffffffffffffffffull : 0x8000000000000000ull);
    }
    default: return raw;
  }
}
__device__ __forceinline__ uint64_t from_ordered(uint64_t w, int32_t cls)
{
  switch (cls) {
    case CLS_SINT: return w ^ 0x8000000000000000ull;
    case CLS_F32: {
      uint32_t const x = static_cast<uint32_t>(w);
      return (x >> 31) ? (x ^ 0x80000000u) : ~x;
    }
    case CLS_F64: return (w >> 63) ? (w ^ 0x8000000000000000ull) : ~w;
    default: return w;
  }
}

template <int OP, int LIFT>
__device__ __forceinline__ uint64_t lift(device_column const& col, uint64_t raw, bool valid, int64_t j)
{
  if constexpr (LIFT == LIFT_INT) {
    if (!valid) return identity_of<OP>();
    if (col.cls == CLS_SINT) {
      int const sh = 64 - 8 * col.width;
      return static_cast<uint64_t>(static_cast<int64_t>(raw << sh) >> sh);
    }
    return col.cls == CLS_BOOL ? (raw != 0 ? 1 : 0) : raw;
  } else if constexpr (LIFT == LIFT_BITS) {
    return valid ? raw : identity_of<OP>();
  } else if constexpr (LIFT == LIFT_ORDERED) {
    return valid ? ordered_word(raw, col.cls, col.width) : identity_of<OP>();
  } else if constexpr (LIFT == LIFT_ONE) {
    return 1;
  } else if constexpr (LIFT == LIFT_VALID) {
    return valid ? 1 : 0;
  } else if constexpr (LIFT == LIFT_VALID_POS) {
    return valid ? static_cast<uint64_t>(j) + 1 : 0;
  } else if constexpr (LIFT == LIFT_BIT0_POS) {
    return (raw & 1) ? static_cast<uint64_t>(j) + 1 : 0;
  } else if constexpr (LIFT == LIFT_BIT1_POS) {
    return (raw & 2) ? static_cast<uint64_t>(j) + 1 : 0;
  } else if constexpr (LIFT == LIFT_BIT0) {
    return raw & 1;
  } else {
    return (raw >> 2) & 1;
  }
}

__device__ __forceinline__ void store_width(void* out, int64_t i, int32_t width, uint64_t v)
{
  switch (width) {
    case 1: gstore(static_cast<uint8_t*>(out) + i, static_cast<uint8_t>(v)); break;
    case 2: gstore(static_cast<uint16_t*>(out) + i, static_cast<uint16_t>(v)); break;
    case 4: gstore(static_cast<uint32_t*>(out) + i, static_cast<uint32_t>(v)); break;
    default: gstore(static_cast<uint64_t*>(out) + i, v);
  }
}

__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, int o)
{
  uint32_t const lo = __shfl_up(static_cast<uint32_t>(v), o, 64);
  uint32_t const hi = __shfl_up(static_cast<uint32_t>(v >> 32), o, 64);
  return (static_cast<uint64_t>(hi) << 32) | lo;
}

// segmented scan over the workgroup's threads of (value, holds-a-boundary) pairs, where (a, fa) then (b, fb) combine to
// (fb ? b : a op b, fa | fb). ev / ef: what the threads before this one combine to (ef false and ev the identity for thread 0);
// tv: all threads combined.
template <int OP, int THREADS>
__device__ __forceinline__ void block_seg_scan(uint64_t v, bool f, uint64_t& ev, bool& ef, uint64_t& tv, uint64_t* sv, uint32_t* sf)
{
  int const lane = threadIdx.x & 63;
  int const w    = threadIdx.x >> 6;
  uint64_t iv    = v;
  bool ifl       = f;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    uint64_t const ov = shfl_up64(iv, o);
    bool const of     = __shfl_up(static_cast<int>(ifl), o, 64) != 0;
    if (lane >= o) {
      if (!ifl) iv = op_of<OP>(ov, iv);
      ifl = ifl || of;
    }
  }
  uint64_t xv = shfl_up64(iv, 1);
  bool xf     = __shfl_up(static_cast<int>(ifl), 1, 64) != 0;
  if (lane == 0) {
    xv = identity_of<OP>();
    xf = false;
  }
  __syncthreads();  // sv / sf may still be read from the previous use
  if (lane == 63) {
    sv[w] = iv;
    sf[w] = ifl;
  }
  __syncthreads();
  uint64_t pv = identity_of<OP>(), all = identity_of<OP>();
  bool pf = false;
#pragma unroll
  for (int i = 0; i < THREADS / 64; ++i) {
    uint64_t const s = sv[i];
    bool const sfl   = sf[i] != 0;
    if (i < w) {
      pv = sfl ? s : op_of<OP>(pv, s);
      pf = pf || sfl;
    }
    all = sfl ? s : op_of<OP>(all, s);
  }
  ev = xf ? xv : op_of<OP>(pv, xv);
  ef = xf || pf;
  tv = all;
}

// A tile passes through LDS both ways: the workgroup reads it coalesced (consecutive lanes, consecutive positions) and each thread
// then takes SG_ITEMS consecutive positions from LDS for its sequential part of the scan; results go back through LDS and leave
// coalesced, instead of 64 lanes each reading and writing a run of its own.
constexpr int SG_PAD_TILE = SG_TILE + SG_TILE / 16;
__device__ __forceinline__ int padded(int e) { return e + (e >> 4); }  // one spare slot per 16: the thread-run reads miss bank clashes

struct tile_lds {
  uint64_t v[SG_PAD_TILE];   // the tile's values (or words) in scan order, later one kind's results
  int32_t lab[SG_TILE + 1];  // labels of scan positions base - 1 .. base + SG_TILE - 1
  uint8_t valid[SG_TILE];
};

// the positions of one thread: values (or words), validity and segment starts
struct thread_items {
  uint64_t raw[SG_ITEMS];
  uint32_t valid;  // bit r: position r valid
  uint32_t start;  // bit r: position r starts a group (in scan direction)
  uint32_t live;   // bit r: position r < n
};

__device__ __forceinline__ int64_t physical(scan_src const& src, int64_t j) { return src.backward ? src.n - 1 - j : j; }

// the workgroup's tile into LDS (coalesced), then this thread's SG_ITEMS consecutive positions out of it
__device__ __forceinline__ void load_items(scan_src const& src, int64_t base, tile_lds& L, thread_items& t)
{
#pragma unroll 4
  for (int r = 0; r < SG_ITEMS; ++r) {
    int const e     = r * SG_THREADS + threadIdx.x;
    int64_t const j = base + e;
    if (j < src.n) {
      int64_t const p = physical(src, j);
      if (src.read_values) L.v[padded(e)] = src.bits ? gload(src.bits + p) : col_load_bits(src.col, p);
      L.valid[e]  = src.valid == nullptr || ((gload(src.valid + (p >> 5)) >> (p & 31)) & 1u);
      L.lab[e + 1] = gload(src.labels + p);
    }
  }
  if (threadIdx.x == 0) L.lab[0] = base > 0 ? gload(src.labels + physical(src, base - 1)) : -1;
  __syncthreads();
  t.valid = t.start = t.live = 0;
  int const first = threadIdx.x * SG_ITEMS;
#pragma unroll
  for (int r = 0; r < SG_ITEMS; ++r) {
    int const e = first + r;
    t.raw[r]    = 0;
    if (base + e < src.n) {
      if (src.read_values) t.raw[r] = L.v[padded(e)];
      t.valid |= static_cast<uint32_t>(L.valid[e]) << r;
      t.start |= static_cast<uint32_t>(base + e == 0 || L.lab[e + 1] != L.lab[e]) << r;
      t.live |= 1u << r;
    }
  }
}

// the thread's own (trailing segment aggregate, holds a boundary)
template <int OP, int LIFT>
__device__ __forceinline__ uint64_t thread_aggregate(scan_src const& src, thread_items const& t, int64_t first)
{
  uint64_t acc = identity_of<OP>();
#pragma unroll
  for (int r = 0; r < SG_ITEMS; ++r) {
    if (!((t.live >> r) & 1u)) continue;
    uint64_t const x = lift<OP, LIFT>(src.col, t.raw[r], (t.valid >> r) & 1u, first + r);
    acc              = ((t.start >> r) & 1u) ? x : op_of<OP>(acc, x);
  }
  return acc;
}

template <int OP, int LIFT>
__device__ void tile_carry_kind(scan_src const& src, scan_kind const& kd, int k, thread_items const& t, int64_t first, uint64_t* tile_val,
                                int64_t tiles, uint64_t* sv, uint32_t* sf)
{
  uint64_t const acc = thread_aggregate<OP, LIFT>(src, t, first);
  uint64_t ev, tv;
  bool ef;
  block_seg_scan<OP, SG_THREADS>(acc, t.start != 0, ev, ef, tv, sv, sf);
  if (threadIdx.x == 0) tile_val[static_cast<int64_t>(k) * tiles + blockIdx.x] = tv;
}

// (not inlined: fifteen inlined (operator, lift) bodies in one kernel took 256 VGPRs and spilled; one call per kind and tile costs
// less than that)
template <int OP, int LIFT>
__device__ __noinline__ void apply_kind(scan_src const& src, scan_kind const& kd, thread_items const& t, int64_t base, uint64_t carry, tile_lds& L,
                           uint64_t* sv, uint32_t* sf)
{
  int const first     = threadIdx.x * SG_ITEMS;
  uint64_t const acc  = thread_aggregate<OP, LIFT>(src, t, base + first);
  uint64_t ev, tv;
  bool ef;
  block_seg_scan<OP, SG_THREADS>(acc, t.start != 0, ev, ef, tv, sv, sf);  // (its barriers also end the previous kind's stores)
  uint64_t run = ef ? ev : op_of<OP>(carry, ev);
#pragma unroll
  for (int r = 0; r < SG_ITEMS; ++r) {
    if (!((t.live >> r) & 1u)) continue;
    uint64_t const x = lift<OP, LIFT>(src.col, t.raw[r], (t.valid >> r) & 1u, base + first + r);
    run              = ((t.start >> r) & 1u) ? x : op_of<OP>(run, x);
    L.v[padded(first + r)] = run;
  }
  __syncthreads();
#pragma unroll 4
  for (int r = 0; r < SG_ITEMS; ++r) {
    int const e     = r * SG_THREADS + threadIdx.x;
    int64_t const j = base + e;
    if (j < src.n) {
      uint64_t const v = L.v[padded(e)];
      store_width(kd.out, physical(src, j), kd.width, LIFT == LIFT_ORDERED ? from_ordered(v, src.col.cls) : v);
    }
  }
}

// the kinds into LDS with constant indices: indexing the kernel argument's array by a runtime k would copy the whole argument into
// scratch memory, per lane
__device__ __forceinline__ void stage_kinds(scan_src const& src, scan_kind* sk)
{
#pragma unroll
  for (int i = 0; i < SG_KINDS; ++i)
    if (threadIdx.x == i) sk[i] = src.kind[i];
  __syncthreads();
}

// the (operator, lift) pairs the host builds, one instantiation each: a runtime lift inside the item loops made the compiler
// evaluate every lift of every item and select (256 VGPRs and scratch spills)
#define SG_PAIR(fn, o, l, ...) \
  case (o) * 16 + (l): fn<o, l>(__VA_ARGS__); break;
#define SG_DISPATCH(kd, fn, ...)                                                                                                 \
  switch ((kd).op * 16 + (kd).lift) {                                                                                            \
    SG_PAIR(fn, OP_ADD_I, LIFT_INT, __VA_ARGS__) SG_PAIR(fn, OP_ADD_I, LIFT_ONE, __VA_ARGS__)                                    \
    SG_PAIR(fn, OP_ADD_I, LIFT_VALID, __VA_ARGS__) SG_PAIR(fn, OP_ADD_I, LIFT_BIT0, __VA_ARGS__)                                 \
    SG_PAIR(fn, OP_ADD_I, LIFT_BIT2, __VA_ARGS__) SG_PAIR(fn, OP_ADD_F32, LIFT_BITS, __VA_ARGS__)                                \
    SG_PAIR(fn, OP_ADD_F64, LIFT_BITS, __VA_ARGS__) SG_PAIR(fn, OP_MUL_I, LIFT_INT, __VA_ARGS__)                                 \
    SG_PAIR(fn, OP_MUL_F32, LIFT_BITS, __VA_ARGS__) SG_PAIR(fn, OP_MUL_F64, LIFT_BITS, __VA_ARGS__)                              \
    SG_PAIR(fn, OP_MIN_U, LIFT_ORDERED, __VA_ARGS__) SG_PAIR(fn, OP_MAX_U, LIFT_ORDERED, __VA_ARGS__)                            \
    SG_PAIR(fn, OP_MAX_U, LIFT_VALID_POS, __VA_ARGS__) SG_PAIR(fn, OP_MAX_U, LIFT_BIT0_POS, __VA_ARGS__)                         \
    SG_PAIR(fn, OP_MAX_U, LIFT_BIT1_POS, __VA_ARGS__)                                                                            \
    default: __builtin_trap();                                                                                                   \
  }
#define SG_DISPATCH_OP(op, fn, ...)                        \
  switch (op) {                                            \
    case OP_ADD_I: fn<OP_ADD_I>(__VA_ARGS__); break;       \
    case OP_ADD_F32: fn<OP_ADD_F32>(__VA_ARGS__); break;   \
    case OP_ADD_F64: fn<OP_ADD_F64>(__VA_ARGS__); break;   \
    case OP_MUL_I: fn<OP_MUL_I>(__VA_ARGS__); break;       \
    case OP_MUL_F32: fn<OP_MUL_F32>(__VA_ARGS__); break;   \
    case OP_MUL_F64: fn<OP_MUL_F64>(__VA_ARGS__); break;   \
    case OP_MIN_U: fn<OP_MIN_U>(__VA_ARGS__); break;       \
    default: fn<OP_MAX_U>(__VA_ARGS__); break;             \
  }

// tile_val[k * tiles + tile] = aggregate of the tile's trailing segment for kind k; tile_flag[tile] = the tile holds a group start
__global__ void __launch_bounds__(SG_THREADS) k_seg_tile_carry(scan_src src, uint64_t* tile_val, uint32_t* tile_flag, int64_t tiles)
{
  __shared__ uint64_t sv[SG_THREADS / 64];
  __shared__ uint32_t sf[SG_THREADS / 64];
  __shared__ tile_lds L;
  __shared__ scan_kind sk[SG_KINDS];
  stage_kinds(src, sk);
  int64_t const base  = static_cast<int64_t>(blockIdx.x) * SG_TILE;
  int64_t const first = base + static_cast<int64_t>(threadIdx.x) * SG_ITEMS;
  thread_items t;
  load_items(src, base, L, t);
  bool const any = __syncthreads_or(t.start != 0);
  if (threadIdx.x == 0) tile_flag[blockIdx.x] = any ? 1u : 0u;
  for (int k = 0; k < src.nkinds; ++k) SG_DISPATCH(sk[k], tile_carry_kind, src, sk[k], k, t, first, tile_val, tiles, sv, sf)
}

template <int OP>
__device__ void spine_kind(uint64_t* val, uint32_t const* flag, int64_t tiles, uint64_t* sv, uint32_t* sf)
{
  int64_t const per = (tiles + SG_SPINE - 1) / SG_SPINE;
  int64_t const lo  = std::min<int64_t>(static_cast<int64_t>(threadIdx.x) * per, tiles);
  int64_t const hi  = std::min<int64_t>(lo + per, tiles);
  uint64_t acc      = identity_of<OP>();
  bool any          = false;
  for (int64_t i = lo; i < hi; ++i) {
    bool const f = gload(flag + i) != 0;
    acc          = f ? gload(val + i) : op_of<OP>(acc, gload(val + i));
    any          = any || f;
  }
  uint64_t ev, tv;
  bool ef;
  block_seg_scan<OP, SG_SPINE>(acc, any, ev, ef, tv, sv, sf);
  uint64_t run = ev;  // what flows into tile lo (the identity before tile 0)
  for (int64_t i = lo; i < hi; ++i) {
    uint64_t const v = gload(val + i);
    bool const f     = gload(flag + i) != 0;
    gstore(val + i, run);
    run = f ? v : op_of<OP>(run, v);
  }
}

// in place: tile_val[k * tiles + tile] becomes the carry INTO the tile (the aggregate of the segment that runs into it)
__global__ void __launch_bounds__(SG_SPINE) k_seg_spine(scan_src src, uint64_t* tile_val, uint32_t const* tile_flag, int64_t tiles)
{
  __shared__ uint64_t sv[SG_SPINE / 64];
  __shared__ uint32_t sf[SG_SPINE / 64];
  __shared__ scan_kind sk[SG_KINDS];
  stage_kinds(src, sk);
  for (int k = 0; k < src.nkinds; ++k)
    SG_DISPATCH_OP(sk[k].op, spine_kind, tile_val + static_cast<int64_t>(k) * tiles, tile_flag, tiles, sv, sf)
}

__global__ void __launch_bounds__(SG_THREADS) k_seg_apply(scan_src src, uint64_t const* tile_carry, int64_t tiles)
{
  __shared__ uint64_t sv[SG_THREADS / 64];
  __shared__ uint32_t sf[SG_THREADS / 64];
  __shared__ tile_lds L;
  __shared__ scan_kind sk[SG_KINDS];
  stage_kinds(src, sk);
  int64_t const base = static_cast<int64_t>(blockIdx.x) * SG_TILE;
  thread_items t;
  load_items(src, base, L, t);
  for (int k = 0; k < src.nkinds; ++k) {
    uint64_t const carry = gload(tile_carry + static_cast<int64_t>(k) * tiles + blockIdx.x);
    SG_DISPATCH(sk[k], apply_kind, src, sk[k], t, base, carry, L, sv, sf)
  }
}
#undef SG_DISPATCH
#undef SG_DISPATCH_OP
#undef SG_PAIR

// the segmented inclusive scans of src's kinds (reduce, spine, apply)
void segmented_scan(scan_src const& src, hipStream_t s)
{
  if (src.n <= 0 || src.nkinds == 0) return;
  int64_t const tiles = (src.n + SG_TILE - 1) / SG_TILE;
  scratch tmp{s, get_current_device_resource_ref(), {}};
  auto* tile_val  = tmp.alloc<uint64_t>(static_cast<std::size_t>(tiles * src.nkinds));
  auto* tile_flag = tmp.alloc<uint32_t>(static_cast<std::size_t>(tiles));
  {
    prof::scope p_{"scan_tiles", s};
    hipLaunchKernelGGL(k_seg_tile_carry, dim3(static_cast<unsigned>(tiles)), dim3(SG_THREADS), 0, s, src, tile_val, tile_flag, tiles);
  }
  {
    prof::scope p_{"scan_spine", s};
    hipLaunchKernelGGL(k_seg_spine, dim3(1), dim3(SG_SPINE), 0, s, src, tile_val, tile_flag, tiles);
  }
  {
    prof::scope p_{"scan_apply", s};
    hipLaunchKernelGGL(k_seg_apply, dim3(static_cast<unsigned>(tiles)), dim3(SG_THREADS), 0, s, src, tile_val, tiles);
  }
  CUDF_HIP_TRY(hipGetLastError());
}

// ---------------------------------------------------------------------------------------------------------
// group order

// bits[i] = the value of row order[i] (order == nullptr: row i), when bits != nullptr; mask bit i = its validity, when mask != nullptr
__global__ void __launch_bounds__(256) k_group_values(device_column col, uint32_t const* order, int64_t nk, uint64_t* bits,
                                                      bitmask_type* mask, int32_t* null_count)
{
  int64_t const e = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  bool valid      = false;
  if (e < nk) {
    uint32_t const row = order ? gload(order + e) : static_cast<uint32_t>(e);
    if (bits) gstore(bits + e, col_load_bits(col, row));
    valid = col_is_valid(col, row);
  }
  if (mask == nullptr) return;
  uint64_t const m = __ballot(valid);
  int const lane   = threadIdx.x & 63;
  int64_t const w0 = (e - lane) >> 5;  // first mask word of this wave's 64 positions
  if (lane == 0 && e < nk) {
    gstore(mask + w0, static_cast<bitmask_type>(m));
    int64_t const live  = nk - e < 64 ? nk - e : 64;
    int32_t const nulls = static_cast<int32_t>(live) - __popcll(m);
    if (nulls) atomicAdd(null_count, nulls);
  }
  if (lane == 32 && e < nk) gstore(mask + w0 + 1, static_cast<bitmask_type>(m >> 32));
}

// RANK: per position p of the (label, value) order, bit 0 = p starts a run of equal values (nulls equal nulls) inside its group,
// bit 1 = p ends one, bit 2 = the value is valid
__global__ void __launch_bounds__(256) k_rank_words(device_column col, uint32_t const* vrow, int32_t const* labels, int32_t const* offsets,
                                                    int64_t nk, uint64_t* words)
{
  int64_t const p = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (p >= nk) return;
  int32_t const g    = gload(labels + p);
  uint32_t const row = gload(vrow + p);
  bool const valid   = col_is_valid(col, row);
  auto const same    = [&](int64_t q) {
    uint32_t const other = gload(vrow + q);
    bool const ov        = col_is_valid(col, other);
    return valid == ov && (!valid || sortable_word(col, row) == sortable_word(col, other));
  };
  bool const starts = p == gload(offsets + g) || !same(p - 1);
  bool const ends   = p + 1 == gload(offsets + g + 1) || !same(p + 1);
  gstore(words + p, static_cast<uint64_t>(starts) | (static_cast<uint64_t>(ends) << 1) | (static_cast<uint64_t>(valid) << 2));
}

// pos[order[q]] = q: the group-order position of a row
__global__ void __launch_bounds__(256) k_positions(uint32_t const* order, int64_t nk, int32_t* pos)
{
  int64_t const q = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (q < nk) gstore(pos + gload(order + q), static_cast<int32_t>(q));
}

struct rank_args {
  uint32_t const* vrow;        // value-order position -> row
  int32_t const* pos;          // row -> group-order position
  int32_t const* labels;
  int32_t const* offsets;
  uint64_t const* starts;      // forward MAX scan of (run start + 1): p's run starts at starts[p] - 1
  uint64_t const* ends;        // backward MAX scan of (nk - run end): p's run ends at nk - ends[p]
  uint64_t const* dense;       // forward SUM scan of run starts
  uint64_t const* valid_runs;  // forward SUM scan of valid values (nullptr: count every row)
  int64_t nk;
  int32_t method;
  int32_t percentage;
  void* out;                   // INT32, or FLOAT64 for AVERAGE and every percentage
};

// the rank of every position of the value order, written to its row's group-order position
// (reference group_rank_scan.cu: min/max/first/average/dense rank scans and group_rank_to_percentage)
__global__ void __launch_bounds__(256) k_rank_finish(rank_args a)
{
  int64_t const p = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (p >= a.nk) return;
  int32_t const g   = gload(a.labels + p);
  int64_t const gs  = gload(a.offsets + g);
  int64_t const ge  = gload(a.offsets + g + 1);
  auto const rmin   = [&] { return static_cast<int64_t>(gload(a.starts + p)) - gs; };
  auto const rmax   = [&] { return a.nk - static_cast<int64_t>(gload(a.ends + p)) - gs + 1; };
  double r          = 0.0;
  int32_t ri        = 0;
  switch (static_cast<rank_method>(a.method)) {
    case rank_method::FIRST: ri = static_cast<int32_t>(p - gs + 1); break;
    case rank_method::MIN: ri = static_cast<int32_t>(rmin()); break;
    case rank_method::MAX: ri = static_cast<int32_t>(rmax()); break;
    case rank_method::DENSE: ri = static_cast<int32_t>(gload(a.dense + p)); break;
    default: {
      int32_t const lo = static_cast<int32_t>(rmin()), hi = static_cast<int32_t>(rmax());
      r                = lo + (hi - lo) / 2.0;
    }
  }
  if (static_cast<rank_method>(a.method) != rank_method::AVERAGE) r = ri;
  int64_t const q = gload(a.pos + gload(a.vrow + p));
  if (a.percentage == static_cast<int32_t>(rank_percentage::NONE)) {
    if (static_cast<rank_method>(a.method) == rank_method::AVERAGE) gstore(static_cast<double*>(a.out) + q, r);
    else gstore(static_cast<int32_t*>(a.out) + q, ri);
    return;
  }
  int32_t const count = a.valid_runs ? static_cast<int32_t>(gload(a.valid_runs + ge - 1)) : static_cast<int32_t>(ge - gs);
  bool const zero     = a.percentage == static_cast<int32_t>(rank_percentage::ZERO_NORMALIZED);
  double result;
  if (static_cast<rank_method>(a.method) == rank_method::DENSE) {
    // the dense rank at position (group start + count - 1) of the value order (group_rank_scan.cu:280-291)
    int64_t const last_index = gs + count - 1;
    int32_t const last       = last_index < 0 ? 1 : static_cast<int32_t>(gload(a.dense + last_index));
    result                   = zero ? r / last : (last == 1 ? 0.0 : (r - 1.0) / (last - 1));
  } else {
    result = zero ? r / count : (count == 1 ? 0.0 : (r - 1.0) / (count - 1));
  }
  gstore(static_cast<double*>(a.out) + q, result);
}

// replace_nulls: out[p] = the value at the position the scan found (state - 1 forward, n - state backward), null if none
__global__ void __launch_bounds__(256) k_replace_finish(device_column col, uint32_t const* order, uint64_t const* state, int64_t n,
                                                        bool backward, void* out, bitmask_type* mask, int32_t* null_count)
{
  int64_t const e = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  bool valid      = false;
  if (e < n) {
    uint64_t const st = gload(state + e);
    valid             = st != 0;
    uint64_t v        = 0;
    if (valid) {
      int64_t const q    = backward ? n - static_cast<int64_t>(st) : static_cast<int64_t>(st) - 1;
      uint32_t const row = order ? gload(order + q) : static_cast<uint32_t>(q);
      v                  = col_load_bits(col, row);
    }
    store_width(out, e, col.width, v);
  }
  uint64_t const m = __ballot(valid);
  int const lane   = threadIdx.x & 63;
  int64_t const w0 = (e - lane) >> 5;
  if (lane == 0 && e < n) {
    gstore(mask + w0, static_cast<bitmask_type>(m));
    int64_t const live  = n - e < 64 ? n - e : 64;
    int32_t const nulls = static_cast<int32_t>(live) - __popcll(m);
    if (nulls) atomicAdd(null_count, nulls);
  }
  if (lane == 32 && e < n) gstore(mask + w0 + 1, static_cast<bitmask_type>(m >> 32));
}

// ---------------------------------------------------------------------------------------------------------
// host side

bool scan_kind_ok(aggregation::Kind k)
{
  return k == aggregation::SUM || k == aggregation::PRODUCT || k == aggregation::MIN || k == aggregation::MAX ||
         k == aggregation::COUNT_VALID || k == aggregation::COUNT_ALL || k == aggregation::RANK;
}

// result type of a scan kind over `source` (EMPTY: not supported; reference group_scan_util.cuh is_group_scan_supported)
data_type scan_type(data_type source, aggregation const& a)
{
  auto const invalid = data_type{type_id::EMPTY};
  if (cudf::detail::class_of(source.id()) == CLS_NONE) return invalid;
  switch (a.kind) {
    case aggregation::COUNT_VALID:
    case aggregation::COUNT_ALL: return data_type{type_id::INT32};
    case aggregation::RANK: {
      auto const& r = dynamic_cast<cudf::detail::rank_aggregation const&>(a);
      bool const fp = r._method == rank_method::AVERAGE || r._percentage != rank_percentage::NONE;
      return data_type{fp ? type_id::FLOAT64 : type_id::INT32};
    }
    default: return cudf::detail::target_type(source, a.kind);  // SUM, PRODUCT, MIN, MAX
  }
}

// the request's grouped values: bits (nullptr when the key order is the identity) and the mask (nullptr when not nullable)
struct grouped_values {
  uint64_t* bits{nullptr};
  bitmask_type* mask{nullptr};
  rmm::device_buffer mask_buf{};
  int32_t null_count{0};
};

grouped_values group_values(helper const& h, column_view const& values, bool want_bits, scratch& tmp, hipStream_t s)
{
  grouped_values g;
  bool const need_bits = want_bits && !h.identity_order;
  if (values.nullable()) {
    g.mask_buf = rmm::device_buffer{bitmask_allocation_size_bytes(static_cast<size_type>(h.nk)), s, get_current_device_resource_ref()};
    g.mask     = static_cast<bitmask_type*>(g.mask_buf.data());
  }
  if (!need_bits && g.mask == nullptr) return g;
  if (need_bits) g.bits = tmp.alloc<uint64_t>(static_cast<std::size_t>(h.nk));
  auto* d_nulls = tmp.alloc<int32_t>(1);
  CUDF_HIP_TRY(hipMemsetAsync(d_nulls, 0, sizeof(int32_t), s));
  {
    prof::scope p_{"scan_gather", s};
    hipLaunchKernelGGL(k_group_values, dim3(blocks_of(h.nk)), dim3(256), 0, s, cudf::detail::make_device_column(values),
                       h.identity_order ? nullptr : h.order, h.nk, g.bits, g.mask, d_nulls);
  }
  CUDF_HIP_TRY(hipGetLastError());
  if (g.mask) {
    CUDF_HIP_TRY(hipMemcpyAsync(&g.null_count, d_nulls, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    CUDF_HIP_TRY(hipStreamSynchronize(s));
  }
  return g;
}

rmm::device_buffer copy_mask(grouped_values const& g, int64_t nk, hipStream_t s, rmm::device_async_resource_ref mr)
{
  if (g.mask == nullptr) return rmm::device_buffer{};
  return rmm::device_buffer{g.mask, bitmask_allocation_size_bytes(static_cast<size_type>(nk)), s, mr};
}

scan_src make_src(helper const& h, column_view const& values, grouped_values const& g)
{
  scan_src src{};
  src.col         = cudf::detail::make_device_column(values);
  src.bits        = g.bits;
  src.valid       = g.mask;
  src.labels      = h.labels;
  src.n           = h.nk;
  src.read_values = 1;
  return src;
}

// one RANK result (reference sort/scan.cpp:137-210)
std::unique_ptr<column> rank_scan(helper& h, column_view const& values, cudf::detail::rank_aggregation const& r, bool presorted,
                                  grouped_values const& g, hipStream_t s, rmm::device_async_resource_ref mr)
{
  int64_t const nk = h.nk;
  scratch tmp{s, get_current_device_resource_ref(), {}};
  bool const descending  = r._column_order == order::DESCENDING;
  bool const nulls_first = (r._null_precedence == null_order::BEFORE) != descending;
  // pre-sorted keys: the values are taken as ordered inside their groups already (as the reference does for Spark)
  uint32_t const* vrow = presorted ? h.order : h.value_order(values, descending, nulls_first);
  auto* words          = tmp.alloc<uint64_t>(static_cast<std::size_t>(nk));
  auto* pos            = tmp.alloc<int32_t>(static_cast<std::size_t>(h.n));
  auto const dcol      = cudf::detail::make_device_column(values);
  {
    prof::scope p_{"scan_rank_words", s};
    hipLaunchKernelGGL(k_rank_words, dim3(blocks_of(nk)), dim3(256), 0, s, dcol, vrow, h.labels, h.offsets, nk, words);
    hipLaunchKernelGGL(k_positions, dim3(blocks_of(nk)), dim3(256), 0, s, h.order, nk, pos);
  }
  CUDF_HIP_TRY(hipGetLastError());
  bool const needs_min   = r._method == rank_method::MIN || r._method == rank_method::AVERAGE;
  bool const needs_max   = r._method == rank_method::MAX || r._method == rank_method::AVERAGE;
  bool const needs_dense = r._method == rank_method::DENSE;
  bool const count_valid = r._percentage != rank_percentage::NONE && values.nullable() && r._null_handling == null_policy::EXCLUDE;
  rank_args a{};
  scan_src fwd{};
  fwd.bits        = words;
  fwd.labels      = h.labels;
  fwd.n           = nk;
  fwd.read_values = 1;
  auto add_kind   = [&](scan_src& src, int32_t op, int32_t lift) {
    auto* out = tmp.alloc<uint64_t>(static_cast<std::size_t>(nk));
    src.kind[src.nkinds++] = scan_kind{op, lift, 8, out};
    return static_cast<uint64_t const*>(out);
  };
  if (needs_min) a.starts = add_kind(fwd, OP_MAX_U, LIFT_BIT0_POS);
  if (needs_dense) a.dense = add_kind(fwd, OP_ADD_I, LIFT_BIT0);
  if (count_valid) a.valid_runs = add_kind(fwd, OP_ADD_I, LIFT_BIT2);
  segmented_scan(fwd, s);
  if (needs_max) {
    scan_src bwd  = fwd;
    bwd.nkinds    = 0;
    bwd.backward  = 1;
    a.ends        = add_kind(bwd, OP_MAX_U, LIFT_BIT1_POS);
    segmented_scan(bwd, s);
  }
  bool const fp = r._method == rank_method::AVERAGE || r._percentage != rank_percentage::NONE;
  auto const type = data_type{fp ? type_id::FLOAT64 : type_id::INT32};
  auto out        = std::make_unique<column>(type, static_cast<size_type>(nk),
                                      rmm::device_buffer{static_cast<std::size_t>(nk) * size_of(type), s, mr},
                                      r._null_handling == null_policy::EXCLUDE ? copy_mask(g, nk, s, mr) : rmm::device_buffer{},
                                      r._null_handling == null_policy::EXCLUDE ? g.null_count : 0);
  a.vrow       = vrow;
  a.pos        = pos;
  a.labels     = h.labels;
  a.offsets    = h.offsets;
  a.nk         = nk;
  a.method     = static_cast<int32_t>(r._method);
  a.percentage = static_cast<int32_t>(r._percentage);
  a.out        = out->mutable_view().head();
  {
    prof::scope p_{"scan_rank_finish", s};
    hipLaunchKernelGGL(k_rank_finish, dim3(blocks_of(nk)), dim3(256), 0, s, a);
  }
  CUDF_HIP_TRY(hipGetLastError());
  CUDF_HIP_TRY(hipStreamSynchronize(s));  // the temporaries above go with tmp
  return out;
}

std::unique_ptr<table> keys_in_group_order(helper const& h, stream_ref stream, rmm::device_async_resource_ref mr)
{
  column_view const order_view{data_type{type_id::INT32}, static_cast<size_type>(h.nk), h.order, nullptr, 0};
  return cudf::gather(h.keys, order_view, out_of_bounds_policy::DONT_CHECK, stream, mr);
}
}  // namespace

}  // namespace cudf::groupby::detail

namespace cudf::groupby {

std::pair<std::unique_ptr<table>, std::vector<aggregation_result>> groupby::scan(std::span<scan_request const> requests, stream_ref stream,
                                                                                 rmm::device_async_resource_ref mr)
{
  CUDF_FUNC_RANGE();
  using namespace detail;
  // reference groupby.cu:245-251, sort/scan.cpp:48, group_scan_util.cuh:42
  CUDF_EXPECTS(std::all_of(requests.begin(), requests.end(), [this](auto const& r) { return r.values.size() == _keys.num_rows(); }),
               "Size mismatch between request values and groupby keys.");
  for (auto const& r : requests)
    for (auto const& a : r.aggregations) {
      if (!scan_kind_ok(a->kind)) CUDF_FAIL("Unsupported groupby scan aggregation");
      if (scan_type(r.values.type(), *a).id() == type_id::EMPTY) CUDF_FAIL("Unsupported groupby scan type-agg combination.");
    }
  CUDF_EXPECTS(_keys.num_columns() > 0, "The sort-based groupby needs at least one key column.");
  hipStream_t const s = stream.value();
  auto const empty    = [&] {
    std::vector<aggregation_result> res(requests.size());
    for (std::size_t i = 0; i < requests.size(); ++i)
      for (auto const& a : requests[i].aggregations) res[i].results.push_back(make_empty_column(scan_type(requests[i].values.type(), *a)));
    return std::pair{empty_like(_keys), std::move(res)};
  };
  if (_keys.num_rows() == 0) return empty();
  bool const presorted = _keys_are_sorted == sorted::YES;
  helper h{_keys, s};
  h.build(_include_null_keys == null_policy::EXCLUDE, presorted);
  if (h.nk == 0) return empty();
  int64_t const nk = h.nk;

  std::vector<aggregation_result> results(requests.size());
  for (std::size_t ri = 0; ri < requests.size(); ++ri) {
    auto const& req    = requests[ri];
    auto const& values = req.values;
    auto& out          = results[ri].results;
    out.resize(req.aggregations.size());
    bool const any_value_kind = std::any_of(req.aggregations.begin(), req.aggregations.end(), [](auto const& a) {
      return a->kind != aggregation::COUNT_ALL && a->kind != aggregation::COUNT_VALID && a->kind != aggregation::RANK;
    });
    scratch tmp{s, get_current_device_resource_ref(), {}};
    auto g   = group_values(h, values, any_value_kind, tmp, s);
    auto src        = make_src(h, values, g);
    src.read_values = any_value_kind ? 1 : 0;
    // the scan kinds, SG_KINDS at a time
    auto flush = [&] {
      segmented_scan(src, s);
      src.nkinds = 0;
    };
    for (std::size_t j = 0; j < req.aggregations.size(); ++j) {
      auto const& a = *req.aggregations[j];
      if (a.kind == aggregation::RANK) continue;
      auto const type  = scan_type(values.type(), a);
      auto const cls   = cudf::detail::class_of(values.type().id());
      bool const fp32  = cls == CLS_F32, fp64 = cls == CLS_F64;
      scan_kind k{};
      k.width = static_cast<int32_t>(size_of(type));
      switch (a.kind) {
        case aggregation::SUM:
          k.op   = fp32 ? OP_ADD_F32 : fp64 ? OP_ADD_F64 : OP_ADD_I;
          k.lift = (fp32 || fp64) ? LIFT_BITS : LIFT_INT;
          break;
        case aggregation::PRODUCT:
          k.op   = fp32 ? OP_MUL_F32 : fp64 ? OP_MUL_F64 : OP_MUL_I;
          k.lift = (fp32 || fp64) ? LIFT_BITS : LIFT_INT;
          break;
        case aggregation::MIN:
        case aggregation::MAX:
          k.op   = a.kind == aggregation::MIN ? OP_MIN_U : OP_MAX_U;
          k.lift = LIFT_ORDERED;
          break;
        default:  // COUNT_VALID, COUNT_ALL
          k.op   = OP_ADD_I;
          k.lift = a.kind == aggregation::COUNT_ALL ? LIFT_ONE : LIFT_VALID;
      }
      bool const counts = a.kind == aggregation::COUNT_ALL || a.kind == aggregation::COUNT_VALID;
      auto col = std::make_unique<column>(type, static_cast<size_type>(nk), rmm::device_buffer{static_cast<std::size_t>(nk) * size_of(type), s, mr},
                                          counts ? rmm::device_buffer{} : copy_mask(g, nk, s, mr), counts ? 0 : g.null_count);
      k.out                     = col->mutable_view().head();
      out[j]                    = std::move(col);
      src.kind[src.nkinds++]    = k;
      if (src.nkinds == SG_KINDS) flush();
    }
    if (src.nkinds > 0) flush();
    for (std::size_t j = 0; j < req.aggregations.size(); ++j) {
      auto const& a = *req.aggregations[j];
      if (a.kind != aggregation::RANK) continue;
      out[j] = rank_scan(h, values, dynamic_cast<cudf::detail::rank_aggregation const&>(a), presorted, g, s, mr);
    }
    CUDF_HIP_TRY(hipStreamSynchronize(s));  // tmp's buffers are released when the request is done
  }
  return {keys_in_group_order(h, stream, mr), std::move(results)};
}

std::pair<std::unique_ptr<table>, std::unique_ptr<table>> groupby::replace_nulls(table_view const& values,
                                                                                 std::span<replace_policy const> replace_policies,
                                                                                 stream_ref stream, rmm::device_async_resource_ref mr)
{
  CUDF_FUNC_RANGE();
  using namespace detail;
  // reference groupby.cu:291-296
  CUDF_EXPECTS(_keys.num_rows() == values.num_rows(), "Size mismatch between group labels and value.");
  CUDF_EXPECTS(static_cast<size_type>(replace_policies.size()) == values.num_columns(),
               "Size mismatch between num_columns and replace_policies.");
  for (auto const& c : values)
    CUDF_EXPECTS(cudf::detail::class_of(c.type().id()) != CLS_NONE, "Only fixed-width columns of at most 8 bytes can be filled.",
                 cudf::data_type_error);
  CUDF_EXPECTS(_keys.num_columns() > 0, "The sort-based groupby needs at least one key column.");
  if (values.num_rows() == 0) return {empty_like(_keys), empty_like(values)};
  hipStream_t const s = stream.value();
  helper h{_keys, s};
  h.build(_include_null_keys == null_policy::EXCLUDE, _keys_are_sorted == sorted::YES);
  if (h.nk == 0) return {empty_like(_keys), empty_like(values)};
  int64_t const nk = h.nk;
  column_view const order_view{data_type{type_id::INT32}, static_cast<size_type>(nk), h.order, nullptr, 0};
  std::vector<std::unique_ptr<column>> cols;
  for (size_type c = 0; c < values.num_columns(); ++c) {
    auto const& col = values.column(c);
    if (!col.nullable()) {  // nothing to fill: the values in group order
      cols.push_back(std::move(cudf::gather(table_view{{col}}, order_view, out_of_bounds_policy::DONT_CHECK, stream, mr)->release()[0]));
      continue;
    }
    scratch tmp{s, get_current_device_resource_ref(), {}};
    auto g              = group_values(h, col, false, tmp, s);
    auto src            = make_src(h, col, g);
    src.read_values     = 0;
    src.backward        = replace_policies[c] == replace_policy::FOLLOWING ? 1 : 0;
    auto* state         = tmp.alloc<uint64_t>(static_cast<std::size_t>(nk));
    src.kind[0]         = scan_kind{OP_MAX_U, LIFT_VALID_POS, 8, state};
    src.nkinds          = 1;
    segmented_scan(src, s);
    auto out = std::make_unique<column>(col.type(), static_cast<size_type>(nk),
                                        rmm::device_buffer{static_cast<std::size_t>(nk) * size_of(col.type()), s, mr},
                                        rmm::device_buffer{bitmask_allocation_size_bytes(static_cast<size_type>(nk)), s, mr}, 0);
    auto* d_nulls = tmp.alloc<int32_t>(1);
    CUDF_HIP_TRY(hipMemsetAsync(d_nulls, 0, sizeof(int32_t), s));
    {
      prof::scope p_{"scan_fill", s};
      hipLaunchKernelGGL(k_replace_finish, dim3(blocks_of(nk)), dim3(256), 0, s, cudf::detail::make_device_column(col),
                         h.identity_order ? nullptr : h.order, state, nk, src.backward != 0, out->mutable_view().head(),
                         out->mutable_view().null_mask(), d_nulls);
    }
    CUDF_HIP_TRY(hipGetLastError());
    int32_t nulls = 0;
    CUDF_HIP_TRY(hipMemcpyAsync(&nulls, d_nulls, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    CUDF_HIP_TRY(hipStreamSynchronize(s));
    out->set_null_count(nulls);
    cols.push_back(std::move(out));
  }
  return {keys_in_group_order(h, stream, mr), std::make_unique<table>(std::move(cols))};
}

}  // namespace cudf::groupby
