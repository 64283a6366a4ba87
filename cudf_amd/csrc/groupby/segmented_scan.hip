// SPDX-License-Identifier: Apache-2.0
// One segmented inclusive scan core for every scan kind (segmented_scan.hpp):
//   k_seg_tile_carry  per tile of 2048 positions: does it hold a group boundary, and the aggregate of its trailing segment
//   k_seg_spine       one workgroup: segmented scan of those tile carries (each thread walks a run of tiles, then a block scan)
//   k_seg_apply       every tile again, scanned with the carry that flows into it
// No workgroup waits on another (no decoupled look-back), so a scan cannot hang behind a workgroup that is not resident.
#include "segmented_scan.hpp"
#include "../common/profiler.hpp"

#include <cudf/utilities/error.hpp>

#include <algorithm>

namespace cudf::groupby::detail {
namespace {
using cudf::detail::CLS_BOOL;
using cudf::detail::CLS_F32;
using cudf::detail::CLS_F64;
using cudf::detail::CLS_SINT;
using cudf::detail::col_load_bits;
using cudf::detail::device_column;
using cudf::detail::gload;
using cudf::detail::gstore;
using cudf::detail::ordered_word;
namespace prof = cudf::detail::prof;

constexpr int SG_THREADS = 256;
constexpr int SG_ITEMS   = 8;                        // consecutive positions per thread
constexpr int SG_TILE    = SG_THREADS * SG_ITEMS;    // positions per workgroup
constexpr int SG_SPINE   = 1024;                     // threads of the spine workgroup

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
    if (col.cls == CLS_SINT) return static_cast<uint64_t>(cudf::detail::sign_extend(raw, col.width));
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

}  // namespace

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

}  // namespace cudf::groupby::detail
