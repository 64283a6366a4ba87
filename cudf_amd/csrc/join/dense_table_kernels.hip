// SPDX-License-Identifier: Apache-2.0
// gfx950 kernels of the dense direct-address table (engine.hpp join_args::dense_head): key range, build, row lists, count and
// retrieve passes. The partitioned passes over the same table are in dense_part_kernels.hip.
#include "join_device.hpp"
#include "../common/profiler.hpp"

#include <cudf/utilities/error.hpp>

namespace cudf::detail::join {
namespace {

template <bool SIGNED>
__global__ void __launch_bounds__(256) k_key_minmax(join_args const* __restrict__ ap, uint64_t* out)
{
  join_args const& a = *ap;
  using T = std::conditional_t<SIGNED, long long, unsigned long long>;
  __shared__ T s_lo[4], s_hi[4];
  int64_t const n      = a.build.nrows;
  int64_t const stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  bool const narrow    = a.build.col[0].width == 4;  // a 4-byte integer key column: widened like the join's scatter does
  uint64_t const* keys = static_cast<uint64_t const*>(a.build.col[0].head) + (narrow ? 0 : a.build.col[0].offset);
  uint32_t const* keys32 = static_cast<uint32_t const*>(a.build.col[0].head) + a.build.col[0].offset;
  bool const masked    = a.check_nulls && a.build.col[0].mask != nullptr;
  T lo = SIGNED ? static_cast<T>(INT64_MAX) : static_cast<T>(UINT64_MAX), hi = SIGNED ? static_cast<T>(INT64_MIN) : T{0};
  constexpr int R = 4;  // loads in flight per thread
  for (int64_t i0 = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i0 < n; i0 += R * stride) {
    T k[R];
    bool ok[R];
#pragma unroll
    for (int j = 0; j < R; ++j) {
      int64_t const i = i0 + j * stride;
      ok[j]           = i < n;
      if (narrow) {
        uint32_t const k32 = ok[j] ? gload(keys32 + i) : 0u;
        k[j]               = SIGNED ? static_cast<T>(static_cast<int32_t>(k32)) : static_cast<T>(k32);
      } else {
        k[j] = ok[j] ? static_cast<T>(gload(keys + i)) : T{0};
      }
      ok[j]           = ok[j] && !(masked && !col_is_valid(a.build.col[0], i));
    }
#pragma unroll
    for (int j = 0; j < R; ++j) {
      lo = ok[j] && k[j] < lo ? k[j] : lo;
      hi = ok[j] && k[j] > hi ? k[j] : hi;
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    T const l2 = __shfl_xor(lo, o), h2 = __shfl_xor(hi, o);
    lo = l2 < lo ? l2 : lo;
    hi = h2 > hi ? h2 : hi;
  }
  if ((threadIdx.x & 63) == 0) {
    s_lo[threadIdx.x >> 6] = lo;
    s_hi[threadIdx.x >> 6] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) {
      lo = s_lo[w] < lo ? s_lo[w] : lo;
      hi = s_hi[w] > hi ? s_hi[w] : hi;
    }
    atomicMin(reinterpret_cast<T*>(out), lo);
    atomicMax(reinterpret_cast<T*>(out) + 1, hi);
  }
}

__global__ void __launch_bounds__(256) k_dense_build(join_args const* __restrict__ ap)
{
  join_args const& a   = *ap;
  int64_t const n      = a.build.nrows;
  int64_t const stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  uint64_t const* keys = static_cast<uint64_t const*>(a.build.col[0].head) + a.build.col[0].offset;
  bool const masked    = a.check_nulls && a.build.col[0].mask != nullptr;
  bool dup             = false;
  for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < n; i += stride) {
    if (masked && !col_is_valid(a.build.col[0], i)) continue;  // a NULL key is never inserted (null_equality::UNEQUAL)
    uint64_t const idx = gload(keys + i) - a.dense_lo;         // < dense_range: lo / range come from these very keys
    int32_t const old  = atomicExch(a.dense_head + idx, static_cast<int32_t>(i));
    gstore(a.dense_next + i, old);
    dup = dup || old >= 0;
  }
  if (__any(dup) && (threadIdx.x & 63) == 0) gstore(a.dense_dups, 1);
}

// count pass over a dense table: same outputs as k_probe_count (match cache, per-workgroup pair counts, optional row counts)
__global__ void __launch_bounds__(256) k_dense_count(join_args const* __restrict__ ap)
{
  join_args const& a = *ap;
  __shared__ unsigned long long s_total;
  int64_t const n       = a.probe.nrows;
  int const kind        = a.kind;
  uint64_t const* pkeys = static_cast<uint64_t const*>(a.probe.col[0].head) + a.probe.col[0].offset;
  bitmask_type const* probe_mask = a.check_nulls ? a.probe.col[0].mask : nullptr;
  int64_t const probe_off        = a.probe.col[0].offset;
  uint64_t const lo = a.dense_lo, range = a.dense_range;
  bool const dups   = a.dense_has_dups != 0;
  if (threadIdx.x == 0) s_total = 0;
  __syncthreads();
  constexpr int R = 4;
  unsigned long long local_count = 0;
  int64_t const begin = static_cast<int64_t>(blockIdx.x) * a.chunk, end = min(n, begin + a.chunk);
  for (int64_t base = begin; base < end; base += static_cast<int64_t>(blockDim.x) * R) {
    int64_t j[R];
    bool live[R], in[R];
    uint64_t idx[R];
    int32_t head[R];
#pragma unroll
    for (int k = 0; k < R; ++k) {
      j[k]    = base + static_cast<int64_t>(k) * blockDim.x + threadIdx.x;
      live[k] = j[k] < end;
      in[k]   = false;
      idx[k]  = 0;
      if (live[k]) {
        bool valid = true;
        if (probe_mask != nullptr) valid = (gload(probe_mask + ((probe_off + j[k]) >> 5)) >> ((probe_off + j[k]) & 31)) & 1u;
        idx[k] = gload(pkeys + j[k]) - lo;
        in[k]  = valid && idx[k] < range;  // a key outside the build side's range matches nothing and reads nothing
      }
    }
#pragma unroll
    for (int k = 0; k < R; ++k) head[k] = in[k] ? gload(a.dense_head + idx[k]) : -1;
    // (some build key repeats: dense_head holds the OFFSETS of the keys' row lists - engine.hpp - and a key's row count is the
    // difference to its neighbour; a chain walk per probe row took 149 ms for 1000 probes of a key with 100,000 build rows)
    int32_t next_off[R];
#pragma unroll
    for (int k = 0; k < R; ++k) next_off[k] = (dups && in[k]) ? gload(a.dense_head + idx[k] + 1) : 0;
#pragma unroll
    for (int k = 0; k < R; ++k) {
      if (!live[k]) continue;
      unsigned int const cnt = dups ? (in[k] ? static_cast<unsigned int>(next_off[k] - head[k]) : 0u) : (head[k] >= 0 ? 1u : 0u);
      uint32_t const what    = dups ? static_cast<uint32_t>(idx[k]) : static_cast<uint32_t>(head[k]);  // the key's list / its one build row
      local_count += count_row(a, kind, j[k], cnt == 0 ? MATCH_NONE : (what | (cnt > 1 ? MATCH_MULTI : 0u)), cnt);
    }
  }
  count_block_total(local_count, &s_total, a.block_counts);
}

// retrieve pass over a dense table: streams the match cache; rows with several matches walk their key's chain
__global__ void __launch_bounds__(256) k_dense_retrieve(join_args const* __restrict__ ap)
{
  join_args const& a = *ap;
  __shared__ unsigned long long s_cursor;
  int64_t const n = a.probe.nrows;
  int const kind  = a.kind;
  if (threadIdx.x == 0) s_cursor = a.block_counts[blockIdx.x];
  __syncthreads();
  int const lane = threadIdx.x & 63;
  auto emit = [&](bool want, size_type prow, size_type brow) { wave_emit_pair(a, kind, want, prow, brow, &s_cursor, lane); };
  int64_t const begin = static_cast<int64_t>(blockIdx.x) * a.chunk, end = min(n, begin + a.chunk);
  bool const dups = a.dense_has_dups != 0;
  for (int64_t j0 = begin; j0 < end; j0 += blockDim.x) {
    int64_t const j  = j0 + threadIdx.x;
    bool const live  = j < end;
    uint32_t const c = live ? gload(a.match_cache + j) : MATCH_NONE;
    bool const none  = c == MATCH_NONE;
    bool const multi = !none && (c & MATCH_MULTI);
    size_type const prow = static_cast<size_type>(j + a.probe_row_base);
    int32_t r = static_cast<int32_t>(c & ~MATCH_MULTI);
    if (!dups) {  // unique build keys: the cache holds the one build row
      emit(live && !none, prow, r);
      if (kind != 0) emit(live && none, prow, JoinNoMatch);
      continue;
    }
    // Row lists (some build key repeats): the cache holds the key's index; its rows are dense_next[off, off + cnt).
    uint32_t const off = none ? 0u : static_cast<uint32_t>(gload(a.dense_head + r));
    uint32_t const cnt = none ? 0u : (multi ? static_cast<uint32_t>(gload(a.dense_head + r + 1)) - off : 1u);
    emit(live && !none, prow, none ? JoinNoMatch : gload(a.dense_next + off));
    if (kind != 0) emit(live && none, prow, JoinNoMatch);
    // very long lists (a hot build key): only the output range is reserved here, the pairs are written by the whole grid
    // (k_dense_big_emit) - the rows that hit a hot key may all sit in ONE workgroup's chunk of probe rows
    bool huge = a.big_list != nullptr && cnt > BIG_LIST;
    if (huge) {
      uint32_t const w = atomicAdd(a.big_count, 1u);
      if (w < BIG_LIST_CAP) {
        unsigned long long const base = atomicAdd(&s_cursor, static_cast<unsigned long long>(cnt - 1));
        gstore(reinterpret_cast<u32x4*>(a.big_list) + w, u32x4{static_cast<uint32_t>(prow), off + 1u, cnt - 1u, static_cast<uint32_t>(base)});
        gstore(a.big_list + 4u * BIG_LIST_CAP + w, static_cast<uint32_t>(base >> 32));
      } else {
        huge = false;  // (the list is full: this wave emits the row's pairs itself)
      }
    }
    // short lists: every lane walks its own; long lists: the WAVE emits 64 pairs per step, coalesced
    bool const big = cnt > 64 && !huge;
    uint32_t t     = 1;
    bool walking   = cnt > 1 && !big && !huge;
    while (__any(walking)) {
      int32_t const br = walking ? gload(a.dense_next + off + t) : JoinNoMatch;
      emit(walking, prow, br);
      ++t;
      walking = walking && t < cnt;
    }
    unsigned long long bigm = __ballot(big);
    while (bigm != 0) {
      int const src = __ffsll(static_cast<long long>(bigm)) - 1;
      bigm &= bigm - 1;
      uint32_t const boff = __shfl(off, src), bcnt = __shfl(cnt, src);
      size_type const bp  = __shfl(prow, src);
      for (uint32_t base = 1; base < bcnt; base += 64) {
        uint32_t const tt = base + static_cast<uint32_t>(lane);
        bool const w      = tt < bcnt;
        emit(w, bp, w ? gload(a.dense_next + boff + tt) : JoinNoMatch);
      }
    }
  }
}

// The pairs of the work list of hot-key probe rows (join_args::big_list): every workgroup takes its share of every entry's chunks.
__global__ void __launch_bounds__(256) k_dense_big_emit(join_args const* __restrict__ ap)
{
  join_args const& a   = *ap;
  uint32_t const items = min(gload(a.big_count), BIG_LIST_CAP);
  constexpr uint32_t CH = 2048;  // pairs per chunk
  for (uint32_t it = 0; it < items; ++it) {
    u32x4 const e   = gload(reinterpret_cast<u32x4 const*>(a.big_list) + it);
    uint64_t const base = (static_cast<uint64_t>(gload(a.big_list + 4u * BIG_LIST_CAP + it)) << 32) | e.w;
    uint32_t const chunks = (e.z + CH - 1) / CH;
    for (uint32_t c = blockIdx.x; c < chunks; c += gridDim.x) {
      for (uint32_t t = c * CH + threadIdx.x; t < min(e.z, (c + 1) * CH); t += blockDim.x) {
        int32_t const br = gload(a.dense_next + e.y + t);
        uint64_t const o = base + t;
        if (o < a.out_capacity) {
          gstore(a.out_probe + o, static_cast<size_type>(e.x));
          gstore(a.out_build + o, br);
        }
        if (a.kind == 2) gstore(a.build_matched + br, uint8_t{1});
      }
    }
  }
}

// ---- row lists for duplicated dense build keys: counts (k_dense_csr_count) -> exclusive scan in place (k_scan_u32_*) -> lists
// (k_dense_csr_fill). dense_head: [padded range + 1] counts, then offsets; dense_next: the build rows grouped by key.
__global__ void __launch_bounds__(256) k_dense_csr_count(join_args const* __restrict__ ap)
{
  join_args const& a   = *ap;
  int64_t const n      = a.build.nrows;
  int64_t const stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  uint64_t const* keys = static_cast<uint64_t const*>(a.build.col[0].head) + a.build.col[0].offset;
  bool const masked    = a.check_nulls && a.build.col[0].mask != nullptr;
  int const lane = threadIdx.x & 63;
  int64_t const rounds = (n + stride - 1) / stride;
  int64_t i            = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
  for (int64_t it = 0; it < rounds; ++it, i += stride) {  // (every lane runs every round: the ballots below are wave-wide)
    bool pending       = i < n && !(masked && !col_is_valid(a.build.col[0], i));
    uint64_t const idx = pending ? gload(keys + i) - a.dense_lo : 0;
    // same-address global atomics serialise (a build key with 100,000 rows): the first keys of the wave are counted once per
    // key, by one lane
    for (int round = 0; round < 2; ++round) {
      unsigned long long const todo = __ballot(pending);
      if (todo == 0) break;
      int const lead                = __ffsll(static_cast<long long>(todo)) - 1;
      uint64_t const lidx           = __shfl(static_cast<unsigned long long>(idx), lead);
      unsigned long long const same = __ballot(pending && idx == lidx);
      if (lane == lead) atomicAdd(a.dense_head + lidx, __popcll(same));
      if (idx == lidx) pending = false;
    }
    if (pending) atomicAdd(a.dense_head + idx, 1);
  }
}
__global__ void __launch_bounds__(256) k_dense_csr_fill(join_args const* __restrict__ ap, int32_t* cursor)
{
  join_args const& a   = *ap;
  int64_t const n      = a.build.nrows;
  int64_t const stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  uint64_t const* keys = static_cast<uint64_t const*>(a.build.col[0].head) + a.build.col[0].offset;
  bool const masked    = a.check_nulls && a.build.col[0].mask != nullptr;
  int const lane = threadIdx.x & 63;
  int64_t const rounds = (n + stride - 1) / stride;
  int64_t i            = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
  for (int64_t it = 0; it < rounds; ++it, i += stride) {
    bool const valid   = i < n && !(masked && !col_is_valid(a.build.col[0], i));
    bool pending       = valid;
    uint64_t const idx = valid ? gload(keys + i) - a.dense_lo : 0;
    int32_t pos        = 0;
    for (int round = 0; round < 2; ++round) {  // (wave-aggregated as in k_dense_csr_count: one atomic per key, ranks by popcount)
      unsigned long long const todo = __ballot(pending);
      if (todo == 0) break;
      int const lead                = __ffsll(static_cast<long long>(todo)) - 1;
      uint64_t const lidx           = __shfl(static_cast<unsigned long long>(idx), lead);
      unsigned long long const same = __ballot(pending && idx == lidx);
      int32_t base                  = 0;
      if (lane == lead) base = atomicAdd(cursor + lidx, __popcll(same));
      base = __shfl(base, lead);
      if (pending && idx == lidx) {
        pos     = base + __popcll(same & ((1ull << lane) - 1));
        pending = false;
      }
    }
    if (pending) pos = atomicAdd(cursor + idx, 1);
    if (valid) gstore(a.dense_next + gload(a.dense_head + idx) + pos, static_cast<int32_t>(i));
  }
}
// Exclusive scan of n uint32 (n a multiple of SCAN_TILE, at most 2^29 + SCAN_TILE) in place, three launches: tile sums, scan of the
// tile sums by one workgroup, tile-local scan + tile offset.
constexpr int SCAN_TILE = 1024 * 8;
__global__ void __launch_bounds__(1024) k_scan_u32_sums(uint32_t const* __restrict__ v, uint32_t* __restrict__ sums)
{
  __shared__ uint32_t s_w[16];
  u32x4 const* p = reinterpret_cast<u32x4 const*>(v + static_cast<int64_t>(blockIdx.x) * SCAN_TILE) + threadIdx.x * 2;
  u32x4 const a = gload(p), b = gload(p + 1);
  uint32_t t    = a.x + a.y + a.z + a.w + b.x + b.y + b.z + b.w;
  for (int o = 32; o > 0; o >>= 1) t += __shfl_down(t, o);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t tot = 0;
    for (int w = 0; w < 16; ++w) tot += s_w[w];
    sums[blockIdx.x] = tot;
  }
}
__global__ void __launch_bounds__(1024) k_scan_u32_tiles(uint32_t* sums, int32_t ntiles)
{
  __shared__ uint32_t s_w[16];
  __shared__ uint32_t s_carry;
  if (threadIdx.x == 0) s_carry = 0;
  __syncthreads();
  for (int base = 0; base < ntiles; base += 1024) {
    int const i        = base + threadIdx.x;
    uint32_t const x   = i < ntiles ? sums[i] : 0;
    uint32_t const off = s_carry + block_exclusive_scan(x, s_w);
    if (i < ntiles) sums[i] = off;
    __syncthreads();
    if (threadIdx.x == 1023) s_carry = off + x;
    __syncthreads();
  }
}
__global__ void __launch_bounds__(1024) k_scan_u32_apply(uint32_t* __restrict__ v, uint32_t const* __restrict__ sums)
{
  __shared__ uint32_t s_w[16];
  u32x4* p = reinterpret_cast<u32x4*>(v + static_cast<int64_t>(blockIdx.x) * SCAN_TILE) + threadIdx.x * 2;
  u32x4 a = gload(p), b = gload(p + 1);
  uint32_t const mine = a.x + a.y + a.z + a.w + b.x + b.y + b.z + b.w;
  uint32_t run = gload(sums + blockIdx.x) + block_exclusive_scan(mine, s_w);
  u32x4 oa, ob;
  oa.x = run; run += a.x;
  oa.y = run; run += a.y;
  oa.z = run; run += a.z;
  oa.w = run; run += a.w;
  ob.x = run; run += b.x;
  ob.y = run; run += b.y;
  ob.z = run; run += b.z;
  ob.w = run;
  gstore(p, oa);
  gstore(p + 1, ob);
}
}  // namespace

void launch_key_minmax(join_args const& a, join_args* d_args, int is_signed, uint64_t* out, hipStream_t stream)
{
  struct range_init { uint64_t lo, hi; };
  range_init const init{is_signed ? static_cast<uint64_t>(INT64_MAX) : UINT64_MAX, is_signed ? static_cast<uint64_t>(INT64_MIN) : uint64_t{0}};
  hipLaunchKernelGGL(k_store_args<range_init>, dim3(1), dim3(1), 0, stream, init, reinterpret_cast<range_init*>(out));
  hipLaunchKernelGGL(k_store_args<join_args>, dim3(1), dim3(1), 0, stream, a, d_args);
  cudf::detail::prof::scope prof_{"join_build", stream};
  unsigned const grid = static_cast<unsigned>(std::clamp<int64_t>((a.build.nrows + 4095) / 4096, 1, 4096));
  if (is_signed) hipLaunchKernelGGL(k_key_minmax<true>, dim3(grid), dim3(256), 0, stream, d_args, out);
  else hipLaunchKernelGGL(k_key_minmax<false>, dim3(grid), dim3(256), 0, stream, d_args, out);
  CUDF_HIP_TRY(hipGetLastError());
}
void launch_dense_build(join_args const& a, join_args* d_args, hipStream_t stream)
{
  hipLaunchKernelGGL(k_store_args<join_args>, dim3(1), dim3(1), 0, stream, a, d_args);
  cudf::detail::prof::scope prof_{"join_build", stream};
  hipLaunchKernelGGL(k_dense_build, dim3(grid_for(a.build.nrows)), dim3(256), 0, stream, d_args);
  CUDF_HIP_TRY(hipGetLastError());
}
std::size_t dense_csr_entries(uint64_t range) { return static_cast<std::size_t>((range + 1 + SCAN_TILE - 1) / SCAN_TILE) * SCAN_TILE; }
void launch_dense_csr(join_args const& a, join_args* d_args, int32_t* cursor, uint32_t* tile_sums, hipStream_t stream)
{
  // a.dense_head: dense_csr_entries(range) zeroed words; cursor: `range` zeroed words; tile_sums: entries / SCAN_TILE words
  hipLaunchKernelGGL(k_store_args<join_args>, dim3(1), dim3(1), 0, stream, a, d_args);
  cudf::detail::prof::scope prof_{"join_build", stream};
  int32_t const ntiles = static_cast<int32_t>(dense_csr_entries(a.dense_range) / SCAN_TILE);
  hipLaunchKernelGGL(k_dense_csr_count, dim3(grid_for(a.build.nrows)), dim3(256), 0, stream, d_args);
  hipLaunchKernelGGL(k_scan_u32_sums, dim3(ntiles), dim3(1024), 0, stream, reinterpret_cast<uint32_t const*>(a.dense_head), tile_sums);
  hipLaunchKernelGGL(k_scan_u32_tiles, dim3(1), dim3(1024), 0, stream, tile_sums, ntiles);
  hipLaunchKernelGGL(k_scan_u32_apply, dim3(ntiles), dim3(1024), 0, stream, reinterpret_cast<uint32_t*>(a.dense_head), tile_sums);
  hipLaunchKernelGGL(k_dense_csr_fill, dim3(grid_for(a.build.nrows)), dim3(256), 0, stream, d_args, cursor);
  CUDF_HIP_TRY(hipGetLastError());
}
void launch_dense_count(join_args const& a, join_args* d_args, hipStream_t stream)
{
  hipLaunchKernelGGL(k_store_args<join_args>, dim3(1), dim3(1), 0, stream, a, d_args);
  cudf::detail::prof::scope prof_{"join_count", stream};
  hipLaunchKernelGGL(k_dense_count, dim3(a.nblocks), dim3(256), 0, stream, d_args);
  CUDF_HIP_TRY(hipGetLastError());
}
void launch_dense_retrieve(join_args const& a, join_args* d_args, hipStream_t stream)
{
  hipLaunchKernelGGL(k_store_args<join_args>, dim3(1), dim3(1), 0, stream, a, d_args);
  cudf::detail::prof::scope prof_{"join_retrieve", stream};
  hipLaunchKernelGGL(k_dense_retrieve, dim3(a.nblocks), dim3(256), 0, stream, d_args);
  CUDF_HIP_TRY(hipGetLastError());
}
void launch_dense_big_emit(join_args* d_args, hipStream_t stream)
{
  cudf::detail::prof::scope prof_{"join_retrieve", stream};
  hipLaunchKernelGGL(k_dense_big_emit, dim3(2048), dim3(256), 0, stream, d_args);
  CUDF_HIP_TRY(hipGetLastError());
}
}  // namespace cudf::detail::join
