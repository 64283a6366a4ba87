// SPDX-License-Identifier: Apache-2.0
// gfx950 kernels of the open-addressing table in HBM (engine.hpp join_args::table): build, count pass, retrieve pass.
#include "join_device.hpp"
#include "../common/profiler.hpp"

#include <cudf/utilities/error.hpp>

namespace cudf::detail::join {
namespace {

// 64-bit row hash of the join keys (the engine's own; results do not depend on it). A NULL element hashes
// to a constant so that NULL == NULL rows meet under null_equality::EQUAL.
__device__ __forceinline__ uint64_t join_row_hash(device_table const& t, int64_t i, bool check_nulls)
{
  uint64_t h = 0x9e3779b97f4a7c15ull;
  for (int c = 0; c < t.ncols; ++c) {
    uint64_t bits = 0x6a09e667f3bcc909ull;
    if (!check_nulls || col_is_valid(t.col[c], i)) bits = normalize_key_bits(col_load_bits(t.col[c], i), t.col[c].cls);
    h = mix64(h ^ bits);
  }
  return h;
}
__device__ __forceinline__ uint64_t hash64_single(uint64_t key) { return mix64(0x9e3779b97f4a7c15ull ^ key); }

__device__ __forceinline__ uint64_t home_slot(uint64_t h, join_args const& a)
{
  return (static_cast<uint64_t>(static_cast<uint32_t>(h)) * a.capacity) >> 32;  // capacity < 2^32
}
__device__ __forceinline__ uint64_t make_entry(uint64_t h, int64_t row)
{
  return ((h >> 32) << 32) | static_cast<uint32_t>(row);
}

// Probe sequence of a row hash, in STEPS of 16 bytes (an aligned pair of 8-byte slots): SEQ_LINEAR consecutive
// steps from the home step, then hops of a key-dependent stride coprime to the number of steps (the hops reach every
// step). Plain linear probing lets ONE heavily duplicated build key poison its neighbourhood: 100,000 equal keys form a
// 100,000-slot run that every probe with a home slot inside it walks to the end (0.25 % of 100M probes: 1 s). With the
// hops, the duplicates beyond the window sit on their key's own trail. Build, count and retrieve passes walk the same
// sequence; an entry always takes the first empty slot of its sequence, so a walk may stop at the first empty slot.
constexpr uint32_t SEQ_LINEAR = 16;
__device__ __noinline__ uint64_t seq_stride(uint64_t h, uint64_t nsteps)
{
  if (nsteps <= 2) return 1;
  uint64_t s = 1 + mix64(h ^ 0x2545f4914f6cdd1dull) % (nsteps - 1);
  for (;;) {
    uint64_t x = s, y = nsteps;
    while (y != 0) {
      uint64_t const t = x % y;
      x                = y;
      y                = t;
    }
    if (x == 1) return s;
    s = s + 1 >= nsteps ? 1 : s + 1;
  }
}
// Advances from step number n (the home step st0 is number 0) and updates n; `stride` caches seq_stride (0 = not computed
// yet). Hop positions that fall back into the linear window were visited already: they keep their number but are
// passed over (a probe that walked them twice counted their matches twice). Tiny tables stay linear.
__device__ __forceinline__ uint64_t seq_next(uint64_t st, uint32_t& n, uint64_t h, uint64_t nsteps, uint64_t& stride, uint64_t st0)
{
  if (n + 1 < SEQ_LINEAR || nsteps <= 4 * SEQ_LINEAR) {
    ++n;
    return st + 1 == nsteps ? 0 : st + 1;
  }
  if (stride == 0) stride = seq_stride(h, nsteps);
  for (;;) {
    st += stride;
    if (st >= nsteps) st -= nsteps;
    ++n;
    uint64_t const d = st >= st0 ? st - st0 : st + nsteps - st0;
    if (d >= SEQ_LINEAR) return st;
  }
}
// position number n of the sequence that starts at step st0 (n: a number seq_next stopped at)
__device__ __forceinline__ uint64_t seq_at(uint64_t st0, uint32_t n, uint64_t h, uint64_t nsteps, uint64_t& stride)
{
  if (n < SEQ_LINEAR || nsteps <= 4 * SEQ_LINEAR) return (st0 + n) % nsteps;
  if (stride == 0) stride = seq_stride(h, nsteps);
  // n < 2^20, stride < 2^32: no overflow
  return (static_cast<uint64_t>(n - (SEQ_LINEAR - 1)) * stride + (st0 + SEQ_LINEAR - 1) % nsteps) % nsteps;
}

// ------------------------------------------------------------------ build
template <bool SINGLE64>
__global__ void __launch_bounds__(256) k_build(join_args const* __restrict__ ap)
{
  join_args const& a = *ap;
  int64_t const n      = a.build.nrows;
  int64_t const stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  uint64_t const cap   = a.capacity;
  uint64_t const* keys = SINGLE64 ? static_cast<uint64_t const*>(a.build.col[0].head) + a.build.col[0].offset : nullptr;
  for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < n; i += stride) {
    uint64_t h;
    if constexpr (SINGLE64) {
      // with null_equality::UNEQUAL a NULL key row is never inserted
      if (a.check_nulls && a.build.col[0].mask != nullptr && !col_is_valid(a.build.col[0], i)) continue;
      h = hash64_single(gload(keys + i));
    } else {
      // null_equality::UNEQUAL: rows containing a NULL can never match and are not inserted
      // (reference hash_join.cu:77-84, join_common_utils.cuh:36-47)
      if (a.check_nulls && !a.nulls_equal && row_has_null(a.build, i)) continue;
      h = join_row_hash(a.build, i, a.check_nulls);
    }
    uint64_t const entry = make_entry(h, i);
    uint64_t const home  = home_slot(h, a);
    uint64_t const nsteps = cap >> 1;                    // 8-byte slots: a step is an aligned pair of slots (capacity is even)
    uint64_t const st0   = home >> 1;
    uint64_t st = st0, stride = 0;
    uint32_t n  = 0;                                     // step number; the slots of steps [0, n) are known to be occupied
    // The home slot is tried with the compare-and-swap itself (empty three times out of four); further slots are read
    // first and only an empty one is claimed: a walk over occupied slots costs loads, not atomics.
    bool blind = true;
    // Hints {44 hash bits | n}: "the first n steps of this hash's sequence are full". An insert that has walked
    // BUILD_SKIP_AFTER steps looks its hint up and jumps ahead; one that ended beyond that leaves a hint. Hints are
    // advisory: any value ever stored is true (slots are never emptied during the build), a racing store can only lose
    // some of the shortcut. (Two different heavy keys that agree in 44 hash bits would share hints: 2^-44 per pair.)
    uint64_t* const hint    = a.build_skip + ((h >> 12) & (BUILD_SKIP_ENTRIES - 1));
    uint64_t const hint_tag = (h >> 20) << 20;
    for (;;) {
      bool done = false;
      for (int q = n == 0 ? static_cast<int>(home & 1) : 0; q < 2; ++q) {  // (the home slot may be the second of its pair)
        uint64_t* const where = a.table + st * 2 + q;
        if (blind || __hip_atomic_load(where, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == EMPTY_SLOT) {
          blind = false;
          if (atomicCAS(reinterpret_cast<unsigned long long*>(where), EMPTY_SLOT, static_cast<unsigned long long>(entry)) == EMPTY_SLOT) {
            done = true;
            break;
          }
        }
      }
      if (done) break;
      uint32_t const before = n;
      st = seq_next(st, n, h, nsteps, stride, st0);
      if ((before / BUILD_SKIP_AFTER) != (n / BUILD_SKIP_AFTER)) {  // a long walk (many equal keys): is a longer full prefix known?
        uint64_t const e = __hip_atomic_load(hint, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        uint32_t const d = static_cast<uint32_t>(e & 0xfffffull);
        if ((e >> 20 << 20) == hint_tag && d > n) {
          n  = d;
          st = seq_at(st0, n, h, nsteps, stride);
        }
      }
    }
    if (n >= BUILD_SKIP_AFTER && n < 0xfffffu) {
      uint64_t const e = __hip_atomic_load(hint, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if ((e >> 20 << 20) != hint_tag || (e & 0xfffffull) < n) __hip_atomic_store(hint, hint_tag | n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// ------------------------------------------------------------------ probe: count pass
// One workgroup per contiguous chunk of probe rows; R rows per lane with their first loads issued together. Writes the per-row match cache and the
// per-workgroup pair count.
// MODE 0: any key columns (row hash, rows_equal).
// MODE 1: one 8-byte integer key whose NULLs never match, 8-byte slots {tag | row}: candidates are verified against
//         the build key column.
// The pass is bound by the NUMBER of random memory requests (1.2 G requests in 18.6 ms = 66 G/s, the rate the
// random-load microbenchmark reaches), not by their dependency chains: reading a 64-byte window of slots per row with
// four 16-byte loads measured SLOWER (21.9 ms). So 8-byte slots are walked in aligned PAIRS - one 16-byte request
// covers two slots - and the planner keeps the table at load <= 0.25, where a walk to the first empty slot is 1.4
// slots on average instead of 2.5.
constexpr int MODE_GENERIC = 0, MODE_KEY64 = 1;

template <int MODE>
__global__ void __launch_bounds__(256) k_probe_count(join_args const* __restrict__ ap)
{
  join_args const& a = *ap;
  __shared__ unsigned long long s_total;
  constexpr bool KEY64 = MODE != MODE_GENERIC;
  int64_t const n    = a.probe.nrows;
  uint64_t const cap = a.capacity;
  int const kind     = a.kind;
  uint64_t const nsteps = cap >> 1;  // 16-byte steps in the table: 8-byte slots, walked in aligned pairs (capacity is even)
  uint64_t const* pkeys = KEY64 ? static_cast<uint64_t const*>(a.probe.col[0].head) + a.probe.col[0].offset : nullptr;
  uint64_t const* bkeys = KEY64 ? static_cast<uint64_t const*>(a.build.col[0].head) + a.build.col[0].offset : nullptr;
  u64x2 const* table16  = reinterpret_cast<u64x2 const*>(a.table);
  bitmask_type const* probe_mask = (KEY64 && a.check_nulls) ? a.probe.col[0].mask : nullptr;
  int64_t const probe_off        = KEY64 ? a.probe.col[0].offset : 0;
  if (threadIdx.x == 0) s_total = 0;
  __syncthreads();
  constexpr int R = 4;
  unsigned long long local_count = 0;
  {
    int64_t const begin = static_cast<int64_t>(blockIdx.x) * a.chunk;
    int64_t const end   = min(n, begin + a.chunk);
    for (int64_t base = begin; base < end; base += static_cast<int64_t>(blockDim.x) * R) {
      int64_t j[R];
      bool live[R], active[R];
      uint64_t h[R], pkey[R], slot[R];
      u64x2 v0[R];
#pragma unroll
      for (int k = 0; k < R; ++k) {
        j[k]      = base + static_cast<int64_t>(k) * blockDim.x + threadIdx.x;
        live[k]   = j[k] < end;
        active[k] = live[k];
        h[k] = pkey[k] = 0;
        if (live[k]) {
          if constexpr (KEY64) {
            if (probe_mask != nullptr && !((gload(probe_mask + ((probe_off + j[k]) >> 5)) >> ((probe_off + j[k]) & 31)) & 1u)) {
              active[k] = false;  // NULL probe key under null_equality::UNEQUAL matches nothing
            } else {
              pkey[k] = gload(pkeys + j[k]);
              h[k]    = hash64_single(pkey[k]);
            }
          } else if (a.check_nulls && !a.nulls_equal && row_has_null(a.probe, j[k])) {
            active[k] = false;  // matches nothing (null_equality::UNEQUAL)
          } else {
            h[k] = join_row_hash(a.probe, j[k], a.check_nulls);
          }
        }
        slot[k] = active[k] ? home_slot(h[k], a) : 0;
      }
#pragma unroll
      for (int k = 0; k < R; ++k) {
        v0[k] = u64x2{EMPTY_SLOT, EMPTY_SLOT};
        if (active[k]) v0[k] = gload(table16 + (slot[k] >> 1));
      }
#pragma unroll
      for (int k = 0; k < R; ++k) {
        if (!live[k]) continue;
        uint32_t const tag = static_cast<uint32_t>(h[k] >> 32);
        uint32_t first     = MATCH_NONE;
        unsigned int cnt   = 0;
        // one table entry: false at the first empty slot
        auto visit = [&](uint64_t ee) -> bool {
          if (ee == EMPTY_SLOT) return false;
          bool match = false;
          if (static_cast<uint32_t>(ee >> 32) == tag) {
            size_type const brow = static_cast<size_type>(static_cast<uint32_t>(ee));
            if constexpr (MODE == MODE_KEY64) match = gload(bkeys + brow) == pkey[k];
            else match = rows_equal(a.probe, j[k], a.build, brow, a.nulls_equal != 0);
          }
          if (match) {
            if (cnt == 0) first = static_cast<uint32_t>(ee);
            ++cnt;
          }
          return true;
        };
        if (active[k]) {
          u64x2 v     = v0[k];
          uint64_t st = slot[k] >> 1, stride = 0;
          uint32_t ns = 0;              // step number along the key's probe sequence (seq_next)
          bool skip   = slot[k] & 1;    // the home slot is the second of its pair
          for (;;) {
            if (!skip && !visit(v.x)) break;
            skip = false;
            if (!visit(v.y)) break;
            st = seq_next(st, ns, h[k], nsteps, stride, slot[k] >> 1);
            v  = gload(table16 + st);
          }
        }
        local_count += count_row(a, kind, j[k], cnt > 1 ? (first | MATCH_MULTI) : first, cnt);
      }
    }
  }
  count_block_total(local_count, &s_total, a.block_counts);
}

// ------------------------------------------------------------------ probe: retrieve pass
// Streams the match cache. Rows with zero or one match are emitted straight from it; rows with several matches walk
// the table again. Output slots come from a workgroup-local LDS cursor (64-lane ballot + popcount prefix, one LDS
// atomic per wave and round) on top of the chunk's exclusive offset from the count pass: no global atomics (a
// single global counter was measured 16x slower than the whole count pass: same-address atomics serialise).
template <int MODE>
__global__ void __launch_bounds__(256) k_probe_retrieve(join_args const* __restrict__ ap)
{
  join_args const& a = *ap;
  __shared__ unsigned long long s_cursor;
  int64_t const n    = a.probe.nrows;
  uint64_t const cap = a.capacity;
  int const kind     = a.kind;
  constexpr bool KEY64 = MODE != MODE_GENERIC;
  uint64_t const* pkeys = KEY64 ? static_cast<uint64_t const*>(a.probe.col[0].head) + a.probe.col[0].offset : nullptr;
  uint64_t const* bkeys = KEY64 ? static_cast<uint64_t const*>(a.build.col[0].head) + a.build.col[0].offset : nullptr;
  if (threadIdx.x == 0) s_cursor = a.block_counts[blockIdx.x];
  __syncthreads();
  int const lane = threadIdx.x & 63;
  auto emit = [&](bool want, size_type prow, size_type brow) { wave_emit_pair(a, kind, want, prow, brow, &s_cursor, lane); };
  int64_t const begin = static_cast<int64_t>(blockIdx.x) * a.chunk;
  int64_t const end   = min(n, begin + a.chunk);
  for (int64_t j0 = begin; j0 < end; j0 += blockDim.x) {  // every lane of a wave iterates together (ballots)
    int64_t const j   = j0 + threadIdx.x;
    bool const live   = j < end;
    uint32_t const c  = live ? gload(a.match_cache + j) : MATCH_NONE;
    bool const none   = c == MATCH_NONE;
    bool const multi  = !none && (c & MATCH_MULTI);
    size_type prow    = static_cast<size_type>(j + a.probe_row_base);
    uint64_t pkey     = 0;
    // zero or one match: straight from the cache
    emit(live && !none && !multi, prow, static_cast<size_type>(c & ~MATCH_MULTI));
    if (kind != 0) emit(live && none, prow, JoinNoMatch);
    // several matches: walk the table again (rare with unique build keys)
    if (__any(multi)) {
      uint64_t h = 0;
      if (multi) {
        if constexpr (KEY64) {
          pkey = gload(pkeys + j);
          h = hash64_single(pkey);
        } else {
          h = join_row_hash(a.probe, j, a.check_nulls);
        }
      }
      uint64_t slot      = multi ? home_slot(h, a) : 0;
      uint32_t const tag = static_cast<uint32_t>(h >> 32);
      bool walking       = multi;
      uint64_t const nsteps = cap >> 1;  // the sequence advances in 16-byte steps: aligned pairs of 8-byte slots
      uint64_t const st0 = slot >> 1;
      uint64_t stride    = 0;
      uint32_t ns        = 0;
      while (__any(walking)) {
        bool match     = false;
        size_type brow = 0;
        if (walking) {
          uint64_t const e = gload(a.table + slot);
          if (e == EMPTY_SLOT) {
            walking = false;
          } else {
            brow = static_cast<size_type>(static_cast<uint32_t>(e));
            if (static_cast<uint32_t>(e >> 32) == tag) {
              if constexpr (MODE == MODE_KEY64) match = gload(bkeys + brow) == pkey;
              else match = rows_equal(a.probe, j, a.build, brow, a.nulls_equal != 0);
            }
            if ((slot & 1) == 0) slot += 1;  // the second slot of the pair, then the first of the next step
            else slot = seq_next(slot >> 1, ns, h, nsteps, stride, st0) * 2;
          }
        }
        emit(match, prow, brow);
      }
    }
  }
}
}  // namespace

void launch_build(join_args const& a, join_args* d_args, hipStream_t stream)
{
  hipLaunchKernelGGL(k_store_args<join_args>, dim3(1), dim3(1), 0, stream, a, d_args);
  cudf::detail::prof::scope prof_{"join_build", stream};
  if (a.single64) hipLaunchKernelGGL(k_build<true>, dim3(grid_for(a.build.nrows)), dim3(256), 0, stream, d_args);
  else hipLaunchKernelGGL(k_build<false>, dim3(grid_for(a.build.nrows)), dim3(256), 0, stream, d_args);
  CUDF_HIP_TRY(hipGetLastError());
}
void launch_count(join_args const& a, join_args* d_args, hipStream_t stream)
{
  CUDF_EXPECTS(a.table != nullptr && a.dense_head == nullptr, "hash join: the open-addressing table's passes need that table");
  hipLaunchKernelGGL(k_store_args<join_args>, dim3(1), dim3(1), 0, stream, a, d_args);
  cudf::detail::prof::scope prof_{"join_count", stream};
  if (a.single64) hipLaunchKernelGGL((k_probe_count<MODE_KEY64>), dim3(a.nblocks), dim3(256), 0, stream, d_args);
  else hipLaunchKernelGGL((k_probe_count<MODE_GENERIC>), dim3(a.nblocks), dim3(256), 0, stream, d_args);
  CUDF_HIP_TRY(hipGetLastError());
}
void launch_retrieve(join_args const& a, join_args* d_args, hipStream_t stream)
{
  CUDF_EXPECTS(a.table != nullptr && a.dense_head == nullptr, "hash join: the open-addressing table's passes need that table");
  hipLaunchKernelGGL(k_store_args<join_args>, dim3(1), dim3(1), 0, stream, a, d_args);
  cudf::detail::prof::scope prof_{"join_retrieve", stream};
  if (a.single64) hipLaunchKernelGGL((k_probe_retrieve<MODE_KEY64>), dim3(a.nblocks), dim3(256), 0, stream, d_args);
  else hipLaunchKernelGGL((k_probe_retrieve<MODE_GENERIC>), dim3(a.nblocks), dim3(256), 0, stream, d_args);
  CUDF_HIP_TRY(hipGetLastError());
}
}  // namespace cudf::detail::join
