// SPDX-License-Identifier: Apache-2.0
// The open-addressing set of rows and the small-range integer forms, device side: what the kernels of cudf::filtered_join
// (join/filtered_join_kernels.hip), cudf::distinct_hash_join (join/distinct_join_kernels.hip) and cudf::distinct
// (stream_compaction/distinct_kernels.hip) share. Key loads, the slot sequence with its one build loop (claim) and one lookup loop
// (find), the chunked first pass over the probe rows (probe_chunk) and the ordered compaction of its mask (compact_chunk). What a
// slot holds is each operator's own: filtered_join_impl.hpp (set_args), distinct_join_impl.hpp (map_kind), distinct_impl.hpp.
// Host side: row_set_host.hpp.
#pragma once
#include "device_table.hpp"

#include <cudf/utilities/error.hpp>

#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>

namespace cudf::detail::rowset {

// An unused slot: all ones. No entry has this value: a {hash | row} or {key | row} word ends in a row < 2^31, and an inline 8-byte
// key of this value is kept outside the table by its operator (a flag, a side word or a state word of its own).
constexpr uint64_t EMPTY = ~uint64_t{0};

// what pass 1 loads ahead of one probe row: a single key column's (widened or normalised) bits, or nothing
struct key {
  uint64_t v;
  bool valid;
};
struct no_key {};

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

// The slot sequence. Slot s starts at word slots[s * stride] (stride: 8-byte words per slot; that first word claims the slot), the
// walk starts at `home` and goes on linearly, wrapping at `capacity`. The capacity exceeds the rows inserted (set_capacity,
// row_set_host.hpp), so an EMPTY slot always remains and ends every walk. same(cur) tells whether the non-empty word `cur` holds
// the caller's key.
struct claimed {
  uint64_t slot;  // where the walk ended
  bool inserted;  // this call's CAS put `entry` there; false: same(cur) held for the word found there
  uint64_t cur;   // the word found (EMPTY when inserted)
};

// Build: CAS `entry` into the first empty slot of the walk, unless a slot of the same key comes first. A slot's first word
// changes once, from EMPTY to its entry, so a word that lost the CAS is tested like any other.
template <typename Same>
__device__ __forceinline__ claimed claim(uint64_t* slots, uint64_t stride, uint64_t capacity, uint64_t home, uint64_t entry,
                                         Same const& same)
{
  uint64_t s = home;
  while (true) {
    auto* const word = reinterpret_cast<unsigned long long*>(slots + s * stride);
    uint64_t cur     = gload(slots + s * stride);
    if (cur == EMPTY) {
      cur = atomicCAS(word, static_cast<unsigned long long>(EMPTY), static_cast<unsigned long long>(entry));
      if (cur == EMPTY) return {s, true, cur};
    }
    if (same(cur)) return {s, false, cur};
    s = next_slot(s, capacity);
  }
}

// Lookup (after the build kernel has ended): the first word of the walk for which same(cur) holds, or EMPTY when the key is absent.
template <typename Same>
__device__ __forceinline__ uint64_t find(uint64_t const* slots, uint64_t stride, uint64_t capacity, uint64_t home, Same const& same)
{
  uint64_t s = home;
  while (true) {
    uint64_t const cur = gload(slots + s * stride);
    if (cur == EMPTY || same(cur)) return cur;
    s = next_slot(s, capacity);
  }
}

// Pass 1 over the probe rows, cut into a.nwaves contiguous chunks of a.chunk rows (geometry_of, row_set_host.hpp). Wave `wave`
// answers rows [wave * chunk, + chunk) of a.nrows, UNROLL x 64 rows at a time: every lane first loads its rows' keys with load(row)
// (clamped to the chunk, so that the loads need no branch and stay in flight together), then calls answer(key, row), which tells
// whether the row qualifies and does any store of its own. MASK: the ballot of a 64-row group is its word of a.mask (a word never
// spans two chunks), their sum the chunk's entry of a.counts; the scanned counts and the mask feed compact_chunk.
// `a` is the kernel's own argument struct, read in place: as five values, mask and counts stayed in scalar registers across the
// lookup, which cost the {hash | row} probes an occupancy step.
template <int UNROLL, bool MASK, typename Args, typename Load, typename Answer>
__device__ __forceinline__ void probe_chunk(Args const& a, int64_t wave, Load const& load, Answer const& answer)
{
  int const lane       = threadIdx.x & 63;
  int64_t const begin  = wave * a.chunk;
  int64_t const end    = a.nrows < begin + a.chunk ? a.nrows : begin + a.chunk;
  unsigned long long n = 0;
  for (int64_t r0 = begin; r0 < end; r0 += UNROLL * 64) {
    decltype(load(int64_t{0})) k[UNROLL];
#pragma unroll
    for (int j = 0; j < UNROLL; ++j) {
      int64_t const r = r0 + j * 64 + lane;
      k[j]            = load(r < end ? r : end - 1);
    }
#pragma unroll
    for (int j = 0; j < UNROLL; ++j) {
      int64_t const r = r0 + j * 64 + lane;
      bool const q    = r < end && answer(k[j], r);
      if constexpr (MASK) {
        uint64_t const m = __ballot(q);
        if (r0 + j * 64 < end) {
          if (lane == 0) gstore(a.mask + ((r0 + j * 64) >> 6), m);
          n += __popcll(m);
        }
      }
    }
  }
  if constexpr (MASK) {
    if (lane == 0 && wave < a.nwaves) gstore(a.counts + wave, n);
  }
}

// Ordered compaction of one wave's chunk, rows [wave * chunk, + chunk) of `nrows`: the wave streams the mask words of its chunk, 64
// at a time (one per lane), and calls emit(position, row) in the lane of every set bit, position = the chunk's offset (counts,
// scanned) plus the bits before the row: the words' exclusive prefix over the wave, then each word's bits below the lane (mbcnt).
// No atomics; positions ascend with the rows.
template <typename Emit>
__device__ __forceinline__ void compact_chunk(uint64_t const* mask, unsigned long long const* counts, int64_t wave, int64_t chunk,
                                              int64_t nrows, Emit const& emit)
{
  int const lane      = threadIdx.x & 63;
  int64_t const begin = wave * chunk;
  int64_t const end   = nrows < begin + chunk ? nrows : begin + chunk;
  if (begin >= end) return;
  uint64_t base       = gload(counts + wave);
  int64_t const w_end = (end + 63) >> 6;
  for (int64_t w0 = begin >> 6; w0 < w_end; w0 += 64) {
    uint64_t const word = w0 + lane < w_end ? gload(mask + w0 + lane) : 0;
    uint32_t const c    = __popcll(word);
    uint32_t inc        = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      uint32_t const t = __shfl_up(inc, o);
      if (lane >= o) inc += t;
    }
    uint32_t const exc   = inc - c;
    uint32_t const total = __shfl(inc, 63);
    int const nw         = static_cast<int>(w_end - w0 < 64 ? w_end - w0 : 64);
    for (int k = 0; k < nw; ++k) {
      uint64_t const wk = __shfl(word, k);
      if (wk == 0) continue;  // (uniform)
      uint32_t const at   = __shfl(exc, k);
      uint32_t const rank = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(wk >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(wk), 0u));
      if ((wk >> lane) & 1) emit(base + at + rank, (w0 + k) * 64 + lane);
    }
    base += total;
  }
}

// ------------------------------------------------------------------ launch helpers (host)
// blocks of a grid-stride kernel over n items: at most 16 per CU
inline unsigned grid_for(int64_t n, int threads = 256)
{
  return static_cast<unsigned>(std::clamp<int64_t>((n + threads - 1) / threads, 1, 256 * 16));
}

// f.operator()<W>() for the byte width of an integer key column
template <typename F>
void dispatch_width(int width, F&& f)
{
  switch (width) {
    case 1: return f.template operator()<1>();
    case 2: return f.template operator()<2>();
    case 4: return f.template operator()<4>();
    case 8: return f.template operator()<8>();
    default: CUDF_FAIL("the small-range integer forms take 1-, 2-, 4- or 8-byte keys");
  }
}

// f.operator()<W, SIGNED>()
template <typename F>
void dispatch_int(int width, bool is_signed, F&& f)
{
  dispatch_width(width, [&]<int W>() { return is_signed ? f.template operator()<W, true>() : f.template operator()<W, false>(); });
}

}  // namespace cudf::detail::rowset
