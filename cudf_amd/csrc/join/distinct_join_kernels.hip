// SPDX-License-Identifier: Apache-2.0
// gfx950 kernels of cudf::distinct_hash_join (distinct_join_impl.hpp): the direct-table and hash-map builds, the probe that answers
// one build row per left row, and the ordered compaction of the matches into {left, right} index pairs. Replaces the reference's
// cuco::static_set insert / find and thrust copy_if (cpp/src/join/distinct_hash_join.cu).
#include "distinct_join_impl.hpp"
#include "../common/profiler.hpp"
#include "../common/row_set.hpp"

namespace cudf::detail::djoin {
namespace {

using namespace rowset;

constexpr int THREADS = 256;  // 4 waves per workgroup

// ------------------------------------------------------------------ keys
// The entry of the direct table that the raw bits of a W-byte key select: key - lo, wrapping within W bytes. The wrap makes the
// subtraction right for signed and unsigned columns alike (lo holds the raw bits of the smallest key of the column's own order).
template <int W>
__device__ __forceinline__ uint64_t direct_entry(table_args const& t, device_column const& c, uint64_t raw)
{
  uint64_t const key = c.cls == CLS_BOOL ? static_cast<uint64_t>(raw != 0) : raw;
  uint64_t const off = key - t.lo;
  if constexpr (W == 8) return off;
  else return off & ((uint64_t{1} << (8 * W)) - 1);
}

// One store per wave of the row a lane holds (JoinNoMatch: none) into a side word: whichever lane comes first.
__device__ __forceinline__ void store_side(size_type* p, size_type row)
{
  uint64_t const m = __ballot(row != JoinNoMatch);
  if (m != 0 && static_cast<int>(threadIdx.x & 63) == __ffsll(static_cast<unsigned long long>(m)) - 1) gstore(p, row);
}

// ------------------------------------------------------------------ builds
// Plain stores: with duplicate keys the racing stores leave one of the rows.
template <int W>
__global__ void __launch_bounds__(THREADS) k_build_direct(table_args a)
{
  device_column const& c = a.build.col[0];
  int64_t const n        = a.build.nrows;
  int64_t const stride   = static_cast<int64_t>(gridDim.x) * blockDim.x;
  size_type null_row     = JoinNoMatch;
  for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < n; i += stride) {
    if (!col_is_valid(c, i)) {  // never inserted: a NULL probe key reads side[0] instead
      null_row = static_cast<size_type>(i);
      continue;
    }
    uint64_t const off = direct_entry<W>(a, c, load_int<W, false>(c, i));
    if (off < a.range) gstore(a.direct + off, static_cast<size_type>(i));  // (lo and range cover every valid build key)
  }
  if (a.nulls_equal) store_side(a.side, null_row);
}

template <int W>
__global__ void __launch_bounds__(THREADS) k_build_key(table_args a)
{
  device_column const& c = a.build.col[0];
  int64_t const n        = a.build.nrows;
  int64_t const stride   = static_cast<int64_t>(gridDim.x) * blockDim.x;
  size_type null_row = JoinNoMatch, sentinel_row = JoinNoMatch;
  for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < n; i += stride) {
    if (!col_is_valid(c, i)) {
      null_row = static_cast<size_type>(i);
      continue;
    }
    uint64_t const key = normalize_key_bits(load_bits<W>(c, i), c.cls);
    if (W == 8 && key == EMPTY) {  // the one value a slot's key word cannot hold
      sentinel_row = static_cast<size_type>(i);
      continue;
    }
    // the word that claims the slot: the key itself (8 bytes), or the key above the row (4 bytes; a row is < 2^31, so no entry
    // equals EMPTY). A duplicate key: the row that claimed the slot stays.
    uint64_t const entry = W == 8 ? key : (key << 32) | static_cast<uint32_t>(i);
    auto const got       = claim(a.slots, W == 8 ? 2 : 1, a.capacity, home_slot(murmur3_32_bits(key, W, 0), a.capacity), entry,
                                 [&](uint64_t cur) { return (W == 8 ? cur : cur >> 32) == key; });
    // the 16-byte slot takes its row next to the key
    if (W == 8 && got.inserted) gstore(reinterpret_cast<uint32_t*>(a.slots + 2 * got.slot + 1), static_cast<uint32_t>(i));
  }
  if (a.nulls_equal) store_side(a.side, null_row);
  if constexpr (W == 8) store_side(a.side + 1, sentinel_row);
}

__global__ void __launch_bounds__(THREADS) k_build_rows(table_args a)
{
  int64_t const n      = a.build.nrows;
  int64_t const stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  bool const eq        = a.nulls_equal != 0;
  for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < n; i += stride) {
    if (!eq && row_has_null(a.build, i)) continue;  // null_equality::UNEQUAL: such a row equals no row
    uint32_t const h = row_hash(a.build, i, 0);
    claim(a.slots, 1, a.capacity, home_slot(h, a.capacity), (static_cast<uint64_t>(h) << 32) | static_cast<uint32_t>(i), [&](uint64_t cur) {
      return (cur >> 32) == h && rows_equal(a.build, static_cast<uint32_t>(cur), a.build, i, eq);  // a duplicate row
    });
  }
}

// ------------------------------------------------------------------ the probe: one build row per left row
// The build row of a {key or hash | row} word that rowset::find returned; EMPTY: the key is absent.
__device__ __forceinline__ size_type row_of(uint64_t word)
{
  return word == EMPTY ? JoinNoMatch : static_cast<size_type>(static_cast<uint32_t>(word));
}

// load(r): what the lookup needs of left row r, fetched ahead; lookup(key, r): the equal build row or JoinNoMatch.
template <int W>
struct direct_lookup {
  static constexpr int UNROLL = 8;
  probe_args const& a;
  __device__ key load(int64_t r) const { return {load_int<W, false>(a.probe.col[0], r), col_is_valid(a.probe.col[0], r)}; }
  __device__ size_type lookup(key k, int64_t) const
  {
    if (!k.valid) return gload(a.t.side);
    uint64_t const off = direct_entry<W>(a.t, a.probe.col[0], k.v);
    if (off >= a.t.range) return JoinNoMatch;  // outside the build keys' range: no memory access
    return gload(a.t.direct + off);
  }
};

template <int W>
struct key_lookup {
  static constexpr int UNROLL = 4;
  probe_args const& a;
  __device__ key load(int64_t r) const
  {
    device_column const& c = a.probe.col[0];
    return {normalize_key_bits(load_bits<W>(c, r), c.cls), col_is_valid(c, r)};
  }
  __device__ size_type lookup(key k, int64_t) const
  {
    if (!k.valid) return gload(a.t.side);
    if (W == 8 && k.v == EMPTY) return gload(a.t.side + 1);
    uint64_t s = home_slot(murmur3_32_bits(k.v, W, 0), a.t.capacity);
    if constexpr (W == 8) {
      // rowset::find's walk, written out: it loads one word per slot, and this slot's key and row come in one 16-byte load
      while (true) {
        u64x2 const cur = gload(reinterpret_cast<u64x2 const*>(a.t.slots) + s);
        if (cur.x == k.v) return static_cast<size_type>(static_cast<uint32_t>(cur.y));
        if (cur.x == EMPTY) return JoinNoMatch;
        s = next_slot(s, a.t.capacity);
      }
    } else {
      return row_of(find(a.t.slots, 1, a.t.capacity, s, [&](uint64_t cur) { return (cur >> 32) == k.v; }));
    }
  }
};

struct rows_lookup {
  static constexpr int UNROLL = 1;
  probe_args const& a;
  __device__ no_key load(int64_t) const { return {}; }
  __device__ size_type lookup(no_key, int64_t r) const
  {
    bool const eq = a.t.nulls_equal != 0;
    if (!eq && row_has_null(a.probe, r)) return JoinNoMatch;
    uint32_t const h = row_hash(a.probe, r, 0);
    return row_of(find(a.t.slots, 1, a.t.capacity, home_slot(h, a.t.capacity), [&](uint64_t cur) {
      return (cur >> 32) == h && rows_equal(a.probe, r, a.t.build, static_cast<uint32_t>(cur), eq);
    }));
  }
};

// rowset::probe_chunk over the left table: each row is looked up and the row found written, coalesced. COMPACT (inner_join): with
// the mask words and the chunk counts of the rows that found one.
template <bool COMPACT, typename Lookup>
__global__ void __launch_bounds__(THREADS) k_probe(probe_args a)
{
  Lookup const p{a};
  int64_t const wave = static_cast<int64_t>(blockIdx.x) * (THREADS / 64) + (threadIdx.x >> 6);
  probe_chunk<Lookup::UNROLL, COMPACT>(
    a, wave, [&](int64_t r) { return p.load(r); },
    [&](auto const& k, int64_t r) {
      size_type const f = p.lookup(k, r);
      gstore(a.found + r, f);
      return f != JoinNoMatch;
    });
}

// ------------------------------------------------------------------ inner_join, pass 2: ordered compaction of the pairs
__global__ void __launch_bounds__(THREADS) k_compact_pairs(probe_args a)
{
  int64_t const wave = static_cast<int64_t>(blockIdx.x) * (THREADS / 64) + (threadIdx.x >> 6);
  compact_chunk(a.mask, a.counts, wave, a.chunk, a.nrows, [&](uint64_t o, int64_t row) {
    if (o >= a.out_capacity) return;
    gstore(a.out_left + o, static_cast<size_type>(row));
    gstore(a.out_right + o, gload(a.found + row));
  });
}

template <bool COMPACT>
void launch_probe_of(probe_args const& a, hipStream_t stream)
{
  dim3 const grid(a.nwaves / (THREADS / 64)), block(THREADS);
  if (a.t.table_form == static_cast<int32_t>(form::direct)) {
    dispatch_width(a.probe.col[0].width, [&]<int W>() { hipLaunchKernelGGL((k_probe<COMPACT, direct_lookup<W>>), grid, block, 0, stream, a); });
  } else if (a.t.kind == static_cast<int32_t>(map_kind::key4)) {
    hipLaunchKernelGGL((k_probe<COMPACT, key_lookup<4>>), grid, block, 0, stream, a);
  } else if (a.t.kind == static_cast<int32_t>(map_kind::key8)) {
    hipLaunchKernelGGL((k_probe<COMPACT, key_lookup<8>>), grid, block, 0, stream, a);
  } else {
    hipLaunchKernelGGL((k_probe<COMPACT, rows_lookup>), grid, block, 0, stream, a);
  }
}
}  // namespace

void launch_build(table_args const& a, hipStream_t stream)
{
  bool const direct = a.table_form == static_cast<int32_t>(form::direct);
  cudf::detail::prof::scope prof_{direct ? "djoin_build_direct" : "djoin_build_map", stream};
  dim3 const grid(grid_for(a.build.nrows, THREADS)), block(THREADS);
  if (direct) {
    dispatch_width(a.build.col[0].width, [&]<int W>() { hipLaunchKernelGGL((k_build_direct<W>), grid, block, 0, stream, a); });
  } else if (a.kind == static_cast<int32_t>(map_kind::key4)) {
    hipLaunchKernelGGL((k_build_key<4>), grid, block, 0, stream, a);
  } else if (a.kind == static_cast<int32_t>(map_kind::key8)) {
    hipLaunchKernelGGL((k_build_key<8>), grid, block, 0, stream, a);
  } else {
    hipLaunchKernelGGL(k_build_rows, grid, block, 0, stream, a);
  }
  CUDF_HIP_TRY(hipGetLastError());
}

void launch_probe(probe_args const& a, hipStream_t stream)
{
  CUDF_EXPECTS(a.nwaves % (THREADS / 64) == 0, "distinct_hash_join: the probe takes whole workgroups of waves");
  bool const direct = a.t.table_form == static_cast<int32_t>(form::direct);
  cudf::detail::prof::scope prof_{direct ? "djoin_probe_direct" : "djoin_probe_map", stream};
  if (a.mask != nullptr) launch_probe_of<true>(a, stream);
  else launch_probe_of<false>(a, stream);
  CUDF_HIP_TRY(hipGetLastError());
}

void launch_compact(probe_args const& a, hipStream_t stream)
{
  cudf::detail::prof::scope prof_{"djoin_compact", stream};
  hipLaunchKernelGGL(k_compact_pairs, dim3(a.nwaves / (THREADS / 64)), dim3(THREADS), 0, stream, a);
  CUDF_HIP_TRY(hipGetLastError());
}

}  // namespace cudf::detail::djoin
