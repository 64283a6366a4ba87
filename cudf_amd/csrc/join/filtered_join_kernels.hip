// SPDX-License-Identifier: Apache-2.0
// gfx950 kernels of cudf::filtered_join (filtered_join_impl.hpp): the bitmap and hash-set builds, the probes that answer one bit per
// left row, and the ordered compaction of those bits into ascending row indices. Replaces the reference's cuco::static_set
// insert / contains and thrust::copy_if over a counting iterator (cpp/src/join/filtered_join/filtered_join.cu, semi_anti_join).
#include "filtered_join_impl.hpp"
#include "../common/profiler.hpp"
#include "../common/row_set.hpp"
#include "../common/row_set_host.hpp"

#include <mutex>

namespace cudf::detail::fjoin {
namespace {

using namespace rowset;

constexpr int PROBE_THREADS = 256;   // pass 1 (global bitmap, set) and pass 2: 4 waves per workgroup
constexpr int LDS_THREADS   = 1024;  // pass 1 from an LDS bitmap: 16 waves share one copy
constexpr int LDS_BYTES_MAX = 128 * 1024;

// ------------------------------------------------------------------ builds
template <int W, bool SIGNED>
__global__ void __launch_bounds__(256) k_bitmap_build(bitmap_args a)
{
  int64_t const stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  bool seen_null       = false;
  for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < a.nrows; i += stride) {
    if (!col_is_valid(a.key, i)) {  // never inserted: a NULL probe key asks probe_args::null_match instead
      seen_null = true;
      continue;
    }
    uint64_t const off = load_int<W, SIGNED>(a.key, i) - a.lo;  // < range: lo and range cover every valid build key
    if (off < a.range) atomicOr(a.bits + (off >> 5), 1u << (off & 31));
  }
  if (__any(seen_null) && (threadIdx.x & 63) == 0) gstore(a.seen_null, 1);
}

template <int W>
__global__ void __launch_bounds__(256) k_set_build_inline(set_args a)
{
  device_column const& c = a.build.col[0];
  int64_t const n        = a.build.nrows;
  int64_t const stride   = static_cast<int64_t>(gridDim.x) * blockDim.x;
  bool seen_null = false, seen_sentinel = false;
  for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < n; i += stride) {
    if (!col_is_valid(c, i)) {
      seen_null = true;
      continue;
    }
    uint64_t const key = normalize_key_bits(load_bits<W>(c, i), c.cls);
    if (key == EMPTY) {  // (8-byte keys only) the one value a slot cannot hold
      seen_sentinel = true;
      continue;
    }
    claim(a.slots, 1, a.capacity, home_slot(murmur3_32_bits(key, W, 0), a.capacity), key, [&](uint64_t cur) { return cur == key; });
  }
  if (__any(seen_null) && (threadIdx.x & 63) == 0) gstore(a.seen_null, 1);
  if (__any(seen_sentinel) && (threadIdx.x & 63) == 0) gstore(a.seen_sentinel, 1);
}

__global__ void __launch_bounds__(256) k_set_build_rows(set_args a)
{
  int64_t const n      = a.build.nrows;
  int64_t const stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  bool const eq        = a.nulls_equal != 0;
  for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < n; i += stride) {
    if (!eq && row_has_null(a.build, i)) continue;  // null_equality::UNEQUAL: such a row equals no row
    uint32_t const h = row_hash(a.build, i, 0);
    claim(a.slots, 1, a.capacity, home_slot(h, a.capacity), (static_cast<uint64_t>(h) << 32) | static_cast<uint32_t>(i), [&](uint64_t cur) {
      return (cur >> 32) == h && rows_equal(a.build, static_cast<uint32_t>(cur), a.build, i, eq);  // a distinct set
    });
  }
}

// ------------------------------------------------------------------ pass 1: one bit per left row
// rowset::probe_chunk over wave `wave`'s chunk of the left table, with p.load(row) and p.test(key, row): a row qualifies when it
// has a match (semi) or has none (anti).
template <int UNROLL, typename Probe>
__device__ __forceinline__ void probe_wave(probe_args const& a, int64_t wave, Probe const& p)
{
  bool const anti = a.anti != 0;
  probe_chunk<UNROLL, true>(
    a, wave, [&](int64_t r) { return p.load(r); },
    [&](auto const& k, int64_t r) { return p.test(k, r) != anti; });
}

template <int W, bool SIGNED, bool LDS>
struct bitmap_probe {
  probe_args const& a;
  uint32_t const* lds;
  __device__ key load(int64_t r) const { return {load_int<W, SIGNED>(a.probe.col[0], r), col_is_valid(a.probe.col[0], r)}; }
  __device__ bool test(key k, int64_t) const
  {
    if (!k.valid) return a.null_match != 0;
    uint64_t const off = k.v - a.bm.lo;
    if (off >= a.bm.range) return false;  // outside the build keys' range: no memory access
    uint32_t const word = LDS ? lds[off >> 5] : gload(a.bm.bits + (off >> 5));
    return (word >> (off & 31)) & 1u;
  }
};

template <int W, bool SIGNED>
__global__ void __launch_bounds__(PROBE_THREADS) k_bitmap_probe(probe_args a)
{
  int64_t const wave = static_cast<int64_t>(blockIdx.x) * (PROBE_THREADS / 64) + (threadIdx.x >> 6);
  probe_wave<8>(a, wave, bitmap_probe<W, SIGNED, false>{a, nullptr});
}

template <int W, bool SIGNED>
__global__ void __launch_bounds__(LDS_THREADS) k_bitmap_probe_lds(probe_args a)
{
  extern __shared__ __attribute__((aligned(16))) uint32_t s_bits[];
  // the bitmap's words, 16 bytes at a time (the buffer and the LDS copy are whole 16-byte units)
  int64_t const units = static_cast<int64_t>((a.bm.range + 127) >> 7);
  for (int64_t u = threadIdx.x; u < units; u += LDS_THREADS)
    reinterpret_cast<u32x4*>(s_bits)[u] = gload(reinterpret_cast<u32x4 const*>(a.bm.bits) + u);
  __syncthreads();
  int64_t const wave = static_cast<int64_t>(blockIdx.x) * (LDS_THREADS / 64) + (threadIdx.x >> 6);
  probe_wave<8>(a, wave, bitmap_probe<W, SIGNED, true>{a, s_bits});
}

template <int W>
struct set_probe_inline {
  probe_args const& a;
  __device__ key load(int64_t r) const
  {
    device_column const& c = a.probe.col[0];
    return {normalize_key_bits(load_bits<W>(c, r), c.cls), col_is_valid(c, r)};
  }
  __device__ bool test(key k, int64_t) const
  {
    if (!k.valid) return a.null_match != 0;
    if (k.v == EMPTY) return a.sentinel_match != 0;
    uint64_t const home = home_slot(murmur3_32_bits(k.v, W, 0), a.set.capacity);
    return find(a.set.slots, 1, a.set.capacity, home, [&](uint64_t cur) { return cur == k.v; }) != EMPTY;
  }
};

struct set_probe_rows {
  probe_args const& a;
  __device__ no_key load(int64_t) const { return {}; }
  __device__ bool test(no_key, int64_t r) const
  {
    bool const eq = a.set.nulls_equal != 0;
    if (!eq && row_has_null(a.probe, r)) return false;
    uint32_t const h = row_hash(a.probe, r, 0);
    return find(a.set.slots, 1, a.set.capacity, home_slot(h, a.set.capacity), [&](uint64_t cur) {
             return (cur >> 32) == h && rows_equal(a.probe, r, a.set.build, static_cast<uint32_t>(cur), eq);
           }) != EMPTY;
  }
};

template <int W>
__global__ void __launch_bounds__(PROBE_THREADS) k_set_probe_inline(probe_args a)
{
  int64_t const wave = static_cast<int64_t>(blockIdx.x) * (PROBE_THREADS / 64) + (threadIdx.x >> 6);
  probe_wave<4>(a, wave, set_probe_inline<W>{a});
}

__global__ void __launch_bounds__(PROBE_THREADS) k_set_probe_rows(probe_args a)
{
  int64_t const wave = static_cast<int64_t>(blockIdx.x) * (PROBE_THREADS / 64) + (threadIdx.x >> 6);
  probe_wave<1>(a, wave, set_probe_rows{a});
}

// ------------------------------------------------------------------ pass 2: ordered compaction
// Wave `wave` writes the rows of the set bits of its chunk's mask words at their positions of the output (rowset::compact_chunk).
__global__ void __launch_bounds__(PROBE_THREADS) k_compact(uint64_t const* mask, unsigned long long const* counts, int64_t chunk,
                                                           int64_t nrows, size_type* out, uint64_t out_capacity)
{
  int64_t const wave = static_cast<int64_t>(blockIdx.x) * (PROBE_THREADS / 64) + (threadIdx.x >> 6);
  compact_chunk(mask, counts, wave, chunk, nrows, [&](uint64_t o, int64_t row) {
    if (o < out_capacity) gstore(out + o, static_cast<size_type>(row));
  });
}

// an empty right table: anti_join returns every left row
__global__ void __launch_bounds__(256) k_sequence(size_type* out, int64_t n)
{
  for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * blockDim.x)
    gstore(out + i, static_cast<size_type>(i));
}

}  // namespace

uint64_t lds_bits_max() { return uint64_t{LDS_BYTES_MAX} * 8; }

void launch_bitmap_build(bitmap_args const& a, hipStream_t stream)
{
  cudf::detail::prof::scope prof_{"fjoin_bitmap_build", stream};
  dispatch_int(a.key.width, a.key.cls == CLS_SINT, [&]<int W, bool S>() {
    hipLaunchKernelGGL((k_bitmap_build<W, S>), dim3(grid_for(a.nrows)), dim3(256), 0, stream, a);
  });
  CUDF_HIP_TRY(hipGetLastError());
}

void launch_set_build(set_args const& a, hipStream_t stream)
{
  cudf::detail::prof::scope prof_{"fjoin_set_build", stream};
  unsigned const grid = grid_for(a.build.nrows);
  if (!a.inline_key) hipLaunchKernelGGL(k_set_build_rows, dim3(grid), dim3(256), 0, stream, a);
  else if (a.build.col[0].width == 4) hipLaunchKernelGGL(k_set_build_inline<4>, dim3(grid), dim3(256), 0, stream, a);
  else hipLaunchKernelGGL(k_set_build_inline<8>, dim3(grid), dim3(256), 0, stream, a);
  CUDF_HIP_TRY(hipGetLastError());
}

void launch_bitmap_probe(probe_args const& a, bool lds, hipStream_t stream)
{
  if (lds) {
    CUDF_EXPECTS(a.bm.range <= lds_bits_max() && a.nwaves % (LDS_THREADS / 64) == 0, "filtered_join: bitmap exceeds the LDS probe");
    std::size_t const bytes = static_cast<std::size_t>((a.bm.range + 127) >> 7) * 16;
    cudf::detail::prof::scope prof_{"fjoin_probe_lds", stream};
    dispatch_int(a.probe.col[0].width, a.probe.col[0].cls == CLS_SINT, [&]<int W, bool S>() {
      static std::once_flag once;  // opt the kernel into more than 64 KiB of dynamic LDS, once per process
      std::call_once(once, [] {
        CUDF_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<void const*>(&k_bitmap_probe_lds<W, S>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES_MAX));
      });
      hipLaunchKernelGGL((k_bitmap_probe_lds<W, S>), dim3(a.nwaves / (LDS_THREADS / 64)), dim3(LDS_THREADS), bytes, stream, a);
    });
  } else {
    cudf::detail::prof::scope prof_{"fjoin_probe_bitmap", stream};
    dispatch_int(a.probe.col[0].width, a.probe.col[0].cls == CLS_SINT, [&]<int W, bool S>() {
      hipLaunchKernelGGL((k_bitmap_probe<W, S>), dim3(a.nwaves / (PROBE_THREADS / 64)), dim3(PROBE_THREADS), 0, stream, a);
    });
  }
  CUDF_HIP_TRY(hipGetLastError());
}

void launch_set_probe(probe_args const& a, hipStream_t stream)
{
  cudf::detail::prof::scope prof_{"fjoin_probe_set", stream};
  dim3 const grid(a.nwaves / (PROBE_THREADS / 64));
  if (!a.set.inline_key) hipLaunchKernelGGL(k_set_probe_rows, grid, dim3(PROBE_THREADS), 0, stream, a);
  else if (a.probe.col[0].width == 4) hipLaunchKernelGGL(k_set_probe_inline<4>, grid, dim3(PROBE_THREADS), 0, stream, a);
  else hipLaunchKernelGGL(k_set_probe_inline<8>, grid, dim3(PROBE_THREADS), 0, stream, a);
  CUDF_HIP_TRY(hipGetLastError());
}

void launch_fjoin_sequence(size_type* out, int64_t n, hipStream_t stream)
{
  cudf::detail::prof::scope prof_{"fjoin_sequence", stream};
  hipLaunchKernelGGL(k_sequence, dim3(grid_for(n)), dim3(256), 0, stream, out, n);
  CUDF_HIP_TRY(hipGetLastError());
}

}  // namespace cudf::detail::fjoin

void cudf::detail::rowset::launch_compact_indices(uint64_t const* mask, unsigned long long const* counts, geometry g, int64_t nrows,
                                                  size_type* out, uint64_t out_capacity, hipStream_t stream)
{
  cudf::detail::prof::scope prof_{"fjoin_compact", stream};
  hipLaunchKernelGGL(fjoin::k_compact, dim3(g.nwaves / (fjoin::PROBE_THREADS / 64)), dim3(fjoin::PROBE_THREADS), 0, stream, mask, counts,
                     g.chunk, nrows, out, out_capacity);
  CUDF_HIP_TRY(hipGetLastError());
}
