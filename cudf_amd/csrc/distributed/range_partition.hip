// SPDX-License-Identifier: Apache-2.0
// The hash-range split of table rows by owner rank (include/cudf/distributed.hpp): the flat-column form of a table and the partition
// kernels. The split restates the reference's partitioning.cu:187-337 (histogram, scan, LDS-staged scatter) for a handful of
// destinations and 64-lane waves.
#include "../common/device_table.hpp"
#include "../common/profiler.hpp"
#include "detail.hpp"

#include <cudf/null_mask.hpp>

#include <hip/hip_runtime.h>

#include <algorithm>

namespace cudf {
namespace distributed {
namespace {
using cudf::detail::device_column;
using cudf::detail::device_table;
using cudf::detail::gload;
using cudf::detail::gstore;
using cudf::detail::MAX_COLS;
using detail::RP_MAX_PARTS;

// ------------------------------------------------------------------ hash-range partition kernels
constexpr int RP_BLOCK = 1024, RP_R = 4, RP_TILE = RP_BLOCK * RP_R;
struct rp_args {
  device_table hashed;
  device_table all;
  int32_t nparts;
  int32_t wgs;
  int64_t nrows;
  int64_t chunk;       // rows per workgroup (multiple of RP_TILE)
  uint32_t* counts;    // [wgs][nparts]
  int64_t* cell_base;  // [wgs][nparts]
  int64_t* offsets;    // [nparts + 1]
  void* out[MAX_COLS];
};
template <typename T>
__global__ void k_store(T v, T* dst)
{
  *dst = v;
}
__device__ __forceinline__ uint32_t dest_of(rp_args const& a, int64_t row)
{
  uint32_t const h = cudf::detail::row_hash(a.hashed, row, 0u);
  return static_cast<uint32_t>((static_cast<uint64_t>(h) * static_cast<uint32_t>(a.nparts)) >> 32);
}
__global__ void __launch_bounds__(RP_BLOCK) k_rp_hist(rp_args const* __restrict__ ap)
{
  __shared__ uint32_t whist[16 * RP_MAX_PARTS];  // one histogram per wave: 64 lanes on <= 64 addresses
  rp_args const& a = *ap;
  int const N = a.nparts, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < 16 * N; i += RP_BLOCK) whist[i] = 0;
  __syncthreads();
  int64_t const begin = static_cast<int64_t>(blockIdx.x) * a.chunk, end = min(a.nrows, begin + a.chunk);
  for (int64_t r = begin + threadIdx.x; r < end; r += RP_BLOCK) atomicAdd(&whist[wave * N + dest_of(a, r)], 1u);
  __syncthreads();
  for (int d = threadIdx.x; d < N; d += RP_BLOCK) {
    uint32_t t = 0;
    for (int w = 0; w < 16; ++w) t += whist[w * N + d];
    a.counts[static_cast<int64_t>(blockIdx.x) * N + d] = t;
  }
}
__global__ void __launch_bounds__(64) k_rp_scan(rp_args const* __restrict__ ap)
{
  // one lane per destination (nparts <= 64): its rows over all workgroups, a wave-wide exclusive scan over the destinations,
  // then the cell bases (one lane walking all wgs * nparts cells was a millisecond of dependent loads on every shuffle)
  rp_args const& a = *ap;
  int const N = a.nparts, d = threadIdx.x;
  int64_t tot = 0;
  if (d < N)
    for (int w = 0; w < a.wgs; ++w) tot += a.counts[static_cast<int64_t>(w) * N + d];
  int64_t inc = tot;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    int64_t const t = __shfl_up(inc, o);
    if (d >= o) inc += t;
  }
  if (d < N) {
    int64_t run  = inc - tot;
    a.offsets[d] = run;
    for (int w = 0; w < a.wgs; ++w) {
      a.cell_base[static_cast<int64_t>(w) * N + d] = run;
      run += a.counts[static_cast<int64_t>(w) * N + d];
    }
    if (d == N - 1) a.offsets[N] = run;
  }
}
template <typename T>
__device__ __forceinline__ void move_column(device_column const& col, void* out, int64_t tile, int64_t end, uint32_t const (&lpos)[RP_R],
                                            T* stage, uint8_t const* sdest, uint32_t const* doff, int64_t const* gcur, uint32_t tile_rows)
{
  T const* src = static_cast<T const*>(col.head) + col.offset;
  T v[RP_R];
#pragma unroll
  for (int k = 0; k < RP_R; ++k) {
    int64_t const r = tile + static_cast<int64_t>(k) * RP_BLOCK + threadIdx.x;
    if (r < end) v[k] = gload(src + r);
  }
#pragma unroll
  for (int k = 0; k < RP_R; ++k) {
    int64_t const r = tile + static_cast<int64_t>(k) * RP_BLOCK + threadIdx.x;
    if (r < end) stage[lpos[k]] = v[k];
  }
  __syncthreads();
  for (uint32_t j = threadIdx.x; j < tile_rows; j += RP_BLOCK) {
    uint32_t const d = sdest[j];
    gstore(static_cast<T*>(out) + gcur[d] + (j - doff[d]), stage[j]);
  }
  __syncthreads();
}
// Columns [c0, c1) of the flat table (every launch ranks the rows again: a pipelined shuffle moves one column per launch so that the
// exchange of column c runs beside the scatter of column c + 1).
__global__ void __launch_bounds__(RP_BLOCK) k_rp_scatter(rp_args const* __restrict__ ap, int c0, int c1)
{
  __shared__ uint64_t stage64[RP_TILE];        // one column's values of a tile, in destination order
  __shared__ uint8_t sdest[RP_TILE];           // destination of every staged position
  __shared__ uint32_t whist[16 * RP_MAX_PARTS];
  __shared__ uint32_t doff[RP_MAX_PARTS + 1];  // first staged position of a destination
  __shared__ int64_t gcur[RP_MAX_PARTS];       // this workgroup's write cursor per destination
  rp_args const& a = *ap;
  int const N = a.nparts, wave = threadIdx.x >> 6;
  int64_t const begin = static_cast<int64_t>(blockIdx.x) * a.chunk, end = min(a.nrows, begin + a.chunk);
  for (int d = threadIdx.x; d < N; d += RP_BLOCK) gcur[d] = a.cell_base[static_cast<int64_t>(blockIdx.x) * N + d];
  for (int64_t tile = begin; tile < end; tile += RP_TILE) {
    for (int i = threadIdx.x; i < 16 * N; i += RP_BLOCK) whist[i] = 0;
    __syncthreads();
    uint32_t dst[RP_R], rank[RP_R], lpos[RP_R];
#pragma unroll
    for (int k = 0; k < RP_R; ++k) {
      int64_t const r = tile + static_cast<int64_t>(k) * RP_BLOCK + threadIdx.x;
      dst[k] = 0; rank[k] = 0;
      if (r < end) {
        dst[k]  = dest_of(a, r);
        rank[k] = atomicAdd(&whist[wave * N + dst[k]], 1u);  // rank inside (wave, destination); waves rank in row order
      }
    }
    __syncthreads();
    // per destination: exclusive prefix over the waves (in place), tile total; then the staged offset of every destination
    if (static_cast<int>(threadIdx.x) < N) {
      uint32_t run = 0;
      for (int w = 0; w < 16; ++w) {
        uint32_t const c = whist[w * N + threadIdx.x];
        whist[w * N + threadIdx.x] = run;
        run += c;
      }
      doff[threadIdx.x + 1] = run;  // (totals for now)
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t run = 0;
      for (int d = 0; d < N; ++d) {
        uint32_t const c = doff[d + 1];
        doff[d] = run;
        run += c;
      }
      doff[N] = run;
    }
    __syncthreads();
    uint32_t const tile_rows = doff[N];
#pragma unroll
    for (int k = 0; k < RP_R; ++k) {
      int64_t const r = tile + static_cast<int64_t>(k) * RP_BLOCK + threadIdx.x;
      lpos[k] = 0;
      if (r < end) {
        // rows of one (wave, destination) keep their order: row sets k are ranked one after the other by the same wave
        lpos[k]        = doff[dst[k]] + whist[wave * N + dst[k]] + rank[k];
        sdest[lpos[k]] = static_cast<uint8_t>(dst[k]);
      }
    }
    __syncthreads();
    for (int c = c0; c < c1; ++c) {
      device_column const col = a.all.col[c];
      switch (col.width) {
        case 1: move_column<uint8_t>(col, a.out[c], tile, end, lpos, reinterpret_cast<uint8_t*>(stage64), sdest, doff, gcur, tile_rows); break;
        case 2: move_column<uint16_t>(col, a.out[c], tile, end, lpos, reinterpret_cast<uint16_t*>(stage64), sdest, doff, gcur, tile_rows); break;
        case 4: move_column<uint32_t>(col, a.out[c], tile, end, lpos, reinterpret_cast<uint32_t*>(stage64), sdest, doff, gcur, tile_rows); break;
        default: move_column<uint64_t>(col, a.out[c], tile, end, lpos, stage64, sdest, doff, gcur, tile_rows);
      }
    }
    if (static_cast<int>(threadIdx.x) < N) gcur[threadIdx.x] += doff[threadIdx.x + 1] - doff[threadIdx.x];
    __syncthreads();
  }
}

// validity bits [offset, offset + n) -> one byte per row (1 = valid), and back
__global__ void __launch_bounds__(256) k_mask_to_bytes(bitmask_type const* mask, int64_t offset, int64_t n, uint8_t* out)
{
  int64_t const i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
  if (i < n) out[i] = mask == nullptr ? 1 : ((mask[(offset + i) >> 5] >> ((offset + i) & 31)) & 1u);
}
__global__ void __launch_bounds__(256) k_bytes_to_mask(uint8_t const* bytes, int64_t n, bitmask_type* mask, int32_t* null_count)
{
  int64_t const i               = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
  bool const valid              = i < n && bytes[i] != 0;
  unsigned long long const b    = __ballot(valid);
  unsigned long long const live = __ballot(i < n);
  int const lane                = threadIdx.x & 63;
  if (i < n && (lane & 31) == 0) mask[i >> 5] = static_cast<uint32_t>(b >> (lane & 32));
  int const nulls = __popcll(live & ~b);
  if (lane == 0 && nulls) atomicAdd(null_count, nulls);
}
}  // namespace

// ------------------------------------------------------------------ the flat-column form of a table
namespace detail {
flat_table flatten(table_view const& input, uint64_t with_validity, hipStream_t s)
{
  flat_table f;
  f.ninput = input.num_columns();
  auto tmp = cudf::get_current_device_resource_ref();
  for (auto const& c : input) {
    CUDF_EXPECTS(c.num_children() == 0 && size_of_id(c.type().id()) >= 1 && size_of_id(c.type().id()) <= 8,
                 "distributed shuffle: fixed-width columns of at most 8 bytes only");
    f.cols.push_back(column_view{c.type(), c.size(), c.head(), nullptr, 0, c.offset()});
  }
  for (int c = 0; c < f.ninput; ++c) {
    if (!((with_validity >> c) & 1u)) continue;
    auto const& col = input.column(c);
    f.temps.emplace_back(static_cast<std::size_t>(std::max<size_type>(col.size(), 1)), s, tmp);
    if (col.size() > 0) {
      hipLaunchKernelGGL(k_mask_to_bytes, dim3(static_cast<unsigned>((col.size() + 255) / 256)), dim3(256), 0, s,
                         col.has_nulls() ? col.null_mask() : nullptr, static_cast<int64_t>(col.offset()), static_cast<int64_t>(col.size()),
                         static_cast<uint8_t*>(f.temps.back().data()));
    }
    f.cols.push_back(column_view{data_type{type_id::UINT8}, col.size(), f.temps.back().data(), nullptr, 0, 0});
    f.validity_of.push_back(c);
  }
  CUDF_EXPECTS(static_cast<int>(f.cols.size()) <= MAX_COLS,
               "distributed shuffle: at most 16 flat columns (a column with nulls on any rank counts twice: its validity travels as a "
               "byte column)",
               std::invalid_argument);
  return f;
}
std::unique_ptr<table> assemble(table_view const& like, flat_table const& f, std::vector<rmm::device_buffer>&& bufs, int64_t nrows,
                                stream_ref stream, rmm::device_async_resource_ref mr)
{
  hipStream_t const s = stream.value();
  std::vector<std::unique_ptr<column>> cols;
  for (int c = 0; c < f.ninput; ++c)
    cols.push_back(std::make_unique<column>(like.column(c).type(), static_cast<size_type>(nrows), std::move(bufs[c]), rmm::device_buffer{}, 0));
  if (!f.validity_of.empty() && nrows > 0) {
    rmm::device_buffer counters{sizeof(int32_t) * f.validity_of.size(), s, cudf::get_current_device_resource_ref()};
    CUDF_HIP_TRY(hipMemsetAsync(counters.data(), 0, counters.size(), s));
    std::vector<rmm::device_buffer> masks;
    for (std::size_t j = 0; j < f.validity_of.size(); ++j) {
      masks.push_back(create_null_mask(static_cast<size_type>(nrows), mask_state::UNINITIALIZED, stream, mr));
      hipLaunchKernelGGL(k_bytes_to_mask, dim3(static_cast<unsigned>((nrows + 255) / 256)), dim3(256), 0, s,
                         static_cast<uint8_t const*>(bufs[f.ninput + j].data()), nrows, static_cast<bitmask_type*>(masks.back().data()),
                         static_cast<int32_t*>(counters.data()) + j);
    }
    CUDF_HIP_TRY(hipGetLastError());
    std::vector<int32_t> h(f.validity_of.size());
    CUDF_HIP_TRY(hipMemcpyAsync(h.data(), counters.data(), counters.size(), hipMemcpyDeviceToHost, s));
    CUDF_HIP_TRY(hipStreamSynchronize(s));
    for (std::size_t j = 0; j < f.validity_of.size(); ++j)
      if (h[j] > 0) cols[f.validity_of[j]]->set_null_mask(std::move(masks[j]), h[j]);
  }
  return std::make_unique<table>(std::move(cols));
}

// ------------------------------------------------------------------ host driver of the split
std::pair<std::vector<rmm::device_buffer>, std::vector<int64_t>> partition_flat(flat_table const& f, table_view const& hashed, int N,
                                                                                stream_ref stream, rmm::device_async_resource_ref mr,
                                                                                scatter_pipeline* pipe)
{
  CUDF_EXPECTS(N >= 1 && N <= RP_MAX_PARTS, "distributed shuffle: 1 to 64 destinations", std::invalid_argument);
  hipStream_t const s = stream.value();
  int64_t const n     = f.cols.empty() ? 0 : f.cols.front().size();
  std::vector<rmm::device_buffer> out;
  for (auto const& c : f.cols) out.emplace_back(static_cast<std::size_t>(std::max<int64_t>(n, 1)) * size_of_id(c.type().id()), s, mr);
  std::vector<int64_t> h_off(static_cast<std::size_t>(N) + 1, 0);
  auto all_ready_on_main = [&] {  // (no side work: every column is ready where the caller's stream stands)
    if (pipe != nullptr)
      for (auto e : pipe->column_ready) CUDF_HIP_TRY(hipEventRecord(e, s));
  };
  if (n == 0) {
    all_ready_on_main();
    return {std::move(out), std::move(h_off)};
  }
  if (N == 1) {  // one destination: the rows stay as they are
    for (std::size_t c = 0; c < f.cols.size(); ++c) {
      auto const w = size_of_id(f.cols[c].type().id());
      CUDF_HIP_TRY(hipMemcpyAsync(out[c].data(), static_cast<char const*>(f.cols[c].head()) + static_cast<std::size_t>(f.cols[c].offset()) * w,
                                  static_cast<std::size_t>(n) * w, hipMemcpyDeviceToDevice, s));
    }
    h_off[1] = n;
    all_ready_on_main();
    return {std::move(out), std::move(h_off)};
  }
  auto tmp = cudf::get_current_device_resource_ref();
  rp_args a{};
  a.hashed = cudf::detail::make_device_table(hashed);
  a.all    = cudf::detail::make_device_table(table_view{f.cols});
  a.nparts = N;
  a.nrows  = n;
  a.wgs    = static_cast<int32_t>(std::clamp<int64_t>((n + RP_TILE - 1) / RP_TILE, 1, 512));
  a.chunk  = ((n + a.wgs - 1) / a.wgs + RP_TILE - 1) / RP_TILE * RP_TILE;
  rmm::device_buffer counts{sizeof(uint32_t) * a.wgs * N, s, tmp}, cell{sizeof(int64_t) * a.wgs * N, s, tmp},
    offs{sizeof(int64_t) * (N + 1), s, tmp}, d_args{sizeof(rp_args), s, tmp};
  a.counts    = static_cast<uint32_t*>(counts.data());
  a.cell_base = static_cast<int64_t*>(cell.data());
  a.offsets   = static_cast<int64_t*>(offs.data());
  for (std::size_t c = 0; c < f.cols.size(); ++c) a.out[c] = out[c].data();
  auto* da = static_cast<rp_args*>(d_args.data());
  hipLaunchKernelGGL(k_store<rp_args>, dim3(1), dim3(1), 0, s, a, da);
  {
    cudf::detail::prof::scope p_{"range_partition_hist", s};
    hipLaunchKernelGGL(k_rp_hist, dim3(a.wgs), dim3(RP_BLOCK), 0, s, da);
  }
  hipLaunchKernelGGL(k_rp_scan, dim3(1), dim3(64), 0, s, da);
  if (pipe == nullptr) {
    cudf::detail::prof::scope p_{"range_partition_scatter", s};
    hipLaunchKernelGGL(k_rp_scatter, dim3(a.wgs), dim3(RP_BLOCK), 0, s, da, 0, a.all.ncols);
  } else {
    // one launch per column on the side stream, behind the scan; the caller's stream goes on to the count exchange
    CUDF_HIP_TRY(hipEventRecord(pipe->scan_done, s));
    CUDF_HIP_TRY(hipStreamWaitEvent(pipe->side, pipe->scan_done, 0));
    for (int c = 0; c < a.all.ncols; ++c) {
      hipLaunchKernelGGL(k_rp_scatter, dim3(a.wgs), dim3(RP_BLOCK), 0, pipe->side, da, c, c + 1);
      CUDF_HIP_TRY(hipEventRecord(pipe->column_ready[static_cast<std::size_t>(c)], pipe->side));
    }
  }
  CUDF_HIP_TRY(hipGetLastError());
  CUDF_HIP_TRY(hipMemcpyAsync(h_off.data(), a.offsets, sizeof(int64_t) * (N + 1), hipMemcpyDeviceToHost, s));
  CUDF_HIP_TRY(hipStreamSynchronize(s));
  if (pipe != nullptr) {
    // the scratch of this function (histogram cells, argument block) is read by the side stream's launches: its stream-ordered release
    // on `s` waits for the last of them
    CUDF_HIP_TRY(hipStreamWaitEvent(s, pipe->column_ready.back(), 0));
  }
  return {std::move(out), std::move(h_off)};
}

uint64_t nullable_bits(table_view const& t)
{
  uint64_t b = 0;
  for (int c = 0; c < t.num_columns(); ++c)
    if (t.column(c).has_nulls()) b |= uint64_t{1} << c;
  return b;
}
}  // namespace detail

// ------------------------------------------------------------------ range_partition
std::pair<std::unique_ptr<table>, std::vector<size_type>> range_partition(table_view const& input, std::vector<size_type> const& key_columns,
                                                                          int num_destinations, stream_ref stream,
                                                                          rmm::device_async_resource_ref mr)
{
  auto const hashed = input.select(key_columns);
  CUDF_EXPECTS(hashed.num_columns() >= 1, "range_partition: at least one key column", std::invalid_argument);
  auto f            = detail::flatten(input, detail::nullable_bits(input), stream.value());
  auto [bufs, off]  = detail::partition_flat(f, hashed, num_destinations, stream, mr);
  std::vector<size_type> offsets(off.begin(), off.end());
  return {detail::assemble(input, f, std::move(bufs), input.num_rows(), stream, mr), std::move(offsets)};
}

}  // namespace distributed
}  // namespace cudf
