// SPDX-License-Identifier: Apache-2.0
// gfx950 kernels every table form of the hash join shares: the scan of the per-workgroup pair counts and the full join's complement.
#include "join_device.hpp"
#include "../common/profiler.hpp"

#include <cudf/utilities/error.hpp>

namespace cudf::detail::join {
namespace {

// exclusive scan of the per-block pair counts (nblocks <= 65536): one workgroup
__global__ void __launch_bounds__(1024) k_scan_counts(unsigned long long* counts, int32_t nblocks)
{
  __shared__ unsigned long long wave_tot[16];
  __shared__ unsigned long long carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < nblocks; base += 1024) {
    int const i                  = base + threadIdx.x;
    unsigned long long const v   = i < nblocks ? counts[i] : 0;
    unsigned long long const off = carry + block_exclusive_scan(v, wave_tot);
    if (i < nblocks) counts[i] = off;
    __syncthreads();
    if (threadIdx.x == 1023) carry = off + v;
    __syncthreads();
  }
  if (threadIdx.x == 0) counts[nblocks] = carry;
}

// full join: {JoinNoMatch, r} for the rows r of the build side no probe row matched, appended at *total; one global atomic per workgroup
__global__ void __launch_bounds__(256) k_complement(uint8_t const* build_matched, int64_t n, unsigned long long* total, size_type* out_probe,
                                                    size_type* out_build, uint64_t out_capacity)
{
  __shared__ unsigned long long s_cursor;
  __shared__ unsigned int s_count;
  int64_t const chunk  = (n + gridDim.x - 1) / gridDim.x;
  int64_t const begin  = static_cast<int64_t>(blockIdx.x) * chunk;
  int64_t const end    = min(n, begin + chunk);
  if (threadIdx.x == 0) s_count = 0;
  __syncthreads();
  unsigned int mine = 0;
  for (int64_t r = begin + threadIdx.x; r < end; r += blockDim.x) mine += build_matched[r] == 0;
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&s_count, mine);
  __syncthreads();
  if (threadIdx.x == 0) s_cursor = s_count ? atomicAdd(total, static_cast<unsigned long long>(s_count)) : 0ull;
  __syncthreads();
  if (s_count == 0) return;
  int const lane = threadIdx.x & 63;
  for (int64_t r0 = begin; r0 < end; r0 += blockDim.x) {
    int64_t const r   = r0 + threadIdx.x;
    bool const lonely = r < end && build_matched[r] == 0;
    uint64_t const o  = wave_reserve(lonely, &s_cursor, lane);
    if (lonely && o < out_capacity) {
      gstore(out_probe + o, JoinNoMatch);
      gstore(out_build + o, static_cast<size_type>(r));
    }
  }
}

__global__ void __launch_bounds__(256) k_mark_matched(size_type const* right_indices, std::size_t n, uint8_t* build_matched)
{
  for (std::size_t i = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x; i < n;
       i += static_cast<std::size_t>(gridDim.x) * blockDim.x) {
    size_type const r = gload(right_indices + i);
    if (r != JoinNoMatch) gstore(build_matched + r, uint8_t{1});
  }
}
}  // namespace

void launch_scan(unsigned long long* counts, int32_t n, hipStream_t stream)
{
  hipLaunchKernelGGL(k_scan_counts, dim3(1), dim3(1024), 0, stream, counts, n);
  CUDF_HIP_TRY(hipGetLastError());
}
void launch_mark_matched(size_type const* right_indices, std::size_t n, uint8_t* build_matched, hipStream_t stream)
{
  if (n == 0) return;
  hipLaunchKernelGGL(k_mark_matched, dim3(grid_for(static_cast<int64_t>(n))), dim3(256), 0, stream, right_indices, n, build_matched);
  CUDF_HIP_TRY(hipGetLastError());
}
void launch_complement(uint8_t const* build_matched, int64_t nrows, unsigned long long* total, size_type* out_probe, size_type* out_build,
                       uint64_t out_capacity, hipStream_t stream)
{
  cudf::detail::prof::scope prof_{"join_complement", stream};
  hipLaunchKernelGGL(k_complement, dim3(grid_for(nrows)), dim3(256), 0, stream, build_matched, nrows, total, out_probe, out_build, out_capacity);
  CUDF_HIP_TRY(hipGetLastError());
}
}  // namespace cudf::detail::join
