// SPDX-License-Identifier: Apache-2.0
// hash_join_impl, the dense direct-address table (engine.hpp join_args::dense_head, dense_part_args, dense_stage_args): the decision
// from the build keys' exact minimum / maximum, the partitioned and atomic builds, row lists, and the ordered, left-direct and
// partitioned probes of a dense unique table.
#include "hash_join_impl.hpp"

#include <algorithm>
#include <cmath>
#include <new>

namespace cudf::detail {

// exact minimum / maximum of build key columns [0, ncols) -> h[2c], h[2c + 1] (one read-back); false: some column has no valid key.
// d_args receives the kernels' argument scratch (ncols join_args), which the dense build reuses.
bool hash_join_impl::key_minmax(int ncols, uint64_t* h, rmm::device_buffer& d_args, hipStream_t s) const
{
  auto tmp = cudf::get_current_device_resource_ref();
  rmm::device_buffer mm{2 * ncols * sizeof(uint64_t), s, tmp};
  d_args = rmm::device_buffer{ncols * sizeof(join_args), s, tmp};
  bool sgn[2];
  for (int c = 0; c < ncols; ++c) {
    sgn[c]         = class_of(_right.column(c).type().id()) == CLS_SINT;
    join_args a    = base_args(_right, 0);
    a.build.col[0] = _build_dev.col[c];
    join::launch_key_minmax(a, static_cast<join_args*>(d_args.data()) + c, sgn[c] ? 1 : 0, static_cast<uint64_t*>(mm.data()) + 2 * c, s);
  }
  CUDF_HIP_TRY(hipMemcpyAsync(h, mm.data(), 2 * ncols * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  CUDF_HIP_TRY(hipStreamSynchronize(s));
  for (int c = 0; c < ncols; ++c)
    if (sgn[c] ? static_cast<int64_t>(h[2 * c]) > static_cast<int64_t>(h[2 * c + 1]) : h[2 * c] > h[2 * c + 1]) return false;
  return true;
}

// One integer key column whose valid build keys span a small range: the direct-address table over [min, max] replaces the hash
// table. false: the keys do not take it (the caller tries the radix join, then the hash table).
bool hash_join_impl::try_dense_build(table_view const& right, stream_ref stream)
{
  auto const rows = static_cast<uint64_t>(right.num_rows());
  if (rows < static_cast<uint64_t>(env_i64("CUDF_AMD_JOIN_DENSE_MIN_ROWS", 1 << 16)) || env_i64("CUDF_AMD_JOIN_DENSE", 1) == 0) return false;
  hipStream_t const s = stream.value();
  auto tmp            = cudf::get_current_device_resource_ref();
  uint64_t h_mm[2]    = {0, 0};
  rmm::device_buffer d_args;
  bool const any_valid = key_minmax(1, h_mm, d_args, s);
  uint64_t const width = h_mm[1] - h_mm[0];  // exact in two's complement for either ordering
  // at most 4 table entries (16 bytes) per build row, and at most 2^29 entries (2 GiB)
  if (!any_valid || width >= std::min<uint64_t>(std::max<uint64_t>(4 * rows, uint64_t{1} << 20), uint64_t{1} << 29)) return false;
  _dense_lo    = h_mm[0];
  _dense_range = width + 1;
  _dense_head  = rmm::device_buffer{_dense_range * sizeof(int32_t), s, _mr};
  _dense_next  = rmm::device_buffer{rows * sizeof(int32_t), s, _mr};
  CUDF_HIP_TRY(hipMemsetAsync(_dense_head.data(), 0xff, _dense_head.size(), s));
  // big tables: rows partitioned by key range, plain stores that stay in L2, uniqueness from a count (dense_part_kernels.hip)
  bool part_built = false;
  try {
    part_built = try_dense_part_build(right, stream);
  } catch (std::bad_alloc const&) {  // (no room for the partition scratch: the atomic-exchange build needs none)
    CUDF_HIP_TRY(hipMemsetAsync(_dense_head.data(), 0xff, _dense_head.size(), s));
  }
  if (part_built) {
    _state = _key.width == 8 ? build_state::dense_part8 : build_state::dense_part4;
    return true;
  }
  if (_key.width != 8) {  // a 4-byte key whose rows did not take the partitioned build (the direct passes read 8-byte keys)
    _dense_head = rmm::device_buffer{};
    _dense_next = rmm::device_buffer{};
    return false;
  }
  _state = build_state::dense_unique;
  rmm::device_buffer dups{sizeof(int32_t), s, tmp};
  CUDF_HIP_TRY(hipMemsetAsync(dups.data(), 0, sizeof(int32_t), s));
  join_args b  = base_args(right, 0);
  b.dense_dups = static_cast<int32_t*>(dups.data());
  join::launch_dense_build(b, static_cast<join_args*>(d_args.data()), s);
  int32_t h_dups = 0;
  CUDF_HIP_TRY(hipMemcpyAsync(&h_dups, dups.data(), sizeof(int32_t), hipMemcpyDeviceToHost, s));
  CUDF_HIP_TRY(hipStreamSynchronize(s));
  if (h_dups == 0) return true;
  _state = build_state::dense_csr;  // row lists instead of chains (engine.hpp launch_dense_csr)
  std::size_t const entries = join::dense_csr_entries(_dense_range);
  _dense_head = rmm::device_buffer{entries * sizeof(int32_t), s, _mr};
  CUDF_HIP_TRY(hipMemsetAsync(_dense_head.data(), 0, _dense_head.size(), s));
  rmm::device_buffer cursor{_dense_range * sizeof(int32_t), s, tmp}, sums{entries / 8192 * sizeof(uint32_t) + 16, s, tmp};
  CUDF_HIP_TRY(hipMemsetAsync(cursor.data(), 0, cursor.size(), s));
  join_args c = base_args(right, 0);
  join::launch_dense_csr(c, static_cast<join_args*>(d_args.data()), static_cast<int32_t*>(cursor.data()), static_cast<uint32_t*>(sums.data()), s);
  CUDF_HIP_TRY(hipStreamSynchronize(s));
  return true;
}

// rows -> records {key - lo | row << 32} in regions (partition, slice); `expected` = the rows a slice may have to take
void hash_join_impl::dense_partition(uint64_t const* keys, bitmask_type const* mask, int64_t mask_offset, int64_t nrows, dense_side& out,
                                     stream_ref stream) const
{
  hipStream_t const s = stream.value();
  auto tmp            = cudf::get_current_device_resource_ref();
  // slices of >= 1 MB (CUDF_AMD_JOIN_DENSE_PART_SLICE_LOG2: keys per slice, the tests shrink it), at most 256 of them
  int const shift     = std::max(static_cast<int>(env_i64("CUDF_AMD_JOIN_DENSE_PART_SLICE_LOG2", 18)), ceil_log2(_dense_range) - 8);
  int64_t const P     = static_cast<int64_t>((_dense_range - 1) >> shift) + 1;
  int64_t Pring = 16;
  while (Pring < P) Pring <<= 1;
  // one workgroup of 1024 threads per CU, tiles of 4096 rows (two workgroups of 512 threads per CU measured 8 % slower on C3: 1.73
  // against 1.60 ms for both scatters, profiles/r3_c3_dense_part.txt)
  int64_t const tile_rows = 4 * 1024;
  int64_t const tiles = (nrows + tile_rows - 1) / tile_rows, S = std::clamp<int64_t>(tiles, 1, 256);
  double const mean   = static_cast<double>(std::min<int64_t>(nrows, (tiles + S - 1) / S * tile_rows)) / static_cast<double>(P);
  int64_t const cap   = (static_cast<int64_t>(mean * 1.02 + 6.0 * std::sqrt(std::max(mean, 1.0)) + 64.0) + 31) / 32 * 32;
  out.recs   = rmm::device_buffer{static_cast<std::size_t>(Pring * S * cap) * sizeof(uint64_t), s, tmp};
  out.counts = rmm::device_buffer{static_cast<std::size_t>(Pring * S) * sizeof(int32_t), s, tmp};
  out.ovf    = rmm::device_buffer{sizeof(int32_t), s, tmp};
  out.cap    = cap;
  out.P      = static_cast<int32_t>(Pring);
  out.P_used = static_cast<int32_t>(P);
  out.S      = static_cast<int32_t>(S);
  CUDF_HIP_TRY(hipMemsetAsync(out.counts.data(), 0, out.counts.size(), s));
  CUDF_HIP_TRY(hipMemsetAsync(out.ovf.data(), 0, sizeof(int32_t), s));
  join::radix_scatter_args a{};
  a.level          = 1;
  a.keys           = keys;
  a.key_width      = _key.width;
  a.key_signed     = _key.is_signed ? 1 : 0;
  a.mask           = mask;
  a.mask_offset    = mask_offset;
  a.nrows          = nrows;
  a.P              = static_cast<int32_t>(Pring);
  a.capl           = 14 - ceil_log2(static_cast<uint64_t>(Pring));  // 16384 ring slots of 8 bytes
  a.shift          = shift;
  a.slices         = static_cast<int32_t>(S);
  a.out_key        = static_cast<uint64_t*>(out.recs.data());
  a.region_cap     = cap;
  a.region_count   = static_cast<int32_t*>(out.counts.data());
  a.overflow       = static_cast<int32_t*>(out.ovf.data());
  a.dense          = 1;
  a.dense_lo       = _dense_lo;
  a.dense_range    = _dense_range;
  a.pending_budget = 64;
  rmm::device_buffer d_args{sizeof(join::radix_scatter_args), s, tmp};
  join::launch_radix_scatter(a, static_cast<join::radix_scatter_args*>(d_args.data()), s);
}

join::dense_part_args hash_join_impl::dense_part_args_of(dense_side const& side) const
{
  join::dense_part_args a{};
  a.recs         = static_cast<uint64_t const*>(side.recs.data());
  a.region_count = static_cast<int32_t const*>(side.counts.data());
  a.region_cap   = side.cap;
  a.P            = side.P;
  a.P_used       = side.P_used;
  a.S            = side.S;
  a.head         = const_cast<int32_t*>(static_cast<int32_t const*>(_dense_head.data()));
  a.overflow     = static_cast<int32_t const*>(side.ovf.data());
  return a;
}

// the dense table of a big build side without atomics; false: a key repeats (or the rows cluster): the caller builds it the
// other way (head is all -1 again)
bool hash_join_impl::try_dense_part_build(table_view const& right, stream_ref stream)
{
  auto const& col    = right.column(0);
  int64_t const rows = right.num_rows();
  if (rows < env_i64("CUDF_AMD_JOIN_DENSE_PART_MIN_BUILD", 4 << 20) ||
      static_cast<int64_t>(_dense_range) < env_i64("CUDF_AMD_JOIN_DENSE_PART_MIN_RANGE", 8 << 20) || rows > (int64_t{1} << 31) - 1)
    return false;
  hipStream_t const s = stream.value();
  auto tmp            = cudf::get_current_device_resource_ref();
  dense_side side;
  dense_partition(key_bytes(col, _key.width), (_has_nulls && col.has_nulls()) ? col.null_mask() : nullptr, col.offset(), rows, side, stream);
  auto a = dense_part_args_of(side);
  // {filled table entries, records the scatter produced}: equal <=> no build key repeats
  rmm::device_buffer d_args{sizeof(join::dense_part_args), s, tmp}, tally{2 * sizeof(unsigned long long), s, tmp};
  CUDF_HIP_TRY(hipMemsetAsync(tally.data(), 0, 2 * sizeof(unsigned long long), s));
  auto* d_tally = static_cast<unsigned long long*>(tally.data());
  join::launch_dense_part_store(a, static_cast<join::dense_part_args*>(d_args.data()), s);
  join::launch_dense_count_filled(a.head, _dense_range, d_tally, s);
  join::launch_sum_region_counts(a.region_count, static_cast<int64_t>(side.P) * side.S, d_tally + 1, s);
  unsigned long long h_tally[2] = {0, 0};
  int32_t h_ovf                 = 0;
  CUDF_HIP_TRY(hipMemcpyAsync(h_tally, d_tally, sizeof(h_tally), hipMemcpyDeviceToHost, s));
  CUDF_HIP_TRY(hipMemcpyAsync(&h_ovf, side.ovf.data(), sizeof(int32_t), hipMemcpyDeviceToHost, s));
  CUDF_HIP_TRY(hipStreamSynchronize(s));
  if (h_ovf != 0 || h_tally[0] != h_tally[1]) {
    CUDF_HIP_TRY(hipMemsetAsync(_dense_head.data(), 0xff, _dense_head.size(), s));
    return false;
  }
  return true;
}

// the probe column against the dense table: dense_stage_args' keys / mask / nrows / dense_* / head / probe_row_base
join::dense_stage_args hash_join_impl::dense_stage_of(table_view const& left, int64_t row_base) const
{
  auto const& col = left.column(0);
  join::dense_stage_args a{};
  a.keys           = key_bytes(col, _key.width);
  a.key_width      = _key.width;
  a.key_signed     = _key.is_signed ? 1 : 0;
  a.mask           = (_has_nulls && col.has_nulls()) ? col.null_mask() : nullptr;
  a.mask_offset    = col.offset();
  a.nrows          = left.num_rows();
  a.dense_lo       = _dense_lo;
  a.dense_range    = _dense_range;
  a.head           = static_cast<int32_t const*>(_dense_head.data());
  a.probe_row_base = row_base;
  return a;
}

// share of the probe rows whose key is valid and inside the dense table's range (a sample of ~64K rows; one small kernel + read-back)
double hash_join_impl::dense_inrange_share(table_view const& left, stream_ref stream) const
{
  hipStream_t const s = stream.value();
  auto tmp            = cudf::get_current_device_resource_ref();
  rmm::device_buffer d_args{sizeof(join::dense_stage_args), s, tmp}, d_out{2 * sizeof(unsigned long long), s, tmp};
  join::launch_dense_inrange_sample(dense_stage_of(left, 0), static_cast<join::dense_stage_args*>(d_args.data()), 1 << 16, static_cast<unsigned long long*>(d_out.data()), s);
  unsigned long long h[2] = {0, 0};
  CUDF_HIP_TRY(hipMemcpyAsync(h, d_out.data(), sizeof(h), hipMemcpyDeviceToHost, s));
  CUDF_HIP_TRY(hipStreamSynchronize(s));
  return h[0] == 0 ? 0.0 : static_cast<double>(h[1]) / static_cast<double>(h[0]);
}

// inner join against a dense unique table with the pairs in probe-row order (engine.hpp dense_stage_args); nullopt: not this call
std::optional<join_index_pair> hash_join_impl::dense_ordered_probe(table_view const& left, stream_ref stream, rmm::device_async_resource_ref mr,
                                                                   int64_t row_base) const
{
  int64_t const rows = left.num_rows();
  if ((_has_nulls && left.column(0).has_nulls() && _nulls_equal == null_equality::EQUAL) ||
      rows < env_i64("CUDF_AMD_JOIN_DENSE_ORDERED_MIN_PROBE", 1 << 20) || rows + row_base > (int64_t{1} << 31) - 1)
    return std::nullopt;
  hipStream_t const s = stream.value();
  auto tmp            = cudf::get_current_device_resource_ref();
  join::dense_stage_args a = dense_stage_of(left, row_base);
  // ~16K waves (64 per CU) of at least 4096 rows each
  a.wave_rows = std::max<int64_t>(4096, ((rows + 16383) / 16384 + 63) / 64 * 64);
  a.nwaves    = static_cast<int32_t>((rows + a.wave_rows - 1) / a.wave_rows);
  rmm::device_buffer stage{static_cast<std::size_t>(a.nwaves) * static_cast<std::size_t>(a.wave_rows) * sizeof(uint64_t), s, tmp},
    counts{(static_cast<std::size_t>(a.nwaves) + 1) * sizeof(unsigned long long), s, tmp}, d_args{sizeof(join::dense_stage_args), s, tmp};
  a.stage       = static_cast<uint64_t*>(stage.data());
  a.pair_counts = static_cast<unsigned long long*>(counts.data());
  join::launch_dense_probe_staged(a, static_cast<join::dense_stage_args*>(d_args.data()), s);
  unsigned long long const total = scan_total(a.pair_counts, a.nwaves, s);
  join::radix_join_args e{};  // (the copy of the staged pairs is the radix join's: one "partition" per wave)
  e.nparts      = a.nwaves;
  e.pair_counts = a.pair_counts;
  e.stage       = a.stage;
  e.stage_cap   = a.wave_rows;
  return emit_staged(e, total, s, mr);
}

// LEFT join against a dense unique table: one pair per probe row, in order - a single pass (engine.hpp launch_dense_left_direct)
std::optional<join_index_pair> hash_join_impl::dense_left_direct(table_view const& left, stream_ref stream, rmm::device_async_resource_ref mr,
                                                                 int64_t row_base) const
{
  if ((_has_nulls && left.column(0).has_nulls() && _nulls_equal == null_equality::EQUAL) ||
      left.num_rows() < env_i64("CUDF_AMD_JOIN_DENSE_ORDERED_MIN_PROBE", 1 << 20) || left.num_rows() + row_base > (int64_t{1} << 31) - 1)
    return std::nullopt;
  hipStream_t const s = stream.value();
  auto out            = alloc_pairs(static_cast<std::size_t>(left.num_rows()), s, mr);
  rmm::device_buffer d_args{sizeof(join::dense_stage_args), s, cudf::get_current_device_resource_ref()};
  join::launch_dense_left_direct(dense_stage_of(left, row_base), static_cast<join::dense_stage_args*>(d_args.data()), out.first->data(), out.second->data(), s);
  // (no synchronisation: the scratch goes back to the pool in stream order, the caller reads the result on this stream)
  return out;
}

// inner join of a big probe side against the dense unique table, probe rows partitioned by key range; nullopt: this probe side
// does not take it
std::optional<join_index_pair> hash_join_impl::dense_part_probe(table_view const& left, stream_ref stream, rmm::device_async_resource_ref mr,
                                                                int64_t row_base) const
{
  auto const& col        = left.column(0);
  bool const probe_nulls = _has_nulls && col.has_nulls();
  int64_t const rows     = left.num_rows();
  if ((probe_nulls && _nulls_equal == null_equality::EQUAL) || rows < env_i64("CUDF_AMD_JOIN_DENSE_PART_MIN_PROBE", 8 << 20) ||
      rows > (int64_t{1} << 31) - 1)
    return std::nullopt;
  hipStream_t const s = stream.value();
  auto tmp            = cudf::get_current_device_resource_ref();
  dense_side side;
  dense_partition(key_bytes(col, _key.width), probe_nulls ? col.null_mask() : nullptr, col.offset(), rows, side, stream);
  auto a                     = dense_part_args_of(side);
  std::size_t const nregions = static_cast<std::size_t>(join::dense_part_grid());  // (one stage and one pair count per workgroup)
  a.stage_cap                = join::dense_part_regions_per_workgroup(side.P_used, side.S) * side.cap;
  rmm::device_buffer counts{(nregions + 1) * sizeof(unsigned long long), s, tmp},
    stage{nregions * static_cast<std::size_t>(a.stage_cap) * sizeof(uint64_t), s, tmp}, d_args{sizeof(join::dense_part_args), s, tmp};
  a.pair_counts    = static_cast<unsigned long long*>(counts.data());
  a.stage          = static_cast<uint64_t*>(stage.data());
  a.probe_row_base = row_base;
  join::launch_dense_part_lookup(a, static_cast<join::dense_part_args*>(d_args.data()), s);
  int32_t h_ovf = 0;
  unsigned long long const total =
    scan_total(a.pair_counts, static_cast<int32_t>(nregions), s, static_cast<int32_t const*>(side.ovf.data()), &h_ovf);
  if (h_ovf != 0) return std::nullopt;
  join::radix_join_args e{};  // (the copy of the staged pairs is the radix join's)
  e.nparts      = static_cast<int32_t>(nregions);
  e.pair_counts = a.pair_counts;
  e.stage       = a.stage;
  e.stage_cap   = a.stage_cap;
  return emit_staged(e, total, s, mr);
}

}  // namespace cudf::detail
