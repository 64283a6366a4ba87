// SPDX-License-Identifier: Apache-2.0
// hash_join_impl, the LDS radix join (engine.hpp radix_scatter_args / radix_join_args): two integer key columns packed into one
// word, the two-level ring scatter of either side, the build into LDS-sized partitions and the probe (count pass with staged pairs,
// then the copy).
#include "hash_join_impl.hpp"

#include <algorithm>
#include <cmath>

namespace cudf::detail {

// Two integer key columns whose build-side ranges need at most 63 bits together travel through the radix join as ONE word (engine.hpp
// radix_scatter_args::pack): the exact minimum / maximum of both build columns decide (two passes over the build keys, one read-back).
void hash_join_impl::decide_packed_words(stream_ref stream)
{
  if (env_i64("CUDF_AMD_JOIN_PACK_RANGE", 1) == 0 || _right.num_rows() < 2) return;
  for (int c = 0; c < 2; ++c) {
    auto const cls = class_of(_right.column(c).type().id());
    if (cls != CLS_SINT && cls != CLS_UINT) return;
  }
  uint64_t h[4] = {0, 0, 0, 0};
  rmm::device_buffer d_args;
  if (!key_minmax(2, h, d_args, stream.value())) return;
  int bits[2];
  for (int c = 0; c < 2; ++c) {
    uint64_t const range = h[2 * c + 1] - h[2 * c];
    bits[c]              = 0;
    while (bits[c] < 64 && (range >> bits[c]) != 0) ++bits[c];
  }
  if (bits[0] + bits[1] > 63) return;
  _key.packed = true;
  _key.lo[0] = h[0], _key.lo[1] = h[2];
  _key.range[0] = h[1] - h[0], _key.range[1] = h[3] - h[2];
  _key.bits1 = bits[1];
}

second_key hash_join_impl::second_of(table_view const& t) const
{
  second_key k2{};
  if (!_key.two_columns()) return k2;
  bool const kw2 = _key.shape == key_layout::form::two_words;
  auto const& c  = t.column(1);
  k2.width       = kw2 ? static_cast<int32_t>(size_of_id(c.type().id())) : 0;
  k2.cls         = kw2 ? float_class_of(c) : 0;
  k2.is_signed   = class_of(c.type().id()) == CLS_SINT ? 1 : 0;
  k2.keys        = reinterpret_cast<uint32_t const*>(key_bytes(c, kw2 ? k2.width : 4));
  k2.mask        = (_has_nulls && c.has_nulls()) ? c.null_mask() : nullptr;
  k2.mask_offset = c.offset();
  return k2;
}

// ---- one side's two ring-scatter levels of {key, row id}; false: a region overflowed (heavily duplicated keys)
bool hash_join_impl::radix_partition(uint64_t const* keys, bitmask_type const* mask, int64_t mask_offset, int64_t nrows, int64_t valid_rows,
                                     radix_side& out, stream_ref stream, rmm::device_async_resource_ref mr2, second_key k2,
                                     bool keep_outside) const
{
  hipStream_t const s = stream.value();
  auto tmp            = cudf::get_current_device_resource_ref();
  bool const kw2      = _key.shape == key_layout::form::two_words;
  int64_t const P1 = 128, P2 = _rx_nparts / P1, S1 = std::clamp<int64_t>((nrows + 4095) / 4096, 1, 256), slices2 = 4;
  auto cap_for = [](double mean) {  // six sigmas of a Poisson cell on top of its mean, whole 32-record granules
    return (static_cast<int64_t>(mean + 6.0 * std::sqrt(std::max(mean, 1.0)) + 64.0) + 31) / 32 * 32;
  };
  int64_t const tiles = (nrows + 4095) / 4096, wg_rows = std::min<int64_t>(nrows, (tiles + S1 - 1) / S1 * 4096);
  int64_t const cap1  = cap_for(static_cast<double>(wg_rows) / static_cast<double>(P1));
  int64_t const cap2  = cap_for(static_cast<double>(valid_rows) / static_cast<double>(_rx_nparts * slices2) * 1.02);
  rmm::device_buffer ovf{sizeof(int32_t), s, tmp}, d_args{sizeof(join::radix_scatter_args), s, tmp};
  CUDF_HIP_TRY(hipMemsetAsync(ovf.data(), 0, sizeof(int32_t), s));
  out.key1 = rmm::device_buffer{static_cast<std::size_t>(P1 * S1 * cap1) * 8, s, tmp};
  out.row1 = rmm::device_buffer{static_cast<std::size_t>(P1 * S1 * cap1) * 4, s, tmp};
  out.cnt1 = rmm::device_buffer{static_cast<std::size_t>(P1 * S1) * 4, s, tmp};
  if (_key.two_words()) {
    out.key1w = rmm::device_buffer{static_cast<std::size_t>(P1 * S1 * cap1) * 8, s, tmp};
    out.key2w = rmm::device_buffer{static_cast<std::size_t>(_rx_nparts * slices2 * cap2) * 8, s, mr2};
  }
  out.key2 = rmm::device_buffer{static_cast<std::size_t>(_rx_nparts * slices2 * cap2) * 8, s, mr2};
  out.row2 = rmm::device_buffer{static_cast<std::size_t>(_rx_nparts * slices2 * cap2) * 4, s, mr2};
  out.cnt2 = rmm::device_buffer{static_cast<std::size_t>(_rx_nparts * slices2) * 4, s, mr2};
  out.cap2    = cap2;
  out.slices2 = static_cast<int32_t>(slices2);
  CUDF_HIP_TRY(hipMemsetAsync(out.cnt1.data(), 0, out.cnt1.size(), s));
  CUDF_HIP_TRY(hipMemsetAsync(out.cnt2.data(), 0, out.cnt2.size(), s));
  join::radix_scatter_args a1{};
  a1.level        = 1;
  a1.keys         = keys;
  a1.key_width    = _key.width;
  a1.key_signed   = _key.is_signed ? 1 : 0;
  a1.key_class    = _key.cls;
  a1.keys2        = kw2 ? nullptr : k2.keys;
  a1.kw           = _key.two_words() ? 2 : 1;
  a1.key2         = kw2 ? static_cast<void const*>(k2.keys) : nullptr;
  a1.key2_width   = k2.width;
  a1.key2_class   = k2.cls;
  a1.out_key1     = _key.two_words() ? static_cast<uint64_t*>(out.key1w.data()) : nullptr;
  if (_key.packed) {
    a1.pack              = 1;
    a1.pack_bits1        = _key.bits1;
    a1.pack_keep_outside = keep_outside ? 1 : 0;
    a1.key2_signed       = k2.is_signed;
    a1.pack_lo0 = _key.lo[0], a1.pack_lo1 = _key.lo[1];
    a1.pack_range0 = _key.range[0], a1.pack_range1 = _key.range[1];
  }
  a1.mask2        = k2.mask;
  a1.mask2_offset = k2.mask_offset;
  a1.mask         = mask;
  a1.mask_offset  = mask_offset;
  a1.nrows        = nrows;
  a1.P            = static_cast<int32_t>(P1);
  int const ring_log2 = _key.two_words() ? 12 : 13;  // (two-word keys: half as many ring slots, 2048-row tiles)
  a1.capl         = ring_log2 - ceil_log2(P1);
  a1.shift        = 64 - ceil_log2(P1);
  a1.slices       = static_cast<int32_t>(S1);
  a1.out_key      = static_cast<uint64_t*>(out.key1.data());
  a1.out_row      = static_cast<uint32_t*>(out.row1.data());
  a1.region_cap   = cap1;
  a1.region_count = static_cast<int32_t*>(out.cnt1.data());
  a1.overflow     = static_cast<int32_t*>(ovf.data());
  join::launch_radix_scatter(a1, static_cast<join::radix_scatter_args*>(d_args.data()), s);
  join::radix_scatter_args a2{};
  a2.level           = 2;
  a2.in_key          = a1.out_key;
  a2.kw              = a1.kw;
  a2.in_key1         = a1.out_key1;
  a2.out_key1        = _key.two_words() ? static_cast<uint64_t*>(out.key2w.data()) : nullptr;
  a2.in_row          = a1.out_row;
  a2.in_region_count = a1.region_count;
  a2.in_region_cap   = cap1;
  a2.in_slices       = static_cast<int32_t>(S1);
  a2.nseg            = static_cast<int32_t>(P1);
  a2.P               = static_cast<int32_t>(P2);
  a2.capl            = ring_log2 - ceil_log2(P2);
  a2.shift           = 64 - ceil_log2(P1) - ceil_log2(P2);
  a2.slices          = static_cast<int32_t>(slices2);
  a2.out_key         = static_cast<uint64_t*>(out.key2.data());
  a2.out_row         = static_cast<uint32_t*>(out.row2.data());
  a2.region_cap      = cap2;
  a2.region_count    = static_cast<int32_t*>(out.cnt2.data());
  a2.overflow        = a1.overflow;
  rmm::device_buffer d_args2{sizeof(join::radix_scatter_args), s, tmp};
  join::launch_radix_scatter(a2, static_cast<join::radix_scatter_args*>(d_args2.data()), s);
  int32_t h_ovf = 0;
  CUDF_HIP_TRY(hipMemcpyAsync(&h_ovf, ovf.data(), sizeof(int32_t), hipMemcpyDeviceToHost, s));
  CUDF_HIP_TRY(hipStreamSynchronize(s));
  out.key1  = rmm::device_buffer{};  // (the first level's regions go back to the pool)
  out.key1w = rmm::device_buffer{};
  out.row1 = rmm::device_buffer{};
  out.cnt1 = rmm::device_buffer{};
  return h_ovf == 0;
}

// ---- build side: false if it does not take the radix join (too small or too big for 2048 ... 32768 partitions, a region or a
// partition that overflows: heavily duplicated keys)
bool hash_join_impl::try_radix_build(table_view const& right, stream_ref stream)
{
  auto const& col     = right.column(0);
  int64_t const rows  = right.num_rows();
  // (two packed columns: the rows with a NULL in either are dropped; their number is at least the larger of the two null counts)
  int64_t const valid = rows - std::max<int64_t>(col.nullable() ? col.null_count() : 0, (_key.two_columns() && right.column(1).nullable()) ? right.column(1).null_count() : 0);
  // partitions: a power of two with at most ~3500 build rows each (LDS tables of 8192 slots: load <= 0.43), 128 x (16 ... 256)
  int64_t nparts = 2048;
  while (nparts < (_key.two_words() ? 16384 : 32768) && valid > nparts * 3500) nparts <<= 1;  // (two-word keys: second-level rings of at least 32 slots)
  if (valid < env_i64("CUDF_AMD_JOIN_RADIX_MIN_BUILD", 3 << 20) || valid > nparts * 3500) return false;
  _rx_nparts = static_cast<int32_t>(nparts);
  hipStream_t const s = stream.value();
  if (!radix_partition(key_bytes(col, _key.width), (_has_nulls && col.has_nulls()) ? col.null_mask() : nullptr, col.offset(), rows, valid, _rx_build, stream, _mr,
                       second_of(right)))
    return false;
  // every partition must fit its LDS table
  auto tmp = cudf::get_current_device_resource_ref();
  rmm::device_buffer mx{sizeof(int32_t), s, tmp};
  CUDF_HIP_TRY(hipMemsetAsync(mx.data(), 0, sizeof(int32_t), s));
  join::launch_radix_partition_max(static_cast<int32_t const*>(_rx_build.cnt2.data()), _rx_nparts, _rx_build.slices2, static_cast<int32_t*>(mx.data()), s);
  int32_t h_max = 0;
  CUDF_HIP_TRY(hipMemcpyAsync(&h_max, mx.data(), sizeof(int32_t), hipMemcpyDeviceToHost, s));
  CUDF_HIP_TRY(hipStreamSynchronize(s));
  if (h_max > RADIX_FILL_LIMIT) {
    _rx_build = radix_side{};
    return false;
  }
  _state = build_state::radix;
  return true;
}

// inner or left join of a big probe side against the radix-partitioned build side; nullopt: this probe side does not take it.
// size_only != nullptr: the count pass only - *size_only = the number of pairs, the pair holds no vectors (inner / left_join_size
// against a radix build: no second copy of the build side in an open-addressing table just to count)
std::optional<join_index_pair> hash_join_impl::radix_probe(table_view const& left, stream_ref stream, rmm::device_async_resource_ref mr,
                                                           int64_t row_base, bool left_join, std::size_t* size_only) const
{
  auto const& col         = left.column(0);
  bool const probe_nulls  = _has_nulls && col.has_nulls();
  bool const second_nulls = _key.two_columns() && _has_nulls && left.column(1).has_nulls();
  // (a NULL that could match; a left join of two key columns with NULLs: the rows dropped for a NULL in either column are not one
  // column's null count)
  if ((probe_nulls || second_nulls) && (_nulls_equal == null_equality::EQUAL || (left_join && _key.two_columns()))) return std::nullopt;
  int64_t const rows  = left.num_rows();
  int64_t const valid = rows - std::max<int64_t>(col.nullable() ? col.null_count() : 0, second_nulls ? left.column(1).null_count() : 0);
  if (rows < env_i64("CUDF_AMD_JOIN_RADIX_MIN_PROBE", 8 << 20) || rows > (int64_t{1} << 31) - 1) return std::nullopt;
  hipStream_t const s = stream.value();
  auto tmp            = cudf::get_current_device_resource_ref();
  radix_side probe;
  if (!radix_partition(key_bytes(col, _key.width), probe_nulls ? col.null_mask() : nullptr, col.offset(), rows, valid, probe, stream, tmp,
                       second_of(left), left_join))
    return std::nullopt;
  rmm::device_buffer counts{(static_cast<std::size_t>(_rx_nparts) + 1) * sizeof(unsigned long long), s, tmp}, ovf{sizeof(int32_t), s, tmp},
    d_args{sizeof(join::radix_join_args), s, tmp};
  CUDF_HIP_TRY(hipMemsetAsync(ovf.data(), 0, sizeof(int32_t), s));
  join::radix_join_args a{};
  a.kw          = _key.two_words() ? 2 : 1;
  a.b_key1      = _key.two_words() ? static_cast<uint64_t const*>(_rx_build.key2w.data()) : nullptr;
  a.p_key1      = _key.two_words() ? static_cast<uint64_t const*>(probe.key2w.data()) : nullptr;
  a.b_key       = static_cast<uint64_t const*>(_rx_build.key2.data());
  a.b_row       = static_cast<uint32_t const*>(_rx_build.row2.data());
  a.b_count     = static_cast<int32_t const*>(_rx_build.cnt2.data());
  a.b_cap       = _rx_build.cap2;
  a.b_slices    = _rx_build.slices2;
  a.p_key       = static_cast<uint64_t const*>(probe.key2.data());
  a.p_row       = static_cast<uint32_t const*>(probe.row2.data());
  a.p_count     = static_cast<int32_t const*>(probe.cnt2.data());
  a.p_cap       = probe.cap2;
  a.p_slices    = probe.slices2;
  a.nparts      = _rx_nparts;
  a.cap         = RADIX_TABLE_SLOTS;
  a.fill_limit  = RADIX_FILL_LIMIT;
  a.pair_counts = static_cast<unsigned long long*>(counts.data());
  a.probe_row_base = row_base;
  a.overflow    = static_cast<int32_t*>(ovf.data());
  a.left        = left_join ? 1 : 0;
  a.stage_cap   = probe.cap2 * probe.slices2;  // (as many pairs as the partition has room for probe rows: enough unless keys repeat a lot)
  rmm::device_buffer stage{static_cast<std::size_t>(_rx_nparts) * static_cast<std::size_t>(a.stage_cap) * sizeof(uint64_t), s, tmp};
  a.stage = static_cast<uint64_t*>(stage.data());
  join::launch_radix_join(a, static_cast<join::radix_join_args*>(d_args.data()), false, s);
  int32_t h_ovf                  = 0;
  unsigned long long const total = scan_total(a.pair_counts, _rx_nparts, s, a.overflow, &h_ovf);
  if ((h_ovf & 3) != 0) return std::nullopt;
  // (left join: the probe rows with a NULL key never entered a partition; their {row, JoinNoMatch} pairs follow the partitions')
  unsigned long long const null_rows = (left_join && probe_nulls) ? static_cast<unsigned long long>(col.null_count()) : 0ull;
  unsigned long long const pairs_all = total + null_rows;
  if (size_only != nullptr) {
    *size_only = static_cast<std::size_t>(pairs_all);
    return join_index_pair{nullptr, nullptr};
  }
  auto out = emit_staged(a, pairs_all, s, mr);
  // (a partition whose pairs overflowed its stage is joined again; the count pass's argument buffer is free again in stream order)
  if ((h_ovf & 4) != 0) join::launch_radix_join(a, static_cast<join::radix_join_args*>(d_args.data()), true, s);
  if (null_rows != 0)  // (pair_counts[nparts] = the number of pairs of the partitions: the cursor the NULL rows append at)
    join::launch_radix_null_rows(col.null_mask(), col.offset(), rows, row_base, a.out_probe, a.out_build, pairs_all, a.pair_counts + _rx_nparts, s);
  // (no synchronisation: the scratch goes back to the pool in stream order, the caller reads the result on this stream)
  return out;
}

}  // namespace cudf::detail
