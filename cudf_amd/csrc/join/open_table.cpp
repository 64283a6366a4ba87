// SPDX-License-Identifier: Apache-2.0
// hash_join_impl, the tables' own passes (engine.hpp join_args): the open-addressing multiset in HBM (slots of {hash tag | build
// row}, linear window + key-dependent stride) - what every probe used before the partitioned joins and what everything they do not
// take still uses - and the count -> scan -> retrieve (-> complement) passes over it or over the dense direct-address table.
#include "hash_join_impl.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace cudf::detail {

join_args hash_join_impl::base_args(table_view const& probe, int kind) const
{
  join_args a{};
  a.build       = _build_dev;
  a.probe       = make_device_table(probe);
  a.table       = const_cast<uint64_t*>(static_cast<uint64_t const*>(_table.data()));
  a.capacity    = _capacity;
  a.nulls_equal = _nulls_equal == null_equality::EQUAL;
  a.check_nulls = _has_nulls && (cudf::has_nulls(_right) || cudf::has_nulls(probe));
  a.kind        = kind;
  if (_state == build_state::dense_part8 || _state == build_state::dense_unique || _state == build_state::dense_csr) {
    a.dense_head     = const_cast<int32_t*>(static_cast<int32_t const*>(_dense_head.data()));
    a.dense_next     = const_cast<int32_t*>(static_cast<int32_t const*>(_dense_next.data()));
    a.dense_lo       = _dense_lo;
    a.dense_range    = _dense_range;
    a.dense_has_dups = _state == build_state::dense_csr ? 1 : 0;
  }
  // one 8-byte integer key per side (the probe side has the build side's types: validate_probe); NULLs are fine as long as they
  // can never match (UNEQUAL): then every key comparison is between valid values and needs no descriptor walk
  a.single64    = _key.shape == key_layout::form::one && _key.width == 8 && _key.cls == 0 && (!a.check_nulls || !a.nulls_equal);
  // one workgroup per contiguous chunk of probe rows (>= 2048 rows each, at most 16 workgroups per CU)
  int64_t const n = probe.num_rows();
  a.nblocks       = static_cast<int32_t>(std::clamp<int64_t>((n + 2047) / 2048, 1, 256 * 16));
  a.chunk         = (n + a.nblocks - 1) / a.nblocks;
  a.chunk         = (a.chunk + 1023) / 1024 * 1024;
  return a;
}

void hash_join_impl::build_classic(stream_ref stream) const
{
  auto const rows     = static_cast<uint64_t>(_right.num_rows());
  double const target_load = std::min(_classic_load, 0.25);
  uint64_t capacity = static_cast<uint64_t>(std::ceil(static_cast<double>(rows) / target_load));
  if (capacity * 8 > (uint64_t{36} << 30)) capacity = static_cast<uint64_t>(std::ceil(static_cast<double>(rows) / _classic_load));
  capacity          = std::clamp<uint64_t>(capacity, rows + 1, (uint64_t{1} << 32) - 2);  // always one empty slot
  capacity          = std::min<uint64_t>((capacity + 1) / 2 * 2, ((uint64_t{1} << 32) - 1) / 2 * 2);  // even: 16-byte aligned slot pairs
  rmm::device_buffer table{capacity * sizeof(uint64_t), stream.value(), _mr};
  CUDF_HIP_TRY(hipMemsetAsync(table.data(), 0xff, capacity * sizeof(uint64_t), stream.value()));
  join_args a = base_args(_right, 0);
  a.table     = static_cast<uint64_t*>(table.data());
  a.capacity  = capacity;
  rmm::device_buffer d_args{sizeof(join_args), stream.value(), cudf::get_current_device_resource_ref()};
  rmm::device_buffer skip{sizeof(uint64_t) * join::BUILD_SKIP_ENTRIES, stream.value(), cudf::get_current_device_resource_ref()};
  CUDF_HIP_TRY(hipMemsetAsync(skip.data(), 0xff, skip.size(), stream.value()));  // no home slot is 2^40 - 1
  a.build_skip = static_cast<uint64_t*>(skip.data());
  join::launch_build(a, static_cast<join_args*>(d_args.data()), stream.value());
  CUDF_HIP_TRY(hipStreamSynchronize(stream.value()));  // d_args goes out of scope; build is done for probes on any stream
  _table    = std::move(table);  // (only a finished table is kept: a failed build is tried again by the next call)
  _capacity = capacity;
}

// the lazy states build the open table on first need (probes are const and may run concurrently)
void hash_join_impl::ensure_classic(stream_ref stream) const
{
  std::lock_guard<std::mutex> g{_classic_mu};
  if (_capacity == 0 && (_state == build_state::radix || _state == build_state::dense_part4)) build_classic(stream);
}

// the count pass over a's probe rows: per-workgroup pair counts (a.block_counts, scan_total makes them offsets) and the per-row
// match cache of the retrieve pass (a.match_cache), in the returned scratch
hash_join_impl::count_scratch hash_join_impl::count_pass(join_args& a, hipStream_t s) const
{
  auto tmp = cudf::get_current_device_resource_ref();
  count_scratch c{rmm::device_buffer{(static_cast<std::size_t>(a.nblocks) + 1) * sizeof(unsigned long long), s, tmp},
                  rmm::device_buffer{static_cast<std::size_t>(a.probe.nrows) * sizeof(uint32_t), s, tmp},
                  rmm::device_buffer{sizeof(join_args), s, tmp}};
  a.block_counts = static_cast<unsigned long long*>(c.counts.data());
  a.match_cache  = static_cast<uint32_t*>(c.cache.data());
  auto* d_args = static_cast<join_args*>(c.d_args.data());
  if (a.dense_head != nullptr) join::launch_dense_count(a, d_args, s);  // (base_args sets dense_head from _state)
  else join::launch_count(a, d_args, s);
  return c;
}

std::unique_ptr<rmm::device_uvector<size_type>> hash_join_impl::match_counts(table_view const& left, join_kind kind, stream_ref stream,
                                                                             rmm::device_async_resource_ref mr) const
{
  validate_probe(left);
  hipStream_t const s = stream.value();
  auto const n        = static_cast<std::size_t>(left.num_rows());
  auto out            = std::make_unique<rmm::device_uvector<size_type>>(n, s, mr);
  if (n == 0) return out;
  if (_state == build_state::empty) {  // nothing to match: 0 per row, or the row's own JoinNoMatch pair
    std::vector<size_type> h(n, kind == join_kind::INNER_JOIN ? 0 : 1);
    CUDF_HIP_TRY(hipMemcpyAsync(out->data(), h.data(), n * sizeof(size_type), hipMemcpyHostToDevice, s));
    CUDF_HIP_TRY(hipStreamSynchronize(s));
    return out;
  }
  ensure_classic(stream);
  join_args a  = base_args(left, kind == join_kind::INNER_JOIN ? 0 : 1);
  a.row_counts = out->data();
  auto scratch = count_pass(a, s);
  CUDF_HIP_TRY(hipStreamSynchronize(s));
  return out;
}

// count (match cache, per-workgroup pair counts) -> scan -> retrieve (-> complement) over the open-addressing table in HBM or the
// dense direct-address table (rounds 1 and 2)
join_index_pair hash_join_impl::probe_tables(table_view const& left, join_kind kind, int k, std::optional<std::size_t> output_size,
                                             stream_ref stream, rmm::device_async_resource_ref mr, int64_t row_base) const
{
  hipStream_t const s = stream.value();
  ensure_classic(stream);
  // ---- size: given, or counted with one probe pass (reference: compute_join_output_size, size_impl.cuh:26-61)
  // The count pass always runs: its per-workgroup counts place every pair without global atomics (the pass
  // costs ~6% of the retrieve it replaces); a caller-supplied output_size is checked against it.
  join_args a      = base_args(left, k == 0 ? 0 : 1);
  a.probe_row_base = row_base;
  auto scratch     = count_pass(a, s);
  auto* d_args     = static_cast<join_args*>(scratch.d_args.data());
  std::size_t const pairs = static_cast<std::size_t>(scan_total(a.block_counts, a.nblocks, s));
  if (output_size.has_value() && kind != join_kind::FULL_JOIN)
    CUDF_EXPECTS(*output_size == pairs, "hash join: output_size does not match the number of matches", std::invalid_argument);
  std::size_t const room = pairs + (kind == join_kind::FULL_JOIN ? static_cast<std::size_t>(_right.num_rows()) : 0);
  auto out               = alloc_pairs(room, s, mr);
  a.kind = k;
  dev_scalar<unsigned long long> cursor{static_cast<unsigned long long>(pairs), s};  // complement appends after the pairs
  a.total        = cursor.ptr();
  a.out_probe    = out.first->data();
  a.out_build    = out.second->data();
  a.out_capacity = room;
  rmm::device_buffer matched{};
  if (kind == join_kind::FULL_JOIN) {
    matched = rmm::device_buffer{static_cast<std::size_t>(_right.num_rows()), s, cudf::get_current_device_resource_ref()};
    CUDF_HIP_TRY(hipMemsetAsync(matched.data(), 0, matched.size(), s));
    a.build_matched = static_cast<uint8_t*>(matched.data());
  }
  rmm::device_buffer big{};
  if (_state == build_state::dense_csr) {  // work list for probe rows that hit a hot build key (engine.hpp join_args::big_list)
    big = rmm::device_buffer{(5 * static_cast<std::size_t>(join::BIG_LIST_CAP) + 4) * sizeof(uint32_t), s, cudf::get_current_device_resource_ref()};
    a.big_list  = static_cast<uint32_t*>(big.data());
    a.big_count = a.big_list + 5 * static_cast<std::size_t>(join::BIG_LIST_CAP);
    CUDF_HIP_TRY(hipMemsetAsync(a.big_count, 0, sizeof(uint32_t), s));
  }
  if (a.dense_head != nullptr) join::launch_dense_retrieve(a, d_args, s);
  else join::launch_retrieve(a, d_args, s);
  if (a.big_list != nullptr) join::launch_dense_big_emit(d_args, s);
  if (kind == join_kind::FULL_JOIN) {
    join::launch_complement(a.build_matched, _right.num_rows(), a.total, a.out_probe, a.out_build, a.out_capacity, s);
    std::size_t const total = static_cast<std::size_t>(cursor.value());
    if (total != room) {  // exact-size outputs
      auto exact = alloc_pairs(total, s, mr);
      CUDF_HIP_TRY(hipMemcpyAsync(exact.first->data(), out.first->data(), total * sizeof(size_type), hipMemcpyDeviceToDevice, s));
      CUDF_HIP_TRY(hipMemcpyAsync(exact.second->data(), out.second->data(), total * sizeof(size_type), hipMemcpyDeviceToDevice, s));
      CUDF_HIP_TRY(hipStreamSynchronize(s));
      return exact;
    }
    return out;
  }
  CUDF_HIP_TRY(hipStreamSynchronize(s));  // d_args / counts go out of scope
  return out;
}

}  // namespace cudf::detail
