// SPDX-License-Identifier: Apache-2.0
// Host side of cudf::distinct_hash_join (include/cudf/join/distinct_hash_join.hpp): the choice of build form, validation, the
// trivial cases and the two probes. Reference counterpart: cpp/src/join/distinct_hash_join.cu (constructor, inner_join, left_join).
// Build forms and kernels: distinct_join_impl.hpp, distinct_join_kernels.hip; the model: DESIGN.md section 4, "Joins on a
// unique-key build table".
#include "distinct_join_impl.hpp"
#include "../common/profiler.hpp"
#include "../common/row_set_host.hpp"

#include <algorithm>

namespace cudf {
namespace detail {

distinct_join_impl::distinct_join_impl(table_view const& right, null_equality compare_nulls, double load_factor, stream_ref stream,
                                       rmm::device_async_resource_ref mr)
  : _right{right}, _nulls_equal{compare_nulls}, _mr{mr}
{
  load_factor = checked_load_factor(load_factor);
  CUDF_EXPECTS(0 != right.num_columns(), "Hash join right table is empty");  // (reference distinct_hash_join.cu:174)
  if (right.num_rows() == 0) return;
  _table.build       = make_device_table(right);
  _table.nulls_equal = _nulls_equal == null_equality::EQUAL ? 1 : 0;
  if (try_direct_build(stream)) return;
  map_build(load_factor, stream);
}

// The two side words, preset to JoinNoMatch (distinct_join_impl.hpp, table_args::side).
void distinct_join_impl::alloc_side(hipStream_t s)
{
  _side = rmm::device_buffer{2 * sizeof(size_type), s, _mr};
  CUDF_HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(_side.data()), JoinNoMatch, 2, s));
  _table.side = static_cast<size_type*>(_side.data());
}

// One integer or bool key column whose valid build keys span a small range takes the direct table (rowset::small_key_range): at
// most CUDF_AMD_DJOIN_DENSE_RATIO (8) entries per build row and the table at most CUDF_AMD_DJOIN_DENSE_MAX_BYTES (2^31) bytes.
// CUDF_AMD_DJOIN_DENSE=0 sends every key to the map.
bool distinct_join_impl::try_direct_build(stream_ref stream)
{
  if (_right.num_columns() != 1 || env_i64("CUDF_AMD_DJOIN_DENSE", 1) == 0) return false;
  device_column const& c = _table.build.col[0];
  hipStream_t const s    = stream.value();
  auto const ratio       = static_cast<uint64_t>(std::clamp<int64_t>(env_i64("CUDF_AMD_DJOIN_DENSE_RATIO", 8), 0, int64_t{1} << 32));
  auto const max_bytes   = static_cast<uint64_t>(std::max<int64_t>(env_i64("CUDF_AMD_DJOIN_DENSE_MAX_BYTES", int64_t{1} << 31), 0));
  auto const r = rowset::small_key_range(c, _right.num_rows(), _right.num_rows(), ratio, max_bytes / sizeof(size_type), s, true);
  if (!r) return false;
  if (r->range == 0 && !_table.nulls_equal) return true;  // no valid build key and a NULL matches nothing: the empty form
  // the table counts within the key's width: 1- and 2-byte keys index it by their raw bits, and of the first key of a 4-byte
  // column (which small_key_range widens to 64 bits) it keeps the raw bits
  uint64_t const range = r->range;
  uint64_t const lo    = c.width <= 2 ? 0 : c.width == 4 ? r->lo & 0xffffffffu : r->lo;
  auto const entries   = static_cast<std::size_t>(std::max<uint64_t>(range, 1));
  _entries           = rmm::device_buffer{entries * sizeof(size_type), s, _mr};
  CUDF_HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(_entries.data()), JoinNoMatch, entries, s));
  alloc_side(s);
  _table.lo         = lo;
  _table.range      = range;
  _table.direct     = static_cast<size_type*>(_entries.data());
  _table.table_form = static_cast<int32_t>(djoin::form::direct);
  djoin::launch_build(_table, s);
  return true;
}

// The open-addressing map of the build rows (rowset::set_capacity slots).
void distinct_join_impl::map_build(double load_factor, stream_ref stream)
{
  hipStream_t const s = stream.value();
  auto const kind     = !rowset::inline_key_column(_table.build) ? djoin::map_kind::rows
                        : _table.build.col[0].width == 4         ? djoin::map_kind::key4
                                                                 : djoin::map_kind::key8;
  _table.capacity     = rowset::set_capacity(_right.num_rows(), load_factor, "distinct_hash_join: the hash map");
  _table.kind         = static_cast<int32_t>(kind);
  _entries = rmm::device_buffer{static_cast<std::size_t>(_table.capacity) * (kind == djoin::map_kind::key8 ? 16 : 8), s, _mr};
  CUDF_HIP_TRY(hipMemsetAsync(_entries.data(), 0xff, _entries.size(), s));
  alloc_side(s);
  _table.slots      = static_cast<uint64_t*>(_entries.data());
  _table.table_form = static_cast<int32_t>(djoin::form::map);
  djoin::launch_build(_table, s);
}

djoin::probe_args distinct_join_impl::probe_args_of(table_view const& left) const
{
  rowset::validate_probe(_right, left, "Distinct hash join");  // (the reference checks nothing here)
  rowset::geometry const g = rowset::geometry_of(left.num_rows());
  djoin::probe_args a{};
  a.probe  = make_device_table(left);
  a.t      = _table;
  a.nrows  = left.num_rows();
  a.chunk  = g.chunk;
  a.nwaves = g.nwaves;
  return a;
}

join_index_pair distinct_join_impl::inner_join(table_view const& left, stream_ref stream, rmm::device_async_resource_ref mr) const
{
  hipStream_t const s = stream.value();
  int64_t const n     = left.num_rows();
  // trivial cases first, as the reference (distinct_hash_join.cu inner_join): no left rows, or no right rows
  if (n == 0 || _table.table_form == static_cast<int32_t>(djoin::form::empty)) return alloc_pairs(0, s, mr);
  djoin::probe_args a = probe_args_of(left);
  rmm::device_buffer found{static_cast<std::size_t>(n) * sizeof(size_type), s, cudf::get_current_device_resource_ref()};
  rowset::compaction c{n, s};
  a.found  = static_cast<size_type*>(found.data());
  a.mask   = c.mask();
  a.counts = c.counts();
  djoin::launch_probe(a, s);
  auto const total = c.total(s);
  auto out         = alloc_pairs(static_cast<std::size_t>(total), s, mr);
  a.out_left       = out.first->data();
  a.out_right      = out.second->data();
  a.out_capacity   = total;
  if (total > 0) djoin::launch_compact(a, s);
  // (no synchronisation: the scratch goes back to the pool in stream order, the caller reads the result on this stream)
  return out;
}

// One pass, nothing read back: the probe writes the result itself.
std::unique_ptr<rmm::device_uvector<size_type>> distinct_join_impl::left_join(table_view const& left, stream_ref stream,
                                                                              rmm::device_async_resource_ref mr) const
{
  hipStream_t const s = stream.value();
  int64_t const n     = left.num_rows();
  auto out            = std::make_unique<rmm::device_uvector<size_type>>(static_cast<std::size_t>(n), s, mr);
  if (n == 0) return out;
  if (_table.table_form == static_cast<int32_t>(djoin::form::empty)) {
    CUDF_HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(out->data()), JoinNoMatch, static_cast<std::size_t>(n), s));
    return out;
  }
  djoin::probe_args a = probe_args_of(left);
  a.found             = out->data();
  djoin::launch_probe(a, s);
  return out;
}

}  // namespace detail

// ---------------------------------------------------------------- cudf::distinct_hash_join
distinct_hash_join::~distinct_hash_join() = default;

distinct_hash_join::distinct_hash_join(table_view const& right, null_equality compare_nulls, double load_factor, stream_ref stream,
                                       rmm::device_async_resource_ref mr)
  : _impl{[&] {
      CUDF_FUNC_RANGE();
      return std::make_unique<detail::distinct_join_impl const>(right, compare_nulls, load_factor, stream, mr);
    }()}
{
}

std::pair<std::unique_ptr<rmm::device_uvector<size_type>>, std::unique_ptr<rmm::device_uvector<size_type>>> distinct_hash_join::inner_join(
  table_view const& left, stream_ref stream, rmm::device_async_resource_ref mr) const
{
  CUDF_FUNC_RANGE();
  return _impl->inner_join(left, stream, mr);
}

std::unique_ptr<rmm::device_uvector<size_type>> distinct_hash_join::left_join(table_view const& left, stream_ref stream,
                                                                              rmm::device_async_resource_ref mr) const
{
  CUDF_FUNC_RANGE();
  return _impl->left_join(left, stream, mr);
}

}  // namespace cudf
