// SPDX-License-Identifier: Apache-2.0
// Host side of cudf::filtered_join (include/cudf/join/filtered_join.hpp): the choice of build form, validation, the trivial cases and
// the two probes. Reference counterpart: cpp/src/join/filtered_join/filtered_join.cu (constructor, semi_anti_join, semi_join,
// anti_join). Build forms and kernels: filtered_join_impl.hpp, filtered_join_kernels.hip; the model: DESIGN.md section 4, "Semi and anti joins".
#include "filtered_join_impl.hpp"
#include "../common/profiler.hpp"
#include "../common/row_set_host.hpp"

#include <algorithm>

namespace cudf {
namespace detail {

namespace {
std::unique_ptr<rmm::device_uvector<size_type>> no_rows(stream_ref stream, rmm::device_async_resource_ref mr)
{
  return std::make_unique<rmm::device_uvector<size_type>>(0, stream.value(), mr);
}
}  // namespace

filtered_join_impl::filtered_join_impl(table_view const& right, null_equality compare_nulls, double load_factor, stream_ref stream,
                                       rmm::device_async_resource_ref mr)
  : _right{right}, _nulls_equal{compare_nulls}, _mr{mr}
{
  load_factor = checked_load_factor(load_factor);
  if (right.num_rows() == 0) return;
  _build_dev = make_device_table(right);
  if (try_bitmap_build(stream)) return;
  set_build(load_factor, stream);
}

// One integer key column whose valid build keys span a small range takes the bitmap (rowset::small_key_range): at most
// CUDF_AMD_FJOIN_DENSE_RATIO (32) bits per build row and at most CUDF_AMD_FJOIN_DENSE_MAX_BITS (2^31: 256 MiB, the Infinity Cache)
// bits. CUDF_AMD_FJOIN_DENSE=0 sends every key to the hash set.
bool filtered_join_impl::try_bitmap_build(stream_ref stream)
{
  if (_right.num_columns() != 1 || env_i64("CUDF_AMD_FJOIN_DENSE", 1) == 0) return false;
  device_column const& c = _build_dev.col[0];
  hipStream_t const s    = stream.value();
  auto const ratio       = static_cast<uint64_t>(std::clamp<int64_t>(env_i64("CUDF_AMD_FJOIN_DENSE_RATIO", 32), 0, int64_t{1} << 32));
  auto const max_bits    = static_cast<uint64_t>(std::max<int64_t>(env_i64("CUDF_AMD_FJOIN_DENSE_MAX_BITS", int64_t{1} << 31), 0));
  auto const r           = rowset::small_key_range(c, _right.num_rows(), _right.num_rows(), ratio, max_bits, s);
  if (!r) return false;
  _lo    = r->lo;
  _range = r->range;
  _bits  = rmm::device_buffer{std::max<std::size_t>(1, static_cast<std::size_t>((_range + 127) >> 7)) * 16, s, _mr};
  CUDF_HIP_TRY(hipMemsetAsync(_bits.data(), 0, _bits.size(), s));
  dev_scalar<int32_t> seen_null{0, s};
  fjoin::bitmap_args b{};
  b.key       = c;
  b.nrows     = _right.num_rows();
  b.lo        = _lo;
  b.range     = _range;
  b.bits      = static_cast<uint32_t*>(_bits.data());
  b.seen_null = seen_null.ptr();
  fjoin::launch_bitmap_build(b, s);
  _null_match = _nulls_equal == null_equality::EQUAL && seen_null.value() != 0;  // (synchronises)
  _form       = fjoin::form::bitmap;
  return true;
}

// The open-addressing set of the distinct build rows (rowset::set_capacity slots).
void filtered_join_impl::set_build(double load_factor, stream_ref stream)
{
  hipStream_t const s = stream.value();
  _capacity           = rowset::set_capacity(_right.num_rows(), load_factor, "filtered_join: the hash set");
  _inline_key         = rowset::inline_key_column(_build_dev);
  _slots = rmm::device_buffer{static_cast<std::size_t>(_capacity) * sizeof(uint64_t), s, _mr};
  CUDF_HIP_TRY(hipMemsetAsync(_slots.data(), 0xff, _slots.size(), s));
  dev_scalar<uint64_t> seen{0, s};  // {NULL key, rowset::EMPTY key}
  fjoin::set_args a{};
  a.build         = _build_dev;
  a.slots         = static_cast<uint64_t*>(_slots.data());
  a.capacity      = _capacity;
  a.inline_key    = _inline_key ? 1 : 0;
  a.nulls_equal   = _nulls_equal == null_equality::EQUAL ? 1 : 0;
  a.seen_null     = reinterpret_cast<int32_t*>(seen.ptr());
  a.seen_sentinel = reinterpret_cast<int32_t*>(seen.ptr()) + 1;
  fjoin::launch_set_build(a, s);
  uint64_t const flags = seen.value();  // (synchronises)
  _null_match          = _inline_key && a.nulls_equal && (flags & 0xffffffffu) != 0;
  _sentinel_match      = _inline_key && (flags >> 32) != 0;
  _form                = fjoin::form::set;
}

std::unique_ptr<rmm::device_uvector<size_type>> filtered_join_impl::probe(table_view const& left, bool anti, stream_ref stream,
                                                                          rmm::device_async_resource_ref mr) const
{
  hipStream_t const s = stream.value();
  int64_t const n     = left.num_rows();
  // trivial cases first, as the reference (filtered_join.cu semi_join / anti_join): no left rows, or no right rows
  if (n == 0) return no_rows(stream, mr);
  if (_form == fjoin::form::empty) {
    if (!anti) return no_rows(stream, mr);
    auto out = std::make_unique<rmm::device_uvector<size_type>>(static_cast<std::size_t>(n), s, mr);
    fjoin::launch_fjoin_sequence(out->data(), n, s);
    return out;
  }
  rowset::validate_probe(_right, left, "Filtered join");
  rowset::compaction c{n, s};
  fjoin::probe_args a{};
  a.probe          = make_device_table(left);
  a.anti           = anti ? 1 : 0;
  a.null_match     = _null_match ? 1 : 0;
  a.sentinel_match = _sentinel_match ? 1 : 0;
  a.nrows          = n;
  a.chunk          = c.g.chunk;
  a.nwaves         = c.g.nwaves;
  a.mask           = c.mask();
  a.counts         = c.counts();
  if (_form == fjoin::form::bitmap) {
    a.bm.key   = _build_dev.col[0];
    a.bm.lo    = _lo;
    a.bm.range = _range;
    a.bm.bits  = static_cast<uint32_t*>(const_cast<void*>(_bits.data()));
    // CUDF_AMD_FJOIN_LDS_BITS (2^20): the largest bitmap probed from LDS (at most the kernel's 128 KiB)
    auto const lds_bits = static_cast<uint64_t>(std::max<int64_t>(env_i64("CUDF_AMD_FJOIN_LDS_BITS", int64_t{1} << 20), 0));
    fjoin::launch_bitmap_probe(a, _range <= std::min(lds_bits, fjoin::lds_bits_max()), s);
  } else {
    a.set.build       = _build_dev;
    a.set.slots       = static_cast<uint64_t*>(const_cast<void*>(_slots.data()));
    a.set.capacity    = _capacity;
    a.set.inline_key  = _inline_key ? 1 : 0;
    a.set.nulls_equal = _nulls_equal == null_equality::EQUAL ? 1 : 0;
    fjoin::launch_set_probe(a, s);
  }
  return std::make_unique<rmm::device_uvector<size_type>>(c.compact_indices(s, mr));
}

}  // namespace detail

// ---------------------------------------------------------------- cudf::filtered_join
filtered_join::~filtered_join() = default;

filtered_join::filtered_join(table_view const& right, null_equality compare_nulls, stream_ref stream, rmm::device_async_resource_ref mr)
  : filtered_join{right, compare_nulls, 0.5, stream, mr}  // (reference default load factor, filtered_join.cu)
{
}

filtered_join::filtered_join(table_view const& right, null_equality compare_nulls, double load_factor, stream_ref stream,
                             rmm::device_async_resource_ref mr)
  : _impl{[&] {
      CUDF_FUNC_RANGE();
      return std::make_unique<detail::filtered_join_impl const>(right, compare_nulls, load_factor, stream, mr);
    }()}
{
}

std::unique_ptr<rmm::device_uvector<size_type>> filtered_join::semi_join(table_view const& left, stream_ref stream,
                                                                         rmm::device_async_resource_ref mr) const
{
  CUDF_FUNC_RANGE();
  return _impl->probe(left, false, stream, mr);
}

std::unique_ptr<rmm::device_uvector<size_type>> filtered_join::anti_join(table_view const& left, stream_ref stream,
                                                                         rmm::device_async_resource_ref mr) const
{
  CUDF_FUNC_RANGE();
  return _impl->probe(left, true, stream, mr);
}

}  // namespace cudf
