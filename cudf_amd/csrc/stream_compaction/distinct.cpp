// SPDX-License-Identifier: Apache-2.0
// Host side of cudf::distinct, distinct_indices, stable_distinct (include/cudf/stream_compaction.hpp) and cudf::distinct_count
// (include/cudf/reduction/distinct_count.hpp): the choice of form, the trivial cases, the build -> sweep -> ordered compaction
// sequence and the gather. Reference counterparts: cpp/src/stream_compaction/{distinct.cu,stable_distinct.cu},
// cpp/src/reductions/distinct_count.cu. Forms and kernels: distinct_impl.hpp, distinct_kernels.hip; the model: DESIGN.md
// section 4, "Distinct rows".
#include "distinct_impl.hpp"
#include "../common/env.hpp"
#include "../common/profiler.hpp"
#include "../common/row_set_host.hpp"

#include <cudf/copying.hpp>
#include <cudf/reduction/distinct_count.hpp>
#include <cudf/stream_compaction.hpp>

#include <algorithm>

namespace cudf {
namespace detail {
namespace distinct {
namespace {

// The state of one build over a key table: the form's buffers and the kernel arguments that point at them.
struct table_state {
  build_args a{};
  uint64_t lds_entries{0};  // dense: > 0 when the build reduces in LDS first
  bool dense{false};
  rmm::device_buffer state, slots, special, counter;
};

// One integer key column takes the dense form (rowset::small_key_range) when its valid keys span at most
// CUDF_AMD_DISTINCT_DENSE_RATIO (2) state words per row and CUDF_AMD_DISTINCT_DENSE_MAX_ENTRIES (2^28: 1 GiB).
// CUDF_AMD_DISTINCT_DENSE=0 sends every key to the hash set.
std::optional<rowset::key_range> dense_range(device_column const& c, int64_t rows, hipStream_t s)
{
  if (env_i64("CUDF_AMD_DISTINCT_DENSE", 1) == 0) return std::nullopt;
  auto const ratio = static_cast<uint64_t>(std::clamp<int64_t>(env_i64("CUDF_AMD_DISTINCT_DENSE_RATIO", 2), 0, int64_t{1} << 32));
  auto const max_entries =
    static_cast<uint64_t>(std::max<int64_t>(env_i64("CUDF_AMD_DISTINCT_DENSE_MAX_ENTRIES", int64_t{1} << 28), 0));
  // the range of the first 65,536 rows is part of the whole range: when it already fails, the full pass over the keys is skipped
  constexpr int64_t prefix = 65536;
  if (rows > 4 * prefix && !rowset::small_key_range(c, prefix, rows, ratio, max_entries, s)) return std::nullopt;
  return rowset::small_key_range(c, rows, rows, ratio, max_entries, s);
}

// Builds the state of `keys` (at least one row and one column). flags: one zeroed byte per row, set for the rows that bypass the
// state (nullptr when counting).
void build(table_state& t, table_view const& keys, mode m, null_equality nulls, nan_equality nans, uint8_t* flags, stream_ref stream)
{
  hipStream_t const s = stream.value();
  auto tmp            = cudf::get_current_device_resource_ref();
  int64_t const n     = keys.num_rows();
  build_args& a       = t.a;
  a.keys              = make_device_table(keys);  // (throws beyond MAX_COLS or for a column that is not fixed-width)
  a.nrows             = n;
  a.mode              = static_cast<int32_t>(m);
  a.nulls_equal       = nulls == null_equality::EQUAL ? 1 : 0;
  a.nans_equal        = nans == nan_equality::ALL_EQUAL ? 1 : 0;
  a.flags             = flags;
  t.special           = rmm::device_buffer{2 * sizeof(uint32_t), s, tmp};
  t.counter           = rmm::device_buffer{2 * sizeof(unsigned long long), s, tmp};
  CUDF_HIP_TRY(hipMemsetAsync(t.special.data(), 0xff, t.special.size(), s));
  CUDF_HIP_TRY(hipMemsetAsync(t.counter.data(), 0, t.counter.size(), s));
  a.special = static_cast<uint32_t*>(t.special.data());
  a.counter = static_cast<unsigned long long*>(t.counter.data());

  device_column const& c = a.keys.col[0];
  if (auto const r = keys.num_columns() == 1 ? dense_range(c, n, s) : std::nullopt) {
    uint64_t const range = r->range;
    t.dense = true;
    a.lo    = r->lo;
    a.range = range;
    t.state = rmm::device_buffer{static_cast<std::size_t>(std::max<uint64_t>(range, 1)) * sizeof(uint32_t), s, tmp};
    CUDF_HIP_TRY(hipMemsetAsync(t.state.data(), 0xff, t.state.size(), s));
    a.state        = static_cast<uint32_t*>(t.state.data());
    a.state_stride = 1;
    // CUDF_AMD_DISTINCT_LDS_ENTRIES (16383, the most the kernel takes): the largest range reduced in LDS first; 0: never
    auto const lds = static_cast<uint64_t>(std::max<int64_t>(env_i64("CUDF_AMD_DISTINCT_LDS_ENTRIES", int64_t(lds_entries_max())), 0));
    t.lds_entries  = range <= std::min(lds, lds_entries_max()) ? std::min(lds, lds_entries_max()) : 0;
    launch_dense_build(a, t.lds_entries, s);
    return;
  }
  // the set: rowset::set_capacity at load CUDF_AMD_DISTINCT_LOAD_PERCENT (80) / 100. Distinct keys fill at most
  // that share of it, and only when every row is distinct; the slots are initialised and swept in full, so their bytes cost
  // every call ("Distinct rows"). CUDF_AMD_DISTINCT_INLINE=0 keeps {row hash | row} slots for every key.
  double const load = std::clamp(static_cast<double>(env_i64("CUDF_AMD_DISTINCT_LOAD_PERCENT", 80)), 10.0, 95.0) / 100;
  a.capacity        = rowset::set_capacity(n, load, "distinct: the hash set");
  a.inline_key      = rowset::inline_key_column(a.keys) && env_i64("CUDF_AMD_DISTINCT_INLINE", 1) != 0 ? 1 : 0;
  // inline keys under a keep rule: 16-byte records {key, state[2]}, all bits set (rowset::EMPTY, STATE_EMPTY); otherwise 8-byte slots
  a.slot_stride = a.inline_key && m != mode::count ? 2 : 1;
  t.slots = rmm::device_buffer{static_cast<std::size_t>(a.capacity * a.slot_stride) * sizeof(uint64_t), s, tmp};
  CUDF_HIP_TRY(hipMemsetAsync(t.slots.data(), 0xff, t.slots.size(), s));
  a.slots = static_cast<uint64_t*>(t.slots.data());
  if (a.slot_stride == 2) {
    a.state        = reinterpret_cast<uint32_t*>(a.slots) + 2;
    a.state_stride = 4;
  }
  launch_set_build(a, s);
}

mode mode_of(duplicate_keep_option keep)
{
  switch (keep) {
    case duplicate_keep_option::KEEP_ANY: return mode::any;
    case duplicate_keep_option::KEEP_FIRST: return mode::first;
    case duplicate_keep_option::KEEP_LAST: return mode::last;
    case duplicate_keep_option::KEEP_NONE: return mode::none;
  }
  CUDF_FAIL("Unsupported duplicate_keep_option", std::invalid_argument);
}

std::unique_ptr<column> empty_indices() { return make_empty_column(data_type{type_id::INT32}); }

// {distinct rows, a valid NaN key was seen}
std::pair<int64_t, bool> count_rows(table_view const& keys, null_equality nulls, nan_equality nans, stream_ref stream)
{
  table_state t;
  build(t, keys, mode::count, nulls, nans, nullptr, stream);
  unsigned long long h[2] = {0, 0};
  CUDF_HIP_TRY(hipMemcpyAsync(h, t.counter.data(), sizeof(h), hipMemcpyDeviceToHost, stream.value()));
  CUDF_HIP_TRY(hipStreamSynchronize(stream.value()));
  return {static_cast<int64_t>(h[0]), h[1] != 0};
}
}  // namespace

std::unique_ptr<column> indices(table_view const& input, duplicate_keep_option keep, null_equality nulls, nan_equality nans,
                                stream_ref stream, rmm::device_async_resource_ref mr)
{
  int64_t const n = input.num_rows();
  mode const m    = mode_of(keep);
  if (n == 0 || input.num_columns() == 0) return empty_indices();
  hipStream_t const s = stream.value();
  rmm::device_buffer flags{static_cast<std::size_t>(n), s, cudf::get_current_device_resource_ref()};
  CUDF_HIP_TRY(hipMemsetAsync(flags.data(), 0, flags.size(), s));
  table_state t;
  build(t, input, m, nulls, nans, static_cast<uint8_t*>(flags.data()), stream);
  launch_sweep(t.a, s);
  // the flag bytes -> mask words and chunk counts (every word written by the pack) -> ascending indices
  rowset::compaction c{n, s};
  launch_pack(static_cast<uint8_t const*>(flags.data()), c.mask(), n, c.g.chunk, c.g.nwaves, c.counts(), s);
  return std::make_unique<column>(c.compact_indices(s, mr), rmm::device_buffer{}, 0);
}

std::unique_ptr<table> distinct(table_view const& input, std::vector<size_type> const& keys, duplicate_keep_option keep,
                                null_equality nulls, nan_equality nans, stream_ref stream, rmm::device_async_resource_ref mr)
{
  // as the reference (distinct.cu:153-157): the trivial cases first, then select (std::out_of_range for a key outside input)
  if (input.num_rows() == 0 || input.num_columns() == 0 || keys.empty()) return empty_like(input);
  auto const idx = indices(input.select(keys), keep, nulls, nans, stream, cudf::get_current_device_resource_ref());
  return cudf::gather(input, idx->view(), out_of_bounds_policy::DONT_CHECK, stream, mr);
}

}  // namespace distinct
}  // namespace detail

std::unique_ptr<column> distinct_indices(table_view const& input, duplicate_keep_option keep, null_equality nulls_equal,
                                         nan_equality nans_equal, stream_ref stream, rmm::device_async_resource_ref mr)
{
  CUDF_FUNC_RANGE();
  return detail::distinct::indices(input, keep, nulls_equal, nans_equal, stream, mr);
}

// The indices come out ascending, so the order of `distinct` is the input order too: both are the same gather.
std::unique_ptr<table> distinct(table_view const& input, std::vector<size_type> const& keys, duplicate_keep_option keep,
                                null_equality nulls_equal, nan_equality nans_equal, stream_ref stream, rmm::device_async_resource_ref mr)
{
  CUDF_FUNC_RANGE();
  return detail::distinct::distinct(input, keys, keep, nulls_equal, nans_equal, stream, mr);
}

std::unique_ptr<table> stable_distinct(table_view const& input, std::vector<size_type> const& keys, duplicate_keep_option keep,
                                       null_equality nulls_equal, nan_equality nans_equal, stream_ref stream,
                                       rmm::device_async_resource_ref mr)
{
  CUDF_FUNC_RANGE();
  return detail::distinct::distinct(input, keys, keep, nulls_equal, nans_equal, stream, mr);
}

size_type distinct_count(table_view const& input, null_equality nulls_equal, stream_ref stream)
{
  CUDF_FUNC_RANGE();
  if (input.num_rows() == 0 || input.num_columns() == 0) return 0;
  return static_cast<size_type>(detail::distinct::count_rows(input, nulls_equal, nan_equality::ALL_EQUAL, stream).first);
}

// reference cpp/src/reductions/distinct_count.cu:190-219, line for line
size_type distinct_count(column_view const& input, null_policy null_handling, nan_policy nan_handling, stream_ref stream)
{
  CUDF_FUNC_RANGE();
  if (input.size() == 0) return 0;
  if (input.null_count() == input.size()) return null_handling == null_policy::INCLUDE ? 1 : 0;
  auto const [n, has_nan] = detail::distinct::count_rows(table_view{{input}}, null_equality::EQUAL, nan_equality::ALL_EQUAL, stream);
  auto count              = static_cast<size_type>(n);
  bool const has_null     = input.null_count() > 0;
  if (null_handling == null_policy::EXCLUDE && has_null) --count;
  if (nan_handling == nan_policy::NAN_IS_NULL && has_nan && (has_null || null_handling == null_policy::EXCLUDE)) --count;
  return count;
}

}  // namespace cudf
