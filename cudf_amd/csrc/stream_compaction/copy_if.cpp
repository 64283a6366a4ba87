// SPDX-License-Identifier: Apache-2.0
// Host side of cudf::apply_boolean_mask, apply_deletion_mask, drop_nulls, drop_nans, unique (include/cudf/stream_compaction.hpp)
// and cudf::unique_count (include/cudf/reduction/unique_count.hpp): the trivial cases, the choice of the selection kernel and the
// sequence selection -> sizing read-back -> allocation -> copy_if_data -> copy_if_validity -> null-count read-back. Reference
// counterparts: cpp/src/stream_compaction/{apply_boolean_mask,drop_nulls,drop_nans,unique}.cu and
// cpp/src/reductions/unique_count{,_column}.cu. Kernels: copy_if_impl.hpp, copy_if_kernels.hip; the model: DESIGN.md section 4,
// "Filtering rows".
#include "copy_if_impl.hpp"
#include "../common/profiler.hpp"
#include "../common/row_set_host.hpp"

#include <cudf/null_mask.hpp>
#include <cudf/reduction/unique_count.hpp>
#include <cudf/stream_compaction.hpp>

#include <algorithm>

namespace cudf {
namespace detail {
namespace copy_if {
namespace {

// the limits of cudf::gather: every column of the table moves as 1-, 2-, 4- or 8-byte elements
void expect_movable(table_view const& input)
{
  for (auto const& c : input)
    CUDF_EXPECTS(is_fixed_width(c.type()) && c.num_children() == 0 && size_of(c.type()) <= 8,
                 "stream compaction: only fixed-width columns of at most 8 bytes.");
}

template <typename Args>
Args select_args(rowset::compaction& c)
{
  Args a{};
  a.nrows  = c.nrows;
  a.chunk  = c.g.chunk;
  a.nwaves = c.g.nwaves;
  a.mask   = c.mask();
  a.counts = c.counts();
  return a;
}

// Pass 2: the rows of `input` whose bit of c's mask is set, in row order. The one sizing read-back (c.total), then every launch on
// `stream`; the null counts of all nullable columns come back in one copy.
std::unique_ptr<table> compact(table_view const& input, rowset::compaction& c, stream_ref stream, rmm::device_async_resource_ref mr)
{
  hipStream_t const s  = stream.value();
  auto tmp             = cudf::get_current_device_resource_ref();
  uint64_t const total = c.total(s);
  if (total == 0) return empty_like(input);
  auto const n_out = static_cast<size_type>(total);

  std::vector<std::unique_ptr<column>> out;
  std::vector<size_type> nullable;
  for (size_type i = 0; i < input.num_columns(); ++i) {
    auto const& col = input.column(i);
    // (ALL_NULL: the whole allocation zero-filled on `stream`; copy_if_validity only ORs bits in)
    out.push_back(std::make_unique<column>(col.type(), n_out, rmm::device_buffer{static_cast<std::size_t>(total) * size_of(col.type()), s, mr},
                                           create_null_mask(n_out, col.nullable() ? mask_state::ALL_NULL : mask_state::UNALLOCATED, stream, mr),
                                           0));
    if (col.nullable()) nullable.push_back(i);
  }

  compact_base b{};
  b.mask     = c.mask();
  b.counts   = c.counts();
  b.chunk    = c.g.chunk;
  b.nrows    = c.nrows;
  b.out_rows = total;
  b.nwaves   = c.g.nwaves;

  rmm::device_buffer d_data{sizeof(data_args), s, tmp};
  for (size_type first = 0; first < input.num_columns(); first += DATA_COLS) {
    data_args a{};
    static_cast<compact_base&>(a) = b;
    a.ncols                       = std::min<int32_t>(DATA_COLS, input.num_columns() - first);
    for (int k = 0; k < a.ncols; ++k) {
      auto const& col = input.column(first + k);
      auto const w    = static_cast<int64_t>(size_of(col.type()));
      a.col[k]        = {static_cast<char const*>(col.head()) + static_cast<int64_t>(col.offset()) * w,
                         out[static_cast<std::size_t>(first + k)]->mutable_view().head(), w};
    }
    launch_copy_if_data(a, static_cast<data_args*>(d_data.data()), s);
  }

  if (!nullable.empty()) {
    rmm::device_buffer valid{nullable.size() * sizeof(unsigned long long), s, tmp};
    CUDF_HIP_TRY(hipMemsetAsync(valid.data(), 0, valid.size(), s));
    auto* const d_valid = static_cast<unsigned long long*>(valid.data());
    rmm::device_buffer d_validity{sizeof(validity_args), s, tmp};
    for (std::size_t first = 0; first < nullable.size(); first += VALIDITY_COLS) {
      validity_args a{};
      static_cast<compact_base&>(a) = b;
      a.ncols                       = static_cast<int32_t>(std::min<std::size_t>(VALIDITY_COLS, nullable.size() - first));
      for (int k = 0; k < a.ncols; ++k) {
        auto const i    = nullable[first + static_cast<std::size_t>(k)];
        auto const& col = input.column(i);
        a.col[k]        = {col.null_mask(), col.offset(), out[static_cast<std::size_t>(i)]->mutable_view().null_mask(), d_valid + first + k};
      }
      launch_copy_if_validity(a, static_cast<validity_args*>(d_validity.data()), s);
    }
    std::vector<unsigned long long> h(nullable.size());
    CUDF_HIP_TRY(hipMemcpyAsync(h.data(), d_valid, valid.size(), hipMemcpyDeviceToHost, s));
    CUDF_HIP_TRY(hipStreamSynchronize(s));
    for (std::size_t k = 0; k < nullable.size(); ++k)
      out[static_cast<std::size_t>(nullable[k])]->set_null_count(static_cast<size_type>(total - h[k]));
  }
  return std::make_unique<table>(std::move(out));
}

// reference apply_boolean_mask.cu detail::apply_mask, in its order: an empty mask first, then the type, then the size
std::unique_ptr<table> apply_mask(table_view const& input, column_view const& m, bool deletion, stream_ref stream,
                                  rmm::device_async_resource_ref mr)
{
  if (m.is_empty()) return empty_like(input);
  CUDF_EXPECTS(m.type().id() == type_id::BOOL8, "Mask must be Boolean type");
  CUDF_EXPECTS(input.num_rows() == 0 || input.num_rows() == m.size(), "Column size mismatch");
  if (input.num_rows() == 0 || input.num_columns() == 0) return empty_like(input);
  expect_movable(input);
  rowset::compaction c{input.num_rows(), stream.value()};
  auto a = select_args<bool_args>(c);
  a.m    = make_device_column(m);
  launch_select_bool(a, deletion, stream.value());
  return compact(input, c, stream, mr);
}

std::unique_ptr<table> drop_nulls(table_view const& input, std::vector<size_type> const& keys, size_type keep_threshold,
                                  stream_ref stream, rmm::device_async_resource_ref mr)
{
  auto const keys_view = input.select(keys);  // (std::out_of_range for a key outside input)
  // reference drop_nulls.cu:70-72: a copy, whatever the threshold
  if (keys_view.num_columns() == 0 || keys_view.num_rows() == 0 || !cudf::has_nulls(keys_view))
    return std::make_unique<table>(input, stream, mr);
  (void)make_device_table(keys_view);  // (the key limits: more than 16 columns, a column that is not fixed-width)
  expect_movable(input);
  int64_t const n = input.num_rows();
  // mask-less keys are valid in every row: they count towards the threshold here, and the kernels see the nullable keys alone
  rowset::compaction c{n, stream.value()};
  auto a = select_args<valid_args>(c);
  for (auto const& k : keys_view)
    if (k.nullable()) a.key[a.nkeys++] = {k.null_mask(), k.offset()};
  int64_t const need = static_cast<int64_t>(keep_threshold) - (keys_view.num_columns() - a.nkeys);
  if (need <= 0) return std::make_unique<table>(input, stream, mr);  // every row meets it
  if (need > a.nkeys) return empty_like(input);                      // no row can
  a.need = static_cast<int32_t>(need);
  if (a.need == a.nkeys) launch_select_valid_words(a, stream.value());
  else launch_select_valid_count(a, stream.value());
  return compact(input, c, stream, mr);
}

std::unique_ptr<table> drop_nans(table_view const& input, std::vector<size_type> const& keys, size_type keep_threshold,
                                 stream_ref stream, rmm::device_async_resource_ref mr)
{
  auto const keys_view = input.select(keys);
  if (keys_view.num_columns() == 0 || keys_view.num_rows() == 0) return std::make_unique<table>(input, stream, mr);
  for (auto const& k : keys_view)
    CUDF_EXPECTS(k.type().id() == type_id::FLOAT32 || k.type().id() == type_id::FLOAT64, "Key column is not of type floating-point");
  expect_movable(input);
  rowset::compaction c{input.num_rows(), stream.value()};
  auto a = select_args<nan_args>(c);
  a.keys = make_device_table(keys_view);
  a.need = keep_threshold;
  launch_select_nan(a, stream.value());
  return compact(input, c, stream, mr);
}

std::unique_ptr<table> unique(table_view const& input, std::vector<size_type> const& keys, duplicate_keep_option keep_option,
                              null_equality nulls_equal, stream_ref stream, rmm::device_async_resource_ref mr)
{
  // reference unique.cu:47-51: KEEP_ANY is KEEP_FIRST; the trivial cases before the keys are selected
  if (input.num_rows() == 0 || input.num_columns() == 0 || keys.empty()) return empty_like(input);
  keep k = keep::first;
  switch (keep_option) {
    case duplicate_keep_option::KEEP_ANY:
    case duplicate_keep_option::KEEP_FIRST: k = keep::first; break;
    case duplicate_keep_option::KEEP_LAST: k = keep::last; break;
    case duplicate_keep_option::KEEP_NONE: k = keep::none; break;
    default: CUDF_FAIL("Unsupported duplicate_keep_option", std::invalid_argument);
  }
  auto const keys_view = input.select(keys);
  rowset::compaction c{input.num_rows(), stream.value()};
  auto a        = select_args<unique_args>(c);
  a.keys        = make_device_table(keys_view);
  a.nulls_equal = nulls_equal == null_equality::EQUAL ? 1 : 0;
  expect_movable(input);
  launch_select_unique(a, k, stream.value());
  return compact(input, c, stream, mr);
}

}  // namespace
}  // namespace copy_if
}  // namespace detail

std::unique_ptr<table> apply_boolean_mask(table_view const& input, column_view const& boolean_mask, stream_ref stream,
                                          rmm::device_async_resource_ref mr)
{
  CUDF_FUNC_RANGE();
  return detail::copy_if::apply_mask(input, boolean_mask, false, stream, mr);
}

std::unique_ptr<table> apply_deletion_mask(table_view const& input, column_view const& deletion_mask, stream_ref stream,
                                           rmm::device_async_resource_ref mr)
{
  CUDF_FUNC_RANGE();
  return detail::copy_if::apply_mask(input, deletion_mask, true, stream, mr);
}

std::unique_ptr<table> drop_nulls(table_view const& input, std::vector<size_type> const& keys, size_type keep_threshold,
                                  stream_ref stream, rmm::device_async_resource_ref mr)
{
  CUDF_FUNC_RANGE();
  return detail::copy_if::drop_nulls(input, keys, keep_threshold, stream, mr);
}

std::unique_ptr<table> drop_nulls(table_view const& input, std::vector<size_type> const& keys, stream_ref stream,
                                  rmm::device_async_resource_ref mr)
{
  CUDF_FUNC_RANGE();
  return detail::copy_if::drop_nulls(input, keys, static_cast<size_type>(keys.size()), stream, mr);
}

std::unique_ptr<table> drop_nans(table_view const& input, std::vector<size_type> const& keys, size_type keep_threshold,
                                 stream_ref stream, rmm::device_async_resource_ref mr)
{
  CUDF_FUNC_RANGE();
  return detail::copy_if::drop_nans(input, keys, keep_threshold, stream, mr);
}

std::unique_ptr<table> drop_nans(table_view const& input, std::vector<size_type> const& keys, stream_ref stream,
                                 rmm::device_async_resource_ref mr)
{
  CUDF_FUNC_RANGE();
  return detail::copy_if::drop_nans(input, keys, static_cast<size_type>(keys.size()), stream, mr);
}

std::unique_ptr<table> unique(table_view const& input, std::vector<size_type> const& keys, duplicate_keep_option keep,
                              null_equality nulls_equal, stream_ref stream, rmm::device_async_resource_ref mr)
{
  CUDF_FUNC_RANGE();
  return detail::copy_if::unique(input, keys, keep, nulls_equal, stream, mr);
}

// Pass 1 alone: the selection's set bits are the count. No output is allocated and no compaction runs.
size_type unique_count(table_view const& input, null_equality nulls_equal, stream_ref stream)
{
  CUDF_FUNC_RANGE();
  using namespace detail::copy_if;
  if (input.num_rows() == 0 || input.num_columns() == 0) return 0;
  detail::rowset::compaction c{input.num_rows(), stream.value()};
  auto a        = select_args<unique_args>(c);
  a.keys        = detail::make_device_table(input);
  a.nulls_equal = nulls_equal == null_equality::EQUAL ? 1 : 0;
  launch_select_unique(a, keep::first, stream.value());
  return static_cast<size_type>(c.total(stream.value()));
}

size_type unique_count(column_view const& input, null_policy null_handling, nan_policy nan_handling, stream_ref stream)
{
  CUDF_FUNC_RANGE();
  using namespace detail::copy_if;
  if (input.size() == 0 || input.null_count() == input.size()) return 0;  // reference unique_count_column.cu:56
  detail::rowset::compaction c{input.size(), stream.value()};
  auto a           = select_args<unique_column_args>(c);
  a.keys           = detail::make_device_table(table_view{{input}});
  a.count_nulls    = null_handling == null_policy::INCLUDE ? 1 : 0;
  bool const is_fp = input.type().id() == type_id::FLOAT32 || input.type().id() == type_id::FLOAT64;
  a.nan_is_null    = nan_handling == nan_policy::NAN_IS_NULL && is_fp ? 1 : 0;
  launch_select_unique_column(a, stream.value());
  return static_cast<size_type>(c.total(stream.value()));
}

}  // namespace cudf
