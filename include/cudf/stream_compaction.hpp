// SPDX-License-Identifier: Apache-2.0
// cudf::distinct, cudf::distinct_indices and cudf::stable_distinct: the distinct rows of a table by its key columns. Signatures
// follow reference cpp/include/cudf/stream_compaction.hpp (duplicate_keep_option, distinct, distinct_indices, stable_distinct); the
// stream and memory-resource types are this library's, as in hash_join.hpp.
//
// Contract:
//  - Key rows are compared column by column; -0 equals +0. nan_equality::ALL_EQUAL: NaN equals NaN; UNEQUAL: a row with a NaN in
//    any key column equals no row. null_equality::EQUAL: a null equals a null in the same column; UNEQUAL: a row with a null in any
//    key column equals no row. A row that equals no other row survives every keep option, KEEP_NONE included.
//  - KEEP_FIRST / KEEP_LAST keep the smallest / largest row index of each set of equal rows; KEEP_ANY exactly one row of each set;
//    KEEP_NONE only the rows that have no equal row.
//  - distinct_indices: the surviving row indices of `input` (every column a key) as an INT32 column without nulls, exactly sized,
//    in ascending order.
//  - distinct / stable_distinct: every column of `input`, payload included, gathered with one index vector (rows stay whole) from
//    distinct_indices(input.select(keys), ...). Row order: unspecified for distinct, input order for stable_distinct.
//  - Zero rows, zero columns or an empty `keys` give an empty table of input's schema (an empty INT32 column for distinct_indices).
//  - A key index outside `input` throws std::out_of_range (table_view::select). Key tables beyond the device tables' limits (more
//    than 16 columns, a column that is not fixed-width) throw cudf::logic_error, as the joins do.
// The model and forms: DESIGN.md section 4, "Distinct rows".
//
// cudf::apply_boolean_mask, apply_deletion_mask, drop_nulls, drop_nans and unique: the rows of a table that pass a predicate.
// Signatures follow the same reference header; the contract restates reference cpp/src/stream_compaction/{apply_boolean_mask,
// drop_nulls,drop_nans,unique}.cu, the code where its doc comments differ.
//
// Contract, all five:
//  - Stable: the surviving rows keep their input order. Rows stay whole: every column of `input`, payload included, is compacted
//    with the one selection. The output's schema is the input's.
//  - An output column of at least one row has a null mask exactly when its input column has one; its null_count is exact and the
//    mask bits beyond the output size are zero. (A column of zero rows holds no mask in this library.)
//  - Sliced inputs are served: columns, key columns and the boolean mask at any offset.
//  - Every column of `input` is fixed-width of at most 8 bytes (the limits of cudf::gather), any number of them; otherwise
//    cudf::logic_error. Key tables (drop_nulls, drop_nans, unique) beyond the device tables' limits (more than 16 key columns, a key
//    that is not fixed-width of at most 8 bytes) throw cudf::logic_error, as distinct does; a key index outside `input` throws
//    std::out_of_range.
//  - apply_boolean_mask: row i survives iff mask element i is valid and non-zero. In the reference's order: an empty mask gives an
//    empty table of input's schema, whatever input's size (its EmptyMask test: six rows, no mask element); then a mask that is not
//    BOOL8 throws cudf::logic_error; then boolean_mask.size() != input.num_rows() throws cudf::logic_error unless input has no rows.
//    This library's table_view carries no row count without columns, so a table of zero columns has zero rows and gives an empty
//    table (the reference's ZeroColumnsPreservesRowCount cannot be stated here).
//  - apply_deletion_mask: row i survives iff mask element i is valid and zero: a null mask element deletes the row, as a true one
//    does (reference deletion_mask_filter; its tests NullDeletionMask and AllDeletedMixedNullAndTrue). Checks as above.
//  - drop_nulls: row i survives iff at least keep_threshold of its key fields are valid; a key column without a mask counts as
//    valid in every row. The form without a threshold uses keys.size(). When `keys` is empty, when there are no rows, or when no
//    key column has a null (null_count() == 0 in all of them), the result is a copy of `input`, whatever the threshold
//    (drop_nulls.cu:70-72).
//  - drop_nans: row i survives iff at least keep_threshold of its key fields are not NaN; a null field counts as not NaN. Empty
//    `keys` or no rows give a copy of `input`; otherwise a key column that is not FLOAT32 or FLOAT64 throws cudf::logic_error.
//  - unique: for input whose equal key rows are adjacent (sorted input). KEEP_ANY means KEEP_FIRST. Zero rows, zero columns or
//    empty `keys` give an empty table of input's schema (before the keys are looked at). Row i equals its neighbour as distinct
//    compares rows with NaN equal to NaN: -0 equals +0, nulls by nulls_equal. KEEP_FIRST keeps i iff i == 0 or row i differs from
//    row i - 1; KEEP_LAST iff i == n - 1 or row i differs from row i + 1; KEEP_NONE iff both.
// The model and kernels: DESIGN.md section 4, "Filtering rows".
#pragma once
#include <cudf/column/column.hpp>
#include <cudf/table/table.hpp>
#include <cudf/table/table_view.hpp>
#include <cudf/types.hpp>
#include <cudf/utilities/default_stream.hpp>

#include <memory>
#include <vector>

namespace cudf {

enum class duplicate_keep_option {
  KEEP_ANY = 0,  ///< Keep an unspecified occurrence
  KEEP_FIRST,    ///< Keep first occurrence
  KEEP_LAST,     ///< Keep last occurrence
  KEEP_NONE      ///< Keep no (remove all) occurrences of duplicates
};

std::unique_ptr<table> distinct(table_view const& input, std::vector<size_type> const& keys,
                                duplicate_keep_option keep        = duplicate_keep_option::KEEP_ANY,
                                null_equality nulls_equal         = null_equality::EQUAL,
                                nan_equality nans_equal           = nan_equality::ALL_EQUAL,
                                stream_ref stream                 = get_default_stream(),
                                rmm::device_async_resource_ref mr = get_current_device_resource_ref());

std::unique_ptr<column> distinct_indices(table_view const& input, duplicate_keep_option keep = duplicate_keep_option::KEEP_ANY,
                                         null_equality nulls_equal         = null_equality::EQUAL,
                                         nan_equality nans_equal           = nan_equality::ALL_EQUAL,
                                         stream_ref stream                 = get_default_stream(),
                                         rmm::device_async_resource_ref mr = get_current_device_resource_ref());

std::unique_ptr<table> stable_distinct(table_view const& input, std::vector<size_type> const& keys,
                                       duplicate_keep_option keep        = duplicate_keep_option::KEEP_ANY,
                                       null_equality nulls_equal         = null_equality::EQUAL,
                                       nan_equality nans_equal           = nan_equality::ALL_EQUAL,
                                       stream_ref stream                 = get_default_stream(),
                                       rmm::device_async_resource_ref mr = get_current_device_resource_ref());

std::unique_ptr<table> drop_nulls(table_view const& input, std::vector<size_type> const& keys, size_type keep_threshold,
                                  stream_ref stream                 = get_default_stream(),
                                  rmm::device_async_resource_ref mr = get_current_device_resource_ref());

std::unique_ptr<table> drop_nulls(table_view const& input, std::vector<size_type> const& keys,
                                  stream_ref stream                 = get_default_stream(),
                                  rmm::device_async_resource_ref mr = get_current_device_resource_ref());

std::unique_ptr<table> drop_nans(table_view const& input, std::vector<size_type> const& keys, size_type keep_threshold,
                                 stream_ref stream                 = get_default_stream(),
                                 rmm::device_async_resource_ref mr = get_current_device_resource_ref());

std::unique_ptr<table> drop_nans(table_view const& input, std::vector<size_type> const& keys,
                                 stream_ref stream                 = get_default_stream(),
                                 rmm::device_async_resource_ref mr = get_current_device_resource_ref());

std::unique_ptr<table> apply_boolean_mask(table_view const& input, column_view const& boolean_mask,
                                          stream_ref stream                 = get_default_stream(),
                                          rmm::device_async_resource_ref mr = get_current_device_resource_ref());

std::unique_ptr<table> apply_deletion_mask(table_view const& input, column_view const& deletion_mask,
                                           stream_ref stream                 = get_default_stream(),
                                           rmm::device_async_resource_ref mr = get_current_device_resource_ref());

std::unique_ptr<table> unique(table_view const& input, std::vector<size_type> const& keys, duplicate_keep_option keep,
                              null_equality nulls_equal         = null_equality::EQUAL,
                              stream_ref stream                 = get_default_stream(),
                              rmm::device_async_resource_ref mr = get_current_device_resource_ref());

}  // namespace cudf
