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

}  // namespace cudf
