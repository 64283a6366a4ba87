// SPDX-License-Identifier: Apache-2.0
// cudf::merge: sorted tables combined into one sorted table, without sorting them again.
// The signature follows reference cpp/include/cudf/merge.hpp; the stream and memory-resource types are this library's, as in
// sorting.hpp. Columns that are not fixed-width (strings, lists, structs, dictionaries) are not served.
//
// Contract:
//  - Every table of tables_to_merge has the same column types and is sorted on its columns key_cols, in that order of
//    significance, under column_order / null_precedence (one entry per KEY column; rows compare as in sorting.hpp).
//  - The result holds every row of every input, whole (all columns, null masks included), sorted on the key columns. A column of
//    the result is nullable if that column is nullable in any input that has rows.
//  - Rows of ONE input table whose keys compare equal keep their relative order. The order of equal-key rows that come from
//    DIFFERENT tables is unspecified (the two tables with the fewest rows are merged first, again and again, as the reference does).
//  - No tables: an empty table with zero columns. Then, before any shortcut, cudf::logic_error for: mismatched column counts or
//    column types; empty key_cols; more key columns than columns; column_order.size() != key_cols.size() (an empty column_order
//    does NOT mean ascending here); a non-empty null_precedence of another size (empty means null_order::BEFORE); a total row count
//    beyond INT32_MAX; a key index outside [0, num_columns) or one that repeats; columns beyond the device tables' limits (more
//    than 16 key columns, a column that is not fixed-width of at most 8 bytes).
//  - One non-empty table: a copy of it. No non-empty table: empty_like of the first.
//  - Intermediate tables come from the current device resource; only the last merge allocates from `mr`.
//  - Inputs that are not sorted give a table of the right shape whose rows are unspecified (each is some row of some input); every
//    read and write stays in bounds.
// Merge by two searches and the two-source gather: DESIGN.md section 4, "Search and merge".
#pragma once
#include <cudf/table/table.hpp>
#include <cudf/table/table_view.hpp>
#include <cudf/types.hpp>
#include <cudf/utilities/default_stream.hpp>

#include <memory>
#include <vector>

namespace cudf {

std::unique_ptr<table> merge(std::vector<table_view> const& tables_to_merge, std::vector<size_type> const& key_cols,
                             std::vector<order> const& column_order, std::vector<null_order> const& null_precedence = {},
                             stream_ref stream = get_default_stream(), rmm::device_async_resource_ref mr = get_current_device_resource_ref());

}  // namespace cudf
