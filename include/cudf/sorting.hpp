// SPDX-License-Identifier: Apache-2.0
// cudf::sorted_order, sort, sort_by_key, their stable_ forms and is_sorted: the lexicographic order of the rows of a table; and
// cudf::rank: the rank of every element of a column. Signatures follow reference cpp/include/cudf/sorting.hpp (sorted_order,
// stable_sorted_order, is_sorted, sort, stable_sort, sort_by_key, stable_sort_by_key, rank); the stream and memory-resource types
// are this library's, as in stream_compaction.hpp. top_k and the segmented sorts are not served.
//
// Contract:
//  - Rows compare column by column, the first column most significant. Within a column -0 equals +0, every NaN is one value
//    above +inf, BOOL8 compares as 0 or 1 (reference detail/row_operator/lexicographic.cuh).
//  - An empty column_order means ASCENDING for every column, an empty null_precedence null_order::BEFORE for every column.
//  - null_order::BEFORE: a null is smaller than every value; AFTER: larger. DESCENDING flips the whole comparison of its column,
//    nulls included: a column's nulls come first in the output exactly when (null_precedence == BEFORE) != (order == DESCENDING).
//    Nulls of one column are equal to each other.
//  - sorted_order / stable_sorted_order: an INT32 column without nulls of input.num_rows() elements, the permutation of the row
//    indices that puts the rows in order. Rows that compare equal keep their input order in stable_sorted_order; sorted_order does
//    not promise it (here both run the same stable radix sort).
//  - sort / stable_sort: every column of `input` gathered with sorted_order(input, ...). sort_by_key / stable_sort_by_key: every
//    column of `values` gathered with the order of `keys`; rows stay whole.
//  - Zero rows give an empty column (an empty table of the input's schema); zero key columns give the identity order.
//  - is_sorted: true for zero columns, zero rows or one row; otherwise true iff no row is lexicographically less than its
//    predecessor (equal adjacent rows are sorted).
//  - cudf::logic_error: a non-empty column_order or null_precedence whose size differs from the number of key columns;
//    values.num_rows() != keys.num_rows(); key tables beyond the device tables' limits (more than 16 columns, a column that is not
//    fixed-width), as the joins and distinct throw.
//
// rank (reference sorting.hpp:165-230, cpp/src/sort/rank.cu:253-353):
//  - Ranks start at 1 and follow the stable sorted order of the column under (column_order, null_precedence). Rows tie when they
//    compare equal above: NaNs tie, -0 ties with +0, and all nulls tie with each other.
//  - FIRST: the position in the stable order + 1. MIN / MAX: the first / last position of the row's run of tied rows + 1.
//    AVERAGE: MIN + (run length - 1) / 2.0. DENSE: the number of runs up to and including the row's.
//    input {3, 4, 5, 4, 1, 2}: FIRST {3, 4, 6, 5, 1, 2}, AVERAGE {3, 4.5, 6, 4.5, 1, 2}, MIN {3, 4, 6, 4, 1, 2},
//    MAX {3, 5, 6, 5, 1, 2}, DENSE {3, 4, 5, 4, 1, 2}.
//  - The result is FLOAT64 when method == AVERAGE or `percentage` is set, else INT32; an empty input gives an empty column of it.
//  - null_policy::INCLUDE: nulls are ranked like any value, and the result has no mask. null_policy::EXCLUDE: the result carries
//    a copy of the input's validity (from bit 0, whatever the input's offset) and its null count, and the values under a null are
//    unspecified; an input without a mask gives a result without one.
//  - percentage: every rank is divided, in double, by count = size (INCLUDE) or size - null_count (EXCLUDE); for DENSE by the
//    dense rank of sorted position count - 1 instead.
//  - EXCLUDE is meant for nulls sorted last (ASCENDING with AFTER, DESCENDING with BEFORE). EXCLUDE with nulls sorted first on a
//    column that has nulls is undefined in the reference (sorting.hpp:204-206). Here the same formulas run unchanged, so the nulls
//    take the first ranks and a percentage still divides by the count of valid rows; nothing throws, and the values are not part
//    of the contract.
//  - cudf::logic_error: a column that is not fixed-width of at most 8 bytes, as sorted_order throws.
// The radix words and the pass arithmetic: DESIGN.md section 4, "Sorting"; the rank pass: "Ranking".
#pragma once
#include <cudf/aggregation.hpp>
#include <cudf/column/column.hpp>
#include <cudf/table/table.hpp>
#include <cudf/table/table_view.hpp>
#include <cudf/types.hpp>
#include <cudf/utilities/default_stream.hpp>

#include <memory>
#include <vector>

namespace cudf {

std::unique_ptr<column> sorted_order(table_view const& input, std::vector<order> const& column_order = {},
                                     std::vector<null_order> const& null_precedence = {},
                                     stream_ref stream                              = get_default_stream(),
                                     rmm::device_async_resource_ref mr              = get_current_device_resource_ref());

std::unique_ptr<column> stable_sorted_order(table_view const& input, std::vector<order> const& column_order = {},
                                            std::vector<null_order> const& null_precedence = {},
                                            stream_ref stream                              = get_default_stream(),
                                            rmm::device_async_resource_ref mr              = get_current_device_resource_ref());

bool is_sorted(table_view const& table, std::vector<order> const& column_order, std::vector<null_order> const& null_precedence,
               stream_ref stream = get_default_stream());

std::unique_ptr<table> sort(table_view const& input, std::vector<order> const& column_order = {},
                            std::vector<null_order> const& null_precedence = {}, stream_ref stream = get_default_stream(),
                            rmm::device_async_resource_ref mr = get_current_device_resource_ref());

std::unique_ptr<table> stable_sort(table_view const& input, std::vector<order> const& column_order = {},
                                   std::vector<null_order> const& null_precedence = {}, stream_ref stream = get_default_stream(),
                                   rmm::device_async_resource_ref mr = get_current_device_resource_ref());

std::unique_ptr<table> sort_by_key(table_view const& values, table_view const& keys, std::vector<order> const& column_order = {},
                                   std::vector<null_order> const& null_precedence = {}, stream_ref stream = get_default_stream(),
                                   rmm::device_async_resource_ref mr = get_current_device_resource_ref());

std::unique_ptr<table> stable_sort_by_key(table_view const& values, table_view const& keys,
                                          std::vector<order> const& column_order         = {},
                                          std::vector<null_order> const& null_precedence = {},
                                          stream_ref stream                              = get_default_stream(),
                                          rmm::device_async_resource_ref mr              = get_current_device_resource_ref());

std::unique_ptr<column> rank(column_view const& input, rank_method method, order column_order, null_policy null_handling,
                             null_order null_precedence, bool percentage, stream_ref stream = get_default_stream(),
                             rmm::device_async_resource_ref mr = get_current_device_resource_ref());

}  // namespace cudf
