// SPDX-License-Identifier: Apache-2.0
// cudf::sorted_order, sort, sort_by_key, their stable_ forms and is_sorted: the lexicographic order of the rows of a table.
// Signatures follow reference cpp/include/cudf/sorting.hpp (sorted_order, stable_sorted_order, is_sorted, sort, stable_sort,
// sort_by_key, stable_sort_by_key); the stream and memory-resource types are this library's, as in stream_compaction.hpp.
// rank, top_k and the segmented sorts are not served.
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
// The radix words and the pass arithmetic: DESIGN.md section 4, "Sorting".
#pragma once
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

}  // namespace cudf
