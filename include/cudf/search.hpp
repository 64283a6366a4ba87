// SPDX-License-Identifier: Apache-2.0
// cudf::lower_bound and upper_bound: where the rows of one table fall in a sorted table.
// Signatures follow reference cpp/include/cudf/search.hpp (lower_bound, upper_bound); the stream and memory-resource types are this
// library's, as in sorting.hpp. contains is not served: its form that takes a cudf::scalar needs a type this library does not have.
//
// Contract:
//  - The result is an INT32 column without nulls of needles.num_rows() elements. lower_bound: element i is the number of haystack
//    rows that compare less than needle row i, the first position at which the needle can be inserted with the haystack still
//    sorted. upper_bound: the number of haystack rows that compare less than or equal to it, the last such position.
//  - Rows compare as in sorting.hpp (column by column, the first most significant; -0 equals +0, one NaN above +inf, BOOL8 as 0 or 1;
//    DESCENDING flips a column's whole comparison, nulls included), across the two tables: a null needle ties with a null haystack
//    element of the same column.
//  - An empty column_order means ASCENDING for every column, an empty null_precedence null_order::BEFORE for every column.
//  - `haystack` is assumed sorted under these orders. One that is not gives unspecified values in [0, haystack.num_rows()].
//  - Zero haystack rows give all zeros; zero needle rows give an empty INT32 column.
//  - cudf::logic_error: a non-empty column_order or null_precedence whose size differs from haystack.num_columns() (checked first,
//    for empty tables too); key tables beyond the device tables' limits (more than 16 columns, a column that is not fixed-width),
//    as sorted_order throws. std::invalid_argument: haystack and needles with different column counts or column types.
//
// Examples:
//   haystack {10, 20, 20, 30, 50}, needle {20}: lower_bound {1}, upper_bound {3}.
//   haystack {{10, 20, 20, 20, 20}, {5.0, 0.5, 0.5, 0.7, 0.7}, {90, 77, 78, 61, 61}}, needle {{20}, {0.7}, {61}}:
//   lower_bound {3}, upper_bound {5}.
// The search kernel and the joint plan of the two tables: DESIGN.md section 4, "Search and merge".
#pragma once
#include <cudf/column/column.hpp>
#include <cudf/table/table_view.hpp>
#include <cudf/types.hpp>
#include <cudf/utilities/default_stream.hpp>

#include <memory>
#include <vector>

namespace cudf {

std::unique_ptr<column> lower_bound(table_view const& haystack, table_view const& needles, std::vector<order> const& column_order,
                                    std::vector<null_order> const& null_precedence, stream_ref stream = get_default_stream(),
                                    rmm::device_async_resource_ref mr = get_current_device_resource_ref());

std::unique_ptr<column> upper_bound(table_view const& haystack, table_view const& needles, std::vector<order> const& column_order,
                                    std::vector<null_order> const& null_precedence, stream_ref stream = get_default_stream(),
                                    rmm::device_async_resource_ref mr = get_current_device_resource_ref());

}  // namespace cudf
