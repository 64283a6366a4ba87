// SPDX-License-Identifier: Apache-2.0
// cudf::unique_count of a column and of a table: the number of runs of equal consecutive rows, what a caller asks of sorted input.
// Signatures follow reference cpp/include/cudf/reduction/unique_count.hpp; the stream type is this library's.
//
// Contract (reference cpp/src/reductions/unique_count.cu and unique_count_column.cu, the code):
//  - table: the number of rows i with i == 0 or row i different from row i - 1, rows compared as cudf::unique compares them (NaN
//    equals NaN, -0 equals +0, nulls by nulls_equal). 0 for zero rows; a table of zero columns has zero rows here.
//  - column: 0 when the column is empty or all null. Otherwise row i counts under these rules, in this order:
//      1. null_policy::EXCLUDE: a null row never counts; with nan_policy::NAN_IS_NULL a NaN row never counts either.
//      2. Row 0 counts.
//      3. INCLUDE with NAN_IS_NULL: a null or NaN row counts iff row i - 1 is neither null nor NaN.
//      4. Every other row counts iff it differs from row i - 1, nulls equal and NaNs equal.
//    The comparison is with the input's previous row, not with the previous row that counted: {1, null, 1} under EXCLUDE gives 2.
//  - Pass 1 of the stream compaction alone ("Filtering rows"): no output is allocated.
//  - Key columns are limited as for cudf::unique (include/cudf/stream_compaction.hpp).
#pragma once
#include <cudf/column/column_view.hpp>
#include <cudf/table/table_view.hpp>
#include <cudf/types.hpp>
#include <cudf/utilities/default_stream.hpp>

namespace cudf {

size_type unique_count(column_view const& input, null_policy null_handling, nan_policy nan_handling,
                       stream_ref stream = get_default_stream());

size_type unique_count(table_view const& input, null_equality nulls_equal = null_equality::EQUAL,
                       stream_ref stream = get_default_stream());

}  // namespace cudf
