// SPDX-License-Identifier: Apache-2.0
// cudf::distinct_count of a column and of a table. Signatures follow reference cpp/include/cudf/reduction/distinct_count.hpp; the
// stream type is this library's.
//
// Contract (reference cpp/src/reductions/distinct_count.cu, detail::distinct_count):
//  - table: the number of distinct rows, rows compared as cudf::distinct compares them with NaN equal to NaN; nulls_equal as there.
//    Zero rows give 0.
//  - column: 0 for an empty column (distinct_count.cu:195). If every element is null: 1 with null_policy::INCLUDE, 0 with EXCLUDE
//    (:197-199). Otherwise the table count with nulls EQUAL, less 1 when the column has nulls and the policy is EXCLUDE, less 1
//    more when nan_policy::NAN_IS_NULL, the column holds a valid NaN, and it has nulls or the policy is EXCLUDE (:201-218).
//  - Key columns are limited as for cudf::distinct (include/cudf/stream_compaction.hpp).
#pragma once
#include <cudf/column/column_view.hpp>
#include <cudf/table/table_view.hpp>
#include <cudf/types.hpp>
#include <cudf/utilities/default_stream.hpp>

namespace cudf {

size_type distinct_count(column_view const& input, null_policy null_handling, nan_policy nan_handling,
                         stream_ref stream = get_default_stream());

size_type distinct_count(table_view const& input, null_equality nulls_equal = null_equality::EQUAL,
                         stream_ref stream = get_default_stream());

}  // namespace cudf
