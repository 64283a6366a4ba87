// SPDX-License-Identifier: Apache-2.0
// Replacement policies (reference cpp/include/cudf/replace.hpp:32); groupby::replace_nulls takes one per column.
#pragma once

namespace cudf {

// PRECEDING: a null takes the nearest valid value before it; FOLLOWING: the nearest valid value after it
enum class replace_policy : bool { PRECEDING, FOLLOWING };

}  // namespace cudf
