// SPDX-License-Identifier: Apache-2.0
// The sort helper shared by the sort-based aggregate (sort_groupby.hip) and the scans (scan_groupby.hip): the reference's
// sort_groupby_helper (cpp/include/cudf/detail/groupby/sort_helper.hpp) built on the stable LSD radix sort of sort_groupby.hip.
// One definition of the sorter and of the helper lives in sort_groupby.hip; this header only declares them.
#pragma once
#include "call.hpp"

#include <cudf/table/table_view.hpp>

#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <optional>
#include <tuple>
#include <utility>

namespace cudf::groupby::detail {

// order-preserving 64-bit word of one element: unsigned comparison of words == the reference's ascending order of values
// (NaN above every number and all NaNs one value, -0 == +0: cpp/include/cudf/detail/row_operator/lexicographic.cuh)
__device__ __forceinline__ uint64_t sortable_word(cudf::detail::device_column const& c, int64_t row)
{
  using namespace cudf::detail;
  uint64_t const raw = col_load_bits(c, row);
  switch (c.cls) {
    case CLS_SINT: {
      int const sh = 64 - 8 * c.width;
      return static_cast<uint64_t>(static_cast<int64_t>(raw << sh) >> sh) ^ 0x8000000000000000ull;
    }
    case CLS_BOOL: return raw != 0;
    case CLS_F32: {
      uint32_t b = static_cast<uint32_t>(normalize_key_bits(raw, CLS_F32));
      return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
    }
    case CLS_F64: {
      uint64_t b = normalize_key_bits(raw, CLS_F64);
      return b ^ ((b >> 63) ? 0xffffffffffffffffull : 0x8000000000000000ull);
    }
    default: return raw;
  }
}

inline unsigned blocks_of(int64_t n) { return static_cast<unsigned>(std::max<int64_t>((n + 255) / 256, 1)); }

// out[0 .. n) = exclusive prefix sums of in[0 .. n); *total (device, optional) = the sum. in == out is allowed.
void exclusive_scan(uint32_t const* in, uint32_t* out, int64_t n, uint32_t* total, scratch& sc, hipStream_t s);

// The key order, the group labels and offsets, and per values column the order inside the groups.
struct helper {
  table_view keys;
  cudf::detail::device_table dkeys;
  int64_t n{0};    // rows
  int64_t nk{0};   // rows whose key takes part (n minus the rows of excluded null keys)
  int32_t G{0};    // groups
  uint32_t* order{nullptr};     // position in key order -> row, nk used
  int32_t* labels{nullptr};     // per position
  int32_t* offsets{nullptr};    // G + 1
  int32_t* first_row{nullptr};  // per group: a row holding its key
  bool identity_order{false};   // order[i] == i for every i < nk == n (pre-sorted keys, nothing dropped)
  scratch keep;                 // the arrays above
  hipStream_t s;

  helper(table_view const& k, hipStream_t stream);

  // inner_values: a values column whose order INSIDE the groups is wanted and nobody needs the rows of a group in their original
  // order: its words are sorted first, the key columns after them (see sort_groupby.hip).
  void build(bool exclude_null_keys, bool presorted, column_view const* inner_values = nullptr);

  // rows in (label, null, value) order (reference sort_helper.cu:205-225 sorted_values, and the (label, value) sort of
  // scan.cpp's RANK): vrow[i] for i in the group's range. Ties keep key order (the sort is stable). descending inverts the value
  // words; nulls_first puts a group's nulls before its values. The reference's row comparator flips a column's whole ordering
  // for DESCENDING, nulls included, so a caller passes nulls_first = (null_precedence == BEFORE) != (order == DESCENDING).
  uint32_t* value_order(column_view const& values, bool descending = false, bool nulls_first = false);

  // valid rows of `values` before each position of the key order (nk + 1 entries), and per group
  uint32_t* valid_before(column_view const& values, scratch& tmp, uint32_t** flags_out = nullptr);

 private:
  // a value order is reusable only for the same column contents and the same ordering
  using value_key = std::tuple<void const*, size_type, bitmask_type const*, int32_t, size_type, bool, bool>;
  static value_key key_of(column_view const& v, bool descending, bool nulls_first)
  {
    return {v.head(), v.offset(), v.null_mask(), static_cast<int32_t>(v.type().id()), v.size(), descending, nulls_first};
  }
  std::map<value_key, uint32_t*> _value_orders;
  std::optional<value_key> _value_orders_in_key_order;
};

}  // namespace cudf::groupby::detail
