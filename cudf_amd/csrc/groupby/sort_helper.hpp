// SPDX-License-Identifier: Apache-2.0
// The sort helper shared by the sort-based aggregate (sort_aggregate.hip) and the scans (scan_groupby.hip): the reference's
// sort_groupby_helper (cpp/include/cudf/detail/groupby/sort_helper.hpp) built on the radix sort of radix_sort.hpp, and the device
// idioms both sides share. The definitions are in sort_helper.hip.
#pragma once
#include "radix_sort.hpp"

#include <cudf/table/table_view.hpp>

#include <map>
#include <optional>
#include <tuple>

namespace cudf::groupby::detail {

// order-preserving 64-bit word of one element: unsigned comparison of words == the reference's ascending order of values
// (NaN above every number and all NaNs one value, -0 == +0: cpp/include/cudf/detail/row_operator/lexicographic.cuh)
__device__ __forceinline__ uint64_t sortable_word(cudf::detail::device_column const& c, int64_t row)
{
  return cudf::detail::ordered_word(cudf::detail::normalize_key_bits(cudf::detail::col_load_bits(c, row), c.cls), c.cls, c.width);
}

// are the values of rows a and b equal (nulls equal nulls)?
__device__ __forceinline__ bool same_value(cudf::detail::device_column const& c, uint32_t a, bool a_valid, uint32_t b)
{
  return a_valid == cudf::detail::col_is_valid(c, b) && (!a_valid || sortable_word(c, a) == sortable_word(c, b));
}

// One element (e of n) per lane: writes the two 32-bit mask words of this wave's 64 elements and adds their nulls to *null_count.
// Every lane of the wave calls it.
__device__ __forceinline__ void store_wave_validity(bool valid, int64_t e, int64_t n, bitmask_type* mask, int32_t* null_count)
{
  uint64_t const m = __ballot(valid);
  int const lane   = threadIdx.x & 63;
  int64_t const w0 = (e - lane) >> 5;  // first mask word of this wave's 64 elements
  if (lane == 0 && e < n) {
    cudf::detail::gstore(mask + w0, static_cast<bitmask_type>(m));
    int64_t const live  = n - e < 64 ? n - e : 64;
    int32_t const nulls = static_cast<int32_t>(live) - __popcll(m);
    if (nulls) atomicAdd(null_count, nulls);
  }
  if (lane == 32 && e < n) cudf::detail::gstore(mask + w0 + 1, static_cast<bitmask_type>(m >> 32));
}

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
  int32_t* first_row{nullptr};  // per group: the first row of the input that holds its key
  bool identity_order{false};   // order[i] == i for every i < nk == n (pre-sorted keys, nothing dropped)
  scratch keep;                 // the arrays above
  hipStream_t s;

  helper(table_view const& k, hipStream_t stream);

  // inner_values: a values column whose order INSIDE the groups is wanted and nobody needs the rows of a group in their original
  // order: its words are sorted first, the key columns after them (see sort_helper.hip).
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
