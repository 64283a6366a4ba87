// SPDX-License-Identifier: Apache-2.0
// The packed radix words of cudf::sorted_order / is_sorted / rank (include/cudf/sorting.hpp) and of cudf::lower_bound / upper_bound /
// merge (search.hpp, merge.hpp): the plan the host makes of a key table (sorting.cpp) and the launchers of the kernels that read
// it (sorting_kernels.hip, search_merge_kernels.hip) or its sorted words (rank_kernels.hip).
//
// Layout. Each key column is a field of vbits + nbit bits: vbits = 1 for BOOL8, otherwise 8 * width; nbit = 1 if the column has
// nulls, else 0. The columns are walked from the last to the first and each field is placed above the fields already in the
// current 64-bit word, so an earlier column is more significant; a field that does not fit starts a new word. A 65-bit field (a
// nullable 8-byte column) puts its 64 value bits in a word of their own and its null bit becomes the lowest field of the next
// word. The words are sorted in the order they were made (least significant first) by the stable LSD radix sort of
// groupby/radix_sort.hpp, which skips the bytes in which all words agree.
//
// Inside a field, from the field's lowest bit up:
//   value bits  the width-tight order-preserving code of the element: the sign bit of the width-byte integer flipped, floats
//               normalised (-0 -> +0, every NaN the canonical quiet NaN) and sign-magnitude folded, BOOL8 as 0 / 1 - ordered_word
//               (common/device_table.hpp) without the sign extension to 64 bits. Complemented for DESCENDING. All zero for a null
//               row, so nulls tie and keep their input order.
//   null bit    above the value bits: 0 for the kind of row (null or valid) that comes first in the output, 1 for the other. Nulls
//               come first exactly when (null_precedence == BEFORE) != (order == DESCENDING).
#pragma once
#include "../common/device_table.hpp"

#include <cudf/aggregation.hpp>

#include <hip/hip_runtime.h>

#include <vector>

namespace cudf::detail::sorting {

constexpr int MAX_FIELDS = 2 * MAX_COLS;  // of a whole plan: a column gives one field, a nullable 8-byte column two
constexpr int MAX_WORDS  = 2 * MAX_COLS;

struct plan_field {
  device_column col;   // (mask == nullptr: the column has no nulls)
  int32_t shift;       // lowest bit of the value bits in the word
  int32_t vbits;       // 0: the field is the null bit alone (the upper half of a 65-bit field)
  int32_t null_pos;    // bit of the null bit in the word; -1: none in this word
  int32_t invert;      // DESCENDING: the value bits are complemented
  int32_t null_first;  // nulls come first in the output: the null bit is 1 for a VALID row
};

// one radix word: at most one field per key column
struct plan_word {
  plan_field f[MAX_COLS];
  int32_t nfields;
};

// every word of a key table, least significant first: word w is made of f[begin[w] .. begin[w + 1])
struct packed_plan {
  plan_field f[MAX_FIELDS];
  int32_t begin[MAX_WORDS + 1];
  int32_t nwords;

  [[nodiscard]] plan_word word(int w) const
  {
    plan_word out{};
    out.nfields = begin[w + 1] - begin[w];
    for (int i = 0; i < out.nfields; ++i) out.f[i] = f[begin[w] + i];
    return out;
  }
};

// Throws unless column_order and null_precedence are empty or have one entry per column of `keys`.
void check_orders(table_view const& keys, std::vector<order> const& column_order, std::vector<null_order> const& null_precedence);
// The words of `keys`, least significant first ("Layout"). Bit c of `force_null_bit`: column c gets a null bit even without a mask,
// so that two tables of one schema get one layout when only one of them has nulls in the column (the side without a mask reads as
// all valid).
packed_plan make_plan(table_view const& keys, std::vector<order> const& column_order, std::vector<null_order> const& null_precedence,
                      uint32_t force_null_bit = 0);

// words[i] = word `w` of row (payload ? payload[i] : i) for i < n; or_and[0] |= word, or_and[1] &= word
void launch_fill_packed_words(plan_word const& w, uint32_t const* payload, uint64_t* words, uint64_t* or_and, int64_t n, hipStream_t s);
// *flag (device, zeroed by the caller) becomes non-zero if some row i in [1, n) is lexicographically less than row i - 1; p: the
// plan in device memory, at least one word
void launch_is_sorted(packed_plan const* p, int64_t n, uint32_t* flag, hipStream_t s);

// ---- cudf::rank (rank_kernels.hip): the sorted words of ONE column, word i that of sorted position i, and order[i] the row at
// that position. hi == nullptr: one word; otherwise lo is the value word and hi the null-bit word of a nullable 8-byte column.
struct rank_words {
  uint64_t const* lo;
  uint64_t const* hi;
};
constexpr int RANK_TILE = 2048;  // the sorted positions one workgroup ranks at a time (256 threads, 8 each)
// OUT is int32_t or double. With `percentage` (double only) every rank is divided by `divisor`.
// out[order[i]] = i + 1
template <typename OUT>
void launch_rank_first(uint32_t const* order, OUT* out, int64_t n, bool percentage, double divisor, hipStream_t s);
// method MIN / MAX / AVERAGE: out[order[i]] = the first position of i's run of equal words + 1 / the last + 1 / their mean
template <typename OUT>
void launch_rank_ties(rank_words const& w, uint32_t const* order, OUT* out, int64_t n, rank_method method, bool percentage,
                      double divisor, hipStream_t s);
// counts[t] = the runs that start in tile t, for every tile of RANK_TILE positions; *q_heads = those of position q's tile that
// start at or before q (q < 0: 0)
void launch_rank_dense_count(rank_words const& w, int64_t n, uint32_t* counts, int64_t q, uint32_t* q_heads, hipStream_t s);
// out[order[i]] = the runs that start at or before i; tile_base: the exclusive scan of `counts`. The divisor of a percentage is
// the dense rank of position q, tile_base[q / RANK_TILE] + *q_heads, read on the device.
template <typename OUT>
void launch_rank_dense_apply(rank_words const& w, uint32_t const* order, OUT* out, int64_t n, uint32_t const* tile_base,
                             bool percentage, int64_t q, uint32_t const* q_heads, hipStream_t s);

// ---- rows of two tables (search_merge_kernels.hip). `plans` is device memory that holds two plans of ONE layout, [0] of the
// haystack and [1] of the needles (launch_store_plans writes them in stream order); nwords is that layout's word count, at least 1.
void launch_store_plans(packed_plan const& haystack, packed_plan const& needles, packed_plan* plans, hipStream_t s);
// out[i] = the number of haystack rows less than (upper: less than or equal to) needle row i, for i < needle_rows
void launch_bound_search(packed_plan const* plans, int nwords, int64_t haystack_rows, int64_t needle_rows, bool upper, int32_t* out,
                         hipStream_t s);
// order[i + bound(i)] = tag | i for every needle row i, with the bound of launch_bound_search; order has haystack_rows +
// needle_rows entries and every position written is inside it
void launch_merge_positions(packed_plan const* plans, int nwords, int64_t haystack_rows, int64_t needle_rows, bool upper, uint32_t tag,
                            uint32_t* order, hipStream_t s);

constexpr uint32_t MERGE_SIDE_B = 0x80000000u;  // an entry of `order`: the side in bit 31, the row of that side's table below
constexpr int MERGE_COLS        = 4;            // columns per launch of the two-source gather
struct merge_cols {
  device_column a[MERGE_COLS];  // column c of side A and of side B: one type; a mask on either, both or neither
  device_column b[MERGE_COLS];
  void* out[MERGE_COLS];
  int32_t ncols;
};
// out[c][i] = element (order[i] & ~MERGE_SIDE_B) of a[c] or b[c], by the side bit, for i < n
void launch_merge_gather(merge_cols const& g, uint32_t const* order, int64_t n, hipStream_t s);
// out_mask bit i = the validity of that element; *null_count (device, zeroed by the caller) += the nulls
void launch_merge_mask(device_column const& a, device_column const& b, uint32_t const* order, int64_t n, bitmask_type* out_mask,
                       int32_t* null_count, hipStream_t s);

}  // namespace cudf::detail::sorting
