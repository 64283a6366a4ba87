// SPDX-License-Identifier: Apache-2.0
// The packed radix words of cudf::sorted_order / is_sorted (include/cudf/sorting.hpp): the plan the host makes of a key table
// (sorting.cpp) and the launchers of the kernels that read it (sorting_kernels.hip).
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

#include <hip/hip_runtime.h>

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

// words[i] = word `w` of row (payload ? payload[i] : i) for i < n; or_and[0] |= word, or_and[1] &= word
void launch_fill_packed_words(plan_word const& w, uint32_t const* payload, uint64_t* words, uint64_t* or_and, int64_t n, hipStream_t s);
// *flag (device, zeroed by the caller) becomes non-zero if some row i in [1, n) is lexicographically less than row i - 1; p: the
// plan in device memory, at least one word
void launch_is_sorted(packed_plan const* p, int64_t n, uint32_t* flag, hipStream_t s);

}  // namespace cudf::detail::sorting
