// SPDX-License-Identifier: Apache-2.0
// The device primitives under the sort-based groupby (radix_sort.hip): a stable least-significant-digit radix sort of
// (64-bit word, 32-bit payload) pairs in 8-bit digits, and a device-wide exclusive scan of uint32.
#pragma once
#include "call.hpp"

#include <hip/hip_runtime.h>

namespace cudf::detail::sorting {
struct plan_word;  // sorting/sorting_impl.hpp
}

namespace cudf::groupby::detail {

// out[0 .. n) = exclusive prefix sums of in[0 .. n); *total (device, optional) = the sum. in == out is allowed.
void exclusive_scan(uint32_t const* in, uint32_t* out, int64_t n, uint32_t* total, scratch& sc, hipStream_t s);
// out[i] = i
void iota(uint32_t* out, int64_t n, hipStream_t s);

// what to make a word of; p = the payload of the position (the position itself before the first pass), row = order ? order[p] : p
enum word_source : int32_t {
  WORD_VALUE      = 0,  // sortable_word(col[row]), 0 for a null; inverted if `invert`
  WORD_NULL_FLAG  = 1,  // 1 for a null of col[row]
  WORD_ANY_NULL   = 2,  // 1 if any column of `keys` holds a null in the row
  WORD_LABEL_NULL = 3   // (labels[p] << 1) | null flag of col[row] (nulls_first: valid flag)
};

struct fill_args {
  // the caller of pair_sorter::sort_by sets these
  cudf::detail::device_table keys;  // WORD_ANY_NULL
  cudf::detail::device_column col;  // the others
  uint32_t const* order;            // nullptr: row = p
  int32_t const* labels;            // WORD_LABEL_NULL
  int32_t source;
  bool invert;                      // WORD_VALUE: descending
  bool nulls_first;                 // WORD_LABEL_NULL: the flag is 1 for a valid row instead of a null one
  // the sorter sets these
  uint32_t const* payload;          // nullptr: identity
  int64_t n;
  uint64_t* words;
  uint64_t* or_and;                 // [0] |= word, [1] &= word
  uint32_t* ones;                   // WORD_ANY_NULL: number of words equal to 1
};

// (word, payload) pairs in two buffers each; sort_by() fills one word column and runs the passes it needs. Digits in which all
// words agree are skipped (one OR / AND reduction per word column tells), so a 32-bit key column of a few million distinct values
// costs three passes, not eight.
class pair_sorter {
 public:
  pair_sorter(int64_t n, scratch& sc, hipStream_t s);
  // makes the words of fa's source from the payloads in front and sorts the pairs by them, stably (one synchronisation: the
  // OR / AND of the words comes back to pick the digits that differ); returns the count of WORD_ANY_NULL ones
  uint32_t sort_by(fill_args fa);
  // as sort_by, by one packed word of several key columns (cudf::sorted_order: sorting/sorting_impl.hpp)
  void sort_by_packed(cudf::detail::sorting::plan_word const& w);
  // the words in front: those of the last sort_by(), in sorted order
  [[nodiscard]] uint64_t const* words() const { return _k[_cur]; }
  // payload after the last pass, materialised (identity if nothing ever moved)
  uint32_t* finish();

 private:
  [[nodiscard]] uint32_t const* payload() const { return _identity ? nullptr : _p[_cur]; }
  void reset_reduction();
  uint32_t sort_filled();
  void pass(int shift);
  int64_t _n;
  scratch& _sc;
  hipStream_t _s;
  uint32_t _nblocks{0};
  uint64_t* _k[2]{};
  uint32_t* _p[2]{};
  uint32_t* _hist{nullptr};
  uint64_t* _or_and{nullptr};
  uint32_t* _ones{nullptr};
  int _cur{0};
  bool _identity{true};
};

}  // namespace cudf::groupby::detail
