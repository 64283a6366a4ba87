// SPDX-License-Identifier: Apache-2.0
// cudf::distinct, private: the forms, the kernel arguments and the launchers of distinct_kernels.hip (DESIGN.md section 4,
// "Distinct rows").
//
// A build pass gives every set of equal key rows one 32-bit state word that names its surviving row:
//  - dense: one integer key column whose valid keys span a small range [lo, lo + range): state[key - lo]. Reduced in LDS per
//    workgroup first when the range fits (CUDF_AMD_DISTINCT_LDS_ENTRIES), the touched entries then merged into HBM.
//  - set: the open-addressing set of common/row_set.hpp over the distinct rows. One 4- or 8-byte
//    key column keeps its normalised bits in the slot; under a keep rule the slot is a 16-byte record {key, state[2]} on the cache
//    line the probe just read: state[0] is the row whose CAS inserted the key (a plain store), state[1] folds the other rows
//    (KEEP_FIRST / LAST: atomicMin, skipped when state[0] is already better; KEEP_NONE: a plain store of STATE_MULTI). Other keys keep {row hash | row} in the
//    slot, whose row IS the state: KEEP_FIRST / KEEP_LAST lower / raise it with a 64-bit atomicMin / atomicMax (equal rows have
//    equal hashes), KEEP_NONE marks a repeated row with bit 31 (ROW_MULTI).
// The NULL key (nulls EQUAL) and, for inline 8-byte keys, the key rowset::EMPTY have a state word of their own (special[0], [1]).
// A row that equals no row (a null key under nulls UNEQUAL, a NaN under nans UNEQUAL) bypasses the table: the build sets its bit.
// State words: STATE_EMPTY (no row yet), a row (< 2^31), or STATE_MULTI (KEEP_NONE: more than one row).
// Every update of a state word in HBM reads it first and skips the atomic when the word already holds the rule's answer (words only
// move towards it, so a stale read never skips wrongly). KEEP_ANY in the dense form stores the row into an empty word, no atomic.
// The sweep then streams the state words (or slots) and stores one flag byte per surviving row (plain stores: a row survives
// once); a pack pass turns the bytes into the mask words and per-chunk counts of a rowset::compaction (common/row_set_host.hpp),
// whose scan and ordered compaction write ascending indices. Counting stops after the build: it counts the
// state words that went from empty to taken, plus the bypass rows.
#pragma once
#include "../common/device_table.hpp"

#include <hip/hip_runtime.h>
#include <cstdint>

namespace cudf::detail::distinct {

constexpr uint32_t STATE_EMPTY = 0xffffffffu;
constexpr uint32_t STATE_MULTI = 0xfffffffeu;
constexpr uint64_t ROW_MULTI   = uint64_t{1} << 31;

enum class mode : int32_t { any = 0, first, last, none, count };

struct build_args {
  device_table keys;
  int64_t nrows;
  int32_t mode;         // distinct::mode
  int32_t nulls_equal;  // 1: a null equals a null in the same column
  int32_t nans_equal;   // 1: NaN equals NaN
  // dense: key k has state word state[k - lo], k in [lo, lo + range)
  uint64_t lo, range;
  // set
  uint64_t* slots;      // capacity slots, rowset::EMPTY-filled
  uint64_t capacity;
  int32_t inline_key;   // 1: the slot holds the key's normalised bits and state[slot] its row; 0: {row hash << 32 | row}
  uint64_t slot_stride; // inline set: 8-byte words per slot (1: the key alone, counting; 2: {key, state} records)
  uint32_t* state;      // dense: range words; inline set: the two state words of slot s at state[s * state_stride]; nullptr otherwise
  uint64_t state_stride;  // 4-byte words between consecutive state words (dense 1, inline records 4)
  uint32_t* special;    // 2 words: the NULL key, the key rowset::EMPTY (inline 8-byte keys)
  uint8_t* flags;       // nrows zeroed bytes: 1 for a surviving row (nullptr when counting)
  unsigned long long* counter;  // [0] (counting) new state words + bypass rows; [1] set when a valid NaN key was seen
};

// the build of each form; lds_entries > 0: the dense build reduces in LDS first (range <= lds_entries)
void launch_dense_build(build_args const& a, uint64_t lds_entries, hipStream_t stream);
void launch_set_build(build_args const& a, hipStream_t stream);
// survivors -> flag bytes (not when counting)
void launch_sweep(build_args const& a, hipStream_t stream);
// flag bytes -> mask bits (64 rows per word), and counts[w] = the surviving rows of [w * chunk, (w + 1) * chunk)
void launch_pack(uint8_t const* flags, uint64_t* mask, int64_t nrows, int64_t chunk, int32_t nwaves, unsigned long long* counts,
                         hipStream_t stream);
// the largest dense range the LDS build takes
uint64_t lds_entries_max();

}  // namespace cudf::detail::distinct
