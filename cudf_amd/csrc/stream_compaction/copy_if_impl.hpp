// SPDX-License-Identifier: Apache-2.0
// cudf::apply_boolean_mask, apply_deletion_mask, drop_nulls, drop_nans, unique and unique_count, private: the kernel arguments
// and the launchers of copy_if_kernels.hip ("Filtering rows").
//
// Pass 1 (selection) writes one bit per row into the mask words of a rowset::compaction (common/row_set_host.hpp), 64 rows per
// word, and the number of set bits per chunk; its scan gives every chunk its offset in the output and the output's size.
//  - select_bool / select_nan / select_valid_count / select_unique / select_unique_column: rowset::probe_chunk<..., MASK = true>
//    with a load and an answer of their own, a row per lane.
//  - select_valid_words: drop_nulls when every nullable key must be valid. No per-row work: a lane funnels the 64 validity bits of
//    each nullable key at the column's bit offset, ANDs them and stores the word.
// Pass 2 turns the selection into columns without an index vector:
//  - copy_if_data: a wave per chunk walks the chunk's mask words (rowset::compact_chunk) and copies, for every set bit, the
//    element of each column of a batch from the row to its position. The batch is read from device memory, in place.
//  - copy_if_validity: the bitmask compaction. It never reads column data: per 64 selection words a lane extracts the validity
//    bits of its 64 rows at the set positions of its selection word (a software parallel extract), ORs them at its position into a
//    wave-private LDS staging area, and the wave writes the staged words out: interior words with plain stores, the two words it
//    shares with its neighbours with a global atomicOr into the zero-filled output mask. Valid bits are counted per column.
#pragma once
#include "../common/device_table.hpp"

#include <hip/hip_runtime.h>
#include <cstdint>

namespace cudf::detail::copy_if {

// ------------------------------------------------------------------ pass 1
// What every selection kernel gets: the chunk geometry and the two outputs of rowset::probe_chunk.
struct select_base {
  int64_t nrows;
  int64_t chunk;
  int32_t nwaves;
  uint64_t* mask;              // ceil(nrows / 64) words, every one written
  unsigned long long* counts;  // nwaves entries
};

// apply_boolean_mask / apply_deletion_mask: row i qualifies iff element i of `m` is valid and (deletion ? zero : non-zero)
struct bool_args : select_base {
  device_column m;
};

// the validity words of a key column: bit (offset + i) of `mask` is row i's
struct valid_key {
  bitmask_type const* mask;
  int64_t offset;
};
// drop_nulls over the nullable keys alone (the host has counted the mask-less keys towards the threshold): row i qualifies iff at
// least `need` of the nkeys bits are set; select_valid_words: need == nkeys
struct valid_args : select_base {
  valid_key key[MAX_COLS];
  int32_t nkeys;
  int32_t need;
};

// drop_nans: row i qualifies iff at least `need` of the float key fields are null or not NaN
struct nan_args : select_base {
  device_table keys;
  int32_t need;
};

enum class keep : int32_t { first = 0, last, none };
// unique / unique_count(table): rows compared with their neighbours by rows_equal
struct unique_args : select_base {
  device_table keys;
  int32_t nulls_equal;
};
// unique_count(column): reference cpp/src/reductions/unique_count_column.cu
struct unique_column_args : select_base {
  device_table keys;  // the one column
  int32_t count_nulls;  // null_policy::INCLUDE
  int32_t nan_is_null;  // nan_policy::NAN_IS_NULL (and the column is FLOAT32 or FLOAT64)
};

void launch_select_bool(bool_args const& a, bool deletion, hipStream_t stream);
void launch_select_valid_words(valid_args const& a, hipStream_t stream);
void launch_select_valid_count(valid_args const& a, hipStream_t stream);
void launch_select_nan(nan_args const& a, hipStream_t stream);
void launch_select_unique(unique_args const& a, keep k, hipStream_t stream);
void launch_select_unique_column(unique_column_args const& a, hipStream_t stream);

// ------------------------------------------------------------------ pass 2
// What both compaction kernels read of the selection (counts scanned: the chunks' offsets).
struct compact_base {
  uint64_t const* mask;
  unsigned long long const* counts;
  int64_t chunk;
  int64_t nrows;
  uint64_t out_rows;  // the scan's total: no position reaches it
  int32_t nwaves;
  int32_t ncols;
};

constexpr int DATA_COLS = 4;  // columns per copy_if_data launch (as k_gather_multi; 8 took 187 VGPRs)
struct data_col {
  void const* src;  // element 0 of the (sliced) column
  void* dst;
  int64_t width;    // 1, 2, 4, 8
};
struct data_args : compact_base {
  data_col col[DATA_COLS];
};

constexpr int VALIDITY_COLS = 16;  // nullable columns per copy_if_validity launch
struct validity_col {
  bitmask_type const* src;  // bit (offset + i) is row i's
  int64_t offset;
  bitmask_type* dst;        // zero-filled, bitmask_allocation_size_bytes(out_rows)
  unsigned long long* valid;  // zeroed; the set bits written to dst are added to it
};
struct validity_args : compact_base {
  validity_col col[VALIDITY_COLS];
};

// `d_args`: the arguments in device memory, stored in stream order before the launch; the kernels read them there
void launch_copy_if_data(data_args const& a, data_args* d_args, hipStream_t stream);
void launch_copy_if_validity(validity_args const& a, validity_args* d_args, hipStream_t stream);

}  // namespace cudf::detail::copy_if
