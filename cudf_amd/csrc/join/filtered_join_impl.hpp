// SPDX-License-Identifier: Apache-2.0
// cudf::filtered_join, private to the join: the build forms, the kernel arguments and the launchers of
// filtered_join_kernels.hip, and the implementation class behind include/cudf/join/filtered_join.hpp.
//
// Two build forms answer "does the right table hold a row equal to this left row" ("Semi and anti joins"):
//  - bitmap: one integer key column whose valid build keys span a small range [lo, lo + range): one bit per key, set with
//    atomicOr. A probe is a range test and one bit test; a key outside the range touches no memory. Probed from LDS when the
//    bitmap fits (CUDF_AMD_FJOIN_LDS_BITS), through L2 / the Infinity Cache otherwise.
//  - set: the open-addressing set of common/row_set.hpp over the DISTINCT build rows, in HBM. One 4- or 8-byte key column keeps its
//    normalised key bits in the slot (the probe never reads the build table); other keys keep {32-bit row hash | build row} and
//    compare rows with rows_equal.
// Both probes answer one bit per left row (rowset::probe_chunk); the ordered compaction (rowset::compaction, common/row_set_host.hpp)
// turns the bits into ascending indices.
#pragma once
#include "../common/device_table.hpp"

#include <cudf/join/filtered_join.hpp>

#include <hip/hip_runtime.h>
#include <cstdint>

namespace cudf::detail {
namespace fjoin {

enum class form : int8_t {
  empty,   // no build rows
  bitmap,  // one integer key column over a small range
  set,     // the hash set of distinct build rows
};

struct bitmap_args {
  device_column key;  // the (only) key column
  int64_t nrows;
  uint64_t lo;        // the first key of the bitmap, widened to 64 bits (sign-extended for signed columns)
  uint64_t range;     // keys [lo, lo + range); range <= 2^32 * 32
  uint32_t* bits;     // ceil(range / 32) words
  int32_t* seen_null; // build only: set when a build row has a NULL key
};

struct set_args {
  device_table build;
  uint64_t* slots;
  uint64_t capacity;    // slots: > the build rows
  int32_t inline_key;   // 1: one 4- or 8-byte key column, the slot holds its normalised bits zero-extended (an 8-byte key equal to
                        // rowset::EMPTY goes to seen_sentinel instead); 0: the slot holds {row hash << 32 | build row}
  int32_t nulls_equal;
  int32_t* seen_null;      // build only (inline keys): a build row has a NULL key
  int32_t* seen_sentinel;  // build only (inline keys): a build key equals rowset::EMPTY
};

// Pass 1 of the probe side: one bit per left row and the number of qualifying rows per chunk, into the scratch of a
// rowset::compaction over the left rows (its geometry, mask and counts).
struct probe_args {
  device_table probe;
  int32_t anti;        // 1: a row qualifies when it has NO match
  int32_t null_match;  // single-column forms: what a row with a NULL key answers (nulls EQUAL and the build has a NULL row)
  int32_t sentinel_match;  // inline set of an 8-byte key: a probe key equal to rowset::EMPTY matches
  bitmap_args bm;
  set_args set;
  int64_t nrows;
  int64_t chunk;
  int32_t nwaves;      // a multiple of 16
  uint64_t* mask;      // ceil(nrows / 64) words
  unsigned long long* counts;  // nwaves + 1
};

void launch_bitmap_build(bitmap_args const& a, hipStream_t stream);
void launch_set_build(set_args const& a, hipStream_t stream);
// pass 1; lds: the bitmap is copied to LDS by every workgroup (a.bm.range <= lds_bits_max())
void launch_bitmap_probe(probe_args const& a, bool lds, hipStream_t stream);
void launch_set_probe(probe_args const& a, hipStream_t stream);
// out[i] = i for i < n
void launch_fjoin_sequence(size_type* out, int64_t n, hipStream_t stream);
// bits of the largest bitmap the LDS probe takes (the kernel's dynamic LDS)
uint64_t lds_bits_max();

}  // namespace fjoin

class filtered_join_impl {
 public:
  filtered_join_impl(table_view const& right, null_equality compare_nulls, double load_factor, stream_ref stream,
                     rmm::device_async_resource_ref mr);
  [[nodiscard]] std::unique_ptr<rmm::device_uvector<size_type>> probe(table_view const& left, bool anti, stream_ref stream,
                                                                      rmm::device_async_resource_ref mr) const;

 private:
  bool try_bitmap_build(stream_ref stream);
  void set_build(double load_factor, stream_ref stream);

  table_view _right;
  null_equality _nulls_equal;
  rmm::device_async_resource_ref _mr;
  device_table _build_dev{};
  fjoin::form _form{fjoin::form::empty};
  bool _null_match{false};      // single-column forms: a NULL probe key matches
  bool _sentinel_match{false};  // inline set, 8-byte key: the key rowset::EMPTY is in the set
  // bitmap
  uint64_t _lo{0}, _range{0};
  rmm::device_buffer _bits{};
  // set
  bool _inline_key{false};
  uint64_t _capacity{0};
  rmm::device_buffer _slots{};
};

}  // namespace cudf::detail
