// SPDX-License-Identifier: Apache-2.0
// cudf::filtered_join, private to the join: the build forms, the kernel arguments and the launchers of
// filtered_join_kernels.hip, and the implementation class behind include/cudf/join/filtered_join.hpp.
//
// Two build forms answer "does the right table hold a row equal to this left row" ("Semi and anti joins"):
//  - bitmap: one integer key column whose valid build keys span a small range [lo, lo + range): one bit per key, set with
//    atomicOr. A probe is a range test and one bit test; a key outside the range touches no memory. Probed from LDS when the
//    bitmap fits (CUDF_AMD_FJOIN_LDS_BITS), through L2 / the Infinity Cache otherwise.
//  - set: an open-addressing set of the DISTINCT build rows in HBM, linear probing, built with 64-bit CAS. One 4- or 8-byte key
//    column keeps its normalised key bits in the slot (the probe never reads the build table); other keys keep
//    {32-bit row hash | build row} and compare rows with rows_equal.
// Both probes answer one bit per left row; the ordered compaction (launch_fjoin_compact) turns the bits into ascending indices.
#pragma once
#include "../common/device_table.hpp"

#include <cudf/join/filtered_join.hpp>

#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>

namespace cudf::detail {
namespace fjoin {

constexpr uint64_t SET_EMPTY = ~uint64_t{0};  // an unused slot of the set (no valid entry has this value, see set_args::inline_key)

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
  int32_t inline_key;   // 1: one 4- or 8-byte key column, the slot holds its normalised bits zero-extended (SET_EMPTY for an
                        // 8-byte key of that value goes to seen_sentinel instead); 0: the slot holds {row hash << 32 | build row}
  int32_t nulls_equal;
  int32_t* seen_null;      // build only (inline keys): a build row has a NULL key
  int32_t* seen_sentinel;  // build only (inline keys): a build key equals SET_EMPTY
};

// The probe side and the ordered compaction. Left rows are cut into `nwaves` contiguous chunks of `chunk` rows (a multiple of
// 512), one per wave; pass 1 writes one bit per row (mask, 64 rows per word, a word never spans two chunks) and the number of
// qualifying rows per chunk (counts); launch_scan turns the counts into exclusive offsets; pass 2 writes the qualifying rows of
// each chunk at its offset, in row order.
struct probe_args {
  device_table probe;
  int32_t anti;        // 1: a row qualifies when it has NO match
  int32_t null_match;  // single-column forms: what a row with a NULL key answers (nulls EQUAL and the build has a NULL row)
  int32_t sentinel_match;  // inline set of an 8-byte key: a probe key equal to SET_EMPTY matches
  bitmap_args bm;
  set_args set;
  int64_t nrows;
  int64_t chunk;
  int32_t nwaves;      // a multiple of 16
  uint64_t* mask;      // ceil(nrows / 64) words
  unsigned long long* counts;  // nwaves + 1
  size_type* out;
  uint64_t out_capacity;
};

// Rows per wave chunk of pass 1 and of the compaction: at most 8192 waves (32 per CU), chunks of >= 4096 rows, a multiple of 512
// (pass 1 tests 8 x 64 rows at a time); the number of waves a multiple of 16 (the LDS probe's workgroup).
struct geometry {
  int32_t nwaves;
  int64_t chunk;
};
inline geometry geometry_of(int64_t n)
{
  int64_t waves       = std::clamp<int64_t>((n + 4095) / 4096, 16, 8192);
  int64_t const chunk = ((n + waves - 1) / waves + 511) / 512 * 512;
  waves               = ((n + chunk - 1) / chunk + 15) / 16 * 16;
  return {static_cast<int32_t>(waves), chunk};
}

void launch_bitmap_build(bitmap_args const& a, hipStream_t stream);
void launch_set_build(set_args const& a, hipStream_t stream);
// pass 1; lds: the bitmap is copied to LDS by every workgroup (a.bm.range <= lds_bits_max())
void launch_bitmap_probe(probe_args const& a, bool lds, hipStream_t stream);
void launch_set_probe(probe_args const& a, hipStream_t stream);
// pass 2 (counts scanned)
void launch_fjoin_compact(probe_args const& a, hipStream_t stream);
// out[i] = i for i < n
void launch_fjoin_sequence(size_type* out, int64_t n, hipStream_t stream);
// [lo, lo + range): the valid keys of integer column c (SINT: compared signed), from launch_key_minmax; synchronises `s`. range 0:
// no valid key. false: the keys span all 2^64 values.
bool valid_key_range(device_column const& c, int64_t rows, uint64_t& lo, uint64_t& range, hipStream_t s);
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
  void validate_probe(table_view const& left) const;
  bool try_bitmap_build(stream_ref stream);
  void set_build(double load_factor, stream_ref stream);

  table_view _right;
  null_equality _nulls_equal;
  rmm::device_async_resource_ref _mr;
  device_table _build_dev{};
  fjoin::form _form{fjoin::form::empty};
  bool _null_match{false};      // single-column forms: a NULL probe key matches
  bool _sentinel_match{false};  // inline set, 8-byte key: the key SET_EMPTY is in the set
  // bitmap
  uint64_t _lo{0}, _range{0};
  rmm::device_buffer _bits{};
  // set
  bool _inline_key{false};
  uint64_t _capacity{0};
  rmm::device_buffer _slots{};
};

}  // namespace cudf::detail
