// SPDX-License-Identifier: Apache-2.0
// cudf::distinct_hash_join, private to the join: the build forms, the kernel arguments and the launchers of
// distinct_join_kernels.hip, and the implementation class behind include/cudf/join/distinct_hash_join.hpp.
//
// The build rows are distinct, so the table maps a key to ONE build row ("Joins on a unique-key build table"):
//  - direct: one integer (or bool) key column whose valid build keys span a small range [lo, lo + range): a size_type array over
//    the range, preset to JoinNoMatch, build row r stored at key - lo with a plain store. A probe is a range test and one 4-byte
//    load; a key outside the range touches no memory.
//  - map: the open-addressing table of common/row_set.hpp in HBM, one of three slot layouts (map_kind).
// In the single-column layouts a NULL key is never inserted: the build keeps the row of a NULL build key in a side word (nulls
// EQUAL only), and a NULL probe key answers that word. Both side words live in device memory, so that neither the constructor nor
// a probe reads them back.
#pragma once
#include "../common/device_table.hpp"

#include <cudf/join/distinct_hash_join.hpp>

#include <hip/hip_runtime.h>
#include <cstdint>

namespace cudf::detail {
namespace djoin {

enum class form : int32_t {
  empty,   // no build rows, or none that can match
  direct,  // one integer key column over a small range
  map,     // the open-addressing table
};

enum class map_kind : int32_t {
  key4,  // one 4-byte key column: an 8-byte slot {normalised key bits << 32 | build row}, claimed with one CAS
  key8,  // one 8-byte key column: a 16-byte slot {normalised key bits, build row}; the key is claimed with a 64-bit CAS, the row
         // stored after it (probes run after the build kernel has ended). The key rowset::EMPTY goes to side[1] instead.
  rows,  // any other key: an 8-byte slot {32-bit row hash << 32 | build row}, rows compared with rows_equal
};

struct table_args {
  device_table build;
  int32_t table_form;  // form
  int32_t kind;        // map_kind
  int32_t nulls_equal;
  // direct
  uint64_t lo;          // the first key of the table: the raw bits of the key's width, zero-extended
  uint64_t range;       // keys [lo, lo + range), wrapping within the key's width; range <= 2^32 entries
  size_type* direct;    // max(range, 1) entries
  // map
  uint64_t* slots;      // capacity slots of 8 bytes (key4, rows) or 16 bytes (key8)
  uint64_t capacity;    // > the build rows: every probe sequence ends at an empty slot
  // single-column layouts: side[0] = the row of a NULL build key (nulls EQUAL), side[1] = the row of the 8-byte key rowset::EMPTY;
  // JoinNoMatch when there is none
  size_type* side;
};

// The probe (rowset::probe_chunk over rowset::geometry_of's chunks). The pass writes found[i] = the build row of left row i or
// JoinNoMatch. For left_join that is the result. For inner_join (mask != nullptr) it also fills the scratch of a rowset::compaction,
// and after its scan the compaction writes {i, found[i]} of the set bits, ascending.
struct probe_args {
  device_table probe;
  table_args t;
  int64_t nrows;
  int64_t chunk;
  int32_t nwaves;
  size_type* found;            // nrows
  uint64_t* mask;              // inner_join: ceil(nrows / 64) words; left_join: nullptr
  unsigned long long* counts;  // inner_join: nwaves + 1
  size_type* out_left;
  size_type* out_right;
  uint64_t out_capacity;
};

void launch_build(table_args const& a, hipStream_t stream);
void launch_probe(probe_args const& a, hipStream_t stream);
void launch_compact(probe_args const& a, hipStream_t stream);

}  // namespace djoin

class distinct_join_impl {
 public:
  distinct_join_impl(table_view const& right, null_equality compare_nulls, double load_factor, stream_ref stream,
                     rmm::device_async_resource_ref mr);
  [[nodiscard]] join_index_pair inner_join(table_view const& left, stream_ref stream, rmm::device_async_resource_ref mr) const;
  [[nodiscard]] std::unique_ptr<rmm::device_uvector<size_type>> left_join(table_view const& left, stream_ref stream,
                                                                          rmm::device_async_resource_ref mr) const;

 private:
  bool try_direct_build(stream_ref stream);
  void map_build(double load_factor, stream_ref stream);
  void alloc_side(hipStream_t s);
  djoin::probe_args probe_args_of(table_view const& left) const;

  table_view _right;
  null_equality _nulls_equal;
  rmm::device_async_resource_ref _mr;
  djoin::table_args _table{};  // form::empty until a build succeeds
  rmm::device_buffer _entries{}, _side{};
};

}  // namespace cudf::detail
