// SPDX-License-Identifier: Apache-2.0
// cudf::distinct_hash_join — a hash join for a right (build) table whose rows are distinct: build once, probe many left tables.
// Public members follow reference cpp/include/cudf/join/distinct_hash_join.hpp (class distinct_hash_join); the stream and
// memory-resource types are this library's, as in hash_join.hpp and filtered_join.hpp. inner_join / left_join are const and may
// run concurrently on different streams.
//
// Contract:
//  - inner_join: {left_indices, right_indices}, one pair per left row that has an equal row in `right`, both vectors sized exactly.
//    This implementation guarantees that the left indices come out strictly ascending (the reference gets the same order from its
//    stable copy_if, without promising it).
//  - left_join: ONE vector of exactly left.num_rows() entries: right_indices[i] is the right row equal to left row i, or JoinNoMatch.
//    It is already a gather map for the right table. The call reads nothing back from the device: the result is valid in stream
//    order.
//  - Row equality is hash_join's: column by column, all NaNs are equal, -0 == +0; with null_equality::EQUAL a null equals a null in
//    the same column; with UNEQUAL a right row with a null key is not inserted and a left row with a null key matches nothing.
//  - A right table without columns throws cudf::logic_error. load_factor must lie in (0, 1] (std::invalid_argument); it sizes the
//    hash map of the build rows ("Joins on a unique-key build table").
//  - A right table without rows yields an empty inner_join and an all-JoinNoMatch left_join; a left table without rows yields empty
//    results.
//  - Otherwise the left table must have the right's column count (std::invalid_argument) and column types
//    (cudf::data_type_error). This is stricter than the reference, which checks neither.
//  - Duplicate right rows: undefined behaviour in the reference; here they are harmless. No call faults or hangs, every left row
//    that has equal right rows gets exactly ONE of them, and which one is unspecified (it may differ between two objects built on
//    the same table, not between two probes of one object).
// Lifetime (as for hash_join and filtered_join): the caller keeps `right`'s memory alive while the object lives; a probe returns
// without synchronising its stream, and the object's build state, which goes back to the pool on the build stream when the object
// is destroyed, must outlive, or be stream-synchronised with, every probe stream it was used on.
#pragma once
#include <cudf/join/join.hpp>
#include <memory>
#include <utility>

namespace cudf {
namespace detail {
class distinct_join_impl;
}

class distinct_hash_join {
 public:
  distinct_hash_join() = delete;
  ~distinct_hash_join();
  distinct_hash_join(distinct_hash_join const&)            = delete;
  distinct_hash_join(distinct_hash_join&&)                 = delete;
  distinct_hash_join& operator=(distinct_hash_join const&) = delete;
  distinct_hash_join& operator=(distinct_hash_join&&)      = delete;

  distinct_hash_join(table_view const& right, null_equality compare_nulls = null_equality::EQUAL, double load_factor = 0.5,
                     stream_ref stream = get_default_stream(), rmm::device_async_resource_ref mr = get_current_device_resource_ref());

  [[nodiscard]] std::pair<std::unique_ptr<rmm::device_uvector<size_type>>, std::unique_ptr<rmm::device_uvector<size_type>>> inner_join(
    table_view const& left, stream_ref stream = get_default_stream(),
    rmm::device_async_resource_ref mr = get_current_device_resource_ref()) const;
  [[nodiscard]] std::unique_ptr<rmm::device_uvector<size_type>> left_join(
    table_view const& left, stream_ref stream = get_default_stream(),
    rmm::device_async_resource_ref mr = get_current_device_resource_ref()) const;

 private:
  std::unique_ptr<detail::distinct_join_impl const> _impl;
};
}  // namespace cudf
