// SPDX-License-Identifier: Apache-2.0
// cudf::filtered_join — left semi and anti joins: build once on the right (filter) table, probe many left tables. Public members
// follow reference cpp/include/cudf/join/filtered_join.hpp (class filtered_join); the stream and memory-resource types are this
// library's, as in hash_join.hpp. semi_join / anti_join are const and may run concurrently on different streams.
//
// Contract:
//  - semi_join: the left row indices that have at least one equal row in `right`; anti_join: those that have none.
//  - The indices come out in ascending order, each left row at most once, the vector sized exactly.
//  - Row equality is hash_join's: column by column, NaN == NaN, -0 == +0; with null_equality::EQUAL a null equals a null in the
//    same column; with UNEQUAL a row with a null key never matches (it is absent from semi_join, present in anti_join).
//  - An empty left table yields an empty result; an empty right table an empty semi_join and every left row from anti_join.
//  - Otherwise the left table must have the right's column count (std::invalid_argument) and column types (cudf::data_type_error).
//  - load_factor must lie in (0, 1] (std::invalid_argument); it sizes the hash set of the build rows ("Semi and anti joins").
// Lifetime (as for hash_join): the caller keeps `right`'s memory alive while the object lives; a probe returns without
// synchronising its stream, and the object's build state, which goes back to the pool on the build stream when the object is
// destroyed, must outlive, or be stream-synchronised with, every probe stream it was used on.
#pragma once
#include <cudf/join/join.hpp>
#include <memory>

namespace cudf {
namespace detail {
class filtered_join_impl;
}

class filtered_join {
 public:
  filtered_join() = delete;
  ~filtered_join();
  filtered_join(filtered_join const&)            = delete;
  filtered_join(filtered_join&&)                 = delete;
  filtered_join& operator=(filtered_join const&) = delete;
  filtered_join& operator=(filtered_join&&)      = delete;

  filtered_join(table_view const& right, null_equality compare_nulls, stream_ref stream,
                rmm::device_async_resource_ref mr = get_current_device_resource_ref());
  filtered_join(table_view const& right, null_equality compare_nulls, double load_factor, stream_ref stream,
                rmm::device_async_resource_ref mr = get_current_device_resource_ref());

  [[nodiscard]] std::unique_ptr<rmm::device_uvector<size_type>> semi_join(
    table_view const& left, stream_ref stream = get_default_stream(),
    rmm::device_async_resource_ref mr = get_current_device_resource_ref()) const;
  [[nodiscard]] std::unique_ptr<rmm::device_uvector<size_type>> anti_join(
    table_view const& left, stream_ref stream = get_default_stream(),
    rmm::device_async_resource_ref mr = get_current_device_resource_ref()) const;

 private:
  std::unique_ptr<detail::filtered_join_impl const> _impl;
};
}  // namespace cudf
