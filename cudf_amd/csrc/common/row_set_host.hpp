// SPDX-License-Identifier: Apache-2.0
// Host side of what cudf::filtered_join (join/filtered_join.cpp), cudf::distinct_hash_join (join/distinct_join.cpp) and
// cudf::distinct (stream_compaction/distinct.cpp) share: the admission of the small-range integer form, the capacity and slot
// layout of the set, the chunk geometry of the probe with the scratch of the ordered compaction, and the probe validation.
// Device side: row_set.hpp.
#pragma once
#include "device_table.hpp"
#include "../join/hash_join_impl.hpp"

#include <rmm/device_buffer.hpp>
#include <rmm/device_uvector.hpp>

#include <algorithm>
#include <cmath>
#include <optional>
#include <stdexcept>
#include <string>

namespace cudf::detail::rowset {

// ------------------------------------------------------------------ the small-range integer form
// [lo, lo + range): the valid keys of integer column c (SINT: compared signed), from launch_key_minmax; synchronises `s`. range 0:
// no valid key. false: the keys span all 2^64 values.
inline bool valid_key_range(device_column const& c, int64_t rows, uint64_t& lo, uint64_t& range, hipStream_t s)
{
  bool const is_signed = c.cls == CLS_SINT;
  auto tmp             = cudf::get_current_device_resource_ref();
  join::join_args a{};
  a.build.ncols  = 1;
  a.build.nrows  = static_cast<int32_t>(rows);
  a.build.col[0] = c;
  a.check_nulls  = 1;
  rmm::device_buffer mm{2 * sizeof(uint64_t), s, tmp}, d_args{sizeof(join::join_args), s, tmp};
  join::launch_key_minmax(a, static_cast<join::join_args*>(d_args.data()), is_signed ? 1 : 0, static_cast<uint64_t*>(mm.data()), s);
  uint64_t h[2] = {0, 0};
  CUDF_HIP_TRY(hipMemcpyAsync(h, mm.data(), sizeof(h), hipMemcpyDeviceToHost, s));
  CUDF_HIP_TRY(hipStreamSynchronize(s));
  bool const any_valid = is_signed ? static_cast<int64_t>(h[0]) <= static_cast<int64_t>(h[1]) : h[0] <= h[1];
  lo = range = 0;
  if (!any_valid) return true;  // (no valid key: an empty range)
  uint64_t const width = h[1] - h[0];  // exact in two's complement for either ordering
  if (width == ~uint64_t{0}) return false;
  lo    = h[0];
  range = width + 1;
  return true;
}

struct key_range {
  uint64_t lo;     // the first key, widened to 64 bits (sign-extended for signed columns)
  uint64_t range;  // keys [lo, lo + range); 0: no valid key
};

// Whether one integer key column (1, 2, 4 or 8 bytes; timestamps, durations and decimals included; bool when the caller takes it)
// takes a table indexed by key - lo. 1- and 2-byte keys take it over their whole type range (at most 2^16 entries), without a look
// at the keys. 4- and 8-byte keys take it over [min, max] of the valid keys of the first `rows` rows, when that range is at most
// `ratio` entries per row of `of_rows` and at most `max_entries`. (`rows` < `of_rows`: a cheap first look at a prefix, whose range
// is part of the whole range.)
inline std::optional<key_range> small_key_range(device_column const& c, int64_t rows, int64_t of_rows, uint64_t ratio, uint64_t max_entries,
                                                hipStream_t s, bool take_bool = false)
{
  if (c.cls != CLS_SINT && c.cls != CLS_UINT && !(take_bool && c.cls == CLS_BOOL)) return std::nullopt;
  key_range r{0, uint64_t{1} << (8 * c.width)};
  if (c.width <= 2) {
    if (c.cls == CLS_SINT) r.lo = static_cast<uint64_t>(-static_cast<int64_t>(r.range / 2));
    return r;
  }
  if (!valid_key_range(c, rows, r.lo, r.range, s)) return std::nullopt;
  if (r.range > max_entries || r.range > ratio * static_cast<uint64_t>(of_rows)) return std::nullopt;
  return r;
}

// ------------------------------------------------------------------ the set
// Slots of the open-addressing set of `rows` rows: ceil(rows / load), at least rows + 1 (so that at load factor 1 an absent key
// still reaches an empty slot and every walk ends), counted in 64 bits. `what` names the table in the error.
inline uint64_t set_capacity(int64_t rows, double load, char const* what)
{
  auto const n       = static_cast<double>(rows);
  double const slots = std::max(std::ceil(n / load), n + 1);
  CUDF_EXPECTS(slots < 0x1p58, std::string{what} + " of this load factor exceeds the addressable memory", std::overflow_error);
  return static_cast<uint64_t>(slots);
}

// One 4- or 8-byte integer or float key column: the slot keeps the key's normalised bits; every other key keeps {row hash | row}.
inline bool inline_key_column(device_table const& t)
{
  device_column const& c = t.col[0];
  return t.ncols == 1 && (c.width == 4 || c.width == 8) && (c.cls == CLS_SINT || c.cls == CLS_UINT || c.cls == CLS_F32 || c.cls == CLS_F64);
}

// ------------------------------------------------------------------ probe geometry and ordered compaction
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

// out[position] = row for every set bit of the mask, ascending (rowset::compact_chunk; counts scanned). The kernel is
// filtered_join's pass 2 ("fjoin_compact", join/filtered_join_kernels.hip).
void launch_compact_indices(uint64_t const* mask, unsigned long long const* counts, geometry g, int64_t nrows, size_type* out,
                            uint64_t out_capacity, hipStream_t stream);

// The scratch of the ordered compaction of `nrows` rows: a pass 1 of the caller's writes one bit per row (mask, 64 rows per word)
// and the number of set bits per chunk (counts); total() scans the counts into the chunks' offsets; a pass 2 writes the set bits'
// rows at offset + rank, in row order, without atomics. The scratch goes back to the pool in stream order: no synchronisation
// after pass 2.
struct compaction {
  int64_t nrows;
  geometry g;
  rmm::device_buffer mask_buf, counts_buf;
  compaction(int64_t n, hipStream_t s)
    : nrows{n},
      g{geometry_of(n)},
      mask_buf{static_cast<std::size_t>((n + 63) / 64) * sizeof(uint64_t), s, cudf::get_current_device_resource_ref()},
      counts_buf{static_cast<std::size_t>(g.nwaves + 1) * sizeof(unsigned long long), s, cudf::get_current_device_resource_ref()}
  {
  }
  [[nodiscard]] uint64_t* mask() { return static_cast<uint64_t*>(mask_buf.data()); }                          // ceil(nrows / 64) words
  [[nodiscard]] unsigned long long* counts() { return static_cast<unsigned long long*>(counts_buf.data()); }  // nwaves + 1
  // the number of set bits (the one read-back: sizes the output exactly)
  [[nodiscard]] unsigned long long total(hipStream_t s) { return scan_total(counts(), g.nwaves, s); }
  // the rows of the set bits, ascending, in exactly as many entries from `mr`
  [[nodiscard]] rmm::device_uvector<size_type> compact_indices(hipStream_t s, rmm::device_async_resource_ref mr)
  {
    auto const n = total(s);
    rmm::device_uvector<size_type> out(static_cast<std::size_t>(n), s, mr);
    if (n > 0) launch_compact_indices(mask(), counts(), g, nrows, out.data(), n, s);
    return out;
  }
};

// ------------------------------------------------------------------ validation
// as hash_join (join.cpp validate_probe; reference hash_join.cu:47-59); `who` opens the first message
inline void validate_probe(table_view const& right, table_view const& left, char const* who)
{
  CUDF_EXPECTS(0 != left.num_columns(), std::string{who} + " left table is empty", std::invalid_argument);
  CUDF_EXPECTS(right.num_columns() == left.num_columns(), "Mismatch in number of columns to be joined on", std::invalid_argument);
  CUDF_EXPECTS(same_types(right, left), "Mismatch in joining column data types", cudf::data_type_error);
}

}  // namespace cudf::detail::rowset
