// SPDX-License-Identifier: Apache-2.0
// Host side of cudf::hash_join, private to the join: the build state, the key layout and the shared plumbing of the probes.
// The class is defined over four files, one per concern:
//   join.cpp        public hash_join methods, free functions, validation, trivial joins, the dispatch (probe,
//                   probe_partitioned_paths), full-join finishing, the shared helpers declared below
//   dense_table.cpp the dense direct-address table: the decision from the build keys' min / max, the partitioned and atomic builds,
//                   row lists (CSR), the in-range sample, the ordered, left-direct and partitioned probes
//   radix_join.cpp  the LDS radix join: packing two key words, partitioning, the build and the probe
//   open_table.cpp  the open-addressing table in HBM: build, count pass, retrieve and complement, match counts
#pragma once
#include "engine.hpp"
#include "../common/env.hpp"

#include <cudf/join/hash_join.hpp>
#include <cudf/join/join.hpp>
#include <cudf/utilities/error.hpp>

#include <mutex>
#include <optional>
#include <stdexcept>

namespace cudf::detail {

using join::join_args;

template <typename T>
struct dev_scalar {  // one T in device memory, stream ordered
  rmm::device_buffer buf;
  hipStream_t s;
  dev_scalar(T init, hipStream_t stream) : buf{sizeof(T), stream, cudf::get_current_device_resource_ref()}, s{stream}
  {
    static_assert(sizeof(T) <= 8);
    T host = init;
    CUDF_HIP_TRY(hipMemcpyAsync(buf.data(), &host, sizeof(T), hipMemcpyHostToDevice, s));
    CUDF_HIP_TRY(hipStreamSynchronize(s));
  }
  T* ptr() { return static_cast<T*>(buf.data()); }
  T value()
  {
    T host{};
    CUDF_HIP_TRY(hipMemcpyAsync(&host, buf.data(), sizeof(T), hipMemcpyDeviceToHost, s));
    CUDF_HIP_TRY(hipStreamSynchronize(s));
    return host;
  }
};

// reference join_common_utils.hpp:25-32 (hash_join, filtered_join)
inline double checked_load_factor(double load_factor)
{
  CUDF_EXPECTS(load_factor > 0, "Invalid load factor: must be greater than 0.", std::invalid_argument);
  CUDF_EXPECTS(load_factor <= 1, "Invalid load factor: must be less than or equal to 1.", std::invalid_argument);
  return load_factor;
}
inline bool same_types(table_view const& a, table_view const& b)
{
  if (a.num_columns() != b.num_columns()) return false;
  for (size_type i = 0; i < a.num_columns(); ++i)
    if (a.column(i).type() != b.column(i).type()) return false;
  return true;
}
inline int32_t float_class_of(column_view const& c)
{
  auto const cls = class_of(c.type().id());
  return (cls == CLS_F32 || cls == CLS_F64) ? static_cast<int32_t>(cls) : 0;
}
inline int ceil_log2(uint64_t v)
{
  int l = 0;
  while ((uint64_t{1} << l) < v) ++l;
  return l;
}
inline uint64_t const* key_bytes(column_view const& c, int width)
{
  return reinterpret_cast<uint64_t const*>(c.head<uint8_t>() + static_cast<std::size_t>(c.offset()) * static_cast<std::size_t>(width));
}

// two index vectors of n entries; n beyond a column's size throws
join_index_pair alloc_pairs(std::size_t n, hipStream_t s, rmm::device_async_resource_ref mr);
// the given pairs, in order, then {JoinNoMatch, r} for every build row r < nr that none of them names (full joins)
join_index_pair append_unmatched(host_span<device_span<size_type const> const> lefts, host_span<device_span<size_type const> const> rights,
                                 std::size_t nr, hipStream_t s, rmm::device_async_resource_ref mr);
// exclusive scan of counts[0, n) in place; returns counts[n] (and *h_flag = *d_flag when given), read back in one synchronisation
unsigned long long scan_total(unsigned long long* counts, int32_t n, hipStream_t s, int32_t const* d_flag = nullptr, int32_t* h_flag = nullptr);
// the staged pairs of e (pair_counts scanned by scan_total) copied into `total` exact pairs; e.out_* point at them afterwards
join_index_pair emit_staged(join::radix_join_args& e, unsigned long long total, hipStream_t s, rmm::device_async_resource_ref mr);

struct second_key {  // the second key column: of two packed 4-byte columns (radix_scatter_args::keys2) or of a two-word key (key2)
  int32_t width{0}, cls{0};  // two-word keys
  int32_t is_signed{0};
  uint32_t const* keys{nullptr};
  bitmask_type const* mask{nullptr};
  int64_t mask_offset{0};
};

// The build table's key as the partitioned joins take it, classified once by the constructor. The probe side needs no test of
// its own: validate_probe gives it the build side's column count and types.
struct key_layout {
  enum class form : int8_t {
    none,       // only the open-addressing table takes these keys (or a build-side NULL could match)
    one,        // one integer column of 4 / 8 bytes (4-byte keys are widened by the first scatter level), or a float column (radix join)
    packed2,    // two 4-byte integer columns, packed into the radix join's 8-byte key
    two_words,  // two columns of 4 / 8 bytes each, any class: a two-word radix key
  };
  form shape{form::none};
  int width{0};           // bytes of the (first) key column; 4 for packed2; 0: form::none
  bool is_signed{false};  // the (first) column is a signed integer
  int32_t cls{0};         // CLS_F32 / CLS_F64: the (first) column is a float whose normalised bits are the key; 0: integer
  // two_words only: the build-side ranges of two integer columns fit 63 bits - the single-word join serves them (engine.hpp
  // radix_scatter_args::pack)
  bool packed{false};
  uint64_t lo[2]{0, 0}, range[2]{0, 0};
  int bits1{0};
  [[nodiscard]] bool two_columns() const { return shape == form::packed2 || shape == form::two_words; }
  [[nodiscard]] bool two_words() const { return shape == form::two_words && !packed; }
};

// What the constructor built. The open-addressing table of the lazy states is built on first need (ensure_classic).
enum class build_state : int8_t {
  empty,         // no build rows
  open,          // the open-addressing table, built by the constructor
  radix,         // LDS radix partitions; the open table lazily
  dense_part4,   // dense unique table of a 4-byte key, partitioned build; the open table lazily
  dense_part8,   // dense unique table of an 8-byte key, partitioned build; the table passes use the dense head
  dense_unique,  // dense unique table of an 8-byte key, atomic build
  dense_csr,     // dense table of an 8-byte key with row lists: some key repeats
};

class hash_join_impl {
 public:
  hash_join_impl(table_view const& right, bool has_nulls, null_equality compare_nulls, double load_factor, stream_ref stream,
                 rmm::device_async_resource_ref mr);
  [[nodiscard]] std::size_t join_size(table_view const& left, join_kind kind, stream_ref stream) const;
  // Per-left-row match counts (reference inner/left/full_join_match_context, hash_join.hpp:276-329).
  [[nodiscard]] std::unique_ptr<rmm::device_uvector<size_type>> match_counts(table_view const& left, join_kind kind, stream_ref stream,
                                                                             rmm::device_async_resource_ref mr) const;
  [[nodiscard]] join_index_pair partitioned(join_partition_context const& ctx, join_kind kind, stream_ref stream,
                                            rmm::device_async_resource_ref mr) const;
  [[nodiscard]] join_index_pair probe(table_view const& left, join_kind kind, std::optional<std::size_t> output_size, stream_ref stream,
                                      rmm::device_async_resource_ref mr, int64_t row_base = 0) const;

 private:
  // ---- join.cpp
  void validate_probe(table_view const& left) const;
  std::optional<join_index_pair> probe_partitioned_paths(table_view const& left, int k, stream_ref stream, rmm::device_async_resource_ref mr,
                                                         int64_t row_base) const;

  // ---- dense_table.cpp
  struct dense_side {
    rmm::device_buffer recs, counts, ovf;
    int64_t cap{0};
    int32_t P{0}, S{0}, P_used{0};
  };
  bool key_minmax(int ncols, uint64_t* h, rmm::device_buffer& d_args, hipStream_t s) const;
  bool try_dense_build(table_view const& right, stream_ref stream);
  bool try_dense_part_build(table_view const& right, stream_ref stream);
  void dense_partition(uint64_t const* keys, bitmask_type const* mask, int64_t mask_offset, int64_t nrows, dense_side& out, stream_ref stream) const;
  join::dense_part_args dense_part_args_of(dense_side const& side) const;
  join::dense_stage_args dense_stage_of(table_view const& left, int64_t row_base) const;
  [[nodiscard]] double dense_inrange_share(table_view const& left, stream_ref stream) const;
  std::optional<join_index_pair> dense_ordered_probe(table_view const& left, stream_ref stream, rmm::device_async_resource_ref mr, int64_t row_base) const;
  std::optional<join_index_pair> dense_left_direct(table_view const& left, stream_ref stream, rmm::device_async_resource_ref mr, int64_t row_base) const;
  std::optional<join_index_pair> dense_part_probe(table_view const& left, stream_ref stream, rmm::device_async_resource_ref mr, int64_t row_base) const;

  // ---- radix_join.cpp
  struct radix_side {
    rmm::device_buffer key1, row1, cnt1, key2, row2, cnt2;
    rmm::device_buffer key1w, key2w;  // two-word keys: the second word of level 1 / level 2
    int64_t cap2{0};
    int32_t slices2{0};
  };
  static constexpr int32_t RADIX_TABLE_SLOTS = 8192, RADIX_FILL_LIMIT = 5200;
  void decide_packed_words(stream_ref stream);
  second_key second_of(table_view const& t) const;
  bool radix_partition(uint64_t const* keys, bitmask_type const* mask, int64_t mask_offset, int64_t nrows, int64_t valid_rows, radix_side& out,
                       stream_ref stream, rmm::device_async_resource_ref mr2, second_key k2, bool keep_outside = false) const;
  bool try_radix_build(table_view const& right, stream_ref stream);
  std::optional<join_index_pair> radix_probe(table_view const& left, stream_ref stream, rmm::device_async_resource_ref mr, int64_t row_base,
                                             bool left_join = false, std::size_t* size_only = nullptr) const;

  // ---- open_table.cpp
  struct count_scratch {
    rmm::device_buffer counts, cache, d_args;
  };
  join_args base_args(table_view const& probe, int kind) const;
  void build_classic(stream_ref stream) const;
  void ensure_classic(stream_ref stream) const;
  count_scratch count_pass(join_args& a, hipStream_t s) const;
  [[nodiscard]] join_index_pair probe_tables(table_view const& left, join_kind kind, int k, std::optional<std::size_t> output_size,
                                             stream_ref stream, rmm::device_async_resource_ref mr, int64_t row_base) const;

  table_view _right;
  bool _has_nulls;
  null_equality _nulls_equal;
  rmm::device_async_resource_ref _mr;
  device_table _build_dev{};
  key_layout _key{};
  build_state _state{build_state::empty};
  double _classic_load{0.5};
  // the open-addressing table in HBM: built by the constructor (build_state::open), or on first need in the lazy states
  mutable std::mutex _classic_mu;
  mutable uint64_t _capacity{0};  // 0: not built
  mutable rmm::device_buffer _table{};
  // LDS radix join: the build side in LDS-sized partitions
  int32_t _rx_nparts{0};
  radix_side _rx_build{};
  // the dense direct-address table over [_dense_lo, _dense_lo + _dense_range)
  uint64_t _dense_lo{0}, _dense_range{0};
  rmm::device_buffer _dense_head{}, _dense_next{};
};

}  // namespace cudf::detail
