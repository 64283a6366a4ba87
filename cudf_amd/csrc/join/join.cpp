// SPDX-License-Identifier: Apache-2.0
// Host side of cudf::hash_join and cudf::inner_join / left_join / full_join: the public methods, validation, trivial joins, the
// dispatch over the partitioned paths and the tables, full-join finishing and the plumbing the probes share (hash_join_impl.hpp).
// Reference counterparts: cpp/src/join/join.cu:30-118 (build on the smaller side, swap results),
// cpp/src/join/hash_join/hash_join.cu:32-59 (is_trivial_join, validate_hash_join_probe), :113-149 (ctor/build),
// retrieve_impl.cuh:169-222 (probe entry), size_impl.cuh:26-61 (size), join_utils.cu:45-221 (trivial left join,
// full-join complement), join_common_utils.hpp:25-32 (load-factor check).
#include "hash_join_impl.hpp"
#include "../common/profiler.hpp"

#include <cudf/null_mask.hpp>

#include <new>
#include <stdexcept>
#include <vector>

namespace cudf {
namespace detail {

namespace {
bool is_trivial_join(table_view const& left, table_view const& right, join_kind kind)
{
  if (left.is_empty() || right.is_empty()) return true;
  if (kind == join_kind::LEFT_JOIN && left.num_rows() == 0) return true;
  if (kind == join_kind::INNER_JOIN && (left.num_rows() == 0 || right.num_rows() == 0)) return true;
  return false;
}

// The key shape of a build table for the partitioned joins (key_layout): one key column, or two, of 4 or 8 bytes each - integers
// (timestamps, durations and decimals included) or floats, whose NORMALISED bits (-0 -> +0, one NaN: the row equality of
// common/device_table.hpp) serve as the key. Two 4-byte integer columns are packed into one 8-byte word. A build-side NULL that could
// match leaves only the open-addressing table.
key_layout classify_key(table_view const& right, bool has_nulls, null_equality compare_nulls)
{
  using form  = key_layout::form;
  key_layout k{};
  int const n = right.num_columns();
  if (n > 2 || (has_nulls && cudf::has_nulls(right) && compare_nulls == null_equality::EQUAL)) return k;
  bool words = true, int32s = true;  // every column is a key word | a 4-byte integer
  for (int c = 0; c < n; ++c) {
    auto const id      = right.column(c).type().id();
    auto const cls     = class_of(id);
    auto const w       = size_of_id(id);
    bool const integer = cls == CLS_SINT || cls == CLS_UINT;
    words  = words && (integer || cls == CLS_F32 || cls == CLS_F64) && (w == 4 || w == 8);
    int32s = int32s && integer && w == 4;
  }
  if (!words) return k;
  k.shape     = n == 1 ? form::one : int32s ? form::packed2 : form::two_words;
  k.width     = static_cast<int>(size_of_id(right.column(0).type().id()));
  k.is_signed = class_of(right.column(0).type().id()) == CLS_SINT;
  k.cls       = float_class_of(right.column(0));
  return k;
}

// n pairs written from host: {i + base, JoinNoMatch} (probe_side) or {JoinNoMatch, i + base}
join_index_pair lonely_rows(std::size_t n, int64_t base, bool probe_side, stream_ref stream, rmm::device_async_resource_ref mr)
{
  std::vector<size_type> rows(n), none(n, JoinNoMatch);
  for (std::size_t i = 0; i < n; ++i) rows[i] = static_cast<size_type>(static_cast<int64_t>(i) + base);
  auto out = alloc_pairs(n, stream.value(), mr);
  if (n) {
    CUDF_HIP_TRY(hipMemcpyAsync(out.first->data(), (probe_side ? rows : none).data(), n * sizeof(size_type), hipMemcpyHostToDevice, stream.value()));
    CUDF_HIP_TRY(hipMemcpyAsync(out.second->data(), (probe_side ? none : rows).data(), n * sizeof(size_type), hipMemcpyHostToDevice, stream.value()));
    CUDF_HIP_TRY(hipStreamSynchronize(stream.value()));
  }
  return out;
}
}  // namespace

// ---------------------------------------------------------------- shared plumbing (hash_join_impl.hpp)
join_index_pair alloc_pairs(std::size_t n, hipStream_t s, rmm::device_async_resource_ref mr)
{
  CUDF_EXPECTS(n <= static_cast<std::size_t>(std::numeric_limits<size_type>::max()),
               "Join result exceeds the maximum column size; use the *_join_size API and chunk the probe side.", std::overflow_error);
  return {std::make_unique<rmm::device_uvector<size_type>>(n, s, mr), std::make_unique<rmm::device_uvector<size_type>>(n, s, mr)};
}

join_index_pair append_unmatched(host_span<device_span<size_type const> const> lefts, host_span<device_span<size_type const> const> rights,
                                 std::size_t nr, hipStream_t s, rmm::device_async_resource_ref mr)
{
  auto tmp      = cudf::get_current_device_resource_ref();
  std::size_t P = 0;
  for (auto const& l : lefts) P += l.size();
  rmm::device_buffer matched{nr, s, tmp};
  CUDF_HIP_TRY(hipMemsetAsync(matched.data(), 0, nr, s));
  for (auto const& r : rights) join::launch_mark_matched(r.data(), r.size(), static_cast<uint8_t*>(matched.data()), s);
  // the complement goes to buffers of its own: its size is known only afterwards, and the output is allocated exactly
  rmm::device_uvector<size_type> comp_l{nr, s, tmp}, comp_r{nr, s, tmp};
  std::size_t U = 0;
  if (nr > 0) {
    dev_scalar<unsigned long long> cursor{0ull, s};
    join::launch_complement(static_cast<uint8_t const*>(matched.data()), static_cast<int64_t>(nr), cursor.ptr(), comp_l.data(), comp_r.data(), nr, s);
    U = static_cast<std::size_t>(cursor.value());  // (synchronises)
  }
  auto out       = alloc_pairs(P + U, s, mr);
  std::size_t at = 0;
  for (std::size_t i = 0; i < lefts.size(); at += lefts[i].size(), ++i) {
    if (lefts[i].empty()) continue;
    CUDF_HIP_TRY(hipMemcpyAsync(out.first->data() + at, lefts[i].data(), lefts[i].size_bytes(), hipMemcpyDeviceToDevice, s));
    CUDF_HIP_TRY(hipMemcpyAsync(out.second->data() + at, rights[i].data(), rights[i].size_bytes(), hipMemcpyDeviceToDevice, s));
  }
  if (U > 0) {
    CUDF_HIP_TRY(hipMemcpyAsync(out.first->data() + P, comp_l.data(), U * sizeof(size_type), hipMemcpyDeviceToDevice, s));
    CUDF_HIP_TRY(hipMemcpyAsync(out.second->data() + P, comp_r.data(), U * sizeof(size_type), hipMemcpyDeviceToDevice, s));
  }
  // (the given vectors and the scratch go back to the pool in stream order behind these copies)
  return out;
}

unsigned long long scan_total(unsigned long long* counts, int32_t n, hipStream_t s, int32_t const* d_flag, int32_t* h_flag)
{
  join::launch_scan(counts, n, s);
  unsigned long long total = 0;
  CUDF_HIP_TRY(hipMemcpyAsync(&total, counts + n, sizeof(total), hipMemcpyDeviceToHost, s));
  if (d_flag != nullptr) CUDF_HIP_TRY(hipMemcpyAsync(h_flag, d_flag, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  CUDF_HIP_TRY(hipStreamSynchronize(s));
  return total;
}

join_index_pair emit_staged(join::radix_join_args& e, unsigned long long total, hipStream_t s, rmm::device_async_resource_ref mr)
{
  auto out       = alloc_pairs(static_cast<std::size_t>(total), s, mr);
  e.out_probe    = out.first->data();
  e.out_build    = out.second->data();
  e.out_capacity = total;
  rmm::device_buffer d_args{sizeof(join::radix_join_args), s, cudf::get_current_device_resource_ref()};
  join::launch_radix_emit_staged(e, static_cast<join::radix_join_args*>(d_args.data()), s);
  // (no synchronisation: the scratch goes back to the pool in stream order, the caller reads the result on this stream)
  return out;
}

// ---------------------------------------------------------------- hash_join_impl: construction, dispatch
hash_join_impl::hash_join_impl(table_view const& right, bool has_nulls, null_equality compare_nulls, double load_factor, stream_ref stream,
                               rmm::device_async_resource_ref mr)
  : _right{right}, _has_nulls{has_nulls}, _nulls_equal{compare_nulls}, _mr{mr}
{
  CUDF_EXPECTS(0 != right.num_columns(), "Hash join right table is empty", std::invalid_argument);
  load_factor = checked_load_factor(load_factor);
  if (right.num_rows() == 0) return;
  _build_dev = make_device_table(right);
  // `load_factor` is the caller's upper bound (reference default 0.5). The probe is bound by random memory requests
  // and a multiset walk ends at the first empty slot: 2.5 slots at load 0.5, 1.4 at 0.25 - so the table is kept
  // at <= 0.25 unless that would take more than 1/8 of the device memory (build_classic).
  // 8-byte slots {hash tag | row}, direct windowed probe. (The sliced table with inline keys and a radix-partitioned probe side
  // of rounds 1-3 was superseded by the LDS radix join and removed in round 4.)
  _key = classify_key(right, _has_nulls, _nulls_equal);
  if (_key.shape == key_layout::form::two_words) decide_packed_words(stream);
  _classic_load = load_factor;
  // Dense build keys (one integer key column, NULLs never match, valid values within a small range): a direct-address table
  // replaces the hash table - see engine.hpp and dense_table.cpp
  if (_key.shape == key_layout::form::one && _key.cls == 0 && try_dense_build(right, stream)) return;
  // LDS radix join (engine.hpp): the build side partitioned into LDS-sized partitions; the open-addressing table in HBM is then
  // only built if a call needs it (left / full joins, match contexts, small probe sides, a probe side that overflows a region)
  if (_key.width != 0) {
    bool radix_built = false;
    try {
      radix_built = try_radix_build(right, stream);
    } catch (std::bad_alloc const&) {
      _rx_build = radix_side{};
    }
    if (radix_built) return;
  }
  build_classic(stream);
  _state = build_state::open;
}

void hash_join_impl::validate_probe(table_view const& left) const
{
  // reference validate_hash_join_probe, hash_join.cu:47-59
  CUDF_EXPECTS(0 != left.num_columns(), "Hash join left table is empty", std::invalid_argument);
  CUDF_EXPECTS(_right.num_columns() == left.num_columns(), "Mismatch in number of columns to be joined on",
               std::invalid_argument);
  CUDF_EXPECTS(_has_nulls || !cudf::has_nulls(left),
               "Left table has nulls while right table was not hashed with null check.", std::invalid_argument);
  CUDF_EXPECTS(same_types(_right, left), "Mismatch in joining column data types", cudf::data_type_error);
}

std::size_t hash_join_impl::join_size(table_view const& left, join_kind kind, stream_ref stream) const
{
  validate_probe(left);
  if (kind == join_kind::INNER_JOIN) {
    if (is_trivial_join(left, _right, kind)) return 0;
  } else {
    if (_state == build_state::empty) return left.num_rows();
    if (is_trivial_join(left, _right, kind)) return kind == join_kind::FULL_JOIN ? _right.num_rows() : 0;
  }
  if (kind == join_kind::FULL_JOIN) {
    // needs the matched set of the build side: run the real join and take its size
    auto r = probe(left, kind, std::nullopt, stream, cudf::get_current_device_resource_ref());
    return r.first->size();
  }
  if (_state == build_state::radix) {  // the radix join's count pass (partition the probe side, count per partition): nothing else is built
    std::size_t pairs = 0;
    try {
      if (radix_probe(left, stream, cudf::get_current_device_resource_ref(), 0, kind == join_kind::LEFT_JOIN, &pairs).has_value()) return pairs;
    } catch (std::bad_alloc const&) {  // (its scratch did not fit: the tables below)
    }
  }
  ensure_classic(stream);
  join_args a  = base_args(left, kind == join_kind::INNER_JOIN ? 0 : 1);
  auto scratch = count_pass(a, stream.value());
  return static_cast<std::size_t>(scan_total(a.block_counts, a.nblocks, stream.value()));
}

// Join of rows [start, end) of the context's left table; left indices refer to the complete table (reference
// partitioned_inner/left/full_join, hash_join.hpp:353-412). The full-join form emits the probe side only.
join_index_pair hash_join_impl::partitioned(join_partition_context const& ctx, join_kind kind, stream_ref stream,
                                            rmm::device_async_resource_ref mr) const
{
  CUDF_EXPECTS(ctx.left_table_context != nullptr, "join_partition_context has no match context", std::invalid_argument);
  CUDF_EXPECTS(ctx.left_table_context->_match_counts != nullptr, "join match context has no match counts",
               std::invalid_argument);
  auto const& left = ctx.left_table_context->_left_table;
  CUDF_EXPECTS(ctx.left_start_idx >= 0 && ctx.left_start_idx <= ctx.left_end_idx && ctx.left_end_idx <= left.num_rows(),
               "join partition is outside the bounds of the left table", std::invalid_argument);
  std::vector<column_view> cols;
  for (auto const& c : left) {
    size_type nulls = 0;
    if (c.nullable() && c.null_count() > 0)
      nulls = cudf::null_count(c.null_mask(), c.offset() + ctx.left_start_idx, c.offset() + ctx.left_end_idx, stream);
    cols.emplace_back(c.type(), ctx.left_end_idx - ctx.left_start_idx, c.head(), c.null_mask(), nulls,
                      c.offset() + ctx.left_start_idx);
  }
  auto const k = kind == join_kind::FULL_JOIN ? join_kind::LEFT_JOIN : kind;
  return probe(table_view{cols}, k, std::nullopt, stream, mr, ctx.left_start_idx);
}

join_index_pair hash_join_impl::probe(table_view const& left, join_kind kind, std::optional<std::size_t> output_size, stream_ref stream,
                                      rmm::device_async_resource_ref mr, int64_t row_base) const
{
  validate_probe(left);
  if (kind == join_kind::INNER_JOIN) {
    if (is_trivial_join(left, _right, kind)) return alloc_pairs(0, stream.value(), mr);
  } else {
    // right side empty: every left row pairs with JoinNoMatch (reference get_trivial_left_join_indices)
    if (_state == build_state::empty) return lonely_rows(left.num_rows(), row_base, true, stream, mr);
    if (is_trivial_join(left, _right, kind)) {
      // left side has no rows: a full join still returns every right row unmatched
      if (kind == join_kind::FULL_JOIN && !left.is_empty() && _right.num_rows() > 0) return lonely_rows(_right.num_rows(), 0, false, stream, mr);
      return alloc_pairs(0, stream.value(), mr);
    }
  }
  int const k = kind == join_kind::INNER_JOIN ? 0 : kind == join_kind::LEFT_JOIN ? 1 : 2;
  // FULL join (round 4): the LEFT join of the partitioned paths (radix partitions, dense unique table) + the build rows nobody
  // matched - marked from the left join's build indices, appended by the complement kernel of the table path (reference
  // hash_join.cu full-join complement, join_utils.cu:45-221)
  std::optional<join_index_pair> r;
  if (k == 2) {
    r = probe_partitioned_paths(left, 1, stream, cudf::get_current_device_resource_ref(), row_base);
    if (r.has_value()) {
      device_span<size_type const> const lp{*r->first}, rp{*r->second};
      r = append_unmatched({&lp, 1}, {&rp, 1}, static_cast<std::size_t>(_right.num_rows()), stream.value(), mr);
    }
  }
  if (!r.has_value()) r = probe_partitioned_paths(left, k, stream, mr, row_base);
  if (!r.has_value()) return probe_tables(left, kind, k, output_size, stream, mr, row_base);
  if (output_size.has_value())
    CUDF_EXPECTS(*output_size == r->first->size(), "hash join: output_size does not match the number of matches", std::invalid_argument);
  return std::move(*r);
}

// ---- round 3: the paths in front of the tables' count / retrieve passes (engine.hpp), in the order they are tried. nullopt: none
// of them takes this call (kind, key shape, size, a region that overflowed, no room for the scratch).
std::optional<join_index_pair> hash_join_impl::probe_partitioned_paths(table_view const& left, int k, stream_ref stream,
                                                                       rmm::device_async_resource_ref mr, int64_t row_base) const
{
  // (the partitioned joins take scratch of ~3x the probe column - regions sized for the worst case, the pair stage: when the pool
  // cannot give it, the direct passes still can run)
  auto or_nothing = [](auto&& f) -> std::optional<join_index_pair> {
    try {
      return f();
    } catch (std::bad_alloc const&) {
      return std::nullopt;
    }
  };
  // big inner and left joins on one sparse integer key: both sides in LDS-sized partitions
  if (_state == build_state::radix && (k == 0 || k == 1)) {
    if (auto r = or_nothing([&] { return radix_probe(left, stream, mr, row_base, k == 1); }); r.has_value()) return r;
  }
  // a dense unique table. CUDF_AMD_JOIN_DENSE_PROBE: 1 (default) inner joins by the ordered direct probe (pairs in probe-row
  // order), 2 by probe rows partitioned by key range (~0.6 ms less at C3, pairs partition-major), 0 neither; left joins in one pass
  int64_t dense_probe     = env_i64("CUDF_AMD_JOIN_DENSE_PROBE", -1);
  bool const dense_part   = _state == build_state::dense_part4 || _state == build_state::dense_part8;
  bool const unique_table = dense_part || _state == build_state::dense_unique;
  if (dense_probe < 0) {
    // The ordered direct probe pays one random access into the table per probe key INSIDE the table's range (a key outside is
    // rejected by the range test for free): with 30 % of C3's probe keys in range it takes 3.3 ms, with 95 % in range 9.3 ms - the
    // probe rows partitioned by key range (L2-local lookups) take 6.0 ms + the pairs partition-major (profiles/r4_c3_inrange.txt).
    // A strided sample of the probe keys decides; the table must be large enough for the partitions to matter.
    dense_probe = 1;
    if (dense_part && k == 0 && left.num_rows() >= env_i64("CUDF_AMD_JOIN_DENSE_PART_MIN_PROBE", 8 << 20)) {
      double const share = dense_inrange_share(left, stream);
      if (share > 0.55) dense_probe = 2;
    }
  }
  if (unique_table && k == 0 && dense_probe == 1) {
    if (auto r = or_nothing([&] { return dense_ordered_probe(left, stream, mr, row_base); }); r.has_value()) return r;
  }
  if (unique_table && k == 1 && dense_probe != 0) {
    if (auto r = or_nothing([&] { return dense_left_direct(left, stream, mr, row_base); }); r.has_value()) return r;
  }
  if (dense_part && k == 0 && dense_probe != 0) {
    if (auto r = or_nothing([&] { return dense_part_probe(left, stream, mr, row_base); }); r.has_value()) return r;
  }
  return std::nullopt;
}
}  // namespace detail

// ---------------------------------------------------------------- cudf::hash_join
hash_join::~hash_join() = default;

hash_join::hash_join(table_view const& right, null_equality compare_nulls, stream_ref stream,
                     rmm::device_async_resource_ref mr)
  // If we cannot know beforehand about null existence then let's assume that there are nulls (reference hash_join.cu:190-199)
  : hash_join{right, nullable_join::YES, compare_nulls, 0.5, stream, mr}
{
}

hash_join::hash_join(table_view const& right, nullable_join has_nulls, null_equality compare_nulls, double load_factor,
                     stream_ref stream, rmm::device_async_resource_ref mr)
  : _impl{[&] {
      CUDF_FUNC_RANGE();  // (reference hash_join.cu:62: the build is the constructor's work)
      return std::make_unique<detail::hash_join_impl const>(right, has_nulls == nullable_join::YES, compare_nulls, load_factor, stream, mr);
    }()}
{
}

join_index_pair hash_join::inner_join(table_view const& left, std::optional<std::size_t> output_size, stream_ref stream,
                                      rmm::device_async_resource_ref mr) const
{
  CUDF_FUNC_RANGE();
  return _impl->probe(left, join_kind::INNER_JOIN, output_size, stream, mr);
}
join_index_pair hash_join::left_join(table_view const& left, std::optional<std::size_t> output_size, stream_ref stream,
                                     rmm::device_async_resource_ref mr) const
{
  CUDF_FUNC_RANGE();
  return _impl->probe(left, join_kind::LEFT_JOIN, output_size, stream, mr);
}
join_index_pair hash_join::full_join(table_view const& left, std::optional<std::size_t> output_size, stream_ref stream,
                                     rmm::device_async_resource_ref mr) const
{
  CUDF_FUNC_RANGE();
  return _impl->probe(left, join_kind::FULL_JOIN, output_size, stream, mr);
}
std::size_t hash_join::inner_join_size(table_view const& left, stream_ref stream) const
{
  CUDF_FUNC_RANGE();
  return _impl->join_size(left, join_kind::INNER_JOIN, stream);
}
std::size_t hash_join::left_join_size(table_view const& left, stream_ref stream) const
{
  CUDF_FUNC_RANGE();
  return _impl->join_size(left, join_kind::LEFT_JOIN, stream);
}
std::size_t hash_join::full_join_size(table_view const& left, stream_ref stream, rmm::device_async_resource_ref) const
{
  CUDF_FUNC_RANGE();
  return _impl->join_size(left, join_kind::FULL_JOIN, stream);
}

join_match_context hash_join::inner_join_match_context(table_view const& left, stream_ref stream,
                                                       rmm::device_async_resource_ref mr) const
{
  CUDF_FUNC_RANGE();
  return join_match_context{left, _impl->match_counts(left, join_kind::INNER_JOIN, stream, mr)};
}
join_match_context hash_join::left_join_match_context(table_view const& left, stream_ref stream,
                                                      rmm::device_async_resource_ref mr) const
{
  CUDF_FUNC_RANGE();
  return join_match_context{left, _impl->match_counts(left, join_kind::LEFT_JOIN, stream, mr)};
}
join_match_context hash_join::full_join_match_context(table_view const& left, stream_ref stream,
                                                      rmm::device_async_resource_ref mr) const
{
  CUDF_FUNC_RANGE();
  return join_match_context{left, _impl->match_counts(left, join_kind::FULL_JOIN, stream, mr)};
}
join_index_pair hash_join::partitioned_inner_join(join_partition_context const& context, stream_ref stream,
                                                  rmm::device_async_resource_ref mr) const
{
  CUDF_FUNC_RANGE();
  return _impl->partitioned(context, join_kind::INNER_JOIN, stream, mr);
}
join_index_pair hash_join::partitioned_left_join(join_partition_context const& context, stream_ref stream,
                                                 rmm::device_async_resource_ref mr) const
{
  CUDF_FUNC_RANGE();
  return _impl->partitioned(context, join_kind::LEFT_JOIN, stream, mr);
}
join_index_pair hash_join::partitioned_full_join(join_partition_context const& context, stream_ref stream,
                                                 rmm::device_async_resource_ref mr) const
{
  CUDF_FUNC_RANGE();
  return _impl->partitioned(context, join_kind::FULL_JOIN, stream, mr);
}
// Concatenates the partial probe-side results and appends (JoinNoMatch, r) for every right row r that no partial
// matched (reference hash_join.hpp:414-441, join_utils.cu:45-221).
join_index_pair hash_join::finalize_partitioned_full_join(
  cudf::host_span<cudf::device_span<size_type const> const> left_partials,
  cudf::host_span<cudf::device_span<size_type const> const> right_partials, size_type left_table_num_rows,
  size_type right_table_num_rows, stream_ref stream, rmm::device_async_resource_ref mr)
{
  CUDF_FUNC_RANGE();
  CUDF_EXPECTS(left_partials.size() == right_partials.size(), "left and right partial results differ in number",
               std::invalid_argument);
  CUDF_EXPECTS(left_table_num_rows >= 0 && right_table_num_rows >= 0, "negative table size", std::invalid_argument);
  std::size_t probe_pairs = 0;
  for (std::size_t i = 0; i < left_partials.size(); ++i) {
    CUDF_EXPECTS(left_partials[i].size() == right_partials[i].size(), "partial index vectors differ in size",
                 std::invalid_argument);
    probe_pairs += left_partials[i].size();
  }
  CUDF_EXPECTS(probe_pairs + static_cast<std::size_t>(right_table_num_rows) <= static_cast<std::size_t>(std::numeric_limits<size_type>::max()),
               "Join result exceeds the maximum column size", std::overflow_error);
  auto out = detail::append_unmatched(left_partials, right_partials, static_cast<std::size_t>(right_table_num_rows), stream.value(), mr);
  CUDF_HIP_TRY(hipStreamSynchronize(stream.value()));
  return out;
}


// ---------------------------------------------------------------- free functions
join_index_pair inner_join(table_view const& left, table_view const& right, null_equality compare_nulls, stream_ref stream,
                           rmm::device_async_resource_ref mr)
{
  CUDF_FUNC_RANGE();
  auto const has_nulls = (cudf::has_nulls(left) || cudf::has_nulls(right)) ? nullable_join::YES : nullable_join::NO;
  // build on the smaller table; ties build on right (reference join.cu:50-57)
  if (right.num_rows() > left.num_rows()) {
    hash_join hj{left, has_nulls, compare_nulls, 0.5, stream};
    auto [right_result, left_result] = hj.inner_join(right, std::nullopt, stream, mr);
    return {std::move(left_result), std::move(right_result)};
  }
  hash_join hj{right, has_nulls, compare_nulls, 0.5, stream};
  return hj.inner_join(left, std::nullopt, stream, mr);
}

join_index_pair left_join(table_view const& left, table_view const& right, null_equality compare_nulls, stream_ref stream,
                          rmm::device_async_resource_ref mr)
{
  CUDF_FUNC_RANGE();
  auto const has_nulls = (cudf::has_nulls(left) || cudf::has_nulls(right)) ? nullable_join::YES : nullable_join::NO;
  hash_join hj{right, has_nulls, compare_nulls, 0.5, stream};
  return hj.left_join(left, std::nullopt, stream, mr);
}

join_index_pair full_join(table_view const& left, table_view const& right, null_equality compare_nulls, stream_ref stream,
                          rmm::device_async_resource_ref mr)
{
  CUDF_FUNC_RANGE();
  auto const has_nulls = (cudf::has_nulls(left) || cudf::has_nulls(right)) ? nullable_join::YES : nullable_join::NO;
  hash_join hj{right, has_nulls, compare_nulls, 0.5, stream};
  return hj.full_join(left, std::nullopt, stream, mr);
}
}  // namespace cudf
