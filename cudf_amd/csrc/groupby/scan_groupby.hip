// SPDX-License-Identifier: Apache-2.0
// groupby::scan and groupby::replace_nulls on the sort-based groupby (reference cpp/src/groupby/groupby.cu scan / replace_nulls,
// sort/scan.cpp, group_scan_util.cuh, group_rank_scan.cu, group_replace_nulls.cu). The rows are put in group order by the sort
// helper (sort_helper.hpp) and every scan kind is answered by the segmented inclusive scan core (segmented_scan.hpp). One pass
// serves all the scan kinds of a request (up to SG_KINDS at a time): each grouped value is read once and one result per kind is
// written. The values are gathered into group order once per request, and not at all when the key order is the identity.
// RANK scans run-start / run-end / valid words of the (label, value) order with the same core and scatter the ranks back into
// group order; replace_nulls scans the position of the last valid row, forward (PRECEDING) or backward (FOLLOWING), and gathers.
#include "sort_helper.hpp"
#include "segmented_scan.hpp"
#include "../common/profiler.hpp"

#include <cudf/copying.hpp>
#include <cudf/groupby.hpp>
#include <cudf/null_mask.hpp>
#include <cudf/utilities/error.hpp>

#include <hip/hip_runtime.h>

#include <algorithm>

namespace cudf::groupby::detail {
namespace {
using cudf::detail::CLS_F32;
using cudf::detail::CLS_F64;
using cudf::detail::CLS_NONE;
using cudf::detail::col_is_valid;
using cudf::detail::col_load_bits;
using cudf::detail::device_column;
using cudf::detail::gload;
using cudf::detail::gstore;
namespace prof = cudf::detail::prof;

// bits[i] = the value of row order[i] (order == nullptr: row i), when bits != nullptr; mask bit i = its validity, when mask != nullptr
__global__ void __launch_bounds__(256) k_group_values(device_column col, uint32_t const* order, int64_t nk, uint64_t* bits,
                                                      bitmask_type* mask, int32_t* null_count)
{
  int64_t const e = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  bool valid      = false;
  if (e < nk) {
    uint32_t const row = order ? gload(order + e) : static_cast<uint32_t>(e);
    if (bits) gstore(bits + e, col_load_bits(col, row));
    valid = col_is_valid(col, row);
  }
  if (mask != nullptr) store_wave_validity(valid, e, nk, mask, null_count);
}

// RANK: per position p of the (label, value) order, bit 0 = p starts a run of equal values (nulls equal nulls) inside its group,
// bit 1 = p ends one, bit 2 = the value is valid
__global__ void __launch_bounds__(256) k_rank_words(device_column col, uint32_t const* vrow, int32_t const* labels, int32_t const* offsets,
                                                    int64_t nk, uint64_t* words)
{
  int64_t const p = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (p >= nk) return;
  int32_t const g    = gload(labels + p);
  uint32_t const row = gload(vrow + p);
  bool const valid   = col_is_valid(col, row);
  bool const starts  = p == gload(offsets + g) || !same_value(col, row, valid, gload(vrow + p - 1));
  bool const ends    = p + 1 == gload(offsets + g + 1) || !same_value(col, row, valid, gload(vrow + p + 1));
  gstore(words + p, static_cast<uint64_t>(starts) | (static_cast<uint64_t>(ends) << 1) | (static_cast<uint64_t>(valid) << 2));
}

// pos[order[q]] = q: the group-order position of a row
__global__ void __launch_bounds__(256) k_positions(uint32_t const* order, int64_t nk, int32_t* pos)
{
  int64_t const q = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (q < nk) gstore(pos + gload(order + q), static_cast<int32_t>(q));
}

struct rank_args {
  uint32_t const* vrow;        // value-order position -> row
  int32_t const* pos;          // row -> group-order position
  int32_t const* labels;
  int32_t const* offsets;
  uint64_t const* starts;      // forward MAX scan of (run start + 1): p's run starts at starts[p] - 1
  uint64_t const* ends;        // backward MAX scan of (nk - run end): p's run ends at nk - ends[p]
  uint64_t const* dense;       // forward SUM scan of run starts
  uint64_t const* valid_runs;  // forward SUM scan of valid values (nullptr: count every row)
  int64_t nk;
  int32_t method;
  int32_t percentage;
  void* out;                   // INT32, or FLOAT64 for AVERAGE and every percentage
};

// the rank of every position of the value order, written to its row's group-order position
// (reference group_rank_scan.cu: min/max/first/average/dense rank scans and group_rank_to_percentage)
__global__ void __launch_bounds__(256) k_rank_finish(rank_args a)
{
  int64_t const p = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (p >= a.nk) return;
  int32_t const g   = gload(a.labels + p);
  int64_t const gs  = gload(a.offsets + g);
  int64_t const ge  = gload(a.offsets + g + 1);
  auto const rmin   = [&] { return static_cast<int64_t>(gload(a.starts + p)) - gs; };
  auto const rmax   = [&] { return a.nk - static_cast<int64_t>(gload(a.ends + p)) - gs + 1; };
  double r          = 0.0;
  int32_t ri        = 0;
  switch (static_cast<rank_method>(a.method)) {
    case rank_method::FIRST: ri = static_cast<int32_t>(p - gs + 1); break;
    case rank_method::MIN: ri = static_cast<int32_t>(rmin()); break;
    case rank_method::MAX: ri = static_cast<int32_t>(rmax()); break;
    case rank_method::DENSE: ri = static_cast<int32_t>(gload(a.dense + p)); break;
    default: {
      int32_t const lo = static_cast<int32_t>(rmin()), hi = static_cast<int32_t>(rmax());
      r                = lo + (hi - lo) / 2.0;
    }
  }
  if (static_cast<rank_method>(a.method) != rank_method::AVERAGE) r = ri;
  int64_t const q = gload(a.pos + gload(a.vrow + p));
  if (a.percentage == static_cast<int32_t>(rank_percentage::NONE)) {
    if (static_cast<rank_method>(a.method) == rank_method::AVERAGE) gstore(static_cast<double*>(a.out) + q, r);
    else gstore(static_cast<int32_t*>(a.out) + q, ri);
    return;
  }
  int32_t const count = a.valid_runs ? static_cast<int32_t>(gload(a.valid_runs + ge - 1)) : static_cast<int32_t>(ge - gs);
  bool const zero     = a.percentage == static_cast<int32_t>(rank_percentage::ZERO_NORMALIZED);
  double result;
  if (static_cast<rank_method>(a.method) == rank_method::DENSE) {
    // the dense rank at position (group start + count - 1) of the value order (group_rank_scan.cu:280-291)
    int64_t const last_index = gs + count - 1;
    int32_t const last       = last_index < 0 ? 1 : static_cast<int32_t>(gload(a.dense + last_index));
    result                   = zero ? r / last : (last == 1 ? 0.0 : (r - 1.0) / (last - 1));
  } else {
    result = zero ? r / count : (count == 1 ? 0.0 : (r - 1.0) / (count - 1));
  }
  gstore(static_cast<double*>(a.out) + q, result);
}

// replace_nulls: out[p] = the value at the position the scan found (state - 1 forward, n - state backward), null if none
__global__ void __launch_bounds__(256) k_replace_finish(device_column col, uint32_t const* order, uint64_t const* state, int64_t n,
                                                        bool backward, void* out, bitmask_type* mask, int32_t* null_count)
{
  int64_t const e = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  bool valid      = false;
  if (e < n) {
    uint64_t const st = gload(state + e);
    valid             = st != 0;
    uint64_t v        = 0;
    if (valid) {
      int64_t const q    = backward ? n - static_cast<int64_t>(st) : static_cast<int64_t>(st) - 1;
      uint32_t const row = order ? gload(order + q) : static_cast<uint32_t>(q);
      v                  = col_load_bits(col, row);
    }
    store_width(out, e, col.width, v);
  }
  store_wave_validity(valid, e, n, mask, null_count);
}

// ---------------------------------------------------------------------------------------------------------
// host side

bool scan_kind_ok(aggregation::Kind k)
{
  return k == aggregation::SUM || k == aggregation::PRODUCT || k == aggregation::MIN || k == aggregation::MAX ||
         k == aggregation::COUNT_VALID || k == aggregation::COUNT_ALL || k == aggregation::RANK;
}

// result type of a scan kind over `source` (EMPTY: not supported; reference group_scan_util.cuh is_group_scan_supported)
data_type scan_type(data_type source, aggregation const& a)
{
  auto const invalid = data_type{type_id::EMPTY};
  if (cudf::detail::class_of(source.id()) == CLS_NONE) return invalid;
  switch (a.kind) {
    case aggregation::COUNT_VALID:
    case aggregation::COUNT_ALL: return data_type{type_id::INT32};
    case aggregation::RANK: {
      auto const& r = dynamic_cast<cudf::detail::rank_aggregation const&>(a);
      bool const fp = r._method == rank_method::AVERAGE || r._percentage != rank_percentage::NONE;
      return data_type{fp ? type_id::FLOAT64 : type_id::INT32};
    }
    default: return cudf::detail::target_type(source, a.kind);  // SUM, PRODUCT, MIN, MAX
  }
}

// the request's grouped values: bits (nullptr when the key order is the identity) and the mask (nullptr when not nullable)
struct grouped_values {
  uint64_t* bits{nullptr};
  bitmask_type* mask{nullptr};
  rmm::device_buffer mask_buf{};
  int32_t null_count{0};
};

grouped_values group_values(helper const& h, column_view const& values, bool want_bits, scratch& tmp, hipStream_t s)
{
  grouped_values g;
  bool const need_bits = want_bits && !h.identity_order;
  if (values.nullable()) {
    g.mask_buf = rmm::device_buffer{bitmask_allocation_size_bytes(static_cast<size_type>(h.nk)), s, get_current_device_resource_ref()};
    g.mask     = static_cast<bitmask_type*>(g.mask_buf.data());
  }
  if (!need_bits && g.mask == nullptr) return g;
  if (need_bits) g.bits = tmp.alloc<uint64_t>(static_cast<std::size_t>(h.nk));
  auto* d_nulls = tmp.alloc<int32_t>(1);
  CUDF_HIP_TRY(hipMemsetAsync(d_nulls, 0, sizeof(int32_t), s));
  {
    prof::scope p_{"scan_gather", s};
    hipLaunchKernelGGL(k_group_values, dim3(blocks_of(h.nk)), dim3(256), 0, s, cudf::detail::make_device_column(values),
                       h.identity_order ? nullptr : h.order, h.nk, g.bits, g.mask, d_nulls);
  }
  CUDF_HIP_TRY(hipGetLastError());
  if (g.mask) {
    CUDF_HIP_TRY(hipMemcpyAsync(&g.null_count, d_nulls, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    CUDF_HIP_TRY(hipStreamSynchronize(s));
  }
  return g;
}

rmm::device_buffer copy_mask(grouped_values const& g, int64_t nk, hipStream_t s, rmm::device_async_resource_ref mr)
{
  if (g.mask == nullptr) return rmm::device_buffer{};
  return rmm::device_buffer{g.mask, bitmask_allocation_size_bytes(static_cast<size_type>(nk)), s, mr};
}

scan_src make_src(helper const& h, column_view const& values, grouped_values const& g)
{
  scan_src src{};
  src.col         = cudf::detail::make_device_column(values);
  src.bits        = g.bits;
  src.valid       = g.mask;
  src.labels      = h.labels;
  src.n           = h.nk;
  src.read_values = 1;
  return src;
}

// one RANK result (reference sort/scan.cpp:137-210)
std::unique_ptr<column> rank_scan(helper& h, column_view const& values, cudf::detail::rank_aggregation const& r, bool presorted,
                                  grouped_values const& g, hipStream_t s, rmm::device_async_resource_ref mr)
{
  int64_t const nk = h.nk;
  scratch tmp{s, get_current_device_resource_ref(), {}};
  bool const descending  = r._column_order == order::DESCENDING;
  bool const nulls_first = (r._null_precedence == null_order::BEFORE) != descending;
  // pre-sorted keys: the values are taken as ordered inside their groups already (as the reference does for Spark)
  uint32_t const* vrow = presorted ? h.order : h.value_order(values, descending, nulls_first);
  auto* words          = tmp.alloc<uint64_t>(static_cast<std::size_t>(nk));
  auto* pos            = tmp.alloc<int32_t>(static_cast<std::size_t>(h.n));
  auto const dcol      = cudf::detail::make_device_column(values);
  {
    prof::scope p_{"scan_rank_words", s};
    hipLaunchKernelGGL(k_rank_words, dim3(blocks_of(nk)), dim3(256), 0, s, dcol, vrow, h.labels, h.offsets, nk, words);
    hipLaunchKernelGGL(k_positions, dim3(blocks_of(nk)), dim3(256), 0, s, h.order, nk, pos);
  }
  CUDF_HIP_TRY(hipGetLastError());
  bool const needs_min   = r._method == rank_method::MIN || r._method == rank_method::AVERAGE;
  bool const needs_max   = r._method == rank_method::MAX || r._method == rank_method::AVERAGE;
  bool const needs_dense = r._method == rank_method::DENSE;
  bool const count_valid = r._percentage != rank_percentage::NONE && values.nullable() && r._null_handling == null_policy::EXCLUDE;
  rank_args a{};
  scan_src fwd{};
  fwd.bits        = words;
  fwd.labels      = h.labels;
  fwd.n           = nk;
  fwd.read_values = 1;
  auto add_kind   = [&](scan_src& src, int32_t op, int32_t lift) {
    auto* out = tmp.alloc<uint64_t>(static_cast<std::size_t>(nk));
    src.kind[src.nkinds++] = scan_kind{op, lift, 8, out};
    return static_cast<uint64_t const*>(out);
  };
  if (needs_min) a.starts = add_kind(fwd, OP_MAX_U, LIFT_BIT0_POS);
  if (needs_dense) a.dense = add_kind(fwd, OP_ADD_I, LIFT_BIT0);
  if (count_valid) a.valid_runs = add_kind(fwd, OP_ADD_I, LIFT_BIT2);
  segmented_scan(fwd, s);
  if (needs_max) {
    scan_src bwd  = fwd;
    bwd.nkinds    = 0;
    bwd.backward  = 1;
    a.ends        = add_kind(bwd, OP_MAX_U, LIFT_BIT1_POS);
    segmented_scan(bwd, s);
  }
  bool const fp = r._method == rank_method::AVERAGE || r._percentage != rank_percentage::NONE;
  auto const type = data_type{fp ? type_id::FLOAT64 : type_id::INT32};
  auto out        = std::make_unique<column>(type, static_cast<size_type>(nk),
                                      rmm::device_buffer{static_cast<std::size_t>(nk) * size_of(type), s, mr},
                                      r._null_handling == null_policy::EXCLUDE ? copy_mask(g, nk, s, mr) : rmm::device_buffer{},
                                      r._null_handling == null_policy::EXCLUDE ? g.null_count : 0);
  a.vrow       = vrow;
  a.pos        = pos;
  a.labels     = h.labels;
  a.offsets    = h.offsets;
  a.nk         = nk;
  a.method     = static_cast<int32_t>(r._method);
  a.percentage = static_cast<int32_t>(r._percentage);
  a.out        = out->mutable_view().head();
  {
    prof::scope p_{"scan_rank_finish", s};
    hipLaunchKernelGGL(k_rank_finish, dim3(blocks_of(nk)), dim3(256), 0, s, a);
  }
  CUDF_HIP_TRY(hipGetLastError());
  CUDF_HIP_TRY(hipStreamSynchronize(s));  // the temporaries above go with tmp
  return out;
}

std::unique_ptr<table> keys_in_group_order(helper const& h, stream_ref stream, rmm::device_async_resource_ref mr)
{
  column_view const order_view{data_type{type_id::INT32}, static_cast<size_type>(h.nk), h.order, nullptr, 0};
  return cudf::gather(h.keys, order_view, out_of_bounds_policy::DONT_CHECK, stream, mr);
}
}  // namespace

}  // namespace cudf::groupby::detail

namespace cudf::groupby {

std::pair<std::unique_ptr<table>, std::vector<aggregation_result>> groupby::scan(std::span<scan_request const> requests, stream_ref stream,
                                                                                 rmm::device_async_resource_ref mr)
{
  CUDF_FUNC_RANGE();
  using namespace detail;
  // reference groupby.cu:245-251, sort/scan.cpp:48, group_scan_util.cuh:42
  CUDF_EXPECTS(std::all_of(requests.begin(), requests.end(), [this](auto const& r) { return r.values.size() == _keys.num_rows(); }),
               "Size mismatch between request values and groupby keys.");
  for (auto const& r : requests)
    for (auto const& a : r.aggregations) {
      if (!scan_kind_ok(a->kind)) CUDF_FAIL("Unsupported groupby scan aggregation");
      if (scan_type(r.values.type(), *a).id() == type_id::EMPTY) CUDF_FAIL("Unsupported groupby scan type-agg combination.");
    }
  CUDF_EXPECTS(_keys.num_columns() > 0, "The sort-based groupby needs at least one key column.");
  hipStream_t const s = stream.value();
  auto const empty    = [&] {
    std::vector<aggregation_result> res(requests.size());
    for (std::size_t i = 0; i < requests.size(); ++i)
      for (auto const& a : requests[i].aggregations) res[i].results.push_back(make_empty_column(scan_type(requests[i].values.type(), *a)));
    return std::pair{empty_like(_keys), std::move(res)};
  };
  if (_keys.num_rows() == 0) return empty();
  bool const presorted = _keys_are_sorted == sorted::YES;
  helper h{_keys, s};
  h.build(_include_null_keys == null_policy::EXCLUDE, presorted);
  if (h.nk == 0) return empty();
  int64_t const nk = h.nk;

  std::vector<aggregation_result> results(requests.size());
  for (std::size_t ri = 0; ri < requests.size(); ++ri) {
    auto const& req    = requests[ri];
    auto const& values = req.values;
    auto& out          = results[ri].results;
    out.resize(req.aggregations.size());
    bool const any_value_kind = std::any_of(req.aggregations.begin(), req.aggregations.end(), [](auto const& a) {
      return a->kind != aggregation::COUNT_ALL && a->kind != aggregation::COUNT_VALID && a->kind != aggregation::RANK;
    });
    scratch tmp{s, get_current_device_resource_ref(), {}};
    auto g   = group_values(h, values, any_value_kind, tmp, s);
    auto src        = make_src(h, values, g);
    src.read_values = any_value_kind ? 1 : 0;
    // the scan kinds, SG_KINDS at a time
    auto flush = [&] {
      segmented_scan(src, s);
      src.nkinds = 0;
    };
    for (std::size_t j = 0; j < req.aggregations.size(); ++j) {
      auto const& a = *req.aggregations[j];
      if (a.kind == aggregation::RANK) continue;
      auto const type  = scan_type(values.type(), a);
      auto const cls   = cudf::detail::class_of(values.type().id());
      bool const fp32  = cls == CLS_F32, fp64 = cls == CLS_F64;
      scan_kind k{};
      k.width = static_cast<int32_t>(size_of(type));
      switch (a.kind) {
        case aggregation::SUM:
          k.op   = fp32 ? OP_ADD_F32 : fp64 ? OP_ADD_F64 : OP_ADD_I;
          k.lift = (fp32 || fp64) ? LIFT_BITS : LIFT_INT;
          break;
        case aggregation::PRODUCT:
          k.op   = fp32 ? OP_MUL_F32 : fp64 ? OP_MUL_F64 : OP_MUL_I;
          k.lift = (fp32 || fp64) ? LIFT_BITS : LIFT_INT;
          break;
        case aggregation::MIN:
        case aggregation::MAX:
          k.op   = a.kind == aggregation::MIN ? OP_MIN_U : OP_MAX_U;
          k.lift = LIFT_ORDERED;
          break;
        default:  // COUNT_VALID, COUNT_ALL
          k.op   = OP_ADD_I;
          k.lift = a.kind == aggregation::COUNT_ALL ? LIFT_ONE : LIFT_VALID;
      }
      bool const counts = a.kind == aggregation::COUNT_ALL || a.kind == aggregation::COUNT_VALID;
      auto col = std::make_unique<column>(type, static_cast<size_type>(nk), rmm::device_buffer{static_cast<std::size_t>(nk) * size_of(type), s, mr},
                                          counts ? rmm::device_buffer{} : copy_mask(g, nk, s, mr), counts ? 0 : g.null_count);
      k.out                     = col->mutable_view().head();
      out[j]                    = std::move(col);
      src.kind[src.nkinds++]    = k;
      if (src.nkinds == SG_KINDS) flush();
    }
    if (src.nkinds > 0) flush();
    for (std::size_t j = 0; j < req.aggregations.size(); ++j) {
      auto const& a = *req.aggregations[j];
      if (a.kind != aggregation::RANK) continue;
      out[j] = rank_scan(h, values, dynamic_cast<cudf::detail::rank_aggregation const&>(a), presorted, g, s, mr);
    }
    CUDF_HIP_TRY(hipStreamSynchronize(s));  // tmp's buffers are released when the request is done
  }
  return {keys_in_group_order(h, stream, mr), std::move(results)};
}

std::pair<std::unique_ptr<table>, std::unique_ptr<table>> groupby::replace_nulls(table_view const& values,
                                                                                 std::span<replace_policy const> replace_policies,
                                                                                 stream_ref stream, rmm::device_async_resource_ref mr)
{
  CUDF_FUNC_RANGE();
  using namespace detail;
  // reference groupby.cu:291-296
  CUDF_EXPECTS(_keys.num_rows() == values.num_rows(), "Size mismatch between group labels and value.");
  CUDF_EXPECTS(static_cast<size_type>(replace_policies.size()) == values.num_columns(),
               "Size mismatch between num_columns and replace_policies.");
  for (auto const& c : values)
    CUDF_EXPECTS(cudf::detail::class_of(c.type().id()) != CLS_NONE, "Only fixed-width columns of at most 8 bytes can be filled.",
                 cudf::data_type_error);
  CUDF_EXPECTS(_keys.num_columns() > 0, "The sort-based groupby needs at least one key column.");
  if (values.num_rows() == 0) return {empty_like(_keys), empty_like(values)};
  hipStream_t const s = stream.value();
  helper h{_keys, s};
  h.build(_include_null_keys == null_policy::EXCLUDE, _keys_are_sorted == sorted::YES);
  if (h.nk == 0) return {empty_like(_keys), empty_like(values)};
  int64_t const nk = h.nk;
  column_view const order_view{data_type{type_id::INT32}, static_cast<size_type>(nk), h.order, nullptr, 0};
  std::vector<std::unique_ptr<column>> cols;
  for (size_type c = 0; c < values.num_columns(); ++c) {
    auto const& col = values.column(c);
    if (!col.nullable()) {  // nothing to fill: the values in group order
      cols.push_back(std::move(cudf::gather(table_view{{col}}, order_view, out_of_bounds_policy::DONT_CHECK, stream, mr)->release()[0]));
      continue;
    }
    scratch tmp{s, get_current_device_resource_ref(), {}};
    auto g              = group_values(h, col, false, tmp, s);
    auto src            = make_src(h, col, g);
    src.read_values     = 0;
    src.backward        = replace_policies[c] == replace_policy::FOLLOWING ? 1 : 0;
    auto* state         = tmp.alloc<uint64_t>(static_cast<std::size_t>(nk));
    src.kind[0]         = scan_kind{OP_MAX_U, LIFT_VALID_POS, 8, state};
    src.nkinds          = 1;
    segmented_scan(src, s);
    auto out = std::make_unique<column>(col.type(), static_cast<size_type>(nk),
                                        rmm::device_buffer{static_cast<std::size_t>(nk) * size_of(col.type()), s, mr},
                                        rmm::device_buffer{bitmask_allocation_size_bytes(static_cast<size_type>(nk)), s, mr}, 0);
    auto* d_nulls = tmp.alloc<int32_t>(1);
    CUDF_HIP_TRY(hipMemsetAsync(d_nulls, 0, sizeof(int32_t), s));
    {
      prof::scope p_{"scan_fill", s};
      hipLaunchKernelGGL(k_replace_finish, dim3(blocks_of(nk)), dim3(256), 0, s, cudf::detail::make_device_column(col),
                         h.identity_order ? nullptr : h.order, state, nk, src.backward != 0, out->mutable_view().head(),
                         out->mutable_view().null_mask(), d_nulls);
    }
    CUDF_HIP_TRY(hipGetLastError());
    int32_t nulls = 0;
    CUDF_HIP_TRY(hipMemcpyAsync(&nulls, d_nulls, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    CUDF_HIP_TRY(hipStreamSynchronize(s));
    out->set_null_count(nulls);
    cols.push_back(std::move(out));
  }
  return {keys_in_group_order(h, stream, mr), std::make_unique<table>(std::move(cols))};
}

}  // namespace cudf::groupby
