// SPDX-License-Identifier: Apache-2.0
// The sort-based aggregate: what the reference falls back to when a request holds a kind the hash tables cannot serve
// (cpp/src/groupby/groupby.cu:64-69 -> cpp/src/groupby/sort/aggregate.cpp). The sort helper (sort_helper.hpp) puts the rows in key
// order and labels the groups; NTH_ELEMENT, NUNIQUE, MEDIAN and QUANTILE read that order here. The kinds the hash engine serves are
// handed to it with the group label as the key and come back aligned to the sorted unique keys.
#include "sort_helper.hpp"
#include "../common/profiler.hpp"

#include <cudf/copying.hpp>
#include <cudf/groupby.hpp>
#include <cudf/null_mask.hpp>
#include <cudf/utilities/error.hpp>

#include <hip/hip_runtime.h>

#include <limits>

namespace cudf::groupby::detail {
namespace {
using cudf::detail::CLS_BOOL;
using cudf::detail::CLS_F32;
using cudf::detail::CLS_SINT;
using cudf::detail::CLS_UINT;
using cudf::detail::col_is_valid;
using cudf::detail::col_load_bits;
using cudf::detail::device_column;
using cudf::detail::gload;
using cudf::detail::gstore;
namespace prof = cudf::detail::prof;

// row_label[order[i]] = labels[i]
__global__ void __launch_bounds__(256) k_row_labels(uint32_t const* order, int32_t const* labels, int64_t nk, int32_t* row_label)
{
  int64_t const i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i < nk) gstore(row_label + gload(order + i), gload(labels + i));
}

// where[label] = j for the engine's j-th result row; the label G (rows of excluded keys) is dropped
__global__ void __launch_bounds__(256) k_invert_labels(int32_t const* result_labels, int64_t rows, int32_t G, int32_t* where)
{
  int64_t const j = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (j >= rows) return;
  int32_t const g = gload(result_labels + j);
  if (g >= 0 && g < G) gstore(where + g, static_cast<int32_t>(j));
}

// NTH_ELEMENT counting every row (reference group_nth_element.cu:58-72): index = the group's n-th row in key order
__global__ void __launch_bounds__(256) k_nth_of_all(int32_t const* offsets, int32_t G, int32_t n, uint32_t const* order, int32_t* index,
                                                    int32_t none)
{
  int32_t const g = blockIdx.x * 256 + threadIdx.x;
  if (g >= G) return;
  int32_t const first = gload(offsets + g), size = gload(offsets + g + 1) - first;
  bool const inside   = n < 0 ? size >= -n : size > n;
  gstore(index + g, inside ? static_cast<int32_t>(gload(order + first + (n < 0 ? size + n : n))) : none);
}

// NTH_ELEMENT skipping nulls (:73-116): the row whose count of valid rows before it inside the group equals n
__global__ void __launch_bounds__(256) k_nth_of_valid(uint32_t const* valid, uint32_t const* valid_before /* nk + 1 */, int32_t const* labels,
                                                      int32_t const* offsets, int64_t nk, int32_t n, uint32_t const* order, int32_t* index)
{
  int64_t const i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= nk || !gload(valid + i)) return;
  int32_t const g     = gload(labels + i);
  uint32_t const base = gload(valid_before + gload(offsets + g));
  int32_t const intra = static_cast<int32_t>(gload(valid_before + i) - base);
  int32_t nth         = n;
  if (n < 0) nth = static_cast<int32_t>(gload(valid_before + gload(offsets + g + 1)) - base) + n;
  if (intra == nth) gstore(index + g, static_cast<int32_t>(gload(order + i)));
}

// NUNIQUE (group_nunique.cu:50-59): 1 where a countable row starts a run of equal values inside its group
__global__ void __launch_bounds__(256) k_unique_flags(device_column col, uint32_t const* vrow, int32_t const* labels, int32_t const* offsets,
                                                      int64_t nk, bool count_nulls, uint32_t* flags)
{
  int64_t const i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= nk) return;
  uint32_t const row = gload(vrow + i);
  bool const valid   = col_is_valid(col, row);
  uint32_t f         = 0;
  if (valid || count_nulls) {
    f = (gload(offsets + gload(labels + i)) == i || !same_value(col, row, valid, gload(vrow + i - 1))) ? 1u : 0u;
  }
  gstore(flags + i, f);
}

// out[g] = scanned[offsets[g + 1]] - scanned[offsets[g]]  (scanned holds nk + 1 entries)
__global__ void __launch_bounds__(256) k_segment_sums(uint32_t const* scanned, int32_t const* offsets, int32_t G, int32_t* out)
{
  int32_t const g = blockIdx.x * 256 + threadIdx.x;
  if (g < G) gstore(out + g, static_cast<int32_t>(gload(scanned + gload(offsets + g + 1)) - gload(scanned + gload(offsets + g))));
}
__global__ void __launch_bounds__(256) k_group_sizes(int32_t const* offsets, int32_t G, int32_t* out)
{
  int32_t const g = blockIdx.x * 256 + threadIdx.x;
  if (g < G) gstore(out + g, gload(offsets + g + 1) - gload(offsets + g));
}

__device__ __forceinline__ double as_double(device_column const& c, uint32_t row)
{
  uint64_t const raw = col_load_bits(c, row);
  switch (c.cls) {
    case CLS_SINT: return static_cast<double>(cudf::detail::sign_extend(raw, c.width));
    case CLS_UINT: return static_cast<double>(raw);
    case CLS_BOOL: return raw != 0 ? 1.0 : 0.0;
    case CLS_F32: return static_cast<double>(__uint_as_float(static_cast<uint32_t>(raw)));
    default: return __longlong_as_double(static_cast<long long>(raw));
  }
}

struct quantile_args {
  device_column col;
  uint32_t const* vrow;
  int32_t const* offsets;
  int32_t const* counts;  // valid rows per group (they lead each group of vrow)
  double const* q;
  int32_t nq;
  int32_t interp;
  int64_t total;          // G * nq
  double* out;
  bitmask_type* mask;
  int32_t* null_count;
};

// one (group, quantile) per thread (reference group_quantiles.cu:43-71, quantiles_util.hpp:20-176)
__global__ void __launch_bounds__(256) k_quantiles(quantile_args a)
{
  int64_t const e   = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  bool const inside = e < a.total;
  bool valid        = false;
  if (inside) {
    int32_t const g    = static_cast<int32_t>(e / a.nq);
    int32_t const size = gload(a.counts + g);
    double result      = 0.0;
    if (size > 0) {
      valid                 = true;
      uint32_t const* first = a.vrow + gload(a.offsets + g);
      double const quantile = fmin(fmax(gload(a.q + e % a.nq), 0.0), 1.0);
      double const pos      = quantile * (size - 1);
      int32_t const lower   = static_cast<int32_t>(floor(pos));
      int32_t const higher  = static_cast<int32_t>(ceil(pos));
      double const fraction = pos - lower;
      auto at               = [&](int32_t k) { return as_double(a.col, gload(first + k)); };
      switch (a.interp) {
        case static_cast<int32_t>(interpolation::LOWER): result = at(lower); break;
        case static_cast<int32_t>(interpolation::HIGHER): result = at(higher); break;
        case static_cast<int32_t>(interpolation::NEAREST): result = at(static_cast<int32_t>(nearbyint(pos))); break;
        case static_cast<int32_t>(interpolation::NEAREST_HALF_UP): result = at(static_cast<int32_t>(round(pos))); break;
        case static_cast<int32_t>(interpolation::MIDPOINT):
          if (a.col.cls == CLS_SINT && a.col.width == 8) {
            // halves and remainders apart, so that no sum leaves the int64 range (quantiles_util.hpp:46-53)
            int64_t const l = static_cast<int64_t>(col_load_bits(a.col, gload(first + lower)));
            int64_t const h = static_cast<int64_t>(col_load_bits(a.col, gload(first + higher)));
            result          = static_cast<double>(l / 2 + h / 2) + static_cast<double>(l % 2 + h % 2) * 0.5;
          } else {
            result = at(lower) / 2 + at(higher) / 2;
          }
          break;
        default: {  // LINEAR
          double const one_minus = 1.0 - fraction;
          result                 = one_minus * at(lower) + fraction * at(higher);
        }
      }
    }
    gstore(a.out + e, result);
  }
  store_wave_validity(valid, e, a.total, a.mask, a.null_count);
}

bool arithmetic(type_id t) { return t >= type_id::INT8 && t <= type_id::BOOL8; }

std::unique_ptr<column> int32_column(int64_t size, stream_ref stream, rmm::device_async_resource_ref mr)
{
  return std::make_unique<column>(data_type{type_id::INT32}, static_cast<size_type>(size),
                                  rmm::device_buffer{static_cast<std::size_t>(size) * sizeof(int32_t), stream.value(), mr}, rmm::device_buffer{}, 0);
}

// result column j of the engine's answer, reordered by `where` (one INT32 per group)
std::unique_ptr<column> reorder(column_view const& c, column_view const& where, stream_ref stream, rmm::device_async_resource_ref mr)
{
  if (c.type().id() == type_id::STRUCT) {
    // SUM_OVERFLOW {sum, overflow}: the children carry no masks, the struct's mask travels with the first child and returns to the struct
    column_view const sum_with_mask{c.child(0).type(), c.size(), c.child(0).head(), c.null_mask(), c.null_count(), c.child(0).offset()};
    auto t    = cudf::gather(table_view{{sum_with_mask, c.child(1)}}, where, out_of_bounds_policy::DONT_CHECK, stream, mr);
    auto cols = t->release();
    auto const nulls = cols[0]->null_count();
    auto sum         = cols[0]->release();
    std::vector<std::unique_ptr<column>> children;
    children.push_back(std::make_unique<column>(c.child(0).type(), where.size(), std::move(*sum.data), rmm::device_buffer{}, 0));
    children.push_back(std::move(cols[1]));
    return std::make_unique<column>(data_type{type_id::STRUCT}, where.size(), rmm::device_buffer{},
                                    c.nullable() ? std::move(*sum.null_mask) : rmm::device_buffer{}, c.nullable() ? nulls : 0, std::move(children));
  }
  auto t = cudf::gather(table_view{{c}}, where, out_of_bounds_policy::DONT_CHECK, stream, mr);
  return std::move(t->release()[0]);
}
}  // namespace

std::pair<std::unique_ptr<table>, std::vector<aggregation_result>> sort_aggregate(table_view const& keys, null_policy include_null_keys,
                                                                                  bool keys_are_sorted,
                                                                                  std::span<aggregation_request const> requests,
                                                                                  stream_ref stream, rmm::device_async_resource_ref mr)
{
  hipStream_t const s = stream.value();
  CUDF_EXPECTS(keys.num_columns() > 0, "The sort-based groupby needs at least one key column.");
  helper h{keys, s};
  // which order the one sort should produce (helper::build)
  column_view const* inner_values = nullptr;
  bool any_nth                    = false;
  for (auto const& r : requests)
    for (auto const& a : r.aggregations) {
      any_nth = any_nth || a->kind == aggregation::NTH_ELEMENT;
      if (inner_values == nullptr && (a->kind == aggregation::MEDIAN || a->kind == aggregation::QUANTILE || a->kind == aggregation::NUNIQUE) &&
          r.values.size() == keys.num_rows() && r.values.head() != nullptr)
        inner_values = &r.values;
    }
  h.build(include_null_keys == null_policy::EXCLUDE, keys_are_sorted, any_nth ? nullptr : inner_values);
  int32_t const G = h.G;

  std::vector<aggregation_result> results(requests.size());
  for (std::size_t r = 0; r < requests.size(); ++r) results[r].results.resize(requests[r].aggregations.size());

  if (G == 0) {  // every key excluded: typed empty results
    for (std::size_t r = 0; r < requests.size(); ++r)
      for (std::size_t j = 0; j < requests[r].aggregations.size(); ++j) {
        auto const kind = requests[r].aggregations[j]->kind;
        if (kind == aggregation::SUM_OVERFLOW) {
          std::vector<std::unique_ptr<column>> children;
          children.push_back(make_empty_column(requests[r].values.type()));
          children.push_back(make_empty_column(data_type{type_id::BOOL8}));
          results[r].results[j] =
            std::make_unique<column>(data_type{type_id::STRUCT}, 0, rmm::device_buffer{}, rmm::device_buffer{}, 0, std::move(children));
        } else {
          results[r].results[j] = make_empty_column(cudf::detail::target_type(requests[r].values.type(), kind));
        }
      }
    return {empty_like(keys), std::move(results)};
  }

  // the unique keys, ascending
  column_view const first_rows{data_type{type_id::INT32}, G, h.first_row, nullptr, 0};
  auto unique_keys = cudf::gather(keys, first_rows, out_of_bounds_policy::DONT_CHECK, stream, mr);

  // ---- the kinds the hash engine serves: keyed on the row's group label
  {
    std::vector<aggregation_request> engine_requests;
    std::vector<std::pair<std::size_t, std::size_t>> slots;  // (request, aggregation) of every engine result, in order
    for (std::size_t r = 0; r < requests.size(); ++r) {
      aggregation_request er{requests[r].values, {}};
      for (std::size_t j = 0; j < requests[r].aggregations.size(); ++j) {
        auto const& a = requests[r].aggregations[j];
        if (!is_engine_kind(a->kind)) continue;
        auto clone = a->clone();
        auto* as_groupby = dynamic_cast<groupby_aggregation*>(clone.get());
        CUDF_EXPECTS(as_groupby != nullptr, "not a groupby aggregation");
        clone.release();
        er.aggregations.emplace_back(as_groupby);
        slots.emplace_back(r, j);
      }
      if (!er.aggregations.empty()) engine_requests.push_back(std::move(er));
    }
    if (!engine_requests.empty()) {
      scratch tmp{s, get_current_device_resource_ref(), {}};
      auto* row_label = tmp.alloc<int32_t>(static_cast<std::size_t>(h.n));
      if (h.nk < h.n) fill_i32(row_label, h.n, G, s);
      hipLaunchKernelGGL(k_row_labels, dim3(blocks_of(h.nk)), dim3(256), 0, s, h.order, h.labels, h.nk, row_label);
      CUDF_HIP_TRY(hipGetLastError());
      column_view const label_col{data_type{type_id::INT32}, static_cast<size_type>(h.n), row_label, nullptr, 0};
      cudf::groupby::groupby by_label{table_view{{label_col}}, null_policy::INCLUDE};
      auto [label_keys, engine_results] = by_label.aggregate(engine_requests, stream, get_current_device_resource_ref());
      auto where = int32_column(G, stream, get_current_device_resource_ref());
      hipLaunchKernelGGL(k_invert_labels, dim3(blocks_of(label_keys->num_rows())), dim3(256), 0, s,
                         label_keys->get_column(0).view().data<int32_t>(), static_cast<int64_t>(label_keys->num_rows()), G,
                         where->mutable_view().data<int32_t>());
      CUDF_HIP_TRY(hipGetLastError());
      std::size_t slot = 0;
      for (auto& er : engine_results)
        for (auto& c : er.results) {
          auto const [r, j]     = slots[slot++];
          results[r].results[j] = reorder(c->view(), where->view(), stream, mr);
        }
    }
  }

  // ---- the kinds that need the order
  for (std::size_t r = 0; r < requests.size(); ++r) {
    auto const& values = requests[r].values;
    auto const dcol    = cudf::detail::make_device_column(values);
    for (std::size_t j = 0; j < requests[r].aggregations.size(); ++j) {
      auto const& a = *requests[r].aggregations[j];
      if (!is_sort_kind(a.kind)) continue;
      scratch tmp{s, get_current_device_resource_ref(), {}};
      if (a.kind == aggregation::NTH_ELEMENT) {
        auto const& nth = dynamic_cast<cudf::detail::nth_element_aggregation const&>(a);
        auto index      = int32_column(G, stream, get_current_device_resource_ref());
        auto* d_index   = index->mutable_view().data<int32_t>();
        int32_t const none = values.size();  // out of bounds: a null row of the gather
        if (nth._null_handling == null_policy::INCLUDE || !values.has_nulls()) {
          hipLaunchKernelGGL(k_nth_of_all, dim3(blocks_of(G)), dim3(256), 0, s, h.offsets, G, nth._n, h.order, d_index, none);
        } else {
          uint32_t* valid = nullptr;
          auto* before    = h.valid_before(values, tmp, &valid);
          fill_i32(d_index, G, none, s);
          hipLaunchKernelGGL(k_nth_of_valid, dim3(blocks_of(h.nk)), dim3(256), 0, s, valid, before, h.labels, h.offsets, h.nk, nth._n, h.order,
                             d_index);
        }
        CUDF_HIP_TRY(hipGetLastError());
        auto t   = cudf::gather(table_view{{values}}, index->view(), out_of_bounds_policy::NULLIFY, stream, mr);
        auto col = std::move(t->release()[0]);
        if (!col->has_nulls()) col->set_null_mask(rmm::device_buffer{}, 0);
        results[r].results[j] = std::move(col);
      } else if (a.kind == aggregation::NUNIQUE) {
        auto const& nu = dynamic_cast<cudf::detail::nunique_aggregation const&>(a);
        auto* vrow     = h.value_order(values);
        auto* flags    = tmp.alloc<uint32_t>(static_cast<std::size_t>(h.nk) + 1);
        hipLaunchKernelGGL(k_unique_flags, dim3(blocks_of(h.nk)), dim3(256), 0, s, dcol, vrow, h.labels, h.offsets, h.nk,
                           nu._null_handling == null_policy::INCLUDE, flags);
        exclusive_scan(flags, flags, h.nk, flags + h.nk, tmp, s);
        auto out = int32_column(G, stream, mr);
        hipLaunchKernelGGL(k_segment_sums, dim3(blocks_of(G)), dim3(256), 0, s, flags, h.offsets, G, out->mutable_view().data<int32_t>());
        CUDF_HIP_TRY(hipGetLastError());
        results[r].results[j] = std::move(out);
      } else {  // MEDIAN, QUANTILE
        CUDF_EXPECTS(arithmetic(values.type().id()), "Only arithmetic types are supported in quantiles");
        std::vector<double> q{0.5};
        auto interp = interpolation::LINEAR;
        if (a.kind == aggregation::QUANTILE) {
          auto const& qa = dynamic_cast<cudf::detail::quantile_aggregation const&>(a);
          q              = qa._quantiles;
          interp         = qa._interpolation;
        }
        auto* vrow   = h.value_order(values);
        auto* counts = tmp.alloc<int32_t>(static_cast<std::size_t>(G));
        if (values.has_nulls()) {
          auto* before = h.valid_before(values, tmp);
          hipLaunchKernelGGL(k_segment_sums, dim3(blocks_of(G)), dim3(256), 0, s, before, h.offsets, G, counts);
        } else {
          hipLaunchKernelGGL(k_group_sizes, dim3(blocks_of(G)), dim3(256), 0, s, h.offsets, G, counts);
        }
        int64_t const total = static_cast<int64_t>(G) * static_cast<int64_t>(q.size());
        CUDF_EXPECTS(total <= std::numeric_limits<size_type>::max(), "quantile result exceeds the column size limit", std::overflow_error);
        auto out = make_fixed_width_column(data_type{type_id::FLOAT64}, static_cast<size_type>(total), mask_state::UNINITIALIZED, stream, mr);
        if (total > 0) {
          auto* d_q     = tmp.alloc<double>(q.size());
          auto* d_nulls = tmp.alloc<int32_t>(1);
          CUDF_HIP_TRY(hipMemcpyAsync(d_q, q.data(), q.size() * sizeof(double), hipMemcpyHostToDevice, s));
          CUDF_HIP_TRY(hipMemsetAsync(d_nulls, 0, sizeof(int32_t), s));
          quantile_args qa{};
          qa.col        = dcol;
          qa.vrow       = vrow;
          qa.offsets    = h.offsets;
          qa.counts     = counts;
          qa.q          = d_q;
          qa.nq         = static_cast<int32_t>(q.size());
          qa.interp     = static_cast<int32_t>(interp);
          qa.total      = total;
          qa.out        = out->mutable_view().data<double>();
          qa.mask       = out->mutable_view().null_mask();
          qa.null_count = d_nulls;
          {
            prof::scope p_{"sort_quantiles", s};
            hipLaunchKernelGGL(k_quantiles, dim3(blocks_of(total)), dim3(256), 0, s, qa);
          }
          CUDF_HIP_TRY(hipGetLastError());
          int32_t h_nulls = 0;
          CUDF_HIP_TRY(hipMemcpyAsync(&h_nulls, d_nulls, sizeof(int32_t), hipMemcpyDeviceToHost, s));
          CUDF_HIP_TRY(hipStreamSynchronize(s));
          out->set_null_count(h_nulls);
        }
        results[r].results[j] = std::move(out);
      }
    }
  }
  return {std::move(unique_keys), std::move(results)};
}

}  // namespace cudf::groupby::detail
