// SPDX-License-Identifier: Apache-2.0
// The segmented inclusive scan core under groupby::scan and groupby::replace_nulls (segmented_scan.hip): the positions of `src`
// in group order, segments = runs of equal labels, up to SG_KINDS scan kinds answered by one pass over the values.
#pragma once
#include "call.hpp"

#include <hip/hip_runtime.h>

namespace cudf::groupby::detail {

constexpr int SG_KINDS = 8;  // scan kinds per fused pass

// the associative operator of a kind; every state is 64 bits
enum scan_op : int32_t { OP_ADD_I, OP_ADD_F32, OP_ADD_F64, OP_MUL_I, OP_MUL_F32, OP_MUL_F64, OP_MIN_U, OP_MAX_U };
// what a position contributes
enum scan_lift : int32_t {
  LIFT_INT,        // the value sign- or zero-extended to 64 bits (integer SUM / PRODUCT wrap as two's complement)
  LIFT_BITS,       // the value's bits (float SUM / PRODUCT)
  LIFT_ORDERED,    // order-preserving word of the value (MIN / MAX)
  LIFT_ONE,        // 1 (COUNT_ALL)
  LIFT_VALID,      // 1 for a valid value (COUNT_VALID)
  LIFT_VALID_POS,  // scan position + 1 of a valid value, else 0 (replace_nulls)
  LIFT_BIT0_POS,   // scan position + 1 where bit 0 of the word is set, else 0 (RANK: run starts)
  LIFT_BIT1_POS,   // the same for bit 1 (RANK: run ends, scanned backward)
  LIFT_BIT0,       // bit 0 of the word (RANK DENSE)
  LIFT_BIT2        // bit 2 of the word (RANK: valid values)
};

struct scan_kind {
  int32_t op;
  int32_t lift;   // LIFT_ORDERED results are decoded back to the value
  int32_t width;  // bytes per output element
  void* out;      // one element per position, indexed like the input
};

struct scan_src {
  cudf::detail::device_column col;  // the values, read at the position itself when bits == nullptr (rows already in group order)
  uint64_t const* bits;       // the values gathered into group order, or one word per position (RANK)
  bitmask_type const* valid;  // validity per position; nullptr: every position valid
  int32_t const* labels;      // group of each position
  int64_t n;
  int32_t backward;           // scan from the last position to the first
  int32_t read_values;        // some kind reads the value (or word) of a position
  int32_t nkinds;
  scan_kind kind[SG_KINDS];
};

// the segmented inclusive scans of src's kinds (reduce, spine, apply)
void segmented_scan(scan_src const& src, hipStream_t s);

__device__ __forceinline__ void store_width(void* out, int64_t i, int32_t width, uint64_t v)
{
  switch (width) {
    case 1: cudf::detail::gstore(static_cast<uint8_t*>(out) + i, static_cast<uint8_t>(v)); break;
    case 2: cudf::detail::gstore(static_cast<uint16_t*>(out) + i, static_cast<uint16_t>(v)); break;
    case 4: cudf::detail::gstore(static_cast<uint32_t*>(out) + i, static_cast<uint32_t>(v)); break;
    default: cudf::detail::gstore(static_cast<uint64_t*>(out) + i, v);
  }
}

}  // namespace cudf::groupby::detail
