// SPDX-License-Identifier: Apache-2.0
// Device side of the packed radix words of sorting_impl.hpp: row_word() makes one word of one row from a plan's fields. Shared by
// the kernels that sort and check one table (sorting_kernels.hip) and those that compare the rows of two (search_merge_kernels.hip).
#pragma once
#include "sorting_impl.hpp"

namespace cudf::detail::sorting {

// the loads of one field of one row: the element's bits and the mask word that holds the row's validity bit
__device__ __forceinline__ void load_field(plan_field const& f, uint32_t row, uint64_t& raw, uint32_t& mask_word)
{
  raw       = f.vbits != 0 ? col_load_bits(f.col, row) : 0;
  mask_word = f.col.mask != nullptr ? gload(f.col.mask + ((static_cast<int64_t>(f.col.offset) + row) >> 5)) : ~0u;
}

// the field's bits in its word (sorting_impl.hpp, "Inside a field")
__device__ __forceinline__ uint64_t field_bits(plan_field const& f, uint32_t row, uint64_t raw, uint32_t mask_word)
{
  bool const valid = (mask_word >> ((static_cast<int64_t>(f.col.offset) + row) & 31)) & 1u;
  uint64_t out     = 0;
  if (f.vbits != 0) {
    uint64_t const vmask = f.vbits == 64 ? ~0ull : (1ull << f.vbits) - 1;
    uint64_t code        = f.col.cls == CLS_SINT ? raw ^ (1ull << (f.vbits - 1))
                                                 : ordered_word(normalize_key_bits(raw, f.col.cls), f.col.cls, f.col.width);
    if (f.invert) code = ~code & vmask;
    if (!valid) code = 0;
    out = code << f.shift;
  }
  if (f.null_pos >= 0) out |= static_cast<uint64_t>(valid == (f.null_first != 0)) << f.null_pos;
  return out;
}

// the word made of fields f[0 .. nf) for `row`. Every load of the row is issued before the first loaded value is used.
__device__ __forceinline__ uint64_t row_word(plan_field const* f, int nf, uint32_t row)
{
  uint64_t raw[MAX_COLS];
  uint32_t mask_word[MAX_COLS];
#pragma unroll
  for (int k = 0; k < MAX_COLS; ++k)
    if (k < nf) load_field(f[k], row, raw[k], mask_word[k]);
  uint64_t w = 0;
#pragma unroll
  for (int k = 0; k < MAX_COLS; ++k)
    if (k < nf) w |= field_bits(f[k], row, raw[k], mask_word[k]);
  return w;
}

}  // namespace cudf::detail::sorting
