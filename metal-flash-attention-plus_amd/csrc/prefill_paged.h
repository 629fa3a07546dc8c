// prefill_paged.h — what the paged prefill kernels share (attention_prefill_paged.hip: 16-bit
// pools; attention_prefill_paged_kv8.hip: INT8 pools widened on load): the uniform loads of the
// device values, the block-table lookup, the 32-key segment's address and byte range, and the
// result of a row with no visible key.
#pragma once
#include "attention_fwd2.h"

namespace mfa {

// Uniform (scalar-path) loads of the device values.
typedef const __attribute__((address_space(4))) int32_t* prefill_i32_ptr;

// Block-table entry of the 32-key segment at key t (wave-uniform) of batch item b, as stored:
// the lookup index is clamped to the table row (the look-ahead runs past the last tile), the id
// is clamped to the pools by prefill_segment, where it is used.
__device__ __forceinline__ int prefill_page(const PagedKv& pg, int b, int t) {
  const int j = min(t >> pg.lg_page, pg.max_pages - 1);
  return ((prefill_i32_ptr)pg.block_table)[(int64_t)b * pg.max_pages + j];
}

// Byte offset, from a head's first byte in the pool (pool + kv head offset), of the first row of
// the 32-key segment at key t, and the bytes of the segment a load may touch: the rows below both
// the sequence's length and the page's end (attention_decode.hip's kv_tile; 64-bit page offset).
// ssb: bytes per token slot; rowbytes: valid bytes per row.
__device__ __forceinline__ int64_t prefill_segment(const PagedKv& pg, int page, int t, int len,
                                                   int ssb, int rowbytes, int* bytes) {
  const int pend = ((t >> pg.lg_page) + 1) << pg.lg_page;
  const int rows = min(min(len, pend) - t, 32);
  *bytes = rows > 0 ? (rows - 1) * ssb + rowbytes : 0;
  const int id = min(max(page, 0), pg.num_pages - 1);
  return (int64_t)id * pg.page_bytes + (int64_t)(t & ((1 << pg.lg_page) - 1)) * ssb;
}

// The result of a row with no visible key: zeros and L = -FLT_MAX (-inf once rounded to FP16),
// in store_o_l's lane layout.
template <int DP>
__device__ __forceinline__ void store_dead_row(const FwdParams& p, int b, int h, int q, int hh) {
  float* orow = p.o + (int64_t)b * p.o_sb + (int64_t)h * p.o_sh + (int64_t)q * p.o_ss;
#pragma unroll
  for (int dt = 0; dt < DP / 32; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int d = dt * 32 + 8 * g + 4 * hh;
      if (d < p.D) st_o4<false>(orow + d, 0.f, 0.f, 0.f, 0.f);
    }
  if (hh == 0) store_l(p, -kFltMax, b, h, q);
}

}  // namespace mfa
