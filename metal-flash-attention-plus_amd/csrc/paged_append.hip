// paged_append.hip — the write side of the paged, ragged K/V cache (mfa_paged_kv_append; no
// reference counterpart): the new-token rows of a [B, H_kv, R, D] 16-bit key / value pair go to
// their slots in the page pools the paged decode kernels read (attention_decode.hip, PagedKv).
//
// seq_lens[b] is the length AFTER the append, the value the following decode call reads: row r
// of the n_b = clamp(new_lens[b], 0, R) (R without new_lens) rows of sequence b is key
// t = seq_lens[b] - n_b + r, slot t mod page of pool page clamp(block_table[b][t / page]).
// Rows r >= n_b and rows whose t is outside [0, cap) are dropped; a written row never leaves the
// pools (the page id is clamped to them as the readers clamp it).
//
// mfa_paged_latent_append is the same kernel with one operand (grid.y = 1): the MLA latent pool
// as a key pool with one "head" of kv_latent_dim elements and no head stride.
//
// Memory-bound, one launch for K and V (blockIdx.y picks the operand).  A wave owns one
// (sequence, row) at a time: length, row count and block-table entry are uniform loads on the
// scalar path and the position, page and both base addresses are formed once per row; the lanes
// then walk the row's H_kv · D elements in 16-byte chunks, consecutive lanes on consecutive
// chunks of a head.  16-bit pools: one 16-byte load, one 16-byte store, the bits unchanged.
// INT8 pools: two 16-byte loads feed one 16-byte store of
//   q = clamp(round_half_away(x / scale) + zero_point, -128, 127),
// the arithmetic of quantize.hip element by element (exact widening, IEEE FP32 division — no
// reciprocal —, roundf), so the stored bytes are the library quantiser's and the CPU oracle's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "mfa_device.h"
#include "mfa_dispatch.h"
#include "mfa_launch.h"

namespace mfa {

namespace {

// The SRC parameter: SrcKind's SRC_SAME / SRC_I8 (mfa_stage.h).
constexpr int SRC_SAME = 0, SRC_I8 = 1;

typedef const __attribute__((address_space(4))) int32_t* append_i32_ptr;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// quantize.hip's round_to_int / clamp8 with the zero point added in between.
__device__ __forceinline__ uint32_t append_q8(float x, float scale, int zp) {
  const float r = roundf(x / scale);  // half away from zero
  int32_t i;
  if (!(r == r)) i = 0;
  else if (r >= 2147483647.0f) i = 2147483647;
  else if (r <= -2147483648.0f) i = -2147483647 - 1;
  else i = (int32_t)r;
  const int64_t v = (int64_t)i + zp;
  return (uint32_t)(uint8_t)(int8_t)(v < -128 ? -128 : (v > 127 ? 127 : v));
}

// Eight 16-bit elements (memory order) to bytes 0..7 of the result pair.
template <class E>
__device__ __forceinline__ void append_q8x8(const u32x4& w, float scale, int zp, uint32_t* lo,
                                            uint32_t* hi) {
  uint32_t o[2] = {0u, 0u};
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint16_t bits = (uint16_t)(w[k >> 1] >> (16 * (k & 1)));
    o[k >> 2] |= append_q8(E::to_f32(bits), scale, zp) << (8 * (k & 3));
  }
  *lo = o[0];
  *hi = o[1];
}

}  // namespace

constexpr int kAppendWaves = 4;  // rows in flight per workgroup

template <class E, int SRC>
__global__ __launch_bounds__(64 * kAppendWaves) void mfa_paged_append_kernel(PagedAppendParams p) {
  const int which = blockIdx.y;  // 0: key, 1: value
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const char* const src = (const char*)p.src[which];
  char* const pool = (char*)p.pool[which];
  const int64_t sb = p.s_sb[which], sh = p.s_sh[which], ss = p.s_ss[which];  // bytes
  const float scale = p.scale[which];
  const int zp = p.zp[which];
  // 16-byte destination chunks per head row and per (sequence, row).
  const int chunks = SRC == SRC_I8 ? p.D >> 4 : p.D >> 3;
  const int per_row = chunks * p.Hkv;

  for (int64_t row64 = (int64_t)blockIdx.x * kAppendWaves + wave; row64 < p.rows_total;
       row64 += (int64_t)gridDim.x * kAppendWaves) {
    const int row = (int)row64;
    const int b = row / p.R, r = row - b * p.R;
    const int len = ((append_i32_ptr)p.pg.seq_lens)[b];
    const int n = p.new_lens ? min(max(((append_i32_ptr)p.new_lens)[b], 0), p.R) : p.R;
    const int64_t t64 = (int64_t)len - n + r;  // any int32 length: no wrap
    if (r >= n || t64 < 0 || t64 >= p.cap) continue;
    const int t = (int)t64;  // < cap <= max_pages * page: the lookup stays in the table row
    const int entry = ((append_i32_ptr)p.pg.block_table)[(int64_t)b * p.pg.max_pages +
                                                         (t >> p.pg.lg_page)];
    const int page = min(max(entry, 0), p.pg.num_pages - 1);
    char* const drow = pool + (int64_t)page * p.pg.page_bytes +
                       (int64_t)(t & ((1 << p.pg.lg_page) - 1)) * p.tok_bytes;
    const char* const srow = src + b * sb + r * ss;
    for (int c = lane; c < per_row; c += 64) {
      const int h = c / chunks, ch = c - h * chunks;
      char* const d = drow + h * p.pg.head_bytes + 16 * ch;
      if constexpr (SRC == SRC_I8) {
        const u32x4* s = (const u32x4*)(srow + h * sh + 32 * ch);
        const u32x4 w0 = s[0], w1 = s[1];
        uint32_t q[4];
        append_q8x8<E>(w0, scale, zp, &q[0], &q[1]);
        append_q8x8<E>(w1, scale, zp, &q[2], &q[3]);
        *(u32x4*)d = u32x4{q[0], q[1], q[2], q[3]};
      } else {
        *(u32x4*)d = *(const u32x4*)(srow + h * sh + 16 * ch);
      }
    }
  }
}

hipError_t paged_append_dispatch(const PagedAppendParams& p, int elem, bool i8, int operands,
                                 hipStream_t stream) {
  // A workgroup per kAppendWaves rows up to 32768 workgroups, which then stride over the rest;
  // grid.y: the operands (key and value, or one latent pool).
  const int64_t wgs = (p.rows_total + kAppendWaves - 1) / kAppendWaves;
  const dim3 grid((unsigned)std::min<int64_t>(wgs, 32768), (unsigned)operands, 1),
      block(64 * kAppendWaves);
  if (elem == P_FP16)
    return i8 ? launch(mfa_paged_append_kernel<F16, SRC_I8>, grid, block, 0, stream, p)
              : launch(mfa_paged_append_kernel<F16, SRC_SAME>, grid, block, 0, stream, p);
  if (elem == P_BF16)
    return i8 ? launch(mfa_paged_append_kernel<BF16, SRC_I8>, grid, block, 0, stream, p)
              : launch(mfa_paged_append_kernel<BF16, SRC_SAME>, grid, block, 0, stream, p);
  return hipErrorNotSupported;
}

}  // namespace mfa
