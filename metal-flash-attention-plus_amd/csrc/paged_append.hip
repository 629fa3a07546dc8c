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
// mfa_paged_latent_rope_append has a kernel of its own below: two operands of different widths
// (the latent row and its 64-element rope key row) into two views of the same pages.
//
// mfa_paged_kv_append_rowwise has a kernel of its own as well (mfa_paged_append_rowwise_kernel):
// INT8 pools with one scale per written (row, kv head), computed from the row as it is written.
//
// mfa_paged_latent_append_rowwise is that quantiser on the latent row, with the rope row copied
// by the same wave (mfa_paged_latent_append_rw8_kernel).
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

// Row-wise INT8 pools (mfa_paged_kv_append_rowwise): every written (row, kv head) is quantised
// with a scale of its own, amax / 127, stored in the slot's entry of a scale pool.  The skeleton
// is mfa_paged_append_kernel's (a wave per (sequence, row), scalar-path addressing, blockIdx.y the
// operand); what differs is that a head row must be reduced before it can be written:
//   * a head row belongs to a group of G = next_pow2(D / 16) adjacent lanes (1 .. 16), so a pass
//     of the wave covers 64 / G heads; lane j of a group holds elements 16j .. 16j + 15 in
//     registers (two 16-byte loads) — lanes with 16j >= D and groups past H_kv hold zeros;
//   * the lane's amax (fmaxf: NaNs are ignored) meets the group's in log2 G butterfly steps of
//     __shfl_xor (ds_bpermute: the crossbar, no LDS memory), after which every lane of the group
//     holds the row's amax and forms the scale itself: amax / 127 (IEEE division), or 1 when
//     amax < 2^-64 — such a row quantises to zeros, and the floor bounds 1 / scale and log2 scale
//     for the decode kernels;
//   * the lane quantises its 16 registers, q = clamp(round_half_away(x / scale), -127, 127)
//     (append_q8's arithmetic), and stores one 16-byte chunk; lane 0 of the group stores the scale.
// The input is read once; there is no LDS and no second pass.
constexpr float kRowwiseFloor = 0x1p-64f;

template <class E>
__global__ __launch_bounds__(64 * kAppendWaves) void mfa_paged_append_rowwise_kernel(
    PagedAppendRwParams pr) {
  const PagedAppendParams& p = pr.a;
  const int which = blockIdx.y;  // 0: key, 1: value
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const char* const src = (const char*)p.src[which];
  char* const pool = (char*)p.pool[which];
  float* const spool = pr.scales[which];
  const int64_t sb = p.s_sb[which], sh = p.s_sh[which], ss = p.s_ss[which];  // bytes
  const int G = 1 << pr.lg_group, hpp = 64 >> pr.lg_group;  // lanes per head, heads per pass
  const int hl = lane >> pr.lg_group, ch = lane & (G - 1);
  const bool chunk_live = 16 * ch < p.D;

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
    const int slot = t & ((1 << p.pg.lg_page) - 1);
    char* const drow = pool + (int64_t)page * p.pg.page_bytes + (int64_t)slot * p.tok_bytes;
    float* const srow_sc = spool + (int64_t)page * pr.sc_page + slot;
    const char* const srow = src + b * sb + r * ss;
    for (int h0 = 0; h0 < p.Hkv; h0 += hpp) {  // wave-uniform: every lane takes the shuffles
      const int h = h0 + hl;
      const bool live = chunk_live && h < p.Hkv;
      u32x4 w0 = u32x4{0u, 0u, 0u, 0u}, w1 = w0;
      if (live) {
        const u32x4* s = (const u32x4*)(srow + h * sh + 32 * ch);
        w0 = s[0];
        w1 = s[1];
      }
      float a = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const uint32_t u = k < 4 ? w0[k & 3] : w1[k & 3];
        a = fmaxf(a, fabsf(E::to_f32((uint16_t)u)));
        a = fmaxf(a, fabsf(E::to_f32((uint16_t)(u >> 16))));
      }
      for (int o = 1; o < G; o <<= 1) a = fmaxf(a, __shfl_xor(a, o));
      const float scale = a >= kRowwiseFloor ? a / 127.0f : 1.0f;
      if (live) {
        uint32_t q[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          const uint32_t u = k < 8 ? w0[k >> 1] : w1[(k >> 1) & 3];
          const float x = E::to_f32((uint16_t)(u >> (16 * (k & 1))));
          const float rq = roundf(x / scale);  // half away from zero
          const int32_t i = !(rq == rq) ? 0 : (int32_t)fminf(fmaxf(rq, -127.f), 127.f);
          q[k >> 2] |= (uint32_t)(uint8_t)(int8_t)i << (8 * (k & 3));
        }
        *(u32x4*)(drow + h * p.pg.head_bytes + 16 * ch) = u32x4{q[0], q[1], q[2], q[3]};
        if (ch == 0) srow_sc[h * pr.sc_head] = scale;
      }
    }
  }
}

hipError_t paged_append_rowwise_dispatch(const PagedAppendRwParams& p, int elem,
                                         hipStream_t stream) {
  // mfa_paged_append_kernel's grid: key and value halves of one launch.
  const int64_t wgs = (p.a.rows_total + kAppendWaves - 1) / kAppendWaves;
  const dim3 grid((unsigned)std::min<int64_t>(wgs, 32768), 2, 1), block(64 * kAppendWaves);
  if (elem == P_FP16)
    return launch(mfa_paged_append_rowwise_kernel<F16>, grid, block, 0, stream, p);
  if (elem == P_BF16)
    return launch(mfa_paged_append_rowwise_kernel<BF16>, grid, block, 0, stream, p);
  return hipErrorNotSupported;
}

// The latent row and its rope key row of one new token, to slot t of the same page in two views
// of it (one fused [latent | rope] row, or two pools): mfa_paged_append_kernel's addressing — a
// wave per (sequence, row), position and page formed once from uniform loads — with the lanes
// walking the latent's 16-byte chunks and then the rope row's, each under its own strides.  16-bit
// rows of either type: the bits are copied, so the kernel has no element parameter.
__global__ __launch_bounds__(64 * kAppendWaves) void mfa_paged_rope_append_kernel(
    PagedRopeAppendParams p) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int nlat = p.chunks[0], nall = p.chunks[0] + p.chunks[1];
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
    const int slot = t & ((1 << p.pg.lg_page) - 1);
    for (int c = lane; c < nall; c += 64) {
      const int w = c >= nlat, ch = c - (w ? nlat : 0);   // operand and its chunk
      const char* const sp = (const char*)p.src[w] + b * p.s_sb[w] + r * p.s_ss[w] + 16 * ch;
      char* const dp = (char*)p.pool[w] + (int64_t)page * p.page_bytes[w] +
                       (int64_t)slot * p.tok_bytes[w] + 16 * ch;
      *(u32x4*)dp = *(const u32x4*)sp;
    }
  }
}

hipError_t paged_rope_append_dispatch(const PagedRopeAppendParams& p, hipStream_t stream) {
  // mfa_paged_append_kernel's grid for one operand.
  const int64_t wgs = (p.rows_total + kAppendWaves - 1) / kAppendWaves;
  return launch(mfa_paged_rope_append_kernel, dim3((unsigned)std::min<int64_t>(wgs, 32768)),
                dim3(64 * kAppendWaves), 0, stream, p);
}

// The latent row of one new token into a row-wise INT8 latent pool
// (mfa_paged_latent_append_rowwise): the row-wise quantiser above on one "head" of Lat elements,
// in the rope append's skeleton (a wave per (sequence, row), position and page from uniform
// loads).  A row of 512 (256) elements is one 16-byte load in each of 64 (32) lanes — eight
// elements per lane in registers; the amax (fmaxf: NaNs are ignored) meets the wave's in six
// __shfl_xor steps, every lane forms scale = amax >= 2^-64 ? amax / 127 : 1 itself, quantises its
// eight registers, q = clamp(round_half_away(x / scale), -127, 127) with a NaN element 0, and
// stores eight bytes; lane 0 stores the scale.  With a rope part, lanes 0..7 then copy the rope
// row's eight 16-byte chunks, the bits unchanged.  The input is read once; no LDS, no second pass.
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

template <class E>
__global__ __launch_bounds__(64 * kAppendWaves) void mfa_paged_latent_append_rw8_kernel(
    PagedLatentRw8AppendParams pw) {
  const PagedRopeAppendParams& p = pw.a;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const bool live = lane < p.chunks[0];                    // Lat / 8 lanes hold the row
  const bool rope_lane = p.src[1] != nullptr && lane < p.chunks[1];
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
    const int slot = t & ((1 << p.pg.lg_page) - 1);
    u32x4 w = u32x4{0u, 0u, 0u, 0u};
    if (live)
      w = *(const u32x4*)((const char*)p.src[0] + b * p.s_sb[0] + r * p.s_ss[0] + 16 * lane);
    float x[8];
    float a = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      x[k] = E::to_f32((uint16_t)(w[k >> 1] >> (16 * (k & 1))));
      a = fmaxf(a, fabsf(x[k]));
    }
    for (int o = 32; o > 0; o >>= 1) a = fmaxf(a, __shfl_xor(a, o));
    const float scale = a >= kRowwiseFloor ? a / 127.0f : 1.0f;
    if (live) {
      uint32_t q[2] = {0u, 0u};
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float rq = roundf(x[k] / scale);  // half away from zero
        const int32_t i = !(rq == rq) ? 0 : (int32_t)fminf(fmaxf(rq, -127.f), 127.f);
        q[k >> 2] |= (uint32_t)(uint8_t)(int8_t)i << (8 * (k & 3));
      }
      *(u32x2*)((char*)p.pool[0] + (int64_t)page * p.page_bytes[0] +
                (int64_t)slot * p.tok_bytes[0] + 8 * lane) = u32x2{q[0], q[1]};
      if (lane == 0) pw.scales[(int64_t)page * pw.sc_page + slot] = scale;
    }
    if (rope_lane) {
      const char* const sp = (const char*)p.src[1] + b * p.s_sb[1] + r * p.s_ss[1] + 16 * lane;
      char* const dp = (char*)p.pool[1] + (int64_t)page * p.page_bytes[1] +
                       (int64_t)slot * p.tok_bytes[1] + 16 * lane;
      *(u32x4*)dp = *(const u32x4*)sp;
    }
  }
}

hipError_t paged_latent_append_rw8_dispatch(const PagedLatentRw8AppendParams& p, int elem,
                                            hipStream_t stream) {
  // mfa_paged_append_kernel's grid for one operand.
  const int64_t wgs = (p.a.rows_total + kAppendWaves - 1) / kAppendWaves;
  const dim3 grid((unsigned)std::min<int64_t>(wgs, 32768)), block(64 * kAppendWaves);
  if (elem == P_FP16)
    return launch(mfa_paged_latent_append_rw8_kernel<F16>, grid, block, 0, stream, p);
  if (elem == P_BF16)
    return launch(mfa_paged_latent_append_rw8_kernel<BF16>, grid, block, 0, stream, p);
  return hipErrorNotSupported;
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
