// attention_mla_latent_rw8.hip — the paged latent-space attention of absorbed MLA over a
// row-wise INT8 latent pool (mfa_paged_mla_decode_forward_rowwise): one byte per latent element
// and one FP32 scale per token, the rope key part, where there is one, left in 16 bits.
//
// Key j's latent row is E(scales[j] · (float)q_j[d]): one FP32 product rounded once to the 16-bit
// type E.  The kernel forms exactly those values on the way into LDS and then runs
// mla_latent_tile_body.h on the same Tile16<LAT> image mfa_mla_latent_paged_kernel fills, so the
// call returns, bit for bit, what the 16-bit call returns on a pool that holds the rounded rows.
// Work split, exchange, partial state and the merge are the 16-bit paged kernel's
// (attention_mla_latent.hip); with ROPE the rope k-step, the `krf` fetch a tile ahead and the
// `qrf` fragment are mfa_mla_latent_paged_rope_kernel's.  What is this kernel's own:
//   * staging by 16-byte buffer loads of 16 INT8 elements: LAT / 16 lanes per row, 8 rows
//     (latent 512) or 16 rows (256) per pass, 4 or 2 passes per 32-key tile — 16 staging VGPRs per
//     tile at latent 512 where the 16-bit kernel holds 32.  The row step of a pass goes into the
//     pass's descriptor, so the passes share one lane offset;
//   * the workgroup's LDS is full (two 16-bit tiles and the exchange area), so there is no scale
//     strip: lane l of every wave fetches the scale of tile row l & 31 with the tile's loads — one
//     dword per lane through a descriptor over the scale entries of the tile's rows below len_b,
//     so the entry of a row at or past len_b reads 0 and is never fetched — and the store takes its
//     row's scale from that register by a lane shuffle;
//   * dequantisation in the store: a byte's bits are flipped to the unsigned q + 128,
//     v_cvt_f32_ubyteN widens it exactly, and fma(q + 128, scale, −128·scale) is the exact product
//     scale · q rounded once to FP32 (−128·scale is exact); a register barrier keeps the conversion
//     to E a rounding of that FP32 value, not a fused rounding of the exact product.  A row at or
//     past len_b has zero bytes and a zero scale: +0 in every element, whatever memory holds;
//   * the prefetch distance PF is a compile-time constant.  PF = 2 keeps tiles t + 1 and t + 2 in
//     registers while tile t is computed; the loop is unrolled by two by hand
//     (mla_latent_rw8_step.h) so the two register sets are static.
#include "mfa_stage.h"
#include "mfa_dispatch.h"

namespace mfa {

// Tiles in flight per workgroup (1 or 2); -DMFA_MLA_RW8_DIST=2 builds the other distance for an
// A/B measurement.  Distance 1 is what ships: distance 2 spills at latent 512 (1 VGPR without the
// rope part, 24 with it) and measured no faster there ("Paged MLA over a row-wise INT8
// latent cache").
#ifndef MFA_MLA_RW8_DIST
#define MFA_MLA_RW8_DIST 1
#endif
constexpr int rw8_distance(int) { return MFA_MLA_RW8_DIST; }

typedef const __attribute__((address_space(4))) int32_t* rw8_i32_ptr;

template <class E, int LAT, bool ROPE>
__global__ void __launch_bounds__(256, 2)
    mfa_mla_latent_paged_rw8_kernel(LatentPagedRw8Params pw) {
  constexpr int BK = 32, NT = 256;
  constexpr int WS = LAT / 4;              // latent dims per wave
  constexpr int DS = WS / 16;              // MFMA k-steps of the wave's QK^T slice
  constexpr int ND = WS / 32;              // O^T tiles per wave
  constexpr int CPR = LAT / 16;            // 16-byte loads (16 INT8 elements) per latent row
  constexpr int CPT = BK * CPR / NT;       // loads staged per thread and tile
  constexpr int RPP = NT / CPR;            // rows a pass of the workgroup covers
  constexpr int TILEB = BK * LAT * 2;
  constexpr int XST = 16;                  // floats per lane in the exchange area
  constexpr int ROPED = 64;                // rope elements per key, 16 per wave
  constexpr int PF = rw8_distance(LAT);    // prefetch distance in tiles
  static_assert(PF == 1 || PF == 2, "one or two tiles in flight");
  using A = Arith16<E, LAT>;
  using TT = Tile16<LAT>;
  const LatentPagedRopeParams& pr = pw.r;
  const LatentPagedParams& pp = pr.c;
  const LatentParams& p = pp.l;
  const PagedKv& pg = pp.pg;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const tb0 = smem;                              // 2 latent tiles, 16-bit
  float* const xb = reinterpret_cast<float*>(smem + 2 * TILEB);  // [4 waves][64 lanes][XST]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l32 = lane & 31, hh = lane >> 5;
  const int split = blockIdx.x % p.nsplit;
  const int bq = blockIdx.x / p.nsplit;
  const int b = bq / p.nblk;
  const int r0 = (bq % p.nblk) * 32;
  const int r = r0 + l32;
  const bool rvalid = r < p.R;
  const int spos = rvalid ? r % p.Sq : 0;   // the row's index among its head's Sq rows

  // The sequence's keys (uniform) and the last key this row sees.
  const int len = min(max(((rw8_i32_ptr)pg.seq_lens)[b], 0), p.Skv);
  const int klim = p.causal ? len - p.Sq + spos : len - 1;

  // Keys this block needs: all of the sequence, or up to its rows' largest limit.
  int kend = len;
  if (p.causal) {
    const int rl = min(r0 + 31, p.R - 1);
    const int smax = (r0 / p.Sq == rl / p.Sq) ? rl % p.Sq : p.Sq - 1;
    kend = min(kend, len - p.Sq + smax + 1);
  }
  const int kbeg = split * p.chunk;
  kend = min(kend, kbeg + p.chunk);

  // Q̃ fragments of the wave's slice: d = w·WS + 16·ds + 8·hh + j.
  i16x8 qf[DS];
  {
    const uint16_t* qrow = (const uint16_t*)p.q + ((int64_t)b * p.R + (rvalid ? r : 0)) * LAT;
#pragma unroll
    for (int ds = 0; ds < DS; ++ds) {
      i16x8 v = i16x8{0, 0, 0, 0, 0, 0, 0, 0};
      if (rvalid) v = *reinterpret_cast<const i16x8*>(qrow + wave * WS + 16 * ds + 8 * hh);
      qf[ds] = v;
    }
  }
  // The q_rope fragment (ROPE): d = 16·w + 8·hh + j of row r of the dense [B][R][64] rope query,
  // through a buffer over the block's rows below R (a row past R returns zeros).
  auto qrope_load = [&]() {
    const __amdgpu_buffer_rsrc_t qrs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)((const char*)pr.q_rope + ((int64_t)b * p.R + r0) * (ROPED * 2)), (short)0,
        min(32, p.R - r0) * (ROPED * 2), 0x00020000);
    return __builtin_bit_cast(
        i16x8, __builtin_amdgcn_raw_buffer_load_b128(qrs, l32 * (ROPED * 2) + 32 * wave + 16 * hh,
                                                     0, 0));
  };

  // Block-table entry of the tile at key t (uniform), as stored; the lookup stays in the
  // sequence's table row (the look-ahead runs past the last tile).
  const rw8_i32_ptr trow = (rw8_i32_ptr)pg.block_table + (int64_t)b * pg.max_pages;
  auto entry = [&](int t) { return trow[min(t >> pg.lg_page, pg.max_pages - 1)]; };
  const int pmask = (1 << pg.lg_page) - 1;
  // A tile is one buffer over its page rows below len_b (up to the last such row's end): a
  // 16-byte load of a row at or past len_b lies outside it and returns zeros without a fetch.
  // The token strides are below 2^24 bytes, so a tile's row offsets fit the 32-bit buffer offset.
  // The lane offsets of the staging loads and stores are formed where they are used, from a
  // thread id the compiler cannot see through: kept across the tile's arithmetic they are a
  // dozen loop-invariant registers the latent 512 instantiations do not have.
  auto fresh_tid = [&]() {
    int x = tid;
    asm volatile("" : "+v"(x));
    return x;
  };
  const int tokb = (int)pp.tok_bytes;
  const int vstep = RPP * tokb;                              // pass i: row tid / CPR + i·RPP
  const int rtokb = (int)pr.rope_tok_bytes;
  const int roff = l32 * rtokb + 32 * wave + 16 * hh;        // key row l32, elements 16w + 8hh
  // One tile in registers: its bytes and, in lane l, the scale of its row l & 31.
  struct Stage {
    uint4 q[CPT];
    float sc;
  };
  Stage sg[PF];
  // The rope rows of the tile at key t in page entry `ent`: the same page and slots under the
  // rope strides, the same row count.
  auto rope_rsrc = [&](int t, int ent, bool wanted) {
    const int page = min(max(ent, 0), pg.num_pages - 1);
    const char* const base = (const char*)pr.rope + (int64_t)page * pr.rope_page_bytes +
                             (int64_t)(t & pmask) * pr.rope_tok_bytes;
    const int rows = wanted ? min(len - t, BK) : 0;   // 0: an empty buffer, nothing is fetched
    const int nb = rows > 0 ? (rows - 1) * rtokb + ROPED * 2 : 0;
    return __builtin_amdgcn_make_buffer_rsrc((void*)base, (short)0, nb, 0x00020000);
  };
  auto rope_load = [&](__amdgpu_buffer_rsrc_t rs) {
    return __builtin_bit_cast(i16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, roff, 0, 0));
  };
  // Tile t < len_b: the bytes of its rows below len_b and their scale entries, nothing else.
  auto load = [&](Stage& g, int t, int ent) {
    const int page = min(max(ent, 0), pg.num_pages - 1);
    const int slot = t & pmask;
    const char* const base = (const char*)p.lat + (int64_t)page * pg.page_bytes +
                             (int64_t)slot * pp.tok_bytes;
    const int rows = min(len - t, BK);
    const int nb = (rows - 1) * tokb + LAT;
    const int ft = fresh_tid();
    const int voff0 = (ft / CPR) * tokb + 16 * (ft % CPR);
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
          (void*)(base + i * vstep), (short)0, max(nb - i * vstep, 0), 0x00020000);
      g.q[i] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff0, 0, 0));
    }
    const __amdgpu_buffer_rsrc_t ss = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(pw.scales + (int64_t)page * pw.sc_page + slot), (short)0, rows * 4, 0x00020000);
    g.sc = __builtin_bit_cast(float,
                              __builtin_amdgcn_raw_buffer_load_b32(ss, 4 * (ft & 31), 0, 0));
  };
  // E(scale · q) of the staged bytes into the tile image: 16 elements, two LDS chunks per load.
  auto store = [&](const Stage& g, char* tile) {
    const int ft = fresh_tid();
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      const int row = ft / CPR + i * RPP, ch = 2 * (ft % CPR);
      const float rsc = __shfl(g.sc, row);
      const float nbias = -128.f * rsc;
      const uint32_t src[4] = {g.q[i].x, g.q[i].y, g.q[i].z, g.q[i].w};
      uint32_t w[8];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t u = src[k] ^ 0x80808080u;   // q + 128 in every byte
        float x[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          x[e] = __builtin_fmaf((float)((u >> (8 * e)) & 0xffu), rsc, nbias);
          asm("" : "+v"(x[e]));
        }
        w[2 * k] = (uint32_t)E::from_f32(x[0]) | ((uint32_t)E::from_f32(x[1]) << 16);
        w[2 * k + 1] = (uint32_t)E::from_f32(x[2]) | ((uint32_t)E::from_f32(x[3]) << 16);
      }
      *reinterpret_cast<uint4*>(tile + TT::off(row, ch)) = make_uint4(w[0], w[1], w[2], w[3]);
      *reinterpret_cast<uint4*>(tile + TT::off(row, ch + 1)) = make_uint4(w[4], w[5], w[6], w[7]);
    }
  };

  f32x16 o[ND];
#pragma unroll
  for (int dt = 0; dt < ND; ++dt) o[dt] = zero16();
  float m = -kFltMax, lh = 0.f;
  const float c = p.c_log2;

  // en[k]: the entry of the tile k + 1 tiles ahead of the one being computed.
  int en[PF + 1];
#pragma unroll
  for (int k = 0; k <= PF; ++k) en[k] = 0;
  // The rope operands of the tile about to be computed (ROPE).
  i16x8 krf = i16x8{0, 0, 0, 0, 0, 0, 0, 0}, qrf = krf;
  if (kbeg < kend) {
    const int ent = entry(kbeg);
    load(sg[0], kbeg, ent);
#pragma unroll
    for (int k = 0; k <= PF; ++k) en[k] = entry(kbeg + (k + 1) * BK);
    if constexpr (ROPE) {
      krf = rope_load(rope_rsrc(kbeg, ent, true));
      qrf = qrope_load();
    }
    // Distance 2: the second tile is in flight before the first is stored.
    if constexpr (PF == 2)
      if (kbeg + BK < kend) load(sg[1], kbeg + BK, en[0]);
    store(sg[0], tb0);
  }
  __syncthreads();
  int cur = 0;
  for (int t0 = kbeg; t0 < kend; t0 += 2 * BK) {
    {
      const int t = t0;
#define RW8_HOLD sg[PF - 1]
#define RW8_FILL sg[0]
#include "mla_latent_rw8_step.h"
    }
    if (t0 + BK >= kend) break;
    {
      const int t = t0 + BK;
#define RW8_HOLD sg[0]
#define RW8_FILL sg[PF - 1]
#include "mla_latent_rw8_step.h"
    }
  }

  // Partial state of this key split: Õ unnormalised, (m, l) for the merge pass; the empty state
  // for a row that saw no key here.
  float lp = cross_half_sum(lh);
  if (klim < kbeg) {
    m = -kFltMax;
    lp = 0.f;
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) o[dt] = zero16();
  }
  if (!rvalid) return;
  // The store addresses, too, are formed here and not ahead of the loop.
  const int et = fresh_tid();
  const int ew = et >> 6, eh = (et >> 5) & 1;
  const int64_t prow = ((int64_t)b * p.nsplit + split) * p.R + r0 + (et & 31);
  float* op = p.opart + prow * LAT + ew * WS;
#pragma unroll
  for (int dt = 0; dt < ND; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *reinterpret_cast<float4*>(op + dt * 32 + 8 * g + 4 * eh) =
          make_float4(o[dt][4 * g], o[dt][4 * g + 1], o[dt][4 * g + 2], o[dt][4 * g + 3]);
  if (ew == 0 && eh == 0) p.mlpart[prow] = make_float2(m, lp);
}

// The row-wise route: this kernel's partials from every split, then the 16-bit calls' merge.
template <class E, int LAT, bool ROPE>
static hipError_t launch_latent_paged_rw8(const LatentPagedRw8Params& p, hipStream_t stream) {
  constexpr int LDS = 2 * 32 * LAT * 2 + 4 * 64 * 16 * 4;
  const LatentParams& l = p.r.c.l;
  if (!l.opart || !l.mlpart || !l.wv || l.nsplit < 1 || !p.scales ||
      (ROPE && (!p.r.rope || !p.r.q_rope)))
    return hipErrorInvalidValue;
  hipError_t e = launch(mfa_mla_latent_paged_rw8_kernel<E, LAT, ROPE>,
                        dim3(l.nblk * l.B * l.nsplit), dim3(256), LDS, stream, p);
  if (e != hipSuccess) return e;
  return mla_latent_merge_dispatch(l, E::prec, LAT, stream);
}

template <class E, int LAT>
static hipError_t launch_latent_paged_rw8(const LatentPagedRw8Params& p, bool rope,
                                          hipStream_t stream) {
  return rope ? launch_latent_paged_rw8<E, LAT, true>(p, stream)
              : launch_latent_paged_rw8<E, LAT, false>(p, stream);
}

hipError_t mla_latent_paged_rw8_dispatch(const LatentPagedRw8Params& p, bool rope, int elem,
                                         int lat, hipStream_t stream) {
  if (lat == 512 && elem == P_FP16) return launch_latent_paged_rw8<F16, 512>(p, rope, stream);
  if (lat == 512 && elem == P_BF16) return launch_latent_paged_rw8<BF16, 512>(p, rope, stream);
  if (lat == 256 && elem == P_FP16) return launch_latent_paged_rw8<F16, 256>(p, rope, stream);
  if (lat == 256 && elem == P_BF16) return launch_latent_paged_rw8<BF16, 256>(p, rope, stream);
  return hipErrorNotSupported;
}

}  // namespace mfa
