// attention_mla_latent.hip — attention in the MLA latent space (the absorbed form of
// MLAOptimizedGEMMMFA, MLAOptimizedGEMMMFA.swift:158-240).
//
// The decompress path computes K_h = latent·W_k,h and V_h = latent·W_v,h, then attends per
// head.  Since Q_h·K_hᵀ = (Q_h·W_k,hᵀ)·latentᵀ and P·V_h = (P·latent)·W_v,h, the same result
// comes from
//     Q̃_h = Q_h·W_k,hᵀ                        (general GEMM, B transposed)
//     Õ_h = softmax(scale·Q̃_h·latentᵀ)·latent (this kernel: every head attends to ONE
//                                               [S_kv, LAT] latent, used as both K and V)
//     O_h = Õ_h·W_v,h                          (16-bit GEMM)
// with the softmax scale of the decompressed head dimension.  K/V are never materialised;
// the latent is read once per query block instead of two [S_kv, H·D] tensors.
//
// Kernel structure: all heads share the latent, so query rows of every head of a batch item
// are one flattened [H·S_q, LAT] problem (MQA with a single KV head).  A workgroup is 4 waves
// on 32 query rows; wave w owns latent dims [w·LAT/4, (w+1)·LAT/4) of both products:
//   * Sᵀ_w = latent[:, slice]·Q̃[:, slice]ᵀ on MFMA (key on the register, query on the lane),
//   * the four partial Sᵀ are summed through LDS (fixed order, so every wave holds the same
//     bits and runs the same online softmax),
//   * Õᵀ_w += latent[:, slice]ᵀ·Pᵀ with the latent tile read transposed (ds_read_b64_tr_b16).
// MFMA work is not duplicated; the cost is the partial-S exchange (16 KiB of LDS per tile).
// Latent tiles of 32 keys are register-staged into a double-buffered [32][LAT] LDS image.
// Softmax semantics are the reference forward's (AttentionKernel+Softmax.swift:641-892):
// base-2 online softmax, masked keys at (0.875/log2 e)·(−FLT_MAX) (causal) or −inf (past S_kv),
// L = m + log2 l.  Õ is written in the 16-bit element type for the final 16-bit GEMM.
#include "mfa_stage.h"
#include "mfa_dispatch.h"

namespace mfa {

template <class E, int LAT>
__global__ void __launch_bounds__(256, 2) mfa_mla_latent_kernel(LatentParams p) {
  constexpr int BK = 32, NT = 256;
  constexpr int WS = LAT / 4;              // latent dims per wave
  constexpr int DS = WS / 16;              // MFMA k-steps of the wave's QK^T slice
  constexpr int ND = WS / 32;              // O^T tiles per wave
  constexpr int CPR = LAT / 8;             // 16-byte chunks per latent row
  constexpr int CPT = BK * CPR / NT;       // chunks staged per thread
  constexpr int TILEB = BK * LAT * 2;
  constexpr int XST = 16;                  // floats per lane in the exchange area
  using A = Arith16<E, LAT>;
  using TT = Tile16<LAT>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const tb0 = smem;                              // 2 latent tiles
  float* const xb = reinterpret_cast<float*>(smem + 2 * TILEB);  // [4 waves][64 lanes][XST]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l32 = lane & 31, hh = lane >> 5;
  const int split = blockIdx.x % p.nsplit;
  const int bq = blockIdx.x / p.nsplit;
  const int b = bq / p.nblk;
  const int r0 = (bq % p.nblk) * 32;
  const int r = r0 + l32;
  const bool rvalid = r < p.R;
  const int spos = rvalid ? r % p.Sq : 0;   // query position of the row (causal)

  // Keys this block needs: all of S_kv, or up to the largest query position it holds.
  int kend = p.Skv;
  if (p.causal) {
    const int rl = min(r0 + 31, p.R - 1);
    const int smax = (r0 / p.Sq == rl / p.Sq) ? rl % p.Sq : p.Sq - 1;
    kend = min(kend, smax + 1);
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

  const uint16_t* lat = (const uint16_t*)p.lat + (int64_t)b * p.Skv * LAT;
  uint4 stg[CPT];
  auto load = [&](int t) {
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      const int id = tid + NT * i;
      const int row = id / CPR, ch = id % CPR;
      stg[i] = (t + row < p.Skv)
                   ? *reinterpret_cast<const uint4*>(lat + (int64_t)(t + row) * LAT + 8 * ch)
                   : make_uint4(0u, 0u, 0u, 0u);
    }
  };
  auto store = [&](char* tile) {
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      const int id = tid + NT * i;
      *reinterpret_cast<uint4*>(tile + TT::off(id / CPR, id % CPR)) = stg[i];
    }
  };

  f32x16 o[ND];
#pragma unroll
  for (int dt = 0; dt < ND; ++dt) o[dt] = zero16();
  float m = -kFltMax, lh = 0.f;
  const float c = p.c_log2;

  if (kbeg < kend) {
    load(kbeg);
    store(tb0);
  }
  __syncthreads();
  int cur = 0;
  for (int t = kbeg; t < kend; t += BK) {
    const bool has_next = t + BK < kend;
    if (has_next) load(t + BK);
    const char* kt = tb0 + cur * TILEB;

    // The tile's arithmetic, shared as text with the two paged kernels below.
#define MLA_TILE_LEN p.Skv
#define MLA_TILE_KLIM spos
#include "mla_latent_tile_body.h"
    if (has_next) store(tb0 + (cur ^ 1) * TILEB);
    __syncthreads();
    cur ^= 1;
  }

  if (p.nsplit > 1) {
    // Partial state of this key split: Õ unnormalised, (m, l) for the merge pass.
    const float lp = cross_half_sum(lh);
    if (!rvalid) return;
    const int64_t prow = ((int64_t)b * p.nsplit + split) * p.R + r;
    float* op = p.opart + prow * LAT + wave * WS;
#pragma unroll
    for (int dt = 0; dt < ND; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *reinterpret_cast<float4*>(op + dt * 32 + 8 * g + 4 * hh) =
            make_float4(o[dt][4 * g], o[dt][4 * g + 1], o[dt][4 * g + 2], o[dt][4 * g + 3]);
    if (wave == 0 && hh == 0) p.mlpart[prow] = make_float2(m, lp);
    return;
  }
  float l = cross_half_sum(lh) + kFltMin;
  if (!(l > 0.f)) l = kFltMin;
  if (!rvalid) return;
  const float inv = 1.f / l;
  uint16_t* orow = (uint16_t*)p.olat + ((int64_t)b * p.R + r) * LAT + wave * WS;
#pragma unroll
  for (int dt = 0; dt < ND; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int d = dt * 32 + 8 * g + 4 * hh;
      ushort4 v;
      v.x = E::from_f32(o[dt][4 * g] * inv);
      v.y = E::from_f32(o[dt][4 * g + 1] * inv);
      v.z = E::from_f32(o[dt][4 * g + 2] * inv);
      v.w = E::from_f32(o[dt][4 * g + 3] * inv);
      *reinterpret_cast<ushort4*>(orow + d) = v;
    }
  if (wave == 0 && hh == 0 && p.l) {
    const float L = m + __log2f(l);
    const int64_t li = (int64_t)b * p.R + r;
    if (p.l_f16)
      reinterpret_cast<uint16_t*>(p.l)[li] = f32_to_f16(L);
    else
      reinterpret_cast<float*>(p.l)[li] = L;
  }
}

// The same tile body over a paged latent cache (mfa_paged_mla_decode_forward; PagedKv's
// conventions, one [page][LAT] row set per page).  What differs from the kernel above:
//   * len_b = clamp(seq_lens[b], 0, p.Skv) is a device value, loaded once per workgroup on the
//     scalar path; p.Skv is the host-side cap that sized the split;
//   * key tiles start at multiples of 32 counted from key 0 (chunk is a multiple of 32 whenever
//     there is more than one split), so a tile lies in one page: one block-table entry (lookup
//     clamped to the sequence's row, id clamped to the pool) and one 64-bit base per tile, the
//     next tile's entry fetched a tile ahead of its loads; rows at or past len_b are zeros and are
//     not fetched;
//   * causal is the KV-cache convention: row q of the Sq rows of a head attends to keys
//     j <= klim = len_b − Sq + q (unmasked: klim = len_b − 1);
//   * a row with no visible key in this split (klim < kbeg: every row of an empty sequence, the
//     leading causal rows of a sequence shorter than Sq, rows whose keys end before the split)
//     leaves the empty state (m = −FLT_MAX, l = 0, Õ = 0) — with the finite causal mask value it
//     would otherwise carry a uniform average — so a row dead in every split merges to exact
//     zeros and L at its floor;
//   * always the split route: every workgroup writes its partial state, also with one split and
//     also when it has no key (the scratch is not initialised); the merge applies W_v.
typedef const __attribute__((address_space(4))) int32_t* latent_i32_ptr;

template <class E, int LAT>
__global__ void __launch_bounds__(256, 2) mfa_mla_latent_paged_kernel(LatentPagedParams pp) {
  constexpr int BK = 32, NT = 256;
  constexpr int WS = LAT / 4;              // latent dims per wave
  constexpr int DS = WS / 16;              // MFMA k-steps of the wave's QK^T slice
  constexpr int ND = WS / 32;              // O^T tiles per wave
  constexpr int CPR = LAT / 8;             // 16-byte chunks per latent row
  constexpr int CPT = BK * CPR / NT;       // chunks staged per thread
  constexpr int TILEB = BK * LAT * 2;
  constexpr int XST = 16;                  // floats per lane in the exchange area
  using A = Arith16<E, LAT>;
  using TT = Tile16<LAT>;
  const LatentParams& p = pp.l;
  const PagedKv& pg = pp.pg;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const tb0 = smem;                              // 2 latent tiles
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
  const int len = min(max(((latent_i32_ptr)pg.seq_lens)[b], 0), p.Skv);
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

  // Block-table entry of the tile at key t (uniform), as stored; the lookup stays in the
  // sequence's table row (the look-ahead runs past the last tile).
  const latent_i32_ptr trow = (latent_i32_ptr)pg.block_table + (int64_t)b * pg.max_pages;
  auto entry = [&](int t) { return trow[min(t >> pg.lg_page, pg.max_pages - 1)]; };
  const int pmask = (1 << pg.lg_page) - 1;
  // A tile is one buffer over its page rows below len_b (up to the last such row's end): a
  // 16-byte load of a row at or past len_b lies outside it and returns zeros without a fetch.
  // The token stride is below 2^24 bytes, so a tile's row offsets fit the 32-bit buffer offset.
  const int tokb = (int)pp.tok_bytes;
  const int voff0 = (tid / CPR) * tokb + 16 * (tid % CPR);   // chunk i: row tid / CPR + i·NT / CPR
  const int vstep = (NT / CPR) * tokb;
  uint4 stg[CPT];
  auto load = [&](int t, int ent) {
    const int page = min(max(ent, 0), pg.num_pages - 1);
    const char* const base = (const char*)p.lat + (int64_t)page * pg.page_bytes +
                             (int64_t)(t & pmask) * pp.tok_bytes;
    const int nb = (min(len - t, BK) - 1) * tokb + LAT * 2;
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc((void*)base, (short)0, nb, 0x00020000);
#pragma unroll
    for (int i = 0; i < CPT; ++i)
      stg[i] = __builtin_bit_cast(
          uint4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff0 + i * vstep, 0, 0));
  };
  auto store = [&](char* tile) {
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      const int id = tid + NT * i;
      *reinterpret_cast<uint4*>(tile + TT::off(id / CPR, id % CPR)) = stg[i];
    }
  };

  f32x16 o[ND];
#pragma unroll
  for (int dt = 0; dt < ND; ++dt) o[dt] = zero16();
  float m = -kFltMax, lh = 0.f;
  const float c = p.c_log2;

  int ent_next = 0;
  if (kbeg < kend) {
    load(kbeg, entry(kbeg));
    store(tb0);
    ent_next = entry(kbeg + BK);
  }
  __syncthreads();
  int cur = 0;
  for (int t = kbeg; t < kend; t += BK) {
    const bool has_next = t + BK < kend;
    if (has_next) load(t + BK, ent_next);
    ent_next = entry(t + 2 * BK);
    const char* kt = tb0 + cur * TILEB;

#define MLA_TILE_LEN len
#define MLA_TILE_KLIM klim
#include "mla_latent_tile_body.h"
    if (has_next) store(tb0 + (cur ^ 1) * TILEB);
    __syncthreads();
    cur ^= 1;
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
  const int64_t prow = ((int64_t)b * p.nsplit + split) * p.R + r;
  float* op = p.opart + prow * LAT + wave * WS;
#pragma unroll
  for (int dt = 0; dt < ND; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *reinterpret_cast<float4*>(op + dt * 32 + 8 * g + 4 * hh) =
          make_float4(o[dt][4 * g], o[dt][4 * g + 1], o[dt][4 * g + 2], o[dt][4 * g + 3]);
  if (wave == 0 && hh == 0) p.mlpart[prow] = make_float2(m, lp);
}

// Ragged prompt chunks over the paged latent cache (mfa_paged_mla_prefill_forward): the paged
// kernel's staging and addressing, the dense kernel's non-split epilogue (l += FLT_MIN, Õ
// normalised and rounded to E, L = m + log2 l), and rows that differ per sequence:
//   * n_b = new_lens ? clamp(new_lens[b], 0, Sq) : Sq is a second scalar load; row q < n_b of a
//     head's Sq rows is key position len_b − n_b + q, the slot the latent append wrote;
//   * a row is live iff q < n_b and that position is >= 0; its limit klim is the position
//     (causal) or len_b − 1 (unmasked), and a dead row carries klim = −1, so liveness costs no
//     register of its own;
//   * the Q̃ fragments of a dead row are zeros and are never loaded (the projection of an unused
//     query row may be NaN); what the tile body makes of them is replaced at the store by zero Õ
//     — the output GEMM then gives an exact-zero O row — and L at its floor;
//   * the key loop ends at the largest limit among the block's live rows: the neighbours' smax
//     logic with n_b − 1 in place of Sq − 1; a block with no live row has no key, so it loads no
//     latent row and stores the dead result;
//   * no split: one workgroup per 32-row block runs all of the block's keys.
template <class E, int LAT>
__global__ void __launch_bounds__(256, 2) mfa_mla_latent_prefill_kernel(LatentPrefillParams pp) {
  constexpr int BK = 32, NT = 256;
  constexpr int WS = LAT / 4;              // latent dims per wave
  constexpr int DS = WS / 16;              // MFMA k-steps of the wave's QK^T slice
  constexpr int ND = WS / 32;              // O^T tiles per wave
  constexpr int CPR = LAT / 8;             // 16-byte chunks per latent row
  constexpr int CPT = BK * CPR / NT;       // chunks staged per thread
  constexpr int TILEB = BK * LAT * 2;
  constexpr int XST = 16;                  // floats per lane in the exchange area
  using A = Arith16<E, LAT>;
  using TT = Tile16<LAT>;
  const LatentParams& p = pp.c.l;
  const PagedKv& pg = pp.c.pg;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const tb0 = smem;                              // 2 latent tiles
  float* const xb = reinterpret_cast<float*>(smem + 2 * TILEB);  // [4 waves][64 lanes][XST]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l32 = lane & 31, hh = lane >> 5;
  const int b = blockIdx.x / p.nblk;
  const int r0 = (blockIdx.x % p.nblk) * 32;
  const int r = r0 + l32;
  const bool rvalid = r < p.R;

  // The sequence's keys and rows (uniform), and the last key this row sees (-1: a dead row).
  const int len = min(max(((latent_i32_ptr)pg.seq_lens)[b], 0), p.Skv);
  const int nrow = pp.new_lens ? min(max(((latent_i32_ptr)pp.new_lens)[b], 0), p.Sq) : p.Sq;
  const int first = len - nrow;             // key position of the head's row 0
  int klim = -1;
  {
    const int spos = r % p.Sq;              // the row's index among its head's Sq rows
    if (rvalid && spos < nrow && first + spos >= 0) klim = p.causal ? first + spos : len - 1;
  }

  // Keys this block needs: none without a live row (every wave holds the same 32 rows, so the
  // vote is the workgroup's); else all of the sequence, or up to its live rows' largest limit.
  int kend = 0;
  if (__builtin_amdgcn_ballot_w64(klim >= 0) != 0) {
    kend = len;
    if (p.causal) {
      const int rl = min(r0 + 31, p.R - 1);
      const int smax = (r0 / p.Sq == rl / p.Sq) ? min(rl % p.Sq, nrow - 1) : nrow - 1;
      kend = min(kend, first + smax + 1);
    }
  }

  // Q̃ fragments of the wave's slice: d = w·WS + 16·ds + 8·hh + j.
  i16x8 qf[DS];
  {
    const uint16_t* qrow = (const uint16_t*)p.q + ((int64_t)b * p.R + (rvalid ? r : 0)) * LAT;
#pragma unroll
    for (int ds = 0; ds < DS; ++ds) {
      i16x8 v = i16x8{0, 0, 0, 0, 0, 0, 0, 0};
      if (klim >= 0) v = *reinterpret_cast<const i16x8*>(qrow + wave * WS + 16 * ds + 8 * hh);
      qf[ds] = v;
    }
  }

  // Block-table entry of the tile at key t (uniform), as stored; the lookup stays in the
  // sequence's table row (the look-ahead runs past the last tile).
  const latent_i32_ptr trow = (latent_i32_ptr)pg.block_table + (int64_t)b * pg.max_pages;
  auto entry = [&](int t) { return trow[min(t >> pg.lg_page, pg.max_pages - 1)]; };
  const int pmask = (1 << pg.lg_page) - 1;
  // A tile is one buffer over its page rows below len_b (up to the last such row's end): a
  // 16-byte load of a row at or past len_b lies outside it and returns zeros without a fetch.
  // The token stride is below 2^24 bytes, so a tile's row offsets fit the 32-bit buffer offset.
  const int tokb = (int)pp.c.tok_bytes;
  const int voff0 = (tid / CPR) * tokb + 16 * (tid % CPR);   // chunk i: row tid / CPR + i·NT / CPR
  const int vstep = (NT / CPR) * tokb;
  uint4 stg[CPT];
  auto load = [&](int t, int ent) {
    const int page = min(max(ent, 0), pg.num_pages - 1);
    const char* const base = (const char*)p.lat + (int64_t)page * pg.page_bytes +
                             (int64_t)(t & pmask) * pp.c.tok_bytes;
    const int nb = (min(len - t, BK) - 1) * tokb + LAT * 2;
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc((void*)base, (short)0, nb, 0x00020000);
#pragma unroll
    for (int i = 0; i < CPT; ++i)
      stg[i] = __builtin_bit_cast(
          uint4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff0 + i * vstep, 0, 0));
  };
  auto store = [&](char* tile) {
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      const int id = tid + NT * i;
      *reinterpret_cast<uint4*>(tile + TT::off(id / CPR, id % CPR)) = stg[i];
    }
  };

  f32x16 o[ND];
#pragma unroll
  for (int dt = 0; dt < ND; ++dt) o[dt] = zero16();
  float m = -kFltMax, lh = 0.f;
  const float c = p.c_log2;

  int ent_next = 0;
  if (0 < kend) {
    load(0, entry(0));
    store(tb0);
    ent_next = entry(BK);
  }
  __syncthreads();
  int cur = 0;
  for (int t = 0; t < kend; t += BK) {
    const bool has_next = t + BK < kend;
    if (has_next) load(t + BK, ent_next);
    ent_next = entry(t + 2 * BK);
    const char* kt = tb0 + cur * TILEB;

#define MLA_TILE_LEN len
#define MLA_TILE_KLIM klim
#include "mla_latent_tile_body.h"
    if (has_next) store(tb0 + (cur ^ 1) * TILEB);
    __syncthreads();
    cur ^= 1;
  }

  float l = cross_half_sum(lh) + kFltMin;
  if (!(l > 0.f)) l = kFltMin;
  if (!rvalid) return;
  const bool live = klim >= 0;
  const float inv = 1.f / l;
  uint16_t* orow = (uint16_t*)p.olat + ((int64_t)b * p.R + r) * LAT + wave * WS;
#pragma unroll
  for (int dt = 0; dt < ND; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int d = dt * 32 + 8 * g + 4 * hh;
      // The product rounded to FP32 and then to E, as the dense kernel's separate multiply and
      // convert do: next to the select hipcc otherwise fuses the two into v_fma_mixlo_f16, one
      // rounding of the exact product, and the two calls disagree at FP16 ties.
      float x[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        x[e] = o[dt][4 * g + e] * inv;
        asm("" : "+v"(x[e]));
      }
      ushort4 v;
      v.x = E::from_f32(x[0]);
      v.y = E::from_f32(x[1]);
      v.z = E::from_f32(x[2]);
      v.w = E::from_f32(x[3]);
      if (!live) v = make_ushort4(0, 0, 0, 0);
      *reinterpret_cast<ushort4*>(orow + d) = v;
    }
  if (wave == 0 && hh == 0 && p.l) {
    const float L = live ? m + __log2f(l) : -kFltMax;
    const int64_t li = (int64_t)b * p.R + r;
    if (p.l_f16)
      reinterpret_cast<uint16_t*>(p.l)[li] = f32_to_f16(L);
    else
      reinterpret_cast<float*>(p.l)[li] = L;
  }
}

// Merge of the key splits (flash-decoding): M = max m_s, w_s = exp2(m_s − M),
// Õ = Σ w_s Õ_s / Σ w_s l_s, L = M + log2 Σ w_s l_s.  MNB rows (the same query row r of MNB
// consecutive batch items) per 256-thread workgroup, launched with MNB = 1.  The split states
// are combined per row into an FP32 Õ row image in LDS; with W_v, the projection then reads
// each W_v element once for the workgroup's rows, the latent dimension split over 16 k groups.
constexpr int MNT = 256;

template <class E, int LAT, int MNB>
__global__ void __launch_bounds__(MNT) mfa_mla_latent_merge_kernel(LatentParams p) {
  constexpr int TPR = LAT / 4;        // threads per row in the combine step (4 dims each)
  constexpr int RPI = MNT / TPR;      // rows combined per iteration
  // Õ rows [MNB][LAT], then (projection) 16 k groups' partial sums [16][MNB][128].
  __shared__ __attribute__((aligned(16))) float smf[MNB * LAT + 16 * MNB * 128];
  float (*orow)[LAT] = reinterpret_cast<float (*)[LAT]>(smf);
  const int r = blockIdx.x % p.R;
  const int b0 = (blockIdx.x / p.R) * MNB;
  const int tid = threadIdx.x;
  const int d = 4 * (tid % TPR);
  for (int nb = tid / TPR; nb < MNB; nb += RPI) {
    const int b = b0 + nb;
    if (b >= p.B) break;
    // SU splits' loads in flight at a time (a one-split-at-a-time loop is a chain of HBM
    // latencies), merged online: running max M, rescaled sum l and Õ accumulator.
    constexpr int SU = 16;
    float M = -kFltMax;
    float l = 0.f;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int s0 = 0; s0 < p.nsplit; s0 += SU) {
      float2 ml[SU];
      float4 x[SU];
#pragma unroll
      for (int u = 0; u < SU; ++u) {
        ml[u] = make_float2(-kFltMax, 0.f);
        x[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (s0 + u < p.nsplit) {
          const int64_t prow = ((int64_t)b * p.nsplit + s0 + u) * p.R + r;
          ml[u] = p.mlpart[prow];
          x[u] = *reinterpret_cast<const float4*>(p.opart + prow * LAT + d);
        }
      }
      float Mc = M;
#pragma unroll
      for (int u = 0; u < SU; ++u) Mc = fmaxf(Mc, ml[u].x);
      const float cr = __builtin_amdgcn_exp2f(M - Mc);
      M = Mc;
      l *= cr;
      acc.x *= cr; acc.y *= cr; acc.z *= cr; acc.w *= cr;
#pragma unroll
      for (int u = 0; u < SU; ++u) {
        const float w = __builtin_amdgcn_exp2f(ml[u].x - M);
        l += w * ml[u].y;
        acc.x += w * x[u].x; acc.y += w * x[u].y; acc.z += w * x[u].z; acc.w += w * x[u].w;
      }
    }
    l += kFltMin;
    if (!(l > 0.f)) l = kFltMin;
    const float inv = 1.f / l;
    const int64_t row = (int64_t)b * p.R + r;
    if (p.wv) {
      *reinterpret_cast<float4*>(&orow[nb][d]) =
          make_float4(acc.x * inv, acc.y * inv, acc.z * inv, acc.w * inv);
    } else {
      ushort4 v;
      v.x = E::from_f32(acc.x * inv);
      v.y = E::from_f32(acc.y * inv);
      v.z = E::from_f32(acc.z * inv);
      v.w = E::from_f32(acc.w * inv);
      *reinterpret_cast<ushort4*>((uint16_t*)p.olat + row * LAT + d) = v;
    }
    if (d == 0 && p.l) {
      const float L = M + __log2f(l);
      if (p.l_f16)
        reinterpret_cast<uint16_t*>(p.l)[row] = f32_to_f16(L);
      else
        reinterpret_cast<float*>(p.l)[row] = L;
    }
  }
  if (!p.wv) return;
  __syncthreads();
  // Fused output projection O[b, r, :] = Õ[b, r, :]·W_v[:, h·D : (h+1)·D], per 128-dim chunk:
  // lane group dg (16 lanes) x k group kg (16 per workgroup) — each thread loads 8 consecutive
  // W_v dims (16 B) for LAT/16 latent rows, all loads independent, and keeps 8 x MNB partial
  // sums; the 16 k groups are summed through LDS.
  const int nbv = min(MNB, p.B - b0);
  const int hq = r / p.Sq;
  const uint16_t* w = (const uint16_t*)p.wv + (int64_t)hq * p.D;
  const int64_t ldw = (int64_t)p.H * p.D;
  const bool vec = (p.D % 8) == 0 && (ldw % 8) == 0 && ((uintptr_t)p.wv % 16) == 0;
  const int dg = tid & 15, kg = tid >> 4;
  constexpr int KPG = LAT / 16;
  float* red = smf + MNB * LAT;  // [16 k groups][MNB][128]
  for (int dd0 = 0; dd0 < p.D; dd0 += 128) {
    float acc[MNB][8];
#pragma unroll
    for (int nb = 0; nb < MNB; ++nb)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[nb][j] = 0.f;
    const int dd = dd0 + 8 * dg;
    if (dd < p.D) {
#pragma unroll 16
      for (int kk = 0; kk < KPG; ++kk) {
        const int k = kg * KPG + kk;
        const uint16_t* wr = w + (int64_t)k * ldw + dd;
        float wf[8];
        if (vec) {
          const i16x8 w8 = *reinterpret_cast<const i16x8*>(wr);
#pragma unroll
          for (int j = 0; j < 8; ++j) wf[j] = E::to_f32((uint16_t)w8[j]);
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) wf[j] = dd + j < p.D ? E::to_f32(wr[j]) : 0.f;
        }
#pragma unroll
        for (int nb = 0; nb < MNB; ++nb) {
          const float o = orow[nb][k];
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[nb][j] = __builtin_fmaf(o, wf[j], acc[nb][j]);
        }
      }
    }
#pragma unroll
    for (int nb = 0; nb < MNB; ++nb)
#pragma unroll
      for (int j = 0; j < 8; j += 4)
        *reinterpret_cast<float4*>(red + (kg * MNB + nb) * 128 + 8 * dg + j) =
            make_float4(acc[nb][j], acc[nb][j + 1], acc[nb][j + 2], acc[nb][j + 3]);
    __syncthreads();
    for (int o = tid; o < MNB * 128; o += MNT) {
      const int nb = o >> 7, dl = o & 127;
      if (nb < nbv && dd0 + dl < p.D) {
        float sum = 0.f;
#pragma unroll
        for (int g2 = 0; g2 < 16; ++g2) sum += red[(g2 * MNB + nb) * 128 + dl];
        p.out[((int64_t)(b0 + nb) * p.R + r) * p.D + dd0 + dl] = sum;
      }
    }
    __syncthreads();
  }
}

template <class E, int LAT>
static hipError_t launch_latent(const LatentParams& p, hipStream_t stream) {
  constexpr int LDS = 2 * 32 * LAT * 2 + 4 * 64 * 16 * 4;
  auto kern = mfa_mla_latent_kernel<E, LAT>;
  hipError_t e = launch(kern, dim3(p.nblk * p.B * p.nsplit), dim3(256), LDS, stream, p);
  if (e != hipSuccess || p.nsplit <= 1) return e;
  // One row per workgroup measured fastest (B32 S_q 1: MNB 1/2/4 = 14.5/15.6/17.9 us): the
  // W_v re-reads per batch item come from L2.
  return launch(mfa_mla_latent_merge_kernel<E, LAT, 1>, dim3(p.B * p.R), dim3(MNT), 0, stream, p);
}

// The paged route: partials from every split, then the merge with W_v — also for one split.
template <class E, int LAT>
static hipError_t launch_latent_paged(const LatentPagedParams& p, hipStream_t stream) {
  constexpr int LDS = 2 * 32 * LAT * 2 + 4 * 64 * 16 * 4;
  const LatentParams& l = p.l;
  if (!l.opart || !l.mlpart || !l.wv || l.nsplit < 1) return hipErrorInvalidValue;
  hipError_t e = launch(mfa_mla_latent_paged_kernel<E, LAT>, dim3(l.nblk * l.B * l.nsplit),
                        dim3(256), LDS, stream, p);
  if (e != hipSuccess) return e;
  return launch(mfa_mla_latent_merge_kernel<E, LAT, 1>, dim3(l.B * l.R), dim3(MNT), 0, stream, l);
}

// The paged prefill: one launch, the latent-space output left in l.olat for the output GEMM.
template <class E, int LAT>
static hipError_t launch_latent_prefill(const LatentPrefillParams& p, hipStream_t stream) {
  constexpr int LDS = 2 * 32 * LAT * 2 + 4 * 64 * 16 * 4;
  const LatentParams& l = p.c.l;
  if (!l.q || !l.olat || l.Sq < 1 || l.nblk < 1) return hipErrorInvalidValue;
  return launch(mfa_mla_latent_prefill_kernel<E, LAT>, dim3(l.nblk * l.B), dim3(256), LDS, stream,
                p);
}

// Decode query projection Q̃[b, h, :] = q[b, h, :] · W_k[:, h·D : (h+1)·D]ᵀ (S_q = 1): a workgroup
// takes one head, QC latent columns and 32 batch rows; the W_k slice [QC][D] and the query rows
// [32][D] sit in LDS (rows padded by 16 B), each thread accumulates QC/8 columns of one row in
// FP32 over D.  Replaces a 128x128-tile GEMM launch whose 64 workgroups were mostly padding
// (M = B rows per head).
constexpr int QC = 16;
template <class E>
__global__ void __launch_bounds__(256) mfa_mla_qproj_kernel(const uint16_t* __restrict__ q,
                                                            const uint16_t* __restrict__ wk,
                                                            uint16_t* __restrict__ qt, int B,
                                                            int H, int D, int Lat) {
  constexpr int NJ = QC / 8;  // columns per thread
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int RS = D * 2 + 16;  // padded row stride (bytes)
  char* const wsl = smem;            // [QC][RS]
  char* const qsl = smem + QC * RS;  // [32][RS]
  const int h = blockIdx.x, l0 = blockIdx.y * QC, b0 = blockIdx.z * 32;
  const int tid = threadIdx.x;
  const int cpr = D / 8;  // 16-byte chunks per row
  for (int i = tid; i < QC * cpr; i += 256) {
    const int r = i / cpr, c = i % cpr;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (l0 + r < Lat)
      v = *reinterpret_cast<const uint4*>(wk + (int64_t)(l0 + r) * H * D + (int64_t)h * D + 8 * c);
    *reinterpret_cast<uint4*>(wsl + r * RS + 16 * c) = v;
  }
  for (int i = tid; i < 32 * cpr; i += 256) {
    const int r = i / cpr, c = i % cpr;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (b0 + r < B) v = *reinterpret_cast<const uint4*>(q + ((int64_t)(b0 + r) * H + h) * D + 8 * c);
    *reinterpret_cast<uint4*>(qsl + r * RS + 16 * c) = v;
  }
  __syncthreads();
  const int br = tid >> 3, lg = tid & 7;
  float acc[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) acc[j] = 0.f;
  for (int c = 0; c < cpr; ++c) {
    const uint4 qv = *reinterpret_cast<const uint4*>(qsl + br * RS + 16 * c);
    float qf[8];
    const uint32_t qw[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      qf[2 * e] = E::to_f32((uint16_t)(qw[e] & 0xffffu));
      qf[2 * e + 1] = E::to_f32((uint16_t)(qw[e] >> 16));
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const uint4 wv = *reinterpret_cast<const uint4*>(wsl + (lg * NJ + j) * RS + 16 * c);
      const uint32_t ww[4] = {wv.x, wv.y, wv.z, wv.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc[j] = __builtin_fmaf(qf[2 * e], E::to_f32((uint16_t)(ww[e] & 0xffffu)), acc[j]);
        acc[j] = __builtin_fmaf(qf[2 * e + 1], E::to_f32((uint16_t)(ww[e] >> 16)), acc[j]);
      }
    }
  }
  const int b = b0 + br;
  if (b >= B) return;
  uint16_t* orow = qt + ((int64_t)b * H + h) * Lat + l0 + lg * NJ;
#pragma unroll
  for (int j = 0; j < NJ; ++j)
    if (l0 + lg * NJ + j < Lat) orow[j] = E::from_f32(acc[j]);
}

hipError_t mla_qproj_dispatch(const void* q, const void* wk, void* qt, int B, int H, int D,
                              int Lat, int elem, hipStream_t stream) {
  if (D % 8 != 0 || D > 256 || ((uintptr_t)q & 15) || ((uintptr_t)wk & 15))
    return hipErrorNotSupported;
  const dim3 grid(H, (Lat + QC - 1) / QC, (B + 31) / 32);
  const size_t lds = (size_t)(QC + 32) * (D * 2 + 16);
  // Through launch(): the paged MLA plan lists this launch, and the launch log records it.
  if (elem == P_FP16)
    return launch(mfa_mla_qproj_kernel<F16>, grid, dim3(256), lds, stream, (const uint16_t*)q,
                  (const uint16_t*)wk, (uint16_t*)qt, B, H, D, Lat);
  if (elem == P_BF16)
    return launch(mfa_mla_qproj_kernel<BF16>, grid, dim3(256), lds, stream, (const uint16_t*)q,
                  (const uint16_t*)wk, (uint16_t*)qt, B, H, D, Lat);
  return hipErrorNotSupported;
}

hipError_t mla_latent_dispatch(const LatentParams& p, int elem, int lat, hipStream_t stream) {
  if (lat == 512 && elem == P_FP16) return launch_latent<F16, 512>(p, stream);
  if (lat == 512 && elem == P_BF16) return launch_latent<BF16, 512>(p, stream);
  if (lat == 256 && elem == P_FP16) return launch_latent<F16, 256>(p, stream);
  if (lat == 256 && elem == P_BF16) return launch_latent<BF16, 256>(p, stream);
  return hipErrorNotSupported;
}

hipError_t mla_latent_paged_dispatch(const LatentPagedParams& p, int elem, int lat,
                                     hipStream_t stream) {
  if (lat == 512 && elem == P_FP16) return launch_latent_paged<F16, 512>(p, stream);
  if (lat == 512 && elem == P_BF16) return launch_latent_paged<BF16, 512>(p, stream);
  if (lat == 256 && elem == P_FP16) return launch_latent_paged<F16, 256>(p, stream);
  if (lat == 256 && elem == P_BF16) return launch_latent_paged<BF16, 256>(p, stream);
  return hipErrorNotSupported;
}

hipError_t mla_latent_prefill_dispatch(const LatentPrefillParams& p, int elem, int lat,
                                       hipStream_t stream) {
  if (lat == 512 && elem == P_FP16) return launch_latent_prefill<F16, 512>(p, stream);
  if (lat == 512 && elem == P_BF16) return launch_latent_prefill<BF16, 512>(p, stream);
  if (lat == 256 && elem == P_FP16) return launch_latent_prefill<F16, 256>(p, stream);
  if (lat == 256 && elem == P_BF16) return launch_latent_prefill<BF16, 256>(p, stream);
  return hipErrorNotSupported;
}

template __global__ void mfa_mla_latent_prefill_kernel<F16, 512>(LatentPrefillParams);
template __global__ void mfa_mla_latent_prefill_kernel<BF16, 512>(LatentPrefillParams);
template __global__ void mfa_mla_latent_prefill_kernel<F16, 256>(LatentPrefillParams);
template __global__ void mfa_mla_latent_prefill_kernel<BF16, 256>(LatentPrefillParams);
template __global__ void mfa_mla_latent_paged_kernel<F16, 512>(LatentPagedParams);
template __global__ void mfa_mla_latent_paged_kernel<BF16, 512>(LatentPagedParams);
template __global__ void mfa_mla_latent_paged_kernel<F16, 256>(LatentPagedParams);
template __global__ void mfa_mla_latent_paged_kernel<BF16, 256>(LatentPagedParams);
template __global__ void mfa_mla_latent_kernel<F16, 512>(LatentParams);
template __global__ void mfa_mla_latent_merge_kernel<F16, 512, 1>(LatentParams);
template __global__ void mfa_mla_latent_merge_kernel<BF16, 512, 1>(LatentParams);
template __global__ void mfa_mla_latent_merge_kernel<F16, 256, 1>(LatentParams);
template __global__ void mfa_mla_latent_merge_kernel<BF16, 256, 1>(LatentParams);
template __global__ void mfa_mla_latent_kernel<BF16, 512>(LatentParams);
template __global__ void mfa_mla_latent_kernel<F16, 256>(LatentParams);
template __global__ void mfa_mla_latent_kernel<BF16, 256>(LatentParams);

}  // namespace mfa
