// attention_prefill_paged.hip — ragged, multi-row causal forward over the paged K/V cache
// (mfa_paged_prefill_forward; no reference counterpart): the attention step of a prompt, or a
// chunk of one, whose keys are already in the page pools (mfa_paged_kv_append wrote them) behind a
// prefix of earlier keys.  The read side's addressing is attention_decode.hip's (PagedKv), the
// tile body is the tuned 16-bit forward's (attention_fwd2.h: fwd2_tile, RowState, load_q2,
// store_o_l), unchanged.
//
// Rows and keys.  len_b = clamp(seq_lens[b], 0, cap) is the length AFTER the chunk was appended,
// n_b = new_lens ? clamp(new_lens[b], 0, R) : R the rows of sequence b in `query`.  Row q < n_b is
// key position t_q = len_b - n_b + q: causal rows attend to keys j <= t_q, unmasked rows to keys
// 0 .. len_b - 1.  Rows with no visible key (q >= n_b, t_q < 0, len_b == 0) get exact zeros and
// L = -FLT_MAX (-inf in FP16): every row of O and L is written whatever the device values are.
//
// One workgroup of 4 waves x 32 rows owns a 128-row query block of one (b, h).  What differs from
// mfa_fwd2_kernel (attention_fwd_v2.hip):
//   * len_b and n_b are scalar loads through the constant address space, once per workgroup; the
//     mask sees the lane's key position t_q, the stores its row q; the key bound is len_b (a local
//     copy of FwdParams with C = len_b);
//   * a workgroup whose block has no live row writes the dead-row result and leaves before any K/V
//     load;
//   * tiles start at absolute keys that are multiples of BK, counted from key 0, whatever the
//     page size: the order of the arithmetic, and so every bit of O and L, is the same for any
//     paging of the same keys;
//   * a tile is staged in 32-key segments (PagedDma): a page holds whole segments (page size a
//     power of two >= 32), so each segment has one page id, one base and one range-checked buffer
//     descriptor whose range ends at the rows below both len_b and the page's end — neither an
//     unused slot nor a foreign page is fetched, rows past the range land as zeros (and are masked);
//   * page ids are scalar loads from the block table issued one tile before their tile's DMA
//     (two before its compute), the lookup clamped to the table row and the id clamped to the
//     pools where it is used; all tile bookkeeping is wave-uniform.
// Causal: the key loop ends at the block's last visible key, and the grid runs the heaviest
// (last) row blocks of every (b, h) first; the lengths are device values, so a block past n_b
// costs one early exit.  Causal window (MFA_SPARSITY_CAUSAL_WINDOW): mfa_paged_window_prefill_kernel,
// the same body with WIN set (prefill_paged_body.h), whose key loop also starts at the block's
// first visible tile and which never fetches a segment wholly below the window.
//
// Not here (DESIGN.md §3 "Paged prefill"): K/V tiles shared between the query heads of a kv
// group, split-KV for a short chunk over a very long prefix (the decode call's shape).  INT8
// pools are attention_prefill_paged_kv8.hip's (mfa_quantized_paged_prefill_forward); INT4 pools
// and block-wise scales are not read by any prefill kernel.
#include "prefill_paged.h"

namespace mfa {

namespace {

// LDS-DMA of one [BK][DP] 16-bit tile of a paged head into the TileA image, in 32-key segments
// with a base and a byte range each.  The piece geometry is DmaA's (mfa_stage.h): piece n is half
// of 8-row block n / (DP/64), wave w issues pieces w + NW·i; a 32-row segment is four 8-row blocks,
// so piece i of every wave lies in segment SEG(i) and its lane offset is relative to that
// segment's first row.
template <int DP, int BK, int NT>
struct PagedDma {
  static constexpr int NW = NT / 64;
  static constexpr int PPRB = DP / 64;
  static constexpr int NPIECE = BK * DP * 2 / 1024;
  static constexpr int PPW = NPIECE / NW;
  static constexpr int NSEG = BK / 32;
  static_assert(DP % 64 == 0 && BK % 32 == 0 && NPIECE % NW == 0 && PPW >= 1, "DMA geometry");
  static constexpr int seg_of(int i) { return (NW * i) / PPRB / 4; }
  static constexpr bool uniform_segments() {
    for (int i = 0; i < PPW; ++i)
      if ((NW * i) / PPRB / 4 != (NW * i + NW - 1) / PPRB / 4) return false;
    return true;
  }
  int w;
  int off[PPW];

  // step: bytes per token slot; rowbytes: valid bytes per row (D · 2); tid: thread index.
  __device__ __forceinline__ void init(int step, int rowbytes, int tid) {
    static_assert(uniform_segments(), "a wave's piece i must lie in one segment for every wave");
    w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l = tid & 63;
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
      const int n = w + NW * i;
      const int rblk = n / PPRB, sub = 2 * (n % PPRB) + (l >> 5);
      const int r7 = (l & 31) >> 2;
      const int ch = 4 * sub + ((l & 3) ^ ((2 * rblk + (r7 >> 2)) & 3));
      off[i] = ch * 16 < rowbytes ? ((rblk & 3) * 8 + r7) * step + ch * 16 : 0x40000000;
    }
  }
  // head + rel[s]: first row of segment s; bytes[s]: the bytes of it a load may touch.
  __device__ __forceinline__ void issue(const char* head, const int64_t (&rel)[NSEG],
                                        const int (&bytes)[NSEG], char* dst) const {
#pragma unroll
    for (int i = 0; i < PPW; ++i)
      lds_dma16(head + rel[seg_of(i)], bytes[seg_of(i)], off[i], dst + (w + NW * i) * 1024);
  }
};

}  // namespace

template <class E, int DP, int BK>
__global__ void __launch_bounds__(256, 2) mfa_paged_prefill_kernel(PagedPrefillParams pp) {
  constexpr bool WIN = false;
#include "prefill_paged_body.h"
}

// The same under the causal window.
template <class E, int DP, int BK>
__global__ void __launch_bounds__(256, 2) mfa_paged_window_prefill_kernel(PagedPrefillParams pp) {
  constexpr bool WIN = true;
#include "prefill_paged_body.h"
}

// One launch; grid = (batch · heads · 128-row blocks).  p.C is the cap on every length, p.k / p.v
// the pools (16-bit, the compute type), p.R the rows per sequence in the query.
hipError_t fwd_prefill_paged_dispatch(const FwdParams& p, const PagedKv& pg,
                                      const int32_t* new_lens, int elem, hipStream_t stream) {
  if (p.k.prec != elem || p.v.prec != elem || p.k.ss != p.v.ss) return hipErrorNotSupported;
  PagedPrefillParams pp;
  pp.f = p;
  pp.pg = pg;
  pp.new_lens = new_lens;
  pp.f.nblk = (p.R + 127) / 128;
  const int64_t wgs = (int64_t)pp.f.nblk * p.B * p.H;
  if (wgs >= ((int64_t)1 << 31)) return hipErrorNotSupported;
  const dim3 grid((unsigned)wgs), block(256);
  const int DP = p.D <= 64 ? 64 : p.D <= 128 ? 128 : 256;
#define MFA_PREFILL(ELEM, EE, DPV, BKV)                                                       \
  if (elem == ELEM && DP == DPV)                                                              \
    return p.mask.window                                                                      \
               ? launch(mfa_paged_window_prefill_kernel<EE, DPV, BKV>, grid, block,           \
                        4 * BKV * DPV * 2, stream, pp)                                        \
               : launch(mfa_paged_prefill_kernel<EE, DPV, BKV>, grid, block,                  \
                        4 * BKV * DPV * 2, stream, pp);
  MFA_PREFILL(P_FP16, F16, 64, 64)
  MFA_PREFILL(P_FP16, F16, 128, 64)
  MFA_PREFILL(P_FP16, F16, 256, 32)
  MFA_PREFILL(P_BF16, BF16, 64, 64)
  MFA_PREFILL(P_BF16, BF16, 128, 64)
  MFA_PREFILL(P_BF16, BF16, 256, 32)
#undef MFA_PREFILL
  return hipErrorNotSupported;
}

}  // namespace mfa
