// attention_prefill_paged_rw8.hip — the paged prefill over row-wise INT8 pools
// (mfa_paged_prefill_forward_rowwise; no reference counterpart): every key has a K scale and a V
// scale of its own (PagedKvScales), applied inside the kernel.  Rows, keys, dead rows, the early
// exit, the masks, the grid order, the tile grid and the byte staging (LDS-DMA one tile ahead into
// byte slots, widened into the 16-bit ring under the current tile's MFMAs, range-checked 32-key
// segments) are mfa_paged_prefill_kv8_kernel's (attention_prefill_paged_kv8.hip), with zero
// points of 0.
//
// Operands stay exact.  The TileA image holds the integers q; the scales are not multiplied into
// it: scale · q would be rounded to 16 bits, would leave FP16's range for small V scales, and
// prefill and decode would disagree about what the cache holds.  The scales enter in the softmax
// step instead (fwd2_rowwise.h): x = s · kc + lv, the max over x, P = exp2(x - m) = p · vs
// bounded by the lazy-rescale threshold, the denominator sum of P · rv in FP32, o_mul = 1.
//
// The scale strip.  Per tile every wave needs (kc, lv, rv) of BK keys; they are derived once per
// key, by wave 0, and shared through LDS:
//   * with the tile's byte DMA, one tile ahead, wave 0 issues two dword LDS-DMA loads per 32-key
//     segment (K scales, V scales) into the raw runs, with the segment's own page (the
//     block-table entries the byte descriptors were built from) and range: no scale is fetched
//     for a slot at or past the block's last key, for another page, or for a segment wholly below
//     the window;
//   * after the step's PV chain, behind a counted vmcnt wait that orders its own loads, lane l of
//     wave 0 reads key l's two scales, forms kc = ks (· c where Q is not pre-scaled),
//     lv = log2 vs and rv = 1 / vs — (0, 0, 1) for a key that was not fetched — and writes them
//     to the other strip slot; then it re-arms the raw runs with the tile after;
//   * the step's closing barrier publishes that strip slot together with the widened tile;
//   * in the softmax step every lane reads its keys' values back as broadcast ds_read_b128s,
//     four consecutive keys each: 12 per 32-key block (kc, lv and rv of 16 keys).
// Per score that is one FMA more than the per-tensor step (x from s) and an FMA in place of an
// add in the row sum; the derive step is two transcendentals per key and tile, in one wave.
//
// LDS: the per-tensor kernel's 4 tiles of 16 bits + 2 byte slots, then two strip slots of
// 3·BK floats and the raw runs (2·BK/32 runs of 32 floats at a 256-byte pitch):
//   D = 64: 40 KiB + 2.5 KiB, D = 128: 80 KiB + 2.5 KiB, D = 256: 80 KiB + 1.25 KiB.
// At D = 128 and 256 the per-tensor kernel's two workgroups per CU fill the CU's 160 KiB, so this
// kernel runs one workgroup per CU there (and is built for it: __launch_bounds__(256, 1));
// D = 64 keeps two.  DESIGN.md, "Row-wise prefill", has the measured cost.
// The body is prefill_paged_rw8_body.h, included by mfa_paged_prefill_rw8_kernel and, with WIN
// set (the causal window), by mfa_paged_window_prefill_rw8_kernel.
#include "fwd2_rowwise.h"
#include "paged_bytes.h"
#include "prefill_paged.h"

namespace mfa {

// The dynamic LDS of one workgroup: ring | K bytes | V bytes | strip slots | raw scale runs.
template <int DP, int BK>
struct PrefillRw8Lds {
  static constexpr int RAWK = 4 * BK * DP * 2;
  static constexpr int STRIP = RAWK + 2 * PagedBytes<F16, DP, BK>::SLOT;
  static constexpr int RAWSC = STRIP + 2 * 3 * BK * 4;
  static constexpr int BYTES = RAWSC + 2 * (BK / 32) * 256;
  static constexpr int WGS = 2 * BYTES <= 160 * 1024 ? 2 : 1;  // workgroups per CU
};

template <class E, int DP, int BK>
__global__ void __launch_bounds__(256, (PrefillRw8Lds<DP, BK>::WGS))
    mfa_paged_prefill_rw8_kernel(PagedRwPrefillParams pp) {
  constexpr bool WIN = false;
#include "prefill_paged_rw8_body.h"
}

// The same under the causal window.
template <class E, int DP, int BK>
__global__ void __launch_bounds__(256, (PrefillRw8Lds<DP, BK>::WGS))
    mfa_paged_window_prefill_rw8_kernel(PagedRwPrefillParams pp) {
  constexpr bool WIN = true;
#include "prefill_paged_rw8_body.h"
}

// One launch; grid = (batch · heads · 128-row blocks).  p.k / p.v: the INT8 pools (token stride
// in bytes, zero points 0), p.c_log2 without a K scale, p.o_mul = 1; sc: the scale pools.
hipError_t fwd_prefill_paged_rw8_dispatch(const FwdParams& p, const PagedKv& pg,
                                          const PagedKvScales& sc, const int32_t* new_lens,
                                          int elem, hipStream_t stream) {
  if (p.k.prec != P_INT8 || p.v.prec != P_INT8 || p.k.ss != p.v.ss || p.D % 16 != 0 ||
      p.k.zp != 0 || p.v.zp != 0)
    return hipErrorNotSupported;
  PagedRwPrefillParams pp;
  pp.f = p;
  pp.pg = pg;
  pp.new_lens = new_lens;
  pp.sc = sc;
  pp.f.nblk = (p.R + 127) / 128;
  const int64_t wgs = (int64_t)pp.f.nblk * p.B * p.H;
  if (wgs >= ((int64_t)1 << 31)) return hipErrorNotSupported;
  const dim3 grid((unsigned)wgs), block(256);
  const int DP = p.D <= 64 ? 64 : p.D <= 128 ? 128 : 256;
#define MFA_PREFILL_RW8(ELEM, EE, DPV, BKV)                                                   \
  if (elem == ELEM && DP == DPV)                                                              \
    return p.mask.window                                                                      \
               ? launch(mfa_paged_window_prefill_rw8_kernel<EE, DPV, BKV>, grid, block,       \
                        PrefillRw8Lds<DPV, BKV>::BYTES, stream, pp)                           \
               : launch(mfa_paged_prefill_rw8_kernel<EE, DPV, BKV>, grid, block,              \
                        PrefillRw8Lds<DPV, BKV>::BYTES, stream, pp);
  MFA_PREFILL_RW8(P_FP16, F16, 64, 64)
  MFA_PREFILL_RW8(P_FP16, F16, 128, 64)
  MFA_PREFILL_RW8(P_FP16, F16, 256, 32)
  MFA_PREFILL_RW8(P_BF16, BF16, 64, 64)
  MFA_PREFILL_RW8(P_BF16, BF16, 128, 64)
  MFA_PREFILL_RW8(P_BF16, BF16, 256, 32)
#undef MFA_PREFILL_RW8
  return hipErrorNotSupported;
}

}  // namespace mfa
