// attention_prefill_paged_kv8.hip — the paged prefill over per-tensor INT8 pools, widened on load
// (mfa_quantized_paged_prefill_forward; no reference counterpart).  Rows, keys, dead rows, the
// early exit, the masks, the grid order and the tile grid (tiles start at absolute keys that are
// multiples of BK) are mfa_paged_prefill_kernel's (attention_prefill_paged.hip); the tile body is
// the 16-bit forward's fwd2_qk / fwd2_softmax / fwd2_pv and the epilogue store_o_l.
//
// Numerics: the decode call's dequant-exact scheme.  The TileA image holds the exact integers
// q - zero_point in E (mfa_stage.h dequant_fast), k_scale is folded into the softmax multiplier
// (p.c_log2 = 1.442695041f * scale * k_scale, the host's association) and v_scale into p.o_mul,
// which store_o_l applies as o_mul / l.  O and L are therefore bit-identical to
// mfa_paged_prefill_kernel over 16-bit pools holding q - zp at softmax scale scale * k_scale,
// with O multiplied by v_scale.
//
// Staging.  One byte slot per operand (KvBytes' geometry for 256 threads, PagedBytes in paged_bytes.h: every
// thread owns two of the tile's 512 chunk slots) next to the 16-bit ring of two tiles per operand.  At step s
//   * the byte slots hold tile s + 1's K and V bytes, fetched by LDS-DMA during step s - 1;
//   * each lane widens its own chunks of tile s + 1 into the ring's other 16-bit slot in pieces
//     placed between the MFMAs of tile s (K under QK^T, V under PV), after a counted vmcnt wait
//     that orders the lane's own DMA bytes before it reads them — no barrier, since a byte slot
//     is read only by the lanes whose DMA wrote it;
//   * right after an operand's last piece has been written, the same lanes re-arm the byte slot
//     with tile s + 2 (the LDS write of the widened chunk depends on the slot's read, so the DMA
//     is issued behind it);
//   * the step's closing barrier publishes the widened tile.
// A wave-instruction of the byte DMA covers one 8-row group, which lies in one 32-key segment, so
// it takes that segment's base and range-checked descriptor: prefill_segment with one byte per
// element, bounded by the block's last key (kend <= len_b) and the page's end.  Neither an
// unused slot, nor a foreign page, nor a tile past the block's last key is fetched; the
// block-table entries are scalar loads issued one step before their segment's descriptor is
// built.  Rows at or past kend and chunks past D widen to zero (their zero fill would decode to
// -zp); such rows are masked in the body as well.
//
// LDS: 4 tiles of 16 bits + 2 byte slots = 80 KiB at D = 128 and 256, 40 KiB at D = 64: two
// workgroups per CU, as the 16-bit kernel.
// The body is prefill_paged_kv8_body.h, included by mfa_paged_prefill_kv8_kernel and, with WIN
// set (the causal window), by mfa_paged_window_prefill_kv8_kernel.
#include "paged_bytes.h"
#include "prefill_paged.h"

namespace mfa {

template <class E, int DP, int BK>
__global__ void __launch_bounds__(256, 2) mfa_paged_prefill_kv8_kernel(PagedPrefillParams pp) {
  constexpr bool WIN = false;
#include "prefill_paged_kv8_body.h"
}

// The same under the causal window.
template <class E, int DP, int BK>
__global__ void __launch_bounds__(256, 2)
    mfa_paged_window_prefill_kv8_kernel(PagedPrefillParams pp) {
  constexpr bool WIN = true;
#include "prefill_paged_kv8_body.h"
}

template <int DP, int BK>
static constexpr size_t prefill_kv8_lds() {
  return 4 * BK * DP * 2 + 2 * PagedBytes<F16, DP, BK>::SLOT;
}

// One launch; grid = (batch · heads · 128-row blocks).  p.k / p.v: the INT8 pools (token stride
// in bytes, zero points), p.c_log2 and p.o_mul with the pools' scales folded in.
hipError_t fwd_prefill_paged_kv8_dispatch(const FwdParams& p, const PagedKv& pg,
                                          const int32_t* new_lens, int elem, hipStream_t stream) {
  if (p.k.prec != P_INT8 || p.v.prec != P_INT8 || p.k.ss != p.v.ss || p.D % 16 != 0)
    return hipErrorNotSupported;
  PagedPrefillParams pp;
  pp.f = p;
  pp.pg = pg;
  pp.new_lens = new_lens;
  pp.f.nblk = (p.R + 127) / 128;
  const int64_t wgs = (int64_t)pp.f.nblk * p.B * p.H;
  if (wgs >= ((int64_t)1 << 31)) return hipErrorNotSupported;
  const dim3 grid((unsigned)wgs), block(256);
  const int DP = p.D <= 64 ? 64 : p.D <= 128 ? 128 : 256;
#define MFA_PREFILL_KV8(ELEM, EE, DPV, BKV)                                                   \
  if (elem == ELEM && DP == DPV)                                                              \
    return p.mask.window                                                                      \
               ? launch(mfa_paged_window_prefill_kv8_kernel<EE, DPV, BKV>, grid, block,       \
                        prefill_kv8_lds<DPV, BKV>(), stream, pp)                              \
               : launch(mfa_paged_prefill_kv8_kernel<EE, DPV, BKV>, grid, block,              \
                        prefill_kv8_lds<DPV, BKV>(), stream, pp);
  MFA_PREFILL_KV8(P_FP16, F16, 64, 64)
  MFA_PREFILL_KV8(P_FP16, F16, 128, 64)
  MFA_PREFILL_KV8(P_FP16, F16, 256, 32)
  MFA_PREFILL_KV8(P_BF16, BF16, 64, 64)
  MFA_PREFILL_KV8(P_BF16, BF16, 128, 64)
  MFA_PREFILL_KV8(P_BF16, BF16, 256, 32)
#undef MFA_PREFILL_KV8
  return hipErrorNotSupported;
}

}  // namespace mfa
