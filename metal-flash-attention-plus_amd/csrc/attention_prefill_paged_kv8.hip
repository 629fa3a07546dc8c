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
// Staging.  One byte slot per operand (KvBytes' geometry for 256 threads, PagedBytes below: every
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
#include "kv_bytes.h"
#include "prefill_paged.h"

namespace mfa {

namespace {

// KvBytes' byte ring for 256 threads (kv_bytes.h: Kv8Geo's 512 chunk slots, two per thread; lane
// l's bytes of a slot at 16·l or 4·l of its wave's region) over paged segments, with the
// per-lane state cut to what the two slots do not share.  Slot 1 of a thread is slot 0 of the
// thread 256 further, i.e. of virtual wave w + 4:
//   BK = 64 (D <= 128): the same chunks of the row 32 below — the next 32-key segment, the same
//     offset from its first row, the image 4 row blocks further;
//   BK = 32 (D = 256): the same row's chunks 128 columns further — the same segment, its own
//     offset (it may lie past D), the image 4 sub-tiles (2048 bytes) further.
// A slot's second TileA chunk (CE = 16: ch0 is even) sits at the first one's offset ^ 16.
// So segment SEG(k) of slot k is wave-uniform and each DMA wave-instruction takes one segment's
// base and range.
template <class E, int DP, int BK>
struct PagedBytes {
  using G = Kv8Geo<DP, BK>;
  static constexpr int NV = 2, CE = G::CE, CB = CE;
  static constexpr int NPC = CB == 16 ? 1 : CB / 4;  // DMA wave-instructions per chunk slot
  static constexpr int SLOT = 512 * CB;              // bytes per staged tile of one operand
  static constexpr int NH = CE / 8;                  // TileA chunks per slot
  static constexpr int NPIECE = NV * NH;             // widening pieces per operand per tile
  static constexpr int NSEG = BK / 32;
  static constexpr bool ROWS = BK == 64;             // slot 1: 32 rows below (else 128 columns on)
  static_assert((BK == 64 && DP <= 128) || (BK == 32 && DP == 256), "slot 1's place");
  static constexpr int IMG1 = ROWS ? 4 * TileA<DP>::RB : 2048;
  static constexpr int NO = ROWS ? 1 : 2;            // slots with an offset and a validity of their own
  static constexpr int seg_of(int k) { return ROWS ? k : 0; }
  int img;      // TileA offset of slot 0's first chunk
  int rd;       // the lane's place in its wave's region of a byte slot
  int off[NO];  // DMA offset from the segment's first row; past any range where the chunk is past D
  int rq[NO];   // the chunk's row in the tile; 0x3fffffff where the chunk is past D
  int w;        // wave (uniform)

  // ss: stored bytes per row.
  __device__ __forceinline__ void init(int tid, int D, int ss) {
    const int lane = tid & 63;
    w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const G g(tid);
    img = TileA<DP>::off(g.r, g.ch0);
    rd = lane * (CB == 16 ? 16 : 4);
#pragma unroll
    for (int k = 0; k < NO; ++k) {
      const int col = g.col + 128 * k;
      off[k] = col < D ? g.r * ss + col : 0x40000000;
      rq[k] = col < D ? g.r : 0x3fffffff;
    }
  }
  // One operand's tile: segment s at head + rel[s] with nb[s] bytes in range -> slot.
  __device__ __forceinline__ void dma(const char* head, const int64_t (&rel)[NSEG],
                                      const int (&nb)[NSEG], char* slot) const {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int s = seg_of(k), o = off[ROWS ? 0 : k], vw = w + 4 * k;
      if constexpr (CB == 16) {
        lds_dma16(head + rel[s], nb[s], o, slot + vw * 1024);
      } else {
#pragma unroll
        for (int j = 0; j < NPC; ++j)
          lds_dma4(head + rel[s], nb[s], o + 4 * j, slot + j * 2048 + vw * 256);
      }
    }
  }
  // Piece m (slot k = m / NH, half hf = m % NH): its stored bytes.
  __device__ __forceinline__ uint4 read(const char* slot, int m) const {
    const int k = m / NH, hf = m % NH, vw = w + 4 * k;
    if constexpr (CB == 16) {
      const uint2 a = *reinterpret_cast<const uint2*>(slot + vw * 1024 + rd + 8 * hf);
      return make_uint4(a.x, a.y, 0u, 0u);
    } else {
      const uint32_t a = *reinterpret_cast<const uint32_t*>(slot + vw * 256 + rd);
      const uint32_t c = *reinterpret_cast<const uint32_t*>(slot + 2048 + vw * 256 + rd);
      return make_uint4(a, c, 0u, 0u);
    }
  }
  // Piece m widened into the 16-bit image; rows at or past `rows` (the keys left from the
  // tile's first row) and chunks past D give zeros.
  __device__ __forceinline__ void widen(char* img16, const uint4 raw, float zp, int m,
                                        int rows) const {
    const int k = m / NH, hf = m % NH;
    uint4 v = dequant_fast<E, SRC_I8>(raw, zp);
    const bool ok = ROWS ? rq[0] + 32 * k < rows : rq[k] < rows;
    if (!ok) v = make_uint4(0u, 0u, 0u, 0u);
    *reinterpret_cast<uint4*>(img16 + ((img ^ (16 * hf)) + k * IMG1)) = v;
  }
};

}  // namespace

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
