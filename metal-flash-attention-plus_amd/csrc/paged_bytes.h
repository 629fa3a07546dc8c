// paged_bytes.h — the byte staging of the INT8-pool paged prefill kernels
// (attention_prefill_paged_kv8.hip: per-tensor scales; attention_prefill_paged_rw8.hip: row-wise
// scales): one tile's stored bytes by LDS-DMA into a byte slot, widened by the same lanes into the
// 16-bit TileA image.
#pragma once
#include "kv_bytes.h"

namespace mfa {

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

}  // namespace mfa
