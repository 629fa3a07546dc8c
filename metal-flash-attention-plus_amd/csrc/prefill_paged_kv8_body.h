// prefill_paged_kv8_body.h — the body of the INT8-pool paged prefill kernels, as text
// (prefill_paged_body.h says why text): included inside mfa_paged_prefill_kv8_kernel and
// mfa_paged_window_prefill_kv8_kernel (attention_prefill_paged_kv8.hip), which differ in `WIN`
// alone.  The includer provides E, DP, BK, `pp`, a `constexpr bool WIN` and PagedBytes.
//
// WIN: the causal window, with attention_prefill_paged.hip's loop start (t0),
// segment rule (klo) and tile-mask rule, so that the two kernels read the same keys in the same
// order and keep their bit-for-bit contract (mfa.h) under the window too.
  constexpr int NT = 256, BQ = 128, ND = DP / 32;
  constexpr int TILEB = BK * DP * 2;
  constexpr int NSEG = BK / 32;
  using KB = PagedBytes<E, DP, BK>;
  constexpr int NP = KB::NPIECE;            // widening pieces per operand per tile
  constexpr int NDMA = KB::NV * KB::NPC;    // DMA wave-instructions per operand per tile
  // Widening slots: after every other MFMA from the second (K), and the same ending two before
  // the PV chain's last (V), so the re-armed DMA has the rest of the step and the next one.
  constexpr int NMK = (BK / 32) * (DP / 16), NMV = (BK / 32) * 2 * ND;
  constexpr int KP0 = 1, VP0 = NMV - 2 * NP;
  static_assert(KP0 + 2 * (NP - 1) < NMK && VP0 >= 0, "hook slots");
  static_assert(NDMA <= 7, "counted vmcnt wait");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const kb0 = smem;
  char* const vb0 = smem + 2 * TILEB;
  char* const rawk = smem + 4 * TILEB;
  char* const rawv = rawk + KB::SLOT;
  const FwdParams& p = pp.f;
  const PagedKv& pg = pp.pg;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int l32 = lane & 31, hh = lane >> 5;
  const int rbase[2] = {TileA<DP>::row_base(l32, hh, 0), TileA<DP>::row_base(l32, hh, 1)};
  const int trb[2] = {TileA<DP>::tr_base(lane, 0), TileA<DP>::tr_base(lane, 1)};
  int bh, blk;
  if (p.mask.causal) {
    bh = blockIdx.x % (p.B * p.H);
    blk = blockIdx.x / (p.B * p.H);
  } else {
    xcd_unit_block(blockIdx.x, p.B * p.H, p.nblk, &bh, &blk);
  }
  const int rb = p.nblk - 1 - blk;
  const int b = bh / p.H, h = bh % p.H, kvh = h % p.Hkv;
  const int q0 = rb * BQ;
  const int q = q0 + wave * 32 + l32;

  const int len = min(max(((prefill_i32_ptr)pg.seq_lens)[b], 0), p.C);
  const int n = pp.new_lens ? min(max(((prefill_i32_ptr)pp.new_lens)[b], 0), p.R) : p.R;
  const int shift = len - n;
  const int qlast = min(q0 + BQ, n) - 1;
  const int kend = p.mask.causal ? min(len, shift + qlast + 1) : len;
  if (q0 >= n || kend <= 0) {
    if (q < p.R) store_dead_row<DP>(p, b, h, q, hh);
    return;
  }
  const int wsz = WIN ? (int)p.mask.window_size : 0x3fffffff;
  const int klo = WIN ? max(max(shift + q0, 0) - wsz, 0) : 0;
  const int t0 = WIN ? klo & ~(BK - 1) : 0;
  const int tq = shift + q;
  const bool live = q < n && tq >= 0;
  FwdParams lp = p;
  lp.C = len;
  const int qpos = live ? tq : -1;
  const float c = p.c_log2;
  const float zk = (float)p.k.zp, zv = (float)p.v.zp;

  const int ssb = (int)p.k.ss;  // one byte per element
  const char* khead = (const char*)p.k.ptr + (int64_t)kvh * pg.head_bytes;
  const char* vhead = (const char*)p.v.ptr + (int64_t)kvh * pg.head_bytes;
  KB kb;  // K and V share the pool layout: one geometry
  kb.init(tid, p.D, ssb);
  auto dma = [&](const char* head, const int64_t (&rel)[NSEG], const int (&nb)[NSEG], char* slot) {
    kb.dma(head, rel, nb, slot);
  };
  // Segment bases and ranges of the tile at key t from its block-table entries.
  auto segments = [&](int t, const int (&pages)[NSEG], int64_t (&rel)[NSEG], int (&nb)[NSEG]) {
#pragma unroll
    for (int s = 0; s < NSEG; ++s)
      rel[s] = prefill_segment(pg, pages[s], t + 32 * s, kend, ssb, p.D, &nb[s]);
    if constexpr (WIN) {
#pragma unroll
      for (int s = 0; s < NSEG; ++s)
        if (t + 32 * s + 32 <= klo) nb[s] = 0;
    }
  };
  auto pages_of = [&](int t, int (&pages)[NSEG]) {
#pragma unroll
    for (int s = 0; s < NSEG; ++s) pages[s] = prefill_page(pg, b, t + 32 * s);
  };

  int pg0[NSEG], pgn[NSEG];
  int64_t rel[NSEG];
  int nb[NSEG];
  pages_of(t0, pg0);
  pages_of(t0 + BK, pgn);
  segments(t0, pg0, rel, nb);
  dma(khead, rel, nb, rawk);
  dma(vhead, rel, nb, rawv);

  i16x8 qf[DP / 16];
  load_q2<E, DP>(qf, p, b, h, q, live, hh, c);
  RowState<DP> st;
  st.init();
  wait_vm();
  __asm__ __volatile__("" ::: "memory");
  // Tile 0 widened into ring slot 0, then the byte slots re-armed with tile 1.
#pragma unroll
  for (int m = 0; m < NP; ++m) {
    kb.widen(kb0, kb.read(rawk, m), zk, m, kend - t0);
    kb.widen(vb0, kb.read(rawv, m), zv, m, kend - t0);
  }
  segments(t0 + BK, pgn, rel, nb);
  dma(khead, rel, nb, rawk);
  dma(vhead, rel, nb, rawv);
  pages_of(t0 + 2 * BK, pgn);
  __syncthreads();

  int cur = 0;
  for (int t = t0; t < kend; t += BK) {
    // Tile t + 2·BK's segments (its entries were loaded a step ago), then the entries after it.
    segments(t + 2 * BK, pgn, rel, nb);
    pages_of(t + 3 * BK, pgn);
    bool mask_tile = (t + BK > len) || (p.mask.causal && t + BK - 1 > shift + q0);
    if constexpr (WIN) mask_tile = mask_tile || t < shift + qlast - wsz;
    char* const knext = kb0 + (cur ^ 1) * TILEB;
    char* const vnext = vb0 + (cur ^ 1) * TILEB;
    const int nrows = kend - (t + BK);
    f32x16 sc[BK / 32];
    i16x8 pb[BK / 16];
    auto khook = [&](int i) {
#pragma unroll
      for (int m = 0; m < NP; ++m)
        if (i == KP0 + 2 * m) {
          if (m == 0) {
            // K(t + BK)'s bytes; V(t + BK)'s, issued behind them, may still fly.
            __builtin_amdgcn_s_waitcnt(0x0F70 | NDMA);
            __asm__ __volatile__("" ::: "memory");
          }
          kb.widen(knext, kb.read(rawk, m), zk, m, nrows);
          if (m == NP - 1) dma(khead, rel, nb, rawk);
        }
    };
    auto vhook = [&](int i) {
#pragma unroll
      for (int m = 0; m < NP; ++m)
        if (i == VP0 + 2 * m) {
          if (m == 0) {
            // V(t + BK)'s bytes; K(t + 2·BK)'s, issued above, may still fly.
            __builtin_amdgcn_s_waitcnt(0x0F70 | NDMA);
            __asm__ __volatile__("" ::: "memory");
          }
          kb.widen(vnext, kb.read(rawv, m), zv, m, nrows);
          if (m == NP - 1) dma(vhead, rel, nb, rawv);
        }
    };
    fwd2_qk<E, DP, BK>(kb0 + cur * TILEB, rbase, qf, st, sc, khook);
    fwd2_softmax<E, DP, BK>(st, sc, pb, t, mask_tile, qpos, lp, c, wsz, hh);
    fwd2_pv<E, DP, BK>(vb0 + cur * TILEB, trb, pb, st, vhook);
    __syncthreads();
    cur ^= 1;
  }
  // The last re-armed (empty-range) DMAs land before the workgroup's LDS is released.
  wait_vm();

  float l = cross_half_sum(st.lh) + kFltMin;
  if (!(l > 0.f)) l = kFltMin;
  if (live)
    store_o_l<DP>(p, st.o, st.m, l, b, h, q, hh);
  else if (q < p.R)
    store_dead_row<DP>(p, b, h, q, hh);
