// prefill_paged_rw8_body.h — the body of the row-wise INT8-pool paged prefill kernels, as text
// (prefill_paged_body.h says why text): included inside mfa_paged_prefill_rw8_kernel and
// mfa_paged_window_prefill_rw8_kernel (attention_prefill_paged_rw8.hip), which differ in `WIN`
// alone.  The includer provides E, DP, BK, `pp` (a PagedRwPrefillParams) and a
// `constexpr bool WIN`.
//
// Rows, keys, the early exit, the tile grid, the byte staging and its hooks are
// prefill_paged_kv8_body.h's, with a zero point of 0; what differs is the scale strip (wave 0's
// work, below) and the softmax step (fwd2_rowwise.h).  attention_prefill_paged_rw8.hip's header
// has the account.
  constexpr int NT = 256, BQ = 128, ND = DP / 32;
  constexpr int TILEB = BK * DP * 2;
  constexpr int NSEG = BK / 32;
  using KB = PagedBytes<E, DP, BK>;
  using LY = PrefillRw8Lds<DP, BK>;
  constexpr int NP = KB::NPIECE;            // widening pieces per operand per tile
  constexpr int NDMA = KB::NV * KB::NPC;    // byte DMA wave-instructions per operand per tile
  constexpr int NSC = 2 * NSEG;             // scale DMA wave-instructions per tile (wave 0 alone)
  constexpr int NMK = (BK / 32) * (DP / 16), NMV = (BK / 32) * 2 * ND;
  constexpr int KP0 = 1, VP0 = NMV - 2 * NP;
  static_assert(KP0 + 2 * (NP - 1) < NMK && VP0 >= 0, "hook slots");
  static_assert(NDMA + NSC <= 15 && 2 * NDMA <= 15, "counted vmcnt waits");
  // Q is pre-scaled by c on this path (load_q2), so the strip's K scales carry no c.
  constexpr bool PS = E::prec == P_FP16 && DP <= 128;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const kb0 = smem;
  char* const vb0 = smem + 2 * TILEB;
  char* const rawk = smem + LY::RAWK;
  char* const rawv = rawk + KB::SLOT;
  float* const strip = reinterpret_cast<float*>(smem + LY::STRIP);  // two slots of 3·BK floats
  char* const rawsc = smem + LY::RAWSC;     // [k, v][segment]: 32 floats at a 256-byte pitch
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

  const int ssb = (int)p.k.ss;  // one byte per element
  // The kv head's byte and scale runs and the scale page stride, kept in VGPRs (the BK = 64
  // kernels have no SGPR to spare; the DMA helpers read a segment's base back with
  // v_readfirstlane).
  uint64_t khead_ = (uint64_t)(uintptr_t)p.k.ptr + (uint64_t)((int64_t)kvh * pg.head_bytes);
  uint64_t vhead_ = (uint64_t)(uintptr_t)p.v.ptr + (uint64_t)((int64_t)kvh * pg.head_bytes);
  uint64_t kshead = (uint64_t)(uintptr_t)(pp.sc.k + (int64_t)kvh * pp.sc.head);
  uint64_t vshead = (uint64_t)(uintptr_t)(pp.sc.v + (int64_t)kvh * pp.sc.head);
  uint64_t scpage = (uint64_t)pp.sc.page;
  __asm__ __volatile__("" : "+v"(khead_), "+v"(vhead_), "+v"(kshead), "+v"(vshead), "+v"(scpage));
  const char* const khead = (const char*)khead_;
  const char* const vhead = (const char*)vhead_;
  KB kb;  // K and V share the pool layout: one geometry
  kb.init(tid, p.D, ssb);
  const bool w0 = kb.w == 0;  // wave-uniform: the wave that moves the scales
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
    // (They wait a good part of a step for their DMA: in VGPRs, with the heads.)
#pragma unroll
    for (int s = 0; s < NSEG; ++s) __asm__ __volatile__("" : "+v"(rel[s]), "+v"(nb[s]));
  };
  auto pages_of = [&](int t, int (&pages)[NSEG]) {
#pragma unroll
    for (int s = 0; s < NSEG; ++s) pages[s] = prefill_page(pg, b, t + 32 * s);
  };
  // Wave 0: the K and V scales of the tile at key t into the raw runs, each segment with its own
  // page and the range its bytes have (segments' rule); lane l < 32 fetches key 32·s + l of
  // segment s (lanes 32-63 are out of range: they fetch nothing and zero the run's padding).
  const int scoff = lane < 32 ? 4 * lane : 0x40000000;
  auto sc_dma = [&](int t, const int (&pages)[NSEG]) {
#pragma unroll
    for (int s = 0; s < NSEG; ++s) {
      int snb;
      const int64_t srel =
          prefill_scale_segment(pg, (int64_t)scpage, pages[s], t + 32 * s, kend, &snb);
      if constexpr (WIN) {
        if (t + 32 * s + 32 <= klo) snb = 0;
      }
      lds_dma4((const float*)kshead + srel, snb, scoff, rawsc + s * 256);
      lds_dma4((const float*)vshead + srel, snb, scoff, rawsc + (NSEG + s) * 256);
    }
  };
  // Wave 0, once the raw runs of the tile at key tn have landed: lane l < BK derives key tn + l's
  // (kc, lv, rv) into strip slot `slot`.  A key that was not fetched (at or past kend, or in a
  // segment wholly below the window) gets (0, 0, 1): its x is finite and it is masked.
  auto derive = [&](int tn, int slot) {
    __asm__ __volatile__("" ::: "memory");  // the DMA's LDS write is not the compiler's
    if (lane < BK) {
      const float* raw = reinterpret_cast<const float*>(rawsc);
      const int seg = lane >> 5;
      bool ok = tn + lane < kend;
      if constexpr (WIN) ok = ok && tn + 32 * seg + 32 > klo;
      const float ks = ok ? raw[seg * 64 + l32] : 0.f;
      const float vs = ok ? raw[(NSEG + seg) * 64 + l32] : 1.f;
      float* dst = strip + slot * (3 * BK);
      dst[lane] = PS ? ks : ks * c;
      dst[BK + lane] = __builtin_amdgcn_logf(vs);
      dst[2 * BK + lane] = __builtin_amdgcn_rcpf(vs);
    }
  };

  int pg0[NSEG], pgn[NSEG], pgs[NSEG];
  int64_t rel[NSEG];
  int nb[NSEG];
  pages_of(t0, pg0);
  pages_of(t0 + BK, pgn);
  segments(t0, pg0, rel, nb);
  dma(khead, rel, nb, rawk);
  dma(vhead, rel, nb, rawv);
  if (w0) sc_dma(t0, pg0);

  i16x8 qf[DP / 16];
  load_q2<E, DP>(qf, p, b, h, q, live, hh, c);
  RowState<DP> st;
  st.init();
  wait_vm();
  __asm__ __volatile__("" ::: "memory");
  // Tile 0 widened into ring slot 0 and its strip derived into strip slot 0, then the byte
  // slots and the raw runs re-armed with tile 1, in the steady order K, V, scales.
#pragma unroll
  for (int m = 0; m < NP; ++m) {
    kb.widen(kb0, kb.read(rawk, m), 0.f, m, kend - t0);
    kb.widen(vb0, kb.read(rawv, m), 0.f, m, kend - t0);
  }
  if (w0) derive(t0, 0);
  segments(t0 + BK, pgn, rel, nb);
  dma(khead, rel, nb, rawk);
  dma(vhead, rel, nb, rawv);
  if (w0) sc_dma(t0 + BK, pgn);
  pages_of(t0 + 2 * BK, pgn);
  __syncthreads();

  // Counted waits.  At the top of step s a wave has, in issue order, K(s+1), V(s+1) and — wave
  // 0 — scales(s+1) in flight; K(s+2) goes out after K's last piece, V(s+2) after V's, the
  // scales of s+2 after the derive step.  Each wait leaves what was issued behind its subject.
  auto wait_bytes = [&]() {
    if (w0)
      __builtin_amdgcn_s_waitcnt(0x0F70 | (NDMA + NSC));
    else
      __builtin_amdgcn_s_waitcnt(0x0F70 | NDMA);
    __asm__ __volatile__("" ::: "memory");
  };

  int cur = 0;
  for (int t = t0; t < kend; t += BK) {
    // Tile t + 2·BK's segments (its entries were loaded a step ago), then the entries after it.
    segments(t + 2 * BK, pgn, rel, nb);
    // (Kept for the scales, fetched last — in VGPRs, with the scale heads.)
#pragma unroll
    for (int s = 0; s < NSEG; ++s) {
      pgs[s] = pgn[s];
      __asm__ __volatile__("" : "+v"(pgs[s]));
    }
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
          if (m == 0) wait_bytes();  // K(t + BK)'s bytes; V(t + BK)'s and the scales may still fly
          kb.widen(knext, kb.read(rawk, m), 0.f, m, nrows);
          if (m == NP - 1) dma(khead, rel, nb, rawk);
        }
    };
    auto vhook = [&](int i) {
#pragma unroll
      for (int m = 0; m < NP; ++m)
        if (i == VP0 + 2 * m) {
          if (m == 0) wait_bytes();  // V(t + BK)'s bytes; the scales and K(t + 2·BK)'s may still fly
          kb.widen(vnext, kb.read(rawv, m), 0.f, m, nrows);
          if (m == NP - 1) dma(vhead, rel, nb, rawv);
        }
    };
    fwd2_qk<E, DP, BK>(kb0 + cur * TILEB, rbase, qf, st, sc, khook);
    fwd2_rw_softmax<E, DP, BK>(st, sc, pb, strip + cur * (3 * BK), t, mask_tile, qpos, lp, wsz, hh);
    fwd2_pv<E, DP, BK>(vb0 + cur * TILEB, trb, pb, st, vhook);
    if (w0) {
      // The scales of tile t + BK (K(t + 2·BK) and V(t + 2·BK), issued above, may still fly)
      // into the other strip slot, then the raw runs re-armed behind the derive step's reads.
      __builtin_amdgcn_s_waitcnt(0x0F70 | (2 * NDMA));
      derive(t + BK, cur ^ 1);
      sc_dma(t + 2 * BK, pgs);
    }
    // Publishes the widened tile and its strip.
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
