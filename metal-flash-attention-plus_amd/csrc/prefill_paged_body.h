// prefill_paged_body.h — the body of the 16-bit paged prefill kernels, as text.
//
// Not a stand-alone header: the statements of a kernel body, included inside
// mfa_paged_prefill_kernel and mfa_paged_window_prefill_kernel (attention_prefill_paged.hip),
// which differ in `WIN` alone.  Text and not a function for decode32_quant_body.h's reason: lifted
// into a __device__ function the same statements compile to other code, and the kernel without a
// window keeps the code it had.  Contract of the place that includes it: a __global__ function
// template with parameters E, DP and BK, its parameter `pp` (PagedPrefillParams), a
// `constexpr bool WIN` in scope, and PagedDma of that file.  Nothing may follow it but the
// closing brace.
//
// WIN: the causal window (MFA_SPARSITY_CAUSAL_WINDOW; the host sets mask.causal
// and mask.window, window_size <= 2^30), a kernel of its own (mfa_paged_window_prefill_kernel) so
// that the others keep their code:
//   * the key loop starts at the tile of the lowest key the block's first live row sees
//     (klo = max(0, position of that row - W)), still a multiple of BK counted from key 0;
//   * a 32-key segment wholly below klo is not fetched (a zero byte range lands as zeros, every
//     one of its keys is masked for every row of the block, and its block-table entry does not
//     matter): block 0's klo is the sequence's lo_b of the page-release contract (mfa.h);
//   * a tile is masked per element when the window's lower edge of any live row of the block cuts
//     it: the last live row has the highest edge.  Rows late in the block meet leading tiles that
//     are wholly -inf while their state is at its initial max; fwd2_max keeps their offset.
  constexpr int NT = 256, BQ = 128;
  constexpr int TILEB = BK * DP * 2;
  using Dma = PagedDma<DP, BK, NT>;
  constexpr int NSEG = Dma::NSEG;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const kb0 = smem;
  char* const vb0 = smem + 2 * TILEB;
  const FwdParams& p = pp.f;
  const PagedKv& pg = pp.pg;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int l32 = lane & 31, hh = lane >> 5;
  const int rbase[2] = {TileA<DP>::row_base(l32, hh, 0), TileA<DP>::row_base(l32, hh, 1)};
  const int trb[2] = {TileA<DP>::tr_base(lane, 0), TileA<DP>::tr_base(lane, 1)};
  // Causal: heaviest blocks first over the whole grid (balance); otherwise each head's blocks
  // together on one XCD (L2 reuse of its K/V).
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

  // The sequence's keys and rows (uniform).  p.C is the host-side cap on every length.
  const int len = min(max(((prefill_i32_ptr)pg.seq_lens)[b], 0), p.C);
  const int n = pp.new_lens ? min(max(((prefill_i32_ptr)pp.new_lens)[b], 0), p.R) : p.R;
  const int shift = len - n;              // row q is key position shift + q
  // Keys of this block: up to its last live row's position (causal), or all of them.
  const int qlast = min(q0 + BQ, n) - 1;  // last row of the block that belongs to the sequence
  const int kend = p.mask.causal ? min(len, shift + qlast + 1) : len;
  if (q0 >= n || kend <= 0) {
    // No live row: nothing of the cache is read.
    if (q < p.R) store_dead_row<DP>(p, b, h, q, hh);
    return;
  }
  const int wsz = WIN ? (int)p.mask.window_size : 0x3fffffff;
  const int klo = WIN ? max(max(shift + q0, 0) - wsz, 0) : 0;
  const int t0 = WIN ? klo & ~(BK - 1) : 0;
  const int tq = shift + q;
  const bool live = q < n && tq >= 0;
  // The body's view: len keys, the lane's query at key position tq (dead rows: masked wherever
  // the causal mask is applied; their result is replaced below).
  FwdParams lp = p;
  lp.C = len;
  const int qpos = live ? tq : -1;
  const float c = p.c_log2;

  const int ssb = (int)p.k.ss * 2, dbytes = 2 * p.D;
  const char* khead = (const char*)p.k.ptr + (int64_t)kvh * pg.head_bytes;
  const char* vhead = (const char*)p.v.ptr + (int64_t)kvh * pg.head_bytes;
  Dma dma;  // K and V share the pool layout: one set of lane offsets
  dma.init(ssb, dbytes, tid);
  // Tile at key t with its segments' block-table entries `pages` into ring slot `slot`.
  auto stage = [&](int t, const int (&pages)[NSEG], int slot) {
    int64_t rel[NSEG];
    int nb[NSEG];
#pragma unroll
    for (int s = 0; s < NSEG; ++s)
      rel[s] = prefill_segment(pg, pages[s], t + 32 * s, len, ssb, dbytes, &nb[s]);
    if constexpr (WIN) {
#pragma unroll
      for (int s = 0; s < NSEG; ++s)
        if (t + 32 * s + 32 <= klo) nb[s] = 0;
    }
    dma.issue(khead, rel, nb, kb0 + slot * TILEB);
    dma.issue(vhead, rel, nb, vb0 + slot * TILEB);
  };
  int pgn[NSEG];  // entries of the next tile to stage
#pragma unroll
  for (int s = 0; s < NSEG; ++s) pgn[s] = prefill_page(pg, b, t0 + 32 * s);
  stage(t0, pgn, 0);
#pragma unroll
  for (int s = 0; s < NSEG; ++s) pgn[s] = prefill_page(pg, b, t0 + BK + 32 * s);

  i16x8 qf[DP / 16];
  load_q2<E, DP>(qf, p, b, h, q, live, hh, c);
  RowState<DP> st;
  st.init();
  wait_vm();
  __syncthreads();

  int cur = 0;
  for (int t = t0; t < kend; t += BK) {
    if (t + BK < kend) {
      stage(t + BK, pgn, cur ^ 1);
      // The entries of the tile after it: a whole tile's compute before they are used.
#pragma unroll
      for (int s = 0; s < NSEG; ++s) pgn[s] = prefill_page(pg, b, t + 2 * BK + 32 * s);
    }
    // The block's first row bounds the tiles every live row sees whole.
    bool mask_tile = (t + BK > len) || (p.mask.causal && t + BK - 1 > shift + q0);
    if constexpr (WIN) mask_tile = mask_tile || t < shift + qlast - wsz;
    fwd2_tile<E, DP, BK>(kb0 + cur * TILEB, vb0 + cur * TILEB, rbase, trb, qf, st, t, mask_tile,
                         qpos, lp, c, wsz, hh);
    wait_vm();
    __syncthreads();
    cur ^= 1;
  }

  float l = cross_half_sum(st.lh) + kFltMin;
  if (!(l > 0.f)) l = kFltMin;
  if (live)
    store_o_l<DP>(p, st.o, st.m, l, b, h, q, hh);
  else if (q < p.R)
    store_dead_row<DP>(p, b, h, q, hh);
