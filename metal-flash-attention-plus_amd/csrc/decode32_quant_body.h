// decode32_quant_body.h — the INT8 / INT4 32-row decode body (attention_decode.hip), as text.
//
// Not a stand-alone header: it is the statements of a kernel body, included inside
// mfa_fwd_decode_paged_kernel, in its quantised branch.  It is written for both addressing
// policies and both sources, so that mfa_fwd_decode_kernel can include it too; today that kernel
// keeps a copy of its own with ContiguousKv written out (the comment above it says why), and a
// fix to one goes into the other.  Contract of the place that includes it:
//   * a __global__ function template with parameters E (element traits), DP (padded head
//     width) and SRC (SRC_I8 or SRC_I4);
//   * a type PG in scope, the addressing policy (ContiguousKv or PagedKvPolicy), and an object
//     `pg` of it;
//   * `dp`, a DecodeParams (or a reference to one), and `smem`, the dynamic LDS array.
// It ends the kernel: nothing may follow it but the closing braces.
//
// Why text and not a function: the same statements lifted into a __device__ __forceinline__
// function compile to other code (30-240 more instructions per kernel, mostly 64-bit address
// and compare work; the contiguous INT8 kernel measured 3-7 % slower that way); included inside
// the __global__ function they compile to within 6 instructions of the body written in place
// ("Paged decode", the paragraph on shared bodies; profiles/decode_paged_ab.txt
// parts 3 and 5).
  const FwdParams& p = dp.f;
  constexpr bool I4 = SRC == SRC_I4;
  static_assert(!(PG::paged && I4), "paged caches: 16-bit and INT8");
  // INT4 keeps three tiles in flight (four ring slots in the INT8 ring's bytes: the packed
  // tiles are half as large, and V is read from the packed tile too).
  constexpr int BK = 32, NSLOT = SRC == SRC_I4 ? 4 : 2, ND = DP / 32;
  constexpr int ROWB = DP;                  // INT8 compute tile: one byte per element
  using T = Tile16<ROWB / 2>;               // [BK][ROWB bytes], 16-byte chunks XOR-swizzled
  constexpr int TILEB = BK * ROWB;          // one K or V compute tile
  constexpr int ROWBS = I4 ? DP / 2 : DP;   // bytes per stored row
  constexpr int TILEBS = BK * ROWBS;        // one stored (DMA) tile
  constexpr int NPC = TILEBS / 1024;        // 1-KiB DMA pieces per tile
  constexpr int RP = 1024 / ROWBS;          // rows per piece
  static_assert(NPC >= 1 && NPC <= 8, "decode tile geometry");

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int l32 = lane & 31, hh = lane >> 5;
  // Per wave: NSLOT DMA slots (K at 2s·TILEBS, V after it): 4·TILEB in all for both.
  constexpr int WREG = NSLOT * 2 * TILEBS;
  static_assert(WREG == 4 * TILEB, "per-wave LDS region");
  char* const ring = smem + wave * WREG;

  const int split = blockIdx.x;
  const int u = blockIdx.y + gridDim.y * blockIdx.z;    // (b·H_kv + kvh)·nrt + rt
  const int rt = u % dp.nrt;
  const int bk = u / dp.nrt;
  const int kvh = bk % p.Hkv, b = bk / p.Hkv;
  const float c = p.c_log2;
  const int C = kv_len(p, pg, b);

  // The lane's query row of this tile: row = g·R + q of kv head kvh's group (h = kvh + g·H_kv).
  const int row = rt * 32 + l32;
  const bool rvalid = row < dp.rows;
  i16x8 qf[DP / 16];
  // Causal: the lane's query index sees keys 0 .. qcol (the host caps C at R, past which no
  // row sees a key; paged: the R rows are the sequence's last R keys).
  const int qcol = rvalid ? row % p.R + (PG::paged ? C - p.R : 0) : 0x3fffffff;
  // Sliding window (mask row > key + window): the lane's first visible key (host: skip_ok).
  const int wlo = p.mask.window ? qcol - (int)min(p.mask.window_size, 0x3fffffffu) : -0x40000000;
  {
    const int g = rvalid ? row / p.R : 0, q = rvalid ? row % p.R : 0;
    const int h = kvh + g * p.Hkv;
    const uint16_t* qrow =
        (const uint16_t*)p.q.ptr + (int64_t)b * p.q.sb + (int64_t)h * p.q.sh + (int64_t)q * p.q.ss;
#pragma unroll
    for (int s = 0; s < DP / 16; ++s) {
      const int d0 = I4 ? 32 * (s >> 1) + 16 * hh + 8 * (s & 1) : 16 * s + 8 * hh;
      i16x8 v = i16x8{0, 0, 0, 0, 0, 0, 0, 0};
      if (rvalid && d0 < p.D) v = *reinterpret_cast<const i16x8*>(qrow + d0);
      qf[s] = I4 ? i4_order<E>(v) : v;
    }
  }

  // Keys of this split: [k0, k1); this wave's tiles k0 + 32·(wave + 4i).
  const int k0 = kv_split_start<PG>(p, C, split, dp.chunk);
  const int k1 = min(C, k0 + dp.chunk);
  const int nt = k1 > k0 ? (k1 - k0 + BK - 1) / BK : 0;
  // Paged bodies keep the tile bookkeeping on the scalar path (the wave id is uniform).
  const int uwave = PG::paged ? __builtin_amdgcn_readfirstlane(wave) : wave;
  const int mine = nt > uwave ? (nt - uwave + 3) / 4 : 0;
  MFA_PAGE_QUEUE(BK)

  // LDS-DMA of one 32-row tile: piece n holds rows n·RP .. n·RP + RP - 1 (Tile16 rows are
  // contiguous); lane l lands at byte 16·l of it = row n·RP + l / CPR, physical chunk l % CPR,
  // so it fetches logical chunk (l % CPR) ^ swz(row).  Rows past C and chunks past D read as
  // zeros (range-checked descriptor per piece, out-of-row chunks out of range).
  constexpr int CPR = ROWBS / 16;
  constexpr int SH = I4 ? 1 : 0;  // element -> byte offsets
  // Packed INT4 K rows: 16-byte chunk c of row r at physical chunk c ^ swz4(r), so the 8-byte
  // fragment reads of a half-wave (32 rows, one chunk) spread over 16 slots (2-way at most).
  auto swz4 = [](int r) {
    if constexpr (CPR == 2) return (r >> 3) & 1;
    else if constexpr (CPR == 4) return (r >> 2) & 3;
    else return (((r >> 1) & 1) << 2) | ((r >> 2) & 3);
  };
  const int ssb = (int)(p.k.ss >> SH);
  int poff[NPC], voff[NPC];
#pragma unroll
  for (int n = 0; n < NPC; ++n) {
    const int r = n * RP + lane / CPR;
    const int ch = I4 ? (lane % CPR) ^ swz4(r) : (lane % CPR) ^ T::swz(r);
    poff[n] = ch * 16 < (p.D >> SH) ? r * ssb + ch * 16 : 0x40000000;
    // V: the same chunk placement as K (INT4: the transposed 4-bit reads below).
    voff[n] = ch * 16 < (p.D >> SH) ? r * ssb + ch * 16 : 0x40000000;
  }
  const char* khead = (const char*)p.k.ptr + kv_head_bytes(pg, kvh) +
                      (PG::paged ? 0 : ((int64_t)b * p.k.sb + (int64_t)kvh * p.k.sh) >> SH);
  const char* vhead = (const char*)p.v.ptr + kv_head_bytes(pg, kvh) +
                      (PG::paged ? 0 : ((int64_t)b * p.v.sb + (int64_t)kvh * p.v.sh) >> SH);
  const int kbytes = (int)((int64_t)(C - 1) * ssb + (p.D >> SH));
  const int vbytes = (int)((int64_t)(C - 1) * (p.v.ss >> SH) + (p.D >> SH));
  auto issue = [&](int i, int slot, int page) {
    const int t = tile_key(i);
    char* kdst = ring + slot * 2 * TILEBS;
    int nk, nv;
    const char* kp = kv_tile(pg, khead, page, t, C, ssb, p.D >> SH, kbytes, &nk);
    // V rows share the K piece geometry when the row strides agree (host-checked).
    const char* vp = kv_tile(pg, vhead, page, t, C, ssb, p.D >> SH, vbytes, &nv);
#pragma unroll
    for (int n = 0; n < NPC; ++n) lds_dma16(kp, nk, poff[n], kdst + n * 1024);
#pragma unroll
    for (int n = 0; n < NPC; ++n) lds_dma16(vp, nv, voff[n], kdst + TILEBS + n * 1024);
  };
  // ds_read_b64_tr_b8 lanes (see attention_fwd_i8.hip): in each 16-lane group, lane 2j supplies
  // the row of key acc_row(j + 8s, hh) and receives column d0 + (lane & 15) of the 8 rows.
  const int trj = (lane & 15) >> 1;
  const int trg = (lane >> 4) & 1;
  const int trow0 = acc_row(trj, hh), trow1 = acc_row(trj + 8, hh);
  // INT4 V^T fragments by ds_read_b64_tr_b4: in each 16-lane group lane r supplies row r (16
  // nibbles = 16 d's of one key) and receives nibble (lane & 15) of all 16 rows, i.e. d =
  // dt·32 + l32 for 16 keys: nibbles 0-7 are k-step 0's fragment, 8-15 k-step 1's.  The rows
  // are chosen so that, after nib_widen's slot order (FP16: slot j <- nibble pi(j), pi = 0 2 4 6
  // 1 3 5 7; BF16: natural), slot j of k-step ks holds key acc_row(8·ks + j, hh), the key order
  // of the packed P.
  int v4off = 0, v4sw = 0;
  if constexpr (I4) {
    const int r = lane & 15;
    constexpr int PINV[8] = {0, 4, 1, 5, 2, 6, 3, 7};  // pi^-1
    const int jj = E::prec == P_FP16 ? PINV[r & 7] : (r & 7);
    const int key = acc_row(8 * (r >> 3) + jj, hh);
    v4off = key * ROWBS + 8 * ((lane >> 4) & 1);
    v4sw = swz4(key);
  }
  const float zk = (float)(p.k.zp + (I4 ? 8 : 0)), zv = (float)(p.v.zp + (I4 ? 8 : 0));

  f32x16 o[ND];
#pragma unroll
  for (int dt = 0; dt < ND; ++dt) o[dt] = zero16();
  float m = -kFltMax, lh = 0.f;

#pragma unroll
  // (Paged: NSLOT = 2, so the prologue issues tile 0 and step i tile i + 1.)
  for (int n = 0; n < NSLOT - 1; ++n)
    if (mine > n) issue(n, n, pg0);
  for (int i = 0; i < mine; ++i) {
    const int slot = i % NSLOT;
    if (i + NSLOT - 1 < mine) {
      issue(i + NSLOT - 1, (i + NSLOT - 1) % NSLOT, pg1);
      pg_advance(i);
      __builtin_amdgcn_s_waitcnt(vm_wait((NSLOT - 1) * 2 * NPC));  // tile i landed
    } else if (NSLOT >= 4 && i + 2 < mine) {
      __builtin_amdgcn_s_waitcnt(vm_wait(4 * NPC));  // tiles i + 1, i + 2 still in flight
    } else if (NSLOT >= 3 && i + 1 < mine) {
      __builtin_amdgcn_s_waitcnt(vm_wait(2 * NPC));  // tile i + 1 still in flight
    } else {
      wait_vm();
    }
    const char* kt = ring + slot * 2 * TILEBS;
    const char* vt = kt + TILEBS;
    const int t = tile_key(i);

    // S^T = K·Q^T: key l32 on the A operand's row, elements d = 16s + 8hh + j (INT4: the lane
    // order above, two k-steps per 8-byte read of the packed row).
    f32x16 sa[1];
    sa[0] = zero16();
    if constexpr (I4) {
      const char* kp = ring + slot * 2 * TILEBS;
#pragma unroll
      for (int a = 0; a < DP / 32; ++a) {
        const uint2 kb =
            *reinterpret_cast<const uint2*>(kp + l32 * ROWBS + 16 * (a ^ swz4(l32)) + 8 * hh);
        sa[0] = E::mma(nib_widen<E>(kb.x, zk), qf[2 * a], sa[0]);
        sa[0] = E::mma(nib_widen<E>(kb.y, zk), qf[2 * a + 1], sa[0]);
      }
    } else {
#pragma unroll
      for (int st = 0; st < DP / 16; ++st) {
        const uint2 kb = *reinterpret_cast<const uint2*>(kt + T::off(l32, st) + 8 * hh);
        sa[0] = E::mma(widen_i8<E>(kb.x, kb.y, zk), qf[st], sa[0]);
      }
    }
    if (t + BK > C || (p.mask.causal && t + BK - 1 > qcol) || t < wlo) {
      // Keys past C, (causal) keys past the lane's query index and (window) keys below
      // qcol - window: -inf (key offset acc_row(r, hh) within the tile).
      const int last = p.mask.causal ? min(C - 1, qcol) : C - 1;
      mask_outside<1>(sa, wlo - t - 4 * hh, last - t - 4 * hh, -__builtin_inff());
    }
    f32x16& s = sa[0];
    float mx = s[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s[r]);
    mx = cross_half_max(mx) * c;
    if (__any(mx > m)) {
      const float m_new = fmaxf(m, mx);
      const float corr = __builtin_amdgcn_exp2f(m - m_new);
      m = m_new;
      lh *= corr;
#pragma unroll
      for (int dt = 0; dt < ND; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] *= corr;
    }
    float rs = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float pv = __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], c, -m));
      s[r] = pv;
      rs += pv;
    }
    lh += rs;
    i16x8 pb[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int j = 0; j < 8; ++j) pb[ks][j] = (short)E::from_f32(s[8 * ks + j]);
    // O^T += V^T·P^T.
    if constexpr (I4) {
      const char* vp = ring + slot * 2 * TILEBS + TILEBS;
#pragma unroll
      for (int dt = 0; dt < ND; ++dt) {
        const i32x2d w = __builtin_amdgcn_ds_read_tr4_b64_v2i32(
            (__attribute__((address_space(3))) i32x2d*)(vp + v4off + 16 * (dt ^ v4sw)));
        o[dt] = E::mma(nib_widen<E>((uint32_t)w[0], zv), pb[0], o[dt]);
        o[dt] = E::mma(nib_widen<E>((uint32_t)w[1], zv), pb[1], o[dt]);
      }
    } else {
#pragma unroll
      for (int dt = 0; dt < ND; ++dt) {
        const int col = dt * 32 + 16 * trg + 8 * (lane & 1);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const char* pa = vt + T::off(ks ? trow1 : trow0, col >> 4) + (col & 15);
          const i32x2d w = __builtin_amdgcn_ds_read_tr8_b64_v2i32(
              (__attribute__((address_space(3))) i32x2d*)pa);
          o[dt] = E::mma(widen_i8<E>((uint32_t)w[0], (uint32_t)w[1], zv), pb[ks], o[dt]);
        }
      }
    }
  }

  const float l = cross_half_sum(lh);
  // The 4 waves' partials meet in LDS ([4][32][DP] O, then [4][32] (m, l)) over the ring once
  // every wave is done with it.  One split: 256 threads merge them into O and L.  Several
  // splits: they combine them into the workgroup's one partial per row (a quarter of the
  // partial traffic and merge work of a partial per wave), in the merge's arithmetic, so the
  // merge pass of a single split reproduces the in-workgroup result bit for bit.
  __syncthreads();
  float* po = reinterpret_cast<float*>(smem);
  float2* pml = reinterpret_cast<float2*>(smem + 4 * 32 * DP * 4);
  float* prow = po + (wave * 32 + l32) * DP;
#pragma unroll
  for (int dt = 0; dt < ND; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *reinterpret_cast<float4*>(prow + dt * 32 + 8 * g + 4 * hh) =
          make_float4(o[dt][4 * g], o[dt][4 * g + 1], o[dt][4 * g + 2], o[dt][4 * g + 3]);
  if (hh == 0) pml[wave * 32 + l32] = make_float2(m, l);
  __syncthreads();
  constexpr int CH = DP / 4, RPI = 256 / CH;  // 16-byte chunks per row, rows per pass
  const int ch = tid % CH;
#pragma unroll
  for (int k = 0; k < 32 / RPI; ++k) {
    const int r = tid / CH + k * RPI;
    const int qr = rt * 32 + r;
    if (qr < dp.rows) {
      if (dp.fused) {
        const int g = qr / p.R, q = qr % p.R;
        merge_partials(p, pml + r, 32, po + r * DP, 32 * DP, 4, b, kvh + g * p.Hkv, q, 4 * ch,
                       ch == 0);
      } else {
        store_split_partial(p, dp, pml + r, 32, po + r * DP, 32 * DP, u, split, r, 4 * ch);
      }
    }
  }
