// decode16_quant_body.h — the INT8 / INT4 16-row decode body (attention_decode.hip), as text.
//
// Not a stand-alone header: it is the statements of a kernel body, included inside
// mfa_fwd_decode16_kernel and mfa_fwd_decode16_paged_kernel, in their quantised branch.
// Contract of the place that includes it:
//   * a __global__ function template with parameters E (element traits), DP (padded head
//     width) and SRC (SRC_I8 or SRC_I4);
//   * a type PG in scope, the addressing policy (ContiguousKv or PagedKvPolicy), and an object
//     `pg` of it;
//   * `dp`, a DecodeParams (or a reference to one), and `smem`, the dynamic LDS array.
// It ends the kernel: nothing may follow it but the closing braces.  It defines and undefines
// DEC16_KLOAD and DEC16_STEP.
//
// Why text and not a function: the same statements lifted into a __device__ __forceinline__
// function compile to other code in the contiguous kernels (up to 84 more instructions) and
// measured 4-6 % slower at INT4; included inside the __global__ function they compile to
// within 5 instructions of the body that was written in place, and measure the same
// ("Paged decode", the paragraph on shared bodies; profiles/decode_paged_ab.txt
// parts 3 and 5).
  const FwdParams& p = dp.f;
  constexpr bool I4 = SRC == SRC_I4;
  static_assert(!(PG::paged && I4), "paged caches: 16-bit and INT8");
  // V ring slots: 3 (two tiles ahead); 2 at D = 256 (one ahead: two workgroups per CU).
  constexpr int BK = I4 ? 64 : 32, NKB = BK / 16, NV = DP == 256 ? 2 : 3, NDT = DP / 32;
  constexpr int NDB = DP / 16;
  constexpr int SH = I4 ? 1 : 0;            // element -> byte offsets
  constexpr int ROWBS = DP >> SH;           // stored bytes per row
  constexpr int TILEBS = BK * ROWBS;        // one stored key tile
  constexpr int NPV = TILEBS / 1024;        // V DMA pieces per tile
  constexpr int RP = 1024 / ROWBS;          // rows per piece
  constexpr int CPR = ROWBS / 16;           // 16-byte chunks per row
  constexpr int KLB = ROWBS / 4;            // K bytes per lane per 16-key block
  constexpr int NKL = KLB >= 16 ? KLB / 16 : 1;  // K loads per block (b128, or one b64)
  constexpr int NI = NPV + NKB * NKL;       // vm operations per tile
  static_assert(DP == 64 || DP == 128 || DP == 256, "decode16 widths");

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int l16 = lane & 15, g = lane >> 4;
  char* const ring = smem + wave * NV * TILEBS;

  const int split = blockIdx.x;
  const int u = blockIdx.y + gridDim.y * blockIdx.z;    // b·H_kv + kvh (one row tile)
  const int kvh = u % p.Hkv, b = u / p.Hkv;
  const float c = p.c_log2;
  const int C = kv_len(p, pg, b);

  // Q^T fragments: lane (query l16, group g), k-step dt: d = g·DP/4 + 8·dt + (kI4Perm)[j].
  const int row = l16;
  const bool rvalid = row < dp.rows;
  const int qcol = rvalid ? row % p.R + (PG::paged ? C - p.R : 0) : 0x3fffffff;
  const int wlo = p.mask.window ? qcol - (int)min(p.mask.window_size, 0x3fffffffu) : -0x40000000;
  i16x8 qf[NDT];
  {
    const int gq = rvalid ? row / p.R : 0, q = rvalid ? row % p.R : 0;
    const int h = kvh + gq * p.Hkv;
    const uint16_t* qrow =
        (const uint16_t*)p.q.ptr + (int64_t)b * p.q.sb + (int64_t)h * p.q.sh + (int64_t)q * p.q.ss;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
      const int d0 = g * (DP / 4) + 8 * dt;
      i16x8 v = i16x8{0, 0, 0, 0, 0, 0, 0, 0};
      if (rvalid && d0 < p.D) v = *reinterpret_cast<const i16x8*>(qrow + d0);
      qf[dt] = I4 ? i4_order<E>(v) : v;
    }
  }

  // Keys of this split: [k0, k1); this wave's tiles k0 + BK·(wave + 4i).
  const int k0 = kv_split_start<PG>(p, C, split, dp.chunk);
  const int k1 = min(C, k0 + dp.chunk);
  const int nt = k1 > k0 ? (k1 - k0 + BK - 1) / BK : 0;
  // Paged bodies keep the tile bookkeeping on the scalar path (the wave id is uniform).
  const int uwave = PG::paged ? __builtin_amdgcn_readfirstlane(wave) : wave;
  const int mine = nt > uwave ? (nt - uwave + 3) / 4 : 0;
  MFA_PAGE_QUEUE(BK)

  const int ssb = (int)(p.k.ss >> SH);
  const char* khead = (const char*)p.k.ptr + kv_head_bytes(pg, kvh) +
                      (PG::paged ? 0 : ((int64_t)b * p.k.sb + (int64_t)kvh * p.k.sh) >> SH);
  const char* vhead = (const char*)p.v.ptr + kv_head_bytes(pg, kvh) +
                      (PG::paged ? 0 : ((int64_t)b * p.v.sb + (int64_t)kvh * p.v.sh) >> SH);
  const int kbytes = (int)((int64_t)(C - 1) * ssb + (p.D >> SH));
  const int vbytes = (int)((int64_t)(C - 1) * (p.v.ss >> SH) + (p.D >> SH));
  // K row offsets of the lane's 16-key blocks (bytes past D: out of range, read as 0).
  const int kcol = g * KLB < (p.D >> SH) ? g * KLB : 0x40000000;
  int koff[NKB];
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb) koff[kb] = (16 * kb + l16) * ssb + kcol;
  // V chunk swizzle: the 16 (INT4) / 8 + 8 (INT8) rows one transposed read gathers into a
  // 32-lane half spread over the banks (INT4: 2-way at most; INT8: conflict-free).
  auto vsw = [](int r) {
    if constexpr (I4 && CPR == 8) return ((r >> 1) & 1) | (((r >> 4) & 3) << 1);
    else if constexpr (I4) return (r >> 4) & (CPR - 1);
    else if constexpr (CPR == 16) return (r & 3) | (((r >> 2) & 1) << 2) | (((r >> 4) & 1) << 3);
    else if constexpr (CPR == 8) return ((r >> 1) & 1) | (((r >> 2) & 1) << 1) | (((r >> 4) & 1) << 2);
    else return ((r >> 2) & 1) | (((r >> 4) & 1) << 1);
  };
  // V DMA: piece n holds rows n·RP .. n·RP + RP - 1; lane l lands at physical chunk l % CPR of
  // row n·RP + l / CPR and fetches logical chunk (l % CPR) ^ vsw(row).
  int voff[NPV];
#pragma unroll
  for (int n = 0; n < NPV; ++n) {
    const int r = n * RP + lane / CPR;
    const int ch = (lane % CPR) ^ vsw(r);
    voff[n] = ch * 16 < (p.D >> SH) ? r * ssb + ch * 16 : 0x40000000;
  }
  // Transposed V reads: the row this lane supplies, and its swizzle.
  int vtrow, vtsw;
  {
    constexpr int PINV[8] = {0, 4, 1, 5, 2, 6, 3, 7};  // kI4Perm^-1
    int key;
    if constexpr (I4) {
      const int j = E::prec == P_FP16 ? PINV[l16 & 7] : (l16 & 7);
      key = 32 * (l16 >> 3) + 16 * (j >> 2) + 4 * g + (j & 3);
    } else {
      const int j = l16 >> 1;
      key = 16 * (j >> 2) + 4 * g + (j & 3);
    }
    vtrow = key * ROWBS + (I4 ? 0 : 8 * (l16 & 1));
    vtsw = vsw(key);
  }
  const float zk = (float)(p.k.zp + (I4 ? 8 : 0)), zv = (float)(p.v.zp + (I4 ? 8 : 0));

  uint32_t ka[NKB][KLB / 4], kn[NKB][KLB / 4];
#define DEC16_KLOAD(KR, TI, PAGE)                                                                 \
  {                                                                                              \
    int nb_;                                                                                     \
    const char* tp_ =                                                                            \
        kv_tile(pg, khead, PAGE, tile_key(TI), C, ssb, p.D >> SH, kbytes, &nb_);                 \
    const __amdgpu_buffer_rsrc_t rs_ =                                                           \
        __builtin_amdgcn_make_buffer_rsrc((void*)tp_, (short)0, nb_, 0x00020000);                \
    _Pragma("unroll") for (int kb = 0; kb < NKB; ++kb) {                                         \
      if constexpr (KLB >= 16) {                                                                 \
        _Pragma("unroll") for (int x = 0; x < NKL; ++x) {                                        \
          const auto a_ = __builtin_amdgcn_raw_buffer_load_b128(rs_, koff[kb] + 16 * x, 0, 0);   \
          KR[kb][4 * x] = a_[0]; KR[kb][4 * x + 1] = a_[1];                                      \
          KR[kb][4 * x + 2] = a_[2]; KR[kb][4 * x + 3] = a_[3];                                  \
        }                                                                                        \
      } else {                                                                                   \
        const auto a_ = __builtin_amdgcn_raw_buffer_load_b64(rs_, koff[kb], 0, 0);               \
        KR[kb][0] = a_[0]; KR[kb][1] = a_[1];                                                    \
      }                                                                                          \
    }                                                                                            \
  }
  auto vissue = [&](int i, int page) {
    int nb;
    const char* tp = kv_tile(pg, vhead, page, tile_key(i), C, ssb, p.D >> SH, vbytes, &nb);
    char* dst = ring + (i % NV) * TILEBS;
#pragma unroll
    for (int n = 0; n < NPV; ++n) lds_dma16(tp, nb, voff[n], dst + n * 1024);
  };

  f32x4 o[NDB];
#pragma unroll
  for (int db = 0; db < NDB; ++db) o[db] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -kFltMax, lh = 0.f;

  // Issue order V(0) K(0) V(1), then per tile i: K(i + 1) V(i + 2): V(i) always precedes K(i),
  // so one counted vmcnt wait for K(i) covers both.  Two slots (D = 256): K(0) V(0), then per
  // tile K(i + 1) V(i + 1), and the wait is for V(i).
#define DEC16_STEP(KC, KN, I)                                                                     \
  {                                                                                              \
    const int ii = (I);                                                                          \
    if (ii + 1 < mine) DEC16_KLOAD(KN, ii + 1, pg1);                                             \
    if constexpr (NV == 2) {                                                                     \
      if (ii + 1 < mine) {                                                                       \
        vissue(ii + 1, pg1);                                                                     \
        pg_advance(ii);                                                                          \
        __builtin_amdgcn_s_waitcnt(vm_wait(NI));                                                 \
      } else {                                                                                   \
        __builtin_amdgcn_s_waitcnt(vm_wait(0));                                                  \
      }                                                                                          \
    } else if (ii + 2 < mine) {                                                                  \
      vissue(ii + 2, pg2);                                                                       \
      pg_advance(ii);                                                                            \
      __builtin_amdgcn_s_waitcnt(vm_wait(NI + NPV));                                             \
    } else if (ii + 1 < mine) {                                                                  \
      __builtin_amdgcn_s_waitcnt(vm_wait(NI));                                                   \
    } else {                                                                                     \
      __builtin_amdgcn_s_waitcnt(vm_wait(0));                                                    \
    }                                                                                            \
    const char* vs = ring + (ii % NV) * TILEBS;                                                  \
    const int t = tile_key(ii);                                                                  \
    f32x4 sc[NKB];                                                                               \
    _Pragma("unroll") for (int kb = 0; kb < NKB; ++kb) {                                         \
      sc[kb] = f32x4{0.f, 0.f, 0.f, 0.f};                                                        \
      _Pragma("unroll") for (int dt = 0; dt < NDT; ++dt) {                                       \
        if constexpr (I4)                                                                        \
          sc[kb] = mma16<E>(nib_widen<E>(KC[kb][dt], zk), qf[dt], sc[kb]);                       \
        else                                                                                     \
          sc[kb] = mma16<E>(widen_i8<E>(KC[kb][2 * dt], KC[kb][2 * dt + 1], zk), qf[dt], sc[kb]); \
      }                                                                                          \
    }                                                                                            \
    if (t + BK > k1 || (p.mask.causal && t + BK - 1 > qcol) || t < wlo) {                       \
      const int last = (p.mask.causal ? min(k1 - 1, qcol) : k1 - 1) - t, first = wlo - t;        \
      _Pragma("unroll") for (int kb = 0; kb < NKB; ++kb)                                         \
        _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                          \
          const int kk = 16 * kb + 4 * g + e;                                                    \
          sc[kb][e] = kk > last || kk < first ? -__builtin_inff() : sc[kb][e];                   \
        }                                                                                        \
    }                                                                                            \
    float mx = fmaxf(fmaxf(sc[0][0], sc[0][1]), fmaxf(sc[0][2], sc[0][3]));                      \
    _Pragma("unroll") for (int kb = 1; kb < NKB; ++kb)                                           \
      _Pragma("unroll") for (int e = 0; e < 4; ++e) mx = fmaxf(mx, sc[kb][e]);                   \
    mx = xgroup_max(mx) * c;                                                                     \
    if (__any(mx > m)) {                                                                         \
      const float m_new = fmaxf(m, mx);                                                          \
      const float corr = __builtin_amdgcn_exp2f(m - m_new);                                      \
      m = m_new;                                                                                 \
      lh *= corr;                                                                                \
      _Pragma("unroll") for (int db = 0; db < NDB; ++db) o[db] *= corr;                          \
    }                                                                                            \
    float rs = 0.f;                                                                              \
    _Pragma("unroll") for (int kb = 0; kb < NKB; ++kb)                                           \
      _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                            \
        const float pv = __builtin_amdgcn_exp2f(__builtin_fmaf(sc[kb][e], c, -m));               \
        sc[kb][e] = pv;                                                                          \
        rs += pv;                                                                                \
      }                                                                                          \
    lh += rs;                                                                                    \
    i16x8 pb[NKB / 2];                                                                           \
    _Pragma("unroll") for (int cc = 0; cc < NKB / 2; ++cc)                                       \
      _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                            \
        pb[cc][e] = (short)E::from_f32(sc[2 * cc][e]);                                           \
        pb[cc][4 + e] = (short)E::from_f32(sc[2 * cc + 1][e]);                                   \
      }                                                                                          \
    _Pragma("unroll") for (int db = 0; db < NDB; ++db) {                                         \
      if constexpr (I4) {                                                                        \
        const i32x2d w = __builtin_amdgcn_ds_read_tr4_b64_v2i32(                                 \
            (__attribute__((address_space(3))) i32x2d*)(vs + vtrow + 16 * ((db >> 1) ^ vtsw) +   \
                                                        8 * (db & 1)));                          \
        o[db] = mma16<E>(nib_widen<E>((uint32_t)w[0], zv), pb[0], o[db]);                        \
        o[db] = mma16<E>(nib_widen<E>((uint32_t)w[1], zv), pb[NKB / 2 - 1], o[db]);              \
      } else {                                                                                   \
        const i32x2d w = __builtin_amdgcn_ds_read_tr8_b64_v2i32(                                 \
            (__attribute__((address_space(3))) i32x2d*)(vs + vtrow + 16 * (db ^ vtsw)));         \
        o[db] = mma16<E>(widen_i8<E>((uint32_t)w[0], (uint32_t)w[1], zv), pb[0], o[db]);         \
      }                                                                                          \
    }                                                                                            \
  }

  if (mine > 0) {
    if constexpr (NV == 2) {
      DEC16_KLOAD(ka, 0, pg0);
      vissue(0, pg0);
    } else {
      vissue(0, pg0);
      DEC16_KLOAD(ka, 0, pg0);
    }
  }
  if (NV == 3 && mine > 1) vissue(1, pg1);
  for (int i = 0; i < mine; i += 2) {
    DEC16_STEP(ka, kn, i);
    if (i + 1 < mine) DEC16_STEP(kn, ka, i + 1);
  }
#undef DEC16_STEP
#undef DEC16_KLOAD

  const float l = xgroup_sum(lh);
  // The 4 waves' partials meet in LDS ([4][16][DP] O, then [4][16] (m, l)) over the ring; one
  // split: 256 threads merge them; several: the workgroup's one partial per row (as above).
  __syncthreads();
  float* po = reinterpret_cast<float*>(smem);
  float2* pml = reinterpret_cast<float2*>(smem + 4 * 16 * DP * 4);
  float* prow = po + (wave * 16 + l16) * DP;
#pragma unroll
  for (int db = 0; db < NDB; ++db)
    *reinterpret_cast<float4*>(prow + 16 * db + 4 * g) =
        make_float4(o[db][0], o[db][1], o[db][2], o[db][3]);
  if (g == 0) pml[wave * 16 + l16] = make_float2(m, l);
  __syncthreads();
  constexpr int CH = DP / 4, RPI = 256 / CH;  // 16-byte chunks per row, rows per pass
  const int ch = tid % CH;
#pragma unroll
  for (int k = 0; k < 16 / RPI; ++k) {
    const int r = tid / CH + k * RPI;
    if (r < dp.rows) {
      if (dp.fused) {
        const int gq = r / p.R, q = r % p.R;
        merge_partials(p, pml + r, 16, po + r * DP, 16 * DP, 4, b, kvh + gq * p.Hkv, q, 4 * ch,
                       ch == 0);
      } else {
        store_split_partial(p, dp, pml + r, 16, po + r * DP, 16 * DP, u, split, r, 4 * ch);
      }
    }
  }
