// mla_latent_tile_body.h — one 32-key tile of the latent-space attention
// (attention_mla_latent.hip), as text.
//
// Not a stand-alone header: it is the statements of one iteration of the key loop, included
// inside mfa_mla_latent_kernel, mfa_mla_latent_paged_kernel and mfa_mla_latent_prefill_kernel,
// between the staging of the next tile's loads and their store to LDS.  The three kernels differ
// in how a tile reaches LDS and in what leaves the loop; the arithmetic on a staged tile, and its
// order, is this text alone, which is what makes their results comparable bit for bit.
// Contract of the place that includes it:
//   * a __global__ function template with parameters E and LAT, the constants BK, DS, ND, WS,
//     XST, the types A (Arith16<E, LAT>) and the LatentParams `p` in scope;
//   * `kt`, the staged tile of keys [t, t + BK) (rows past the sequence are zeros); `qf`, the
//     wave's Q̃ fragments; `xb`, the exchange area; `wave`, `lane`, `l32`, `hh`; `c` = p.c_log2;
//   * the running state `m`, `lh`, `o[ND]`, which it updates;
//   * MLA_TILE_LEN, the key count of the sequence (keys at or past it are −inf), and
//     MLA_TILE_KLIM, the last key the lane's row sees when p.causal (later keys take the finite
//     mask value), defined by the includer and undefined here.
// Why text and not a function: see decode16_quant_body.h — the latent kernels sit at 249 VGPRs
// at latent 512, and the statements included in place compile to the code they compiled to
// when each kernel held its own copy.
    // Partial S^T over this wave's latent slice.
    f32x16 sp = zero16();
#pragma unroll
    for (int ds = 0; ds < DS; ++ds)
      sp = A::mma(A::read_row(kt, l32, wave * DS + ds, hh), qf[ds], sp);
    // Exchange: each lane's 16 partial values contiguous ([wave][lane][16 floats]); the four
    // 16-byte chunks are rotated by (lane >> 2) & 3 so the lanes of a ds_read_b128 group hit
    // distinct banks.
    const int xsw = (lane >> 2) & 3;
    {
      float* dst = xb + (wave * 64 + lane) * XST;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        *reinterpret_cast<f32x4*>(dst + 4 * (q ^ xsw)) =
            f32x4{sp[4 * q], sp[4 * q + 1], sp[4 * q + 2], sp[4 * q + 3]};
    }
    __syncthreads();
    f32x16 s;
    {
      f32x4 part[4][4];
#pragma unroll
      for (int w = 0; w < 4; ++w)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          part[w][q] = *reinterpret_cast<const f32x4*>(xb + (w * 64 + lane) * XST + 4 * (q ^ xsw));
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          s[4 * q + e] = ((part[0][q][e] + part[1][q][e]) + part[2][q][e]) + part[3][q][e];
    }

    if (t + BK > MLA_TILE_LEN || (p.causal && t + BK - 1 > MLA_TILE_KLIM)) {
      MFA_KEEP_BRANCH();
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int key = t + acc_row(i, hh);
        if (p.causal && key > MLA_TILE_KLIM) s[i] = kMaskValue;
        if (key >= MLA_TILE_LEN) s[i] = -__builtin_inff();
      }
    }
    float mx = s[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) mx = fmaxf(mx, s[i]);
    const float m_tile = cross_half_max(mx) * c;
    if (m_tile > m) {
      const float corr = __builtin_amdgcn_exp2f(m - m_tile);
      m = m_tile;
      lh *= corr;
#pragma unroll
      for (int dt = 0; dt < ND; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[dt][i] *= corr;
    }
    float rs = 0.f;
    if (m < kMaskLevel) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        s[i] = __builtin_amdgcn_exp2f(mul_rn(s[i], c) - m);
        rs += s[i];
      }
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        s[i] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[i], c, -m));
        rs += s[i];
      }
    }
    lh += rs;
    // O^T += latent[:, slice]^T · P^T
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const i16x8 pb = A::pack(s, ks);
#pragma unroll
      for (int dt = 0; dt < ND; ++dt)
        o[dt] = A::mma(A::read_tr(kt, 0, ks, wave * WS + 32 * dt, lane), pb, o[dt]);
    }
#undef MLA_TILE_LEN
#undef MLA_TILE_KLIM
