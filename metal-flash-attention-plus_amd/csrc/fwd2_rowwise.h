// fwd2_rowwise.h — the softmax step of a forward tile whose keys carry a K scale and a V scale
// each (row-wise INT8 pools, attention_prefill_paged_rw8.hip).  It stands in fwd2_softmax's place
// between fwd2_qk and fwd2_pv (attention_fwd2.h), which run unchanged on the exact integers of
// the cache: fwd2_qk with RowState::negm left at zero, so S^T = K·Q^T carries no offset.
//
// The decode kernels' shifted-max scheme (attention_decode.hip, "Row-wise INT8 pools"), on a
// BK-key tile.  S^T has the keys on the accumulator rows: register 4g + k of block j is key
// 32j + 8g + 4hh + k of the tile, in the score and in the packed P alike, so a lane reads the
// three values of its keys as float4s of a strip laid out by key:
//   strip[0 .. BK)       kc  the K scale, times c = log2 e · scale where Q is not pre-scaled by
//                            it (load_q2 pre-scales on the FP16 D <= 128 path); 0 for a key that
//                            was not fetched
//   strip[BK .. 2BK)     lv  log2 of the V scale; 0 for such a key
//   strip[2BK .. 3BK)    rv  1 / V scale; 1 for such a key
// x = s · kc + lv is the log2 of the key's weight times its V scale.  The running max m is taken
// over x, the packed P operand is w = exp2(x - m) = p · vs, at most 2^THR whatever the V scales
// are, and the denominator adds w · rv = exp2(s · ks · c - m) in FP32.  O = sum w · q_V and
// l = sum w · rv are relative to the same m, so O / l needs no further factor (o_mul = 1), and
// L = m + log2 l = log2 sum exp2(s · ks · c): the lv inside m cancels against the rv inside l.
// A masked key is -inf before the max: w = 0 and, rv being finite, w · rv = 0.
#pragma once
#include "attention_fwd2.h"

namespace mfa {

// Scores to x, the masks, the row max and the lazy rescale of O and l (fwd2_max's rarely taken
// branch and threshold).  t, mask_tile, qi, p, wsz, hh: fwd2_max's.
template <class E, int DP, int BK>
__device__ __forceinline__ void fwd2_rw_max(RowState<DP>& st, f32x16 (&s)[BK / 32],
                                            const float* strip, int t, bool mask_tile, int qi,
                                            const FwdParams& p, int wsz, int hh) {
  constexpr int NJ = BK / 32, ND = DP / 32;
  constexpr float THR = 8.0f;
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int k0 = 32 * j + 8 * g + 4 * hh;
      const float4 kc = *reinterpret_cast<const float4*>(strip + k0);
      const float4 lv = *reinterpret_cast<const float4*>(strip + BK + k0);
      s[j][4 * g] = __builtin_fmaf(s[j][4 * g], kc.x, lv.x);
      s[j][4 * g + 1] = __builtin_fmaf(s[j][4 * g + 1], kc.y, lv.y);
      s[j][4 * g + 2] = __builtin_fmaf(s[j][4 * g + 2], kc.z, lv.z);
      s[j][4 * g + 3] = __builtin_fmaf(s[j][4 * g + 3], kc.w, lv.w);
    }
  if (mask_tile) {
    MFA_KEEP_BRANCH();
    // Keys t + 4hh + kk stay for lo <= kk <= hi: below C, at most qi (causal), at least
    // qi - wsz (window).
    const int base = t + 4 * hh;
    int hi = p.C - 1 - base;
    if (p.mask.causal) hi = min(hi, qi - base);
    if (p.mask.window) {
      const int lo = qi - wsz;
      mask_outside<NJ>(s, lo <= -0x40000000 ? -0x40000000 : lo - base, hi, -__builtin_inff());
    } else {
      mask_above<NJ>(s, hi, -__builtin_inff());
    }
  }
  // (Scales are finite and positive by contract, MFMA results finite: never NaN.)
  float mx = s[0][0];
#pragma unroll
  for (int k = 1; k + 1 < 16 * NJ; k += 2)
    mx = max3_nn(mx, s[k / 16][k % 16], s[(k + 1) / 16][(k + 1) % 16]);
  mx = max_nn(mx, s[NJ - 1][15]);
  mx = cross_half_maximum(mx);
  if (__any(mx > st.m + THR)) {
    MFA_KEEP_BRANCH();
    const float m_new = max_nn(st.m, mx);
    const float corr = __builtin_amdgcn_exp2f(st.m - m_new);
    st.m = m_new;
    st.lh *= corr;
#pragma unroll
    for (int dt = 0; dt < ND; ++dt)
#pragma unroll
      for (int i = 0; i < 16; ++i) st.o[dt][i] *= corr;
  }
}

// w = exp2(x - m), the row sum of w · rv, w packed as the PV B operand; straight-line code.
template <class E, int DP, int BK>
__device__ __forceinline__ void fwd2_rw_exp(RowState<DP>& st, f32x16 (&s)[BK / 32],
                                            i16x8 (&pb)[BK / 16], const float* strip, int hh) {
  using A = Arith16<E, DP>;
  constexpr int NJ = BK / 32;
  float rs[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 rv =
          *reinterpret_cast<const float4*>(strip + 2 * BK + 32 * j + 8 * g + 4 * hh);
      const float r4[4] = {rv.x, rv.y, rv.z, rv.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float w = __builtin_amdgcn_exp2f(s[j][4 * g + k] - st.m);
        s[j][4 * g + k] = w;
        rs[k] = __builtin_fmaf(w, r4[k], rs[k]);
      }
    }
  st.lh += (rs[0] + rs[1]) + (rs[2] + rs[3]);
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) pb[j * 2 + ks] = A::pack(s[j], ks);
}

template <class E, int DP, int BK>
__device__ __forceinline__ void fwd2_rw_softmax(RowState<DP>& st, f32x16 (&s)[BK / 32],
                                                i16x8 (&pb)[BK / 16], const float* strip, int t,
                                                bool mask_tile, int qi, const FwdParams& p,
                                                int wsz, int hh) {
  fwd2_rw_max<E, DP, BK>(st, s, strip, t, mask_tile, qi, p, wsz, hh);
  fwd2_rw_exp<E, DP, BK>(st, s, pb, strip, hh);
}

}  // namespace mfa
