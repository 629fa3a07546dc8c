"""Row-wise INT8 paged cache on the GPU: the append bit for bit against an FP32 NumPy replica, the
decode against a float64 softmax over scale * q on the replica's bytes (an append bug cannot hide
a decode bug).  Unused byte slots hold 0x7f, unused scale slots and spare pages NaN."""
import numpy as np
import pytest
import torch

import mfa_amd as mfa
from harness import seen, to_device
from paged_rig import (DEV, P, check_dead_rows, decode_check, decode_descriptor, i32, nan_outputs,
                       scatter)

pytestmark = pytest.mark.gpu
PAGE = 32


def replica(x):
    """Row-wise INT8 of x [..., D] (float32 values): (bytes, scales [...])."""
    a = np.abs(x).max(-1).astype(np.float32)
    s = np.where(a >= np.float32(2.0 ** -64), a / np.float32(127), np.float32(1)).astype(np.float32)
    q = (x.astype(np.float32) / s[..., None]).astype(np.float32).astype(np.float64)
    return np.clip(np.sign(q) * np.floor(np.abs(q) + 0.5), -127, 127).astype(np.int8), s


def reference(Q, Kd, Vd, lens, causal, W=None):
    """float64 O [B, H, R, D], L [B, H, R] (log2 units) over per-sequence K/V [Hkv, C, D]."""
    B, H, R, D = Q.shape
    O, L = np.zeros(Q.shape), np.zeros((B, H, R))
    for b, c in enumerate(lens):
        for h in range(H if c else 0):
            S = Q[b, h].astype(np.float64) @ Kd[b][h % len(Kd[b])].T / np.sqrt(D)
            t, j = c - R + np.arange(R)[:, None], np.arange(c)[None, :]
            if causal:
                S = np.where((j > t) | (j < t - (W if W is not None else c)), -np.inf, S)
            live = np.isfinite(S).any(-1)                  # a causal row before key 0 is dead
            m = np.where(live, S.max(-1), 0.0)[:, None]
            e = np.exp(S - m)
            den = np.where(live, e.sum(-1), 1.0)
            O[b, h] = (e / den[:, None]) @ Vd[b][h % len(Vd[b])]
            L[b, h] = np.where(live, (m[:, 0] + np.log(den)) * np.log2(np.e), 0.0)
    return O, L


def pools(qk, sk, qv, sv, lens=None, release_below=None):
    """The device cache and scales of per-sequence bytes [Hkv, C, D] and scales [Hkv, C]."""
    (kp, vp), table = scatter((qk, qv), PAGE, fill=0x7f)
    (ksp, vsp), _ = scatter(([s[..., None] for s in sk], [s[..., None] for s in sv]), PAGE)
    ksp, vsp = ksp[..., 0].copy(), vsp[..., 0].copy()
    for j in range(0 if release_below is None else release_below // PAGE):  # released: -1, NaN
        ksp[table[0, j]] = vsp[table[0, j]] = np.nan
        table[0, j] = -1
    dev = lambda a: torch.from_numpy(a).to(DEV)
    lens = [x.shape[1] for x in qk] if lens is None else lens
    c = mfa.PagedKVCache.make(P.INT8, PAGE, table.shape[1], kp.shape[0], qk[0].shape[0],
                              qk[0].shape[2], dev(kp), dev(vp), dev(table), i32(lens),
                              k_scale=float("nan"), v_scale=0.0)
    return c, mfa.PagedKVScales.make(PAGE, qk[0].shape[0], dev(ksp), dev(vsp))


def decode(Q, c, s, prec, Hkv, max_seq_len, causal=False, W=None):
    o, l = nan_outputs(Q.shape)
    mfa.paged_decode_forward_rowwise(decode_descriptor(Q, Hkv, prec, max_seq_len, causal, W=W),
                                     to_device(Q, prec), c, s, o, l)
    return o, l


@pytest.mark.parametrize("D", [48, 128, 256])
@pytest.mark.parametrize("prec", [P.FP16, P.BF16], ids=["f16", "bf16"])
def test_append_matches_the_replica_bit_for_bit(prec, D):
    B, R, Hkv, lens, new = 4, 40, 3, (50, 70, 7, 65), (0, 40, 7, 33)   # 40 rows cross a page edge
    rng = np.random.default_rng(D)
    X = [seen((rng.standard_normal((B, R, Hkv * D)) * np.exp2(rng.integers(-6, 6, (B, R, 1))))
              .astype(np.float32), prec) for _ in range(2)]
    for x in X:
        x[1, 0, :D] = 0.0                                   # an all-zero head row
        if prec == P.BF16:
            x[1, 1, D:2 * D] = np.float32(2.0 ** -70)       # amax below the 2^-64 floor
    tab = np.random.default_rng(5).permutation(3 * B + 2)[:3 * B].astype(np.int32).reshape(B, 3)
    want = [np.full((3 * B + 2, Hkv, PAGE, D), 0x55, np.int8) for _ in X]      # sentinels
    wsc = [np.full((3 * B + 2, Hkv, PAGE), -7.0, np.float32) for _ in X]
    for b in range(B):
        for r in range(new[b]):
            t = lens[b] - new[b] + r
            for w, x in enumerate(X):
                want[w][tab[b, t // PAGE], :, t % PAGE], wsc[w][tab[b, t // PAGE], :, t % PAGE] = \
                    replica(x[b, r].reshape(Hkv, D))
    got = [torch.full(w.shape, 0x55, dtype=torch.int8, device=DEV) for w in want]
    gsc = [torch.full(w.shape, -7.0, dtype=torch.float32, device=DEV) for w in wsc]
    c = mfa.PagedKVCache.make(P.INT8, PAGE, tab.shape[1], want[0].shape[0], Hkv, D, got[0], got[1],
                              torch.from_numpy(tab).to(DEV), i32(lens))
    s = mfa.PagedKVScales.make(PAGE, Hkv, gsc[0], gsc[1])
    k, v = (to_device(x, prec).view(B, R, Hkv, D).permute(0, 2, 1, 3) for x in X)   # strided views
    mfa.paged_kv_append_rowwise(mfa.PagedAppendDescriptor.make(prec, B, Hkv, R, D, 96), k, v, c, s,
                                new_lens=i32(new))
    for w in range(2):
        assert np.array_equal(gsc[w].cpu().numpy(), wsc[w]), w
        assert np.array_equal(got[w].cpu().numpy(), want[w]), w


def problem(H, Hkv, R, D, prec, lens, seed=0, kexp=(0, 1), vexp=(0, 1), qmul=1.0):
    """Q and, for K then V, per-sequence replica bytes, scales, float64 values and the 16-bit rows
    they were made from (normals x 2^U[exp range])."""
    rng = np.random.default_rng(seed + D + R)
    Q = seen((qmul * rng.standard_normal((len(lens), H, R, D))).astype(np.float32), prec)
    out = []
    for lo, hi in (kexp, vexp):
        X = [seen((rng.standard_normal((Hkv, c, D)) *
                   np.exp2(rng.uniform(lo, hi, (Hkv, c, 1)))).astype(np.float32), prec) for c in lens]
        qs = [replica(x) for x in X]
        out += [[q for q, _ in qs], [s for _, s in qs],
                [q.astype(np.float64) * s[..., None] for q, s in qs], X]
    return Q, out


CASES = [(prec, D, H, Hkv, R, mask) for prec in (P.FP16, P.BF16) for D in (64, 128, 256)
         for H, Hkv, R in ((4, 4, 1), (32, 4, 2)) for mask in ("none", "causal")]
CASES += [(P.FP16, 128, 4, 4, 1, "window"), (P.BF16, 64, 32, 4, 2, "window")]


@pytest.mark.parametrize("prec,D,H,Hkv,R,mask", CASES, ids=lambda v: str(getattr(v, "name", v)))
def test_decode_matches_float64(prec, D, H, Hkv, R, mask):
    lens = (0, 1, 33, 700) if mask != "window" else (700,)
    W = 40 if mask == "window" else None
    Q, (qk, sk, Kd, _, qv, sv, Vd, _) = problem(H, Hkv, R, D, prec, lens)
    O, L = reference(Q, Kd, Vd, lens, mask != "none", W)
    c, s = pools(qk, sk, qv, sv, release_below=None if W is None else lens[0] - R - W)
    o, l = decode(Q, c, s, prec, Hkv, 4096, mask != "none", W)   # 4096: 700 keys span several splits
    t = np.array(lens)[:, None] - R + np.arange(R)[None, :]
    live = np.broadcast_to(((np.array(lens) > 0)[:, None] & ((t >= 0) | (mask == "none")))[:, None],
                           L.shape)
    check_dead_rows(o.cpu().numpy(), l.float().cpu().numpy().astype(np.float64), live, True)
    dead = torch.from_numpy(~live).to(DEV)
    l = l.float().masked_fill(dead, 0.0)    # the dead rows' floor is checked; the reference has 0
    decode_check(o, l, O, L, lens, f"{mask} D{D} H{H}")


def test_scale_range_keeps_fp16_p_precise():
    # Scales ~ 2^(U - 5.5): V over 2^-24 .. 2^2, K over 2^-10 .. 2^2; Q small, so scores stay O(1).
    H, Hkv, D, lens = 4, 4, 128, (200,)
    Q, (qk, sk, Kd, _, qv, sv, Vd, _) = problem(H, Hkv, 1, D, P.FP16, lens, 3, (-4.5, 7.5),
                                                (-18.5, 7.5), 2.0 ** -7.5)
    assert sv[0].min() < 2.0 ** -22 and sv[0].max() > 1 and sk[0].min() < 2.0 ** -8
    O, L = reference(Q, Kd, Vd, lens, False)
    S = np.einsum("hd,hcd->hc", Q[0, :, 0].astype(np.float64), Kd[0]) / np.sqrt(D)
    e = np.exp(S - S.max(-1, keepdims=True))
    assert (e / e.sum(-1, keepdims=True)).max() < 0.5      # no row dominated by a single key
    c, s = pools(qk, sk, qv, sv)
    o, l = decode(Q, c, s, P.FP16, Hkv, 256)
    err = np.abs(o.cpu().numpy() - O).max()
    print(f"scale range: O err {err:.3e}, max |O| {np.abs(O).max():.3e}")
    assert err < 2e-3 * np.abs(O).max()                    # decode_check's bound, relative to max |O|
    assert np.abs(l.float().cpu().numpy() - L).max() < 7e-3 + 2 ** -11 * np.abs(L).max()


def test_append_then_decode_round_trip():
    # Eager on one stream: lens += n, append, decode; the new rows' slots hold the fills before.
    H, Hkv, D, n, lens, prec = 8, 2, 128, 3, (40, 65), P.BF16
    Q, (qk, sk, Kd, Xk, qv, sv, Vd, Xv) = problem(H, Hkv, 1, D, prec, lens)
    cut = lambda xs, fill: [np.concatenate([x[:, :-n], np.full_like(x[:, -n:], fill)], 1) for x in xs]
    c, s = pools(cut(qk, 0x7f), cut(sk, np.nan), cut(qv, 0x7f), cut(sv, np.nan),
                 lens=[x - n for x in lens])
    c._keep[3].add_(n)
    k, v = (to_device(np.stack([x[:, -n:] for x in X]), prec) for X in (Xk, Xv))
    mfa.paged_kv_append_rowwise(mfa.PagedAppendDescriptor.make(prec, len(lens), Hkv, n, D, 96),
                                k, v, c, s)
    o, l = decode(Q, c, s, prec, Hkv, 96)
    O, L = reference(Q, Kd, Vd, lens, False)
    decode_check(o, l, O, L, lens, "round trip")
