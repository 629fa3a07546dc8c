"""GPU tests of the paged MLA decode with a decoupled RoPE key part and of its append
(mfa_paged_mla_rope_decode_forward, mfa_paged_latent_rope_append).  test_paged_mla_gpu.py's setting:
NaN in every latent and rope slot no sequence owns and in the outputs before the call.  The
reference is float64 numpy on K_h = [latent W_k,h | k_rope], Q_h = [q | q_rope], V_h = latent W_v,h,
held to mla_check's tolerances.  Q and the rope operands are scaled so that both score terms have the same
spread and dropping the rope term moves O by over four times the tolerance in every sequence (asserted)."""
import functools

import numpy as np
import pytest
import torch

import mfa_amd as mfa
from harness import seen, to_device
from paged_rig import (DEV, LatentCache, P, base_descriptor, i32, mla_check, nan_outputs, positions,
                       tag)
from test_mla_absorbed_gpu import make_inputs

pytestmark = pytest.mark.gpu
ROPE = 64


def reference(Q, qr, lats, krs, wk, wv, pos, rope=1.0):
    """O, L = m + log2 l in float64; row q of sequence b sees keys 0..pos[b, q]."""
    H, D = Q.shape[1], Q.shape[3]
    O, L = np.zeros(Q.shape), np.zeros(Q.shape[:3])
    for b, (lat, kr) in enumerate(zip(lats, krs)):
        c, live = lat.shape[0], pos[b] >= 0
        if not live.any():
            continue
        K, V = ((lat.astype(np.float64) @ w).reshape(c, H, D).transpose(1, 0, 2) for w in (wk, wv))
        S = np.einsum("hrd,hcd->hrc", Q[b], K) + rope * np.einsum("hre,ce->hrc", qr[b], kr)
        S = S * (np.log2(np.e) / np.sqrt(D + ROPE))
        S[:, np.arange(c)[None, :] > pos[b][:, None]] = -np.inf
        m = S[:, live].max(-1)
        p = np.exp2(S[:, live] - m[..., None])
        O[b][:, live] = (p / p.sum(-1, keepdims=True)) @ V
        L[b][:, live] = m + np.log2(p.sum(-1))
    return O, L


@functools.lru_cache(maxsize=None)
def problem(B, H, R, D, latent, prec, lens, causal=False, seed=0):
    C = max(max(lens), 1)
    lat, wk, wv, Q = make_inputs(B, H, R, C, D, latent, prec, seed + R + sum(lens))
    rng, g = np.random.default_rng(seed + 99), (D / ROPE) ** 0.25
    Q = seen(4 * Q, prec)
    qr = seen(4 * g * rng.standard_normal((B, H, R, ROPE)).astype(np.float32), prec)
    lats = [lat.reshape(B, C, latent)[b, :max(c, 0)] for b, c in enumerate(lens)]
    krs = [seen(g * rng.standard_normal((max(c, 0), ROPE)).astype(np.float32), prec) for c in lens]
    pos = positions(lens, None, R, causal, decode=True)
    O, L = reference(Q, qr, lats, krs, wk, wv, pos)
    O0, _ = reference(Q, qr, lats, krs, wk, wv, pos, rope=0.0)
    for b, c in enumerate(lens):            # the condition on the inputs: the rope term matters
        assert c <= 0 or np.abs(O[b] - O0[b]).max() > 4 * (5e-2 if prec == P.FP16 else 1e-1), b
    return Q, qr, lats, krs, wk, wv, O, L, pos


def caches(lats, krs, prec, page, fused, **kw):
    """(PagedLatentCache, PagedRopeCache): fused [latent | rope] rows in one pool, or a rope pool of
    its own whose rows are padded to 80 elements (NaN)."""
    latent = lats[0].shape[1]
    if fused:
        c = LatentCache([np.concatenate([a, k], 1) for a, k in zip(lats, krs)], prec, page, **kw)
        st = (page * (latent + ROPE), latent + ROPE)
        return (mfa.PagedLatentCache.make(prec, page, c.max_pages, c.num_pages, latent, c.pool,
                                          c.table, c.lens, strides=st),
                mfa.PagedRopeCache.make(page, c.pool[..., latent:], strides=st))
    c = LatentCache(lats, prec, page, **kw)
    rc = LatentCache([np.pad(k, ((0, 0), (0, 16)), constant_values=np.nan) for k in krs], prec, page, **kw)
    assert np.array_equal(rc.table_np, c.table_np)
    return c.struct(), mfa.PagedRopeCache.make(page, rc.pool, strides=(page * 80, 80))


def forward(Q, qr, wk, wv, pc, rc, latent, prec, msl, causal=False, lpi=None, scale=None):
    """One call on NaN-filled outputs (rc None: the no-rope call) -> (O, L, kernel names)."""
    desc = mfa.PagedMLADecodeDescriptor.make(base_descriptor(prec, causal, lpi=lpi, scale=scale),
                                             *Q.shape, latent, msl, prec)
    o, l = nan_outputs(Q.shape, torch.float32 if lpi is False else torch.float16)
    q, dk, dv = (to_device(x, prec) for x in (Q, wk, wv))
    mfa.last_launches()
    if rc is None:
        mfa.paged_mla_decode_forward(desc, q, dk, dv, pc, o, logsumexp=l)
    else:
        mfa.paged_mla_rope_decode_forward(desc, q, to_device(qr, prec), dk, dv, pc, rc, o, logsumexp=l)
    torch.cuda.synchronize()
    return o, l, [r["name"] for r in mfa.last_launches()]


def run_case(B, H, R, D, latent, prec, page, lens, fused, causal=False, lpi=None, **kw):
    Q, qr, lats, krs, wk, wv, O, L, pos = problem(B, H, R, D, latent, prec, lens, causal)
    pc, rc = caches(lats, krs, prec, page, fused, **kw)
    o, l, names = forward(Q, qr, wk, wv, pc, rc, latent, prec, max(max(lens), 1), causal, lpi)
    assert names[1:] == [f"mfa_mla_latent_paged_rope_kernel<{tag(prec)}, {latent}>",
                         f"mfa_mla_latent_merge_kernel<{tag(prec)}, {latent}, 1>"], names
    mla_check(o, l, O, L, pos, prec, f"latent {latent} {tag(prec)} page {page} lens {lens}")


# 1. Two splits of 160 keys, fused rows: over both splits, under two tiles, ending on a page edge.
@pytest.mark.parametrize("prec", [P.FP16, P.BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("latent", [256, 512])
def test_oracle_fused_rows(gpu, latent, prec):
    run_case(3, 4, 1, 64, latent, prec, 64, (300, 33, 64), True)


# 2. The smallest page, causal rows over a split boundary (limits 125..129, splits of 128 keys), a
#    rope pool with strides of its own, shuffled table with spare pages.
def test_smallest_page_causal_separate_pool(gpu):
    run_case(2, 16, 5, 128, 512, P.BF16, 32, (1000, 130), False, causal=True, spare=9, seed=5)


# 3. Rows without a visible key: an empty sequence, and one shorter than R.
@pytest.mark.parametrize("lpi", [None, False], ids=["L-fp16", "L-fp32"])
def test_dead_rows(gpu, lpi):
    run_case(3, 4, 5, 64, 256, P.FP16, 32, (0, 3, 40), True, causal=True, lpi=lpi)


# 4. A zero q_rope adds exact zeros before the exchange: the no-rope call's bits at the same scale.
def test_zero_q_rope_is_the_no_rope_call(gpu):
    B, H, R, D, latent, prec, lens = 3, 4, 1, 64, 512, P.BF16, (300, 33, 64)
    Q, qr, lats, krs, wk, wv, _, _, _ = problem(B, H, R, D, latent, prec, lens)
    pc, rc = caches(lats, krs, prec, 64, True)
    o, l, names = forward(Q, 0 * qr, wk, wv, pc, rc, latent, prec, 300, scale=0.1)
    o0, l0, names0 = forward(Q, None, wk, wv, pc, None, latent, prec, 300, scale=0.1)
    assert torch.equal(o, o0) and torch.equal(l, l0) and not torch.isnan(o).any()
    assert names == [names0[0], "mfa_mla_latent_paged_rope_kernel<BF16, 512>",
                     "mfa_mla_latent_merge_kernel<BF16, 512, 1>"] and names[2] == names0[2], (names, names0)


# 5. Ragged strided rows appended into fused rows, bits unchanged, nothing else written; then
#    lens += n -> append -> decode as one graph, replayed with new lengths.
def test_append_then_graph_replay(gpu):
    B, H, R, D, latent, prec, page, max_pages, cap = 3, 4, 4, 64, 256, P.FP16, 32, 3, 80
    lens, new = (10, 2, 82), (3, 4, 4)   # (2, 4): rows 0-1 lie before key 0; (82, 4): rows 2-3 past the cap
    rng, W, num_pages = np.random.default_rng(8), latent + ROPE, B * max_pages + 2
    pool = torch.full((num_pages, page, W), 0x7e55, dtype=torch.int16, device=DEV).view(torch.float16)
    table_np = rng.permutation(num_pages)[:B * max_pages].reshape(B, max_pages).astype(np.int32)
    table, dl, dn = torch.from_numpy(table_np).to(DEV), i32(lens), i32(new)
    wide = to_device(rng.standard_normal((B, R, W + 32)).astype(np.float32), prec)
    rows, kr = wide[:, :, 16:16 + latent], wide[:, :, 16 + latent:16 + W]      # strides (R * 352, 352)
    pc = mfa.PagedLatentCache.make(prec, page, max_pages, num_pages, latent, pool, table, dl,
                                   strides=(page * W, W))
    rc = mfa.PagedRopeCache.make(page, pool[..., latent:], strides=(page * W, W))
    want, written = pool.view(torch.int16).clone(), 0
    for b, r in np.ndindex(B, R):
        t = lens[b] - new[b] + r
        if r < new[b] and 0 <= t < cap:
            want[int(table_np[b, t // page]), t % page] = wide[b, r, 16:16 + W].view(torch.int16)
            written += 1
    assert written == 3 + 2 + 2
    adesc = mfa.PagedLatentAppendDescriptor.make(prec, B, R, latent, cap)
    mfa.last_launches()
    mfa.paged_latent_rope_append(adesc, rows, kr, pc, rc, new_lens=dn)
    torch.cuda.synchronize()
    assert [r["name"] for r in mfa.last_launches()] == ["mfa_paged_rope_append_kernel"]
    assert torch.equal(pool.view(torch.int16), want)
    pool.copy_(to_device(rng.standard_normal(tuple(pool.shape)).astype(np.float32), prec))   # finite prefixes
    q, qrope, wk, wv = (to_device(rng.standard_normal(s).astype(np.float32) * a, prec) for s, a in
                        (((B, H, R, D), 1), ((B, H, R, ROPE), 1), ((latent, H * D), latent ** -0.5),
                         ((latent, H * D), latent ** -0.5)))
    desc = mfa.PagedMLADecodeDescriptor.make(base_descriptor(prec, True), B, H, R, D, latent, cap, prec)
    (o, l), stream = nan_outputs((B, H, R, D)), torch.cuda.Stream()
    torch.cuda.synchronize()

    def step():
        dl.add_(dn)
        mfa.paged_latent_rope_append(adesc, rows, kr, pc, rc, new_lens=dn, stream=stream.cuda_stream)
        mfa.paged_mla_rope_decode_forward(desc, q, qrope, wk, wv, pc, rc, o, logsumexp=l,
                                          stream=stream.cuda_stream)

    got, graph = [], torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        step()   # warm-up outside the capture
        stream.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            step()
        for run in (step, graph.replay):
            dl.copy_(torch.tensor((60, 0, 31), dtype=torch.int32)), dn.copy_(torch.tensor((4, 2, 1), dtype=torch.int32))
            o.fill_(float("nan")), l.fill_(float("nan"))
            run()
            stream.synchronize()
            assert dl.tolist() == [64, 2, 32]
            got.append((o.clone(), l.clone(), pool.clone()))
    assert all(torch.equal(a, b) for a, b in zip(got[0], got[1])) and not torch.isnan(got[1][0]).any()
    assert torch.count_nonzero(got[1][0][1, :, :2]).item() == 0          # sequence 1: rows 0-1 dead
