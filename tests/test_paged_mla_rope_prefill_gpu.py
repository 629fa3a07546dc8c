"""GPU tests of mfa_paged_mla_rope_prefill_forward in test_paged_mla_rope_gpu.py's setting (NaN in every latent
and rope slot no sequence owns and in the outputs before the call; its float64 numpy reference on
[latent W_k | k_rope]; mla_check's tolerances; its input scaling).  NaN also fills query and q_rope rows q >= n_b."""
import functools

import numpy as np
import pytest
import torch

import mfa_amd as mfa
from harness import seen, to_device
from paged_rig import DEV, NAN, P, base_descriptor, i32, mla_check, nan_outputs, positions
from test_mla_absorbed_gpu import make_inputs
from test_paged_mla_rope_gpu import ROPE, caches, reference

pytestmark = pytest.mark.gpu


def referenced(Q, qr, lats, krs, wk, wv, pos, prec):
    """O, L; asserts that the rope term moves O by > 4 tolerances wherever a live row sees two keys or more."""
    O, L = reference(Q, qr, lats, krs, wk, wv, pos)
    O0, _ = reference(Q, qr, lats, krs, wk, wv, pos, rope=0.0)
    assert all(p.max() < 1 or np.abs(a - a0).max() > 4 * (5e-2 if prec == P.FP16 else 1e-1) for p, a, a0 in zip(pos, O, O0))
    return O, L


@functools.lru_cache(maxsize=None)
def problem(B, H, R, D, latent, prec, lens, new=None, causal=True):
    C = max(max(lens), 1)
    lat, wk, wv, Q = make_inputs(B, H, R, C, D, latent, prec, R + sum(lens))
    rng, g = np.random.default_rng(99), (D / ROPE) ** 0.25
    Q = seen(4 * Q, prec)
    qr = seen(4 * g * rng.standard_normal((B, H, R, ROPE)).astype(np.float32), prec)
    lats = [lat.reshape(B, C, latent)[b, :max(c, 0)] for b, c in enumerate(lens)]
    krs = [seen(g * rng.standard_normal((max(c, 0), ROPE)).astype(np.float32), prec) for c in lens]
    pos = positions(lens, new, R, causal)
    return (Q, qr, lats, krs, wk, wv) + referenced(Q, qr, lats, krs, wk, wv, pos, prec) + (pos,)


def poisoned(x, new):   # x [B, H, R, .] with NaN in the rows q >= n_b, which the call never uses
    q = np.arange(x.shape[2])[:, None]
    return x if new is None else np.stack([np.where(q < n, xb, np.nan) for xb, n in zip(x, new)])


def forward(Q, qr, wk, wv, pc, rc, latent, prec, msl, new=None, causal=True, lpi=None, scale=None):
    """One call on NaN-filled outputs (rc None: the no-rope call) -> (O, L, kernel names, descriptor)."""
    desc = mfa.PagedMLADecodeDescriptor.make(base_descriptor(prec, causal, lpi=lpi, scale=scale),
                                             *Q.shape, latent, msl, prec)
    o, l = nan_outputs(Q.shape, torch.float32 if lpi is False else torch.float16)
    q, qrope, dk, dv = (to_device(x, prec) for x in (poisoned(Q, new), poisoned(qr, new), wk, wv))
    mfa.last_launches()
    if rc is None:
        mfa.paged_mla_prefill_forward(desc, q, dk, dv, pc, o, new_lens=i32(new), logsumexp=l)
    else:
        mfa.paged_mla_rope_prefill_forward(desc, q, qrope, dk, dv, pc, rc, o, new_lens=i32(new), logsumexp=l)
    torch.cuda.synchronize()
    return o, l, [r["name"] for r in mfa.last_launches()], desc


# (len, n): a prefix of 35 over two tile edges; n > len, rows 0-19 before key 0; an empty sequence; 7 rows
# behind a prefix over the 128-key edge, rows 7-39 dead.  H R = 160: five blocks that straddle heads.
RAGGED = dict(B=4, H=4, R=40, D=64, lens=(75, 20, 0, 130), new=(40, 40, 0, 7))


# 1. Ragged causal chunk, fused rows, 32-key pages, spare pages.  3. At FP16, latent 512: a zero q_rope adds exact
#    zeros before the exchange, so the call gives the no-rope call's bits at the same scale.
@pytest.mark.parametrize("prec", [P.FP16, P.BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("latent", [256, 512])
def test_ragged_causal_chunk_and_zero_q_rope_identity(gpu, latent, prec):
    Q, qr, lats, krs, wk, wv, O, L, pos = problem(latent=latent, prec=prec, **RAGGED)
    pc, rc = caches(lats, krs, prec, 32, True, spare=5)
    o, l, names, desc = forward(Q, qr, wk, wv, pc, rc, latent, prec, 130, RAGGED["new"])
    assert names == [r["name"] for r in mfa.paged_mla_rope_prefill_plan(desc, pc, rc)], names
    mla_check(o, l, O, L, pos, prec, f"ragged, latent {latent}")
    if (latent, prec) == (512, P.FP16):
        o, l, names, _ = forward(Q, 0 * qr, wk, wv, pc, rc, 512, prec, 130, RAGGED["new"], scale=0.1)
        o0, l0, names0, _ = forward(Q, qr, wk, wv, pc, None, 512, prec, 130, RAGGED["new"], scale=0.1)
        assert torch.equal(o, o0) and torch.equal(l, l0) and not torch.isnan(o).any()
        assert names == [names0[0], "mfa_mla_latent_prefill_rope_kernel<F16, 512>", names0[2]], (names, names0)


# 2. A rope pool of its own with padded 80-element rows, unmasked, no new_lens, 256-key pages.
@pytest.mark.parametrize("lpi", [None, False], ids=["L-fp16", "L-fp32"])
def test_separate_pool_unmasked(gpu, lpi):
    Q, qr, lats, krs, wk, wv, O, L, pos = problem(2, 16, 33, 128, 512, P.BF16, (300, 33), causal=False)
    o, l, _, _ = forward(Q, qr, wk, wv, *caches(lats, krs, P.BF16, 256, False), 512, P.BF16, 300, causal=False, lpi=lpi)
    mla_check(o, l, O, L, pos, P.BF16, f"separate pool, unmasked, lpi {lpi}")


# 4. lens += n -> rope append -> prefill as one graph, replayed; then one more token and the rope decode call.
def test_one_graph_then_decode(gpu):
    B, H, R, D, latent, prec, page, max_pages = 2, 4, 40, 64, 256, P.FP16, 32, 4
    rng, W, g, cap = np.random.default_rng(21), latent + ROPE, (D / ROPE) ** 0.25, page * max_pages
    pool = torch.full((2 * max_pages + 3, page, W), 0x7e55, dtype=torch.int16, device=DEV).view(torch.float16)
    table = torch.from_numpy(rng.permutation(len(pool))[:B * max_pages].reshape(B, max_pages).astype(np.int32)).to(DEV)
    dl, dn, stream = i32((0, 0)), i32((0, 0)), torch.cuda.Stream()
    adesc = mfa.PagedLatentAppendDescriptor.make(prec, B, R, latent, cap)
    pc = mfa.PagedLatentCache.make(prec, page, max_pages, len(pool), latent, pool, table, dl, strides=(page * W, W))
    rc = mfa.PagedRopeCache.make(page, pool[..., latent:], strides=(page * W, W))
    _, wk, wv, _ = make_inputs(B, H, R, 1, D, latent, prec, 3)
    draw = lambda a, *shape: seen(a * rng.standard_normal(shape).astype(np.float32), prec)
    rows, kr, q, qrope = (torch.zeros(s, dtype=torch.float16, device=DEV)
                          for s in ((B, R, latent), (B, R, ROPE), (B, H, R, D), (B, H, R, ROPE)))
    dwk, dwv, (o, l) = to_device(wk, prec), to_device(wv, prec), nan_outputs((B, H, R, D))
    desc = lambda r: mfa.PagedMLADecodeDescriptor.make(base_descriptor(prec, True), B, H, r, D, latent, cap, prec)
    torch.cuda.synchronize()

    def step(prefill=True):
        dl.add_(dn)
        mfa.paged_latent_rope_append(adesc, rows, kr, pc, rc, new_lens=dn, stream=stream.cuda_stream)
        if prefill:
            mfa.paged_mla_rope_prefill_forward(desc(R), q, qrope, dwk, dwv, pc, rc, o, new_lens=dn, logsumexp=l,
                                               stream=stream.cuda_stream)

    graph, lats, krs, lens = torch.cuda.CUDAGraph(), [np.zeros((0, latent))] * B, [np.zeros((0, ROPE))] * B, (0, 0)
    with torch.cuda.stream(stream):
        step()   # warm-up outside the capture: nothing appended, every row dead
        stream.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            step()
        for new, Rn in (((40, 5), R), ((7, 40), R), ((1, 1), 1)):
            x, k, Q, qr = draw(1, B, R, latent), draw(g, B, R, ROPE), draw(4, B, H, Rn, D), draw(4 * g, B, H, Rn, ROPE)
            lats, krs = ([np.concatenate([a[b], s[b, :n]]) for b, n in enumerate(new)] for a, s in ((lats, x), (krs, k)))
            pos = positions(lens := tuple(c + n for c, n in zip(lens, new)), new if Rn == R else None, Rn, True)
            O, L = referenced(Q, qr, lats, krs, wk, wv, pos, prec)
            rows.copy_(to_device(x, prec)), kr.copy_(to_device(k, prec)), dn.copy_(i32(new))
            if Rn == R:
                q.copy_(to_device(poisoned(Q, new), prec)), qrope.copy_(to_device(poisoned(qr, new), prec))
                got = o.fill_(NAN), l.fill_(NAN)
                graph.replay()
            else:
                step(prefill=False)
                got = nan_outputs((B, H, 1, D))
                mfa.paged_mla_rope_decode_forward(desc(1), to_device(Q, prec), to_device(qr, prec), dwk, dwv, pc, rc,
                                                  got[0], logsumexp=got[1], stream=stream.cuda_stream)
            stream.synchronize()
            mla_check(*got, O, L, pos, prec, f"lens {lens} new {new} rows {Rn}")
