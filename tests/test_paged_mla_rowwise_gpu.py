"""GPU tests of the paged MLA decode over a row-wise INT8 latent cache and of its append
(mfa_paged_mla_decode_forward_rowwise, mfa_paged_latent_append_rowwise).  test_paged_mla_rope_gpu.py's
setting: every rope and scale slot no sequence owns holds NaN (latent bytes: 0x7f), outputs are NaN before
the call.  Key j's latent row is scale_j * q_j: the oracle test holds the call to float64 numpy on those
exact values, the identity test to the 16-bit call's bits on a pool of the rows rounded to the 16-bit type.
Latent rows carry per-token magnitudes 2^U[-2, 2], and replacing every scale by the mean scale moves O by
over four times the tolerance in every sequence (asserted), so a wrong or misplaced scale shows."""
import functools

import numpy as np
import pytest
import torch

import mfa_amd as mfa
from harness import TORCH_DTYPE, seen, to_device
from paged_rig import DEV, LatentCache, P, base_descriptor, i32, mla_check, nan_outputs, scatter, tag
from test_paged_mla_rope_gpu import ROPE, caches, forward, problem as rope_problem, reference

pytestmark = pytest.mark.gpu


def quantise(x):
    """The append's formula on float32 rows [n, latent] -> (int8 bytes, float32 scales)."""
    a = np.fmax.reduce(np.abs(x), axis=1, initial=0).astype(np.float32)
    scale = np.where(a >= np.float32(2.0 ** -64), a / np.float32(127), np.float32(1)).astype(np.float32)
    r = (x / scale[:, None]).astype(np.float64)
    q = np.clip(np.sign(r) * np.floor(np.abs(r) + 0.5), -127, 127)      # half away from zero
    return np.where(np.isnan(r), 0, q).astype(np.int8), scale


@functools.lru_cache(maxsize=None)
def problem(B, H, R, D, latent, prec, lens, causal=False, seed=0):
    """The rope test's problem with the latent rows spread over four octaves per token and quantised:
    (Q, q_rope, bytes, scales, k_rope, w_k, w_v, O, L, pos), the reference on scale * q exactly."""
    Q, qr, lats, krs, wk, wv, _, _, pos = rope_problem(B, H, R, D, latent, prec, lens, causal, seed)
    rng = np.random.default_rng(seed + 7)
    qs, scs = zip(*(quantise(seen(a * np.exp2(rng.uniform(-2, 2, (a.shape[0], 1))).astype(np.float32), prec))
                    for a in lats))
    exact = [s.astype(np.float64)[:, None] * q for q, s in zip(qs, scs)]
    O, L = reference(Q, qr, exact, krs, wk, wv, pos)
    flat = [np.full_like(s, s.mean() if s.size else 1, np.float64)[:, None] * q for q, s in zip(qs, scs)]
    Om, _ = reference(Q, qr, flat, krs, wk, wv, pos)
    for b, c in enumerate(lens):            # the condition on the inputs: the per-token scale matters
        assert c <= 0 or np.abs(O[b] - Om[b]).max() > 4 * (5e-2 if prec == P.FP16 else 1e-1), b
    return Q, qr, qs, scs, krs, wk, wv, O, L, pos


def rw_caches(qs, scs, krs, prec, page, rope=True, **kw):
    """(PagedLatentCache INT8, PagedLatentScales, PagedRopeCache or None) over fused [latent bytes | rope]
    rows, or latent bytes alone; the three scatters share one block table."""
    latent = qs[0].shape[1]
    (bytes_np,), table = scatter((list(qs),), page, fill=0x7f, **kw)
    sc = LatentCache([s[:, None] for s in scs], P.FP32, page, **kw)
    assert np.array_equal(sc.table_np, table)
    pool = torch.from_numpy(bytes_np).to(DEV)
    if rope:
        kr = LatentCache(list(krs), prec, page, **kw).pool.view(torch.int8)
        pool = torch.cat([pool, kr], dim=-1).contiguous()
    W = pool.shape[-1]
    pc = mfa.PagedLatentCache.make(P.INT8, page, sc.max_pages, sc.num_pages, latent, pool, sc.table, sc.lens,
                                   strides=(page * W, W))
    rc = mfa.PagedRopeCache.make(page, pool[..., latent:], strides=(page * W // 2, W // 2)) if rope else None
    return pc, mfa.PagedLatentScales.make(page, sc.pool), rc


def forward_rw(Q, qr, wk, wv, pc, sc, rc, latent, prec, msl, causal=False, lpi=None):
    """One row-wise call on NaN-filled outputs -> (O, L, kernel names)."""
    desc = mfa.PagedMLADecodeDescriptor.make(base_descriptor(prec, causal, lpi=lpi), *Q.shape, latent, msl, prec)
    o, l = nan_outputs(Q.shape, torch.float32 if lpi is False else torch.float16)
    q, dk, dv = (to_device(x, prec) for x in (Q, wk, wv))
    mfa.last_launches()
    mfa.paged_mla_decode_forward_rowwise(desc, q, dk, dv, pc, sc, o, q_rope=None if rc is None else to_device(qr, prec),
                                         rope=rc, logsumexp=l)
    torch.cuda.synchronize()
    return o, l, [r["name"] for r in mfa.last_launches()]


# 1. Two splits of 160 keys, a length under two tiles, a length ending on a page edge; fused rows.
@pytest.mark.parametrize("prec", [P.FP16, P.BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("latent", [256, 512])
def test_oracle_fused_rows(gpu, latent, prec):
    lens = (300, 33, 64)
    Q, qr, qs, scs, krs, wk, wv, O, L, pos = problem(3, 4, 1, 64, latent, prec, lens)
    pc, sc, rc = rw_caches(qs, scs, krs, prec, 64)
    o, l, _ = forward_rw(Q, qr, wk, wv, pc, sc, rc, latent, prec, 300)
    mla_check(o, l, O, L, pos, prec, f"row-wise latent {latent} {tag(prec)}")


# 2. The 16-bit call's bits on the dequantised pool: rows over a split boundary with rope on the smallest
#    page and a shuffled table with spare pages; no rope at latent 256.
@pytest.mark.parametrize("B,H,R,D,latent,prec,page,lens,rope,causal,kw", [
    (2, 16, 5, 128, 512, P.BF16, 32, (1000, 130), True, True, {"spare": 9, "seed": 5}),
    (3, 4, 1, 64, 256, P.FP16, 64, (300, 33, 64), False, False, {})], ids=["bf16-512-rope", "fp16-256"])
def test_bit_identity_with_the_16_bit_call(gpu, B, H, R, D, latent, prec, page, lens, rope, causal, kw):
    Q, qr, qs, scs, krs, wk, wv, _, _, _ = problem(B, H, R, D, latent, prec, lens, causal)
    dt = TORCH_DTYPE[prec]
    deq = [(torch.from_numpy(s)[:, None] * torch.from_numpy(q).float()).to(dt).float().numpy()
           for q, s in zip(qs, scs)]
    pc16, rc16 = caches(deq, krs, prec, page, rope, **kw)
    pc, sc, rc = rw_caches(qs, scs, krs, prec, page, rope, **kw)
    # forward() gives the rope call the default scale of the joint width; so does the row-wise call.
    o16, l16, n16 = forward(Q, qr, wk, wv, pc16, rc16 if rope else None, latent, prec, max(lens), causal)
    o, l, names = forward_rw(Q, qr, wk, wv, pc, sc, rc, latent, prec, max(lens), causal)
    assert torch.equal(o, o16) and torch.equal(l, l16) and not torch.isnan(o).any()
    assert names == [n16[0], f"mfa_mla_latent_paged_rw8_kernel<{tag(prec)}, {latent}, {str(rope).lower()}>",
                     f"mfa_mla_latent_merge_kernel<{tag(prec)}, {latent}, 1>"] and names[2] == n16[2], (names, n16)


# 3. Rows without a visible key: an empty sequence and one shorter than R, NaN in the unowned scale slots.
@pytest.mark.parametrize("lpi", [None, False], ids=["L-fp16", "L-fp32"])
def test_dead_rows(gpu, lpi):
    lens = (0, 3, 40)
    Q, qr, qs, scs, krs, wk, wv, O, L, pos = problem(3, 4, 5, 64, 256, P.FP16, lens, True)
    pc, sc, rc = rw_caches(qs, scs, krs, P.FP16, 32)
    o, l, _ = forward_rw(Q, qr, wk, wv, pc, sc, rc, 256, P.FP16, 40, True, lpi)
    mla_check(o, l, O, L, pos, P.FP16, f"dead rows lpi {lpi}")


# 4. Ragged strided rows quantised into fused rows, bytes, scales and rope bits by the host formula and
#    nothing else written; then lens += n -> append -> decode as one graph, replayed with new lengths.
def test_append_then_graph_replay(gpu):
    B, H, R, D, latent, prec, page, max_pages, cap = 3, 4, 4, 64, 256, P.BF16, 32, 3, 80
    lens, new = (10, 2, 82), (3, 4, 4)   # (2, 4): rows 0-1 lie before key 0; (82, 4): rows 2-3 past the cap
    rng, W, num_pages = np.random.default_rng(8), latent + 2 * ROPE, B * max_pages + 2
    pool = torch.full((num_pages, page, W), 0x5a, dtype=torch.int8, device=DEV)
    spool = torch.full((num_pages, page + 4), -7.5, dtype=torch.float32, device=DEV)
    table_np = rng.permutation(num_pages)[:B * max_pages].reshape(B, max_pages).astype(np.int32)
    table, dl, dn = torch.from_numpy(table_np).to(DEV), i32(lens), i32(new)
    x = rng.standard_normal((B, R, latent + ROPE + 32)).astype(np.float32)
    x[0, 0, 16:16 + latent] = 0                      # an all-zero row
    x[0, 1, 20] = np.nan                             # one NaN element
    x[1, 2, 16:16 + latent] *= 2.0 ** -70            # amax below 2^-64, non-zero in BF16
    wide = to_device(x, prec)
    rows, kr = wide[:, :, 16:16 + latent], wide[:, :, 16 + latent:16 + latent + ROPE]   # strides (R * 352, 352)
    pc = mfa.PagedLatentCache.make(P.INT8, page, max_pages, num_pages, latent, pool, table, dl, strides=(page * W, W))
    rc = mfa.PagedRopeCache.make(page, pool[..., latent:], strides=(page * W // 2, W // 2))
    sc = mfa.PagedLatentScales.make(page, spool, page_stride=page + 4)
    qh, sh = quantise(rows.float().cpu().numpy().reshape(B * R, latent))
    want, swant, written = pool.clone(), spool.clone(), 0
    for b, r in np.ndindex(B, R):
        t = lens[b] - new[b] + r
        if r < new[b] and 0 <= t < cap:
            pg = int(table_np[b, t // page])
            want[pg, t % page, :latent] = torch.from_numpy(qh[b * R + r]).to(DEV)
            want[pg, t % page, latent:] = kr[b, r].contiguous().view(torch.int8)
            swant[pg, t % page] = float(sh[b * R + r])
            written += 1
    assert written == 3 + 2 + 2 and sh[0] == 1 and qh[1, 4] == 0 and sh[1] > 0        # zero row, NaN element
    assert sh[1 * R + 2] == 1 and float(rows[1, 2].float().abs().max()) > 0           # the tiny row
    adesc = mfa.PagedLatentAppendDescriptor.make(prec, B, R, latent, cap)
    mfa.last_launches()
    mfa.paged_latent_append_rowwise(adesc, rows, pc, sc, k_rope=kr, rope=rc, new_lens=dn)
    torch.cuda.synchronize()
    assert [r["name"] for r in mfa.last_launches()] == ["mfa_paged_latent_append_rw8_kernel<BF16>"]
    assert torch.equal(pool, want) and torch.equal(spool.view(torch.int32), swant.view(torch.int32))
    # Finite prefixes for the decode: every slot rewritten through the append's formula on the host.
    fq, fs = quantise(rng.standard_normal((num_pages * page, latent)).astype(np.float32))
    pool[..., :latent] = torch.from_numpy(fq).to(DEV).view(num_pages, page, latent)
    pool[..., latent:] = to_device(rng.standard_normal((num_pages, page, ROPE)).astype(np.float32), prec).view(torch.int8)
    spool[:, :page] = torch.from_numpy(fs).to(DEV).view(num_pages, page)
    q, qrope, wk, wv = (to_device(rng.standard_normal(s).astype(np.float32) * a, prec) for s, a in
                        (((B, H, R, D), 1), ((B, H, R, ROPE), 1), ((latent, H * D), latent ** -0.5),
                         ((latent, H * D), latent ** -0.5)))
    desc = mfa.PagedMLADecodeDescriptor.make(base_descriptor(prec, True), B, H, R, D, latent, cap, prec)
    (o, l), stream = nan_outputs((B, H, R, D)), torch.cuda.Stream()
    torch.cuda.synchronize()

    def step():
        dl.add_(dn)
        mfa.paged_latent_append_rowwise(adesc, rows, pc, sc, k_rope=kr, rope=rc, new_lens=dn,
                                        stream=stream.cuda_stream)
        mfa.paged_mla_decode_forward_rowwise(desc, q, wk, wv, pc, sc, o, q_rope=qrope, rope=rc, logsumexp=l,
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
            got.append((o.clone(), l.clone(), pool.clone(), spool.clone()))
    assert all(torch.equal(a, b) for a, b in zip(got[0], got[1])) and not torch.isnan(got[1][0]).any()
    assert torch.count_nonzero(got[1][0][1, :, :2]).item() == 0          # sequence 1: rows 0-1 dead
