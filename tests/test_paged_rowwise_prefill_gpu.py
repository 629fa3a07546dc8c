"""Row-wise INT8 paged prefill on the GPU (mfa_paged_prefill_forward_rowwise): against a float64
softmax over scale * q of a NumPy replica of the append's quantiser, per sequence.  Pools and
data are test_paged_rowwise_gpu.py's (pools, problem): pages of 32 keys (the two segments of a
64-key tile come from distant pages, and so do their scales), a shuffled table with spare pages,
byte 0x7f in unused slots, NaN in every unused scale slot and spare page, k_scale = NaN and
v_scale = 0 in the cache struct, NaN-filled outputs.  Bounds: paged_rig.prefill_check's (the operands are exact, so the error
sources are the 16-bit kernel's plus FP32 scale arithmetic)."""
import numpy as np
import pytest
import torch

import mfa_amd as mfa
from harness import to_device
from paged_rig import (DEAD_LENS, DEAD_NEW, DEAD_R, DEV, P, decode_check, decode_descriptor, i32,
                       nan_outputs, positions, prefill_check, prefill_descriptor)
from test_paged_rowwise_gpu import pools, problem   # the replica's bytes and scales, scattered

pytestmark = pytest.mark.gpu

# Per-token exponent range of the K and V rows (normals x 2^U): the tokens' scales spread over a
# factor of two around the unit normals (RMS 1.04) that prefill_check's absolute O bounds were
# set for; an error in O grows with |V|.
EXP = (-0.5, 0.5)


def reference(Q, Kd, Vd, lens, new, causal=True, W=None):
    """float64 O [B, H, R, D], L [B, H, R] (log2 units), the rows' last keys (positions) and the
    largest softmax weight.  Row q of sequence b sits at t_q = len_b - n_b + q and attends
    j <= t_q, cut to j >= t_q - W under the window; all keys without a mask."""
    B, H, R, D = Q.shape
    pos = positions(lens, new, R, causal)
    O, L, pmax = np.zeros(Q.shape), np.zeros((B, H, R)), 0.0
    for b, c in enumerate(lens):
        rows = np.flatnonzero(pos[b] >= 0)
        t, j = pos[b][rows][:, None], np.arange(c)[None, :]
        for h in range(H if rows.size else 0):
            S = Q[b, h, rows].astype(np.float64) @ Kd[b][h % len(Kd[b])].T / np.sqrt(D)
            if causal:
                S = np.where((j > t) | (j < t - (c if W is None else W)), -np.inf, S)
            m = S.max(-1, keepdims=True)
            e = np.exp(S - m)
            den = e.sum(-1, keepdims=True)
            pmax = max(pmax, float((e / den).max()))
            O[b, h, rows] = (e / den) @ Vd[b][h % len(Vd[b])]
            L[b, h, rows] = (m + np.log(den))[:, 0] * np.log2(np.e)
    return O, L, pos, pmax


def prefill(Q, c, s, prec, Hkv, new=None, causal=True, W=None, lpi=None, max_seq_len=512):
    """One call on NaN-filled outputs; asserts that the launch log is the plan and names the
    row-wise kernel.  Returns (O, L)."""
    desc = prefill_descriptor(Q.shape, Hkv, prec, max_seq_len, causal, lpi, W=W)
    o, l = nan_outputs(Q.shape, torch.float32 if lpi is False else torch.float16)
    mfa.last_launches()
    mfa.paged_prefill_forward_rowwise(desc, to_device(Q, prec), c, s, o, new_lens=i32(new),
                                      logsumexp=l)
    torch.cuda.synchronize()
    names = [r["name"] for r in mfa.last_launches()]
    assert names == [r["name"] for r in mfa.paged_prefill_rowwise_plan(desc, c, s)]
    assert len(names) == 1 and "prefill_rw8_kernel<" in names[0] and ("window" in names[0]) == (W is not None)
    return o, l


def run_case(prec, D, H, Hkv, R, lens, new, causal=True, W=None, lpi=None, what=""):
    Q, (qk, sk, Kd, _, qv, sv, Vd, _) = problem(H, Hkv, R, D, prec, lens, 0, EXP, EXP)
    O, L, pos, _ = reference(Q, Kd, Vd, lens, new, causal, W)
    n0 = R if new is None else new[0]
    c, s = pools(qk, sk, qv, sv,
                 release_below=None if W is None else max(0, max(0, lens[0] - n0) - W))
    o, l = prefill(Q, c, s, prec, Hkv, new, causal, W, lpi)
    prefill_check(o, l, O, L, pos, prec, what)


# Causal and unmasked: R = 160 is two row blocks, the second partial; a prefix, a pure prompt, a
# chunk smaller than a wave; lengths ending mid-tile and mid-page; GQA 4 / 2.  Window: W = 40 over
# 300 keys, the pages wholly below lo_b released (table entry -1, NaN scales).
RAGGED = (160, (300, 160, 97), (160, 160, 33))
CASES = [(prec, D, "causal") + RAGGED for prec in (P.FP16, P.BF16) for D in (64, 128, 256)]
CASES += [(P.FP16, 80, "causal") + RAGGED, (P.BF16, 128, "none") + RAGGED,
          (P.FP16, 128, "window", 160, (300,), (160,)), (P.BF16, 256, "window", 33, (300,), (33,))]


@pytest.mark.parametrize("prec,D,mask,R,lens,new", CASES,
                         ids=[f"{c[0].name}-{c[1]}-{c[2]}" for c in CASES])
def test_chunks_match_float64(prec, D, mask, R, lens, new):
    run_case(prec, D, 4, 2, R, lens, new, mask != "none", 40 if mask == "window" else None,
             what=f"{mask} D{D}")


@pytest.mark.parametrize("lpi", [None, False], ids=["l16", "l32"])
def test_dead_rows_are_exact_zeros(lpi):
    run_case(P.FP16, 64, 4, 2, DEAD_R, DEAD_LENS, DEAD_NEW, lpi=lpi, what="dead rows")


def test_scale_range_keeps_fp16_p_precise():
    # test_paged_rowwise_gpu.py's generator parameters: scales ~ 2^(U - 5.5), V over 2^-24 .. 2^2,
    # K over 2^-10 .. 2^2; Q small, so scores stay O(1).  A chunk of 64 rows behind 136 keys.
    H, Hkv, D, R, lens = 4, 4, 128, 64, (200,)
    Q, (qk, sk, Kd, _, qv, sv, Vd, _) = problem(H, Hkv, R, D, P.FP16, lens, 3, (-4.5, 7.5),
                                                (-18.5, 7.5), 2.0 ** -7.5)
    assert sv[0].min() < 2.0 ** -22 and sv[0].max() > 1 and sk[0].min() < 2.0 ** -8
    O, L, _, pmax = reference(Q, Kd, Vd, lens, None)
    assert pmax < 0.5                                      # no row dominated by a single key
    c, s = pools(qk, sk, qv, sv)
    o, l = prefill(Q, c, s, P.FP16, Hkv)
    err, lerr = np.abs(o.cpu().numpy() - O).max(), np.abs(l.float().cpu().numpy() - L).max()
    print(f"scale range: O err {err:.3e}, max |O| {np.abs(O).max():.3e}, L err {lerr:.3e}")
    assert err < 2e-3 * np.abs(O).max()
    assert lerr < 7e-3 + 2 ** -11 * np.abs(L).max()


def test_append_prefill_decode_round_trip():
    # Eager on one stream and one pair of structs: lens += n, append, prefill, decode.  The chunk
    # (n = 40 rows behind a 60-key prefix) crosses a page edge; its slots hold the fills before.
    H, Hkv, D, n, lens, prec = 8, 2, 128, 40, (100,), P.BF16
    Q, (qk, sk, Kd, Xk, qv, sv, Vd, Xv) = problem(H, Hkv, n, D, prec, lens, 0, EXP, EXP)
    cut = lambda xs, fill: [np.concatenate([x[:, :-n], np.full_like(x[:, -n:], fill)], 1) for x in xs]
    c, s = pools(cut(qk, 0x7f), cut(sk, np.nan), cut(qv, 0x7f), cut(sv, np.nan),
                 lens=[x - n for x in lens])
    c._keep[3].add_(n)
    k, v = (to_device(np.stack([x[:, -n:] for x in X]), prec) for X in (Xk, Xv))
    mfa.paged_kv_append_rowwise(mfa.PagedAppendDescriptor.make(prec, 1, Hkv, n, D, 128), k, v, c, s)
    O, L, pos, _ = reference(Q, Kd, Vd, lens, None)
    o, l = prefill(Q, c, s, prec, Hkv, max_seq_len=128)
    prefill_check(o, l, O, L, pos, prec, "round trip prefill")
    # The decode row at the last position against the float64 row the chunk's last row met.
    Q1 = np.ascontiguousarray(Q[:, :, -1:])
    o1, l1 = nan_outputs(Q1.shape)
    mfa.paged_decode_forward_rowwise(decode_descriptor(Q1, Hkv, prec, 128, True), to_device(Q1, prec),
                                     c, s, o1, l1)
    decode_check(o1, l1, O[:, :, -1:], L[:, :, -1:], lens, "round trip decode")


def test_stream_capture_replays_with_new_chunks():
    # lens.add_(n) -> append -> prefill as one linear graph; the second replay against float64.
    B, H, Hkv, D, R, prec = 2, 4, 2, 128, 40, P.FP16
    start, news = (30, 50), ((20, 40), (40, 7))
    final = tuple(a + sum(n[b] for n in news) for b, a in enumerate(start))
    Q, (qk, sk, Kd, Xk, qv, sv, Vd, Xv) = problem(H, Hkv, R, D, prec, final, 0, EXP, EXP)
    keep = lambda xs, fill: [np.concatenate([x[:, :a], np.full_like(x[:, a:], fill)], 1)
                             for x, a in zip(xs, start)]
    c, s = pools(keep(qk, 0x7f), keep(sk, np.nan), keep(qv, 0x7f), keep(sv, np.nan), lens=start)
    lens, nl = c._keep[3], i32((0, 0))
    kn, vn = (torch.zeros((B, Hkv, R, D), dtype=torch.float16, device=DEV) for _ in range(2))
    desc = prefill_descriptor(Q.shape, Hkv, prec, 128)
    adesc = mfa.PagedAppendDescriptor.make(prec, B, Hkv, R, D, 128)
    q = to_device(Q, prec)
    o, l = nan_outputs(Q.shape)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()

    def step():
        lens.add_(nl)
        mfa.paged_kv_append_rowwise(adesc, kn, vn, c, s, new_lens=nl, stream=st.cuda_stream)
        mfa.paged_prefill_forward_rowwise(desc, q, c, s, o, new_lens=nl, logsumexp=l,
                                          stream=st.cuda_stream)

    with torch.cuda.stream(st):
        step()   # warm-up outside the capture: no rows, nothing appended
        st.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            step()
        st.synchronize()
        at = list(start)
        for new in news:
            for X, dst in ((Xk, kn), (Xv, vn)):
                for b in range(B):
                    dst[b, :, :new[b]] = to_device(X[b][:, at[b]:at[b] + new[b]], prec)
            nl.copy_(torch.tensor(new, dtype=torch.int32))
            o.fill_(float("nan"))
            l.fill_(float("nan"))
            graph.replay()
            st.synchronize()
            at = [a + n for a, n in zip(at, new)]
            assert lens.tolist() == at
    O, L, pos, _ = reference(Q, Kd, Vd, final, news[-1])
    prefill_check(o, l, O, L, pos, prec, "graph replay")
