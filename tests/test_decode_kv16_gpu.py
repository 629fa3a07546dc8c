"""GPU tests of the split-KV decode forward on FP16 / BF16 K/V caches (attention_decode.hip,
SRC_SAME; routed from launch_forward in mfa_api.cpp).  MFA_DECODE_KV16=1 routes every eligible
size, so small shapes reach the kernels; MFA_DECODE_KV16=0 is the path these calls took before
(the 128-row kernels).  Every case is held to the oracle on the stored values at the tolerance
the INT8-cache tests hold the same kernel body to (test_quant_gpu.py test_decode_split_kv), and
to the previous path within twice the O tolerance."""
import functools

import numpy as np
import pytest
import torch

import mfa_amd as mfa
import oracle_lib as ol
from harness import TORCH_DTYPE, maxerr, seen, to_device

pytestmark = pytest.mark.gpu

P = mfa.Precision
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def problem(B, H, Hkv, R, C, D, prec, causal=False, window=None):
    """Stored-value inputs and the oracle's result, computed once per case."""
    rng = np.random.default_rng(R * 13 + C + D)
    Q = seen(rng.standard_normal((B, H, R, D)).astype(np.float32), prec)
    K, V = (seen(rng.standard_normal((B, Hkv, C, D)).astype(np.float32), prec) for _ in range(2))
    ref = ol.attention(Q, K, V, causal=causal, window=window)
    for a in (Q, K, V, ref["O"], ref["L"]):
        a.setflags(write=False)
    return Q, K, V, ref


def descriptor(Qn, Kn, prec, causal=False, window=None, lpi=None):
    B, H, R, D = Qn.shape
    base = mfa.AttentionDescriptor.make(low_precision=True, precision=prec, causal=causal,
                                        window=window, low_precision_intermediates=lpi)
    return mfa.MultiHeadDescriptor.make(base, B, H, R, D, Hkv=Kn.shape[1], C=Kn.shape[2])


def forward(Qn, Kn, Vn, prec, causal=False, window=None, lpi=None, want_l=True, k=None, v=None,
            kv_strides=None):
    """One forward on device copies of the arrays (or on the given K/V tensors and strides);
    returns (O, L, launched kernel names)."""
    B, H, R, D = Qn.shape
    desc = descriptor(Qn, Kn, prec, causal, window, lpi)
    q = to_device(Qn, prec)
    k = to_device(Kn, prec) if k is None else k
    v = to_device(Vn, prec) if v is None else v
    o = torch.full((B, H, R, D), float("nan"), dtype=torch.float32, device=DEV)
    l = None
    if want_l:
        l_dtype = torch.float16 if desc.base.low_precision_intermediates else torch.float32
        l = torch.full((B, H, R), float("nan"), dtype=l_dtype, device=DEV)
    mfa.last_launches()
    mfa.MultiHeadAttention().forward(desc, q, k, v, o, l, key_strides=kv_strides,
                                     value_strides=kv_strides)
    torch.cuda.synchronize()
    return o, l, [r["name"] for r in mfa.last_launches()]


def check_case(monkeypatch, shape, prec, causal=False, window=None):
    B, H, Hkv, R, C, D = shape
    Q, K, V, ref = problem(*shape, prec, causal, window)
    monkeypatch.setenv("MFA_DECODE_KV16", "1")
    o, l, names = forward(Q, K, V, prec, causal, window)
    form = "mfa_fwd_decode16_kernel<" if (H // Hkv) * R <= 16 else "mfa_fwd_decode_kernel<"
    assert names[0].startswith(form) and names[0].endswith(", 0>"), names
    assert names[1:] in ([], ["mfa_decode_merge_kernel"], ["mfa_decode_merge4_kernel"]), names
    monkeypatch.setenv("MFA_DECODE_KV16", "0")
    o0, l0, names0 = forward(Q, K, V, prec, causal, window)
    assert not any("decode" in n for n in names0), names0
    omax = max(1.0, float(np.abs(ref["O"]).max()))
    eo, el = maxerr(o, ref["O"]), maxerr(l, ref["L"])
    print(f"{shape} {prec.name} causal={causal} window={window}: O err {eo:.3e} L err {el:.3e} "
          f"parent O err {maxerr(o0, ref['O']):.3e} route-vs-parent {maxerr(o, o0):.3e} {names}")
    assert np.isfinite(o.cpu().numpy()).all() and np.isfinite(l.float().cpu().numpy()).all()
    assert eo < 2e-3 * omax
    assert el < 7e-3 + 2 ** -11 * float(np.abs(ref["L"]).max())
    assert maxerr(o, o0) < 4e-3 * omax
    return names


@pytest.mark.parametrize("shape,prec", [
    ((2, 4, 4, 1, 1000, 128), P.FP16),
    ((1, 8, 2, 3, 777, 64), P.BF16),      # GQA: 12 rows per kv head
    ((2, 4, 1, 5, 300, 256), P.FP16),     # MQA: 20 rows, the 32-row form
    ((1, 2, 2, 1, 33, 64), P.FP16),       # one partial tile
    ((1, 4, 4, 7, 70, 96), P.BF16),       # D 96 in the 128-wide tiles
    ((1, 2, 2, 2, 200, 72), P.FP16),      # D % 16 != 0
    ((2, 4, 2, 8, 2500, 128), P.FP16),    # GQA, 16 rows, split path
    ((1, 4, 4, 2, 3000, 256), P.BF16),
    ((1, 4, 4, 1, 12000, 64), P.FP16),    # 23 splits: the one-wave merge pass
    ((1, 2, 2, 1, 24000, 64), P.FP16),    # 38 splits (> 32 partials per row): the 4-wave merge
    ((1, 16, 1, 4, 300, 128), P.FP16),    # 64 rows per kv head: two row tiles
])
def test_decode_kv16(gpu, shape, prec, monkeypatch):
    names = check_case(monkeypatch, shape, prec)
    if shape[4] == 24000:
        assert names[1:] == ["mfa_decode_merge4_kernel"], names
    elif shape[4] in (12000, 2500, 3000):
        assert names[1:] == ["mfa_decode_merge_kernel"], names


@pytest.mark.parametrize("shape,prec", [
    ((2, 4, 4, 16, 1000, 128), P.FP16),   # 16 rows: keys 0..15 at most
    ((1, 2, 2, 100, 90, 256), P.BF16),    # C < R: every key seen by the last rows
])
def test_decode_kv16_causal(gpu, shape, prec, monkeypatch):
    check_case(monkeypatch, shape, prec, causal=True)


@pytest.mark.parametrize("shape,prec,win", [
    ((1, 4, 4, 16, 1000, 128), P.FP16, 5),   # rows 6..15 lose their first keys
    ((1, 8, 2, 3, 777, 64), P.BF16, 0),      # GQA, window 0: row r sees keys >= r
])
def test_decode_kv16_window(gpu, shape, prec, win, monkeypatch):
    check_case(monkeypatch, shape, prec, window=win)


def test_strided_bshd_cache_equals_contiguous(gpu, monkeypatch):
    # K/V stored [B, C, H_kv, D] and passed by strides: the same bits as the BHSD call.
    shape, prec = (2, 4, 2, 3, 700, 128), P.FP16
    B, H, Hkv, R, C, D = shape
    Q, K, V, _ = problem(*shape, prec)
    monkeypatch.setenv("MFA_DECODE_KV16", "1")
    o, l, names = forward(Q, K, V, prec)
    kb = to_device(K, prec).permute(0, 2, 1, 3).contiguous()
    vb = to_device(V, prec).permute(0, 2, 1, 3).contiguous()
    strides = (C * Hkv * D, D, Hkv * D, 1)
    o2, l2, names2 = forward(Q, K, V, prec, k=kb, v=vb, kv_strides=strides)
    assert names == names2 and names[0].startswith("mfa_fwd_decode16_kernel<"), (names, names2)
    assert torch.equal(o, o2) and torch.equal(l, l2)


@pytest.mark.parametrize("shape,prec", [
    ((1, 2, 2, 2, 200, 72), P.FP16),      # 16-row form, D % 16 != 0
    ((1, 4, 1, 5, 100, 96), P.BF16),      # 20 rows: the 32-row form
    ((1, 2, 2, 1, 2100, 64), P.FP16),     # split path: the last split ends inside a tile
])
def test_garbage_behind_rows_and_keys_is_never_read(gpu, shape, prec, monkeypatch):
    # K/V inside a larger allocation: 8 gap elements behind every row and 40 rows behind every
    # head's last key, all NaN.  Nothing of it may reach O or L.
    B, H, Hkv, R, C, D = shape
    Q, K, V, _ = problem(*shape, prec)
    monkeypatch.setenv("MFA_DECODE_KV16", "1")
    o, l, names = forward(Q, K, V, prec)
    Cp, Dp = C + 40, D + 8
    big = []
    for x in (K, V):
        t = torch.full((B, Hkv, Cp, Dp), float("nan"), dtype=TORCH_DTYPE[prec], device=DEV)
        t[:, :, :C, :D] = to_device(x, prec)
        big.append(t)
    strides = (Hkv * Cp * Dp, Cp * Dp, Dp, 1)
    o2, l2, names2 = forward(Q, K, V, prec, k=big[0], v=big[1], kv_strides=strides)
    assert names == names2 and names[0].startswith("mfa_fwd_decode"), (names, names2)
    assert torch.isfinite(o2).all() and torch.isfinite(l2.float()).all()
    assert torch.equal(o, o2) and torch.equal(l, l2)


@pytest.mark.parametrize("shape,prec", [
    ((2, 4, 4, 1, 300, 128), P.FP16),     # fewer than 16 tiles: one split per unit
    ((2, 4, 1, 5, 300, 256), P.FP16),     # the 32-row form
])
def test_merge_pass_equals_in_workgroup_merge(gpu, shape, prec, monkeypatch):
    Q, K, V, _ = problem(*shape, prec)
    monkeypatch.setenv("MFA_DECODE_KV16", "1")
    o, l, names = forward(Q, K, V, prec)
    assert len(names) == 1, names
    o1, l1, _ = forward(Q, K, V, prec)
    assert torch.equal(o, o1) and torch.equal(l, l1)  # two identical calls
    monkeypatch.setenv("MFA_DECODE_MERGE", "1")
    o2, l2, names2 = forward(Q, K, V, prec)
    assert names2 == [names[0], "mfa_decode_merge_kernel"], names2
    assert torch.equal(o, o2) and torch.equal(l, l2)


def test_split_path_is_deterministic(gpu, monkeypatch):
    Q, K, V, _ = problem(2, 4, 2, 8, 2500, 128, P.FP16)
    monkeypatch.setenv("MFA_DECODE_KV16", "1")
    o, l, names = forward(Q, K, V, P.FP16)
    o1, l1, _ = forward(Q, K, V, P.FP16)
    assert names[1:] == ["mfa_decode_merge_kernel"], names
    assert torch.equal(o, o1) and torch.equal(l, l1)


def test_l_fp32_and_l_null(gpu, monkeypatch):
    shape, prec = (2, 4, 2, 8, 2500, 128), P.FP16
    Q, K, V, ref = problem(*shape, prec)
    monkeypatch.setenv("MFA_DECODE_KV16", "1")
    o, l, _ = forward(Q, K, V, prec)
    o32, l32, names = forward(Q, K, V, prec, lpi=False)
    assert names[0].startswith("mfa_fwd_decode16_kernel<"), names
    assert l32.dtype == torch.float32 and torch.equal(o, o32)
    assert maxerr(l32, ref["L"]) < 1e-3  # FP32 L: no FP16 storage rounding
    on, ln, names = forward(Q, K, V, prec, want_l=False)
    assert ln is None and names[0].startswith("mfa_fwd_decode16_kernel<"), names
    assert torch.equal(o, on)


def test_mla_decode_step_takes_the_route(gpu, monkeypatch):
    # mfa_mla_forward's attention runs on the decompressed BSHD K/V ([B·S, H·D]).
    B, H, Sq, Skv, D, Lat, prec = 2, 4, 1, 2048, 64, 128, P.FP16
    rng = np.random.default_rng(3)
    lat = to_device(rng.standard_normal((B * Skv, Lat)).astype(np.float32), prec)
    wk, wv = (to_device((rng.standard_normal((Lat, H * D)) / np.sqrt(Lat)).astype(np.float32), prec)
              for _ in range(2))
    q = to_device(rng.standard_normal((B, H, Sq, D)).astype(np.float32), prec)
    base = mfa.AttentionDescriptor.make(low_precision=True, precision=prec)
    res = {}
    for sw in ("1", "0"):
        monkeypatch.setenv("MFA_DECODE_KV16", sw)
        o = torch.full((B, H, Sq, D), float("nan"), dtype=torch.float32, device=DEV)
        l = torch.full((B, H, Sq), float("nan"), dtype=torch.float16, device=DEV)
        mfa.last_launches()
        mfa.mla_forward(base, lat, wk, wv, q, o, B, H, Sq, Skv, D, Lat, prec, logsumexp=l)
        torch.cuda.synchronize()
        res[sw] = (o, l, [r["name"] for r in mfa.last_launches()])
    assert any(n.startswith("mfa_fwd_decode16_kernel<F16, 64, 0>") for n in res["1"][2]), res["1"][2]
    assert not any("decode" in n for n in res["0"][2]), res["0"][2]
    o1, o0 = res["1"][0], res["0"][0]
    assert torch.isfinite(o1).all()
    assert maxerr(o1, o0) < 4e-3 * max(1.0, float(o0.abs().max()))
    # Each L lies within the oracle tolerance of the exact value, so the two within twice it.
    assert maxerr(res["1"][1], res["0"][1]) < 2 * (7e-3 + 2 ** -11 * float(res["0"][1].float().abs().max()))


def test_split_partials_under_graph_capture(gpu, monkeypatch):
    # The split partials live in library scratch: run eagerly first (the scratch does not grow
    # during capture), capture the call, then eager, replay, eager: all bit-equal.
    shape, prec = (2, 4, 2, 8, 2500, 128), P.FP16
    B, H, Hkv, R, C, D = shape
    Q, K, V, _ = problem(*shape, prec)
    monkeypatch.setenv("MFA_DECODE_KV16", "1")
    desc = descriptor(Q, K, prec)
    q, k, v = to_device(Q, prec), to_device(K, prec), to_device(V, prec)
    o = torch.empty((B, H, R, D), dtype=torch.float32, device=DEV)
    l = torch.empty((B, H, R), dtype=torch.float16, device=DEV)
    st = torch.cuda.Stream()
    mha = mfa.MultiHeadAttention()
    torch.cuda.synchronize()

    def run():
        mha.forward(desc, q, k, v, o, l, stream=st.cuda_stream)

    with torch.cuda.stream(st):
        mfa.last_launches()
        run()
        st.synchronize()
        names = [r["name"] for r in mfa.last_launches()]
        assert names == ["mfa_fwd_decode16_kernel<F16, 128, 0>", "mfa_decode_merge_kernel"], names
        ref_o, ref_l = o.clone(), l.clone()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            run()
        for phase in ("eager", "replay", "eager again"):
            o.fill_(float("nan"))
            l.fill_(float("nan"))
            if phase == "replay":
                graph.replay()
            else:
                run()
            st.synchronize()
            assert torch.equal(o, ref_o) and torch.equal(l, ref_l), phase
