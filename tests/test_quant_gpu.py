"""GPU parity for the INT8/INT4 path: runtime quantiser (bit-exact vs GEMMQuantization.swift's
arithmetic), quantized forward/backward (QuantizedAttentionTest gates: INT8 relErr < 0.25,
FP16 < 0.05, blockwise INT8 < 0.15; QuantizedAttentionTest.swift:441-791) and the
dequant-exact property: with per-tensor scales the kernel's result equals attention on the
dequantised K/V up to fp32 rounding."""
import os

import numpy as np
import pytest
import torch

import mfa_amd as mfa
import oracle_lib as ol
from harness import (assert_gradients_within_gate, gradient_gate, maxerr, relerr, seen,
                     to_device)

pytestmark = pytest.mark.gpu
P = mfa.Precision
DEV = "cuda:0"


def tdev(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV).to(dtype)


# ----------------------------------------------------------------------- quantiser
@pytest.mark.parametrize("target", [P.INT8, P.INT4])
@pytest.mark.parametrize("src", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("shape", [(37, 19), (64, 128), (5, 1)])
def test_runtime_quantize_tensorwise_bitexact(gpu, target, src, shape):
    x = (np.random.default_rng(shape[0]).standard_normal(shape) * 3).astype(np.float32)
    xt = tdev(x, src)
    xs = xt.float().cpu().numpy()  # values after storage in `src`
    data, scale, _, _ = mfa.quantize(xt, target, rows=shape[0], cols=shape[1])
    torch.cuda.synchronize()
    s_ref = ol.quant_scale_tensor(xs, int(target))
    assert scale.item() == np.float32(s_ref)
    q_ref = ol.quantize(xs, int(target), s_ref)
    assert np.array_equal(data.cpu().numpy(), q_ref)


@pytest.mark.parametrize("target", [P.INT8, P.INT4])
@pytest.mark.parametrize("rows,cols,bs", [(16, 32, 8), (33, 20, 8), (128, 128, 64)])
def test_runtime_quantize_blockwise_bitexact(gpu, target, rows, cols, bs):
    rng = np.random.default_rng(rows + cols)
    x = (rng.standard_normal((rows, cols)) * rng.random((rows, 1)) * 5).astype(np.float32)
    data, _, bsc, bzp = mfa.quantize(tdev(x), target, mfa.QuantMode.blockwise, rows, cols, bs)
    torch.cuda.synchronize()
    s_ref = ol.quant_scales_block(x, rows, cols, bs, int(target))
    assert np.array_equal(bsc.cpu().numpy(), s_ref)
    assert not bzp.cpu().numpy().any()
    assert np.array_equal(data.cpu().numpy(), ol.quantize_block(x, cols, bs, int(target), s_ref))


def test_runtime_quantize_rowwise_scales(gpu):
    x = np.random.default_rng(7).standard_normal((12, 33)).astype(np.float32)
    data, _, sc, _ = mfa.quantize(tdev(x), P.INT8, mfa.QuantMode.rowWise, 12, 33)
    torch.cuda.synchronize()
    s_ref = ol.quant_scales_row(x, 12, 33, int(P.INT8))
    assert np.array_equal(sc.cpu().numpy(), s_ref)
    q = data.cpu().numpy().view(np.int8).reshape(12, 33)
    for r in range(12):
        assert np.array_equal(q[r], ol.quantize(x[r], int(P.INT8), s_ref[r]).view(np.int8))


def test_runtime_quantize_tensorwise_partials_not_stale(gpu):
    # The tensor-wise vector path leaves one absmax partial per workgroup in the workspace and
    # the quantise kernel reduces them: a large-magnitude tensor, then smaller tensors (fewer
    # workgroups, smaller maxima) on recycled workspace memory must each get their own scale.
    sizes = [(1 << 22, 40.0), (1 << 16, 0.5), (1 << 20, 3.0), (4096, 0.01)]
    for i, (n, amp) in enumerate(sizes):
        x = (np.random.default_rng(20 + i).standard_normal(n) * amp).astype(np.float32)
        data, scale, _, _ = mfa.quantize(torch.from_numpy(x).cuda(), P.INT8)
        torch.cuda.synchronize()
        s_ref = ol.quant_scale_tensor(x, int(P.INT8))
        assert scale.item() == np.float32(s_ref), (n, amp)
        assert np.array_equal(data.cpu().numpy(), ol.quantize(x, int(P.INT8), s_ref))


@pytest.mark.parametrize("target", [P.INT8, P.INT4])
@pytest.mark.parametrize("src", [torch.float32, torch.bfloat16])
def test_runtime_quantize_large_vector_paths(gpu, target, src):
    # 2049 x 1024 elements: the 8-wide kernels with several grid-stride steps per thread, and
    # a misaligned view (offset by one element) through the scalar kernels.
    rows, cols = 2049, 1024
    x = (np.random.default_rng(5).standard_normal((rows, cols)) * 2).astype(np.float32)
    xt = tdev(x, src)
    xs = xt.float().cpu().numpy()
    data, scale, _, _ = mfa.quantize(xt, target, rows=rows, cols=cols)
    torch.cuda.synchronize()
    s_ref = ol.quant_scale_tensor(xs, int(target))
    assert scale.item() == np.float32(s_ref)
    assert np.array_equal(data.cpu().numpy(), ol.quantize(xs, int(target), s_ref))
    flat = xt.reshape(-1)[1:]
    data1, scale1, _, _ = mfa.quantize(flat, target, rows=1, cols=flat.numel())
    torch.cuda.synchronize()
    s1 = ol.quant_scale_tensor(xs.reshape(-1)[1:], int(target))
    assert scale1.item() == np.float32(s1)
    assert np.array_equal(data1.cpu().numpy(), ol.quantize(xs.reshape(-1)[1:], int(target), s1))
    # Row-wise and block-wise on the same data (cols % 8 == 0: vector kernels).
    _, _, rsc, _ = mfa.quantize(xt, target, mfa.QuantMode.rowWise, rows, cols)
    dat_b, _, bsc, _ = mfa.quantize(xt, target, mfa.QuantMode.blockwise, rows, cols, 64)
    torch.cuda.synchronize()
    assert np.array_equal(rsc.cpu().numpy(), ol.quant_scales_row(xs, rows, cols, int(target)))
    b_ref = ol.quant_scales_block(xs, rows, cols, 64, int(target))
    assert np.array_equal(bsc.cpu().numpy(), b_ref)
    assert np.array_equal(dat_b.cpu().numpy(), ol.quantize_block(xs, cols, 64, int(target), b_ref))
    # Row-wise with 128-element rows (C3's head dim): 4 rows per wave.
    x128 = xt.reshape(-1, 128)
    dat_r, _, rsc2, _ = mfa.quantize(x128, target, mfa.QuantMode.rowWise, x128.shape[0], 128)
    torch.cuda.synchronize()
    r_ref = ol.quant_scales_row(xs.reshape(-1, 128), x128.shape[0], 128, int(target))
    assert np.array_equal(rsc2.cpu().numpy(), r_ref)
    if target == P.INT8:
        q = dat_r.cpu().numpy().view(np.int8).reshape(-1, 128)
        for r in (0, 1, 777, x128.shape[0] - 1):
            assert np.array_equal(q[r], ol.quantize(xs.reshape(-1, 128)[r], int(target), r_ref[r]).view(np.int8))


@pytest.mark.parametrize("target", [P.INT8, P.INT4])
def test_dequantize_bitexact(gpu, target):
    x = np.random.default_rng(11).standard_normal(1001).astype(np.float32)
    s = ol.quant_scale_tensor(x, int(target))
    q = ol.quantize(x, int(target), s)
    t = mfa.quantized_tensor(tdev(q, torch.uint8), target, scale=s)
    out = torch.empty(1001, dtype=torch.float32, device=DEV)
    mfa.check(mfa.lib.mfa_dequantize(mfa.ctypes.byref(t), 1001, 1001, out.data_ptr(), None))
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), ol.dequantize(q, 1001, int(target), s))


# ----------------------------------------------------------------------- forward
def quantize_host(x, prec):
    s = ol.quant_scale_tensor(x, int(prec))
    q = ol.quantize(x, int(prec), s)
    return q, s, ol.dequantize(q, x.size, int(prec), s).reshape(x.shape)


def run_qforward(Qn, Kn, Vn, qp, kp, vp, causal=False, lpi=True, blockwise=None,
                 integer_matmul=False, window=None):
    B, H, R, D = Qn.shape
    Hkv, C = Kn.shape[1], Kn.shape[2]
    base = mfa.AttentionDescriptor.make(R, C, D, causal=causal, low_precision_intermediates=lpi,
                                        window=window)
    desc = mfa.quantized_descriptor(base, qp, kp, vp, B=B, H=H, Hkv=Hkv,
                                    integer_matmul=integer_matmul)
    deq = {}

    def make(x, prec, name):
        if prec in (P.FP16, P.BF16, P.FP32):
            xd = seen(x, prec)
            deq[name] = xd
            return mfa.quantized_tensor(to_device(x, prec), prec), None
        if blockwise:
            rows, cols = x.size // x.shape[-1], x.shape[-1]
            sc = ol.quant_scales_block(x, rows, cols, blockwise, int(prec))
            q = ol.quantize_block(x, cols, blockwise, int(prec), sc)
            deq[name] = ol.dequantize_block(q, x.size, cols, blockwise, int(prec), sc).reshape(x.shape)
            scd = tdev(sc)
            return mfa.quantized_tensor(tdev(q, torch.uint8), prec, block_scales=scd,
                                        block_size=blockwise), scd
        q, s, d = quantize_host(x, prec)
        deq[name] = d
        return mfa.quantized_tensor(tdev(q, torch.uint8), prec, scale=s), None

    tq, kq_keep = make(Qn, qp, "Q")
    tk, kk_keep = make(Kn, kp, "K")
    tv, kv_keep = make(Vn, vp, "V")
    o = torch.full((B, H, R, D), float("nan"), dtype=torch.float32, device=DEV)
    l = torch.empty((B, H, R), dtype=torch.float16 if lpi else torch.float32, device=DEV)
    mfa.QuantizedAttention().forward(desc, tq, tk, tv, o, l)
    torch.cuda.synchronize()
    return o, l, deq, (kq_keep, kk_keep, kv_keep)


@pytest.mark.parametrize("prec,gate", [(P.FP16, 0.05), (P.INT8, 0.25)])
def test_quantized_forward_correctness_gate(gpu, prec, gate):
    # QuantizedAttentionTest.testQuantizedForwardCorrectness: S32 D16, LCG 0x5EED5EED.
    S, D = 32, 16
    g = ol.LCGStream(0x5EED5EED)
    Q, K, V = (g.draw(S * D).reshape(1, 1, S, D) for _ in range(3))
    o, _, deq, _ = run_qforward(Q, K, V, prec, prec, prec, lpi=False)
    ref = ol.attention(Q, K, V)["O"]
    assert np.isfinite(o.cpu().numpy()).all()
    assert relerr(o, ref) < gate
    exact = ol.attention(deq["Q"], deq["K"], deq["V"])["O"]
    assert maxerr(o, exact) < 5e-3  # dequant-exact: same math on the stored values


@pytest.mark.parametrize("kv", [P.INT8, P.INT4])
@pytest.mark.parametrize("causal", [False, True])
def test_quantized_forward_dequant_exact(gpu, kv, causal):
    B, H, S, D = 2, 4, 200, 128
    rng = np.random.default_rng(3)
    Q, K, V = (rng.standard_normal((B, H, S, D)).astype(np.float32) for _ in range(3))
    o, l, deq, _ = run_qforward(Q, K, V, P.FP16, kv, kv, causal=causal)
    ref = ol.attention(deq["Q"], deq["K"], deq["V"], causal=causal)
    assert maxerr(o, ref["O"]) < 2e-2
    assert maxerr(l, ref["L"]) < 1e-2
    if kv == P.INT8:
        assert relerr(o, ol.attention(Q, K, V, causal=causal)["O"]) < 0.25


def test_blockwise_attention_forward_gate(gpu):
    # QuantizedAttentionTest.testBlockwiseAttentionForward: S32 D32 bs8, gate 0.15.
    S, D, bs = 32, 32, 8
    i = np.arange(S * D)
    br, bc = (i // D) // bs, (i % D) // bs
    Q = ((i % 11).astype(np.float32) * np.float32(0.05) - np.float32(0.25)).reshape(1, 1, S, D)
    K = (((i % 7).astype(np.float32) - 3) * ((br + 1) * (bc + 1)).astype(np.float32) * np.float32(0.1)).reshape(1, 1, S, D)
    V = (((i % 5).astype(np.float32) - 2) * ((br + 1) * (bc + 1)).astype(np.float32) * np.float32(0.1)).reshape(1, 1, S, D)
    o, _, deq, _ = run_qforward(Q, K, V, P.FP16, P.INT8, P.INT8, lpi=False, blockwise=bs)
    assert relerr(o, ol.attention(Q, K, V)["O"]) < 0.15
    assert maxerr(o, ol.attention(deq["Q"], deq["K"], deq["V"])["O"]) < 2e-3


def test_int8_query_and_gqa(gpu):
    B, H, Hkv, S, D = 1, 8, 2, 96, 64
    rng = np.random.default_rng(4)
    Q = rng.standard_normal((B, H, S, D)).astype(np.float32)
    K, V = (rng.standard_normal((B, Hkv, S, D)).astype(np.float32) for _ in range(2))
    o, _, deq, _ = run_qforward(Q, K, V, P.INT8, P.INT8, P.INT8)
    assert maxerr(o, ol.attention(deq["Q"], deq["K"], deq["V"])["O"]) < 2e-2


C3_HEADS = (0, 7, 15)  # first, middle and last head: every XCD-order / pair position class


def test_c3_shape_heads(gpu):
    # BASELINE.json configs[2]: INT8 K/V, H16 S8192 D128; oracle on heads 0, 7 and 15.
    B, H, S, D = 1, 16, 8192, 128
    n = B * H * S * D
    Q = ol.lcg(11, n).reshape(B, H, S, D)
    K = ol.lcg(22, n).reshape(B, H, S, D)
    V = ol.lcg(33, n).reshape(B, H, S, D)
    o, l, deq, _ = run_qforward(Q, K, V, P.FP16, P.INT8, P.INT8)
    on, ln = o.cpu().numpy(), l.float().cpu().numpy()
    assert np.isfinite(on).all() and np.abs(on).max() <= np.abs(deq["V"]).max() * 1.01
    for h in C3_HEADS:
        ref = ol.attention(deq["Q"][:, h:h + 1], deq["K"][:, h:h + 1], deq["V"][:, h:h + 1])
        assert maxerr(on[:, h:h + 1], ref["O"]) < 2e-3, h
        assert maxerr(ln[:, h:h + 1], ref["L"]) < 7e-3 + 2 ** -11 * np.abs(ref["L"]).max(), h


def test_dequant_pass_small_scales(gpu, monkeypatch):
    """Per-tensor INT8 Q and K with small scales: the folded softmax multiplier
    c = log2e·scale·s_q·s_k is then ~1e-9, and the fp16 forward pre-scales the integer Q copy
    by it, so Q·c lands in (or under) the fp16 subnormal range.  Softmax needs S' = S·c only to
    an absolute accuracy, which subnormal rounding keeps (|error| <= 2^-25 per product term);
    held to the direct dequantise-on-load path (c applied in fp32) and the oracle."""
    B, H, S, D = 1, 2, 256, 128
    rng = np.random.default_rng(31)
    for amp_q, amp_k in ((1e-3, 1e-3), (0.3, 2e-4), (30.0, 1e-2)):
        Q = (rng.standard_normal((B, H, S, D)) * amp_q).astype(np.float32)
        K = (rng.standard_normal((B, H, S, D)) * amp_k).astype(np.float32)
        V = rng.standard_normal((B, H, S, D)).astype(np.float32)
        o1, l1, deq, _ = run_qforward(Q, K, V, P.INT8, P.INT8, P.INT8)
        monkeypatch.setenv("MFA_NO_DEQUANT_PASS", "1")
        o2, l2, _, _ = run_qforward(Q, K, V, P.INT8, P.INT8, P.INT8)
        monkeypatch.delenv("MFA_NO_DEQUANT_PASS")
        ref = ol.attention(deq["Q"], deq["K"], deq["V"])
        assert maxerr(o1, o2.cpu().numpy()) < 2e-3, (amp_q, amp_k)
        assert maxerr(o1, ref["O"]) < 2e-3, (amp_q, amp_k)
        assert maxerr(l1, ref["L"]) < 1e-2, (amp_q, amp_k)


# ----------------------------------------------------------------------- backward
@pytest.mark.parametrize("prec,gate", [(P.FP16, 0.05), (P.INT8, 0.25)])
def test_quantized_backward_correctness_gate(gpu, prec, gate):
    # QuantizedAttentionTest.testQuantizedBackwardCorrectness: S32 D16, LCG 0xBACC0DE; O and
    # L (x log2 e) from the CPU reference; dO FP32; gates on dQ/dK/dV relative error.
    S, D = 32, 16
    g = ol.LCGStream(0xBACC0DE)
    Q, K, V = (g.draw(S * D).reshape(1, 1, S, D) for _ in range(3))
    dO = g.draw(S * D, 0.2, -0.1).reshape(1, 1, S, D)
    ref = ol.attention(Q, K, V, dO=dO)
    base = mfa.AttentionDescriptor.make(S, S, D)
    desc = mfa.quantized_descriptor(base, prec, prec, prec)
    keep = []

    def make(x):
        if prec == P.FP16:
            return mfa.quantized_tensor(to_device(x, P.FP16), P.FP16)
        q, s, _ = quantize_host(x, prec)
        t = tdev(q, torch.uint8)
        keep.append(t)
        return mfa.quantized_tensor(t, prec, scale=s)

    tq, tk, tv = make(Q), make(K), make(V)
    o = tdev(ref["O"])
    l = tdev(ref["L"])  # GPU convention (log2 units)
    do = tdev(dO)
    dq = torch.empty((1, 1, S, D), dtype=torch.float32, device=DEV)
    dk, dv = torch.empty_like(dq), torch.empty_like(dq)
    dvals = torch.empty((1, 1, S), dtype=torch.float32, device=DEV)
    qa = mfa.QuantizedAttention()
    qa.backwardQuery(desc, tq, tk, tv, o, do, l, dq, dvals)
    qa.backwardKeyValue(desc, tq, tk, tv, do, l, dvals, dk, dv)
    torch.cuda.synchronize()
    for name, t in (("dQ", dq), ("dK", dk), ("dV", dv)):
        assert np.isfinite(t.cpu().numpy()).all()
        assert relerr(t, ref[name]) < gate, name


def test_quantized_backward_dequant_exact(gpu):
    B, H, S, D = 1, 2, 130, 64
    rng = np.random.default_rng(8)
    Q, K, V, dO = (rng.standard_normal((B, H, S, D)).astype(np.float32) for _ in range(4))
    kq, ks, kd = quantize_host(K, P.INT8)
    vq, vs, vd = quantize_host(V, P.INT8)
    Qd = seen(Q, P.FP16)
    ref = ol.attention(Qd, kd, vd, dO=dO, causal=True)
    base = mfa.AttentionDescriptor.make(S, S, D, causal=True)
    desc = mfa.quantized_descriptor(base, P.FP16, P.INT8, P.INT8, B=B, H=H)
    kt, vt = tdev(kq, torch.uint8), tdev(vq, torch.uint8)
    tq = mfa.quantized_tensor(to_device(Q, P.FP16), P.FP16)
    tk = mfa.quantized_tensor(kt, P.INT8, scale=ks)
    tv = mfa.quantized_tensor(vt, P.INT8, scale=vs)
    o, l = tdev(ref["O"]), tdev(ref["L"])
    do = tdev(dO)
    dq = torch.empty((B, H, S, D), dtype=torch.float32, device=DEV)
    dk, dv = torch.empty_like(dq), torch.empty_like(dq)
    dvals = torch.empty((B, H, S), dtype=torch.float32, device=DEV)
    qa = mfa.QuantizedAttention()
    qa.backwardQuery(desc, tq, tk, tv, o, do, l, dq, dvals)
    qa.backwardKeyValue(desc, tq, tk, tv, do, l, dvals, dk, dv)
    torch.cuda.synchronize()
    assert maxerr(dvals, ref["D"]) < 1e-4
    for name, t in (("dQ", dq), ("dK", dk), ("dV", dv)):
        assert maxerr(t, ref[name]) < 5e-2, name
    # The relative gate on the dequantised K/V as exact inputs.  L and D are FP32 here: the
    # emulation rounds only P and dS, to the FP16 operand type, and dO, which is FP32 in
    # memory here, where it becomes the FP16 operand of dP and dV (D keeps the FP32 values).
    gate = gradient_gate(Qd, kd, vd, dO, P.FP16, ref, causal=True,
                         low_precision_intermediates=False, round_dO=True)
    assert_gradients_within_gate({"dQ": dq, "dK": dk, "dV": dv}, ref, gate, report="dequant")


# ----------------------------------------------------------------------- dequantisation pass
# Shapes with >= 128 query rows per kv head dequantise K/V (and a quantised Q) once into dense
# 16-bit copies (kv_dequant.hip) and run the tuned 16-bit kernels; the copies hold exactly the
# operands dequantise-on-load staging produces, so the result matches the direct path up to
# the two kernels' summation orders.
def test_dequant_pass_matches_direct_path(gpu, monkeypatch):
    B, H, S, D = 1, 4, 256, 128
    rng = np.random.default_rng(21)
    Q, K, V = (rng.standard_normal((B, H, S, D)).astype(np.float32) for _ in range(3))
    for kv in (P.INT8, P.INT4):
        o1, l1, deq, _ = run_qforward(Q, K, V, P.FP16, kv, kv, causal=True)
        monkeypatch.setenv("MFA_NO_DEQUANT_PASS", "1")
        o2, l2, _, _ = run_qforward(Q, K, V, P.FP16, kv, kv, causal=True)
        monkeypatch.delenv("MFA_NO_DEQUANT_PASS")
        assert maxerr(o1, o2.cpu().numpy()) < 2e-3
        ref = ol.attention(deq["Q"], deq["K"], deq["V"], causal=True)
        assert maxerr(o1, ref["O"]) < 2e-2 and maxerr(l1, ref["L"]) < 1e-2


def test_dequant_pass_blockwise_and_quantized_query(gpu):
    B, H, S, D, bs = 1, 2, 256, 64, 16
    rng = np.random.default_rng(22)
    Q, K, V = (rng.standard_normal((B, H, S, D)).astype(np.float32) for _ in range(3))
    o, l, deq, _ = run_qforward(Q, K, V, P.INT8, P.INT8, P.INT8, blockwise=bs)
    ref = ol.attention(deq["Q"], deq["K"], deq["V"])
    assert maxerr(o, ref["O"]) < 2e-2 and maxerr(l, ref["L"]) < 1e-2


@pytest.mark.parametrize("kv", [P.INT8, P.INT4])
@pytest.mark.parametrize("D,zps,S", [(128, (0, 0), 300), (64, (3, -1), 300), (256, (-2, 5), 300),
                                     (128, (4, 2), 100)])
def test_quantized_backward_on_fast_kernels(gpu, kv, D, zps, S, monkeypatch):
    """Low-precision descriptor (FP16 Q and dO), per-tensor quantised K/V, causal: both phases
    run the tuned kernels on the stored bytes — backwardQuery through its LDS byte ring
    (forced with MFA_BWDQ_BYTES=1 at S = 300, the default below 128 query rows per kv head),
    backwardKeyValue in registers — with no dequantisation pass (plan checked), match the
    oracle on the dequantised values, and (S = 300) give dQ bit for bit as the pass + 16-bit
    kernel path (the default there: the same kernel on the dense copy, the same MFMA
    operands)."""
    _quantized_backward_fast(kv, D, zps, S, monkeypatch)


@pytest.mark.parametrize("kv", [P.INT8, P.INT4])
@pytest.mark.parametrize("D,H,Hkv,S,window", [(128, 8, 2, 100, None), (64, 4, 1, 60, None),
                                               (128, 2, 2, 300, 96), (256, 8, 2, 40, 24),
                                               (64, 6, 3, 200, 50)])
def test_quantized_backward_bytes_gqa_window(gpu, kv, D, H, Hkv, S, window, monkeypatch):
    """the byte-ring backwardQuery with GQA / MQA head mapping (kv head = h % Hkv
    of the group) and sliding windows (in place of the causal pattern), held to the oracle and (at >= 128 query rows per
    kv head, where the pass is the default) bit for bit to the pass path."""
    _quantized_backward_fast(kv, D, (2, -3), S, monkeypatch, H=H, Hkv=Hkv, window=window)


def _quantized_backward_fast(kv, D, zps, S, monkeypatch, H=2, Hkv=2, window=None):
    B = 1
    rows_per_kv = (H // Hkv) * S
    if rows_per_kv >= 128:
        monkeypatch.setenv("MFA_BWDQ_BYTES", "1")
    rng = np.random.default_rng(23 + D + 7 * H + Hkv + S)
    Q, dO = (rng.standard_normal((B, H, S, D)).astype(np.float32) * 0.5 for _ in range(2))
    lim = 120 if kv == P.INT8 else 8
    kq8 = rng.integers(-lim, lim, (B, Hkv, S, D)).astype(np.int8)
    vq8 = rng.integers(-lim, lim, (B, Hkv, S, D)).astype(np.int8)
    ks, vs = 0.004 if kv == P.INT8 else 0.06, 0.005 if kv == P.INT8 else 0.07
    kd = ((kq8.astype(np.float32) - zps[0]) * np.float32(ks)).astype(np.float32)
    vd = ((vq8.astype(np.float32) - zps[1]) * np.float32(vs)).astype(np.float32)
    if kv == P.INT8:
        kt, vt = tdev(kq8.view(np.uint8), torch.uint8), tdev(vq8.view(np.uint8), torch.uint8)
    else:  # nibble n encodes n - 8, element 2i in the low nibble (GEMMQuantization.swift:500-515)
        pack = lambda x: ((x[..., 0::2] + 8) | ((x[..., 1::2] + 8) << 4)).astype(np.uint8)
        kt, vt = tdev(pack(kq8.astype(np.int32)), torch.uint8), tdev(pack(vq8.astype(np.int32)), torch.uint8)
    Qd, dOd = seen(Q, P.FP16), seen(dO, P.FP16)
    # (A sliding window replaces the causal pattern: AttentionDescriptor.sparsityPattern holds one.)
    ref = ol.attention(Qd, kd, vd, dO=dOd, causal=window is None, window=window)
    base = mfa.AttentionDescriptor.make(S, S, D, causal=True, window=window, low_precision=True,
                                        precision=P.FP16)
    desc = mfa.quantized_descriptor(base, P.FP16, kv, kv, B=B, H=H, Hkv=Hkv)
    tq = mfa.quantized_tensor(to_device(Q, P.FP16), P.FP16)
    tk = mfa.quantized_tensor(kt, kv, scale=ks, zero_point=zps[0])
    tv = mfa.quantized_tensor(vt, kv, scale=vs, zero_point=zps[1])
    o = tdev(ref["O"])
    l = torch.from_numpy(ref["L"]).half().to(DEV)
    do = to_device(dO, P.FP16)
    qa = mfa.QuantizedAttention()
    src = 1 if kv == P.INT8 else 2

    def run():
        dq = torch.full((B, H, S, D), float("nan"), dtype=torch.float32, device=DEV)
        dk = torch.empty((B, Hkv, S, D), dtype=torch.float32, device=DEV)
        dv = torch.empty_like(dk)
        dvals = torch.empty((B, H, S), dtype=torch.bfloat16, device=DEV)
        plan = (mfa.quantized_plan(desc, mfa.KernelType.backwardQuery, tq, tk, tv) +
                mfa.quantized_plan(desc, mfa.KernelType.backwardKeyValue, tq, tk, tv))
        mfa.last_launches()
        qa.backwardQuery(desc, tq, tk, tv, o, do, l, dq, dvals)
        qa.backwardKeyValue(desc, tq, tk, tv, do, l, dvals, dk, dv)
        torch.cuda.synchronize()
        assert mfa.last_launches() == plan[-4:]  # the log keeps the last four launches
        return [r["name"] for r in plan], dq, dk, dv, dvals

    names, dq, dk, dv, dvals = run()
    assert names == [f"mfa_bwd_q_fast_kernel<F16, {D}, {32 if D == 256 else 64}, false, {src}>",
                     f"mfa_bwd_kv_fast_kernel<F16, {D}, {32 if D == 256 else 64}, {src}, false>"], names
    for name, t in (("dQ", dq), ("dK", dk), ("dV", dv)):
        assert maxerr(t, ref[name]) < 5e-2 * max(1.0, np.abs(ref[name]).max()), name
    # The relative gate on the dequantised K/V as exact inputs (L is FP16, D is BF16).
    gate = gradient_gate(Qd, kd, vd, dOd, P.FP16, ref, causal=window is None, window=window)
    assert_gradients_within_gate({"dQ": dq, "dK": dk, "dV": dv}, ref, gate,
                                 report=f"{kv.name} D={D} S={S} H={H}/{Hkv}")
    if rows_per_kv < 128:
        return
    monkeypatch.delenv("MFA_BWDQ_BYTES")
    names2, dq2, _, _, dvals2 = run()
    assert names2[:2] == [f"mfa_kv_dequant_kernel<F16, {src}>"] * 2, names2
    assert names2[2] == f"mfa_bwd_q_fast_kernel<F16, {D}, {32 if D == 256 else 64}, false, 0>", names2
    assert torch.equal(dq, dq2) and torch.equal(dvals, dvals2)


# ----------------------------------------------------------------------- integer matmul
# The INT8-MFMA forward (attention_fwd_i8.hip) quantises Q per row and P to INT8 (P' =
# round(127 P) against a max rounded up to an integer, so 6-7 bits), so it is not
# dequant-exact.  Its tolerance, written here: relative L2 error vs attention on the
# dequantised K/V (same stored values, float math) < 5e-2 (measured 1.3e-2 .. 3.3e-2 on the
# cases below; the largest for many keys with small, spread-out P), max |L| error < 5e-2,
# and the reference's own INT8 gate (relErr < 0.25 vs the unquantised inputs,
# QuantizedAttentionTest.swift:519-520).
I8MM_REL, I8MM_L = 5e-2, 5e-2


@pytest.mark.parametrize("B,H,Hkv,R,C,D,causal,window,qp", [
    (2, 4, 4, 200, 200, 128, False, None, P.FP16),
    (2, 4, 4, 200, 200, 128, True, None, P.FP16),
    (1, 2, 2, 333, 333, 64, False, 40, P.FP16),
    (1, 4, 2, 257, 129, 96, False, None, P.BF16),
    (1, 2, 2, 512, 512, 128, False, 100, P.BF16),
    (1, 1, 1, 1, 77, 16, False, None, P.FP16),
    (1, 3, 1, 130, 1000, 128, False, None, P.FP16),
])
def test_integer_matmul_forward(gpu, B, H, Hkv, R, C, D, causal, window, qp):
    rng = np.random.default_rng(R * 7 + C)
    Q = rng.standard_normal((B, H, R, D)).astype(np.float32)
    K, V = (rng.standard_normal((B, Hkv, C, D)).astype(np.float32) for _ in range(2))
    o, l, deq, _ = run_qforward(Q, K, V, qp, P.INT8, P.INT8, causal=causal,
                                integer_matmul=True, window=window)
    on = o.cpu().numpy()
    assert np.isfinite(on).all()
    ref = ol.attention(deq["Q"], deq["K"], deq["V"], causal=causal, window=window)
    print(f"integer-matmul relL2 vs dequant-exact {relerr(o, ref['O']):.3e}, "
          f"max|dL| {maxerr(l, ref['L']):.3e}")
    assert relerr(o, ref["O"]) < I8MM_REL
    assert maxerr(l, ref["L"]) < I8MM_L
    assert relerr(o, ol.attention(Q, K, V, causal=causal, window=window)["O"]) < 0.25


@pytest.mark.parametrize("B,H,Hkv,R,C,D,qp", [
    (2, 4, 4, 200, 200, 128, P.FP16),   # odd block count: group 1 of the last pair has no rows
    (1, 4, 2, 257, 129, 96, P.BF16),
    (1, 3, 1, 384, 1000, 128, P.FP16),
])
def test_integer_matmul_shared_tiles_forced(gpu, B, H, Hkv, R, C, D, qp):
    # Two 4-wave groups on adjacent blocks sharing every staged tile (the default for unmasked
    # C3-sized problems), forced at small sizes; same gates as above.
    rng = np.random.default_rng(R * 5 + C)
    Q = rng.standard_normal((B, H, R, D)).astype(np.float32)
    K, V = (rng.standard_normal((B, Hkv, C, D)).astype(np.float32) for _ in range(2))
    os.environ["MFA_I8_SHARE"] = "1"
    try:
        o, l, deq, _ = run_qforward(Q, K, V, qp, P.INT8, P.INT8, integer_matmul=True)
    finally:
        os.environ.pop("MFA_I8_SHARE", None)
    ref = ol.attention(deq["Q"], deq["K"], deq["V"])
    assert np.isfinite(o.cpu().numpy()).all()
    assert relerr(o, ref["O"]) < I8MM_REL
    assert maxerr(l, ref["L"]) < I8MM_L


def test_integer_matmul_ineligible_falls_back_exact(gpu):
    # INT4 K/V (no integer-MFMA kernel) with integer_matmul set runs the dequant-exact path.
    rng = np.random.default_rng(9)
    Q, K, V = (rng.standard_normal((1, 2, 64, 64)).astype(np.float32) for _ in range(3))
    o, _, deq, _ = run_qforward(Q, K, V, P.FP16, P.INT4, P.INT4, integer_matmul=True)
    assert maxerr(o, ol.attention(deq["Q"], deq["K"], deq["V"])["O"]) < 2e-2


def test_integer_matmul_c3_heads(gpu):
    B, H, S, D = 1, 16, 8192, 128
    n = B * H * S * D
    Q = ol.lcg(11, n).reshape(B, H, S, D)
    K = ol.lcg(22, n).reshape(B, H, S, D)
    V = ol.lcg(33, n).reshape(B, H, S, D)
    o, l, deq, _ = run_qforward(Q, K, V, P.FP16, P.INT8, P.INT8, integer_matmul=True)
    on, ln = o.cpu().numpy(), l.float().cpu().numpy()
    assert np.isfinite(on).all()
    for h in C3_HEADS:
        ref = ol.attention(deq["Q"][:, h:h + 1], deq["K"][:, h:h + 1], deq["V"][:, h:h + 1])
        assert relerr(on[:, h:h + 1], ref["O"]) < I8MM_REL, h
        assert maxerr(ln[:, h:h + 1], ref["L"]) < I8MM_L, h


# ----------------------------------------------------------------------- split-KV decode
# Few query rows per kv head (R·H/H_kv < 128) with per-tensor INT8 K/V run the split-KV decode
# kernel (attention_decode.hip): the INT8 bytes are staged by LDS-DMA and widened in registers
# (dequant-exact); the partials of every wave are merged in LDS by the workgroup when a unit
# has one key split, by a second pass otherwise.  Held to the oracle on the
# dequantised values at the dequant-exact tolerance, and to the previous (generic) path.
@pytest.mark.parametrize("B,H,Hkv,R,C,D,qp", [
    (2, 4, 4, 1, 1000, 128, P.FP16),
    (1, 4, 4, 16, 4101, 128, P.FP16),
    (1, 8, 2, 3, 777, 64, P.BF16),     # GQA: 12 rows per kv head
    (2, 4, 1, 5, 300, 256, P.FP16),    # MQA: 20 rows, D 256
    (1, 16, 1, 4, 2048, 128, P.BF16),  # 64 rows per kv head: two row tiles
    (1, 16, 1, 4, 300, 128, P.FP16),   # two row tiles, one split: in-workgroup merge
    (1, 2, 2, 1, 33, 64, P.FP16),      # one partial tile
    (1, 4, 4, 7, 70, 96, P.BF16),      # D 96 in the 128-wide tiles
    (2, 4, 2, 8, 2500, 128, P.FP16),   # GQA, 16 rows, split path
    (1, 4, 4, 2, 3000, 256, P.BF16),   # D 256 on the 16-row kernel (INT8)
    (2, 8, 2, 4, 1500, 256, P.FP16),   # D 256, GQA 16 rows
    (1, 4, 4, 1, 12000, 64, P.FP16),   # 23 splits: the one-wave merge pass
    (1, 2, 2, 1, 24000, 64, P.FP16),   # 38 splits (> 32 partials per row): the 4-wave merge
])
def test_decode_split_kv(gpu, B, H, Hkv, R, C, D, qp, monkeypatch):
    rng = np.random.default_rng(R * 13 + C)
    Q = rng.standard_normal((B, H, R, D)).astype(np.float32)
    K, V = (rng.standard_normal((B, Hkv, C, D)).astype(np.float32) for _ in range(2))
    base = mfa.AttentionDescriptor.make(R, C, D, low_precision=True, precision=qp)
    desc = mfa.quantized_descriptor(base, qp, P.INT8, P.INT8, B=B, H=H, Hkv=Hkv)
    names = [r["name"] for r in mfa.quantized_plan(desc)]
    d16 = (H // Hkv) * R <= 16
    assert names[0].startswith("mfa_fwd_decode16_kernel<" if d16 else "mfa_fwd_decode_kernel<"), names
    # One key split per unit: the workgroup merges its waves in LDS (one launch); more
    # splits take the merge pass.
    assert names[1:] in ([], ["mfa_decode_merge_kernel"], ["mfa_decode_merge4_kernel"]), names
    if C == 24000:
        assert names[1:] == ["mfa_decode_merge4_kernel"], names
    elif C == 12000:
        assert names[1:] == ["mfa_decode_merge_kernel"], names
    o, l, deq, _ = run_qforward(Q, K, V, qp, P.INT8, P.INT8)
    ref = ol.attention(deq["Q"], deq["K"], deq["V"])
    assert np.isfinite(o.cpu().numpy()).all()
    assert maxerr(o, ref["O"]) < 2e-3 * max(1.0, np.abs(ref["O"]).max())
    assert maxerr(l, ref["L"]) < 7e-3 + 2 ** -11 * np.abs(ref["L"]).max()
    monkeypatch.setenv("MFA_DECODE", "0")
    o2, _, _, _ = run_qforward(Q, K, V, qp, P.INT8, P.INT8)
    monkeypatch.delenv("MFA_DECODE")
    # Both paths sit within the oracle tolerance, so within twice it of each other.
    assert maxerr(o, o2.cpu().numpy()) < 4e-3 * max(1.0, np.abs(ref["O"]).max())
    if d16:  # the 16-row kernel against the 32-row one
        monkeypatch.setenv("MFA_DECODE16", "0")
        assert mfa.quantized_plan(desc)[0]["name"].startswith("mfa_fwd_decode_kernel<")
        o4, l4, _, _ = run_qforward(Q, K, V, qp, P.INT8, P.INT8)
        monkeypatch.delenv("MFA_DECODE16")
        assert maxerr(o, o4.cpu().numpy()) < 2e-3
        assert maxerr(l, l4.float().cpu().numpy()) < 7e-3
    if len(names) == 1:  # the in-workgroup merge equals the merge pass bit for bit
        monkeypatch.setenv("MFA_DECODE_MERGE", "1")
        assert [r["name"] for r in mfa.quantized_plan(desc)][1:] == ["mfa_decode_merge_kernel"]
        o3, l3, _, _ = run_qforward(Q, K, V, qp, P.INT8, P.INT8)
        monkeypatch.delenv("MFA_DECODE_MERGE")
        assert torch.equal(o, o3) and torch.equal(l, l3)


# Causal masks on the split-KV decode kernel (key <= query index, masked per lane; the host
# reads no key past R - 1): INT8 and INT4, FP16 / BF16 Q, GQA, against the oracle and the
# generic dequant-on-load kernel (MFA_DECODE=0).
@pytest.mark.parametrize("kv", [P.INT8, P.INT4])
@pytest.mark.parametrize("B,H,Hkv,R,C,D,qp", [
    (2, 4, 4, 16, 1000, 128, P.FP16),   # 16 rows: keys 0..15 at most
    (1, 8, 2, 3, 777, 64, P.BF16),      # GQA: 12 rows per kv head
    (1, 16, 1, 4, 300, 128, P.FP16),    # MQA, two row tiles
    (1, 2, 2, 100, 90, 256, P.BF16),    # C < R: every key seen by the last rows
])
def test_decode_causal(gpu, kv, B, H, Hkv, R, C, D, qp, monkeypatch):
    rng = np.random.default_rng(R * 31 + C)
    Q = rng.standard_normal((B, H, R, D)).astype(np.float32)
    K, V = (rng.standard_normal((B, Hkv, C, D)).astype(np.float32) for _ in range(2))
    base = mfa.AttentionDescriptor.make(R, C, D, causal=True, low_precision=True, precision=qp)
    desc = mfa.quantized_descriptor(base, qp, kv, kv, B=B, H=H, Hkv=Hkv)
    names = [r["name"] for r in mfa.quantized_plan(desc)]
    assert names[0].startswith("mfa_fwd_decode"), names
    o, l, deq, _ = run_qforward(Q, K, V, qp, kv, kv, causal=True)
    ref = ol.attention(deq["Q"], deq["K"], deq["V"], causal=True)
    assert np.isfinite(o.cpu().numpy()).all()
    assert maxerr(o, ref["O"]) < 2e-3 * max(1.0, np.abs(ref["O"]).max())
    assert maxerr(l, ref["L"]) < 7e-3 + 2 ** -11 * np.abs(ref["L"]).max()
    monkeypatch.setenv("MFA_DECODE", "0")
    o2, _, _, _ = run_qforward(Q, K, V, qp, kv, kv, causal=True)
    monkeypatch.delenv("MFA_DECODE")
    # The generic path's BF16 P (8 mantissa bits) is held at twice the FP16 tolerance.
    assert maxerr(o2, ref["O"]) < (2e-3 if qp == P.FP16 else 4e-3) * max(1.0, np.abs(ref["O"]).max())
    # Both paths sit within the oracle tolerance, so within twice it of each other.
    assert maxerr(o, o2.cpu().numpy()) < 4e-3 * max(1.0, np.abs(ref["O"]).max())


# Sliding-window masks (row > key + window masked) on the split-KV decode kernels, masked per
# lane; INT8 and INT4, both kernel forms, against the oracle and the generic path.
@pytest.mark.parametrize("kv", [P.INT8, P.INT4])
@pytest.mark.parametrize("B,H,Hkv,R,C,D,win,qp", [
    (1, 4, 4, 16, 1000, 128, 5, P.FP16),    # 16 rows: rows 6..15 lose their first keys
    (1, 8, 2, 3, 777, 64, 0, P.BF16),       # GQA, window 0: row r sees keys >= r
    (1, 16, 1, 4, 300, 128, 1, P.FP16),     # MQA, two row tiles (the 32-row kernel)
    (2, 2, 2, 40, 60, 256, 10, P.BF16),     # D 256 (the 32-row kernel)
    (1, 2, 2, 9, 500, 256, 3, P.FP16),      # D 256, 9 rows (INT8: the 16-row kernel)
])
def test_decode_window(gpu, kv, B, H, Hkv, R, C, D, win, qp, monkeypatch):
    rng = np.random.default_rng(R * 41 + C)
    Q = rng.standard_normal((B, H, R, D)).astype(np.float32)
    K, V = (rng.standard_normal((B, Hkv, C, D)).astype(np.float32) for _ in range(2))
    base = mfa.AttentionDescriptor.make(R, C, D, window=win, low_precision=True, precision=qp)
    desc = mfa.quantized_descriptor(base, qp, kv, kv, B=B, H=H, Hkv=Hkv)
    names = [r["name"] for r in mfa.quantized_plan(desc)]
    d16 = (H // Hkv) * R <= 16
    assert names[0].startswith("mfa_fwd_decode16_kernel<" if d16 else "mfa_fwd_decode_kernel<"), names
    o, l, deq, _ = run_qforward(Q, K, V, qp, kv, kv, window=win)
    ref = ol.attention(deq["Q"], deq["K"], deq["V"], window=win)
    assert np.isfinite(o.cpu().numpy()).all()
    assert maxerr(o, ref["O"]) < 2e-3 * max(1.0, np.abs(ref["O"]).max())
    assert maxerr(l, ref["L"]) < 7e-3 + 2 ** -11 * np.abs(ref["L"]).max()
    monkeypatch.setenv("MFA_DECODE", "0")
    o2, _, _, _ = run_qforward(Q, K, V, qp, kv, kv, window=win)
    monkeypatch.delenv("MFA_DECODE")
    # The generic path's BF16 P (8 mantissa bits) is held at twice the FP16 tolerance.
    assert maxerr(o2, ref["O"]) < (2e-3 if qp == P.FP16 else 4e-3) * max(1.0, np.abs(ref["O"]).max())


@pytest.mark.parametrize("B,H,Hkv,R,C,D,qp", [
    (2, 4, 4, 1, 1000, 128, P.FP16),
    (1, 8, 2, 3, 777, 64, P.BF16),     # GQA
    (2, 4, 1, 5, 300, 256, P.FP16),    # MQA, D 256
    (1, 16, 1, 4, 300, 128, P.FP16),   # two row tiles, one split: in-workgroup merge
    (1, 2, 2, 16, 4101, 128, P.BF16),  # 16 query rows, partial last tile
    (1, 2, 2, 1, 33, 64, P.FP16),      # one partial 64-key tile
    (1, 4, 4, 7, 70, 96, P.FP16),      # D 96 in the 128-wide tiles
    (1, 4, 4, 3, 2000, 256, P.BF16),   # D 256 on the 16-row kernel
    (2, 8, 2, 4, 700, 224, P.FP16),    # D 224 in the 256-wide tiles, GQA 16 rows
    (1, 2, 2, 3, 20000, 128, P.BF16),  # 39 splits (4-wave merge)
])
def test_decode_int4(gpu, B, H, Hkv, R, C, D, qp, monkeypatch):
    # INT4 K/V cache at decode shapes on the split-KV kernels: the packed tiles are staged as
    # stored and widened in registers (K by row reads, V^T by 4-bit transposed LDS reads); at
    # most 16 rows per kv head take the 16x16x32 kernel.  Held to the oracle on
    # the dequantised values, to the generic dequant-on-load kernel (MFA_DECODE=0) and, for
    # the 16-row kernel, to the 32-row one (MFA_DECODE16=0).
    rng = np.random.default_rng(R * 17 + C)
    Q = rng.standard_normal((B, H, R, D)).astype(np.float32)
    K, V = (rng.standard_normal((B, Hkv, C, D)).astype(np.float32) for _ in range(2))
    base = mfa.AttentionDescriptor.make(R, C, D, low_precision=True, precision=qp)
    desc = mfa.quantized_descriptor(base, qp, P.INT4, P.INT4, B=B, H=H, Hkv=Hkv)
    names = [r["name"] for r in mfa.quantized_plan(desc)]
    d16 = (H // Hkv) * R <= 16
    if d16:
        assert names[0].startswith("mfa_fwd_decode16_kernel<"), names
    else:
        assert names[0].startswith("mfa_fwd_decode_kernel<") and names[0].endswith(", 2>"), names
    o, l, deq, _ = run_qforward(Q, K, V, qp, P.INT4, P.INT4)
    ref = ol.attention(deq["Q"], deq["K"], deq["V"])
    assert np.isfinite(o.cpu().numpy()).all()
    assert maxerr(o, ref["O"]) < 2e-3 * max(1.0, np.abs(ref["O"]).max())
    assert maxerr(l, ref["L"]) < 7e-3 + 2 ** -11 * np.abs(ref["L"]).max()
    monkeypatch.setenv("MFA_DECODE", "0")
    o2, _, _, _ = run_qforward(Q, K, V, qp, P.INT4, P.INT4)
    monkeypatch.delenv("MFA_DECODE")
    # Both paths sit within the oracle tolerance, so within twice it of each other.
    assert maxerr(o, o2.cpu().numpy()) < 4e-3 * max(1.0, np.abs(ref["O"]).max())
    if d16:
        monkeypatch.setenv("MFA_DECODE16", "0")
        assert mfa.quantized_plan(desc)[0]["name"].startswith("mfa_fwd_decode_kernel<")
        o3, l3, _, _ = run_qforward(Q, K, V, qp, P.INT4, P.INT4)
        monkeypatch.delenv("MFA_DECODE16")
        assert maxerr(o, o3.cpu().numpy()) < 2e-3
        assert maxerr(l, l3.float().cpu().numpy()) < 7e-3


def test_decode_int4_zero_points(gpu):
    # Per-tensor zero points on INT4 bytes: nibble n is n - 8, minus zp, exactly.
    B, H, R, C, D = 1, 2, 2, 700, 128
    rng = np.random.default_rng(6)
    Q = rng.standard_normal((B, H, R, D)).astype(np.float32)
    kn = rng.integers(0, 16, (B, H, C, D)).astype(np.uint8)
    vn = rng.integers(0, 16, (B, H, C, D)).astype(np.uint8)
    pack = lambda n: (n.reshape(-1)[0::2] | (n.reshape(-1)[1::2] << 4)).astype(np.uint8)
    ks, vs, kz, vz = 0.2, 0.3, 3, -2
    base = mfa.AttentionDescriptor.make(R, C, D, low_precision=True, precision=P.FP16)
    desc = mfa.quantized_descriptor(base, P.FP16, P.INT4, P.INT4, B=B, H=H)
    tq = mfa.quantized_tensor(to_device(Q, P.FP16), P.FP16)
    tk = mfa.quantized_tensor(tdev(pack(kn), torch.uint8), P.INT4, scale=ks, zero_point=kz)
    tv = mfa.quantized_tensor(tdev(pack(vn), torch.uint8), P.INT4, scale=vs, zero_point=vz)
    o = torch.empty((B, H, R, D), dtype=torch.float32, device=DEV)
    l = torch.empty((B, H, R), dtype=torch.float16, device=DEV)
    assert mfa.quantized_plan(desc, mfa.KernelType.forward, tq, tk, tv)[0]["name"].startswith(
        "mfa_fwd_decode16_kernel<")
    mfa.QuantizedAttention().forward(desc, tq, tk, tv, o, l)
    torch.cuda.synchronize()
    Kd = (kn.astype(np.float32) - 8 - kz) * np.float32(ks)
    Vd = (vn.astype(np.float32) - 8 - vz) * np.float32(vs)
    ref = ol.attention(seen(Q, P.FP16), Kd, Vd)
    assert maxerr(o, ref["O"]) < 2e-3 * max(1.0, np.abs(ref["O"]).max())


def test_decode_nonzero_zero_point(gpu):
    # Per-tensor zero points ride into the widening as (q - zp), exactly.
    B, H, R, C, D = 1, 2, 2, 500, 128
    rng = np.random.default_rng(5)
    Q = rng.standard_normal((B, H, R, D)).astype(np.float32)
    kq = rng.integers(-100, 100, (B, H, C, D)).astype(np.int8)
    vq = rng.integers(-100, 100, (B, H, C, D)).astype(np.int8)
    ks, vs, kz, vz = 0.02, 0.03, 7, -5
    base = mfa.AttentionDescriptor.make(R, C, D, low_precision=True, precision=P.FP16)
    desc = mfa.quantized_descriptor(base, P.FP16, P.INT8, P.INT8, B=B, H=H)
    tq = mfa.quantized_tensor(to_device(Q, P.FP16), P.FP16)
    kt, vt = tdev(kq.view(np.uint8), torch.uint8), tdev(vq.view(np.uint8), torch.uint8)
    tk = mfa.quantized_tensor(kt, P.INT8, scale=ks, zero_point=kz)
    tv = mfa.quantized_tensor(vt, P.INT8, scale=vs, zero_point=vz)
    o = torch.empty((B, H, R, D), dtype=torch.float32, device=DEV)
    l = torch.empty((B, H, R), dtype=torch.float16, device=DEV)
    assert mfa.quantized_plan(desc, mfa.KernelType.forward, tq, tk, tv)[0]["name"].startswith(
        "mfa_fwd_decode16_kernel<")
    mfa.QuantizedAttention().forward(desc, tq, tk, tv, o, l)
    torch.cuda.synchronize()
    Kd = (kq.astype(np.float32) - kz) * np.float32(ks)
    Vd = (vq.astype(np.float32) - vz) * np.float32(vs)
    ref = ol.attention(seen(Q, P.FP16), Kd, Vd)
    assert maxerr(o, ref["O"]) < 2e-3 * max(1.0, np.abs(ref["O"]).max())


# FP16 / BF16 Q with per-tensor INT8 / INT4 K/V at >= 128 query rows per kv head: the
# shared-tile kernel widens the staged bytes to the integers q - zp inside its loop
# (attention_fwd_kv8.hip), with the scales folded as in the dequantisation pass.  Held to the
# oracle on the dequantised values and to the pass + 16-bit kernel path (MFA_KV8=0):
# bit-identical at the padded widths D = 64, 128, 256, where the two run the same tile loop on
# the same operands.
@pytest.mark.parametrize("kv", [P.INT8, P.INT4])
@pytest.mark.parametrize("B,H,Hkv,R,C,D,zps,qp", [
    (1, 4, 4, 300, 1000, 128, (0, 0), P.FP16),    # odd block count: the last pair's group 1 idles
    (2, 4, 2, 256, 333, 128, (0, 0), P.FP16),     # GQA, partial last key tile
    (1, 2, 2, 129, 4101, 96, (7, -5), P.FP16),    # zero points, ragged rows and keys
    (1, 8, 1, 512, 200, 112, (0, 3), P.FP16),     # MQA
    (1, 4, 2, 300, 1000, 128, (3, -2), P.BF16),   # BF16 Q (f32 widening, exact truncation)
    (1, 2, 2, 256, 777, 64, (0, 0), P.FP16),      # D 64: one 8-element chunk per thread
    (1, 3, 3, 200, 300, 48, (5, 1), P.BF16),      # D 48 padded to 64
    (1, 2, 2, 256, 1000, 256, (0, 0), P.FP16),    # D 256: bytes through the LDS byte ring
    (2, 2, 1, 300, 333, 192, (-4, 6), P.BF16),    # D 192 padded to 256, MQA
])
def test_kv8_on_load(gpu, kv, B, H, Hkv, R, C, D, zps, qp, monkeypatch):
    rng = np.random.default_rng(R + C + D)
    Q = rng.standard_normal((B, H, R, D)).astype(np.float32)
    lim = 120 if kv == P.INT8 else 8
    kq = rng.integers(-lim, lim, (B, Hkv, C, D)).astype(np.int8)
    vq = rng.integers(-lim, lim, (B, Hkv, C, D)).astype(np.int8)
    ks, vs = 0.015, 0.02
    base = mfa.AttentionDescriptor.make(R, C, D, low_precision=True, precision=qp)
    desc = mfa.quantized_descriptor(base, qp, kv, kv, B=B, H=H, Hkv=Hkv)
    tq = mfa.quantized_tensor(to_device(Q, qp), qp)
    if kv == P.INT8:
        kt, vt = tdev(kq.view(np.uint8), torch.uint8), tdev(vq.view(np.uint8), torch.uint8)
    else:  # nibble n encodes n - 8, element 2i in the low nibble (GEMMQuantization.swift:500-515)
        pack = lambda x: ((x[..., 0::2] + 8) | ((x[..., 1::2] + 8) << 4)).astype(np.uint8)
        kt, vt = tdev(pack(kq.astype(np.int32)), torch.uint8), tdev(pack(vq.astype(np.int32)), torch.uint8)
    tk = mfa.quantized_tensor(kt, kv, scale=ks, zero_point=zps[0])
    tv = mfa.quantized_tensor(vt, kv, scale=vs, zero_point=zps[1])
    src = 1 if kv == P.INT8 else 2
    DP = 64 if D <= 64 else 128 if D <= 128 else 256
    E = "F16" if qp == P.FP16 else "BF16"
    names = [r["name"] for r in mfa.quantized_plan(desc, mfa.KernelType.forward, tq, tk, tv)]
    if kv == P.INT8 or D % 32 == 0:
        assert names == [f"mfa_fwd2_kv8_kernel<{E}, {DP}, {32 if DP == 256 else 64}, {src}, false>"], names
    else:  # INT4 rows of D / 2 bytes off 16-byte alignment: the dequantisation pass
        assert names[0] == f"mfa_kv_dequant_kernel<{E}, 2>", names

    def run():
        o = torch.full((B, H, R, D), float("nan"), dtype=torch.float32, device=DEV)
        l = torch.full((B, H, R), float("nan"), dtype=torch.float16, device=DEV)
        mfa.QuantizedAttention().forward(desc, tq, tk, tv, o, l)
        torch.cuda.synchronize()
        return o.cpu().numpy(), l.float().cpu().numpy()

    o1, l1 = run()
    monkeypatch.setenv("MFA_KV8", "0")
    assert not mfa.quantized_plan(desc, mfa.KernelType.forward, tq, tk, tv)[-1]["name"].startswith(
        "mfa_fwd2_kv8_kernel")
    o2, l2 = run()
    monkeypatch.delenv("MFA_KV8")
    kd = ((kq.astype(np.float32) - zps[0]) * np.float32(ks)).astype(np.float32)
    vd = ((vq.astype(np.float32) - zps[1]) * np.float32(vs)).astype(np.float32)
    Qs = seen(Q, qp)
    for h in sorted({0, H - 1}):
        ref = ol.attention(Qs[:, h:h + 1], kd[:, h % Hkv:h % Hkv + 1], vd[:, h % Hkv:h % Hkv + 1])
        assert maxerr(o1[:, h:h + 1], ref["O"]) < 2e-3 * max(1.0, np.abs(ref["O"]).max()), h
        assert maxerr(l1[:, h:h + 1], ref["L"]) < 7e-3 + 2 ** -11 * np.abs(ref["L"]).max(), h
    assert np.isfinite(o1).all()
    if D == DP:
        assert np.array_equal(o1, o2) and np.array_equal(l1, l2)
    else:
        assert maxerr(o1, o2) < 1e-5 and maxerr(l1, l2) < 2e-2


# Block-wise INT8 / INT4 K/V scales (and zero points) on load (round 6): the on-load forward's
# block-wise instantiation widens each thread's chunk to (q - zp)·s rounded to the compute type,
# one scale block per chunk (block size a multiple of 16; 8 at D = 64).  Held to the oracle on
# the dequantised FP32 values and bit for bit to the dequantisation pass + 16-bit kernel path
# (MFA_KV8_BW=0), whose dense copy holds the same values.  The block grid is over the
# [B·H_kv·C, D] view (AttentionKernel+OuterProduct.swift:301-316, GEMMHeaders.swift:679-808);
# ragged key counts put block rows across head boundaries.
@pytest.mark.parametrize("kv", [P.INT8, P.INT4])
@pytest.mark.parametrize("B,H,Hkv,R,C,D,bs,zp,qp,causal", [
    (1, 4, 4, 512, 1000, 128, 64, False, P.FP16, False),
    (1, 4, 2, 300, 333, 128, 16, True, P.FP16, False),    # GQA, zero points, partial tiles
    (2, 2, 2, 256, 777, 96, 48, True, P.BF16, False),     # D 96 in 128-wide tiles, bs 48
    (1, 8, 1, 256, 500, 128, 128, False, P.BF16, False),  # MQA
    (1, 2, 2, 256, 300, 64, 8, True, P.FP16, False),      # D 64: 8-element chunks
    (1, 4, 4, 640, 640, 128, 32, True, P.FP16, True),     # causal: adjacent pairs with the mask
])
def test_kv8_blockwise_on_load(gpu, kv, B, H, Hkv, R, C, D, bs, zp, qp, causal, monkeypatch):
    # (These shapes have >= 128 query rows per kv head, where the pass is the default: the
    # on-load kernel is forced, MFA_KV8_BW=1, and held to the pass, MFA_KV8_BW=0.)
    monkeypatch.setenv("MFA_KV8_BW", "1")
    rng = np.random.default_rng(R + C + D + bs)
    Q = rng.standard_normal((B, H, R, D)).astype(np.float32)
    lim = 120 if kv == P.INT8 else 8
    kq = rng.integers(-lim, lim, (B, Hkv, C, D)).astype(np.int8)
    vq = rng.integers(-lim, lim, (B, Hkv, C, D)).astype(np.int8)
    rows = B * Hkv * C
    nb = ((rows + bs - 1) // bs) * ((D + bs - 1) // bs)
    bcols = (D + bs - 1) // bs

    def blocks(lo, hi):
        s = rng.uniform(lo, hi, nb).astype(np.float32)
        z = rng.integers(-3, 4, nb).astype(np.int32) if zp else np.zeros(nb, np.int32)
        return s, z

    (kscale, kzp), (vscale, vzp) = blocks(0.005, 0.03), blocks(0.005, 0.03)
    r_idx = np.arange(rows)[:, None] // bs
    c_idx = np.arange(D)[None, :] // bs
    bi = (r_idx * bcols + c_idx)

    def deq(q, sc, z):
        x = q.reshape(rows, D).astype(np.float32)
        return ((x - z[bi].astype(np.float32)) * sc[bi]).astype(np.float32).reshape(B, Hkv, C, D)

    kd, vd = deq(kq, kscale, kzp), deq(vq, vscale, vzp)
    base = mfa.AttentionDescriptor.make(R, C, D, causal=causal, low_precision=True, precision=qp)
    desc = mfa.quantized_descriptor(base, qp, kv, kv, B=B, H=H, Hkv=Hkv)
    tq = mfa.quantized_tensor(to_device(Q, qp), qp)
    if kv == P.INT8:
        kt, vt = tdev(kq.view(np.uint8), torch.uint8), tdev(vq.view(np.uint8), torch.uint8)
    else:
        pack = lambda x: ((x[..., 0::2] + 8) | ((x[..., 1::2] + 8) << 4)).astype(np.uint8)
        kt, vt = tdev(pack(kq.astype(np.int32)), torch.uint8), tdev(pack(vq.astype(np.int32)), torch.uint8)
    keep = [tdev(kscale), tdev(vscale), torch.from_numpy(kzp).to(DEV), torch.from_numpy(vzp).to(DEV)]
    tk = mfa.QuantizedTensor(kt.data_ptr(), int(kv), 1.0, 0)
    tk.block_scales, tk.block_size = keep[0].data_ptr(), bs
    tv = mfa.QuantizedTensor(vt.data_ptr(), int(kv), 1.0, 0)
    tv.block_scales, tv.block_size = keep[1].data_ptr(), bs
    if zp:
        tk.block_zero_points, tv.block_zero_points = keep[2].data_ptr(), keep[3].data_ptr()
    src = 1 if kv == P.INT8 else 2
    DP = 64 if D <= 64 else 128
    E = "F16" if qp == P.FP16 else "BF16"
    names = [r["name"] for r in mfa.quantized_plan(desc, mfa.KernelType.forward, tq, tk, tv)]
    assert names == [f"mfa_fwd2_kv8_kernel<{E}, {DP}, 64, {src}, true>"], names

    def run():
        o = torch.full((B, H, R, D), float("nan"), dtype=torch.float32, device=DEV)
        l = torch.full((B, H, R), float("nan"), dtype=torch.float16, device=DEV)
        mfa.QuantizedAttention().forward(desc, tq, tk, tv, o, l)
        torch.cuda.synchronize()
        return o.cpu().numpy(), l.float().cpu().numpy()

    o1, l1 = run()
    monkeypatch.setenv("MFA_KV8_BW", "0")
    n2 = [r["name"] for r in mfa.quantized_plan(desc, mfa.KernelType.forward, tq, tk, tv)]
    assert n2[:2] == [f"mfa_kv_dequant_kernel<{E}, {src}>"] * 2, n2
    o2, l2 = run()
    monkeypatch.delenv("MFA_KV8_BW")
    # The default route at these sizes is the pass.
    assert [r["name"] for r in mfa.quantized_plan(desc, mfa.KernelType.forward, tq, tk, tv)] == n2
    assert np.isfinite(o1).all()
    Qs = seen(Q, qp)
    # (BF16 holds (q - zp)·s to 8 significant bits: the pass path shows the same error.)
    tol = 2e-3 if qp == P.FP16 else 2e-2
    for h in sorted({0, H - 1}):
        ref = ol.attention(Qs[:, h:h + 1], kd[:, h % Hkv:h % Hkv + 1], vd[:, h % Hkv:h % Hkv + 1],
                           causal=causal)
        assert maxerr(o1[:, h:h + 1], ref["O"]) < tol * max(1.0, np.abs(ref["O"]).max()), h
        assert maxerr(l1[:, h:h + 1], ref["L"]) < 7e-3 + 2 ** -11 * np.abs(ref["L"]).max(), h
    if not causal:  # (the pass path runs the mirrored kernel on causal shapes: another order)
        assert np.array_equal(o1, o2) and np.array_equal(l1, l2)
    else:
        assert maxerr(o1, o2) < 1e-3 * max(1.0, np.abs(o2).max())


@pytest.mark.parametrize("kv", [P.INT8, P.INT4])
@pytest.mark.parametrize("B,H,Hkv,R,C,D,bs,qp", [
    (1, 8, 2, 16, 900, 128, 32, P.FP16),   # 64 query rows per kv head: on load by default
    (2, 4, 4, 100, 333, 64, 16, P.BF16),   # 100 rows, D 64
])
def test_kv8_blockwise_few_rows_default(gpu, kv, B, H, Hkv, R, C, D, bs, qp, monkeypatch):
    """Block-wise K/V with fewer than 128 query rows per kv head: the on-load kernel is the
    default route (the pass does not pay there); held to the oracle and to the generic
    dequantise-on-store kernel it replaces (MFA_KV8_BW=0)."""
    rng = np.random.default_rng(R * 7 + C + bs)
    Q = rng.standard_normal((B, H, R, D)).astype(np.float32)
    lim = 120 if kv == P.INT8 else 8
    kq = rng.integers(-lim, lim, (B, Hkv, C, D)).astype(np.int8)
    vq = rng.integers(-lim, lim, (B, Hkv, C, D)).astype(np.int8)
    rows, bcols = B * Hkv * C, (D + bs - 1) // bs
    nb = ((rows + bs - 1) // bs) * bcols
    ks, vs = (rng.uniform(0.005, 0.03, nb).astype(np.float32) for _ in range(2))
    kz, vz = (rng.integers(-2, 3, nb).astype(np.int32) for _ in range(2))
    bi = (np.arange(rows)[:, None] // bs) * bcols + np.arange(D)[None, :] // bs
    deq = lambda q, sc, z: ((q.reshape(rows, D).astype(np.float32) - z[bi].astype(np.float32)) *
                            sc[bi]).astype(np.float32).reshape(B, Hkv, C, D)
    kd, vd = deq(kq, ks, kz), deq(vq, vs, vz)
    base = mfa.AttentionDescriptor.make(R, C, D, low_precision=True, precision=qp)
    desc = mfa.quantized_descriptor(base, qp, kv, kv, B=B, H=H, Hkv=Hkv)
    tq = mfa.quantized_tensor(to_device(Q, qp), qp)
    if kv == P.INT8:
        kt, vt = tdev(kq.view(np.uint8), torch.uint8), tdev(vq.view(np.uint8), torch.uint8)
    else:
        pack = lambda x: ((x[..., 0::2] + 8) | ((x[..., 1::2] + 8) << 4)).astype(np.uint8)
        kt, vt = tdev(pack(kq.astype(np.int32)), torch.uint8), tdev(pack(vq.astype(np.int32)), torch.uint8)
    keep = [tdev(ks), tdev(vs), torch.from_numpy(kz).to(DEV), torch.from_numpy(vz).to(DEV)]
    tk = mfa.QuantizedTensor(kt.data_ptr(), int(kv), 1.0, 0)
    tv = mfa.QuantizedTensor(vt.data_ptr(), int(kv), 1.0, 0)
    tk.block_scales, tk.block_zero_points, tk.block_size = keep[0].data_ptr(), keep[2].data_ptr(), bs
    tv.block_scales, tv.block_zero_points, tv.block_size = keep[1].data_ptr(), keep[3].data_ptr(), bs
    src = 1 if kv == P.INT8 else 2
    E = "F16" if qp == P.FP16 else "BF16"
    DP = 64 if D <= 64 else 128
    names = [r["name"] for r in mfa.quantized_plan(desc, mfa.KernelType.forward, tq, tk, tv)]
    assert names == [f"mfa_fwd2_kv8_kernel<{E}, {DP}, 64, {src}, true>"], names

    def run():
        o = torch.full((B, H, R, D), float("nan"), dtype=torch.float32, device=DEV)
        l = torch.full((B, H, R), float("nan"), dtype=torch.float16, device=DEV)
        mfa.QuantizedAttention().forward(desc, tq, tk, tv, o, l)
        torch.cuda.synchronize()
        return o.cpu().numpy(), l.float().cpu().numpy()

    o1, l1 = run()
    monkeypatch.setenv("MFA_KV8_BW", "0")
    assert not mfa.quantized_plan(desc, mfa.KernelType.forward, tq, tk, tv)[-1]["name"].startswith(
        "mfa_fwd2_kv8_kernel")
    o2, _ = run()
    monkeypatch.delenv("MFA_KV8_BW")
    tol = 2e-3 if qp == P.FP16 else 2e-2
    Qs = seen(Q, qp)
    for h in sorted({0, H - 1}):
        ref = ol.attention(Qs[:, h:h + 1], kd[:, h % Hkv:h % Hkv + 1], vd[:, h % Hkv:h % Hkv + 1])
        assert maxerr(o1[:, h:h + 1], ref["O"]) < tol * max(1.0, np.abs(ref["O"]).max()), h
        assert maxerr(l1[:, h:h + 1], ref["L"]) < 7e-3 + 2 ** -11 * np.abs(ref["L"]).max(), h
    assert maxerr(o1, o2) < tol * max(1.0, np.abs(o2).max())


# Causal, FP16 / BF16 Q with per-tensor INT8 / INT4 K/V where the 16-bit path runs the mirrored
# shared-tile schedule (D = 128, up to ~1.5 rounds of blocks): the same schedule widening K/V on
# load (attention_fwd_v2.hip mfa_fwd2_share_kv8_kernel).  Held to the oracle on the dequantised
# values, and bit-identical to the pass + mirrored 16-bit kernel (MFA_KV8=0): phase-1 tiles
# shared by both groups, phase-2 tiles per group, the switch and the merge all see the same
# operands.
@pytest.mark.parametrize("kv", [P.INT8, P.INT4])
@pytest.mark.parametrize("B,H,Hkv,R,C,zps,qp", [
    (1, 4, 4, 1024, 1024, (0, 0), P.FP16),     # 8 blocks: 4 mirrored pairs
    (1, 2, 2, 640, 640, (5, -3), P.FP16),      # 5 blocks: the middle block alone
    (2, 4, 2, 1000, 1000, (0, 2), P.BF16),     # ragged rows, GQA
    (1, 3, 1, 384, 1000, (-7, 0), P.FP16),     # more keys than rows, MQA
    (1, 2, 2, 2048, 2048, (1, 1), P.BF16),
])
def test_kv8_causal_on_load(gpu, kv, B, H, Hkv, R, C, zps, qp, monkeypatch):
    D = 128
    rng = np.random.default_rng(R + 7 * C)
    Q = rng.standard_normal((B, H, R, D)).astype(np.float32)
    lim = 120 if kv == P.INT8 else 8
    kq = rng.integers(-lim, lim, (B, Hkv, C, D)).astype(np.int8)
    vq = rng.integers(-lim, lim, (B, Hkv, C, D)).astype(np.int8)
    ks, vs = 0.015, 0.02
    base = mfa.AttentionDescriptor.make(R, C, D, causal=True, low_precision=True, precision=qp)
    desc = mfa.quantized_descriptor(base, qp, kv, kv, B=B, H=H, Hkv=Hkv)
    tq = mfa.quantized_tensor(to_device(Q, qp), qp)
    if kv == P.INT8:
        kt, vt = tdev(kq.view(np.uint8), torch.uint8), tdev(vq.view(np.uint8), torch.uint8)
    else:
        pack = lambda x: ((x[..., 0::2] + 8) | ((x[..., 1::2] + 8) << 4)).astype(np.uint8)
        kt, vt = tdev(pack(kq.astype(np.int32)), torch.uint8), tdev(pack(vq.astype(np.int32)), torch.uint8)
    tk = mfa.quantized_tensor(kt, kv, scale=ks, zero_point=zps[0])
    tv = mfa.quantized_tensor(vt, kv, scale=vs, zero_point=zps[1])
    src = 1 if kv == P.INT8 else 2
    E = "F16" if qp == P.FP16 else "BF16"
    names = [r["name"] for r in mfa.quantized_plan(desc, mfa.KernelType.forward, tq, tk, tv)]
    assert names == [f"mfa_fwd2_share_kv8_kernel<{E}, 128, 64, {src}>"], names

    def run():
        o = torch.full((B, H, R, D), float("nan"), dtype=torch.float32, device=DEV)
        l = torch.full((B, H, R), float("nan"), dtype=torch.float16, device=DEV)
        mfa.QuantizedAttention().forward(desc, tq, tk, tv, o, l)
        torch.cuda.synchronize()
        return o.cpu().numpy(), l.float().cpu().numpy()

    o1, l1 = run()
    monkeypatch.setenv("MFA_KV8", "0")
    names0 = [r["name"] for r in mfa.quantized_plan(desc, mfa.KernelType.forward, tq, tk, tv)]
    assert names0[-1].startswith("mfa_fwd2_share_kernel<"), names0
    o2, l2 = run()
    monkeypatch.delenv("MFA_KV8")
    kd = ((kq.astype(np.float32) - zps[0]) * np.float32(ks)).astype(np.float32)
    vd = ((vq.astype(np.float32) - zps[1]) * np.float32(vs)).astype(np.float32)
    Qs = seen(Q, qp)
    for h in sorted({0, H - 1}):
        ref = ol.attention(Qs[:, h:h + 1], kd[:, h % Hkv:h % Hkv + 1], vd[:, h % Hkv:h % Hkv + 1],
                           causal=True)
        assert maxerr(o1[:, h:h + 1], ref["O"]) < 2e-3 * max(1.0, np.abs(ref["O"]).max()), h
        assert maxerr(l1[:, h:h + 1], ref["L"]) < 7e-3 + 2 ** -11 * np.abs(ref["L"]).max(), h
    assert np.isfinite(o1).all()
    assert np.array_equal(o1, o2) and np.array_equal(l1, l2)


# Causal (D = 64 / 256, and D = 128 where the mirrored schedule does not apply) and sliding
# window masks on the adjacent-pair on-load kernel (attention_fwd_kv8.hip): the pair stages
# only the key tiles some row of it sees (skip_ok), masked per row like the 16-bit kernels.
# Held to the oracle on the dequantised values and to the pass + 16-bit path (MFA_KV8=0).
@pytest.mark.parametrize("kv", [P.INT8, P.INT4])
@pytest.mark.parametrize("B,H,Hkv,R,C,D,causal,window,qp", [
    (1, 4, 4, 640, 640, 64, True, None, P.FP16),
    (1, 2, 1, 520, 700, 256, True, None, P.BF16),     # ragged rows, MQA, more keys than rows
    (2, 2, 2, 1024, 1024, 256, False, 300, P.FP16),  # window (the sparsity patterns are exclusive)
    (1, 4, 2, 900, 900, 128, False, 200, P.BF16),    # window only (rows keep keys >= r - 200)
    (4, 48, 48, 1024, 1024, 128, True, None, P.FP16),  # 1,536 blocks: not the mirrored schedule
])
def test_kv8_masked_on_load(gpu, kv, B, H, Hkv, R, C, D, causal, window, qp, monkeypatch):
    rng = np.random.default_rng(R + 3 * C + D)
    Q = rng.standard_normal((B, H, R, D)).astype(np.float32)
    lim = 120 if kv == P.INT8 else 8
    kq = rng.integers(-lim, lim, (B, Hkv, C, D)).astype(np.int8)
    vq = rng.integers(-lim, lim, (B, Hkv, C, D)).astype(np.int8)
    ks, vs, zps = 0.015, 0.02, (3, -2)
    base = mfa.AttentionDescriptor.make(R, C, D, causal=causal, window=window, low_precision=True,
                                        precision=qp)
    desc = mfa.quantized_descriptor(base, qp, kv, kv, B=B, H=H, Hkv=Hkv)
    tq = mfa.quantized_tensor(to_device(Q, qp), qp)
    if kv == P.INT8:
        kt, vt = tdev(kq.view(np.uint8), torch.uint8), tdev(vq.view(np.uint8), torch.uint8)
    else:
        pack = lambda x: ((x[..., 0::2] + 8) | ((x[..., 1::2] + 8) << 4)).astype(np.uint8)
        kt, vt = tdev(pack(kq.astype(np.int32)), torch.uint8), tdev(pack(vq.astype(np.int32)), torch.uint8)
    tk = mfa.quantized_tensor(kt, kv, scale=ks, zero_point=zps[0])
    tv = mfa.quantized_tensor(vt, kv, scale=vs, zero_point=zps[1])
    names = [r["name"] for r in mfa.quantized_plan(desc, mfa.KernelType.forward, tq, tk, tv)]
    assert names[0].startswith("mfa_fwd2_kv8_kernel<"), names

    def run():
        o = torch.full((B, H, R, D), float("nan"), dtype=torch.float32, device=DEV)
        l = torch.full((B, H, R), float("nan"), dtype=torch.float16, device=DEV)
        mfa.QuantizedAttention().forward(desc, tq, tk, tv, o, l)
        torch.cuda.synchronize()
        return o.cpu().numpy(), l.float().cpu().numpy()

    o1, l1 = run()
    monkeypatch.setenv("MFA_KV8", "0")
    o2, l2 = run()
    monkeypatch.delenv("MFA_KV8")
    kd = ((kq.astype(np.float32) - zps[0]) * np.float32(ks)).astype(np.float32)
    vd = ((vq.astype(np.float32) - zps[1]) * np.float32(vs)).astype(np.float32)
    Qs = seen(Q, qp)
    assert np.isfinite(o1).all()
    for h in sorted({0, H - 1}):
        ref = ol.attention(Qs[:, h:h + 1], kd[:, h % Hkv:h % Hkv + 1], vd[:, h % Hkv:h % Hkv + 1],
                           causal=causal, window=window)
        assert maxerr(o1[:, h:h + 1], ref["O"]) < 2e-3 * max(1.0, np.abs(ref["O"]).max()), h
        assert maxerr(l1[:, h:h + 1], ref["L"]) < 7e-3 + 2 ** -11 * np.abs(ref["L"]).max(), h
    assert maxerr(o1, o2) < 2e-3 * max(1.0, np.abs(o2).max())
    assert maxerr(l1, l2) < 7e-3 + 2 ** -10 * np.abs(l2).max()  # L is stored in fp16


def _ref_dequant_transposed_block(e, B, H, S, D, bs, scales):
    """The reference's block lookup for a transposed quantised operand, written out per element
    (AttentionKernel+Accumulate.swift:461-472, AttentionKernel+OuterProduct.swift:301-316):
    the head's memory is [D][S]; element (seq c, dim d) of head (b, h) uses block
    ((row0 + d) / bs) * ceil(S / bs) + c / bs with row0 = (b * H + h) * D, because rowExpr =
    d_outer + d, colExpr = traversal + c and num_blocks_col = ceil(leadingDimension / bs),
    leadingDimension = S when transposed.  `e` holds the integers in memory order [B, H, D, S]
    (INT8 as stored; INT4 as q - 8 already).  Returns the logical [B, H, S, D] values."""
    nbc = (S + bs - 1) // bs
    out = np.empty((B, H, S, D), np.float32)
    c = np.arange(S)[:, None]
    d = np.arange(D)[None, :]
    for b in range(B):
        for h in range(H):
            row0 = (b * H + h) * D
            bi = ((row0 + d) // bs) * nbc + c // bs           # [S, D]
            out[b, h] = e[b, h].T.astype(np.float32) * scales[bi]
    return out


@pytest.mark.parametrize("blockwise", [None, 16])
@pytest.mark.parametrize("kv", [P.INT8, P.INT4])
def test_transposed_quantized_kv_matches_reference_layout(gpu, blockwise, kv):
    # A transposed K / V (column-major within each head, AttentionKernelDescriptor
    # transposeState).  Blockwise scales follow the reference's lookup for transposed operands:
    # the block grid is over the memory view [B·H·D rows][S cols] (it was the
    # logical [B·H·S, D] grid).  The quantised tensor is made as the reference's factory makes
    # it for that buffer: its memory view quantised block by block.  Expected values come from
    # the reference's index formula written out per element (_ref_dequant_transposed_block),
    # not from the repo's quantiser; the row-major run checks against its own view.
    B, H, S, D = 1, 2, 96, 64
    rng = np.random.default_rng(21)
    Q, K, V = (rng.standard_normal((B, H, S, D)).astype(np.float32) for _ in range(3))
    # Column and row scale ramps make a wrong block lookup visible.
    K *= np.linspace(0.2, 3.0, S, dtype=np.float32)[None, None, :, None]
    V *= np.linspace(3.0, 0.2, S, dtype=np.float32)[None, None, :, None]
    K *= np.linspace(0.5, 2.0, D, dtype=np.float32)[None, None, None, :]
    tq = mfa.quantized_tensor(to_device(Q, P.FP16), P.FP16)
    keep = []

    def qt(x, transposed):
        mem = np.ascontiguousarray(x.transpose(0, 1, 3, 2)) if transposed else x
        rows, cols = (B * H * D, S) if transposed else (B * H * S, D)
        if blockwise:
            sc = ol.quant_scales_block(mem, rows, cols, blockwise, int(kv))
            q = ol.quantize_block(mem, cols, blockwise, int(kv), sc)
            kw = {"block_scales": tdev(sc), "block_size": blockwise}
        else:
            s = ol.quant_scale_tensor(mem, int(kv))
            q = ol.quantize(mem, int(kv), s)
            kw = {"scale": s}
        if kv == P.INT4:
            ints = np.empty(x.size, np.int32)
            ints[0::2], ints[1::2] = (q[: (x.size + 1) // 2] & 15), (q[: x.size // 2] >> 4)
            ints -= 8
        else:
            ints = np.asarray(q[: x.size]).view(np.int8).astype(np.int32)
        if transposed and blockwise:
            deq = _ref_dequant_transposed_block(ints.reshape(B, H, D, S), B, H, S, D, blockwise, sc)
        elif blockwise:
            deq = ol.dequantize_block(q, x.size, cols, blockwise, int(kv), sc).reshape(x.shape)
        else:
            deq = (ints.astype(np.float32) * np.float32(s)).reshape(mem.shape)
            if transposed:
                deq = np.ascontiguousarray(deq.transpose(0, 1, 3, 2))
        t = mfa.quantized_tensor(tdev(q, torch.uint8), kv, **kw)
        keep.append(t)
        return t, deq

    for tr in (False, True):
        base = mfa.AttentionDescriptor.make(S, S, D, transpose=(False, tr, tr, False))
        desc = mfa.quantized_descriptor(base, P.FP16, kv, kv, B=B, H=H, Hkv=H)
        o = torch.full((B, H, S, D), float("nan"), dtype=torch.float32, device=DEV)
        (tk, dk), (tv, dv) = qt(K, tr), qt(V, tr)
        mfa.QuantizedAttention().forward(desc, tq, tk, tv, o)
        torch.cuda.synchronize()
        ref = ol.attention(seen(Q, P.FP16), dk, dv)["O"]
        assert torch.isfinite(o).all()
        assert maxerr(o, ref) < 5e-3, tr


def test_forward_from_float_transposed_blockwise(gpu):
    # The runtime-quantising entry quantises a transposed buffer as its memory view, so the
    # result equals quantising that view by hand and calling mfa_quantized_forward.
    B, H, S, D, bs = 1, 2, 128, 64, 32
    rng = np.random.default_rng(5)
    Q, K, V = (rng.standard_normal((B, H, S, D)).astype(np.float32) for _ in range(3))
    K *= np.linspace(0.2, 3.0, S, dtype=np.float32)[None, None, :, None]
    Kt, Vt = (np.ascontiguousarray(x.transpose(0, 1, 3, 2)) for x in (K, V))
    base = mfa.AttentionDescriptor.make(S, S, D, transpose=(False, True, True, False))
    desc = mfa.quantized_descriptor(base, P.INT8, P.INT8, P.INT8, B=B, H=H, Hkv=H)
    o1 = torch.full((B, H, S, D), float("nan"), dtype=torch.float32, device=DEV)
    mfa.QuantizedAttention().forward_from_buffers(desc, tdev(Q), tdev(Kt), tdev(Vt), o1, P.INT8,
                                                  mfa.QuantMode.blockwise, bs)
    torch.cuda.synchronize()
    keep = []
    ts = []
    for x, rows, cols in ((Q, B * H * S, D), (Kt, B * H * D, S), (Vt, B * H * D, S)):
        sc = ol.quant_scales_block(x, rows, cols, bs, int(P.INT8))
        q = ol.quantize_block(x, cols, bs, int(P.INT8), sc)
        t = mfa.quantized_tensor(tdev(q, torch.uint8), P.INT8, block_scales=tdev(sc), block_size=bs)
        keep.append(t)
        ts.append(t)
    o2 = torch.full_like(o1, float("nan"))
    mfa.QuantizedAttention().forward(desc, *ts, o2)
    torch.cuda.synchronize()
    assert torch.equal(o1, o2)


@pytest.mark.parametrize("target,mode,bs", [(P.INT8, mfa.QuantMode.tensorWise, 0),
                                            (P.INT4, mfa.QuantMode.tensorWise, 0),
                                            (P.INT8, mfa.QuantMode.blockwise, 32)])
@pytest.mark.parametrize("src", [torch.float16, torch.float32])
def test_forward_from_float_buffers(gpu, target, mode, bs, src):
    # QuantizedAttention.forward(queryBuffer:...:targetQuantization:quantizationMode:descriptor:)
    # (QuantizedAttention.swift:278-336): the C-ABI entry quantizes Q, K, V on the GPU and runs
    # the quantized forward; it must equal mfa_quantize of each tensor followed by
    # mfa_quantized_forward on the results, bit for bit.
    B, H, Hkv, S, D = 1, 4, 2, 256, 64
    g = torch.Generator(device=DEV).manual_seed(3)
    q = torch.randn((B, H, S, D), generator=g, device=DEV).to(src)
    k = torch.randn((B, Hkv, S, D), generator=g, device=DEV).to(src)
    v = torch.randn((B, Hkv, S, D), generator=g, device=DEV).to(src)
    base = mfa.AttentionDescriptor.make(S, S, D, causal=True)
    desc = mfa.quantized_descriptor(base, target, target, target, B=B, H=H, Hkv=Hkv)
    o1 = torch.full((B, H, S, D), float("nan"), dtype=torch.float32, device=DEV)
    qa = mfa.QuantizedAttention()
    qa.forward_from_buffers(desc, q, k, v, o1, target, mode, bs)
    torch.cuda.synchronize()
    keep = []

    def manual(x):
        rows = x.numel() // D
        data, sc, bsc, bzp = mfa.quantize(x.reshape(-1), target, mode, rows, D, bs)
        torch.cuda.synchronize()
        keep.append((data, sc, bsc, bzp))
        if mode == mfa.QuantMode.blockwise:
            return mfa.quantized_tensor(data, target, block_scales=bsc, block_zero_points=bzp,
                                        block_size=bs)
        return mfa.quantized_tensor(data, target, scale=sc.item())

    o2 = torch.full_like(o1, float("nan"))
    qa.forward(desc, manual(q), manual(k), manual(v), o2)
    torch.cuda.synchronize()
    assert torch.isfinite(o1).all()
    assert torch.equal(o1, o2)
    # And the reference's gate against the unquantized inputs (QuantizedAttentionTest.swift:519).
    ref = ol.attention(q.float().cpu().numpy(), k.float().cpu().numpy(), v.float().cpu().numpy(),
                       causal=True)["O"]
    assert relerr(o1, ref) < (0.25 if target == P.INT8 else 0.6)


def test_forward_from_float_buffers_wraps_unquantized_target(gpu):
    # A target without quantization parameters wraps the buffers (:425-441): the FP16 forward.
    B, H, S, D = 1, 2, 128, 64
    g = torch.Generator(device=DEV).manual_seed(4)
    q, k, v = (torch.randn((B, H, S, D), generator=g, device=DEV).half() for _ in range(3))
    base = mfa.AttentionDescriptor.make(S, S, D)
    desc = mfa.quantized_descriptor(base, P.INT8, P.INT8, P.INT8, B=B, H=H)
    o1 = torch.empty((B, H, S, D), dtype=torch.float32, device=DEV)
    mfa.QuantizedAttention().forward_from_buffers(desc, q, k, v, o1, P.FP16)
    torch.cuda.synchronize()
    ref = ol.attention(*(t.float().cpu().numpy() for t in (q, k, v)))["O"]
    assert maxerr(o1, ref) < 5e-3


@pytest.mark.parametrize("kv", [P.INT8, P.INT4])
@pytest.mark.parametrize("D,causal,Hkv,zps,prec", [(128, True, 2, (0, 0), P.FP16),
                                                   (64, False, 4, (3, -2), P.BF16),
                                                   (256, False, 1, (0, 0), P.FP16),
                                                   (256, True, 2, (-5, 4), P.BF16)])
def test_backward_key_value_widens_in_registers(gpu, kv, D, causal, Hkv, zps, prec, monkeypatch):
    """backwardKeyValue alone with 16-bit Q/dO reads per-tensor INT8/INT4 K/V straight into the
    tuned kernel's registers (no dequantisation pass): dK and dV are bit-identical to the pass
    path (MFA_KV_REGS=0), and match the oracle on the dequantised values."""
    B, H, S = 1, 4, 320
    rng = np.random.default_rng(D + 7 * Hkv)
    Q, dO = (rng.standard_normal((B, H, S, D)).astype(np.float32) * 0.5 for _ in range(2))
    K, V = (rng.standard_normal((B, Hkv, S, D)).astype(np.float32) * 0.5 for _ in range(2))
    kq, ks, kd = quantize_host(K, kv)
    vq, vs, vd = quantize_host(V, kv)
    kz, vz = zps
    if kv == P.INT4:
        kz, vz = max(-7, min(7, kz)), max(-7, min(7, vz))
    base = mfa.AttentionDescriptor.make(S, S, D, causal=causal, low_precision=True, precision=prec)
    desc = mfa.quantized_descriptor(base, prec, kv, kv, B=B, H=H, Hkv=Hkv)
    tq = mfa.quantized_tensor(to_device(Q, prec), prec)
    tk = mfa.quantized_tensor(tdev(kq, torch.uint8), kv, scale=ks, zero_point=kz)
    tv = mfa.quantized_tensor(tdev(vq, torch.uint8), kv, scale=vs, zero_point=vz)
    # The reference of the zero-point-shifted tensors: (q - zp) * s.
    kd = ol.dequantize(kq, K.size, int(kv), ks, kz).reshape(K.shape) if kz else kd
    vd = ol.dequantize(vq, V.size, int(kv), vs, vz).reshape(V.shape) if vz else vd
    Qd, dOd = seen(Q, prec), seen(dO, prec)
    # Query head h reads kv head h % Hkv (MultiHeadAttention broadcast).
    ref = ol.attention(Qd, np.tile(kd, (1, H // Hkv, 1, 1)), np.tile(vd, (1, H // Hkv, 1, 1)),
                       dO=dOd, causal=causal)
    o = tdev(ref["O"])
    l = torch.from_numpy(ref["L"]).half().to(DEV)
    do = to_device(dO, prec)
    dvals = torch.empty((B, H, S), dtype=torch.bfloat16, device=DEV)
    qa = mfa.QuantizedAttention()
    dq = torch.empty((B, H, S, D), dtype=torch.float32, device=DEV)
    qa.backwardQuery(desc, tq, tk, tv, o, do, l, dq, dvals)
    outs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("MFA_KV_REGS", mode)
        dk = torch.full((B, Hkv, S, D), float("nan"), dtype=torch.float32, device=DEV)
        dv = torch.full_like(dk, float("nan"))
        mfa.last_launches()
        qa.backwardKeyValue(desc, tq, tk, tv, do, l, dvals, dk, dv)
        torch.cuda.synchronize()
        outs[mode] = (dk, dv, [r["name"] for r in mfa.last_launches()])
    names = outs["1"][2]
    assert not any("dequant" in n for n in names), names
    assert names[-1].startswith("mfa_bwd_kv_fast_kernel<"), names
    assert any("dequant" in n for n in outs["0"][2]), outs["0"][2]
    assert torch.equal(outs["0"][0], outs["1"][0]) and torch.equal(outs["0"][1], outs["1"][1])
    gk = ref["dK"].reshape(B, H // Hkv, Hkv, S, D).sum(axis=1)
    gv = ref["dV"].reshape(B, H // Hkv, Hkv, S, D).sum(axis=1)
    assert maxerr(outs["1"][0], gk) < 5e-2 and maxerr(outs["1"][1], gv) < 5e-2
