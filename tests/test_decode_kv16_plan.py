"""CPU tests of the split-KV decode route for FP16 / BF16 K/V caches (csrc/mfa_api.cpp
decode_kv16_eligible, attention_decode.hip SRC_SAME = 0): the plan query runs the real
dispatcher with launches recorded, so no GPU is needed.  The GPU twin is
test_decode_kv16_gpu.py."""
import ctypes
import os
import subprocess
import sys

import mfa_amd as mfa

P = mfa.Precision


def desc(B, H, Hkv, R, C, D, prec=P.FP16, **kw):
    lp = prec != P.FP32
    base = mfa.AttentionDescriptor.make(low_precision=lp, precision=prec if lp else None, **kw)
    return mfa.MultiHeadDescriptor.make(base, B, H, R, D, Hkv=Hkv, C=C)


def names(*a, **kw):
    return [r["name"] for r in mfa.multihead_plan(desc(*a, **kw))]


def test_bench_decode_shape_is_one_16_row_launch():
    # B32 H16 S_q 1 S_kv 8192 D128 (the INT8 bench shape with an FP16 cache): 512 units, one
    # split each, merged in LDS: no merge launch, no workspace.
    plan = mfa.multihead_plan(desc(32, 16, 16, 1, 8192, 128))
    assert [r["name"] for r in plan] == ["mfa_fwd_decode16_kernel<F16, 128, 0>"]
    assert plan[0]["threads"] == 256 and plan[0]["workgroups"] == 512
    assert plan[0]["lds_bytes"] <= 160 * 1024
    assert names(32, 16, 16, 16, 8192, 128) == ["mfa_fwd_decode16_kernel<F16, 128, 0>"]


def test_split_shapes_add_the_merge_launch():
    assert names(8, 32, 4, 1, 16384, 256, prec=P.BF16) == \
        ["mfa_fwd_decode16_kernel<BF16, 256, 0>", "mfa_decode_merge_kernel"]
    # 38 splits per row (> 32): one row per 4-wave workgroup.
    assert names(1, 2, 2, 1, 24000, 64) == \
        ["mfa_fwd_decode16_kernel<F16, 64, 0>", "mfa_decode_merge4_kernel"]


def test_more_than_16_rows_take_the_32_row_form():
    assert names(8, 32, 4, 4, 16384, 128)[0] == "mfa_fwd_decode_kernel<F16, 128, 0>"
    assert names(2, 4, 1, 5, 4096, 256, prec=P.BF16)[0] == "mfa_fwd_decode_kernel<BF16, 256, 0>"
    assert names(8, 32, 4, 2, 16384, 128)[0] == "mfa_fwd_decode16_kernel<F16, 128, 0>"  # 16 rows
    # By default the 32-row form needs a GQA group of at least 4 query heads: without one the
    # 128-row kernel reads K/V once per head too, and measured as fast or faster.
    _is_today(names(32, 16, 16, 32, 8192, 128))
    _is_today(names(32, 16, 8, 16, 8192, 128))
    assert names(32, 16, 16, 16, 8192, 128)[0].startswith("mfa_fwd_decode16_kernel<")
    _is_today(names(8, 32, 8, 17, 8192, 128))  # 68 rows per kv head


def test_masks_the_kernel_serves(monkeypatch):
    assert names(2, 4, 4, 16, 8192, 128, window=64)[0].startswith("mfa_fwd_decode16_kernel<")
    # Causal: 16 rows see 16 keys at most, below the default bound on keys read.
    _is_today(names(2, 4, 4, 16, 8192, 128, causal=True))
    monkeypatch.setenv("MFA_DECODE_KV16", "1")
    assert names(2, 4, 4, 16, 8192, 128, causal=True) == ["mfa_fwd_decode16_kernel<F16, 128, 0>"]
    # A window that leaves rows without any key (R > C + window) keeps the finite-mask kernels.
    _is_today(names(1, 2, 2, 100, 40, 64, window=3))


def _is_today(ns):
    assert ns and not any("decode" in n for n in ns), ns


def test_ineligible_calls_keep_their_kernels(monkeypatch):
    shape = (32, 16, 16, 1, 8192, 128)
    assert names(*shape)[0].startswith("mfa_fwd_decode16_kernel<")
    # FP32 inputs.
    _is_today(names(*shape, prec=P.FP32))
    # Sparse ranges (the plan needs no mask buffer to pick the kernel).
    _is_today(names(*shape, sparse_mask=mfa.MaskType.sparseRanges))
    # An additive mask, a misaligned K pointer: plans with explicit buffers.
    d = desc(*shape)

    def with_buffers(**kw):
        b = mfa.AttentionBuffers()
        b.Q, b.K, b.V, b.O = 0x100000, 0x200000, 0x300000, 0x400000
        for k, v in kw.items():
            setattr(b, k, v)
        out = mfa.KernelPlan()
        mfa.check(mfa.lib.mfa_multihead_plan(ctypes.byref(d), 0, ctypes.byref(b), ctypes.byref(out)))
        return [r["name"] for r in out.as_list()]

    assert with_buffers()[0].startswith("mfa_fwd_decode16_kernel<")
    _is_today(with_buffers(mask=0x500000))
    _is_today(with_buffers(K=0x200002))
    # The development switch.
    monkeypatch.setenv("MFA_DECODE_KV16", "0")
    _is_today(names(*shape))


def test_small_caches_keep_their_kernels_by_default(monkeypatch):
    # Below the routing bound on keys (at least 512): the existing suite's small decode-like
    # calls, e.g. cross attention with (R, C) = (1, 257), run what they ran.
    _is_today(names(1, 2, 2, 1, 257, 64))
    # MFA_DECODE_KV16=1 routes any eligible size (how the GPU tests reach small shapes).
    monkeypatch.setenv("MFA_DECODE_KV16", "1")
    assert names(1, 2, 2, 1, 257, 64) == ["mfa_fwd_decode16_kernel<F16, 64, 0>"]


_CHILD = r"""
import os, sys
sys.path.insert(0, os.path.join(sys.argv[1], "metal-flash-attention-plus_amd", "python"))
import mfa_amd as mfa
base = mfa.AttentionDescriptor.make(low_precision=True, precision=mfa.Precision.FP16)
d = mfa.MultiHeadDescriptor.make(base, 32, 16, 1, 128, C=8192)
print(mfa.multihead_plan(d)[0]["name"])
"""


def test_switch_is_a_development_switch():
    # Without MFA_DEV=1 the process environment cannot turn the route off (mfa_launch.h dev_env).
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if not k.startswith("MFA_")}
    env["MFA_DECODE_KV16"] = "0"
    r = subprocess.run([sys.executable, "-c", _CHILD, repo], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == "mfa_fwd_decode16_kernel<F16, 128, 0>"


def test_quantized_entry_with_16_bit_kv_takes_the_route():
    base = mfa.AttentionDescriptor.make(1, 8192, 128, low_precision=True, precision=P.FP16)
    q = mfa.quantized_descriptor(base, P.FP16, P.FP16, P.FP16, B=32, H=16)
    assert [r["name"] for r in mfa.quantized_plan(q)] == ["mfa_fwd_decode16_kernel<F16, 128, 0>"]
