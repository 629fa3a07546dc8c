"""CPU tests of the paged, ragged KV-cache decode entry (mfa_paged_decode_forward /
mfa_paged_decode_plan in csrc/mfa_api.cpp; the *_paged_kernel entry points of
attention_decode.hip): the symbols, the plans, every host validation rule and the new kernels'
code-object resources.  The plan query runs the real dispatcher with launches recorded, and a
rejected call returns before anything touches a device, so no GPU is needed.  The GPU twin is
test_paged_decode_gpu.py."""
import ctypes
import os
import re

import pytest

import mfa_amd as mfa
from harness import kernels_named, paged_cache as cache, paged_cache_full as full

P = mfa.Precision
_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_DESCRIPTOR, UNSUPPORTED, INVALID_ARGUMENT = 0, 1, 2, 4  # mfa_status_t


def desc(B=2, H=8, Hkv=2, R=1, D=128, prec=P.FP16, max_seq_len=1000, **kw):
    base = mfa.AttentionDescriptor.make(low_precision=True, precision=prec, **kw)
    return mfa.PagedDecodeDescriptor.make(base, B, H, R, D, max_seq_len, Hkv=Hkv)


def names(d, c=None):
    return [r["name"] for r in mfa.paged_decode_plan(d, cache(d) if c is None else c)]


def test_symbols_are_declared_and_exported():
    for n in ("mfa_paged_decode_forward", "mfa_paged_decode_plan"):
        assert n in mfa.header_functions()
        assert hasattr(mfa.lib, n)
        assert getattr(mfa.lib, n).argtypes is not None
    text = open(mfa.HEADER_PATH).read()
    assert "mfa_paged_kv_cache_t" in text and "mfa_paged_decode_descriptor_t" in text


def test_status_codes_match_the_header():
    text = open(mfa.HEADER_PATH).read()
    for name, val in (("MFA_ERR_INVALID_ARGUMENT", INVALID_ARGUMENT),
                      ("MFA_ERR_INVALID_DESCRIPTOR", INVALID_DESCRIPTOR),
                      ("MFA_ERR_UNSUPPORTED", UNSUPPORTED)):
        assert re.search(name + r"\s*=\s*" + str(val) + r"\b", text), name


def contiguous_names(monkeypatch, B, H, Hkv, R, D, C, prec=P.FP16):
    """What the contiguous decode route launches for one dense cache of C keys."""
    monkeypatch.setenv("MFA_DECODE_KV16", "1")
    base = mfa.AttentionDescriptor.make(low_precision=True, precision=prec)
    d = mfa.MultiHeadDescriptor.make(base, B, H, R, D, Hkv=Hkv, C=C)
    return [r["name"] for r in mfa.multihead_plan(d)]


def test_plan_follows_the_contiguous_layout(monkeypatch):
    # B2 H8/2 R1 D128 FP16, max_seq_len 1000, page 64: the 16-row paged kernel, and the launches
    # of the contiguous route at C = 1000 (decode_layout on max_seq_len: 32 tiles are two splits
    # of 16, so a merge pass follows, there and here).
    plan = mfa.paged_decode_plan(desc(), cache(desc()))
    got = [r["name"] for r in plan]
    assert got[0] == "mfa_fwd_decode16_paged_kernel<F16, 128, 0>"
    assert [n.replace("_paged", "") for n in got] == contiguous_names(monkeypatch, 2, 8, 2, 1, 128, 1000)
    assert plan[0]["threads"] == 256 and plan[0]["lds_bytes"] <= 160 * 1024


def test_one_split_is_a_single_16_row_launch(monkeypatch):
    # Fewer than 32 tiles of keys: one split per unit, merged in LDS, no workspace.
    d = desc(max_seq_len=500)
    plan = mfa.paged_decode_plan(d, cache(d))
    assert [r["name"] for r in plan] == ["mfa_fwd_decode16_paged_kernel<F16, 128, 0>"]
    assert plan[0]["workgroups"] == 4  # B 2 x H_kv 2, one split
    assert contiguous_names(monkeypatch, 2, 8, 2, 1, 128, 500) == ["mfa_fwd_decode16_kernel<F16, 128, 0>"]


def test_split_shapes_add_the_merge_launch():
    assert names(desc(B=1, max_seq_len=2500)) == \
        ["mfa_fwd_decode16_paged_kernel<F16, 128, 0>", "mfa_decode_merge_kernel"]
    # The split follows min(max_seq_len, pages x page size): a short table keeps one split.
    d = desc(B=1, max_seq_len=2500)
    short = mfa.PagedKVCache.make(P.FP16, 64, 7, 8, 2, 128)      # 448 keys at most
    assert names(d, short) == ["mfa_fwd_decode16_paged_kernel<F16, 128, 0>"]
    d = desc(B=2, H=2, Hkv=2, D=64, max_seq_len=24000)
    assert names(d, cache(d, page=256)) == \
        ["mfa_fwd_decode16_paged_kernel<F16, 64, 0>", "mfa_decode_merge4_kernel"]


def test_more_than_16_rows_take_the_32_row_form():
    assert names(desc(R=4))[0] == "mfa_fwd_decode16_paged_kernel<F16, 128, 0>"  # 16 rows
    assert names(desc(R=5))[0] == "mfa_fwd_decode_paged_kernel<F16, 128, 0>"
    d = desc(H=16, Hkv=1, R=4, max_seq_len=500)
    plan = mfa.paged_decode_plan(d, cache(d))
    assert plan[0]["name"] == "mfa_fwd_decode_paged_kernel<F16, 128, 0>"
    assert plan[0]["workgroups"] == 2 * 2  # two row tiles per kv head


def test_int8_caches_take_the_int8_instantiations():
    d = desc()
    c8 = cache(d, prec=P.INT8, k_scale=0.02, v_scale=0.03, k_zero_point=3, v_zero_point=-5)
    assert names(d, c8)[0] == "mfa_fwd_decode16_paged_kernel<F16, 128, 1>"
    d = desc(R=5, prec=P.BF16, max_seq_len=500)
    assert names(d, cache(d, prec=P.INT8)) == ["mfa_fwd_decode_paged_kernel<BF16, 128, 1>"]


@pytest.mark.parametrize("prec,tag", [(P.FP16, "F16"), (P.BF16, "BF16")])
@pytest.mark.parametrize("D,DP", [(64, 64), (72, 128), (128, 128), (256, 256)])
def test_types_and_head_dims_resolve(prec, tag, D, DP):
    assert names(desc(D=D, prec=prec, max_seq_len=500)) == [f"mfa_fwd_decode16_paged_kernel<{tag}, {DP}, 0>"]
    assert names(desc(D=D, prec=prec, R=5))[0] == f"mfa_fwd_decode_paged_kernel<{tag}, {DP}, 0>"


def test_plan_without_a_cache_and_causal():
    assert names(desc(causal=True))[0] == "mfa_fwd_decode16_paged_kernel<F16, 128, 0>"
    assert [r["name"] for r in mfa.paged_decode_plan(desc(max_seq_len=500))] == \
        ["mfa_fwd_decode16_paged_kernel<F16, 128, 0>"]


def status(d, c, query=0x100000, output=0x200000, strides=None):
    """mfa_paged_decode_forward's status for a call the host must reject (or an empty one): none
    of these reaches a launch, so the stand-in addresses are never used."""
    s = (ctypes.c_int64 * 4)(*strides) if strides else None
    st = mfa.lib.mfa_paged_decode_forward(ctypes.byref(d) if d is not None else None, query, s,
                                          ctypes.byref(c) if c is not None else None, output,
                                          None, None)
    if st != OK:
        assert mfa.lib.mfa_last_error(), "empty error message"
    return st


def test_null_pointers_are_invalid_arguments():
    d = desc()
    assert status(None, full(d)) == INVALID_ARGUMENT
    assert status(d, None) == INVALID_ARGUMENT
    assert status(d, full(d), query=None) == INVALID_ARGUMENT
    assert status(d, full(d), output=None) == INVALID_ARGUMENT
    for field in ("k_pool", "v_pool", "block_table", "seq_lens"):
        c = full(d)
        setattr(c, field, None)
        assert status(d, c) == INVALID_ARGUMENT, field
    out = mfa.KernelPlan()
    assert mfa.lib.mfa_paged_decode_plan(None, None, ctypes.byref(out)) == INVALID_ARGUMENT
    assert mfa.lib.mfa_paged_decode_plan(ctypes.byref(d), None, None) == INVALID_ARGUMENT


def test_bad_shapes_are_invalid_descriptors():
    for kw in ({"H": 0, "Hkv": 0}, {"D": 0}, {"max_seq_len": 0}):
        d = desc(**kw)
        c = full(desc())
        assert status(d, c) == INVALID_DESCRIPTOR, kw
    d = desc()
    for field in ("max_pages_per_seq", "num_pages"):
        c = full(d)
        setattr(c, field, 0)
        assert status(d, c) == INVALID_DESCRIPTOR, field
    d = desc(H=8, Hkv=3)
    assert status(d, full(d)) == INVALID_DESCRIPTOR


def test_unsupported_calls():
    d = desc()
    for page in (0, 16, 48, 96):                       # not a power of two, or below 32
        c = full(d)
        c.page_size = page
        assert status(d, c) == UNSUPPORTED, page
    for D in (68, 264, 512):                           # D % 8, D > 256
        dd = desc(D=D)
        assert status(dd, full(dd)) == UNSUPPORTED, D
    dd = desc(D=72)                                    # INT8 rows need D % 16 (16-bit: D % 8)
    assert status(dd, full(dd, prec=P.INT8)) == UNSUPPORTED
    for prec in (P.INT4, P.FP32):                      # INT4 pools: a later change
        assert status(d, full(d, prec=prec)) == UNSUPPORTED, prec
    assert status(d, full(d, prec=P.BF16)) == UNSUPPORTED          # differs from Q's FP16
    assert status(desc(prec=P.BF16), full(d, prec=P.FP16)) == UNSUPPORTED
    base32 = mfa.AttentionDescriptor.make()                         # FP32 query
    assert status(mfa.PagedDecodeDescriptor.make(base32, 2, 8, 1, 128, 1000, Hkv=2),
                  full(d)) == UNSUPPORTED
    # 16-byte alignment of pools, strides and query rows.
    c = full(d)
    c.k_pool = 0x300008
    assert status(d, c) == UNSUPPORTED
    c = full(d)
    c.v_pool = 0x400002
    assert status(d, c) == UNSUPPORTED
    for i in range(3):
        c = full(d)
        c.strides[i] += 4                              # 8 bytes
        assert status(d, c) == UNSUPPORTED, i
    assert status(d, full(d), query=0x100008) == UNSUPPORTED
    assert status(d, full(d), strides=(8 * 128 + 4, 128, 128, 1)) == UNSUPPORTED
    assert status(d, full(d), strides=(128, 16, 1, 8)) == UNSUPPORTED   # d not contiguous
    # The grid: B x H_kv x row tiles.
    big = desc(B=8192, H=8, Hkv=8)
    assert status(big, full(big)) == UNSUPPORTED
    assert names(desc(B=8191, H=8, Hkv=8))             # 65528 units: served
    # Scales and masks.
    assert status(desc(scale=0.0), full(d)) == UNSUPPORTED
    assert status(desc(scale=-1.0), full(d)) == UNSUPPORTED
    assert status(d, full(d, prec=P.INT8, k_scale=0.0)) == UNSUPPORTED
    assert status(d, full(d, prec=P.INT8, k_zero_point=200)) == UNSUPPORTED
    assert status(desc(window=64), full(d)) == UNSUPPORTED
    assert status(desc(sparse_mask=mfa.MaskType.sparseRanges), full(d)) == UNSUPPORTED
    assert status(desc(transpose=(False, True, False, False)), full(d)) == UNSUPPORTED


def test_empty_shapes_succeed_and_launch_nothing():
    for kw in ({"B": 0}, {"R": 0}):
        d = desc(**kw)
        assert status(d, full(desc())) == OK
        c = cache(desc())
        assert status(d, c, query=None, output=None) == OK      # the buffers may be null
        assert mfa.paged_decode_plan(d, cache(desc())) == []


@pytest.fixture(scope="module")
def paged_kernels():
    """Code-object metadata of the paged kernels (harness.code_object_metadata)."""
    return kernels_named("_paged_kernel")


def test_paged_kernels_use_no_scratch_and_fit_the_register_file(paged_kernels):
    # 2 forms x {F16, BF16} x D {64, 128, 256} x {16-bit, INT8}.
    for form in ("mfa_fwd_decode16_paged_kernel", "mfa_fwd_decode_paged_kernel"):
        hits = {n: k for n, k in paged_kernels.items() if form + "I" in n}
        assert len(hits) == 12, (form, sorted(hits))
        for n, k in hits.items():
            assert k["scratch"] == 0 and k["vgpr_spill"] == 0, (n, k)
            assert k["vgpr"] <= 512, (n, k)
