"""CPU tests of the paged prefill over quantised pools (mfa_quantized_paged_prefill_forward /
mfa_quantized_paged_prefill_plan in csrc/mfa_api.cpp; mfa_paged_prefill_kv8_kernel in
attention_prefill_paged_kv8.hip): the symbols, the plans, every host validation rule through the
new entry point, the unchanged 16-bit neighbour and the new kernels' code-object resources.  The
plan query runs the real dispatcher with launches recorded, and a rejected call returns before
anything touches a device, so no GPU is needed.  The GPU twin is test_paged_prefill_kv8_gpu.py."""
import ctypes
import os
import re

import pytest

import mfa_amd as mfa
from harness import kernels_named, paged_cache as cache, paged_cache_full as full

P = mfa.Precision
_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_DESCRIPTOR, UNSUPPORTED, INVALID_ARGUMENT = 0, 1, 2, 4  # mfa_status_t
I8 = dict(prec=P.INT8, k_scale=0.02, v_scale=0.03, k_zero_point=3, v_zero_point=-5)


def desc(B=2, H=8, Hkv=2, R=300, D=128, prec=P.FP16, max_seq_len=1000, **kw):
    base = mfa.AttentionDescriptor.make(low_precision=True, precision=prec, **kw)
    return mfa.PagedPrefillDescriptor.make(base, B, H, R, D, max_seq_len, Hkv=Hkv)


def i8(d, **kw):
    return cache(d, **{**I8, **kw})


def i8_full(d, **kw):
    return full(d, **{**I8, **kw})


def names(p):
    return [r["name"] for r in p]


def test_symbols_are_declared_and_exported():
    for n in ("mfa_quantized_paged_prefill_forward", "mfa_quantized_paged_prefill_plan"):
        assert n in mfa.header_functions()
        assert hasattr(mfa.lib, n)
        assert getattr(mfa.lib, n).argtypes is not None
    assert (mfa.lib.mfa_quantized_paged_prefill_forward.argtypes
            == mfa.lib.mfa_paged_prefill_forward.argtypes)
    assert (mfa.lib.mfa_quantized_paged_prefill_plan.argtypes
            == mfa.lib.mfa_paged_prefill_plan.argtypes)
    assert callable(mfa.quantized_paged_prefill_forward)
    assert '#define MFA_ABI_VERSION 1' in re.sub(r"[ \t]+", " ", open(mfa.HEADER_PATH).read())


def test_int8_pools_launch_the_on_load_kernel():
    for causal in (False, True):
        d = desc(causal=causal)
        p = mfa.quantized_paged_prefill_plan(d, i8(d))
        assert names(p) == ["mfa_paged_prefill_kv8_kernel<F16, 128, 64>"]
        assert "_paged_kernel" not in p[0]["name"] and "mfa_paged_prefill_kernel" not in p[0]["name"]
        assert p[0]["threads"] == 256 and p[0]["lds_bytes"] <= 160 * 1024
        assert p[0]["workgroups"] == 2 * 8 * 3
    d = desc(B=1, H=2, Hkv=2, R=129)
    assert mfa.quantized_paged_prefill_plan(d, i8(d))[0]["workgroups"] == 1 * 2 * 2


@pytest.mark.parametrize("prec,tag", [(P.FP16, "F16"), (P.BF16, "BF16")])
@pytest.mark.parametrize("D,DP,BK", [(64, 64, 64), (80, 128, 64), (128, 128, 64), (192, 256, 32),
                                     (256, 256, 32)])
def test_types_and_head_dims_resolve(prec, tag, D, DP, BK):
    d = desc(D=D, prec=prec)
    p = mfa.quantized_paged_prefill_plan(d, i8(d))
    assert names(p) == [f"mfa_paged_prefill_kv8_kernel<{tag}, {DP}, {BK}>"]
    # K and V rings of two 16-bit tiles each, and one byte slot per operand.
    assert p[0]["lds_bytes"] == 4 * BK * DP * 2 + 2 * BK * DP
    assert 2 * p[0]["lds_bytes"] <= 160 * 1024            # two workgroups per CU


def test_16_bit_or_no_cache_gives_the_siblings_plan():
    for prec in (P.FP16, P.BF16):
        for D in (64, 72, 128, 256):
            d = desc(D=D, prec=prec)
            want = mfa.paged_prefill_plan(d, cache(d))
            assert "mfa_paged_prefill_kernel<" in want[0]["name"]
            assert mfa.quantized_paged_prefill_plan(d, cache(d)) == want
            assert mfa.quantized_paged_prefill_plan(d) == mfa.paged_prefill_plan(d) == want


def test_any_page_size():
    d = desc()
    want = mfa.quantized_paged_prefill_plan(d, i8(d))
    for page in (32, 256, 1024):
        assert mfa.quantized_paged_prefill_plan(d, i8(d, page=page)) == want


def status(d, c, query=0x100000, output=0x200000, strides=None, new_lens=None,
           fn="mfa_quantized_paged_prefill_forward"):
    """The call's status for a call the host must reject (or an empty one): none of these reaches
    a launch, so the stand-in addresses are never used."""
    s = (ctypes.c_int64 * 4)(*strides) if strides else None
    st = getattr(mfa.lib, fn)(ctypes.byref(d) if d is not None else None, query, s, new_lens,
                              ctypes.byref(c) if c is not None else None, output, None, None)
    if st != OK:
        assert mfa.lib.mfa_last_error(), "empty error message"
    return st


@pytest.mark.parametrize("mk", [full, i8_full], ids=["16-bit", "int8"])
def test_null_pointers_are_invalid_arguments(mk):
    d = desc()
    assert status(None, mk(d)) == INVALID_ARGUMENT
    assert status(d, None) == INVALID_ARGUMENT
    assert status(d, mk(d), query=None) == INVALID_ARGUMENT
    assert status(d, mk(d), output=None) == INVALID_ARGUMENT
    for field in ("k_pool", "v_pool", "block_table", "seq_lens"):
        c = mk(d)
        setattr(c, field, None)
        assert status(d, c) == INVALID_ARGUMENT, field
    out = mfa.KernelPlan()
    assert mfa.lib.mfa_quantized_paged_prefill_plan(None, None, ctypes.byref(out)) == INVALID_ARGUMENT
    assert mfa.lib.mfa_quantized_paged_prefill_plan(ctypes.byref(d), None, None) == INVALID_ARGUMENT


@pytest.mark.parametrize("mk", [full, i8_full], ids=["16-bit", "int8"])
def test_bad_shapes_are_invalid_descriptors(mk):
    for kw in ({"H": 0, "Hkv": 0}, {"D": 0}, {"max_seq_len": 0}):
        assert status(desc(**kw), mk(desc())) == INVALID_DESCRIPTOR, kw
    d = desc()
    for field in ("max_pages_per_seq", "num_pages"):
        c = mk(d)
        setattr(c, field, 0)
        assert status(d, c) == INVALID_DESCRIPTOR, field
    d = desc(H=8, Hkv=3)
    assert status(d, mk(d)) == INVALID_DESCRIPTOR


@pytest.mark.parametrize("mk", [full, i8_full], ids=["16-bit", "int8"])
def test_the_siblings_unsupported_calls(mk):
    d = desc()
    for page in (0, 16, 48, 96):                       # not a power of two, or below 32
        c = mk(d)
        c.page_size = page
        assert status(d, c) == UNSUPPORTED, page
    for D in (68, 264, 512):                           # D % 8 (INT8: % 16), D > 256
        dd = desc(D=D)
        assert status(dd, mk(dd)) == UNSUPPORTED, D
    assert status(d, full(d, prec=P.FP32)) == UNSUPPORTED
    assert status(d, full(d, prec=P.BF16)) == UNSUPPORTED          # differs from Q's FP16
    assert status(desc(prec=P.BF16), full(d, prec=P.FP16)) == UNSUPPORTED
    base32 = mfa.AttentionDescriptor.make()                         # FP32 query
    assert status(mfa.PagedPrefillDescriptor.make(base32, 2, 8, 300, 128, 1000, Hkv=2),
                  mk(d)) == UNSUPPORTED
    # 16-byte alignment of pools, strides and query rows.
    c = mk(d)
    c.k_pool = 0x300008
    assert status(d, c) == UNSUPPORTED
    c = mk(d)
    c.v_pool = 0x400002
    assert status(d, c) == UNSUPPORTED
    for i in range(3):
        c = mk(d)
        c.strides[i] += 8 if c.precision == P.INT8 else 4          # 8 bytes
        assert status(d, c) == UNSUPPORTED, i
    c = mk(d)
    c.strides[0] = -c.strides[0]
    assert status(d, c) == UNSUPPORTED
    assert status(d, mk(d), query=0x100008) == UNSUPPORTED
    assert status(d, mk(d), strides=(300 * 128 * 8 + 4, 300 * 128, 128, 1)) == UNSUPPORTED
    assert status(d, mk(d), strides=(128, 16, 1, 8)) == UNSUPPORTED     # d not contiguous
    # Token stride: at least D, below 2^24 bytes.
    c = mk(d)
    c.strides[2] = 64
    assert status(d, c) == UNSUPPORTED
    c = mk(d)
    c.strides[2] = 1 << (24 if c.precision == P.INT8 else 23)
    assert status(d, c) == UNSUPPORTED
    # Rows: B x H x R below 2^31.
    big = desc(B=1 << 12, H=1 << 9, Hkv=1 << 9, R=1 << 10)
    assert status(big, mk(desc(B=1 << 12, H=8, Hkv=2))) == UNSUPPORTED
    # The cap and the table.
    far = desc(max_seq_len=(1 << 30) + 64)
    c = mk(d)
    c.page_size, c.max_pages_per_seq = 1 << 20, 1 << 11
    assert status(far, c) == UNSUPPORTED
    c = mk(d)
    c.max_pages_per_seq = 1 << 30
    assert status(desc(B=4), c) == UNSUPPORTED
    c = mk(d)
    c.num_pages = 0x80000000
    assert status(d, c) == UNSUPPORTED
    # Scales and masks.
    assert status(desc(scale=0.0), mk(d)) == UNSUPPORTED
    assert status(desc(scale=-1.0), mk(d)) == UNSUPPORTED
    assert status(desc(window=64), mk(d)) == UNSUPPORTED
    assert status(desc(causal=True, window=64), mk(d)) == UNSUPPORTED
    assert status(desc(sparse_mask=mfa.MaskType.sparseRanges), mk(d)) == UNSUPPORTED
    assert status(desc(transpose=(False, True, False, False)), mk(d)) == UNSUPPORTED


def test_quantised_pool_rules():
    d = desc()
    assert status(d, full(d, prec=P.INT4)) == UNSUPPORTED
    assert status(d, full(d, prec=P.INT4, k_scale=0.02, v_scale=0.03)) == UNSUPPORTED
    d72 = desc(D=72)                                    # fine for 16-bit pools, D % 16 for INT8
    assert status(d72, i8_full(d72)) == UNSUPPORTED
    assert names(mfa.quantized_paged_prefill_plan(d72, cache(d72))) == \
        ["mfa_paged_prefill_kernel<F16, 128, 64>"]
    for zp in ({"k_zero_point": 200}, {"v_zero_point": 200}, {"k_zero_point": -129}):
        assert status(d, i8_full(d, **zp)) == UNSUPPORTED, zp
    for zp in (-128, 128):                              # the ends of the range are inside it
        assert len(mfa.quantized_paged_prefill_plan(d, i8(d, k_zero_point=zp, v_zero_point=zp))) == 1
    for ks in (0.0, -0.02, float("nan")):
        assert status(d, i8_full(d, k_scale=ks)) == UNSUPPORTED, ks
    # A product that underflows to zero is no scale: 1.44 * (1 / sqrt(128)) * 1e-45.
    assert status(d, i8_full(d, k_scale=1e-45)) == UNSUPPORTED
    # Strides count one-byte elements: 16 more elements are 16 bytes (fine), 8 more are 8 bytes.
    for i in range(3):
        c = i8(d)
        c.strides[i] += 16
        assert len(mfa.quantized_paged_prefill_plan(d, c)) == 1, i
        c = i8_full(d)
        c.strides[i] += 8
        assert status(d, c) == UNSUPPORTED, i
    # ... where the same 16 elements are not 16-byte steps of a 16-bit pool's 8-element rule:
    # 8 more 16-bit elements are 16 bytes and fine there.
    c = cache(d)
    c.strides[1] += 8
    assert len(mfa.quantized_paged_prefill_plan(d, c)) == 1


@pytest.mark.parametrize("mk", [cache, i8], ids=["16-bit", "int8"])
def test_empty_shapes_succeed_and_launch_nothing(mk):
    for kw in ({"B": 0}, {"R": 0}):
        d = desc(**kw)
        c = mk(desc())
        c.k_pool = c.v_pool = c.block_table = c.seq_lens = None
        assert status(d, c, query=None, output=None) == OK   # the buffers may be null
        assert mfa.quantized_paged_prefill_plan(d, mk(desc())) == []
        assert mfa.quantized_paged_prefill_plan(d) == []


def test_the_neighbour_still_rejects_quantised_pools():
    d = desc()
    old = "mfa_paged_prefill_forward"
    assert status(d, i8_full(d), fn=old) == UNSUPPORTED
    assert b"quantised pools" in mfa.lib.mfa_last_error()
    assert status(d, full(d, prec=P.INT4), fn=old) == UNSUPPORTED
    with pytest.raises(Exception):
        mfa.paged_prefill_plan(d, i8(d))
    assert names(mfa.paged_prefill_plan(d, cache(d))) == ["mfa_paged_prefill_kernel<F16, 128, 64>"]


@pytest.fixture(scope="module")
def kernels():
    """Code-object metadata of every kernel whose name has `mfa_paged_prefill` in it
    (harness.code_object_metadata)."""
    return kernels_named("mfa_paged_prefill")


def test_kv8_kernels_use_no_scratch_and_keep_two_workgroups_per_cu(kernels):
    kv8 = {n: k for n, k in kernels.items() if "mfa_paged_prefill_kv8_kernel" in n}
    # {F16, BF16} x D {64, 128, 256}.
    assert len(kv8) == 6, sorted(kv8)
    tags = sorted(re.search(r"kernelINS_(\d\w+?)ELi(\d+)ELi(\d+)", n).groups() for n in kv8)
    assert tags == sorted((t, str(dp), str(bk)) for t in ("3F16", "4BF16")
                          for dp, bk in ((64, 64), (128, 64), (256, 32))), tags
    for n, k in kv8.items():
        assert "_paged_kernel" not in n and "mfa_paged_prefill_kernel" not in n
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0, (n, k)
        # Two workgroups of four waves per CU (launch bounds; 80 KiB of dynamic LDS each): 256
        # registers per lane.  The LDS is dynamic, so the static size in the notes is zero and the
        # plan carries the figure (test_types_and_head_dims_resolve).
        assert k["vgpr"] <= 256, (n, k)
        assert k["lds"] <= 160 * 1024, (n, k)
    # The 16-bit kernels are as many as they were.
    assert sum("mfa_paged_prefill_kernel" in n for n in kernels) == 6, sorted(kernels)
