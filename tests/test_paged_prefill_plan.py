"""CPU tests of the paged prefill entry (mfa_paged_prefill_forward / mfa_paged_prefill_plan in
csrc/mfa_api.cpp; mfa_paged_prefill_kernel in attention_prefill_paged.hip): the symbols, the
ctypes mirror, the plans, every host validation rule, the unchanged neighbours and the new
kernels' code-object resources.  The plan query runs the real dispatcher with launches recorded,
and a rejected call returns before anything touches a device, so no GPU is needed.  The GPU twin
is test_paged_prefill_gpu.py."""
import ctypes
import os
import re

import pytest

import mfa_amd as mfa
from harness import kernels_named, paged_cache as cache, paged_cache_full as full

P = mfa.Precision
_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_DESCRIPTOR, UNSUPPORTED, INVALID_ARGUMENT = 0, 1, 2, 4  # mfa_status_t


def desc(B=2, H=8, Hkv=2, R=300, D=128, prec=P.FP16, max_seq_len=1000, **kw):
    base = mfa.AttentionDescriptor.make(low_precision=True, precision=prec, **kw)
    return mfa.PagedPrefillDescriptor.make(base, B, H, R, D, max_seq_len, Hkv=Hkv)


def plan(d, c=None):
    return mfa.paged_prefill_plan(d, cache(d) if c is None else c)


def test_symbols_are_declared_and_exported():
    for n in ("mfa_paged_prefill_forward", "mfa_paged_prefill_plan"):
        assert n in mfa.header_functions()
        assert hasattr(mfa.lib, n)
        assert getattr(mfa.lib, n).argtypes is not None
    assert "mfa_paged_prefill_descriptor_t" in open(mfa.HEADER_PATH).read()
    assert '#define MFA_ABI_VERSION 1' in re.sub(r"[ \t]+", " ", open(mfa.HEADER_PATH).read())


def test_ctypes_mirror_has_the_headers_fields_in_order():
    text = open(mfa.HEADER_PATH).read()
    body = re.search(r"typedef struct mfa_paged_prefill_descriptor \{(.*?)\} mfa_paged_prefill_descriptor_t;",
                     text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    want = {"mfa_attention_descriptor_t": mfa.AttentionDescriptor, "uint32_t": ctypes.c_uint32}
    assert [(n, want[t]) for n, t in fields] == list(mfa.PagedPrefillDescriptor._fields_)
    # The same layout as the decode descriptor (the two calls share a cache and a shape).
    assert ctypes.sizeof(mfa.PagedPrefillDescriptor) == ctypes.sizeof(mfa.PagedDecodeDescriptor)


def test_one_launch_of_128_row_blocks():
    # B2 H8 R300: three 128-row blocks per (batch, head); one kernel, no merge pass.
    for causal in (False, True):
        p = plan(desc(causal=causal))
        assert [r["name"] for r in p] == ["mfa_paged_prefill_kernel<F16, 128, 64>"]
        assert "_paged_kernel" not in p[0]["name"]
        assert p[0]["threads"] == 256 and p[0]["lds_bytes"] <= 160 * 1024
        assert p[0]["workgroups"] == 2 * 8 * 3
    assert plan(desc(B=3, H=4, Hkv=1, R=128))[0]["workgroups"] == 3 * 4 * 1
    assert plan(desc(B=1, H=2, Hkv=2, R=129))[0]["workgroups"] == 1 * 2 * 2
    assert plan(desc(B=1, H=2, Hkv=2, R=1))[0]["workgroups"] == 2


@pytest.mark.parametrize("prec,tag", [(P.FP16, "F16"), (P.BF16, "BF16")])
@pytest.mark.parametrize("D,DP,BK", [(64, 64, 64), (72, 128, 64), (128, 128, 64), (256, 256, 32)])
def test_types_and_head_dims_resolve(prec, tag, D, DP, BK):
    p = plan(desc(D=D, prec=prec))
    assert [r["name"] for r in p] == [f"mfa_paged_prefill_kernel<{tag}, {DP}, {BK}>"]
    assert p[0]["lds_bytes"] == 4 * BK * DP * 2       # K and V rings of two tiles each


def test_plan_without_a_cache_and_any_page_size():
    want = ["mfa_paged_prefill_kernel<F16, 128, 64>"]
    assert [r["name"] for r in mfa.paged_prefill_plan(desc())] == want
    for page in (32, 256, 1024):
        d = desc()
        assert [r["name"] for r in plan(d, cache(d, page=page))] == want


def status(d, c, query=0x100000, output=0x200000, strides=None, new_lens=None):
    """mfa_paged_prefill_forward's status for a call the host must reject (or an empty one): none
    of these reaches a launch, so the stand-in addresses are never used."""
    s = (ctypes.c_int64 * 4)(*strides) if strides else None
    st = mfa.lib.mfa_paged_prefill_forward(ctypes.byref(d) if d is not None else None, query, s,
                                           new_lens, ctypes.byref(c) if c is not None else None,
                                           output, None, None)
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
    assert mfa.lib.mfa_paged_prefill_plan(None, None, ctypes.byref(out)) == INVALID_ARGUMENT
    assert mfa.lib.mfa_paged_prefill_plan(ctypes.byref(d), None, None) == INVALID_ARGUMENT


def test_bad_shapes_are_invalid_descriptors():
    for kw in ({"H": 0, "Hkv": 0}, {"D": 0}, {"max_seq_len": 0}):
        assert status(desc(**kw), full(desc())) == INVALID_DESCRIPTOR, kw
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
    for prec in (P.INT8, P.INT4, P.FP32):              # quantised pools: out of scope
        assert status(d, full(d, prec=prec)) == UNSUPPORTED, prec
    assert status(d, full(d, prec=P.INT8, k_scale=0.02, v_scale=0.03)) == UNSUPPORTED
    assert status(d, full(d, prec=P.BF16)) == UNSUPPORTED          # differs from Q's FP16
    assert status(desc(prec=P.BF16), full(d, prec=P.FP16)) == UNSUPPORTED
    base32 = mfa.AttentionDescriptor.make()                         # FP32 query
    assert status(mfa.PagedPrefillDescriptor.make(base32, 2, 8, 300, 128, 1000, Hkv=2),
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
    c = full(d)
    c.strides[0] = -c.strides[0]
    assert status(d, c) == UNSUPPORTED
    assert status(d, full(d), query=0x100008) == UNSUPPORTED
    assert status(d, full(d), strides=(300 * 128 * 8 + 4, 300 * 128, 128, 1)) == UNSUPPORTED
    assert status(d, full(d), strides=(128, 16, 1, 8)) == UNSUPPORTED   # d not contiguous
    # Token stride: at least D, below 2^24 bytes.
    c = full(d)
    c.strides[2] = 64
    assert status(d, c) == UNSUPPORTED
    c = full(d)
    c.strides[2] = 1 << 23
    assert status(d, c) == UNSUPPORTED
    # Rows: B x H x R below 2^31.
    big = desc(B=1 << 12, H=1 << 9, Hkv=1 << 9, R=1 << 10)
    assert status(big, full(desc(B=1 << 12, H=8, Hkv=2))) == UNSUPPORTED
    # The cap and the table.
    far = desc(max_seq_len=(1 << 30) + 64)
    c = full(d)
    c.page_size, c.max_pages_per_seq = 1 << 20, 1 << 11
    assert status(far, c) == UNSUPPORTED
    c = full(d)
    c.max_pages_per_seq = 1 << 30
    assert status(desc(B=4), c) == UNSUPPORTED
    c = full(d)
    c.num_pages = 0x80000000
    assert status(d, c) == UNSUPPORTED
    # Scales and masks.
    assert status(desc(scale=0.0), full(d)) == UNSUPPORTED
    assert status(desc(scale=-1.0), full(d)) == UNSUPPORTED
    assert status(desc(window=64), full(d)) == UNSUPPORTED
    assert status(desc(causal=True, window=64), full(d)) == UNSUPPORTED
    assert status(desc(sparse_mask=mfa.MaskType.sparseRanges), full(d)) == UNSUPPORTED
    assert status(desc(transpose=(False, True, False, False)), full(d)) == UNSUPPORTED


def test_empty_shapes_succeed_and_launch_nothing():
    for kw in ({"B": 0}, {"R": 0}):
        d = desc(**kw)
        assert status(d, full(desc())) == OK
        assert status(d, cache(desc()), query=None, output=None) == OK   # the buffers may be null
        assert mfa.paged_prefill_plan(d, cache(desc())) == []
        assert mfa.paged_prefill_plan(d) == []


def test_the_neighbours_still_reject_what_they_rejected():
    base = mfa.AttentionDescriptor.make(low_precision=True, precision=P.FP16)
    dd = mfa.PagedDecodeDescriptor.make(base, 2, 8, 1, 128, 1000, Hkv=2)
    c4 = full(desc(), prec=P.INT4)
    assert mfa.lib.mfa_paged_decode_forward(ctypes.byref(dd), 0x100000, None, ctypes.byref(c4),
                                            0x200000, None, None) == UNSUPPORTED
    wbase = mfa.AttentionDescriptor.make(low_precision=True, precision=P.FP16, window=64)
    dw = mfa.PagedDecodeDescriptor.make(wbase, 2, 8, 1, 128, 1000, Hkv=2)
    assert mfa.lib.mfa_paged_decode_forward(ctypes.byref(dw), 0x100000, None,
                                            ctypes.byref(full(desc())), 0x200000, None,
                                            None) == UNSUPPORTED
    da = mfa.PagedAppendDescriptor.make(P.FP16, 2, 2, 4, 128, 1000)
    assert mfa.lib.mfa_paged_kv_append(ctypes.byref(da), 0x100000, 0x200000, None, None, None,
                                       ctypes.byref(c4), None) == UNSUPPORTED
    # ... and plan what they planned: the decode call still takes a many-row chunk.
    d5 = mfa.PagedDecodeDescriptor.make(base, 2, 8, 5, 128, 1000, Hkv=2)
    assert mfa.paged_decode_plan(d5)[0]["name"] == "mfa_fwd_decode_paged_kernel<F16, 128, 0>"


@pytest.fixture(scope="module")
def prefill_kernels():
    """Code-object metadata of the paged prefill kernels (harness.code_object_metadata)."""
    return kernels_named("mfa_paged_prefill_kernel")


def test_prefill_kernels_use_no_scratch_and_fit_the_register_file(prefill_kernels):
    # {F16, BF16} x D {64, 128, 256}.
    assert len(prefill_kernels) == 6, sorted(prefill_kernels)
    tags = sorted(re.search(r"kernelINS_(\d\w+?)ELi(\d+)ELi(\d+)", n).groups() for n in prefill_kernels)
    assert tags == sorted((t, str(dp), str(bk)) for t in ("3F16", "4BF16")
                          for dp, bk in ((64, 64), (128, 64), (256, 32))), tags
    for n, k in prefill_kernels.items():
        assert "_paged_kernel" not in n
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0, (n, k)
        # Two workgroups of four waves per CU (launch bounds): 256 registers per lane.
        assert k["vgpr"] <= 256, (n, k)
