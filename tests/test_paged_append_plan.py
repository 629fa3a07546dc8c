"""CPU tests of the paged KV-cache append entry (mfa_paged_kv_append / mfa_paged_kv_append_plan
in csrc/mfa_api.cpp; mfa_paged_append_kernel in csrc/paged_append.hip): the symbols, the plan,
every host validation rule and the kernel's code-object resources.  The plan query runs the
real dispatcher with the launch recorded, and a rejected call returns before anything touches a
device, so no GPU is needed.  The GPU twin is test_paged_append_gpu.py."""
import ctypes
import os
import re

import pytest

import mfa_amd as mfa
from harness import kernels_named, paged_cache as cache, paged_cache_full as full

P = mfa.Precision
_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_DESCRIPTOR, UNSUPPORTED, INVALID_ARGUMENT = 0, 1, 2, 4  # mfa_status_t


def desc(B=2, Hkv=2, R=1, D=128, prec=P.FP16, max_seq_len=1000):
    return mfa.PagedAppendDescriptor.make(prec, B, Hkv, R, D, max_seq_len)


def status(d, c, key=0x100000, value=0x200000, kstrides=None, vstrides=None, new_lens=None):
    """mfa_paged_kv_append's status for a call the host must reject (or an empty one): none of
    these reaches a launch, so the stand-in addresses are never used."""
    ks = (ctypes.c_int64 * 4)(*kstrides) if kstrides else None
    vs = (ctypes.c_int64 * 4)(*vstrides) if vstrides else None
    st = mfa.lib.mfa_paged_kv_append(ctypes.byref(d) if d is not None else None, key, value, ks,
                                     vs, new_lens, ctypes.byref(c) if c is not None else None,
                                     None)
    if st != OK:
        assert mfa.lib.mfa_last_error(), "empty error message"
    return st


def test_symbols_are_declared_and_exported():
    for n in ("mfa_paged_kv_append", "mfa_paged_kv_append_plan"):
        assert n in mfa.header_functions()
        assert hasattr(mfa.lib, n)
        assert getattr(mfa.lib, n).argtypes is not None
    text = open(mfa.HEADER_PATH).read()
    assert "mfa_paged_append_descriptor_t" in text
    assert re.search(r"#define\s+MFA_ABI_VERSION\s+1\b", text)
    # The ctypes mirror has the header's fields, in order.
    body = text[text.index("typedef struct mfa_paged_append_descriptor"):
                text.index("} mfa_paged_append_descriptor_t")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in re.findall(r"u?int32_t\s+([^;]+);", body):
        fields += [f.strip() for f in decl.split(",")]
    assert fields == [f[0] for f in mfa.PagedAppendDescriptor._fields_]
    assert ctypes.sizeof(mfa.PagedAppendDescriptor) == 24


@pytest.mark.parametrize("prec,tag", [(P.FP16, "F16"), (P.BF16, "BF16")])
def test_plan_is_one_launch_named_by_input_and_cache_types(prec, tag):
    d = desc(prec=prec)
    plan = mfa.paged_kv_append_plan(d, cache(d))
    assert [r["name"] for r in plan] == [f"mfa_paged_append_kernel<{tag}, 0>"]
    assert plan[0]["threads"] == 256 and plan[0]["lds_bytes"] == 0
    c8 = cache(d, prec=P.INT8, k_scale=0.02, v_scale=0.03, k_zero_point=3, v_zero_point=-5)
    assert [r["name"] for r in mfa.paged_kv_append_plan(d, c8)] == [f"mfa_paged_append_kernel<{tag}, 1>"]
    # A NULL cache plans a 16-bit pool of the input's type.
    assert [r["name"] for r in mfa.paged_kv_append_plan(d)] == [f"mfa_paged_append_kernel<{tag}, 0>"]


def test_grid_stays_below_65536_in_every_dimension():
    # Key and value halves of one launch; B * R rows folded into the first dimension.
    d = desc(B=2, R=1)
    assert mfa.paged_kv_append_plan(d)[0]["workgroups"] == 2
    d = desc(B=3, Hkv=2, R=5, D=72, max_seq_len=64)
    assert mfa.paged_kv_append_plan(d, cache(d, page=32))[0]["workgroups"] == 2 * 4
    d = desc(B=8, Hkv=8, R=8192, max_seq_len=8192)          # a prefill chunk
    wg = mfa.paged_kv_append_plan(d)[0]["workgroups"]
    assert wg % 2 == 0 and 0 < wg // 2 < 65536
    d = desc(B=1 << 15, Hkv=1, R=(1 << 16) - 1, D=64, max_seq_len=1 << 16)   # B * R just below 2^31
    wg = mfa.paged_kv_append_plan(d)[0]["workgroups"]
    assert wg % 2 == 0 and 0 < wg // 2 < 65536


def test_null_pointers_are_invalid_arguments():
    d = desc()
    assert status(None, full(d)) == INVALID_ARGUMENT
    assert status(d, None) == INVALID_ARGUMENT
    assert status(d, full(d), key=None) == INVALID_ARGUMENT
    assert status(d, full(d), value=None) == INVALID_ARGUMENT
    for field in ("k_pool", "v_pool", "block_table", "seq_lens"):
        c = full(d)
        setattr(c, field, None)
        assert status(d, c) == INVALID_ARGUMENT, field
    # new_lens and the strides are optional.  Asked of the plan query, which runs the same checks
    # with both null and records the launch: a real call would start the kernel on the stand-in
    # addresses wherever a GPU is visible.
    assert len(mfa.paged_kv_append_plan(d, full(d))) == 1
    out = mfa.KernelPlan()
    assert mfa.lib.mfa_paged_kv_append_plan(None, None, ctypes.byref(out)) == INVALID_ARGUMENT
    assert mfa.lib.mfa_paged_kv_append_plan(ctypes.byref(d), None, None) == INVALID_ARGUMENT


def test_bad_shapes_are_invalid_descriptors():
    for kw in ({"Hkv": 0}, {"D": 0}, {"max_seq_len": 0}):
        assert status(desc(**kw), full(desc())) == INVALID_DESCRIPTOR, kw
    d = desc()
    for field in ("max_pages_per_seq", "num_pages"):
        c = full(d)
        setattr(c, field, 0)
        assert status(d, c) == INVALID_DESCRIPTOR, field


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
    assert mfa.paged_kv_append_plan(dd, cache(dd))
    assert status(dd, full(dd, prec=P.INT8)) == UNSUPPORTED
    for prec in (P.INT4, P.FP32):                      # INT4 pools: out of scope
        assert status(d, full(d, prec=prec)) == UNSUPPORTED, prec
    assert status(d, full(d, prec=P.BF16)) == UNSUPPORTED          # differs from the input's FP16
    assert status(desc(prec=P.BF16), full(d, prec=P.FP16)) == UNSUPPORTED
    for prec in (P.FP32, P.INT8, P.INT4):              # the new rows are FP16 or BF16
        assert status(desc(prec=prec), full(d, prec=P.INT8)) == UNSUPPORTED, prec
    # 16-byte alignment of the pools and their strides.
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
        c.strides[i] = -c.strides[i]
        assert status(d, c) == UNSUPPORTED, i
    c = full(d)
    c.strides[2] = 64                                  # token stride below D
    assert status(d, c) == UNSUPPORTED
    c = full(d)
    c.strides[2] = 1 << 23                             # 2^24 bytes
    assert status(d, c) == UNSUPPORTED
    # The new rows: d contiguous, strides multiples of 8 elements, 16-byte aligned bases.
    assert status(d, full(d), key=0x100008) == UNSUPPORTED
    assert status(d, full(d), value=0x200004) == UNSUPPORTED
    good = (2 * 128, 128, 128, 1)
    assert status(d, full(d), kstrides=(2 * 128 + 4, 128, 128, 1), vstrides=good) == UNSUPPORTED
    assert status(d, full(d), kstrides=good, vstrides=(2 * 128, 128 + 4, 128, 1)) == UNSUPPORTED
    assert status(d, full(d), kstrides=good, vstrides=(2 * 128, 128, 132, 1)) == UNSUPPORTED
    assert status(d, full(d), kstrides=(128, 16, 1, 8), vstrides=good) == UNSUPPORTED  # d strided
    # Scales (finite, > 0) and zero points ([-128, 128]) of INT8 pools.
    for kw in ({"k_scale": 0.0}, {"v_scale": 0.0}, {"k_scale": -1.0}, {"v_scale": float("inf")},
               {"k_scale": float("nan")}, {"k_zero_point": 200}, {"v_zero_point": -129}):
        assert status(d, full(d, prec=P.INT8, **kw)) == UNSUPPORTED, kw
    assert mfa.paged_kv_append_plan(d, cache(d, prec=P.INT8, k_zero_point=128, v_zero_point=-128))
    # B * R < 2^31, keys per sequence <= 2^30, block table size.
    big = desc(B=1 << 16, R=1 << 15)
    assert status(big, full(big)) == UNSUPPORTED
    far = desc(max_seq_len=(1 << 30) + 1)
    c = full(d, page=1 << 20)
    c.max_pages_per_seq = 1 << 11
    assert status(far, c) == UNSUPPORTED
    c.max_pages_per_seq = 1 << 10                      # the table's span caps it at 2^30: served
    assert status(far, c, key=None) == INVALID_ARGUMENT
    wide = desc(B=1 << 16)
    c = full(d)
    c.max_pages_per_seq = 1 << 15
    assert status(wide, c) == UNSUPPORTED
    c = full(d)
    c.num_pages = 0x80000000
    assert status(d, c) == UNSUPPORTED


def test_empty_shapes_succeed_and_launch_nothing():
    for kw in ({"B": 0}, {"R": 0}):
        d = desc(**kw)
        assert status(d, full(desc())) == OK
        assert status(d, cache(desc()), key=None, value=None) == OK    # the buffers may be null
        assert mfa.paged_kv_append_plan(d, cache(desc())) == []
        assert mfa.paged_kv_append_plan(d) == []


def test_caches_the_reader_accepts_are_accepted():
    # (B, H, Hkv, R, D, precision of Q and input, cache precision, page, max_seq_len, strides)
    shapes = [
        (2, 8, 2, 1, 128, P.FP16, P.FP16, 64, 1000, None),
        (3, 4, 4, 5, 96, P.BF16, P.INT8, 32, 300, None),
        # BSHD-style: one page per sequence over a dense [B, C_alloc, H_kv, D] tensor.
        (2, 4, 2, 1, 128, P.FP16, P.FP16, 1024, 1024, (1024 * 2 * 128, 128, 2 * 128)),
    ]
    for B, H, Hkv, R, D, prec, cprec, page, cap, strides in shapes:
        base = mfa.AttentionDescriptor.make(low_precision=True, precision=prec)
        rd = mfa.PagedDecodeDescriptor.make(base, B, H, R, D, cap, Hkv=Hkv)
        max_pages = -(-cap // page)
        c = mfa.PagedKVCache.make(cprec, page, max_pages, max_pages * B, Hkv, D, strides=strides,
                                  k_scale=0.02, v_scale=0.03, k_zero_point=3, v_zero_point=-5)
        assert mfa.paged_decode_plan(rd, c), (B, H, Hkv, R, D)
        plan = mfa.paged_kv_append_plan(mfa.PagedAppendDescriptor.make(prec, B, Hkv, R, D, cap), c)
        tag = "F16" if prec == P.FP16 else "BF16"
        assert [r["name"] for r in plan] == \
            [f"mfa_paged_append_kernel<{tag}, {1 if cprec == P.INT8 else 0}>"]


@pytest.fixture(scope="module")
def append_kernels():
    """Code-object metadata of the append kernels (harness.code_object_metadata)."""
    return kernels_named("mfa_paged_append_kernel")


def test_append_kernels_use_no_scratch_and_fit_the_register_file(append_kernels):
    # {F16, BF16} x {16-bit, INT8} pools.
    assert len(append_kernels) == 4, sorted(append_kernels)
    for n, k in append_kernels.items():
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, (n, k)
        assert k["lds"] == 0, (n, k)
        # 256-thread workgroups: at most 128 VGPRs keep two of them on a SIMD's register file.
        assert k["vgpr"] <= 128, (n, k)
