"""CPU tests of the row-wise INT8 paged entries (csrc/mfa_api.cpp): the plans, the host rules the
scales struct adds, the new kernels' resources.  The GPU twin is test_paged_rowwise_gpu.py."""
import ctypes

import pytest

import mfa_amd as mfa
from harness import kernels_named, paged_cache as cache, paged_cache_full as full
from paged_rig import decode_kernel_form, tag

P = mfa.Precision
OK, UNSUPPORTED, INVALID_ARGUMENT = 0, 2, 4  # mfa_status_t


def adesc(B=2, Hkv=2, R=1, D=128, prec=P.FP16):
    return mfa.PagedAppendDescriptor.make(prec, B, Hkv, R, D, 1000)


def ddesc(B=2, H=8, Hkv=2, R=1, D=128, prec=P.FP16, max_seq_len=1000, **kw):
    base = mfa.AttentionDescriptor.make(low_precision=True, precision=prec, **kw)
    return mfa.PagedDecodeDescriptor.make(base, B, H, R, D, max_seq_len, Hkv=Hkv)


def scales(d, page=64, **kw):
    s = mfa.PagedKVScales.make(page, d.num_kv_heads, **kw)
    s.k_scales, s.v_scales = 0x700000, 0x800000
    return s


def status(d, c, s, first=0x100000):
    ref = lambda x: ctypes.byref(x) if x is not None else None
    if isinstance(d, mfa.PagedAppendDescriptor):
        st = mfa.lib.mfa_paged_kv_append_rowwise(ref(d), first, 0x200000, None, None, None, ref(c),
                                                 ref(s), None)
    else:
        st = mfa.lib.mfa_paged_decode_forward_rowwise(ref(d), first, None, ref(c), ref(s),
                                                      0x200000, None, None)
    return st, (mfa.lib.mfa_last_error() or b"").decode()


@pytest.mark.parametrize("prec", [P.FP16, P.BF16])
def test_plans_name_the_rowwise_kernels(prec):
    d = adesc(prec=prec)
    want = [f"mfa_paged_append_rowwise_kernel<{tag(prec)}>"]
    assert [r["name"] for r in mfa.paged_kv_append_rowwise_plan(d, cache(d, prec=P.INT8))] == want
    assert [r["name"] for r in mfa.paged_kv_append_rowwise_plan(d)] == want
    for H, Hkv, R, D in ((8, 2, 1, 128), (8, 2, 4, 64), (8, 2, 5, 128), (32, 4, 2, 256), (4, 4, 1, 256)):
        d = ddesc(H=H, Hkv=Hkv, R=R, D=D, prec=prec, max_seq_len=500)
        form = decode_kernel_form(H, Hkv, R if D < 256 else 17)   # D = 256: always the 32-row form
        form = form.replace("_paged_kernel<", "_paged_rw_kernel<")
        for plan in (mfa.paged_decode_rowwise_plan(d, cache(d, prec=P.INT8)),
                     mfa.paged_decode_rowwise_plan(d)):
            assert [r["name"] for r in plan] == [f"{form}{tag(prec)}, {D}>"], (H, Hkv, R, D)


@pytest.mark.parametrize("d", [adesc(), ddesc()], ids=["append", "decode"])
def test_documented_statuses(d):
    c8 = lambda **kw: full(d, prec=P.INT8, **kw)
    assert status(d, c8(), None, first=None)[0] == INVALID_ARGUMENT
    assert status(d, c8(), None)[0] == INVALID_ARGUMENT                    # no scales struct
    for prec in (P.FP16, P.INT4):
        st, msg = status(d, full(d, prec=prec), scales(d))
        assert st == UNSUPPORTED, (prec, msg)
    for kw in ({"k_zero_point": 3}, {"v_zero_point": -1}):
        st, msg = status(d, c8(**kw), scales(d))
        assert st == UNSUPPORTED and "zero point" in msg, kw
    for strides in ((2 * 64 + 2, 64), (2 * 64, 66), (-128, 64), (2 * 64, 32)):   # misaligned, short
        st, msg = status(d, c8(), scales(d, strides=strides))
        assert st == UNSUPPORTED and "scale" in msg, strides
    s = scales(d)
    s.v_scales += 4
    assert status(d, c8(), s)[0] == UNSUPPORTED
    # Precedence: the cache view's rules first, the scales' stride rule before the null buffers.
    bad = c8()
    bad.page_size = 48
    assert "page size 48" in status(d, bad, scales(d, strides=(130, 64)))[1]
    assert status(d, c8(), scales(d, strides=(130, 64)), first=None)[0] == UNSUPPORTED
    # The cache's own scales are ignored.
    assert status(d, c8(k_scale=0.0, v_scale=-1.0), scales(d), first=None)[0] == INVALID_ARGUMENT


def test_empty_batch_succeeds_with_null_buffers():
    for d in (adesc(B=0), ddesc(B=0)):
        assert status(d, cache(adesc(), prec=P.INT8), None, first=None)[0] == OK
    assert mfa.paged_decode_rowwise_plan(ddesc(B=0)) == []


def test_rowwise_kernels_use_no_scratch():
    # Append {F16, BF16}; decode {F16, BF16} x (32-row D {64, 128, 256} + 16-row D {64, 128}).
    hits = {**kernels_named("mfa_paged_append_rowwise_kernel"), **kernels_named("_paged_rw_kernel")}
    assert len(hits) == 12, sorted(hits)
    for n, k in hits.items():
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, (n, k)
