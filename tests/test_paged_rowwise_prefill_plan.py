"""CPU tests of the row-wise INT8 paged prefill entry (mfa_paged_prefill_forward_rowwise in
csrc/mfa_api.cpp, attention_prefill_paged_rw8.hip): the plans, the host rules with the row-wise
decode call's precedence, the empty call, the kernels' resources.  The GPU twin is
test_paged_rowwise_prefill_gpu.py."""
import ctypes

import pytest

import mfa_amd as mfa
from harness import kernels_named, paged_cache as cache, paged_cache_full as full
from paged_rig import tag

P = mfa.Precision
OK, UNSUPPORTED, INVALID_ARGUMENT = 0, 2, 4  # mfa_status_t
# D -> (padded D, keys per tile, dynamic LDS: ring + byte slots + two strip slots + raw scale runs)
SHAPES = {D: (DP, BK, 4 * BK * DP * 2 + 2 * BK * DP + 2 * 3 * BK * 4 + 2 * (BK // 32) * 256)
          for D, DP, BK in ((64, 64, 64), (80, 128, 64), (128, 128, 64), (256, 256, 32))}


def desc(B=2, H=8, Hkv=2, R=300, D=128, prec=P.FP16, **kw):
    base = mfa.AttentionDescriptor.make(low_precision=True, precision=prec, **kw)
    return mfa.PagedPrefillDescriptor.make(base, B, H, R, D, 1000, Hkv=Hkv)


def scales(d, page=64, **kw):
    s = mfa.PagedKVScales.make(page, d.num_kv_heads, **kw)
    s.k_scales, s.v_scales = 0x700000, 0x800000
    return s


def status(d, c, s, first=0x100000):
    ref = lambda x: ctypes.byref(x) if x is not None else None
    st = mfa.lib.mfa_paged_prefill_forward_rowwise(ref(d), first, None, None, ref(c), ref(s),
                                                   0x200000, None, None)
    return st, (mfa.lib.mfa_last_error() or b"").decode()


@pytest.mark.parametrize("prec", [P.FP16, P.BF16])
@pytest.mark.parametrize("D", sorted(SHAPES))
def test_plans_name_the_rowwise_kernel(prec, D):
    DP, BK, lds = SHAPES[D]
    for kw, form in (({}, ""), ({"causal": True}, ""), ({"causal_window": 40}, "window_")):
        d = desc(D=D, prec=prec, **kw)
        for plan in (mfa.paged_prefill_rowwise_plan(d, cache(d, prec=P.INT8), scales(d)),
                     mfa.paged_prefill_rowwise_plan(d)):
            assert [r["name"] for r in plan] == \
                [f"mfa_paged_{form}prefill_rw8_kernel<{tag(prec)}, {DP}, {BK}>"], (kw, plan)
            assert plan[0]["threads"] == 256 and plan[0]["workgroups"] == 2 * 8 * 3
            assert plan[0]["lds_bytes"] == lds
    assert (2 * lds <= 160 * 1024) == (D == 64)     # D >= 128: one workgroup per CU


def test_documented_statuses():
    d = desc()
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


def test_empty_call_succeeds_with_null_buffers():
    for d in (desc(B=0), desc(R=0)):
        assert status(d, cache(desc(), prec=P.INT8), None, first=None)[0] == OK
        assert mfa.paged_prefill_rowwise_plan(d) == []


def test_rowwise_prefill_kernels_use_no_scratch():
    hits = kernels_named("prefill_rw8_kernel")    # {plain, window} x {F16, BF16} x D {64, 128, 256}
    assert len(hits) == 12, sorted(hits)
    for n, k in hits.items():
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, (n, k)
        assert k["lds"] == 0, (n, k)      # all dynamic: the plan's lds_bytes is the whole figure
        # One workgroup of four waves per CU leaves 512 registers per lane; two leave 256.
        assert k["vgpr"] <= (256 if "ELi64ELi64E" in n else 512), (n, k)
