"""CPU tests of mfa_paged_mla_decode_forward_rowwise / mfa_paged_latent_append_rowwise and their plan
twins by test_paged_mla_rope_plan.py's method: symbols, the ctypes mirror, the plans, the status table
with its precedence, the unchanged status of the 16-bit calls for an INT8 latent cache, and the new
kernels' code-object resources.  GPU twin: test_paged_mla_rowwise_gpu.py."""
import ctypes
import re

import pytest

import mfa_amd as mfa
from harness import kernels_named
from test_paged_mla_plan import (INVALID_ARGUMENT, INVALID_DESCRIPTOR, OK, UNSUPPORTED, P, _ref, adesc,
                                 astatus as astatus16, cache, desc, full, names, status as status16)
from test_paged_mla_rope_plan import rope

NEW = ("mfa_paged_mla_decode_forward_rowwise", "mfa_paged_mla_decode_rowwise_plan",
       "mfa_paged_latent_append_rowwise", "mfa_paged_latent_append_rowwise_plan")


def scales(page=64, pool=0x700000, **fields):
    s = mfa.PagedLatentScales.make(page)
    s.scales = pool
    for k, v in fields.items():
        setattr(s, k, v)
    return s


def status(d, c, s, r=None, query=0x100000, q_rope=None):
    st = mfa.lib.mfa_paged_mla_decode_forward_rowwise(_ref(d), query, q_rope, 0x110000, 0x120000, _ref(c),
                                                      _ref(s), _ref(r), 0x200000, None, None)
    return st, mfa.lib.mfa_last_error().decode()


def astatus(d, c, s, r=None, k_rope=None):
    st = mfa.lib.mfa_paged_latent_append_rowwise(_ref(d), 0x100000, None, k_rope, None, None, _ref(c),
                                                 _ref(s), _ref(r), None)
    return st, mfa.lib.mfa_last_error().decode()


def test_symbols_and_mirror():
    for n in NEW:
        assert n in mfa.header_functions() and getattr(mfa.lib, n).argtypes is not None, n
    body = re.search(r"typedef struct mfa_paged_latent_scales \{(.*?)\}", open(mfa.HEADER_PATH).read(), re.S)
    decls = [" ".join(d.split()) for d in re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S).split(";")]
    assert decls[:2] == ["const float* scales", "int64_t page_stride"]
    assert list(mfa.PagedLatentScales._fields_) == [("scales", ctypes.c_void_p), ("page_stride", ctypes.c_int64)]


@pytest.mark.parametrize("prec,tag", [(P.FP16, "F16"), (P.BF16, "BF16")])
@pytest.mark.parametrize("latent", [256, 512])
def test_plans(prec, tag, latent):
    d, a = desc(latent=latent, prec=prec), adesc(latent=latent, prec=prec)
    ref = mfa.paged_mla_decode_plan(d)
    fused = rope(32, pool=None, strides=(32 * (latent // 2 + 64), latent // 2 + 64))
    for c, ca, s, r, w in ((None, None, None, None, False), (None, None, None, None, True),
                           (cache(d, prec=P.INT8), cache(a, prec=P.INT8), scales(pool=None), None, False),
                           (cache(d, prec=P.INT8, page=32), cache(a, prec=P.INT8, page=32), None, fused, True)):
        p = mfa.paged_mla_decode_rowwise_plan(d, c, s, r, with_rope=w)
        assert names(p) == [ref[0]["name"], f"mfa_mla_latent_paged_rw8_kernel<{tag}, {latent}, {str(w).lower()}>",
                            f"mfa_mla_latent_merge_kernel<{tag}, {latent}, 1>"]
        assert [x["workgroups"] for x in p] == [x["workgroups"] for x in ref]
        assert p[1]["threads"] == 256 and p[1]["lds_bytes"] == 2 * 32 * latent * 2 + 16384
        p = mfa.paged_latent_append_rowwise_plan(a, ca, s, r, with_rope=w)
        assert names(p) == [f"mfa_paged_latent_append_rw8_kernel<{tag}>"]
        assert p[0]["workgroups"] == -(-3 * 5 // 4) and p[0]["threads"] == 256
    assert mfa.paged_mla_decode_rowwise_plan(desc(B=0)) == mfa.paged_latent_append_rowwise_plan(adesc(R=0)) == []


def test_status_table_and_precedence():
    d, a = desc(), adesc()
    c8 = lambda x, **kw: full(x, prec=P.INT8, **kw)
    # A pool that is not INT8; the scale stride; the scale pool's alignment.
    for prec in (P.BF16, P.FP16, P.INT4, P.FP32):
        for st, msg in (status(d, full(d, prec=prec), scales()), astatus(a, full(a, prec=prec), scales())):
            assert st == UNSUPPORTED, (prec, msg)
    assert "INT8 latent pool" in status(d, full(d), scales())[1]
    for edit in ({"page_stride": 32}, {"page_stride": 66}, {"page_stride": -64}, {"pool": 0x700008}):
        for st, msg in (status(d, c8(d), scales(**edit)), astatus(a, c8(a), scales(**edit))):
            assert st == UNSUPPORTED and "scale p" in msg, (edit, msg)
    # NULL scales, a NULL scale pool, rope and q_rope given singly.
    for s, r, x in ((None, None, None), (scales(pool=None), None, None), (scales(), rope(), None),
                    (scales(), None, 0x130000), (scales(), rope(pool=None), 0x130000)):
        for st, msg in (status(d, c8(d), s, r, q_rope=x), astatus(a, c8(a), s, r, k_rope=x)):
            assert st == INVALID_ARGUMENT and "requires" in msg, msg
    assert status(None, c8(d), scales())[0] == astatus(a, None, scales())[0] == INVALID_ARGUMENT
    out = mfa.KernelPlan()
    assert mfa.lib.mfa_paged_mla_decode_rowwise_plan(None, None, None, None, 0, ctypes.byref(out)) == INVALID_ARGUMENT
    assert mfa.lib.mfa_paged_latent_append_rowwise_plan(_ref(a), None, None, _ref(rope()), 0,
                                                        ctypes.byref(out)) == INVALID_ARGUMENT
    # Two faults, the earlier phase's status: cache, scales, rope struct, masks, empty exit, nulls, alignment.
    c48 = c8(d)
    c48.page_size = 48
    for (dd, c, s, r, kw), want, part in (
            ((desc(D=0), c8(d), scales(page_stride=66), None, {}), INVALID_DESCRIPTOR, "empty shape"),
            ((d, c48, scales(page_stride=66), None, {}), UNSUPPORTED, "page size 48"),
            ((d, full(d), scales(page_stride=66), None, {}), UNSUPPORTED, "INT8 latent pool"),
            ((d, c8(d), scales(page_stride=66), rope(rope_dim=32), {}), UNSUPPORTED, "scale page stride"),
            ((desc(window=64), c8(d), scales(), rope(rope_dim=32), {}), UNSUPPORTED, "rope dimension 32"),
            ((desc(B=0), c8(d), scales(page_stride=66), None, {"query": None}), UNSUPPORTED, "scale page stride"),
            ((desc(R=0, window=64), c8(d), None, None, {}), UNSUPPORTED, "masks other than causal"),
            ((d, c8(d), scales(pool=0x700008), None, {"query": None}), INVALID_ARGUMENT, "requires")):
        st, msg = status(dd, c, s, r, **kw)
        assert st == want and part in msg, (st, msg)
    assert status(desc(B=0), cache(d, prec=P.INT8), None, query=None)[0] == OK
    assert astatus(adesc(R=0), cache(a, prec=P.INT8), None)[0] == OK
    # The 16-bit calls keep today's status for an INT8 latent cache.
    assert status16(d, c8(d)) == astatus16(a, c8(a)) == UNSUPPORTED
    assert "quantised pools" in mfa.lib.mfa_last_error().decode()


def test_new_kernels_use_no_scratch_and_do_not_spill():
    dec, app = kernels_named("mfa_mla_latent_paged_rw8_kernel"), kernels_named("mfa_paged_latent_append_rw8_kernel")
    tags = sorted(re.search(r"kernelINS_(\d\w+?)ELi(\d+)ELb(\d)E", n).groups() for n in dec)
    assert tags == sorted((t, str(lat), r) for t in ("3F16", "4BF16") for lat in (256, 512) for r in "01"), tags
    assert len(app) == 2, sorted(app)
    lat = lambda n: re.search(r"ELi(\d+)E", n).group(1)
    base = {lat(n): k for n, k in kernels_named("mfa_mla_latent_paged_kernel").items()}
    for n, k in {**dec, **app}.items():
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, (n, k)
    for n, k in dec.items():   # two workgroups per CU: half the unified file per wave, the 16-bit kernel's LDS
        assert k["vgpr"] <= 256 and k["lds"] == base[lat(n)]["lds"], (n, k)
