"""CPU tests of mfa_paged_mla_rope_decode_forward / _plan and mfa_paged_latent_rope_append / _plan
by test_paged_mla_plan.py's method: symbols, the ctypes mirror, the plans, the rope struct's rules and
their precedence, the rope kernel's code-object resources.  GPU twin: test_paged_mla_rope_gpu.py."""
import ctypes
import re

import pytest

import mfa_amd as mfa
from harness import kernels_named
from test_paged_mla_plan import (INVALID_ARGUMENT, INVALID_DESCRIPTOR, OK, UNSUPPORTED, P, _ref, adesc,
                                 cache, desc, full, names)


def rope(page=64, fused=None, pool=0x400000, **fields):
    r = mfa.PagedRopeCache.make(page, strides=fused and (page * (fused + 64), fused + 64))
    r.pool = pool
    for k, v in fields.items():
        setattr(r, k, (ctypes.c_int64 * 2)(*v) if k == "strides" else v)
    return r


def status(d, c, r, query=0x100000, q_rope=0x130000):
    """(status, message) of a decode call the host must reject, or of an empty one."""
    st = mfa.lib.mfa_paged_mla_rope_decode_forward(_ref(d), query, q_rope, 0x110000, 0x120000, _ref(c),
                                                   _ref(r), 0x200000, None, None)
    return st, mfa.lib.mfa_last_error().decode()


def astatus(d, c, r, k_rope=0x130000, strides=None):
    st = mfa.lib.mfa_paged_latent_rope_append(_ref(d), 0x100000, None, k_rope,
                                              strides and (ctypes.c_int64 * 2)(*strides), None, _ref(c),
                                              _ref(r), None)
    return st, mfa.lib.mfa_last_error().decode()


def test_symbols_and_mirror():
    for n in ("mfa_paged_mla_rope_decode_forward", "mfa_paged_mla_rope_decode_plan",
              "mfa_paged_latent_rope_append", "mfa_paged_latent_rope_append_plan"):
        assert n in mfa.header_functions() and getattr(mfa.lib, n).argtypes is not None
    body = re.search(r"typedef struct mfa_paged_rope_cache \{(.*?)\}", open(mfa.HEADER_PATH).read(), re.S)
    decls = [" ".join(d.split()) for d in re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S).split(";")]
    assert decls[:3] == ["const void* pool", "int64_t strides[2]", "uint32_t rope_dim"]
    assert list(mfa.PagedRopeCache._fields_) == [("pool", ctypes.c_void_p), ("strides", ctypes.c_int64 * 2),
                                                 ("rope_dim", ctypes.c_uint32)]


@pytest.mark.parametrize("prec,tag", [(P.FP16, "F16"), (P.BF16, "BF16")])
@pytest.mark.parametrize("latent", [256, 512])
def test_plans(prec, tag, latent):
    # Decode: the no-rope call's projection, grid and LDS, the rope kernel, the same merge.
    d, a = desc(latent=latent, prec=prec), adesc(latent=latent, prec=prec)
    ref = mfa.paged_mla_decode_plan(d)
    for c, ca, r in ((None, None, None), (cache(d), cache(a), None),
                     (cache(d, page=32), cache(a, page=32), rope(32, fused=latent, pool=None))):
        p = mfa.paged_mla_rope_decode_plan(d, c, r)
        assert names(p) == [ref[0]["name"], f"mfa_mla_latent_paged_rope_kernel<{tag}, {latent}>",
                            f"mfa_mla_latent_merge_kernel<{tag}, {latent}, 1>"]
        assert [x["workgroups"] for x in p] == [x["workgroups"] for x in ref]
        assert p[1]["threads"] == 256 and p[1]["lds_bytes"] == 2 * 32 * latent * 2 + 16384
        p = mfa.paged_latent_rope_append_plan(a, ca, r)
        assert names(p) == ["mfa_paged_rope_append_kernel"]
        assert p[0]["workgroups"] == -(-3 * 5 // 4) and p[0]["threads"] == 256
    assert mfa.paged_latent_rope_append_plan(adesc(B=1 << 16, R=4))[0]["workgroups"] == 32768
    assert mfa.paged_mla_rope_decode_plan(desc(B=0)) == mfa.paged_latent_rope_append_plan(adesc(R=0)) == []


@pytest.mark.parametrize("edit,part", [   # the struct's rules, the same for both calls
    ({"rope_dim": 32}, "rope dimension 32"), ({"rope_dim": 128}, "rope dimension 128"),
    ({"strides": (64 * 64 + 4, 64)}, "rope stride 0"), ({"strides": (64 * 64, 68)}, "rope stride 1"),
    ({"strides": (-4096, 64)}, "rope stride 0"), ({"strides": (4096, 56)}, "rope token stride 56"),
    ({"strides": (1 << 30, 1 << 23)}, "rope token stride"), ({"pool": 0x400008}, "16-byte aligned")])
def test_rope_struct_rules(edit, part):
    for st, msg in (status(desc(), full(desc()), rope(**edit)), astatus(adesc(), full(adesc()), rope(**edit))):
        assert st == UNSUPPORTED and part in msg, (st, msg)


def test_status_table_and_precedence():
    d, a = desc(), adesc()
    for r, x in ((None, 0x130000), (rope(pool=None), 0x130000), (rope(), None)):
        for st, msg in (status(d, full(d), r, q_rope=x), astatus(a, full(a), r, k_rope=x)):
            assert st == INVALID_ARGUMENT and "requires" in msg, msg
    assert status(d, full(d), rope(), q_rope=0x130008)[0] == astatus(a, full(a), rope(), k_rope=0x130008)[0] == UNSUPPORTED
    assert astatus(a, full(a), rope(), strides=(5 * 64 + 4, 64))[0] == UNSUPPORTED
    assert status(None, full(d), rope())[0] == INVALID_ARGUMENT
    out = mfa.KernelPlan()
    assert mfa.lib.mfa_paged_mla_rope_decode_plan(None, None, None, ctypes.byref(out)) == INVALID_ARGUMENT
    assert mfa.lib.mfa_paged_latent_rope_append_plan(_ref(a), None, None, None) == INVALID_ARGUMENT
    # Two faults, the earlier phase's status: cache, rope struct, masks, empty exit, nulls, alignment.
    c48 = full(d)
    c48.page_size = 48
    for (dd, c, r, kw), want, part in (
            ((desc(D=0), full(d), rope(rope_dim=32), {}), INVALID_DESCRIPTOR, "empty shape"),
            ((d, c48, rope(rope_dim=32), {}), UNSUPPORTED, "page size 48"),
            ((desc(window=64), full(d), rope(rope_dim=32), {}), UNSUPPORTED, "rope dimension 32"),
            ((desc(B=0), full(d), rope(rope_dim=32), {"query": None}), UNSUPPORTED, "rope dimension 32"),
            ((desc(R=0, window=64), full(d), None, {}), UNSUPPORTED, "masks other than causal"),
            ((d, full(d), rope(pool=0x400008), {"q_rope": None}), INVALID_ARGUMENT, "requires")):
        st, msg = status(dd, c, r, **kw)
        assert st == want and part in msg, (st, msg)
    assert status(desc(B=0), cache(d), None, query=None, q_rope=None)[0] == OK


def test_rope_kernels_use_no_scratch_and_keep_the_lds():
    ks = kernels_named("mfa_mla_latent_paged_rope_kernel")
    tags = sorted(re.search(r"kernelINS_(\d\w+?)ELi(\d+)E", n).groups() for n in ks)
    assert tags == sorted((t, str(lat)) for t in ("3F16", "4BF16") for lat in (256, 512)), tags
    lat = lambda n: re.search(r"ELi(\d+)E", n).group(1)
    base = {lat(n): k for n, k in kernels_named("mfa_mla_latent_paged_kernel").items()}
    for n, k in ks.items():
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, (n, k)
        # Two workgroups per CU: half the unified file per wave.  Static LDS as the no-rope kernel.
        assert k["vgpr"] <= 256 and k["lds"] == base[lat(n)]["lds"], (n, k)
