"""CPU tests of mfa_paged_mla_rope_prefill_forward / _plan (GPU twin: test_paged_mla_rope_prefill_gpu.py)."""
import inspect
import re

import pytest

import mfa_amd as mfa
from harness import kernels_named
from test_paged_mla_plan import INVALID_ARGUMENT, OK, UNSUPPORTED, P, _ref, cache, desc, full, names
from test_paged_mla_rope_plan import rope


def status(d, c, r, query=0x100000, q_rope=0x130000):   # of a call the host rejects, or of an empty one
    st = mfa.lib.mfa_paged_mla_rope_prefill_forward(_ref(d), query, q_rope, 0x110000, 0x120000, None,
                                                    _ref(c), _ref(r), 0x200000, None, None)
    return st, mfa.lib.mfa_last_error().decode()


def test_symbols_and_signatures():
    text = re.sub(r"\s+", " ", open(mfa.HEADER_PATH).read())
    for n, py in (("mfa_paged_mla_rope_prefill_forward", mfa.paged_mla_rope_prefill_forward),
                  ("mfa_paged_mla_rope_prefill_plan", mfa.paged_mla_rope_prefill_plan)):
        assert n in mfa.header_functions() and hasattr(mfa.lib, n)
        params = re.search(r"mfa_status_t %s\((.*?)\);" % n, text).group(1).split(",")
        assert len(getattr(mfa.lib, n).argtypes) == len(params)
        assert set(inspect.signature(py).parameters) == {p.split()[-1].lstrip("*") for p in params} - {"out"}
    assert "#define MFA_ABI_VERSION 1" in text


@pytest.mark.parametrize("prec,tag", [(P.FP16, "F16"), (P.BF16, "BF16")])
@pytest.mark.parametrize("latent", [256, 512])
def test_three_launch_plan(prec, tag, latent):
    d = desc(B=3, H=16, R=40, latent=latent, prec=prec)
    ref = mfa.paged_mla_prefill_plan(d)      # the no-rope call: the same projection and output GEMM
    for c, r in ((None, None), (cache(d), None), (cache(d, page=32), rope(32, fused=latent, pool=None))):
        p = mfa.paged_mla_rope_prefill_plan(d, c, r)
        assert names(p) == [ref[0]["name"], f"mfa_mla_latent_prefill_rope_kernel<{tag}, {latent}>", ref[2]["name"]]
        assert [x["workgroups"] for x in p] == [x["workgroups"] for x in ref]
        assert (p[1]["workgroups"], p[1]["threads"], p[1]["lds_bytes"]) == (3 * 20, 256, 2 * 32 * latent * 2 + 16384)
    assert mfa.paged_mla_rope_prefill_plan(desc(B=0)) == mfa.paged_mla_rope_prefill_plan(desc(R=0)) == []


def test_status_table_and_precedence():
    d = desc(R=40)
    # Every NULL is INVALID_ARGUMENT, also next to a misaligned buffer; alone, that one is reported.
    for r, kw in ((None, {}), (rope(pool=None), {}), (rope(), {"q_rope": None}),
                  (rope(pool=0x400008), {"q_rope": None}), (rope(), {"query": 0x100008, "q_rope": None})):
        st, msg = status(d, full(d), r, **kw)
        assert st == INVALID_ARGUMENT and "requires" in msg, msg
    for dd, r, kw, part in ((d, rope(), {"q_rope": 0x130008}, "16-byte aligned"),
                            (d, rope(rope_dim=32), {}, "rope dimension 32"),
                            (desc(R=40, window=64), rope(), {}, "masks other than causal"),
                            (desc(B=4096, R=40), rope(), {}, "exceed the grid")):   # B * H = 65536
        st, msg = status(dd, full(dd), r, **kw)
        assert st == UNSUPPORTED and part in msg, (st, msg)
    assert status(None, full(d), rope())[0] == INVALID_ARGUMENT
    assert mfa.lib.mfa_paged_mla_rope_prefill_plan(None, None, None, _ref(mfa.KernelPlan())) == INVALID_ARGUMENT
    assert mfa.lib.mfa_paged_mla_rope_prefill_plan(_ref(d), None, None, None) == INVALID_ARGUMENT
    for dd in (desc(B=0, R=40), desc(R=0)):      # the empty call may take NULL buffers
        assert status(dd, cache(dd), None, query=None, q_rope=None)[0] == OK


def test_kernels_use_no_scratch_and_keep_the_lds():
    ks = kernels_named("mfa_mla_latent_prefill_rope_kernel")
    tags = sorted(re.search(r"kernelINS_(\d\w+?)ELi(\d+)E", n).groups() for n in ks)
    assert tags == sorted((t, str(lat)) for t in ("3F16", "4BF16") for lat in (256, 512)), tags
    for n, k in ks.items():
        assert k["scratch"] == k["vgpr_spill"] == k["sgpr_spill"] == k["lds"] == 0 and k["vgpr"] <= 256, (n, k)


def test_the_neighbours_plans_are_what_they_were():
    row = lambda p: [(x["name"], x["workgroups"], x["lds_bytes"]) for x in p]
    assert row(mfa.paged_mla_prefill_plan(desc(R=40))) == [
        ("mfa_gemm_general_kernel<2, 0>", 128, 0), ("mfa_mla_latent_prefill_kernel<BF16, 512>", 40, 81920),
        ("mfa_gemm_general_kernel<2, 2>", 32, 0)]
    assert row(mfa.paged_mla_rope_decode_plan(desc())) == [
        ("mfa_mla_qproj_kernel<BF16>", 512, 13056), ("mfa_mla_latent_paged_rope_kernel<BF16, 512>", 16, 81920),
        ("mfa_mla_latent_merge_kernel<BF16, 512, 1>", 32, 0)]
