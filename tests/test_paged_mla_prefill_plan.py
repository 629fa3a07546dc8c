"""CPU tests of the paged MLA prefill (mfa_paged_mla_prefill_forward / _plan in csrc/mfa_api.cpp;
mfa_mla_latent_prefill_kernel in attention_mla_latent.hip): the symbols, the plan, every host
validation rule with its precedence (test_paged_mla_plan.py's table on the new call), the
unchanged decode plan and the new kernels' code-object resources.  The plan query runs the real
dispatcher with launches recorded, and a rejected call returns before anything touches a device,
so no GPU is needed.  The GPU twin is test_paged_mla_prefill_gpu.py."""
import ctypes
import os
import re

import pytest

import mfa_amd as mfa
from harness import kernels_named

P = mfa.Precision
_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_DESCRIPTOR, UNSUPPORTED, INVALID_ARGUMENT = 0, 1, 2, 4  # mfa_status_t


def desc(B=2, H=16, R=40, D=128, latent=512, max_seq_len=1024, prec=P.BF16, **kw):
    base = mfa.AttentionDescriptor.make(low_precision=True, precision=prec, **kw)
    return mfa.PagedMLADecodeDescriptor.make(base, B, H, R, D, latent, max_seq_len, prec)


def cache(d, prec=None, page=64, full=False):
    """A PagedLatentCache shaped for the descriptor d; null pointers (enough for a plan query) or,
    with `full`, aligned stand-ins for calls the host rejects."""
    max_pages = -(-d.max_seq_len // page) if page else 1
    c = mfa.PagedLatentCache.make(mfa.Precision(d.precision if prec is None else prec), page,
                                  max_pages, max(1, max_pages * d.batch_size), d.kv_latent_dim)
    if full:
        c.pool, c.block_table, c.seq_lens = 0x300000, 0x500000, 0x600000
    return c


def full(d, **kw):
    return cache(d, full=True, **kw)


def _ref(x):
    return ctypes.byref(x) if x is not None else None


def status(d, c, query=0x100000, w_k=0x110000, w_v=0x120000, output=0x200000, new_lens=None):
    """mfa_paged_mla_prefill_forward's status for a call the host must reject (or an empty one):
    none of these reaches a launch, so the stand-in addresses are never used."""
    st = mfa.lib.mfa_paged_mla_prefill_forward(_ref(d), query, w_k, w_v, new_lens, _ref(c), output,
                                               None, None)
    if st != OK:
        assert mfa.lib.mfa_last_error(), "empty error message"
    return st


def names(p):
    return [r["name"] for r in p]


def test_symbols_are_declared_and_exported():
    for n in ("mfa_paged_mla_prefill_forward", "mfa_paged_mla_prefill_plan"):
        assert n in mfa.header_functions()
        assert hasattr(mfa.lib, n)
        assert getattr(mfa.lib, n).argtypes is not None
    assert callable(mfa.paged_mla_prefill_forward) and callable(mfa.paged_mla_prefill_plan)
    assert '#define MFA_ABI_VERSION 1' in re.sub(r"[ \t]+", " ", open(mfa.HEADER_PATH).read())


# ------------------------------------------------------------------------------------ the plan
GEMM = "mfa_gemm_general_kernel<"


@pytest.mark.parametrize("prec,tag", [(P.FP16, "F16"), (P.BF16, "BF16")])
@pytest.mark.parametrize("latent", [256, 512])
def test_three_launches_projection_latent_projection(prec, tag, latent):
    B, H, R = 3, 16, 40
    d = desc(B=B, H=H, R=R, latent=latent, prec=prec, causal=True)
    plans = [mfa.paged_mla_prefill_plan(d, c)
             for c in (None, cache(d), cache(d, page=32), cache(d, page=256), cache(d, page=1024))]
    for p in plans:
        assert len(p) == 3, names(p)
        assert p[0]["name"].startswith(GEMM) and p[2]["name"].startswith(GEMM), names(p)
        assert p[1]["name"] == f"mfa_mla_latent_prefill_kernel<{tag}, {latent}>"
        assert p[1]["threads"] == 256 and p[1]["workgroups"] == B * -(-H * R // 32)
        assert p[1]["lds_bytes"] == 2 * 32 * latent * 2 + 16384
        assert not any("_merge_kernel" in n or "_paged_kernel" in n for n in names(p)), names(p)
        assert p == plans[0]


@pytest.mark.parametrize("B,R", [(1, 1), (4, 1), (1, 7), (2, 2048)])
def test_every_shape_takes_the_same_route(B, R):
    # Also at R == 1 (where the decode call switches to its projection kernel) and at B == 1.
    d = desc(B=B, R=R, max_seq_len=4096)
    p = mfa.paged_mla_prefill_plan(d)
    assert len(p) == 3 and p[0]["name"].startswith(GEMM) and p[2]["name"].startswith(GEMM)
    assert p[0]["name"] == mfa.paged_mla_prefill_plan(desc(B=3, R=40))[0]["name"]
    assert p[1]["name"] == "mfa_mla_latent_prefill_kernel<BF16, 512>"
    assert p[1]["workgroups"] == B * -(-16 * R // 32)
    # The grid follows the rows, not the cap: there is no key split.
    assert mfa.paged_mla_prefill_plan(desc(B=B, R=R, max_seq_len=1 << 20))[1] == p[1]


def test_the_decode_plan_is_unchanged():
    d = desc(R=1)
    p = mfa.paged_mla_decode_plan(d, cache(d))
    assert names(p) == ["mfa_mla_qproj_kernel<BF16>", "mfa_mla_latent_paged_kernel<BF16, 512>",
                        "mfa_mla_latent_merge_kernel<BF16, 512, 1>"]
    assert p[1]["workgroups"] == 1 * 2 * 8 and p[2]["workgroups"] == 2 * 16
    d = desc(R=5, max_seq_len=100, prec=P.FP16, causal=True)
    p = mfa.paged_mla_decode_plan(d, cache(d, page=32))
    assert names(p) == ["mfa_gemm_general_kernel<1, 0>", "mfa_mla_latent_paged_kernel<F16, 512>",
                        "mfa_mla_latent_merge_kernel<F16, 512, 1>"]
    assert p[1]["workgroups"] == -(-16 * 5 // 32) * 2 and p[2]["workgroups"] == 2 * 16 * 5


# --------------------------------------------------------------------------- the status table
def test_unsupported_calls():
    d = desc()
    for page in (0, 16, 48, 96):
        c = full(d)
        c.page_size = page
        assert status(d, c) == UNSUPPORTED, page
    for latent in (384, 128, 1024):
        dd = desc(latent=latent)
        assert status(dd, full(dd)) == UNSUPPORTED, latent
    assert status(d, full(d, prec=P.FP16)) == UNSUPPORTED          # pool differs from BF16
    assert status(desc(prec=P.FP16), full(d, prec=P.BF16)) == UNSUPPORTED
    for prec in (P.FP32, P.INT8, P.INT4):
        assert status(d, full(d, prec=prec)) == UNSUPPORTED, prec
    d32 = desc()
    d32.precision = int(P.FP32)
    assert status(d32, full(d)) == UNSUPPORTED
    c = full(d)
    c.pool = 0x300008
    assert status(d, c) == UNSUPPORTED
    assert status(d, full(d), query=0x100008) == UNSUPPORTED
    assert status(d, full(d), w_k=0x110002) == UNSUPPORTED
    assert status(d, full(d), w_v=0x120004) == UNSUPPORTED
    for i in range(2):
        c = full(d)
        c.strides[i] += 4                                           # 8 bytes
        assert status(d, c) == UNSUPPORTED, i
    c = full(d)
    c.strides[0] = -c.strides[0]
    assert status(d, c) == UNSUPPORTED
    c = full(d)
    c.strides[1] = 256                                              # token stride < latent
    assert status(d, c) == UNSUPPORTED
    c = full(d)
    c.strides[1] = 1 << 23                                          # 2^24 bytes
    assert status(d, c) == UNSUPPORTED
    for D in (68, 264, 512):
        dd = desc(D=D)
        assert status(dd, full(dd)) == UNSUPPORTED, D
    assert status(desc(window=64), full(d)) == UNSUPPORTED
    assert status(desc(causal=True, window=64), full(d)) == UNSUPPORTED
    assert status(desc(sparse_mask=mfa.MaskType.sparseRanges), full(d)) == UNSUPPORTED
    assert status(desc(transpose=(False, True, False, False)), full(d)) == UNSUPPORTED
    assert status(desc(scale=0.0), full(d)) == UNSUPPORTED
    assert status(desc(scale=-1.0), full(d)) == UNSUPPORTED
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


def test_grid_limits():
    def st(B, H, R):
        return status(desc(B=B, H=H, R=R), full(desc(B=B)))
    msg = lambda: mfa.lib.mfa_last_error().decode()
    assert st(1 << 12, 1 << 9, 1 << 10) == UNSUPPORTED and "too many query rows" in msg()
    # B * H < 65536 for every shape: also at R == 1, where the decode call allows B < 2^21.
    assert st(1 << 9, 1 << 8, 2) == UNSUPPORTED and "(batch, head) pairs" in msg()
    assert st(1 << 12, 16, 1) == UNSUPPORTED and "(batch, head) pairs" in msg()
    d = desc(B=1 << 12, H=16, R=1)
    assert mfa.lib.mfa_paged_mla_decode_forward(_ref(d), None, None, None, _ref(full(d)), None,
                                                None, None) == INVALID_ARGUMENT  # decode: buffers
    # B * ceil(H * R / 32) < 2^31 follows from the two above (B * H * R < 2^31), so the largest
    # grid a passing descriptor plans is below it.
    big = desc(B=4095, H=16, R=1 << 15, max_seq_len=1 << 15)
    p = mfa.paged_mla_prefill_plan(big)
    assert p[1]["workgroups"] == 4095 * (16 << 15) // 32 < 1 << 31


def test_bad_shapes_are_invalid_descriptors():
    for kw in ({"H": 0}, {"latent": 0}, {"D": 0}, {"max_seq_len": 0}):
        assert status(desc(**kw), full(desc())) == INVALID_DESCRIPTOR, kw
    for field in ("max_pages_per_seq", "num_pages"):
        c = full(desc())
        setattr(c, field, 0)
        assert status(desc(), c) == INVALID_DESCRIPTOR, field


def test_empty_shapes_succeed_and_launch_nothing():
    for kw in ({"B": 0}, {"R": 0}):
        d = desc(**kw)
        assert status(d, full(desc())) == OK
        assert status(d, cache(desc()), query=None, w_k=None, w_v=None, output=None) == OK
        assert mfa.paged_mla_prefill_plan(d, cache(desc())) == []
        assert mfa.paged_mla_prefill_plan(d) == []


def test_null_pointers_are_invalid_arguments():
    d = desc()
    assert status(None, full(d)) == INVALID_ARGUMENT
    assert status(d, None) == INVALID_ARGUMENT
    for arg in ("query", "w_k", "w_v", "output"):
        assert status(d, full(d), **{arg: None}) == INVALID_ARGUMENT, arg
    for field in ("pool", "block_table", "seq_lens"):
        c = full(d)
        setattr(c, field, None)
        assert status(d, c) == INVALID_ARGUMENT, field
    out = mfa.KernelPlan()
    assert mfa.lib.mfa_paged_mla_prefill_plan(None, None, ctypes.byref(out)) == INVALID_ARGUMENT
    assert mfa.lib.mfa_paged_mla_prefill_plan(ctypes.byref(d), None, None) == INVALID_ARGUMENT


def _edit(**fields):
    def apply(c):
        for k, v in fields.items():
            setattr(c, k, v)
    return apply


def _stride0_and_no_lens(c):
    c.seq_lens = None
    c.strides[0] += 4


# test_paged_mla_plan.py's table, on calls wrong in two ways:
# (descriptor arguments, cache edit, null descriptor, null query, status, message part)
TWO_FAULTS = [
    ({}, _edit(page_size=48), True, False, INVALID_ARGUMENT, "null descriptor or cache"),
    ({"D": 0}, _edit(page_size=48), False, False, INVALID_DESCRIPTOR, "empty shape"),
    ({"H": 0, "latent": 384}, None, False, False, INVALID_DESCRIPTOR, "empty shape"),
    # An empty call does not excuse a bad cache or descriptor.
    ({"B": 0}, _edit(page_size=48), False, False, UNSUPPORTED, "page size 48"),
    ({"R": 0, "latent": 384}, None, False, False, UNSUPPORTED, "latent dimension 384"),
    ({"R": 0, "window": 64}, None, False, True, UNSUPPORTED, "masks other than causal"),
    ({}, _edit(pool=0x300008), False, True, INVALID_ARGUMENT, "requires"),
    ({}, _stride0_and_no_lens, False, False, UNSUPPORTED, "cache stride 0"),
    ({"D": 264}, _edit(pool=0x300002), False, False, UNSUPPORTED, "head dimension 264"),
]


@pytest.mark.parametrize("case", TWO_FAULTS, ids=[f"{i}-{c[5]}" for i, c in enumerate(TWO_FAULTS)])
def test_two_faults_return_the_earlier_phases_status(case):
    dkw, edit, null_desc, null_query, want, part = case
    d = desc(**dkw)
    c = full(desc())
    if edit:
        edit(c)
    st = status(None if null_desc else d, c, query=None if null_query else 0x100000)
    msg = mfa.lib.mfa_last_error().decode()
    assert st == want, (st, msg)
    assert part in msg, msg
    assert "paged MLA prefill" in msg, msg


# -------------------------------------------------------------------------- code-object notes
@pytest.fixture(scope="module")
def prefill_kernels():
    """Code-object metadata of the latent prefill kernels (harness.code_object_metadata)."""
    return kernels_named("mfa_mla_latent_prefill_kernel")


def test_prefill_kernels_use_no_scratch_and_do_not_spill(prefill_kernels):
    assert len(prefill_kernels) == 4, sorted(prefill_kernels)
    tags = sorted(re.search(r"kernelINS_(\d\w+?)ELi(\d+)E", n).groups() for n in prefill_kernels)
    assert tags == sorted((t, str(lat)) for t in ("3F16", "4BF16") for lat in (256, 512)), tags
    for n, k in prefill_kernels.items():
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, (n, k)
        # __launch_bounds__(256, 2): two workgroups of four waves per CU, 256 registers a lane.
        assert k["vgpr"] <= 256, (n, k)
