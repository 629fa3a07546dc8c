"""CPU tests of the paged MLA entry points (mfa_paged_mla_decode_forward / _plan and
mfa_paged_latent_append / _plan in csrc/mfa_api.cpp; mfa_mla_latent_paged_kernel in
attention_mla_latent.hip): the symbols, the ctypes mirrors, the plans, every host validation
rule with its precedence, the unchanged K/V append plan and the new kernels' code-object
resources.  The plan query runs the real dispatcher with launches recorded, and a rejected call
returns before anything touches a device, so no GPU is needed.  The GPU twin is
test_paged_mla_gpu.py."""
import ctypes
import os
import re

import pytest

import mfa_amd as mfa
from harness import kernels_named

P = mfa.Precision
_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_DESCRIPTOR, UNSUPPORTED, INVALID_ARGUMENT = 0, 1, 2, 4  # mfa_status_t


def desc(B=2, H=16, R=1, D=128, latent=512, max_seq_len=1024, prec=P.BF16, **kw):
    base = mfa.AttentionDescriptor.make(low_precision=True, precision=prec, **kw)
    return mfa.PagedMLADecodeDescriptor.make(base, B, H, R, D, latent, max_seq_len, prec)


def adesc(B=3, R=5, latent=512, max_seq_len=1000, prec=P.BF16):
    return mfa.PagedLatentAppendDescriptor.make(prec, B, R, latent, max_seq_len)


def cache(d, prec=None, page=64, full=False):
    """A PagedLatentCache shaped for the decode or append descriptor d; null pointers (enough for
    a plan query) or, with `full`, aligned stand-ins for calls the host rejects."""
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


def status(d, c, query=0x100000, w_k=0x110000, w_v=0x120000, output=0x200000):
    """mfa_paged_mla_decode_forward's status for a call the host must reject (or an empty one):
    none of these reaches a launch, so the stand-in addresses are never used."""
    st = mfa.lib.mfa_paged_mla_decode_forward(_ref(d), query, w_k, w_v, _ref(c), output, None, None)
    if st != OK:
        assert mfa.lib.mfa_last_error(), "empty error message"
    return st


def astatus(d, c, latent=0x100000, strides=None, new_lens=None):
    s = (ctypes.c_int64 * 2)(*strides) if strides else None
    st = mfa.lib.mfa_paged_latent_append(_ref(d), latent, s, new_lens, _ref(c), None)
    if st != OK:
        assert mfa.lib.mfa_last_error(), "empty error message"
    return st


def test_symbols_are_declared_and_exported():
    for n in ("mfa_paged_mla_decode_forward", "mfa_paged_mla_decode_plan",
              "mfa_paged_latent_append", "mfa_paged_latent_append_plan"):
        assert n in mfa.header_functions()
        assert hasattr(mfa.lib, n)
        assert getattr(mfa.lib, n).argtypes is not None
    assert '#define MFA_ABI_VERSION 1' in re.sub(r"[ \t]+", " ", open(mfa.HEADER_PATH).read())


@pytest.mark.parametrize("struct,mirror", [
    ("mfa_paged_latent_cache", mfa.PagedLatentCache),
    ("mfa_paged_mla_descriptor", mfa.PagedMLADecodeDescriptor),
    ("mfa_paged_latent_append_descriptor", mfa.PagedLatentAppendDescriptor)])
def test_ctypes_mirrors_have_the_headers_fields_in_order(struct, mirror):
    text = open(mfa.HEADER_PATH).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s_t;" % (struct, struct), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    want = {"mfa_attention_descriptor_t": mfa.AttentionDescriptor, "uint32_t": ctypes.c_uint32,
            "int32_t": ctypes.c_int32, "const void*": ctypes.c_void_p,
            "const int32_t*": ctypes.c_void_p}
    fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        m = re.fullmatch(r"int64_t strides\[(\d)\]", decl)
        if m:
            fields.append(("strides", ctypes.c_int64 * int(m.group(1))))
            continue
        ctype, names = decl.rsplit(" ", 1) if "," not in decl else decl.split(" ", 1)
        fields += [(n.strip(), want[ctype]) for n in names.split(",")]
    assert fields == list(mirror._fields_)


# ---------------------------------------------------------------------------- the decode plan
def names(p):
    return [r["name"] for r in p]


def test_three_launches_projection_latent_merge():
    # B2 H16 R1 D128 latent 512, 1024 keys: 2 query blocks, 32 tiles -> 8 splits of 4 tiles.
    d = desc()
    for c in (None, cache(d), cache(d, page=32), cache(d, page=1024)):
        p = mfa.paged_mla_decode_plan(d, c)
        assert names(p) == ["mfa_mla_qproj_kernel<BF16>", "mfa_mla_latent_paged_kernel<BF16, 512>",
                            "mfa_mla_latent_merge_kernel<BF16, 512, 1>"]
        B, H, R, nsplit = 2, 16, 1, 8
        assert p[1]["workgroups"] == -(-H * R // 32) * B * nsplit
        assert p[1]["threads"] == 256 and p[1]["lds_bytes"] == 2 * 32 * 512 * 2 + 16384
        assert p[2]["workgroups"] == B * H * R and p[2]["threads"] == 256


def test_one_split_still_three_launches():
    # cap = 100 keys (< 128): 4 tiles -> tiles / 4 = 1 split; R 5: the general GEMM projects.
    d = desc(R=5, max_seq_len=100, prec=P.FP16, causal=True)
    p = mfa.paged_mla_decode_plan(d, cache(d, page=32))
    assert names(p) == ["mfa_gemm_general_kernel<1, 0>", "mfa_mla_latent_paged_kernel<F16, 512>",
                        "mfa_mla_latent_merge_kernel<F16, 512, 1>"]
    assert p[1]["workgroups"] == -(-16 * 5 // 32) * 2 * 1
    assert p[2]["workgroups"] == 2 * 16 * 5
    # The table span, not max_seq_len, is the cap when it is the smaller one.
    c = cache(desc(max_seq_len=64), page=64)
    assert mfa.paged_mla_decode_plan(desc(), c)[1]["workgroups"] == 2


@pytest.mark.parametrize("prec,tag", [(P.FP16, "F16"), (P.BF16, "BF16")])
@pytest.mark.parametrize("latent", [256, 512])
def test_types_and_latent_dims_resolve(prec, tag, latent):
    p = mfa.paged_mla_decode_plan(desc(latent=latent, prec=prec))
    assert names(p)[1:] == [f"mfa_mla_latent_paged_kernel<{tag}, {latent}>",
                            f"mfa_mla_latent_merge_kernel<{tag}, {latent}, 1>"]
    # A single sequence has no batch to project per head: the general GEMM, as the dense call.
    p1 = mfa.paged_mla_decode_plan(desc(B=1, latent=latent, prec=prec))
    assert p1[0]["name"].startswith("mfa_gemm_general_kernel<") and len(p1) == 3


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
    # Rows, the cap and the table.
    assert status(desc(B=1 << 12, H=1 << 9, R=1 << 10), full(desc(B=1 << 12))) == UNSUPPORTED
    assert status(desc(B=1 << 9, H=1 << 8, R=2), full(desc(B=1 << 9))) == UNSUPPORTED  # B x H grid
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
        assert mfa.paged_mla_decode_plan(d, cache(desc())) == []
        assert mfa.paged_mla_decode_plan(d) == []
    for kw in ({"B": 0}, {"R": 0}):
        a = adesc(**kw)
        assert astatus(a, cache(adesc()), latent=None) == OK
        assert mfa.paged_latent_append_plan(a) == []


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
        assert astatus(adesc(), c) == INVALID_ARGUMENT, field
    assert astatus(adesc(), full(adesc()), latent=None) == INVALID_ARGUMENT
    out = mfa.KernelPlan()
    assert mfa.lib.mfa_paged_mla_decode_plan(None, None, ctypes.byref(out)) == INVALID_ARGUMENT
    assert mfa.lib.mfa_paged_mla_decode_plan(ctypes.byref(d), None, None) == INVALID_ARGUMENT
    assert mfa.lib.mfa_paged_latent_append_plan(None, None, ctypes.byref(out)) == INVALID_ARGUMENT


def _edit(**fields):
    def apply(c):
        for k, v in fields.items():
            setattr(c, k, v)
    return apply


def _stride0_and_no_lens(c):
    c.seq_lens = None
    c.strides[0] += 4


# test_paged_status_precedence.py's order, on calls wrong in two ways:
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


# ------------------------------------------------------------------------------- the append
def test_latent_append_is_one_launch_of_the_append_kernel():
    for prec, tag in ((P.FP16, "F16"), (P.BF16, "BF16")):
        for c in (None, cache(adesc(prec=prec), page=32)):
            p = mfa.paged_latent_append_plan(adesc(prec=prec), c)
            assert names(p) == [f"mfa_paged_append_kernel<{tag}, 0>"]
            assert p[0]["workgroups"] == -(-3 * 5 // 4) * 1 and p[0]["threads"] == 256
    big = adesc(B=1 << 16, R=4)
    assert mfa.paged_latent_append_plan(big)[0]["workgroups"] == 32768
    # The K/V append still launches K and V together: twice the workgroups, the same name.
    kv = mfa.PagedAppendDescriptor.make(P.BF16, 3, 2, 5, 128, 1000)
    p = mfa.paged_kv_append_plan(kv)
    assert names(p) == ["mfa_paged_append_kernel<BF16, 0>"]
    assert p[0]["workgroups"] == -(-3 * 5 // 4) * 2 and p[0]["threads"] == 256
    kv = mfa.PagedAppendDescriptor.make(P.FP16, 1 << 16, 2, 4, 128, 1000)
    assert mfa.paged_kv_append_plan(kv)[0]["workgroups"] == 32768 * 2


def test_latent_append_rules():
    a = adesc()
    assert astatus(a, full(a), strides=(5 * 576 + 4, 576)) == UNSUPPORTED     # not 8 elements
    assert astatus(a, full(a), strides=(5 * 576, -576)) == UNSUPPORTED
    assert astatus(a, full(a), latent=0x100008) == UNSUPPORTED
    assert astatus(adesc(latent=384), full(adesc(latent=384))) == UNSUPPORTED
    assert astatus(a, full(a, prec=P.FP16)) == UNSUPPORTED
    assert astatus(a, full(a, prec=P.INT8)) == UNSUPPORTED
    c = full(a)
    c.page_size = 48
    assert astatus(a, c) == UNSUPPORTED
    c = full(a)
    c.strides[1] = 256
    assert astatus(a, c) == UNSUPPORTED
    assert astatus(adesc(latent=0), full(a)) == INVALID_DESCRIPTOR
    assert astatus(adesc(max_seq_len=0), full(a)) == INVALID_DESCRIPTOR
    assert astatus(adesc(B=1 << 16, R=1 << 15), full(adesc(B=1 << 16))) == UNSUPPORTED
    assert astatus(None, full(a)) == INVALID_ARGUMENT and astatus(a, None) == INVALID_ARGUMENT


# -------------------------------------------------------------------------- code-object notes
@pytest.fixture(scope="module")
def latent_kernels():
    """Code-object metadata of the paged latent kernels (harness.code_object_metadata)."""
    return kernels_named("mfa_mla_latent_paged_kernel")


def test_paged_latent_kernels_use_no_scratch_and_do_not_spill(latent_kernels):
    assert len(latent_kernels) == 4, sorted(latent_kernels)
    tags = sorted(re.search(r"kernelINS_(\d\w+?)ELi(\d+)E", n).groups() for n in latent_kernels)
    assert tags == sorted((t, str(lat)) for t in ("3F16", "4BF16") for lat in (256, 512)), tags
    for n, k in latent_kernels.items():
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, (n, k)
        # Two workgroups of four waves per CU (launch bounds): the unified file's 512 per lane.
        assert k["vgpr"] <= 512, (n, k)
