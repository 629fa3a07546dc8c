"""GPU key census of the forward kernels: one census per kernel family and mask kind.

Inputs from `harness.census_inputs` (Q = 0, Gaussian K, V of small non-zero integers in distinct
rows, FP32 L, default scale) make the set of keys each row attends to observable exactly:
2^L is the number of keys and 2^L * O the sum of their V rows, both small integers that every
type holds exactly.  `harness.assert_census` holds each row to them at 0.25, against
`harness.allowed_keys`; rows with no key must be the oracle's uniform average over all C keys.
tests/test_forward_census.py proves on the CPU which wrong forwards this rejects (every
single-key error: bounds off by one, a dropped or padded key, a dropped tile, wrong GQA or
range indexing).

Every test asserts from the launch log that the intended kernel ran.  Shapes are the smallest
at which each part can go wrong (64-key tiles, 128-row blocks): (R, C) from (200, 200),
(384, 384), (129, 330) and (340, 300); B 2 and H / Hkv 4 / 2, with ranges that differ per batch
and kv head, some empty, some reaching past C, some with x > y.
"""
import numpy as np
import pytest
import torch

import mfa_amd as mfa
import oracle_lib as ol
from harness import (allowed_keys, assert_census, census_inputs, census_ranges, run_forward,
                     to_device)
from test_forward_stream_gpu import env, launched

pytestmark = pytest.mark.gpu
P = mfa.Precision
FP32, FP16, BF16 = P.FP32, P.FP16, P.BF16
DEV = "cuda:0"
B, H, HKV = 2, 4, 2
SHAPES = [(200, 200), (384, 384), (129, 330), (340, 300)]
# The window of the tuned kernels leaves no row without a key (R <= C + W at every shape);
# W_DEAD does (340 > 300 + 24), which only the generic and the big-D kernels and ranges accept.
W, W_DEAD = 50, 24
MASKS = {
    "none": {},
    "causal": {"causal": True},
    "window": {"window": W},
    "ranges": {"ranges": True},
    "causal_ranges": {"causal": True, "ranges": True},
    "window_ranges": {"window": W, "ranges": True},
    "window_dead": {"window": W_DEAD},
    "amask": {"amask": True},
}
GENERIC_MASKS = ["none", "causal", "window_dead", "ranges", "causal_ranges", "window_ranges",
                 "amask"]
TUNED_MASKS = ["none", "causal", "window", "ranges", "causal_ranges", "window_ranges"]


def census(R, C, D, prec, mask, Hq=H, Hkv=HKV, batch=B, ranges=None):
    """One census forward; returns the launched kernel names."""
    kw = dict(MASKS[mask]) if isinstance(mask, str) else dict(mask)
    Q, K, V = census_inputs(batch, Hq, Hkv, R, C, D, seed=R + 3 * C + D)
    ok_extra = None
    if kw.pop("ranges", False) or ranges is not None:
        kw["ranges"] = census_ranges(batch, Hkv, R, C, seed=R + C) if ranges is None else ranges
    if kw.pop("amask", False):
        rng = np.random.default_rng(R + 7 * C)
        am = np.where(rng.random((batch, Hq, R, C)) < 0.4, -1e9, 0.0).astype(np.float32)
        am[..., rng.integers(0, C)] = 0.0     # no row fully masked
        kw["amask"] = am
        ok_extra = am == 0
    mfa.last_launches()
    o, l = run_forward(Q, K, V, prec=prec, low_precision_intermediates=False, **kw)
    names = launched()
    assert l.dtype == torch.float32
    ok = allowed_keys(batch, Hq, Hkv, R, C, kw.get("causal", False), kw.get("window"),
                      kw.get("ranges"))
    if ok_extra is not None:
        ok &= ok_extra
    Ks = K if prec == FP32 else ol.round16(K, "fp16" if prec == FP16 else "bf16")
    ref = ol.attention(Q, Ks, V, **kw)
    assert_census(o, l, ok, V, ref["L"])
    return names


# ------------------------------------------------------------------ the generic kernel
@pytest.mark.parametrize("mask", GENERIC_MASKS)
@pytest.mark.parametrize("R,C", [(340, 300), (129, 330)])
def test_generic_fp32(gpu, R, C, mask):
    names = census(R, C, 64, FP32, mask)
    assert len(names) == 1 and names[0].startswith("mfa_fwd_kernel<"), names


@pytest.mark.parametrize("prec", [FP16, BF16])
@pytest.mark.parametrize("mask", GENERIC_MASKS)
@pytest.mark.parametrize("R,C,D", [(340, 300, 64), (200, 200, 36)])
def test_generic_16bit(gpu, R, C, D, mask, prec):
    with env(MFA_FWD_GEN=1):
        names = census(R, C, D, prec, mask)
    assert len(names) == 1 and names[0].startswith("mfa_fwd_kernel<"), names


@pytest.mark.parametrize("prec", [FP16, BF16])
@pytest.mark.parametrize("mask", ["window_dead", "amask"])
def test_generic_16bit_takes_what_the_tuned_kernel_refuses(gpu, mask, prec):
    # No switch: rows without a key under a window, and additive masks, route here by themselves.
    names = census(340, 300, 128, prec, mask)
    assert len(names) == 1 and names[0].startswith("mfa_fwd_kernel<"), names


# ------------------------------------------------------------------ mfa_fwd2_kernel
# D 256 without ranges: ranges at that width are the generic kernel's (fwd2_eligible).
@pytest.mark.parametrize("prec", [FP16, BF16])
@pytest.mark.parametrize("R,C,D,mask", [(R, C, D, m) for R, C, D in
                                        [(200, 200, 64), (340, 300, 128), (129, 330, 128),
                                         (384, 384, 64), (340, 300, 256)]
                                        for m in TUNED_MASKS if not (D == 256 and "ranges" in m)])
def test_single_block_kernel(gpu, R, C, D, mask, prec):
    # Causal pairs are mirrored by default: MFA_FWD_VARIANT=s keeps the single-block kernel.
    with env(MFA_FWD_VARIANT="s"):
        names = census(R, C, D, prec, mask)
    assert len(names) == 1 and names[0].startswith("mfa_fwd2_kernel<"), names


# ------------------------------------------------------------------ adjacent shared tiles
@pytest.mark.parametrize("prec", [FP16, BF16])
@pytest.mark.parametrize("mask", ["none", "window", "ranges", "window_ranges"])
@pytest.mark.parametrize("R,C,D", [(384, 384, 64), (340, 300, 128), (129, 330, 128)])
def test_adjacent_shared_tiles(gpu, R, C, D, mask, prec):
    with env(MFA_FWD_SHARE=1, MFA_FWD_PIPE=0):
        names = census(R, C, D, prec, mask)
    assert len(names) == 1, names
    if "window" in mask:
        # The switch does not take windows (fwd2_dispatch: adj needs no window): the log shows
        # the single-block kernel, censused here under the same environment.
        assert names[0].startswith("mfa_fwd2_kernel<"), names
    else:
        assert names[0].startswith("mfa_fwd2_share_kernel<") and ", false" in names[0], names


@pytest.mark.parametrize("prec", [FP16, BF16])
def test_adjacent_shared_tiles_disjoint_blocks(gpu, prec):
    """test_sparse_gpu.py's test_block_sparse_shared_disjoint_blocks pattern: the two blocks of
    a pair own disjoint key ranges, with empty and narrowed single rows and an odd block count."""
    Bq, Hq, R, C, D = 2, 2, 5 * 128 + 40, 900, 128
    ranges = np.zeros((Bq, Hq, R, 2), dtype=np.uint32)
    blk = np.arange(R) // 128
    ranges[..., 0] = np.where(blk % 2 == 0, 0, C - 300)[None, None]
    ranges[..., 1] = np.where(blk % 2 == 0, 300, C)[None, None]
    ranges[0, 0, 7::23, 1] = ranges[0, 0, 7::23, 0]            # empty rows
    ranges[1, 1, 11::17, 0] = ranges[1, 1, 11::17, 0] + 90      # narrowed rows
    with env(MFA_FWD_SHARE=1):
        names = census(R, C, D, prec, "none", Hq=Hq, Hkv=Hq, batch=Bq, ranges=ranges)
    assert names[0].startswith("mfa_fwd2_share_kernel<") and ", false" in names[0], names


# ------------------------------------------------------------------ mirrored causal pairs
@pytest.mark.parametrize("prec", [FP16, BF16])
@pytest.mark.parametrize("lean", [True, False])
@pytest.mark.parametrize("order", [0, 64])
@pytest.mark.parametrize("R,C,D", [(200, 200, 128), (384, 384, 128), (129, 330, 64),
                                   (340, 300, 64)])
def test_mirrored_causal_pairs(gpu, R, C, D, order, lean, prec):
    kv = {"MFA_FWD_ORDER": order}
    if not lean:
        kv["MFA_FWD_LEAN"] = 0
    with env(**kv):
        names = census(R, C, D, prec, "causal")
    assert len(names) == 1, names
    if lean:
        assert names[0].startswith("mfa_fwd2_share_kernel<") and \
            names[0].endswith("true, true, true, true>"), names
    else:
        assert names[0].startswith("mfa_fwd2_share_plain_kernel<"), names


@pytest.mark.parametrize("prec", [FP16, BF16])
def test_causal_with_ranges_keeps_the_single_block_kernel(gpu, prec):
    # The default causal route with ranges: the log says mfa_fwd2_kernel, not the mirrored pairs.
    names = census(384, 384, 128, prec, "causal_ranges")
    assert len(names) == 1 and names[0].startswith("mfa_fwd2_kernel<"), names


# ------------------------------------------------------------------ the pair kernel
@pytest.mark.parametrize("prec", [FP16, BF16])
@pytest.mark.parametrize("mask", ["none", "causal", "window"])
@pytest.mark.parametrize("R,C,D", [(200, 200, 128), (340, 300, 64), (129, 330, 128)])
def test_pair_kernel(gpu, R, C, D, mask, prec):
    with env(MFA_FWD_VARIANT="pair", MFA_FWD_PAIR="o"):
        names = census(R, C, D, prec, mask)
    assert len(names) == 1 and names[0].startswith("mfa_fwd2_pair_kernel<"), names


# ------------------------------------------------------------------ stream-split
@pytest.mark.parametrize("prec", [FP16, BF16])
@pytest.mark.parametrize("slow", [False, True])
@pytest.mark.parametrize("D", [64, 128])
def test_stream_split(gpu, D, slow, prec):
    kv = {"MFA_FWD_STREAM": 1, "MFA_FWD_STREAM_WGS": 4}
    if slow:
        kv["MFA_FWD_STREAM_SLOW"] = 1
    with env(**kv):
        names = census(300, 300, D, prec, "causal")
    assert names and names[-1].startswith("mfa_fwd2_stream_kernel<"), names


# ------------------------------------------------------------------ pipe
@pytest.mark.parametrize("R,C", [(384, 384), (340, 300), (129, 330)])
def test_pipe(gpu, R, C):
    # FP16 D 128, no mask: all that kernel accepts (test_forward_pipe_gpu.py).
    with env(MFA_FWD_PIPE=1, MFA_FWD_SHARE=1):
        names = census(R, C, 128, FP16, "none")
    assert names and names[-1].startswith("mfa_fwd_pipe_kernel"), names


# ------------------------------------------------------------------ big D
@pytest.mark.parametrize("prec", [FP16, BF16])
@pytest.mark.parametrize("mask", ["none", "causal", "window_dead", "ranges"])
@pytest.mark.parametrize("R,C", [(129, 330), (340, 300)])
def test_big_d(gpu, R, C, mask, prec):
    names = census(R, C, 320, prec, mask)
    assert len(names) == 1 and names[0].startswith("mfa_fwd_bigd_kernel<"), names


# ------------------------------------------------------------------ 16-bit split-KV decode
DECODE_SHAPES = [
    # B, H, Hkv, R, C, D: rows per kv head, form
    (2, 4, 2, 3, 300, 64),      # 6 rows: the 16-row form
    (2, 4, 4, 1, 777, 128),     # 1 row
    (1, 4, 1, 10, 777, 128),    # 40 rows: the 32-row form, two row tiles
    (1, 2, 2, 40, 300, 64),     # 40 rows of one head
    (2, 2, 2, 8, 1024, 128),    # 32 tiles of 32 keys: two splits and the merge pass
]
DECODE_MASKS = {"none": {}, "causal": {"causal": True}, "window": {"window": 5}}


def decode_ok(shape, mask):
    Bq, Hq, Hkv, R, C, D = shape
    kw = DECODE_MASKS[mask]
    return allowed_keys(Bq, Hq, Hkv, R, C, kw.get("causal", False), kw.get("window"))


@pytest.mark.parametrize("prec", [FP16, BF16])
@pytest.mark.parametrize("merge", [False, True])
@pytest.mark.parametrize("mask", list(DECODE_MASKS))
@pytest.mark.parametrize("shape", DECODE_SHAPES)
def test_decode_kv16(gpu, shape, mask, merge, prec):
    Bq, Hq, Hkv, R, C, D = shape
    kv = {"MFA_DECODE_KV16": 1}
    if merge:
        kv["MFA_DECODE_MERGE"] = 1
    with env(**kv):
        names = census(R, C, D, prec, DECODE_MASKS[mask], Hq=Hq, Hkv=Hkv, batch=Bq)
    form = "mfa_fwd_decode16_kernel<" if (Hq // Hkv) * R <= 16 else "mfa_fwd_decode_kernel<"
    assert names[0].startswith(form) and names[0].endswith(", 0>"), names
    # Causal: only the keys some row sees are read, so the 1024-key case has one split there.
    split = C == 1024 and mask != "causal"
    assert names[1:] == (["mfa_decode_merge_kernel"] if merge or split else []), names


# ------------------------------------------------------------------ quantised split-KV decode
@pytest.mark.parametrize("qp", [FP16, BF16])
@pytest.mark.parametrize("kvp", [P.INT8, P.INT4])
@pytest.mark.parametrize("mask", list(DECODE_MASKS))
@pytest.mark.parametrize("shape", DECODE_SHAPES)
def test_decode_quantised(gpu, shape, mask, kvp, qp):
    """Per-tensor INT8 / INT4 K/V with scale 1.0 and a zero point, built as
    test_quant_gpu.py's test_decode_int4_zero_points builds them: the stored integers are V
    itself, exactly."""
    Bq, Hq, Hkv, R, C, D = shape
    kw = DECODE_MASKS[mask]
    Q, _, V = census_inputs(Bq, Hq, Hkv, R, C, D, seed=R + 3 * C + D)
    rng = np.random.default_rng(C + D)
    kz, vz = 3, -2
    tdev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    if kvp == P.INT4:
        kn = rng.integers(0, 16, (Bq, Hkv, C, D)).astype(np.uint8)
        vn = (V + 8 + vz).astype(np.uint8)
        assert vn.min() >= 0 and vn.max() <= 15
        pack = lambda n: (n.reshape(-1)[0::2] | (n.reshape(-1)[1::2] << 4)).astype(np.uint8)
        kt, vt = tdev(pack(kn)), tdev(pack(vn))
        assert ((vn.astype(np.float32) - 8 - vz) == V).all()
    else:
        kq = rng.integers(-100, 100, (Bq, Hkv, C, D)).astype(np.int8)
        vq = (V + vz).astype(np.int8)
        kt, vt = tdev(kq.view(np.uint8)), tdev(vq.view(np.uint8))
        assert ((vq.astype(np.float32) - vz) == V).all()
    base = mfa.AttentionDescriptor.make(R, C, D, low_precision=True, precision=qp,
                                        low_precision_intermediates=False, **kw)
    desc = mfa.quantized_descriptor(base, qp, kvp, kvp, B=Bq, H=Hq, Hkv=Hkv)
    tq = mfa.quantized_tensor(to_device(Q, qp), qp)
    tk = mfa.quantized_tensor(kt, kvp, scale=1.0, zero_point=kz)
    tv = mfa.quantized_tensor(vt, kvp, scale=1.0, zero_point=vz)
    o = torch.full((Bq, Hq, R, D), float("nan"), dtype=torch.float32, device=DEV)
    l = torch.full((Bq, Hq, R), float("nan"), dtype=torch.float32, device=DEV)
    plan = [r["name"] for r in mfa.quantized_plan(desc, mfa.KernelType.forward, tq, tk, tv)]
    form = "mfa_fwd_decode16_kernel<" if (Hq // Hkv) * R <= 16 else "mfa_fwd_decode_kernel<"
    assert plan[0].startswith(form) and not plan[0].endswith(", 0>"), plan
    mfa.last_launches()
    mfa.QuantizedAttention().forward(desc, tq, tk, tv, o, l)
    torch.cuda.synchronize()
    assert launched() == plan, (launched(), plan)
    assert_census(o, l, decode_ok(shape, mask), V, None)
