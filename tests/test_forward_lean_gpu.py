"""GPU check of the lean forms of the tuned forward's building blocks (attention_fwd2.h, LN
bits: counted waits in the QK^T / PV chains, IEEE maximum in the row max, partial row sums that
start from their first term, the PV chain's first reads issued before the softmax, one-bound
mask on causal-only tiles).

None of them may change a value, so every case runs twice in one process — the default kernels
and, with MFA_FWD_LEAN=0, the same kernels on the earlier forms (mfa_fwd2_share_plain_kernel /
mfa_fwd2_plain_kernel) — and O and L are compared bit for bit.  Each side is also held to the CPU
oracle at the bounds the other forward tests use for these kernels: O 5e-3, L 7e-3 plus half an
fp16 ulp of L's storage.

The one place the IEEE maximum may differ from fmaxf is the sign of a zero maximum (a tile whose
largest score is +0 in one lane half and -0 in the other); the sign of a zero row max reaches
neither O nor L (it is added to the offset, or multiplied into a value that is only compared and
subtracted), and no case here differs in any bit.

Shapes (H 2, fp16 unless noted; 64-key tiles, 128-row blocks): the smallest at which each touched
part can go wrong.
  S 256 D 128 causal      one mirrored pair: both phases, switch (or park and fold), merge, two
                          diagonal tiles per block
  S 384                   the odd middle block
  S 200                   ragged last block: key-edge mask together with causal in one tile
  S 512, order on / off   own-tiles-first (park, fold) and shared-tiles-first (switch, merge)
  S 256 bf16; S 256 D 64
  S 256 D 256 non-causal  the single-block kernel's AH = 2 read-ahead path
  S 256 spiked            keys 70, 140, 200 aligned with every query, each ~15 log2 units above
                          the last: the lazy rescale fires in the shared and the own-tile steps
                          of both groups, in either order
"""
import functools
import os

import numpy as np
import pytest

import mfa_amd as mfa
import oracle_lib as ol
from harness import maxerr, run_forward, seen

pytestmark = pytest.mark.gpu
FP16, BF16 = mfa.Precision.FP16, mfa.Precision.BF16
TOL_O, TOL_L = 5e-3, 7e-3

# name: (S, D, precision, causal, MFA_FWD_ORDER or None, spiked)
CASES = {
    "s256": (256, 128, FP16, True, None, False),
    "s384_odd_middle": (384, 128, FP16, True, None, False),
    "s200_ragged": (200, 128, FP16, True, None, False),
    "s512_own_first": (512, 128, FP16, True, 64, False),
    "s512_shared_first": (512, 128, FP16, True, 0, False),
    "s256_bf16": (256, 128, BF16, True, None, False),
    "s256_d64": (256, 64, FP16, True, None, False),
    "s256_d256_full": (256, 256, FP16, False, None, False),
    "s256_rescale": (256, 128, FP16, True, None, True),
    "s256_rescale_shared_first": (256, 128, FP16, True, 0, True),
}


def inputs(S, D, spiked):
    rng = np.random.default_rng(2000 + S + D)
    s = 0.3 if spiked else 1.0
    Q, K, V = ((rng.standard_normal((1, 2, S, D)) * (s if i < 2 else 1.0)).astype(np.float32)
               for i in range(3))
    if spiked:
        # test_forward_v2_gpu.py's forced-rescale recipe.  Tiles 0-1 are the pair's shared tiles,
        # tile 2 is group 0's own and tile 3 group 1's: one spike in each kind, growing so that
        # whichever order the tiles run in, a later spike still passes the threshold of 8.
        d = np.ones(D, dtype=np.float32) / np.sqrt(D)
        Q += 4.0 * d
        K[:, :, 70] = 30.0 * d
        K[:, :, 140] = 60.0 * d
        K[:, :, 200] = 90.0 * d
    return Q, K, V


def forward(Q, K, V, prec, causal, order, lean):
    env = {}
    if order is not None:
        env["MFA_FWD_ORDER"] = str(order)
    if not lean:
        env["MFA_FWD_LEAN"] = "0"
    os.environ.update(env)
    try:
        mfa.last_launches()
        o, l = run_forward(Q, K, V, prec=prec, causal=causal)
        ran = [r["name"] for r in mfa.last_launches()]
    finally:
        for k in env:
            os.environ.pop(k, None)
    return o.cpu().numpy(), l.float().cpu().numpy().astype(np.float64), ran


@functools.lru_cache(maxsize=None)
def runs(name):
    S, D, prec, causal, order, spiked = CASES[name]
    Q, K, V = inputs(S, D, spiked)
    ref = ol.attention(seen(Q, prec), seen(K, prec), seen(V, prec), causal=causal)
    lr = ref["L"].astype(np.float64)
    half_ulp = 0.5 * np.spacing(np.abs(lr).astype(np.float16)).astype(np.float64)
    return {"ref_o": ref["O"], "ref_l": lr, "half_ulp": half_ulp,
            "lean": forward(Q, K, V, prec, causal, order, True),
            "plain": forward(Q, K, V, prec, causal, order, False)}


@pytest.mark.parametrize("name", list(CASES))
def test_switch_selects_the_kernels(gpu, name):
    # The comparison below means something only if the two runs are different kernels.
    r = runs(name)
    causal = CASES[name][3]
    lean, plain = r["lean"][2], r["plain"][2]
    assert len(lean) == 1 and len(plain) == 1, (lean, plain)
    if causal:
        assert lean[0].startswith("mfa_fwd2_share_kernel<") and \
            lean[0].endswith("true, true, true, true>"), lean
        assert plain[0].startswith("mfa_fwd2_share_plain_kernel<"), plain
    else:
        assert lean[0].startswith("mfa_fwd2_kernel<"), lean
        assert plain[0].startswith("mfa_fwd2_plain_kernel<"), plain


@pytest.mark.parametrize("name", list(CASES))
def test_lean_is_bit_identical(gpu, name):
    r = runs(name)
    (o, l, _), (o0, l0, _) = r["lean"], r["plain"]
    do = int(np.count_nonzero(o.view(np.uint32) != o0.view(np.uint32)))
    dl = int(np.count_nonzero(l != l0))
    print(f"{name}: O elements that differ {do} of {o.size}, L {dl} of {l.size}")
    assert do == 0 and dl == 0


@pytest.mark.parametrize("side", ["lean", "plain"])
@pytest.mark.parametrize("name", list(CASES))
def test_each_side_vs_oracle(gpu, name, side):
    r = runs(name)
    o, l, _ = r[side]
    assert np.isfinite(o).all() and np.isfinite(l).all()
    eo = maxerr(o, r["ref_o"])
    excess = float((np.abs(l - r["ref_l"]) - (TOL_L + r["half_ulp"])).max())
    print(f"{name} {side}: O max error {eo:.3e}, L error over the bound {excess:.3e}")
    assert eo <= TOL_O, f"O max error {eo}"
    assert excess <= 0, f"L error exceeds {TOL_L} + half an fp16 ulp by {excess}"
