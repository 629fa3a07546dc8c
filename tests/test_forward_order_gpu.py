"""GPU parity of the own-tiles-first order of the mirrored causal forward
(attention_fwd_v2.hip fwd2_share_own_first_body): a pair whose light block has at most
MFA_FWD_ORDER key tiles runs the heavy block's own tiles first, parks group 0's partial state
in LDS, runs the shared tiles last and folds the park into group 1's state.

Every shape is checked against the CPU oracle at the tolerances test_forward_v2_gpu.py uses for
this kernel (O 5e-3 fp16 / 1e-2 bf16, L 7e-3 plus half an fp16 ulp of storage), against the same
call with the order off (twice those tolerances: both sit within one of the oracle), and twice
in a row for bit-identical results (the fold's roles are fixed, so nothing depends on timing).

Shapes (causal, H2, 64-key tiles, 128-row blocks): the smallest at which each part can go wrong.
  S 256   one pair, nA 2, one own-tile step per group (no deferred V, A's Q staged in step 0)
  S 512   two pairs; pair 0 has three own steps (deferred V), pair 1 one own tile (group 1 none)
  S 640   an odd middle block, which has no A and stays on the shared-first order
  S 1152  nine blocks at threshold 4: pairs 0, 1 own-first, pairs 2, 3 and the middle block not
  S 500, 1100  ragged last block: edge masks on B's last own tile, guarded O stores of B
  S 1024 bf16, S 512 D 64
  S 512 with spiked keys: the lazy rescale fires in the own-tile steps of both groups and again
          in the shared steps, so the park must carry m and lh exactly
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
TOL_L = 7e-3

# name: (S, D, precision, threshold, spiked)
CASES = {
    "s256": (256, 128, FP16, 64, False),
    "s512": (512, 128, FP16, 64, False),
    "s640_odd_middle": (640, 128, FP16, 64, False),
    "s1152_mixed": (1152, 128, FP16, 4, False),
    "s500_ragged": (500, 128, FP16, 64, False),
    "s1100_ragged": (1100, 128, FP16, 64, False),
    "s1024_bf16": (1024, 128, BF16, 64, False),
    "s512_d64": (512, 64, FP16, 64, False),
    "s512_rescale": (512, 128, FP16, 64, True),
}


def tol_o(prec):
    return 5e-3 if prec == FP16 else 1e-2


def inputs(S, D, spiked):
    rng = np.random.default_rng(1000 + S + D)
    s = 0.3 if spiked else 1.0
    Q, K, V = ((rng.standard_normal((1, 2, S, D)) * (s if i < 2 else 1.0)).astype(np.float32)
               for i in range(3))
    if spiked:
        # test_forward_v2_gpu.py's forced-rescale recipe (keys aligned with every query), with
        # three spikes of growing size placed along the order pair 0 (blocks 0 and 3: nA 2,
        # own tiles 2-4 for group 0 and 5-7 for group 1, then shared tiles 0-1) walks them:
        # key 400 (tile 6, group 1's own steps), key 200 (tile 3, group 0's own steps: the parked
        # max) and key 70 (tile 1, a shared step after the park: group 1's max passes the parked
        # one, A's rows rescale too).  Each step is ~+15 log2 units, past the threshold of 8.
        d = np.ones(D, dtype=np.float32) / np.sqrt(D)
        Q += 4.0 * d
        K[:, :, 400] = 30.0 * d
        K[:, :, 200] = 60.0 * d
        K[:, :, 70] = 90.0 * d
    return Q, K, V


def forward(Q, K, V, prec, order):
    os.environ["MFA_FWD_ORDER"] = str(order)
    try:
        mfa.last_launches()
        o, l = run_forward(Q, K, V, prec=prec, causal=True)
        ran = [r["name"] for r in mfa.last_launches()]
    finally:
        os.environ.pop("MFA_FWD_ORDER", None)
    # The routed mirrored kernel (non-temporal image stores, switch image, deferred V) holds
    # both orders; the plan name does not depend on the order.
    assert len(ran) == 1 and ran[0].startswith("mfa_fwd2_share_kernel<"), ran
    assert ran[0].endswith("true, true, true, true>"), ran
    return o.cpu().numpy(), l.float().cpu().numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def runs(name):
    S, D, prec, thr, spiked = CASES[name]
    Q, K, V = inputs(S, D, spiked)
    ref = ol.attention(seen(Q, prec), seen(K, prec), seen(V, prec), causal=True)
    new = forward(Q, K, V, prec, thr)
    again = forward(Q, K, V, prec, thr)
    off = forward(Q, K, V, prec, 0)
    lr = ref["L"].astype(np.float64)
    half_ulp = 0.5 * np.spacing(np.abs(lr).astype(np.float16)).astype(np.float64)
    return {"ref_o": ref["O"], "ref_l": lr, "half_ulp": half_ulp, "new": new, "again": again,
            "off": off, "prec": prec}


@pytest.mark.parametrize("name", list(CASES))
def test_own_first_vs_oracle(gpu, name):
    r = runs(name)
    o, l = r["new"]
    assert np.isfinite(o).all() and np.isfinite(l).all()
    eo = maxerr(o, r["ref_o"])
    excess = float((np.abs(l - r["ref_l"]) - (TOL_L + r["half_ulp"])).max())
    print(f"{name}: O max error {eo:.3e}, L error over the bound {excess:.3e}")
    assert eo <= tol_o(r["prec"]), f"O max error {eo}"
    assert excess <= 0, f"L error exceeds {TOL_L} + half an fp16 ulp by {excess}"


@pytest.mark.parametrize("name", list(CASES))
def test_own_first_vs_shared_first(gpu, name):
    r = runs(name)
    (o, l), (o0, l0) = r["new"], r["off"]
    # The order off is the oracle-checked kernel of test_forward_v2_gpu.py; it must hold here too.
    assert maxerr(o0, r["ref_o"]) <= tol_o(r["prec"])
    eo = maxerr(o, o0)
    excess = float((np.abs(l - l0) - 2 * (TOL_L + r["half_ulp"])).max())
    print(f"{name}: O difference between the orders {eo:.3e}, L over the bound {excess:.3e}")
    assert eo <= 2 * tol_o(r["prec"])
    assert excess <= 0


@pytest.mark.parametrize("name", list(CASES))
def test_own_first_is_deterministic(gpu, name):
    r = runs(name)
    (o, l), (o2, l2) = r["new"], r["again"]
    assert np.array_equal(o, o2) and np.array_equal(l, l2)


def test_orders_differ_where_expected(gpu):
    # The switch reaches the kernel: summing the tiles in another order rounds differently
    # somewhere (were the outputs identical, the new order would not have run).
    r = runs("s512")
    assert not np.array_equal(r["new"][0], r["off"][0])
