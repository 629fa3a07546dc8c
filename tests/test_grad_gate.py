"""CPU proof of the 16-bit gradient gate of tests/harness.py (no GPU needed).

The GPU backward tests hold dQ, dK and dV to `GRAD_MARGIN` x the error that
`harness.emulated_backward` (float64 with the roundings the backward contract allows) shows
against the float64 reference on the same inputs.  This file shows that such a gate has teeth:
on every case below, for FP16 and BF16,

* the emulation passes its own gate with half the margin (there is room), and
* every float64 "mutant" of the reference, a backward that is wrong in one plausible way and
  exact otherwise, is rejected: some tensor exceeds TWICE the gate on some metric.

Which metric of `harness.grad_errors` catches which mutant (measured here; "slice" is the
max error of a (b, h) slice over its max |ref|, "row" the per-row L2 error with a 1 % floor):

  mutant          wrong tensors   caught by
  tile            dQ dK dV        slice and row (64 key rows of dK/dV are zero: row error ~1)
  no_D            dQ dK           slice and row (dO has a component along O, so D has weight)
  dP_twice        dQ dK           slice and row
  dQ_unscaled     dQ              slice and row (dQ is 1/scale too large)
  gqa_head        dK dV           slice and row (GQA cases only)
  dK_last_row     dK              row only under a causal mask: the last key row of dK is tiny
                                  there, the slice metric moves by ~1e-2 or less
  dQ_last_row     dQ              slice and row (the slice metric by less under a causal mask)
  causal_off1     dQ dK dV        slice and row, the row metric by far: the first query rows
                                  change most (causal cases only)
  zeros           dQ dK dV        both, error 1

The weakest rejections, as error / gate over every case and both types: dK_last_row 7.2,
no_D 15.9; every other mutant is over 60.

The mutants are written out here in plain numpy, apart from the harness: with no mutant the
same code must reproduce the C oracle, which cross-checks harness.emulated_backward too.
"""
import functools

import numpy as np
import pytest

import mfa_amd as mfa
import oracle_lib as ol
from harness import (GRAD_GATE_CEILING, GRAD_MARGIN, allowed_keys, emulated_backward,
                     grad_errors, gradient_gate, seen)

FP16, BF16 = mfa.Precision.FP16, mfa.Precision.BF16

CASES = {
    # name: B, H, Hkv, R, C, D, causal
    "noncausal_d64": (1, 2, 2, 256, 256, 64, False),
    "cross_d64": (1, 3, 3, 100, 260, 64, False),
    "causal_d128": (1, 2, 2, 300, 300, 128, True),
    "gqa_causal_d128": (1, 4, 2, 190, 190, 128, True),
    "gqa_noncausal_d64": (2, 4, 1, 96, 96, 64, False),
}
MUTANTS = ["tile", "no_D", "dP_twice", "dQ_unscaled", "gqa_head", "dK_last_row", "dQ_last_row",
           "causal_off1", "zeros"]
# Every mutant on every case it can be applied to: dropping a head needs a GQA group (H > Hkv),
# shifting the causal mask needs one.
MUTANT_CASES = [(n, m) for n, c in CASES.items() for m in MUTANTS
                if not (m == "gqa_head" and c[1] == c[2]) and not (m == "causal_off1" and not c[6])]


def gaussian(shape, seed, s=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * s).astype(np.float32)


def mutant_backward(Q, K, V, dO, causal, mutant=None, scale=None):
    """Float64 backward, wrong in the one way `mutant` names (None: the reference itself)."""
    Q, K, V, dO = (np.asarray(x, dtype=np.float64) for x in (Q, K, V, dO))
    B, H, R, D = Q.shape
    Hkv, C = K.shape[1], K.shape[2]
    sc = 1.0 / np.sqrt(D) if scale is None else scale
    i, j = np.arange(R)[:, None], np.arange(C)[None, :]
    keep = (j <= i + (1 if mutant == "causal_off1" else 0)) if causal else np.ones((R, C), bool)
    t0 = 64 if C >= 192 else 0  # the dropped 64-key tile
    dQ, dK, dV = np.zeros((B, H, R, D)), np.zeros((B, Hkv, C, D)), np.zeros((B, Hkv, C, D))
    for b in range(B):
        for h in range(H):
            kv = h % Hkv
            s = np.where(keep, (Q[b, h] @ K[b, kv].T) * sc, -np.inf)
            p = np.exp(s - s.max(axis=1, keepdims=True))
            p /= p.sum(axis=1, keepdims=True)
            dp = dO[b, h] @ V[b, kv].T
            Dr = (dO[b, h] * (p @ V[b, kv])).sum(axis=1, keepdims=True)
            if mutant == "no_D":
                Dr = 0.0 * Dr
            if mutant == "dP_twice":
                dp = dp * sc
            ds = p * (dp - Dr) * sc
            if mutant == "tile":
                p, ds = p.copy(), ds.copy()
                p[:, t0:t0 + 64] = 0.0
                ds[:, t0:t0 + 64] = 0.0
            dQ[b, h] = ds @ K[b, kv]
            if mutant == "gqa_head" and h == H - 1:
                continue
            dK[b, kv] += ds.T @ Q[b, h]
            dV[b, kv] += p.T @ dO[b, h]
    if mutant == "dQ_unscaled":
        dQ /= sc
    if mutant == "dK_last_row":
        dK[:, :, -1] = 0.0
    if mutant == "dQ_last_row":
        dQ[:, :, -1] = 0.0
    if mutant == "zeros":
        dQ, dK, dV = 0 * dQ, 0 * dK, 0 * dV
    return {"dQ": dQ, "dK": dK, "dV": dV}


@functools.lru_cache(maxsize=None)
def case_data(name, prec):
    """Kernel-visible inputs, the oracle's reference and the gate of one case (computed once).
    Without a causal mask dO = noise + 0.5 * O: with independent noise alone D is small next
    to dP*scale there and a backward that drops it loses only a few percent of dQ.  Under a
    causal mask the first rows see few keys and D has weight by itself (row 0: dP*scale = D);
    a component along O = V_0 would make D so large there that its BF16 truncation alone
    costs dK 2e-2, the limit for a well-conditioned case."""
    B, H, Hkv, R, C, D, causal = CASES[name]
    seed = R + C + D
    Q, K, V = gaussian((B, H, R, D), seed, 0.5), gaussian((B, Hkv, C, D), seed + 2, 0.5), \
        gaussian((B, Hkv, C, D), seed + 3, 0.5)
    Qs, Ks, Vs = seen(Q, prec), seen(K, prec), seen(V, prec)
    O = ol.attention(Qs, Ks, Vs, causal=causal)["O"]
    dOs = seen(gaussian((B, H, R, D), seed + 1, 0.5) + (0.0 if causal else 0.5) * O, prec)
    ref = ol.attention(Qs, Ks, Vs, dO=dOs, causal=causal)
    gate = gradient_gate(Qs, Ks, Vs, dOs, prec, ref, causal=causal)
    for a in (Qs, Ks, Vs, dOs, *ref.values()):
        a.setflags(write=False)
    return Qs, Ks, Vs, dOs, ref, gate


def worst_ratio(got, ref, gate):
    """Largest error / gate over dQ, dK, dV and both metrics."""
    return max(e / g for name in ("dQ", "dK", "dV")
               for e, g in zip(grad_errors(got[name], ref[name]), gate[name]))


@pytest.mark.parametrize("prec", [FP16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_emulation_passes_its_gate_with_room(name, prec):
    Qs, Ks, Vs, dOs, ref, gate = case_data(name, prec)
    causal = CASES[name][6]
    emu = emulated_backward(Qs, Ks, Vs, dOs, prec, causal=causal)
    for k in ("dQ", "dK", "dV"):
        print(name, prec, k, "emulation error (slice, row):", grad_errors(emu[k], ref[k]))
    assert worst_ratio(emu, ref, gate) <= 1.0                  # margin 4: by construction
    assert worst_ratio(emu, ref, gate) <= 2.0 / GRAD_MARGIN    # margin 2: there is room
    assert all(max(g) <= GRAD_GATE_CEILING for g in gate.values())
    # The gate's own reference: numpy float64 without any rounding is the C oracle.
    exact = emulated_backward(Qs, Ks, Vs, dOs, None, causal=causal)
    plain = mutant_backward(Qs, Ks, Vs, dOs, causal)
    for k in ("dQ", "dK", "dV"):
        assert max(grad_errors(exact[k], ref[k])) <= 1e-5, k
        assert max(grad_errors(plain[k], ref[k])) <= 1e-5, k


@pytest.mark.parametrize("prec", [FP16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("name,mutant", MUTANT_CASES)
def test_mutant_is_rejected(name, mutant, prec):
    causal = CASES[name][6]
    Qs, Ks, Vs, dOs, ref, gate = case_data(name, prec)
    bad = mutant_backward(Qs, Ks, Vs, dOs, causal, mutant)
    ratio = worst_ratio(bad, ref, gate)
    print(name, mutant, prec, "worst error / gate:", ratio)
    assert ratio > 2.0, f"{mutant} passes on {name}: worst error is {ratio:.2f} x the gate"


def test_metrics_on_known_errors():
    ref = np.zeros((1, 2, 4, 8))
    ref[0, 0] = 1.0
    ref[0, 1] = 10.0
    ref[0, 1, 0] = 0.0          # a row whose true gradient is zero (row 0 of a causal dQ)
    got = ref.copy()
    assert grad_errors(got, ref) == (0.0, 0.0)
    got[0, 0, 2, 3] += 0.5      # slice 0: max |ref| 1, row norm sqrt(8)
    sl, rw = grad_errors(got, ref)
    assert sl == pytest.approx(0.5)
    assert rw == pytest.approx(0.5 / (np.sqrt(8) * 1.01))
    got = ref.copy()
    got[0, 1, 0, 0] = 1.0       # the zero row: finite, measured against the 1 % floor
    sl, rw = grad_errors(got, ref)
    assert sl == pytest.approx(0.1)
    assert rw == pytest.approx(1.0 / (1e-2 * 10 * np.sqrt(8)))
    # rows=...: excluded rows count in neither metric.
    keep = np.array([False, True, True, True])
    assert grad_errors(got, ref, rows=keep) == (0.0, 0.0)


def test_fully_masked_row_exclusion_is_exactly_the_empty_ranges():
    """test_masked_backward_fully_masked_rows_match_generic (FP32 L) leaves the rows with an
    empty key range out of the gate: check here that its mask holds those rows and no other."""
    from test_backward_gpu import fully_masked_ranges_case
    R, C, ranges, empty = fully_masked_ranges_case()
    ok = allowed_keys(1, 2, 2, R, C, ranges=ranges)
    no_key = ~ok.any(axis=3)                      # [B, H, R]
    assert (no_key == empty[None, None, :]).all()
    assert int(empty.sum()) == len(range(5, R, 9)) and 0 < empty.sum() < R // 8
