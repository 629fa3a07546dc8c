"""CPU proof of the 16-bit forward gate of tests/harness.py (no GPU needed).

The GPU forward tests hold O and L to `FWD_MARGIN` x the error that `harness.emulated_forward`
(float64 with the roundings the forward kernels make) shows against the float64 reference on
the same inputs.  This file shows that such a gate has teeth: on every case below, for FP16
(with and without the tuned kernels' pre-scaled Q) and BF16,

* the emulation passes its own gate with half the margin (there is room), and
* every float64 "mutant" of the reference (test_forward_census.mutant_forward: wrong in one
  plausible way, exact otherwise) exceeds TWICE the gate on some metric, on every case it
  applies to: window, causal and range bounds off by one (each way), the last key dropped,
  one 64-key tile dropped, the wrong GQA map, a scale of 1/sqrt(padded D), and the additive
  mask added after scaling.

Metrics: "slice" is the max error of a (b, h) slice of O over its max |ref|, "row" the per-row
L2 error of O with a 1 % floor (harness.grad_errors), "L" the max abs error of L.

Weakest rejections, as the best error / gate of a mutant on a case, over every case and type
(measured here; test_mutant_is_rejected prints every figure): drop_last_key 8.4 (BF16, 128 x
4096: one key of 4096) and 18 under the causal mask (BF16, row metric, see below), tile 41
(BF16, 128 x 4096), scale_padded 76, range_hi_incl / range_lo_excl 98, window_plus 91,
window_minus 111, gqa_div 274, causal_plus 324, causal_minus 342, mask_after_scale 625.  The
FP16 gates are 6 to 8 times tighter (every FP16 ratio is over 49).

One soft spot: under a causal mask a dropped last key touches the last row alone (200 x 200:
only row 199 attends to key 199).  The slice metric scales that one row's error by the largest
entry of the whole slice and can miss it on other inputs (here 48 FP16 and 4.7 BF16; 2.8 and
0.7 were seen on another draw), and L moves by 1.5 gates.  The row metric sees it (142 FP16,
18 BF16), so that pair is required to exceed twice the gate on the ROW metric.

Not rejected by this gate, and not required to be: `padded_key`, the zero-padded key C counted
in the row sum (score 0, V 0).  Its error sits inside BF16 rounding itself: error / gate is 0.02
to 2.6 for BF16 over the cases below and 0.1 to 12 for FP16 (0 under the causal mask, where no
row reaches key C; test_padded_key_is_inside_the_rounding prints them).  The key census rejects
it exactly: test_forward_census.py::test_mutant_fails_the_census[*-padded_key].
"""
import functools

import numpy as np
import pytest

import mfa_amd as mfa
import oracle_lib as ol
from harness import (FWD_GATE_CEILING, FWD_MARGIN, emulated_forward, forward_errors,
                     forward_gate, seen)
from test_forward_census import mutant_forward, padded_d

FP16, BF16 = mfa.Precision.FP16, mfa.Precision.BF16

CASES = {
    # name: B, H, Hkv, R, C, D, mask kind
    "window64_257": (1, 2, 2, 257, 257, 64, "window"),
    "causal_200_d128": (1, 2, 2, 200, 200, 128, "causal"),
    "ranges_gqa_300": (2, 4, 2, 300, 300, 64, "ranges"),
    "cross_100x300_d80_gqa": (2, 4, 2, 100, 300, 80, None),
    "amask_90x140": (2, 2, 2, 90, 140, 64, "amask"),
    "long_128x4096_d128": (1, 1, 1, 128, 4096, 128, None),
}
# type id: (precision, pre-scaled Q)
TYPES = {"fp16": (FP16, False), "fp16_prescaled": (FP16, True), "bf16": (BF16, False)}
TYPE_CASES = [(n, t) for n, c in CASES.items() for t in TYPES
              if not (t == "fp16_prescaled" and c[6] == "amask")]
BY_KIND = {"window": ["window_plus", "window_minus"], "causal": ["causal_plus", "causal_minus"],
           "ranges": ["range_hi_incl", "range_lo_excl"], "amask": ["mask_after_scale"]}


def mutants_of(case):
    B, H, Hkv, R, C, D, kind = CASES[case]
    m = ["drop_last_key", "tile"] + BY_KIND.get(kind, [])
    if H != Hkv:
        m.append("gqa_div")
    if padded_d(D) != D:
        m.append("scale_padded")
    return m


MUTANT_CASES = [(n, t, m) for n, t in TYPE_CASES for m in mutants_of(n)]


def gaussian(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case_data(name, prec):
    """Kernel-visible inputs, mask arguments and the oracle's reference (computed once)."""
    B, H, Hkv, R, C, D, kind = CASES[name]
    seed = R + C + D
    Qs, Ks, Vs = (seen(gaussian(s, seed + i), prec) for i, s in
                  enumerate([(B, H, R, D), (B, Hkv, C, D), (B, Hkv, C, D)]))
    kw = {}
    if kind == "window":
        kw["window"] = 64
    if kind == "causal":
        kw["causal"] = True
    if kind == "ranges":
        rng = np.random.default_rng(seed + 5)
        lo = rng.integers(0, C - 60, (B, Hkv, R))
        kw["ranges"] = np.stack([lo, lo + rng.integers(20, 100, (B, Hkv, R))], -1).astype(np.uint32)
    if kind == "amask":
        am = (np.random.default_rng(seed + 6).standard_normal((B, H, R, C)) * 3).astype(np.float32)
        am[:, :, :, ::5] = -1e9
        kw["amask"] = am
    ref = ol.attention(Qs, Ks, Vs, **kw)
    for a in (Qs, Ks, Vs, ref["O"], ref["L"]):
        a.setflags(write=False)
    return Qs, Ks, Vs, kw, ref


@functools.lru_cache(maxsize=None)
def gate_of(name, tid):
    prec, pre = TYPES[tid]
    Qs, Ks, Vs, kw, ref = case_data(name, prec)
    return forward_gate(Qs, Ks, Vs, prec, ref, prescaled_q=pre, **kw)


def ratios(got, ref, gate):
    """error / gate for (slice, row, L)."""
    return tuple(e / g for e, g in zip(forward_errors(got, ref), gate))


@pytest.mark.parametrize("name,tid", TYPE_CASES)
def test_emulation_passes_its_gate_with_room(name, tid):
    prec, pre = TYPES[tid]
    Qs, Ks, Vs, kw, ref = case_data(name, prec)
    gate = gate_of(name, tid)
    emu = emulated_forward(Qs, Ks, Vs, prec, prescaled_q=pre, **kw)
    err = forward_errors(emu, ref)
    print(f"{name} {tid}: emulation error (slice, row, L) {err[0]:.3e} {err[1]:.3e} {err[2]:.3e} "
          f"gate {gate[0]:.3e} {gate[1]:.3e} {gate[2]:.3e}")
    assert max(ratios(emu, ref, gate)) <= 2.0 / FWD_MARGIN       # margin 2: there is room
    assert max(gate[:2]) <= FWD_GATE_CEILING
    # The gate's own reference: float64 without any rounding is the C oracle (FP32 outputs).
    for exact in (emulated_forward(Qs, Ks, Vs, None, low_precision_intermediates=False, **kw),
                  mutant_forward(Qs, Ks, Vs, **kw)):
        e = forward_errors(exact, ref)
        assert max(e[:2]) <= 1e-5 and e[2] <= 1e-5, e


@pytest.mark.parametrize("name,tid,mutant", MUTANT_CASES)
def test_mutant_is_rejected(name, tid, mutant):
    prec, _ = TYPES[tid]
    Qs, Ks, Vs, kw, ref = case_data(name, prec)
    bad = mutant_forward(Qs, Ks, Vs, mutant=mutant, **kw)
    r = ratios(bad, ref, gate_of(name, tid))
    print(f"{name} {tid} {mutant}: error / gate slice {r[0]:.2f} row {r[1]:.2f} L {r[2]:.2f}")
    if mutant == "drop_last_key" and CASES[name][6] == "causal":
        assert r[1] > 2.0, f"{mutant} passes the row metric on {name}: {r[1]:.2f} x the gate"
    else:
        assert max(r) > 2.0, f"{mutant} passes on {name}: worst error is {max(r):.2f} x the gate"


@pytest.mark.parametrize("name,tid", TYPE_CASES)
def test_padded_key_is_inside_the_rounding(name, tid):
    """Recorded, not required: the padded key's error against this gate (see the docstring)."""
    prec, _ = TYPES[tid]
    Qs, Ks, Vs, kw, ref = case_data(name, prec)
    bad = mutant_forward(Qs, Ks, Vs, mutant="padded_key", **kw)
    r = ratios(bad, ref, gate_of(name, tid))
    print(f"{name} {tid} padded_key: error / gate slice {r[0]:.2f} row {r[1]:.2f} L {r[2]:.2f}")
    assert np.isfinite(r).all()


def test_prescaling_is_modelled_only_where_the_kernels_do_it():
    Qs, Ks, Vs, kw, ref = case_data("causal_200_d128", FP16)
    plain = emulated_forward(Qs, Ks, Vs, FP16, **kw)
    pre = emulated_forward(Qs, Ks, Vs, FP16, prescaled_q=True, **kw)
    assert np.abs(plain["O"] - pre["O"]).max() > 0
    # BF16 and padded widths over 128 are never pre-scaled, whatever the caller asks.
    Qb, Kb, Vb, kwb, _ = case_data("causal_200_d128", BF16)
    a = emulated_forward(Qb, Kb, Vb, BF16, **kwb)
    b = emulated_forward(Qb, Kb, Vb, BF16, prescaled_q=True, **kwb)
    assert np.array_equal(a["O"], b["O"]) and np.array_equal(a["L"], b["L"])
