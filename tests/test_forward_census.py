"""CPU proof of the forward key census of tests/harness.py (no GPU needed).

The census feeds a forward Q = 0, Gaussian K and a V of small non-zero integers in pairwise
distinct rows (`harness.census_inputs`).  Every unmasked score is then exactly 0, so a correct
forward returns 2^L = n, the number of keys a row attends to, and n * O = the sum of those keys'
V rows, both exact small integers; `harness.assert_census` holds them to 0.25.  This file shows

* that the C oracle passes the census on every mask kind the GPU tests use
  (|2^L - n| and |n*O - sum V| stay four orders of magnitude inside the bound), and that
  `harness.allowed_keys` and the oracle agree on which rows have no key at all;
* that every float64 "mutant" forward below, wrong in one plausible way and exact otherwise,
  fails the census on every mask kind it applies to.

  mutant                 what is wrong
  drop_last_key          key C-1 is never attended to
  padded_key             the zero-padded key C (score 0, V 0) is counted in the row sum
  causal_plus / _minus   key <= row + 1 / key < row instead of key <= row
  window_plus / _minus   row <= key + W + 1 / row <= key + W - 1
  range_hi_incl          x <= key <= y instead of x <= key < y
  range_lo_excl          x < key < y
  ranges_by_query_head   the ranges of (b, h) read where those of (b, h % Hkv) belong
  gqa_div                kv head h // (H / Hkv) instead of h % Hkv
  ranges_batch0          batch 1 reads the ranges of batch 0
  tile                   keys 64..127 dropped
  dead_zero              rows with no key written as zeros, not the uniform average

`mutant_forward` is plain numpy apart from the harness; with no mutant it must reproduce the
oracle, on Gaussian Q as well (test_forward_gate.py uses it for the 16-bit gate's mutants).
"""
import functools

import numpy as np
import pytest

import oracle_lib as ol
from harness import _MASK_VALUE, allowed_keys, assert_census, census_inputs, census_ranges

_LOG2E = float(np.float32(1.442695041))
SHAPE = (2, 4, 2, 300, 257, 64)   # B, H, Hkv, R, C, D
# kind: (causal, window, ranges?, additive mask?)
KINDS = {
    "none": (False, None, False, False),
    "causal": (True, None, False, False),
    "window": (False, 24, False, False),          # R > C + W: the last rows have no key
    "ranges": (False, None, True, False),
    "causal_ranges": (True, None, True, False),
    "window_ranges": (False, 24, True, False),
    "amask": (False, None, False, True),
}
ANY = ["drop_last_key", "padded_key", "tile", "gqa_div"]
MUTANTS = {
    "none": ANY,
    "causal": ANY + ["causal_plus", "causal_minus"],
    "window": ANY + ["window_plus", "window_minus", "dead_zero"],
    "ranges": ANY + ["range_hi_incl", "range_lo_excl", "ranges_by_query_head", "ranges_batch0",
                     "dead_zero"],
    "causal_ranges": ANY + ["causal_plus", "causal_minus", "range_hi_incl", "range_lo_excl",
                            "ranges_by_query_head", "ranges_batch0", "dead_zero"],
    "window_ranges": ANY + ["window_plus", "window_minus", "range_hi_incl", "range_lo_excl",
                            "ranges_by_query_head", "ranges_batch0", "dead_zero"],
    "amask": ANY,
}


def padded_d(D):
    return 64 if D <= 64 else 128 if D <= 128 else 256


def mutant_forward(Q, K, V, causal=False, window=None, amask=None, ranges=None, scale=None,
                   mutant=None):
    """Float64 forward {"O", "L"}, wrong in the one way `mutant` names (None: the reference)."""
    Q, K, V = (np.asarray(x, dtype=np.float64) for x in (Q, K, V))
    B, H, R, D = Q.shape
    Hkv, C = K.shape[1], K.shape[2]
    sc = float(np.float32(1.0 / np.sqrt(np.float32(D)))) if scale is None else float(scale)
    if mutant == "scale_padded":
        sc = 1.0 / np.sqrt(padded_d(D))
    c2 = _LOG2E * sc
    pad = mutant == "padded_key"
    Cx = C + 1 if pad else C
    r, c = np.arange(R)[:, None], np.arange(Cx)[None, :]
    O, L = np.zeros((B, H, R, D)), np.zeros((B, H, R))
    for b in range(B):
        for h in range(H):
            kv = h // (H // Hkv) if mutant == "gqa_div" else h % Hkv
            keep = np.ones((R, Cx), dtype=bool)
            if causal:
                keep &= c <= r + {"causal_plus": 1, "causal_minus": -1}.get(mutant, 0)
            if window is not None:
                keep &= r <= c + int(window) + {"window_plus": 1, "window_minus": -1}.get(mutant, 0)
            if ranges is not None:
                flat = np.asarray(ranges).astype(np.int64).reshape(B * Hkv, R, 2)
                rb = 0 if mutant == "ranges_batch0" else b
                rg = flat[(rb * Hkv + (h if mutant == "ranges_by_query_head" else kv)) % (B * Hkv)]
                lo, hi = rg[:, 0:1], rg[:, 1:2]
                keep &= (c > lo) if mutant == "range_lo_excl" else (c >= lo)
                keep &= (c <= hi) if mutant == "range_hi_incl" else (c < hi)
            if mutant == "drop_last_key":
                keep[:, C - 1] = False
            if mutant == "tile":
                keep[:, 64:128] = False
            k, v = K[b, kv], V[b, kv]
            am = None if amask is None else np.asarray(amask[b, h], dtype=np.float64)
            if pad:
                k, v = np.vstack([k, np.zeros((1, D))]), np.vstack([v, np.zeros((1, D))])
                am = None if am is None else np.hstack([am, np.zeros((R, 1))])
            s = Q[b, h] @ k.T
            if am is None:
                x = c2 * s
            else:
                x = c2 * s + am if mutant == "mask_after_scale" else c2 * (s + am)
            x = np.where(keep, x, -np.inf)
            dead = ~keep.any(axis=1)
            x[dead] = np.where(c < C, 0.0, -np.inf)
            mx = x.max(axis=1, keepdims=True)
            p = np.exp2(x - mx)
            lsum = p.sum(axis=1)
            O[b, h] = (p @ v) / lsum[:, None]
            L[b, h] = np.where(dead, float(np.float32(_MASK_VALUE)) * c2 + np.log2(C),
                               mx[:, 0] + np.log2(lsum))
            if mutant == "dead_zero":
                O[b, h][dead] = 0.0
    return {"O": O, "L": L}


@functools.lru_cache(maxsize=None)
def census_case(kind):
    """Inputs, mask arguments, allowed keys and the oracle's result of one mask kind."""
    B, H, Hkv, R, C, D = SHAPE
    causal, window, with_ranges, with_amask = KINDS[kind]
    Q, K, V = census_inputs(B, H, Hkv, R, C, D, seed=len(kind) + 7)
    kw = {"causal": causal, "window": window}
    ok = None
    if with_ranges:
        kw["ranges"] = census_ranges(B, Hkv, R, C, seed=31)
    if with_amask:
        rng = np.random.default_rng(32)
        am = np.where(rng.random((B, H, R, C)) < 0.4, -1e9, 0.0).astype(np.float32)
        am[..., 3] = 0.0                      # no row fully masked
        kw["amask"] = am
        ok = am == 0
    okm = allowed_keys(B, H, Hkv, R, C, causal, window, kw.get("ranges"))
    ok = okm if ok is None else ok & okm
    ref = ol.attention(Q, K, V, **kw)
    for a in (Q, K, V, ok, ref["O"], ref["L"]):
        a.setflags(write=False)
    return Q, K, V, kw, ok, ref


@pytest.mark.parametrize("kind", list(KINDS))
def test_oracle_passes_the_census(kind):
    Q, K, V, kw, ok, ref = census_case(kind)
    assert_census(ref["O"], ref["L"], ok, V, ref["L"])
    # How far inside the bound the oracle sits, and the dead rows of both descriptions.
    n = ok.sum(axis=3)
    live = n > 0
    dead_oracle = np.abs(ref["L"]) > 1e30
    assert (dead_oracle == ~live).all()
    if kind in ("window", "ranges", "causal_ranges", "window_ranges"):
        assert (~live).any() and live.any()
    two = np.exp2(ref["L"].astype(np.float64)[live])
    assert np.abs(two - n[live]).max() < 1e-3
    # The plain numpy forward is the oracle, and passes too.
    plain = mutant_forward(Q, K, V, **kw)
    assert_census(plain["O"], plain["L"], ok, V, ref["L"])
    assert np.abs(plain["O"] - ref["O"]).max() < 1e-5


@pytest.mark.parametrize("kind,mutant", [(k, m) for k in KINDS for m in MUTANTS[k]])
def test_mutant_fails_the_census(kind, mutant):
    Q, K, V, kw, ok, ref = census_case(kind)
    bad = mutant_forward(Q, K, V, mutant=mutant, **kw)
    with pytest.raises(AssertionError, match="census"):
        assert_census(bad["O"], bad["L"], ok, V, ref["L"])


def test_census_rejects_swapped_keys_and_skipped_rows():
    Q, K, V, kw, ok, ref = census_case("causal")
    o = ref["O"].copy()
    # Row 1 attends to keys {0, 1}: give it keys {0, 2} (same count, another sum).
    o[0, 0, 1] = (V[0, 0, 0] + V[0, 0, 2]) / 2
    with pytest.raises(AssertionError, match="sum of V"):
        assert_census(o, ref["L"], ok, V, ref["L"])
    o = ref["O"].copy()
    o[1, 3, 200] = np.nan                      # a row the kernel never wrote
    with pytest.raises(AssertionError, match="census"):
        assert_census(o, ref["L"], ok, V, ref["L"])
    l = ref["L"].copy()
    l[1, 2, 17] = np.nan
    with pytest.raises(AssertionError, match="key count"):
        assert_census(ref["O"], l, ok, V, ref["L"])
