"""Shared helpers for the GPU parity tests (device tensors <-> oracle arrays)."""
from __future__ import annotations

import functools
import os
import re
import shutil
import subprocess
import tempfile
import types

import numpy as np
import pytest
import torch

import mfa_amd as mfa
import oracle_lib as ol

TORCH_DTYPE = {mfa.Precision.FP32: torch.float32, mfa.Precision.FP16: torch.float16,
               mfa.Precision.BF16: torch.bfloat16}
ROUND = {mfa.Precision.FP16: "fp16", mfa.Precision.BF16: "bf16"}


def to_device(x: np.ndarray, prec: mfa.Precision, dev="cuda:0") -> torch.Tensor:
    """Store x in `prec` on the device (RNE); returns the device tensor."""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev).to(TORCH_DTYPE[prec])


def seen(x: np.ndarray, prec: mfa.Precision) -> np.ndarray:
    """The values the kernel actually sees after storage in `prec`."""
    if prec == mfa.Precision.FP32:
        return np.asarray(x, dtype=np.float32)
    return ol.round16(x, ROUND[prec])


def maxerr(a, b) -> float:
    a = a.detach().float().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().float().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    if a.size == 0:
        return 0.0
    return float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64))))


def relerr(a, b) -> float:
    a = a.detach().float().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().float().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    d = np.linalg.norm((a.astype(np.float64) - b.astype(np.float64)).ravel())
    return float(d / (np.linalg.norm(b.astype(np.float64).ravel()) + 1e-8))


# ------------------------------------------------------------------ 16-bit gradient gate
# An absolute 5e-2 on dQ/dK/dV says nothing when the gradients themselves are that small.
# The gate below is relative to each tensor's own size and comes from the reference alone:
# GRAD_MARGIN x the error of emulated_backward (float64 with the roundings the backward
# contract allows) against the float64 reference on the case's own inputs.
# tests/test_grad_gate.py proves on the CPU that this gate rejects subtly wrong backwards.
GRAD_MARGIN = 4.0
GRAD_GATE_CEILING = 8e-2  # a case whose gate exceeds this is ill-conditioned: change its inputs
_LOG2E = np.float32(1.442695041)


def grad_errors(got, ref, rows=None):
    """(slice error, row error) of one gradient tensor [B, Hx, N, D] against its reference.

    slice error: max|got - ref| over a (b, h) slice / max|ref| of that slice, max over slices.
    row error:   ||got_row - ref_row|| / (||ref_row|| + 1e-2 * largest row norm of the slice),
                 max over every row; the floor keeps rows whose true gradient is zero in.
    rows: optional bool [N]; rows where it is False take no part in either metric."""
    g = np.asarray(got, dtype=np.float64)
    r = np.asarray(ref, dtype=np.float64)
    assert g.shape == r.shape and g.ndim == 4, (g.shape, r.shape)
    if rows is not None:
        g, r = g[:, :, rows], r[:, :, rows]
    if r.size == 0:
        return 0.0, 0.0
    d = g - r
    num = np.abs(d).max(axis=(2, 3))
    den = np.abs(r).max(axis=(2, 3))
    with np.errstate(divide="ignore", invalid="ignore"):
        sl = np.where(den > 0, num / den, np.where(num > 0, np.inf, 0.0))
    rn = np.linalg.norm(r, axis=3)
    floor = 1e-2 * rn.max(axis=2, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        rw = np.linalg.norm(d, axis=3) / (rn + floor)
    rw = np.where(np.isnan(rw), 0.0, rw)  # 0 / 0: a slice whose reference is all zero, met exactly
    return float(sl.max()), float(rw.max())


def allowed_keys(B, H, Hkv, R, C, causal=False, window=None, ranges=None):
    """bool [B, H, R, C]: the keys each row may attend to (the oracle's masks, mfa_oracle.c)."""
    r = np.arange(R)[:, None]
    c = np.arange(C)[None, :]
    ok = np.ones((R, C), dtype=bool)
    if causal:
        ok &= c <= r
    if window is not None:
        ok &= r <= c + int(window)
    ok = np.broadcast_to(ok, (B, H, R, C)).copy()
    if ranges is not None:
        rg = np.asarray(ranges).astype(np.int64)[:, np.arange(H) % Hkv]  # [B, H, R, 2]
        ok &= (c >= rg[..., 0:1]) & (c < rg[..., 1:2])
    return ok


def emulated_backward(Q, K, V, dO, prec, causal=False, window=None, amask=None, ranges=None,
                      scale=None, low_precision_intermediates=True, round_dO=False):
    """The backward in numpy float64 on the kernel-visible inputs, rounded where the backward
    contract (include/mfa/mfa.h) lets the kernels round and nowhere else:

    * L to FP16 and D to BF16 by truncation, when low_precision_intermediates.  The rounded
      D is the one in memory, which the key/value phase reads back for dK.  The query phase
      computes D in FP32 and uses that value for dQ in the same kernel (Drow:
      attention_bwd.h:110/191, attention_bwd_fast.hip:350/515, attention_bigd.hip:210/298),
      so dQ takes the unrounded D: with the truncated one, row 0 of a causal dQ, whose true
      value is exactly 0 = P∘(dP*scale - D), would alone carry an error of ~|D|/256 * |K_0|.
    * P = exp2(S*c - L), as the dV operand, and dS = P∘(dP*scale - D), as the dQ/dK operand,
      to the 16-bit type `prec`.
    * round_dO, for a call whose dO is FP32 in memory while Q is 16-bit (the quantised
      backward allows it, mfa_api.cpp:1371): the kernels round dO to `prec` as the MFMA operand
      of dP and dV (from_f32 in load_row_frags, mfa_stage.h:360-364, called at
      attention_bwd.h:104; the tile staging of the key/value phase, mfa_stage.h:242 and :303)
      and keep the FP32 values for D (rowsum_do_o, attention_bwd.h:57-73).

    Inputs stay exact and every sum is float64.  prec=None (or FP32) rounds nothing: the
    float64 reference itself.  Rows with no key allowed take the oracle's uniform P.
    Uses numpy and the oracle library's rounding helpers only."""
    Q, K, V, dO = (np.asarray(x, dtype=np.float64) for x in (Q, K, V, dO))
    B, H, R, D = Q.shape
    Hkv, C = K.shape[1], K.shape[2]
    kind = ROUND.get(prec)
    sc = np.float32(1.0 / np.sqrt(np.float32(D))) if scale is None else np.float32(scale)
    c2, sc = float(_LOG2E * sc), float(sc)
    ok = allowed_keys(B, H, Hkv, R, C, causal, window, ranges)
    r16 = (lambda x, k: ol.round16(x.astype(np.float32), k).astype(np.float64))
    out = {"O": np.zeros((B, H, R, D)), "L": np.zeros((B, H, R)), "D": np.zeros((B, H, R)),
           "dQ": np.zeros((B, H, R, D)), "dK": np.zeros((B, Hkv, C, D)),
           "dV": np.zeros((B, Hkv, C, D))}
    for b in range(B):
        for h in range(H):
            kv = h % Hkv
            q, k, v, do, m = Q[b, h], K[b, kv], V[b, kv], dO[b, h], ok[b, h]
            s = q @ k.T
            if amask is not None:
                s = s + np.asarray(amask[b, h], dtype=np.float64)
            x = np.where(m, c2 * s, -np.inf)
            dead = ~m.any(axis=1)
            x[dead] = 0.0
            mx = x.max(axis=1, keepdims=True)
            L = mx[:, 0] + np.log2(np.exp2(x - mx).sum(axis=1))
            p = np.exp2(x - L[:, None])
            o = p @ v
            Dq = Dm = sc * (do * o).sum(axis=1)   # D of the query phase / D in memory
            if kind and low_precision_intermediates:
                Lr = np.where(dead, L, r16(L, "fp16"))
                Dm = r16(Dq, "bf16_trunc")
                p = np.exp2(x - Lr[:, None])
            if kind and round_dO:
                do = r16(do, kind)
            dps = (do @ v.T) * sc
            dsq, dsk = p * (dps - Dq[:, None]), p * (dps - Dm[:, None])
            if kind:
                p, dsq, dsk = r16(p, kind), r16(dsq, kind), r16(dsk, kind)
            out["O"][b, h], out["L"][b, h], out["D"][b, h] = o, L, Dm
            out["dQ"][b, h] = dsq @ k
            out["dK"][b, kv] += dsk.T @ q
            out["dV"][b, kv] += p.T @ do
    return out


def gradient_gate(Qs, Ks, Vs, dOs, prec, ref, rows=None, names=("dQ", "dK", "dV"), **kw):
    """{name: (slice gate, row gate)} for dQ, dK, dV: GRAD_MARGIN x the emulation's error
    against `ref` (the float64 reference on the same kernel-visible inputs).  `rows` applies
    to dQ only.  Computed from the reference alone, never from what the GPU returned."""
    emu = emulated_backward(Qs, Ks, Vs, dOs, prec, **kw)
    gate = {}
    for name in names:
        e = grad_errors(emu[name], ref[name], rows if name == "dQ" else None)
        gate[name] = tuple(GRAD_MARGIN * x for x in e)
        assert max(gate[name]) <= GRAD_GATE_CEILING, (
            f"{name}: gate {gate[name]} over {GRAD_GATE_CEILING}: ill-conditioned inputs")
    return gate


def assert_gradients_within_gate(got, ref, gate, rows=None, report=None):
    """Both metrics of dQ, dK, dV in `got` (arrays or tensors) against `ref` under `gate`."""
    errs = {}
    for name in gate:
        g = got[name]
        g = g.detach().float().cpu().numpy() if isinstance(g, torch.Tensor) else np.asarray(g)
        e = errs[name] = grad_errors(g, ref[name], rows if name == "dQ" else None)
        print(f"grad-gate {report or ''} {name}: slice {e[0]:.3e} (gate {gate[name][0]:.3e}) "
              f"row {e[1]:.3e} (gate {gate[name][1]:.3e})")
    for name, e in errs.items():
        assert e[0] <= gate[name][0], f"{name} slice error {e[0]:.3e} > gate {gate[name][0]:.3e}"
        assert e[1] <= gate[name][1], f"{name} row error {e[1]:.3e} > gate {gate[name][1]:.3e}"


# ------------------------------------------------------------------ forward: the key census
# With Q = 0 every unmasked score is exactly 0, P is exactly 1 and every sum is a small integer
# that FP32 holds exactly: a correct forward of any type gives 2^L = n (the number of keys the
# row attends to) and n * O = the sum of those keys' V rows.  V holds small non-zero integers
# in pairwise distinct rows, so one extra, missing or swapped key moves n or a column of the
# sum by at least 1.  tests/test_forward_census.py proves on the CPU what this rejects.
CENSUS_TOL = 0.25  # half the distance to the nearest wrong integer, with a factor of two to spare
_MASK_VALUE = -(0.875 / 1.442695041) * 3.402823466e+38  # mfa_device.h:43, mfa_oracle.c


def census_inputs(B, H, Hkv, R, C, D, seed):
    """(Q, K, V) float32 for a key census: Q = 0, K Gaussian (a kernel that forgets a mask
    meets arbitrary keys), V integers from {-2, -1, 1, 2} with pairwise distinct rows."""
    rng = np.random.default_rng(seed)
    Q = np.zeros((B, H, R, D), dtype=np.float32)
    K = rng.standard_normal((B, Hkv, C, D)).astype(np.float32)
    V = rng.choice(np.array([-2.0, -1.0, 1.0, 2.0], dtype=np.float32), size=(B, Hkv, C, D))
    assert (V != 0).all()
    for b in range(B):
        for kv in range(Hkv):
            assert len(np.unique(V[b, kv], axis=0)) == C, "census V rows must be distinct"
    return Q, K, V


def census_ranges(B, Hkv, R, C, seed):
    """uint32 [B, Hkv, R, 2] key ranges in the manner of test_sparse_gpu.py's
    test_ranges_beyond_sequence: different for every batch and kv head, some reaching past C,
    some empty (x == y) and some with x > y."""
    rng = np.random.default_rng(seed)
    lo = rng.integers(0, C + 40, (B, Hkv, R))
    hi = lo + rng.integers(-5, 200, (B, Hkv, R))
    ranges = np.stack([lo, np.maximum(hi, 0)], -1).astype(np.uint32)
    ranges[:, :, 5::11, 1] = ranges[:, :, 5::11, 0]      # empty rows
    ranges[:, :, 2::7, 0] = ranges[:, :, 2::7, 0] // 4   # rows that start early
    assert (ranges[..., 1] > C).any() and (ranges[..., 0] > ranges[..., 1]).any()
    return ranges


def assert_census(o, l, ok, V, ref_L):
    """O [B, H, R, D] and L [B, H, R] (FP32 L, arrays or tensors) of a forward on
    census_inputs against ok = allowed_keys(...) [B, H, R, C]; ref_L is the oracle's L.

    Rows with n >= 1 allowed keys: rint(2^L) == n, |2^L - n| < CENSUS_TOL and
    |rint(2^L) * O - sum of the allowed V rows| < CENSUS_TOL in every element.
    Rows with none: the oracle's uniform average, |C * O - sum of all V rows| < CENSUS_TOL,
    and L equal to the oracle's to rtol 1e-6.  Every row takes part (NaN fails)."""
    o = o.detach().float().cpu().numpy() if isinstance(o, torch.Tensor) else np.asarray(o)
    l = l.detach().float().cpu().numpy() if isinstance(l, torch.Tensor) else np.asarray(l)
    o, l, V = o.astype(np.float64), l.astype(np.float64), np.asarray(V, dtype=np.float64)
    B, H, R, C = ok.shape
    Hkv = V.shape[1]
    assert o.shape == (B, H, R, V.shape[3]) and l.shape == (B, H, R), (o.shape, l.shape)
    n = ok.sum(axis=3)
    live = n > 0
    okf = ok.astype(np.float64)
    want = np.stack([np.stack([okf[b, h] @ V[b, h % Hkv] for h in range(H)]) for b in range(B)])
    with np.errstate(over="ignore", invalid="ignore"):
        two = np.where(live, np.exp2(np.where(live, l, 0.0)), 0.0)
    cnt = np.rint(two)
    bad_n = live & ~((cnt == n) & (np.abs(two - n) < CENSUS_TOL))
    with np.errstate(invalid="ignore"):
        dev = np.abs(cnt[..., None] * o - want)
    bad_o = live & ~(dev < CENSUS_TOL).all(axis=3)
    for bad, what in ((bad_n, "key count"), (bad_o, "sum of V")):
        if bad.any():
            b, h, r = (int(x) for x in np.argwhere(bad)[0])
            col = int(np.argmax(~(dev[b, h, r] < CENSUS_TOL)))
            raise AssertionError(
                f"census: {what} wrong in {int(bad.sum())} rows; first (b {b}, h {h}, row {r}): "
                f"n {int(n[b, h, r])}, 2^L {two[b, h, r]:.6g}, rint(2^L) - n "
                f"{cnt[b, h, r] - n[b, h, r]:.0f}, first differing column {col}: rint(2^L)*O "
                f"{cnt[b, h, r] * o[b, h, r, col]:.6g} against {want[b, h, r, col]:.6g}")
    dead = ~live
    if dead.any():
        allv = np.stack([np.stack([V[b, h % Hkv].sum(axis=0) for h in range(H)]) for b in range(B)])
        with np.errstate(invalid="ignore"):
            dd = np.abs(C * o - allv[:, :, None, :])
        bad = dead & ~(dd < CENSUS_TOL).all(axis=3)
        assert not bad.any(), (f"census: {int(bad.sum())} rows with no key are not the uniform "
                               f"average; first (b, h, row) {np.argwhere(bad)[0]}")
        assert np.allclose(l[dead], np.asarray(ref_L, dtype=np.float64)[dead], rtol=1e-6, atol=0)


# ------------------------------------------------------------------ 16-bit forward gate
# The forward's counterpart of the gradient gate: O is held to FWD_MARGIN x the error of
# emulated_forward against the float64 reference on the case's own inputs, in the two metrics
# of grad_errors; L to the same multiple of the emulation's max abs error plus the FP32 floor
# below.  tests/test_forward_gate.py proves on the CPU what this rejects.
FWD_MARGIN = 4.0
# Relative (both O metrics): a case whose gate exceeds it is ill-conditioned, change its inputs.
# Measured 4 x emulation over the cases of test_forward_gate.py and every gated GPU case: at
# most 2.7e-3 (FP16) and 1.1e-2 (BF16; 2.5e-3 and 1e-2 on the six cases of the CPU proof alone).
# The ceiling is twice the BF16 figure, rounded down.
FWD_GATE_CEILING = 2e-2


def _padded_d(D):
    return 64 if D <= 64 else 128 if D <= 128 else 256


def emulated_forward(Q, K, V, prec, causal=False, window=None, amask=None, ranges=None,
                     scale=None, low_precision_intermediates=True, prescaled_q=False):
    """The forward in numpy float64 on the kernel-visible inputs, rounded where the forward
    kernels round and nowhere else:

    * P = exp2(S*c - m) goes to the 16-bit type `prec` (round to nearest even) as the PV
      operand, while the row sum l is taken from the unrounded FP32 P: the tuned kernels in
      fwd2_exp (attention_fwd2.h:253-266: rs += pv, then A::pack), the generic kernel at
      attention_fwd.hip:133-135 and :153; pack is E::from_f32 per element (mfa_device.h:228-231,
      :53-61).  O = (P16 V) / l in FP32 (attention_fwd.hip:170).
    * L = m + log2(l) goes to FP16 when low_precision_intermediates (store_l,
      attention_fwd2.h:406-412; attention_fwd.hip:196-201).
    * prescaled_q: the tuned FP16 kernels with a padded head width <= 128 round Q*c to FP16
      before QK^T (prescale_q2, attention_fwd2.h:389-397, PS at :179/:246) and then take
      S' = S - m from the MFMA directly.  BF16 and D = 256 keep Q and scale S in FP32
      (attention_fwd2.h:253), and so does the generic kernel at any type (load_row_frags at
      attention_fwd.hip:46, s*c - m at :133): pass prescaled_q=False for those.

    Inputs stay exact and every sum is float64.  prec=None (or FP32) rounds nothing: the
    float64 reference itself.  The additive mask is added to QK^T before scaling; rows with no
    key allowed take the oracle's uniform P and its L = mask*c + log2 C.
    Returns {"O": [B, H, R, D], "L": [B, H, R]} in float64."""
    Q, K, V = (np.asarray(x, dtype=np.float64) for x in (Q, K, V))
    B, H, R, D = Q.shape
    Hkv, C = K.shape[1], K.shape[2]
    kind = ROUND.get(prec)
    sc = np.float32(1.0 / np.sqrt(np.float32(D))) if scale is None else np.float32(scale)
    c2 = float(_LOG2E * sc)
    ok = allowed_keys(B, H, Hkv, R, C, causal, window, ranges)
    r16 = (lambda x, k: ol.round16(x.astype(np.float32), k).astype(np.float64))
    prescaled_q = bool(prescaled_q and kind == "fp16" and _padded_d(D) <= 128 and D <= 256)
    out = {"O": np.zeros((B, H, R, D)), "L": np.zeros((B, H, R))}
    for b in range(B):
        for h in range(H):
            kv = h % Hkv
            q, k, v, m = Q[b, h], K[b, kv], V[b, kv], ok[b, h]
            if prescaled_q:
                assert amask is None, "the pre-scaling kernels take no additive mask"
                x = r16(q * c2, "fp16") @ k.T
            else:
                s = q @ k.T
                if amask is not None:
                    s = s + np.asarray(amask[b, h], dtype=np.float64)
                x = c2 * s
            x = np.where(m, x, -np.inf)
            dead = ~m.any(axis=1)
            x[dead] = 0.0
            mx = x.max(axis=1, keepdims=True)
            p = np.exp2(x - mx)
            lsum = p.sum(axis=1)
            L = mx[:, 0] + np.log2(lsum)
            if kind:
                p = r16(p, kind)
                if low_precision_intermediates:
                    L = np.where(dead, L, r16(L, "fp16"))
            L = np.where(dead, float(np.float32(_MASK_VALUE)) * c2 + np.log2(C), L)
            out["O"][b, h] = (p @ v) / lsum[:, None]
            out["L"][b, h] = L
    return out


def forward_errors(got, ref):
    """(slice error of O, row error of O, max abs error of L over the rows with a key) of
    got = {"O", "L"} against ref; O in the metrics of grad_errors."""
    lr = np.asarray(ref["L"], dtype=np.float64)
    lg = np.asarray(got["L"], dtype=np.float64)
    live = np.abs(lr) < 1e30
    el = float(np.abs(lg - lr)[live].max()) if live.any() else 0.0
    return (*grad_errors(got["O"], ref["O"]), el)


def forward_gate(Qs, Ks, Vs, prec, ref, **kw):
    """(slice gate of O, row gate of O, gate of L): FWD_MARGIN x the emulation's error against
    `ref` (the float64 reference on the same kernel-visible inputs), computed from the reference
    alone, never from what the GPU returned.  L also gets the FP32 floor D * 2^-24 * max|L|: the
    kernels accumulate each score over D products in FP32 (forward error bound D * u of a dot
    product, u = 2^-24, on scores of L's size), which the float64 emulation does not have;
    it is 8e-5 at D 128 and |L| 10, next to a smallest L error of 2e-3 among the mutants."""
    emu = emulated_forward(Qs, Ks, Vs, prec, **kw)
    sl, rw, el = forward_errors(emu, ref)
    # O's own FP32 floor, 8 ulps = 2^-21: O leaves as acc * (1 / l), a reciprocal and a product
    # on top of the FP32 sums.  It matters only where the emulation is exact (a single key).
    gate = (FWD_MARGIN * sl + 2.0 ** -21, FWD_MARGIN * rw + 2.0 ** -21)
    assert max(gate) <= FWD_GATE_CEILING, (
        f"O: gate {gate} over {FWD_GATE_CEILING}: ill-conditioned inputs")
    lr = np.asarray(ref["L"], dtype=np.float64)
    live = np.abs(lr) < 1e30
    lmax = float(np.abs(lr[live]).max()) if live.any() else 0.0
    return (*gate, FWD_MARGIN * el + Qs.shape[3] * 2.0 ** -24 * lmax)


def prescales_q(names):
    """Whether the launched kernels `names` (mfa.last_launches) are the tuned 16-bit forward
    family built on attention_fwd2.h, which pre-scales an FP16 Q (emulated_forward decides on
    the type and the padded width); the generic and big-D kernels never do."""
    return any(n.startswith(("mfa_fwd2_", "mfa_fwd_pipe_")) for n in names)


def assert_forward_within_gate(o, l, ref, gate, report=None):
    """O (both metrics) and L of a forward (arrays or tensors) against `ref` under `gate`."""
    cpu = lambda x: x.detach().float().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    e = forward_errors({"O": cpu(o), "L": cpu(l)}, ref)
    print(f"fwd-gate {report or ''} O: slice {e[0]:.3e} (gate {gate[0]:.3e}) "
          f"row {e[1]:.3e} (gate {gate[1]:.3e}) L: {e[2]:.3e} (gate {gate[2]:.3e})")
    assert e[0] <= gate[0], f"O slice error {e[0]:.3e} > gate {gate[0]:.3e}"
    assert e[1] <= gate[1], f"O row error {e[1]:.3e} > gate {gate[1]:.3e}"
    assert e[2] <= gate[2], f"L error {e[2]:.3e} > gate {gate[2]:.3e}"


def paged_cache(d, prec=None, page=64, **kw):
    """A PagedKVCache shaped for the paged decode, prefill or append descriptor d, of d's 16-bit
    type unless `prec` is given; its pointers are null (enough for a plan query)."""
    if prec is None:
        prec = d.input_precision if hasattr(d, "input_precision") else d.base.input_memory_precision
    max_pages = -(-d.max_seq_len // page) if page else 1
    return mfa.PagedKVCache.make(mfa.Precision(prec), page, max_pages,
                                 max(1, max_pages * d.batch_size), d.num_kv_heads, d.head_dim, **kw)


def paged_cache_full(d, **kw):
    """paged_cache with every pointer set (aligned stand-ins, for calls the host rejects)."""
    c = paged_cache(d, **kw)
    c.k_pool, c.v_pool, c.block_table, c.seq_lens = 0x300000, 0x400000, 0x500000, 0x600000
    return c


def run_forward(Qn, Kn, Vn, prec=mfa.Precision.FP32, causal=False, window=None, scale=None,
                amask=None, ranges=None, low_precision_intermediates=None, q_strides=None,
                layout=None, dev="cuda:0"):
    """Forward through the C ABI on BHSD numpy inputs; returns (O, L) torch tensors."""
    B, H, R, D = Qn.shape
    Hkv, C = Kn.shape[1], Kn.shape[2]
    lp = prec != mfa.Precision.FP32
    base = mfa.AttentionDescriptor.make(
        low_precision=lp, precision=prec if lp else None, causal=causal, window=window,
        scale=scale, low_precision_intermediates=low_precision_intermediates,
        sparse_mask=(mfa.MaskType.sparseRanges if ranges is not None else None))
    desc = mfa.MultiHeadDescriptor.make(base, B, H, R, D, Hkv=Hkv, C=C)
    q, k, v = to_device(Qn, prec, dev), to_device(Kn, prec, dev), to_device(Vn, prec, dev)
    o = torch.full((B, H, R, D), float("nan"), dtype=torch.float32, device=dev)
    l_dtype = torch.float16 if base.low_precision_intermediates else torch.float32
    l = torch.full((B, H, R), float("nan"), dtype=l_dtype, device=dev)
    mask = None
    if amask is not None:
        mask = torch.from_numpy(np.ascontiguousarray(amask, dtype=np.float32)).to(dev)
    if ranges is not None:
        mask = torch.from_numpy(np.ascontiguousarray(ranges, dtype=np.uint32).view(np.int32)).to(dev)
    mfa.MultiHeadAttention().forward(desc, q, k, v, o, l, mask=mask)
    torch.cuda.synchronize()
    return o, l


# ------------------------------------------------------------------ code-object metadata
_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "metal-flash-attention-plus_amd", "libmfa_amd.so")
_LLVM = "/opt/rocm/lib/llvm/bin"
_NOTE_FIELDS = {"scratch": "private_segment_fixed_size", "vgpr_spill": "vgpr_spill_count",
                "sgpr_spill": "sgpr_spill_count", "vgpr": "vgpr_count",
                "lds": "group_segment_fixed_size"}


@functools.lru_cache(maxsize=None)
def code_object_metadata():
    """{mangled kernel name: {"scratch", "vgpr_spill", "sgpr_spill", "vgpr", "lds"}} of every
    gfx950 kernel in the built library, from the code objects' metadata notes (llvm-objdump
    --offloading, llvm-readelf --notes; nothing is disassembled).  Extracted once per process,
    into a temporary directory.  Skips the calling test or fixture where the library or the ROCm
    LLVM tools are absent.  The result is shared by every caller and read-only."""
    if not (os.path.exists(_LIB) and os.path.exists(os.path.join(_LLVM, "llvm-readelf"))):
        pytest.skip("library or ROCm LLVM tools not present")
    notes = ""
    with tempfile.TemporaryDirectory() as d:
        lib = shutil.copy(_LIB, d)
        subprocess.run([os.path.join(_LLVM, "llvm-objdump"), "--offloading", lib], check=True,
                       capture_output=True, cwd=d)
        for f in sorted(os.listdir(d)):
            if f.endswith("gfx950"):
                notes += subprocess.run([os.path.join(_LLVM, "llvm-readelf"), "--notes",
                                         os.path.join(d, f)], check=True, capture_output=True,
                                        text=True).stdout
    out = {}
    for ent in notes.split("- .agpr_count")[1:]:
        def field(k):
            m = re.search(r"\." + k + r":\s+(\S+)", ent)
            return m.group(1) if m else None
        vals = {k: field(f) for k, f in _NOTE_FIELDS.items()}
        # A field a kernel's note lacks is left out, so only a test that reads it notices.
        out[field("name")] = types.MappingProxyType(
            {k: int(v) for k, v in vals.items() if v is not None})
    assert out, "no kernel metadata found"
    return types.MappingProxyType(out)


def kernels_named(fragment):
    """code_object_metadata() of the kernels whose mangled name contains `fragment`."""
    return {n: k for n, k in code_object_metadata().items() if fragment in n}
