"""Shared helpers for the GPU parity tests (device tensors <-> oracle arrays)."""
from __future__ import annotations

import numpy as np
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
