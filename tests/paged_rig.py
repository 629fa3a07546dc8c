"""What the paged GPU tests share (test_paged_*_gpu.py): a dense per-sequence cache scattered
into page pools through a block table, the three device caches built on it, the rows' key
positions, the cases' data with their oracle results, the calls and the tolerances.

The rule that gives those tests their meaning is stated once, in scatter(): every pool slot no
sequence owns (spare pages, slots past a sequence's length in its last page) holds the fill — NaN
in 16-bit pools, a byte in INT8 pools — so anything read from outside a sequence shows.
scatter() and positions() are numpy only; tests/test_paged_rig.py checks them on the CPU."""
import functools

import numpy as np
import torch

import mfa_amd as mfa
import oracle_lib as ol
from harness import maxerr, seen, to_device

P = mfa.Precision
DEV = "cuda:0"
ZP = 3  # zero point of the INT8 caches
FLT_MAX = float(np.finfo(np.float32).max)
NAN = float("nan")


def i32(xs):
    return None if xs is None else torch.tensor(list(xs), dtype=torch.int32, device=DEV)


def tag(prec):
    return "F16" if prec == P.FP16 else "BF16"


# ------------------------------------------------------------------------ the scattered cache
def scatter(seqs, page, shuffle=True, spare=3, seed=1, table_fill=0, fill=np.nan):
    """seqs: one list per pool (K and V, or one latent) of per-sequence arrays [..., len_b, X].
    Returns (pools, table): pool [num_pages, ..., page, X] per list and the int32 block table
    [B, max_pages], the same for every pool.

    num_pages = sum(ceil(len_b / page)) + spare; max_pages = max(1, a sequence's most pages), one
    more column when table_fill is set; the page ids are a seeded permutation of the pool's pages
    (shuffle) or 0, 1, .. and are handed out in (b, j) order.  Table entries of logical pages no
    sequence owns hold table_fill.  Every slot no sequence owns holds `fill`: NaN (float32 pools),
    a byte, or "random" bytes (int8 pools)."""
    alloc = [x.shape[-2] for x in seqs[0]]
    npg = [-(-c // page) for c in alloc]
    max_pages = max(1, max(npg)) + (1 if table_fill else 0)
    num_pages = sum(npg) + spare
    ids = np.arange(num_pages)
    if shuffle:
        ids = np.random.default_rng(seed).permutation(num_pages)
    table = np.full((len(alloc), max_pages), table_fill, np.int32)
    pools = []
    for which, xs in enumerate(seqs):
        shape = (num_pages,) + xs[0].shape[:-2] + (page, xs[0].shape[-1])
        if isinstance(fill, str):
            assert fill == "random", fill
            pool = np.random.default_rng(77 + which).integers(-128, 128, shape, dtype=np.int8)
        else:
            pool = np.full(shape, fill, np.float32 if np.isnan(fill) else np.int8)
        nxt = 0
        for b, c in enumerate(alloc):
            for j in range(npg[b]):
                n = min(page, c - j * page)
                pool[ids[nxt], ..., :n, :] = xs[b][..., j * page:j * page + n, :]
                table[b, j] = ids[nxt]
                nxt += 1
        pools.append(pool)
    return pools, table


class _Scattered:
    """Block table and lengths of one scattered cache on the device; `lens` overrides the
    allocated lengths as the device lengths.  Returns the numpy pools."""

    def _scatter(self, seqs, page, lens, **kw):
        pools, self.table_np = scatter(seqs, page, **kw)
        self.num_pages, self.max_pages = pools[0].shape[0], self.table_np.shape[1]
        self.table = torch.from_numpy(self.table_np).to(DEV)
        self.lens = i32([x.shape[-2] for x in seqs[0]] if lens is None else lens)
        self.page = page
        return pools


class Cache(_Scattered):
    """16-bit K/V pools (NaN outside the sequences) from per-sequence K, V [Hkv, len_b, D].
    `strides`: None for the pools' own [page][kv head][slot][d] layout."""

    def __init__(self, Ks, Vs, prec, page, lens=None, **kw):
        self.k, self.v = (to_device(p, prec) for p in self._scatter((Ks, Vs), page, lens, **kw))
        self.prec, self.Hkv, self.D = prec, Ks[0].shape[0], Ks[0].shape[2]
        self.scales, self.zps, self.strides = (1.0, 1.0), (0, 0), None

    def struct(self):
        return mfa.PagedKVCache.make(self.prec, self.page, self.max_pages, self.num_pages,
                                     self.Hkv, self.D, self.k, self.v, self.table, self.lens,
                                     strides=self.strides, k_scale=self.scales[0],
                                     v_scale=self.scales[1], k_zero_point=self.zps[0],
                                     v_zero_point=self.zps[1])


class Cache8(Cache):
    """INT8 K/V pools from per-sequence bytes [Hkv, len_b, D]; `fill`: the byte in every slot no
    sequence owns, or "random"."""

    def __init__(self, qk, qv, page, scales, zps=(ZP, ZP), lens=None, fill=0x7f, **kw):
        pools = self._scatter((qk, qv), page, lens, fill=fill, **kw)
        self.k, self.v = (torch.from_numpy(p).to(DEV) for p in pools)
        self.prec, self.Hkv, self.D = P.INT8, qk[0].shape[0], qk[0].shape[2]
        self.scales, self.zps, self.strides = scales, zps, None


def cache_of(Ks, Vs, prec, page, quant=None, **kw):
    """The scattered K/V cache of a decode case (decode_problem): INT8 pools from `quant`, its
    bytes and scales per operand, where it has them."""
    if quant is None:
        return Cache(Ks, Vs, prec, page, **kw)
    return Cache8(quant[0][0], quant[1][0], page, (quant[0][1], quant[1][1]), **kw)


class LatentCache(_Scattered):
    """One 16-bit latent pool (NaN outside the sequences) from per-sequence latents [len_b, Lat]."""

    def __init__(self, lats, prec, page, lens=None, **kw):
        self.pool = to_device(self._scatter((lats,), page, lens, **kw)[0], prec)
        self.prec, self.latent = prec, lats[0].shape[1]

    def struct(self):
        return mfa.PagedLatentCache.make(self.prec, self.page, self.max_pages, self.num_pages,
                                         self.latent, self.pool, self.table, self.lens)


# ------------------------------------------------------------------------------ row positions
def positions(lens, new_lens, R, causal=True, cap=None, decode=False):
    """Last key every query row sees ([B, R] int64, -1: no visible key) under the calls' clamps:
    len_b = clamp(lens[b], 0, cap), n_b = clamp(new_lens[b], 0, R), R without new_lens.  Row
    q < n_b is key position t = len_b - n_b + q and sees the keys up to t (causal) or all len_b
    (unmasked).  A row with t < 0 is dead, except in the unmasked decode call (decode=True),
    where every row of a sequence sees all of its keys."""
    out = np.full((len(lens), R), -1, np.int64)
    for b, c in enumerate(lens):
        c = max(c, 0) if cap is None else min(max(c, 0), cap)
        n = R if new_lens is None else min(max(new_lens[b], 0), R)
        for q in range(n):
            t = c - n + q
            if causal:
                out[b, q] = max(t, -1)
            elif t >= 0 or decode:
                out[b, q] = c - 1
    return out


# -------------------------------------------------------------------------------- tolerances
def check_dead_rows(on, ln, m, l_f16, what=""):
    """on [B, H, R, D], ln [B, H, R] (float64), m: the rows with a visible key.  No NaN anywhere;
    the other rows are exact zeros with L = -inf (FP16 storage) or -FLT_MAX (FP32)."""
    assert not np.isnan(on).any() and not np.isnan(ln).any(), what
    assert np.count_nonzero(on[~m]) == 0, what
    if l_f16:
        assert np.all(np.isneginf(ln[~m])), what
    else:
        assert np.all(ln[~m] == -FLT_MAX), what


def _rows(o, l, pos):
    on, ln = o.cpu().numpy(), l.float().cpu().numpy().astype(np.float64)
    return on, ln, np.broadcast_to((pos >= 0)[:, None, :], ln.shape)   # [B, H, R]


def decode_check(o, l, O, L, lens, what=""):
    """The tolerances of the contiguous decode tests (test_decode_kv16_gpu.py,
    test_quant_gpu.py::test_decode_split_kv), on the sequences that have keys."""
    live = [b for b, c in enumerate(lens) if c > 0]
    on, ln = o.cpu().numpy()[live], l.float().cpu().numpy()[live]
    eo, el = maxerr(on, O[live]), maxerr(ln, L[live])
    omax, lmax = max(1.0, float(np.abs(O[live]).max())), float(np.abs(L[live]).max())
    print(f"{what}: O err {eo:.3e} (bound {2e-3 * omax:.3e}) L err {el:.3e} "
          f"(bound {7e-3 + 2 ** -11 * lmax:.3e})")
    assert np.isfinite(on).all() and np.isfinite(ln).all()
    assert eo < 2e-3 * omax
    assert el < 7e-3 + 2 ** -11 * lmax


def prefill_check(o, l, O, L, pos, prec, what=""):
    """Rows with a visible key: test_forward_v2_gpu.py::check's bounds (O 5e-3 FP16 / 1e-2 BF16
    absolute; L 7e-3 plus half an FP16 ulp of |L| when L is stored in FP16).  The other rows:
    check_dead_rows."""
    on, ln, m = _rows(o, l, pos)
    check_dead_rows(on, ln, m, l.dtype == torch.float16, what)
    if not m.any():
        return
    tol_o = 5e-3 if prec == P.FP16 else 1e-2
    eo = maxerr(on[m], O[m])
    lr = L.astype(np.float64)[m]
    half_ulp = 0.5 * np.spacing(np.abs(lr).astype(np.float16)).astype(np.float64) \
        if l.dtype == torch.float16 else 0.0
    excess = float((np.abs(ln[m] - lr) - (7e-3 + half_ulp)).max())
    print(f"{what}: O err {eo:.3e} (bound {tol_o:.0e}); L error less its bound {excess:.3e}")
    assert np.isfinite(on[m]).all() and np.isfinite(ln[m]).all(), what
    assert eo <= tol_o, what
    assert excess <= 0, what


def mla_check(o, l, O, L, pos, prec, what=""):
    """Rows with a visible key: test_mla_absorbed_gpu.py's tolerances, O within 5e-2 (FP16) / 1e-1
    (BF16), L within 3e-2 / 1e-1.  The other rows: check_dead_rows."""
    on, ln, m = _rows(o, l, pos)
    check_dead_rows(on, ln, m, l.dtype == torch.float16, what)
    if not m.any():
        return
    tol_o, tol_l = (5e-2, 3e-2) if prec == P.FP16 else (1e-1, 1e-1)
    eo, el = maxerr(on[m], O[m]), maxerr(ln[m], L.astype(np.float64)[m])
    print(f"{what}: O err {eo:.3e} (bound {tol_o:.0e}); L err {el:.3e} (bound {tol_l:.0e})")
    assert np.isfinite(on[m]).all() and np.isfinite(ln[m]).all(), what
    assert eo < tol_o and el < tol_l, what


# ------------------------------------------------------------------- the K/V cases' data
def quantise(xs, scale, zp):
    """The INT8 bytes of one operand's sequences."""
    return [np.clip(np.rint(x / np.float32(scale)) + zp, -128, 127).astype(np.int8) for x in xs]


def _amax_scale(xs):
    return np.float32(max(float(np.abs(x).max()) for x in xs if x.size) / 120.0)


def _range_oracle(Q, K, V, b, hi):
    """The oracle on sequence b alone, row q's keys the half-open range [0, hi[q])."""
    ranges = np.zeros((1, K.shape[0], Q.shape[2], 2), np.uint32)
    ranges[0, :, :, 1] = hi.astype(np.uint32)[None, :]
    r = ol.attention(Q[b:b + 1], K[None], V[None], ranges=ranges)
    return r["O"][0], r["L"][0]


@functools.lru_cache(maxsize=None)
def decode_problem(B, H, Hkv, R, D, prec, lens, kv8=False, causal=False):
    """Stored-value Q [B, H, R, D], per-sequence K/V [Hkv, C_b, D] (what the kernel sees; INT8:
    also the bytes and scales) and the oracle's O / L per sequence, computed once per case."""
    rng = np.random.default_rng(R * 13 + sum(lens) + D)
    Q = seen(rng.standard_normal((B, H, R, D)).astype(np.float32), prec)
    raw = [[rng.standard_normal((Hkv, c, D)).astype(np.float32) for c in lens] for _ in range(2)]
    quant = None
    if kv8:
        quant = [(quantise(xs, s, ZP), float(s)) for xs, s in zip(raw, map(_amax_scale, raw))]
        Ks, Vs = ([(q.astype(np.float32) - ZP) * np.float32(s) for q in qs] for qs, s in quant)
    else:
        Ks, Vs = ([seen(x, prec) for x in xs] for xs in raw)
    O = np.zeros((B, H, R, D), np.float32)
    L = np.zeros((B, H, R), np.float32)
    for b, c in enumerate(lens):
        if c == 0:
            continue
        if not causal:
            r = ol.attention(Q[b:b + 1], Ks[b][None], Vs[b][None])
            O[b], L[b] = r["O"][0], r["L"][0]
            continue
        for q in range(R):  # row q sees the first c - R + q + 1 keys
            n = c - R + q + 1
            r = ol.attention(Q[b:b + 1, :, q:q + 1], Ks[b][None, :, :n], Vs[b][None, :, :n])
            O[b, :, q], L[b, :, q] = r["O"][0, :, 0], r["L"][0, :, 0]
    for a in [Q, O, L] + Ks + Vs:
        a.setflags(write=False)
    return Q, Ks, Vs, quant, O, L


@functools.lru_cache(maxsize=None)
def prefill_problem(B, H, Hkv, R, D, prec, lens, new_lens=None, causal=True, seed=0):
    """Stored-value Q [B, H, R, D], per-sequence K/V [Hkv, len_b, D], the oracle's O / L and the
    rows' key positions, computed once per case.  One oracle call per sequence."""
    rng = np.random.default_rng(seed + R * 13 + sum(lens) + D)
    Q = seen(rng.standard_normal((B, H, R, D)).astype(np.float32), prec)
    Ks, Vs = ([seen(rng.standard_normal((Hkv, max(c, 0), D)).astype(np.float32), prec)
               for c in lens] for _ in range(2))
    pos = positions(lens, new_lens, R)
    O = np.zeros((B, H, R, D), np.float32)
    L = np.zeros((B, H, R), np.float32)
    for b, c in enumerate(lens):
        if c <= 0 or not (pos[b] >= 0).any():
            continue
        hi = np.where(pos[b] >= 0, (pos[b] + 1) if causal else c, 0)
        O[b], L[b] = _range_oracle(Q, Ks[b], Vs[b], b, hi)
    for a in [Q, O, L, pos] + Ks + Vs:
        a.setflags(write=False)
    return Q, Ks, Vs, O, L, pos


@functools.lru_cache(maxsize=None)
def prefill8_problem(B, H, Hkv, R, D, prec, lens, new_lens=None, causal=True, seed=0, scales=None,
                     zps=(ZP, ZP), oracle=True):
    """Stored-value Q [B, H, R, D], the bytes of each sequence's K and V [Hkv, len_b, D] with
    their scales, and (oracle=True) the oracle's O / L on scale * (q - zp), once per sequence."""
    rng = np.random.default_rng(seed + R * 13 + sum(lens) + D)
    Q = seen(rng.standard_normal((B, H, R, D)).astype(np.float32), prec)
    raw = [[rng.standard_normal((Hkv, max(c, 0), D)).astype(np.float32) for c in lens]
           for _ in range(2)]
    if scales is None:
        scales = tuple(float(_amax_scale(xs)) for xs in raw)
    qk, qv = (quantise(xs, s, z) for xs, s, z in zip(raw, scales, zps))
    pos = positions(lens, new_lens, R)
    O = np.zeros((B, H, R, D), np.float32)
    L = np.zeros((B, H, R), np.float32)
    for b, c in enumerate(lens):
        if not oracle or c <= 0 or not (pos[b] >= 0).any():
            continue
        K, V = ((q[b].astype(np.float32) - z) * np.float32(s)
                for q, s, z in zip((qk, qv), scales, zps))
        hi = np.where(pos[b] >= 0, (pos[b] + 1) if causal else c, 0)
        O[b], L[b] = _range_oracle(Q, K, V, b, hi)
    for a in [Q, O, L, pos] + qk + qv:
        a.setflags(write=False)
    return Q, qk, qv, scales, O, L, pos


# Rows without a visible key: new_lens 0 and -3 (no row), seq_lens 0 (no key), new_lens 33 >
# seq_lens 20 (rows 0..12 lie before key 0, rows 33.. are not the sequence's), R + 9 (clamped).
DEAD_LENS, DEAD_NEW, DEAD_R = (50, 0, 20, 70, 90), (0, 10, 33, -3, 49), 40


# ----------------------------------------------------------------------------- the calls
def base_descriptor(prec, causal=False, W=None, lpi=None, scale=None):
    """W: the causal window (MFA_SPARSITY_CAUSAL_WINDOW), which stands in `causal`'s place."""
    return mfa.AttentionDescriptor.make(low_precision=True, precision=prec,
                                        causal=causal and W is None, causal_window=W,
                                        low_precision_intermediates=lpi, scale=scale)


def decode_descriptor(Q, Hkv, prec, max_seq_len, causal=False, lpi=None, W=None):
    B, H, R, D = Q.shape
    return mfa.PagedDecodeDescriptor.make(base_descriptor(prec, causal, W, lpi), B, H, R, D,
                                          max_seq_len, Hkv=Hkv)


def prefill_descriptor(shape, Hkv, prec, max_seq_len, causal=True, lpi=None, scale=None, W=None):
    B, H, R, D = shape
    return mfa.PagedPrefillDescriptor.make(base_descriptor(prec, causal, W, lpi, scale), B, H, R,
                                           D, max_seq_len, Hkv=Hkv)


def mla_descriptor(shape, latent, prec, max_seq_len, causal=True, lpi=None):
    B, H, R, D = shape
    return mfa.PagedMLADecodeDescriptor.make(base_descriptor(prec, causal, lpi=lpi), B, H, R, D,
                                             latent, max_seq_len, prec)


def nan_outputs(shape, l_dtype=torch.float16):
    B, H, R, D = shape
    return (torch.full((B, H, R, D), NAN, dtype=torch.float32, device=DEV),
            torch.full((B, H, R), NAN, dtype=l_dtype, device=DEV))


def decode_forward(Q, cache, prec, max_seq_len, causal=False, q=None, W=None):
    """One paged decode call on NaN-filled outputs; returns (O, L, launched kernel names)."""
    desc = decode_descriptor(Q, cache.Hkv, prec, max_seq_len, causal, W=W)
    q = to_device(Q, prec) if q is None else q
    o, l = nan_outputs(Q.shape)
    mfa.last_launches()
    mfa.paged_decode_forward(desc, q, cache.struct(), o, l)
    torch.cuda.synchronize()
    return o, l, [r["name"] for r in mfa.last_launches()]


def prefill_forward(Q, pc, Hkv, prec, max_seq_len, new_lens=None, causal=True, q=None,
                    q_strides=None, lpi=None, scale=None, W=None, call=None):
    """One paged prefill call (mfa.paged_prefill_forward unless `call` is given) on NaN-filled
    outputs; returns (O, L, the launch log, the descriptor)."""
    desc = prefill_descriptor(Q.shape, Hkv, prec, max_seq_len, causal, lpi, scale, W)
    q = to_device(Q, prec) if q is None else q
    o, l = nan_outputs(Q.shape, torch.float32 if lpi is False else torch.float16)
    mfa.last_launches()
    (call or mfa.paged_prefill_forward)(desc, q, pc, o, new_lens=i32(new_lens), logsumexp=l,
                                        query_strides=q_strides)
    torch.cuda.synchronize()
    return o, l, mfa.last_launches(), desc


def decode_kernel_form(H, Hkv, R):
    return "mfa_fwd_decode16_paged_kernel<" if (H // Hkv) * R <= 16 else "mfa_fwd_decode_paged_kernel<"


def prefill_kernel_name(prec, D, kv8=False, window=False):
    dp = 64 if D <= 64 else 128 if D <= 128 else 256
    return (f"mfa_paged_{'window_' if window else ''}prefill{'_kv8' if kv8 else ''}_kernel<"
            f"{tag(prec)}, {dp}, {32 if dp == 256 else 64}>")
