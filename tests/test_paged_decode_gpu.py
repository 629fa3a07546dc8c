"""GPU tests of the paged, ragged KV-cache decode (mfa_paged_decode_forward; attention_decode.hip
mfa_fwd_decode16_paged_kernel / mfa_fwd_decode_paged_kernel).  A dense per-sequence cache is
scattered into a pool through a shuffled block table; every pool slot that belongs to no
sequence (unused pages, slots past a sequence's length in its last page) holds NaN (INT8: byte
0x7f), so anything read from outside a sequence shows.  The reference is the oracle run per
sequence on that sequence's own keys, on the stored (rounded or dequantised) values, at the
tolerances of test_decode_kv16_gpu.py / test_quant_gpu.py::test_decode_split_kv."""
import functools

import numpy as np
import pytest
import torch

import mfa_amd as mfa
import oracle_lib as ol
from harness import TORCH_DTYPE, maxerr, seen, to_device

pytestmark = pytest.mark.gpu

P = mfa.Precision
DEV = "cuda:0"
ZP = 3  # zero point of the INT8 caches


@functools.lru_cache(maxsize=None)
def problem(B, H, Hkv, R, D, prec, lens, kv8=False, causal=False):
    """Stored-value Q [B, H, R, D], per-sequence K/V [Hkv, C_b, D] (what the kernel sees; INT8:
    also the bytes and scales) and the oracle's O / L per sequence, computed once per case."""
    rng = np.random.default_rng(R * 13 + sum(lens) + D)
    Q = seen(rng.standard_normal((B, H, R, D)).astype(np.float32), prec)
    raw = [[rng.standard_normal((Hkv, c, D)).astype(np.float32) for c in lens] for _ in range(2)]
    quant = None
    if kv8:
        quant, stored = [], []
        for xs in raw:
            s = np.float32(max(float(np.abs(x).max()) for x in xs if x.size) / 120.0)
            qs = [np.clip(np.rint(x / s) + ZP, -128, 127).astype(np.int8) for x in xs]
            quant.append((qs, float(s)))
            stored.append([(q.astype(np.float32) - ZP) * s for q in qs])
        Ks, Vs = stored
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


class Cache:
    """Device pools + block table + lengths of one scattered cache."""

    def __init__(self, Ks, Vs, prec, page, lens=None, quant=None, shuffle=True, spare=3, seed=1):
        B = len(Ks)
        Hkv, _, D = Ks[0].shape
        alloc = [k.shape[1] for k in Ks]
        npg = [-(-c // page) for c in alloc]
        self.max_pages = max(1, max(npg))
        self.num_pages = sum(npg) + spare
        ids = np.arange(self.num_pages)
        if shuffle:
            ids = np.random.default_rng(seed).permutation(self.num_pages)
        table = np.zeros((B, self.max_pages), np.int32)
        kv8 = quant is not None
        pools = []
        for xs in ((quant[0][0], quant[1][0]) if kv8 else (Ks, Vs)):
            pool = np.full((self.num_pages, Hkv, page, D), 0x7f if kv8 else np.nan,
                           np.int8 if kv8 else np.float32)
            nxt = 0
            for b in range(B):
                for j in range(npg[b]):
                    n = min(page, alloc[b] - j * page)
                    pool[ids[nxt], :, :n] = xs[b][:, j * page:j * page + n]
                    table[b, j] = ids[nxt]
                    nxt += 1
            pools.append(torch.from_numpy(pool).to(DEV) if kv8 else to_device(pool, prec))
        self.k, self.v = pools
        self.table = torch.from_numpy(table).to(DEV)
        self.lens = torch.tensor(alloc if lens is None else lens, dtype=torch.int32, device=DEV)
        self.prec, self.page, self.Hkv, self.D = (P.INT8 if kv8 else prec), page, Hkv, D
        self.scales = (quant[0][1], quant[1][1]) if kv8 else (1.0, 1.0)
        self.strides = None

    def struct(self):
        zp = ZP if self.prec == P.INT8 else 0
        return mfa.PagedKVCache.make(self.prec, self.page, self.max_pages, self.num_pages,
                                     self.Hkv, self.D, self.k, self.v, self.table, self.lens,
                                     strides=self.strides, k_scale=self.scales[0],
                                     v_scale=self.scales[1], k_zero_point=zp, v_zero_point=zp)


def descriptor(Q, Hkv, prec, max_seq_len, causal=False, lpi=None):
    B, H, R, D = Q.shape
    base = mfa.AttentionDescriptor.make(low_precision=True, precision=prec, causal=causal,
                                        low_precision_intermediates=lpi)
    return mfa.PagedDecodeDescriptor.make(base, B, H, R, D, max_seq_len, Hkv=Hkv)


def forward(Q, cache, prec, max_seq_len, causal=False, q=None):
    """One paged call; returns (O, L, launched kernel names)."""
    B, H, R, D = Q.shape
    desc = descriptor(Q, cache.Hkv, prec, max_seq_len, causal)
    q = to_device(Q, prec) if q is None else q
    o = torch.full((B, H, R, D), float("nan"), dtype=torch.float32, device=DEV)
    l = torch.full((B, H, R), float("nan"), dtype=torch.float16, device=DEV)
    mfa.last_launches()
    mfa.paged_decode_forward(desc, q, cache.struct(), o, l)
    torch.cuda.synchronize()
    return o, l, [r["name"] for r in mfa.last_launches()]


def check(o, l, O, L, lens, what=""):
    """The tolerances of the contiguous decode tests, on the sequences that have keys."""
    live = [b for b, c in enumerate(lens) if c > 0]
    on, ln = o.cpu().numpy()[live], l.float().cpu().numpy()[live]
    eo, el = maxerr(on, O[live]), maxerr(ln, L[live])
    omax, lmax = max(1.0, float(np.abs(O[live]).max())), float(np.abs(L[live]).max())
    print(f"{what}: O err {eo:.3e} (bound {2e-3 * omax:.3e}) L err {el:.3e} "
          f"(bound {7e-3 + 2 ** -11 * lmax:.3e})")
    assert np.isfinite(on).all() and np.isfinite(ln).all()
    assert eo < 2e-3 * omax
    assert el < 7e-3 + 2 ** -11 * lmax


def kernel_form(H, Hkv, R):
    return "mfa_fwd_decode16_paged_kernel<" if (H // Hkv) * R <= 16 else "mfa_fwd_decode_paged_kernel<"


CASES = [
    (3, 4, 4, 1, 128, P.FP16, 64, (1000, 33, 64)),   # two splits, a partial tile, an exact page end
    (2, 8, 2, 3, 64, P.BF16, 32, (777, 31)),         # GQA 12 rows, smallest page, less than a tile
    (2, 4, 1, 5, 256, P.FP16, 128, (300, 129)),      # MQA 20 rows: the 32-row form, D 256
    (1, 16, 1, 4, 128, P.FP16, 64, (300,)),          # 64 rows per kv head: two row tiles
    (1, 2, 2, 2, 72, P.FP16, 64, (200,)),            # D % 16 != 0
    (1, 4, 4, 7, 96, P.BF16, 64, (70,)),             # D 96 in the 128-wide tiles
    (2, 4, 2, 8, 128, P.FP16, 64, (2500, 70)),       # split path; later splits of seq 1 are empty
    (2, 2, 2, 1, 64, P.FP16, 256, (24000, 100)),     # > 32 splits: the 4-wave merge
]


def run_case(case, kv8=False, causal=False):
    B, H, Hkv, R, D, prec, page, lens = case
    Q, Ks, Vs, quant, O, L = problem(B, H, Hkv, R, D, prec, lens, kv8, causal)
    cache = Cache(Ks, Vs, prec, page, quant=quant)
    o, l, names = forward(Q, cache, prec, max(lens), causal)
    assert names[0].startswith(kernel_form(H, Hkv, R)), names
    assert names[0].endswith(", 1>" if kv8 else ", 0>"), names
    assert names[1:] in ([], ["mfa_decode_merge_kernel"], ["mfa_decode_merge4_kernel"]), names
    check(o, l, O, L, lens, f"{case} kv8={kv8} causal={causal} {names}")
    return o, l, names


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c[:5]) + f"-p{c[6]}")
def test_paged_decode(gpu, case):
    _, _, names = run_case(case)
    if case[7][0] == 24000:
        assert names[1:] == ["mfa_decode_merge4_kernel"], names
    elif case[7][0] == 2500:
        assert names[1:] == ["mfa_decode_merge_kernel"], names
    elif max(case[7]) < 512:   # fewer than 16 tiles: one split, merged in the workgroup
        assert len(names) == 1, names


@pytest.mark.parametrize("case", [CASES[0], CASES[2], CASES[6]],
                         ids=lambda c: "-".join(str(x) for x in c[:5]))
def test_paged_decode_int8(gpu, case):
    run_case(case, kv8=True)


def test_empty_sequence_gives_zero_rows(gpu):
    case = (2, 4, 2, 1, 128, P.FP16, 64, (500, 0))
    o, l, _ = run_case(case)
    assert torch.count_nonzero(o[1]).item() == 0          # exact zeros
    assert not torch.isnan(o).any() and not torch.isnan(l.float()).any()
    # (m, l) = (-FLT_MAX, 0) through the merge: L = -FLT_MAX + log2(FLT_MIN), -inf once in FP16.
    assert torch.isinf(l[1].float()).all() and (l[1].float() < 0).all()


@pytest.mark.parametrize("case", [
    (2, 4, 2, 4, 128, P.FP16, 64, (1000, 37)),
    (1, 8, 2, 8, 64, P.BF16, 32, (2500,)),           # 32 rows per kv head, split path
], ids=["16rows", "32rows-split"])
def test_paged_decode_causal(gpu, case):
    run_case(case, causal=True)


# ------------------------------------------------------------------ bit identity with the
# contiguous decode route: all lengths equal to C, max_seq_len = C: the same split layout and
# arithmetic order, whatever the table.
def contiguous_16bit(Q, K, V, prec, monkeypatch):
    B, H, R, D = Q.shape
    base = mfa.AttentionDescriptor.make(low_precision=True, precision=prec)
    desc = mfa.MultiHeadDescriptor.make(base, B, H, R, D, Hkv=K.shape[1], C=K.shape[2])
    o = torch.full((B, H, R, D), float("nan"), dtype=torch.float32, device=DEV)
    l = torch.full((B, H, R), float("nan"), dtype=torch.float16, device=DEV)
    monkeypatch.setenv("MFA_DECODE_KV16", "1")
    mfa.last_launches()
    mfa.MultiHeadAttention().forward(desc, to_device(Q, prec), to_device(K, prec),
                                     to_device(V, prec), o, l)
    torch.cuda.synchronize()
    names = [r["name"] for r in mfa.last_launches()]
    assert names[0].startswith("mfa_fwd_decode16_kernel<"), names
    return o, l, names


@pytest.mark.parametrize("shape,C", [((2, 4, 2, 8, 128), 2500), ((2, 4, 4, 1, 128), 1000),
                                     ((2, 4, 4, 1, 128), 300)],
                         ids=["split-5", "split-2", "fused"])
def test_bit_identical_to_contiguous_route(gpu, shape, C, monkeypatch):
    B, H, Hkv, R, D = shape
    prec = P.FP16
    Q, Ks, Vs, _, _, _ = problem(B, H, Hkv, R, D, prec, (C,) * B)
    o0, l0, names0 = contiguous_16bit(Q, np.stack(Ks), np.stack(Vs), prec, monkeypatch)
    for shuffle in (False, True):
        o, l, names = forward(Q, Cache(Ks, Vs, prec, 64, shuffle=shuffle), prec, C)
        assert [n.replace("_paged", "") for n in names] == names0, (names, names0)
        assert (len(names) == 1) == (C == 300), names
        assert torch.equal(o, o0) and torch.equal(l, l0), shuffle


def contiguous_int8(Q, quant, Hkv, C, prec):
    """The quantised entry on the dense INT8 cache; returns (O, L, launched kernel names)."""
    B, H, R, D = Q.shape
    base = mfa.AttentionDescriptor.make(R, C, D, low_precision_intermediates=True)
    desc = mfa.quantized_descriptor(base, prec, P.INT8, P.INT8, B=B, H=H, Hkv=Hkv)
    kq, vq = (torch.from_numpy(np.stack(q[0])).to(DEV) for q in quant)
    o0 = torch.full((B, H, R, D), float("nan"), dtype=torch.float32, device=DEV)
    l0 = torch.full((B, H, R), float("nan"), dtype=torch.float16, device=DEV)
    mfa.last_launches()
    mfa.QuantizedAttention().forward(
        desc, mfa.quantized_tensor(to_device(Q, prec), prec),
        mfa.quantized_tensor(kq, P.INT8, scale=quant[0][1], zero_point=ZP),
        mfa.quantized_tensor(vq, P.INT8, scale=quant[1][1], zero_point=ZP), o0, l0)
    torch.cuda.synchronize()
    return o0, l0, [r["name"] for r in mfa.last_launches()]


def test_int8_bit_identical_to_contiguous_route(gpu):
    B, H, Hkv, R, D, C, prec = 2, 4, 2, 8, 128, 2500, P.FP16
    Q, Ks, Vs, quant, _, _ = problem(B, H, Hkv, R, D, prec, (C,) * B, kv8=True)
    o0, l0, names0 = contiguous_int8(Q, quant, Hkv, C, prec)
    assert names0 == ["mfa_fwd_decode16_kernel<F16, 128, 1>", "mfa_decode_merge_kernel"], names0
    o, l, names = forward(Q, Cache(Ks, Vs, prec, 64, quant=quant), prec, C)
    assert names == ["mfa_fwd_decode16_paged_kernel<F16, 128, 1>", "mfa_decode_merge_kernel"], names
    assert torch.equal(o, o0) and torch.equal(l, l0)


@pytest.mark.parametrize("C", [2500, 300], ids=["split", "fused"])
def test_int8_32row_bit_identical_to_contiguous_route(gpu, C):
    # 20 rows per kv head: the 32-row form (the test above only reaches the 16-row one).
    B, H, Hkv, R, D, prec = 2, 4, 1, 5, 128, P.FP16
    Q, Ks, Vs, quant, _, _ = problem(B, H, Hkv, R, D, prec, (C,) * B, kv8=True)
    o0, l0, names0 = contiguous_int8(Q, quant, Hkv, C, prec)
    o, l, names = forward(Q, Cache(Ks, Vs, prec, 64, quant=quant), prec, C)
    assert names0[0].startswith("mfa_fwd_decode_kernel<"), names0
    assert names[0].startswith("mfa_fwd_decode_paged_kernel<"), names
    assert names0[0].endswith(", 1>") and names[0].endswith(", 1>"), (names0, names)
    assert names[1:] == names0[1:], (names, names0)
    assert names[1:] == (["mfa_decode_merge_kernel"] if C == 2500 else []), names
    assert torch.equal(o, o0) and torch.equal(l, l0)


def test_one_page_per_sequence_over_a_dense_bshd_cache(gpu):
    # Ragged lengths over a dense [B, C_alloc, H_kv, D] cache: page = the allocated length.
    B, H, Hkv, R, D, prec, lens, alloc = 2, 4, 2, 1, 128, P.FP16, (1000, 513), 1024
    Q, Ks, Vs, _, O, L = problem(B, H, Hkv, R, D, prec, lens)
    dense = []
    for xs in (Ks, Vs):
        t = np.full((B, alloc, Hkv, D), np.nan, np.float32)
        for b, c in enumerate(lens):
            t[b, :c] = xs[b].transpose(1, 0, 2)
        dense.append(to_device(t, prec))
    table = torch.arange(B, dtype=torch.int32, device=DEV).reshape(B, 1)
    lens_t = torch.tensor(lens, dtype=torch.int32, device=DEV)
    cache = mfa.PagedKVCache.make(prec, alloc, 1, B, Hkv, D, dense[0], dense[1], table, lens_t,
                                  strides=(alloc * Hkv * D, D, Hkv * D))
    o = torch.full((B, H, R, D), float("nan"), dtype=torch.float32, device=DEV)
    l = torch.full((B, H, R), float("nan"), dtype=torch.float16, device=DEV)
    mfa.paged_decode_forward(descriptor(Q, Hkv, prec, alloc), to_device(Q, prec), cache, o, l)
    torch.cuda.synchronize()
    check(o, l, O, L, lens, "one page per sequence")


def test_pool_beyond_2_31_bytes(gpu):
    # 128 KiB pages, 16400 of them (2.1 GiB per pool, untouched but for the used pages): the
    # sequence's three pages are the pool's last three, past a 32-bit byte offset.
    B, H, Hkv, R, D, prec, page, lens, num_pages = 1, 2, 1, 1, 256, P.FP16, 256, (700,), 16400
    Q, Ks, Vs, _, O, L = problem(B, H, Hkv, R, D, prec, lens)
    pools = []
    for xs in (Ks, Vs):
        pool = torch.empty((num_pages, Hkv, page, D), dtype=TORCH_DTYPE[prec], device=DEV)
        last = np.full((3, Hkv, page, D), np.nan, np.float32)
        for j in range(3):
            n = min(page, lens[0] - j * page)
            last[2 - j, :, :n] = xs[0][:, j * page:j * page + n]   # pages in descending order
        pool[num_pages - 3:] = to_device(last, prec)
        pools.append(pool)
    table = torch.tensor([[num_pages - 1, num_pages - 2, num_pages - 3]], dtype=torch.int32, device=DEV)
    lens_t = torch.tensor(lens, dtype=torch.int32, device=DEV)
    cache = mfa.PagedKVCache.make(prec, page, 3, num_pages, Hkv, D, pools[0], pools[1], table, lens_t)
    o = torch.full((B, H, R, D), float("nan"), dtype=torch.float32, device=DEV)
    l = torch.full((B, H, R), float("nan"), dtype=torch.float16, device=DEV)
    mfa.paged_decode_forward(descriptor(Q, Hkv, prec, lens[0]), to_device(Q, prec), cache, o, l)
    torch.cuda.synchronize()
    check(o, l, O, L, lens, "pool beyond 2^31 bytes")


def test_lengths_above_max_seq_len_are_clamped(gpu):
    B, H, Hkv, R, D, prec, lens = 2, 4, 2, 8, 128, P.FP16, (2500, 70)
    Q, Ks, Vs, _, O, L = problem(B, H, Hkv, R, D, prec, lens)
    cache = Cache(Ks, Vs, prec, 64)
    o, l, _ = forward(Q, cache, prec, 2500)
    cache.lens = torch.tensor([5000, 70], dtype=torch.int32, device=DEV)
    o2, l2, _ = forward(Q, cache, prec, 2500)
    assert torch.equal(o, o2) and torch.equal(l, l2)
    check(o2, l2, O, L, lens, "clamped")


def test_graph_replay_reads_new_lengths(gpu):
    # One captured call replayed with two sets of device lengths: each replay equals an eager call
    # with the same lengths bit for bit, and the oracle within tolerance.
    B, H, Hkv, R, D, prec, cap = 2, 8, 2, 1, 128, P.FP16, 2500
    Q, Ks, Vs, _, _, _ = problem(B, H, Hkv, R, D, prec, (cap, cap))
    cache = Cache(Ks, Vs, prec, 64)
    pc = cache.struct()
    desc = descriptor(Q, Hkv, prec, cap)
    q = to_device(Q, prec)
    o = torch.empty((B, H, R, D), dtype=torch.float32, device=DEV)
    l = torch.empty((B, H, R), dtype=torch.float16, device=DEV)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()

    def run():
        mfa.paged_decode_forward(desc, q, pc, o, l, stream=st.cuda_stream)

    with torch.cuda.stream(st):
        mfa.last_launches()
        run()   # the scratch does not grow during capture
        st.synchronize()
        names = [r["name"] for r in mfa.last_launches()]
        assert names == ["mfa_fwd_decode16_paged_kernel<F16, 128, 0>", "mfa_decode_merge_kernel"], names
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            run()
        for lens in ((900, 2400), (901, 2401)):
            cache.lens.copy_(torch.tensor(lens, dtype=torch.int32))
            o.fill_(float("nan"))
            l.fill_(float("nan"))
            run()
            st.synchronize()
            eo, el = o.clone(), l.clone()
            o.fill_(float("nan"))
            l.fill_(float("nan"))
            graph.replay()
            st.synchronize()
            assert torch.equal(o, eo) and torch.equal(l, el), lens
            ref = [ol.attention(Q[b:b + 1], Ks[b][None, :, :n], Vs[b][None, :, :n])
                   for b, n in enumerate(lens)]
            check(o, l, np.concatenate([r["O"] for r in ref]), np.concatenate([r["L"] for r in ref]),
                  lens, f"replay {lens}")


def test_launch_log_names_the_plan(gpu):
    for case in (CASES[0], CASES[2], CASES[6]):
        B, H, Hkv, R, D, prec, page, lens = case
        Q, Ks, Vs, _, _, _ = problem(B, H, Hkv, R, D, prec, lens)
        cache = Cache(Ks, Vs, prec, page)
        _, _, names = forward(Q, cache, prec, max(lens))
        plan = mfa.paged_decode_plan(descriptor(Q, Hkv, prec, max(lens)), cache.struct())
        assert names == [r["name"] for r in plan], (names, plan)
