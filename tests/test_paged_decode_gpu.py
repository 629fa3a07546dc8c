"""GPU tests of the paged, ragged KV-cache decode (mfa_paged_decode_forward; attention_decode.hip
mfa_fwd_decode16_paged_kernel / mfa_fwd_decode_paged_kernel).  A dense per-sequence cache is
scattered into a pool through a shuffled block table; every pool slot that belongs to no
sequence (unused pages, slots past a sequence's length in its last page) holds NaN (INT8: byte
0x7f), so anything read from outside a sequence shows.  The reference is the oracle run per
sequence on that sequence's own keys, on the stored (rounded or dequantised) values, at the
tolerances of test_decode_kv16_gpu.py / test_quant_gpu.py::test_decode_split_kv."""
import numpy as np
import pytest
import torch

import mfa_amd as mfa
import oracle_lib as ol
from harness import TORCH_DTYPE, to_device
from paged_rig import DEV, ZP, Cache, P, cache_of, i32
from paged_rig import decode_check, decode_descriptor, decode_forward, decode_kernel_form
from paged_rig import decode_problem

pytestmark = pytest.mark.gpu


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
    Q, Ks, Vs, quant, O, L = decode_problem(B, H, Hkv, R, D, prec, lens, kv8, causal)
    cache = cache_of(Ks, Vs, prec, page, quant)
    o, l, names = decode_forward(Q, cache, prec, max(lens), causal)
    assert names[0].startswith(decode_kernel_form(H, Hkv, R)), names
    assert names[0].endswith(", 1>" if kv8 else ", 0>"), names
    assert names[1:] in ([], ["mfa_decode_merge_kernel"], ["mfa_decode_merge4_kernel"]), names
    decode_check(o, l, O, L, lens, f"{case} kv8={kv8} causal={causal} {names}")
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
    Q, Ks, Vs, _, _, _ = decode_problem(B, H, Hkv, R, D, prec, (C,) * B)
    o0, l0, names0 = contiguous_16bit(Q, np.stack(Ks), np.stack(Vs), prec, monkeypatch)
    for shuffle in (False, True):
        o, l, names = decode_forward(Q, Cache(Ks, Vs, prec, 64, shuffle=shuffle), prec, C)
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
    Q, Ks, Vs, quant, _, _ = decode_problem(B, H, Hkv, R, D, prec, (C,) * B, kv8=True)
    o0, l0, names0 = contiguous_int8(Q, quant, Hkv, C, prec)
    assert names0 == ["mfa_fwd_decode16_kernel<F16, 128, 1>", "mfa_decode_merge_kernel"], names0
    o, l, names = decode_forward(Q, cache_of(Ks, Vs, prec, 64, quant), prec, C)
    assert names == ["mfa_fwd_decode16_paged_kernel<F16, 128, 1>", "mfa_decode_merge_kernel"], names
    assert torch.equal(o, o0) and torch.equal(l, l0)


@pytest.mark.parametrize("C", [2500, 300], ids=["split", "fused"])
def test_int8_32row_bit_identical_to_contiguous_route(gpu, C):
    # 20 rows per kv head: the 32-row form (the test above only reaches the 16-row one).
    B, H, Hkv, R, D, prec = 2, 4, 1, 5, 128, P.FP16
    Q, Ks, Vs, quant, _, _ = decode_problem(B, H, Hkv, R, D, prec, (C,) * B, kv8=True)
    o0, l0, names0 = contiguous_int8(Q, quant, Hkv, C, prec)
    o, l, names = decode_forward(Q, cache_of(Ks, Vs, prec, 64, quant), prec, C)
    assert names0[0].startswith("mfa_fwd_decode_kernel<"), names0
    assert names[0].startswith("mfa_fwd_decode_paged_kernel<"), names
    assert names0[0].endswith(", 1>") and names[0].endswith(", 1>"), (names0, names)
    assert names[1:] == names0[1:], (names, names0)
    assert names[1:] == (["mfa_decode_merge_kernel"] if C == 2500 else []), names
    assert torch.equal(o, o0) and torch.equal(l, l0)


def test_one_page_per_sequence_over_a_dense_bshd_cache(gpu):
    # Ragged lengths over a dense [B, C_alloc, H_kv, D] cache: page = the allocated length.
    B, H, Hkv, R, D, prec, lens, alloc = 2, 4, 2, 1, 128, P.FP16, (1000, 513), 1024
    Q, Ks, Vs, _, O, L = decode_problem(B, H, Hkv, R, D, prec, lens)
    dense = []
    for xs in (Ks, Vs):
        t = np.full((B, alloc, Hkv, D), np.nan, np.float32)
        for b, c in enumerate(lens):
            t[b, :c] = xs[b].transpose(1, 0, 2)
        dense.append(to_device(t, prec))
    table = torch.arange(B, dtype=torch.int32, device=DEV).reshape(B, 1)
    lens_t = i32(lens)
    cache = mfa.PagedKVCache.make(prec, alloc, 1, B, Hkv, D, dense[0], dense[1], table, lens_t,
                                  strides=(alloc * Hkv * D, D, Hkv * D))
    o = torch.full((B, H, R, D), float("nan"), dtype=torch.float32, device=DEV)
    l = torch.full((B, H, R), float("nan"), dtype=torch.float16, device=DEV)
    mfa.paged_decode_forward(decode_descriptor(Q, Hkv, prec, alloc), to_device(Q, prec), cache, o, l)
    torch.cuda.synchronize()
    decode_check(o, l, O, L, lens, "one page per sequence")


def test_pool_beyond_2_31_bytes(gpu):
    # 128 KiB pages, 16400 of them (2.1 GiB per pool, untouched but for the used pages): the
    # sequence's three pages are the pool's last three, past a 32-bit byte offset.
    B, H, Hkv, R, D, prec, page, lens, num_pages = 1, 2, 1, 1, 256, P.FP16, 256, (700,), 16400
    Q, Ks, Vs, _, O, L = decode_problem(B, H, Hkv, R, D, prec, lens)
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
    lens_t = i32(lens)
    cache = mfa.PagedKVCache.make(prec, page, 3, num_pages, Hkv, D, pools[0], pools[1], table, lens_t)
    o = torch.full((B, H, R, D), float("nan"), dtype=torch.float32, device=DEV)
    l = torch.full((B, H, R), float("nan"), dtype=torch.float16, device=DEV)
    mfa.paged_decode_forward(decode_descriptor(Q, Hkv, prec, lens[0]), to_device(Q, prec), cache, o, l)
    torch.cuda.synchronize()
    decode_check(o, l, O, L, lens, "pool beyond 2^31 bytes")


def test_lengths_above_max_seq_len_are_clamped(gpu):
    B, H, Hkv, R, D, prec, lens = 2, 4, 2, 8, 128, P.FP16, (2500, 70)
    Q, Ks, Vs, _, O, L = decode_problem(B, H, Hkv, R, D, prec, lens)
    cache = Cache(Ks, Vs, prec, 64)
    o, l, _ = decode_forward(Q, cache, prec, 2500)
    cache.lens = i32((5000, 70))
    o2, l2, _ = decode_forward(Q, cache, prec, 2500)
    assert torch.equal(o, o2) and torch.equal(l, l2)
    decode_check(o2, l2, O, L, lens, "clamped")


def test_graph_replay_reads_new_lengths(gpu):
    # One captured call replayed with two sets of device lengths: each replay equals an eager call
    # with the same lengths bit for bit, and the oracle within tolerance.
    B, H, Hkv, R, D, prec, cap = 2, 8, 2, 1, 128, P.FP16, 2500
    Q, Ks, Vs, _, _, _ = decode_problem(B, H, Hkv, R, D, prec, (cap, cap))
    cache = Cache(Ks, Vs, prec, 64)
    pc = cache.struct()
    desc = decode_descriptor(Q, Hkv, prec, cap)
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
            decode_check(o, l, np.concatenate([r["O"] for r in ref]),
                         np.concatenate([r["L"] for r in ref]), lens, f"replay {lens}")


def test_launch_log_names_the_plan(gpu):
    for case in (CASES[0], CASES[2], CASES[6]):
        B, H, Hkv, R, D, prec, page, lens = case
        Q, Ks, Vs, _, _, _ = decode_problem(B, H, Hkv, R, D, prec, lens)
        cache = Cache(Ks, Vs, prec, page)
        _, _, names = decode_forward(Q, cache, prec, max(lens))
        plan = mfa.paged_decode_plan(decode_descriptor(Q, Hkv, prec, max(lens)), cache.struct())
        assert names == [r["name"] for r in plan], (names, plan)
