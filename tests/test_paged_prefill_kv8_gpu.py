"""GPU tests of the paged prefill over INT8 pools (mfa_quantized_paged_prefill_forward;
attention_prefill_paged_kv8.hip mfa_paged_prefill_kv8_kernel).  The caches are built as
test_paged_decode_gpu.py builds its INT8 ones (scale = amax / 120, zero point 3, byte 0x7f in
every slot no sequence owns) and scattered through a shuffled block table with spare pages, as
test_paged_prefill_gpu.py scatters its 16-bit ones; output and logsumexp hold NaN before every
call.  The reference is the oracle, once per sequence, on the stored Q and on K/V given as FP32
scale * (q - zp), row q's keys the half-open range [0, t_q + 1); the bounds are
test_paged_prefill_gpu.py::check's, unchanged — the operands after widening are exact, so the
error sources are the 16-bit kernel's.  Beyond the oracle: the result equals, bit for bit, the
16-bit call on a pool holding q - zp (power-of-two scales make both foldings exact)."""
import numpy as np
import pytest
import torch

import mfa_amd as mfa
import oracle_lib as ol
from harness import seen, to_device
from paged_rig import DEAD_LENS, DEAD_NEW, DEAD_R, DEV, ZP, Cache, Cache8, P, decode_check, i32
from paged_rig import positions, prefill8_problem, prefill_check, prefill_descriptor
from paged_rig import prefill_forward, prefill_kernel_name, prefill_problem

pytestmark = pytest.mark.gpu


def forward(Q, pc, Hkv, prec, max_seq_len, new_lens=None, causal=True, lpi=None, scale=None,
            call=None):
    """One call (the new entry point unless `call` is given) on NaN-filled outputs; returns
    (O, L, launched kernel names).  INT8 caches: the launch log must equal the plan."""
    B, H, R, _ = Q.shape
    o, l, log, desc = prefill_forward(Q, pc, Hkv, prec, max_seq_len, new_lens, causal, lpi=lpi,
                                      scale=scale,
                                      call=call or mfa.quantized_paged_prefill_forward)
    if call is None and pc.precision == P.INT8:
        plan = mfa.quantized_paged_prefill_plan(desc, pc)
        assert [(r["name"], r["threads"], r["lds_bytes"], r["workgroups"]) for r in log] == \
               [(r["name"], r["threads"], r["lds_bytes"], r["workgroups"]) for r in plan], (log, plan)
        assert plan[0]["workgroups"] == B * H * -(-R // 128)
    return o, l, [r["name"] for r in log]


def kernel_name(prec, D):
    return prefill_kernel_name(prec, D, kv8=True)


def run_case(B, H, Hkv, R, D, prec, page, lens, new_lens=None, causal=True, lpi=None, **kw):
    Q, qk, qv, scales, O, L, pos = prefill8_problem(B, H, Hkv, R, D, prec, lens, new_lens, causal)
    cache = Cache8(qk, qv, page, scales, **kw)
    o, l, names = forward(Q, cache.struct(), Hkv, prec, max(max(lens), 1), new_lens, causal, lpi)
    assert names == [kernel_name(prec, D)], names
    prefill_check(o, l, O, L, pos, prec,
                  f"kv8 B{B} H{H}/{Hkv} R{R} D{D} page {page} lens {lens} new {new_lens} lpi {lpi}")
    return o, l


# a. A prefix; a pure prompt; a chunk smaller than a wave in a partial second block; a length
#    that ends mid-page.
RAGGED = (3, 4, 2, 160, 128, P.FP16, 64, (300, 160, 97), (160, 160, 33))


def test_ragged_causal_fp16(gpu):
    run_case(*RAGGED)


# b. The smallest page: the two segments of a tile come from distant pages.
def test_bf16_smallest_page(gpu):
    run_case(2, 8, 2, 70, 64, P.BF16, 32, (200, 31), (70, 31), spare=40, seed=5)


# c. D 256 (32-key tiles), MQA, two row blocks.
def test_fp16_d256_mqa(gpu):
    run_case(2, 4, 1, 130, 256, P.FP16, 128, (260, 129), None)


# d. Head dimensions that are not a tile width but are INT8-legal.
@pytest.mark.parametrize("D,prec", [(80, P.FP16), (96, P.BF16)])
def test_odd_head_dims(gpu, D, prec):
    run_case(1, 2, 2, 45, D, prec, 64, (77,), (45,))


# e. No mask.
def test_unmasked(gpu):
    run_case(2, 4, 2, 140, 128, P.FP16, 64, (200, 150), (140, 20), causal=False)


# f. Rows without a visible key.
@pytest.mark.parametrize("lpi", [None, False], ids=["L-fp16", "L-fp32"])
def test_dead_rows(gpu, lpi):
    B, H, Hkv, R, D, prec, page = 5, 2, 1, DEAD_R, 64, P.FP16, 32
    Q, qk, qv, scales, O, L, pos = prefill8_problem(B, H, Hkv, R, D, prec, DEAD_LENS, DEAD_NEW)
    assert [(p >= 0).sum() for p in pos] == [0, 0, 20, 0, R]
    o, l, _ = forward(Q, Cache8(qk, qv, page, scales).struct(), Hkv, prec, 90, DEAD_NEW, lpi=lpi)
    prefill_check(o, l, O, L, pos, prec, f"kv8 dead rows lpi={lpi}")


# g. The pool is decoded exactly: with power-of-two scales the new call equals, bit for bit, the
#    16-bit call on a pool holding float(q - zp) at softmax scale scale * k_scale, times v_scale.
@pytest.mark.parametrize("vzp", [-128, 128])
@pytest.mark.parametrize("prec,D", [(P.FP16, 64), (P.FP16, 128), (P.FP16, 256), (P.BF16, 128)],
                         ids=["f16-64", "f16-128", "f16-256", "bf16-128"])
def test_exact_decode_of_the_pool(gpu, prec, D, vzp):
    B, H, Hkv, R, _, _, page, lens, new = RAGGED
    ks, vs, zps = 2.0 ** -5, 2.0 ** -4, (3, vzp)
    Q, qk, qv, _, _, _, _ = prefill8_problem(B, H, Hkv, R, D, prec, lens, new, scales=(ks, vs), zps=zps,
                                             oracle=False)
    assert any((q == (-128 if vzp < 0 else 127)).any() for q in qv)   # the far end of the range
    scale = np.float32(D ** -0.5)
    o8, l8, n8 = forward(Q, Cache8(qk, qv, page, (ks, vs), zps).struct(), Hkv, prec, 300, new,
                         scale=float(scale))
    assert n8 == [kernel_name(prec, D)]
    ints = [[q.astype(np.float32) - z for q in qs] for qs, z in zip((qk, qv), zps)]
    assert all(np.array_equal(seen(x, prec), x) for xs in ints for x in xs)   # exact in 16 bits
    c16 = Cache(ints[0], ints[1], prec, page)
    o16, l16, n16 = forward(Q, c16.struct(), Hkv, prec, 300, new,
                            scale=float(scale * np.float32(ks)), call=mfa.paged_prefill_forward)
    assert n16 == [prefill_kernel_name(prec, D)]
    assert not torch.isnan(o8).any() and not torch.isnan(l8.float()).any()
    assert torch.equal(o8, o16 * vs)
    assert torch.equal(l8, l16)


# h. The arithmetic does not depend on the paging.
def test_bit_identical_across_pagings(gpu):
    B, H, Hkv, R, D, prec, lens, new = 2, 4, 2, 160, 128, P.FP16, (300, 97), (160, 33)
    Q, qk, qv, scales, O, L, pos = prefill8_problem(B, H, Hkv, R, D, prec, lens, new)
    o0, l0, _ = forward(Q, Cache8(qk, qv, 32, scales, spare=9, seed=3).struct(), Hkv, prec, 300, new)
    prefill_check(o0, l0, O, L, pos, prec, "kv8 page 32")
    o1, l1, _ = forward(Q, Cache8(qk, qv, 256, scales, shuffle=False).struct(), Hkv, prec, 300, new)
    assert torch.equal(o0, o1) and torch.equal(l0, l1)
    # One page per sequence over a dense [B, C_alloc, H_kv, D] tensor.
    alloc, dense = 512, []
    for xs in (qk, qv):
        t = np.full((B, alloc, Hkv, D), 0x7f, np.int8)
        for b, c in enumerate(lens):
            t[b, :c] = xs[b].transpose(1, 0, 2)
        dense.append(torch.from_numpy(t).to(DEV))
    table = torch.arange(B, dtype=torch.int32, device=DEV).reshape(B, 1)
    pc = mfa.PagedKVCache.make(P.INT8, alloc, 1, B, Hkv, D, dense[0], dense[1], table, i32(lens),
                               strides=(alloc * Hkv * D, D, Hkv * D), k_scale=scales[0],
                               v_scale=scales[1], k_zero_point=ZP, v_zero_point=ZP)
    o2, l2, _ = forward(Q, pc, Hkv, prec, 300, new)
    assert torch.equal(o0, o2) and torch.equal(l0, l2)


# i. Nothing outside a sequence reaches the result: neither the bytes of unused slots and spare
#    pages, nor the table entries of logical pages no key lies in.
def test_nothing_outside_a_sequence_is_read(gpu):
    B, H, Hkv, R, D, prec, page, lens, new = 2, 4, 2, 70, 64, P.FP16, 32, (200, 31), (70, 31)
    Q, qk, qv, scales, O, L, pos = prefill8_problem(B, H, Hkv, R, D, prec, lens, new)
    clean = Cache8(qk, qv, page, scales)
    o0, l0, _ = forward(Q, clean.struct(), Hkv, prec, 200, new)
    prefill_check(o0, l0, O, L, pos, prec, "kv8 fill 0x7f")
    noisy = Cache8(qk, qv, page, scales, fill="random")
    assert not torch.equal(clean.k, noisy.k) and torch.equal(clean.table, noisy.table)
    o1, l1, _ = forward(Q, noisy.struct(), Hkv, prec, 200, new)
    assert torch.equal(o0, o1) and torch.equal(l0, l1)
    for fill in (-7, clean.num_pages + 5):
        dirty = Cache8(qk, qv, page, scales, fill="random", table_fill=fill)
        assert (dirty.table_np == fill).sum() >= 7
        o2, l2, _ = forward(Q, dirty.struct(), Hkv, prec, 200, new)
        assert torch.equal(o0, o2) and torch.equal(l0, l2), fill
    # The same at D 128, whose chunk geometry differs (16-byte chunks; two segments per tile).
    B, H, Hkv, R, D, prec, page, lens, new = RAGGED
    Q, qk, qv, scales, _, _, _ = prefill8_problem(B, H, Hkv, R, D, prec, lens, new)
    a = forward(Q, Cache8(qk, qv, page, scales).struct(), Hkv, prec, 300, new)
    b = forward(Q, Cache8(qk, qv, page, scales, fill="random", table_fill=-7).struct(), Hkv, prec,
                300, new)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# j. Append, prefill and decode over one cache struct.
def test_round_trip_with_the_writer(gpu):
    B, H, Hkv, R, D, prec, page = 3, 4, 2, 96, 128, P.FP16, 64
    lens, new = (250, 96, 40), (96, 96, 7)
    rng = np.random.default_rng(4)
    Q = seen(rng.standard_normal((B, H, R, D)).astype(np.float32), prec)
    raw = [[seen(rng.standard_normal((Hkv, c, D)).astype(np.float32), prec) for c in lens]
           for _ in range(2)]
    scales = tuple(float(np.float32(max(float(np.abs(x).max()) for x in xs) / 120.0)) for xs in raw)
    # The writer's documented bytes, by the same formula on the host.
    qk, qv = ([ol.quantize(x, ol.INT8, s, ZP).view(np.int8).reshape(x.shape) for x in xs]
              for xs, s in zip(raw, scales))
    pos = positions(lens, new, R)
    O, L = np.zeros((B, H, R, D), np.float32), np.zeros((B, H, R), np.float32)
    for b in range(B):
        K, V = ((q[b].astype(np.float32) - ZP) * np.float32(s) for q, s in zip((qk, qv), scales))
        ranges = np.zeros((1, Hkv, R, 2), np.uint32)
        ranges[0, :, :, 1] = np.where(pos[b] >= 0, pos[b] + 1, 0).astype(np.uint32)[None, :]
        r = ol.attention(Q[b:b + 1], K[None], V[None], ranges=ranges)
        O[b], L[b] = r["O"][0], r["L"][0]
    # The cache before the chunk: the prefixes scattered by the host, 0x7f everywhere else.
    cache = Cache8(qk, qv, page, scales)
    for b in range(B):
        for t in range(lens[b] - new[b], lens[b]):
            cache.k[cache.table_np[b, t // page], :, t % page] = 0x7f
            cache.v[cache.table_np[b, t // page], :, t % page] = 0x7f
    kn, vn = (np.zeros((B, Hkv, R, D), np.float32) for _ in range(2))
    for b in range(B):
        kn[b, :, :new[b]] = raw[0][b][:, lens[b] - new[b]:]
        vn[b, :, :new[b]] = raw[1][b][:, lens[b] - new[b]:]
    pc, nl = cache.struct(), i32(new)
    mfa.paged_kv_append(mfa.PagedAppendDescriptor.make(prec, B, Hkv, R, D, 256),
                        to_device(kn, prec), to_device(vn, prec), pc, new_lens=nl)
    o, l, _ = forward(Q, pc, Hkv, prec, 256, new)
    prefill_check(o, l, O, L, pos, prec, "kv8 append -> prefill")
    # The decode call over the same lengths at uniform R = min(new): the last rows of each chunk.
    Rd = min(new)
    rows = [slice(n - Rd, n) for n in new]
    qd = np.stack([Q[b][:, rows[b]] for b in range(B)])
    Od = np.stack([O[b][:, rows[b]] for b in range(B)])
    Ld = np.stack([L[b][:, rows[b]] for b in range(B)])
    base = mfa.AttentionDescriptor.make(low_precision=True, precision=prec, causal=True)
    od = torch.full((B, H, Rd, D), float("nan"), dtype=torch.float32, device=DEV)
    ld = torch.full((B, H, Rd), float("nan"), dtype=torch.float16, device=DEV)
    mfa.paged_decode_forward(mfa.PagedDecodeDescriptor.make(base, B, H, Rd, D, 256, Hkv=Hkv),
                             to_device(qd, prec), pc, od, ld)
    torch.cuda.synchronize()
    decode_check(od, ld, Od, Ld, lens, "kv8 decode rows")


# k. lens += n, append, prefill as one linear graph, replayed with new device values.
def test_graph_replay_reads_new_lengths_and_rows(gpu):
    B, H, Hkv, R, D, prec, page, cap = 2, 4, 2, 72, 128, P.FP16, 64, 384
    rng = np.random.default_rng(12)
    max_pages, num_pages = cap // page, 2 * (cap // page) + 3
    # Bytes in every slot: what a step does not append is the prefix it reads.
    k, v = (torch.from_numpy(rng.integers(-128, 128, (num_pages, Hkv, page, D), dtype=np.int8)).to(DEV)
            for _ in range(2))
    table = torch.from_numpy(rng.permutation(num_pages)[:B * max_pages].reshape(B, max_pages)
                             .astype(np.int32)).to(DEV)
    lens, nl = i32((0, 0)), i32((0, 0))
    pc = mfa.PagedKVCache.make(P.INT8, page, max_pages, num_pages, Hkv, D, k, v, table, lens,
                               k_scale=0.03, v_scale=0.04, k_zero_point=3, v_zero_point=-5)
    q, kn, vn = (to_device(rng.standard_normal((B, h, R, D)).astype(np.float32), prec)
                 for h in (H, Hkv, Hkv))
    desc = prefill_descriptor((B, H, R, D), Hkv, prec, cap)
    adesc = mfa.PagedAppendDescriptor.make(prec, B, Hkv, R, D, cap)
    o = torch.empty((B, H, R, D), dtype=torch.float32, device=DEV)
    l = torch.empty((B, H, R), dtype=torch.float16, device=DEV)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()

    def step():
        lens.add_(nl)
        mfa.paged_kv_append(adesc, kn, vn, pc, new_lens=nl, stream=st.cuda_stream)
        mfa.quantized_paged_prefill_forward(desc, q, pc, o, new_lens=nl, logsumexp=l,
                                            stream=st.cuda_stream)

    with torch.cuda.stream(st):
        step()   # warm-up outside the capture
        st.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            step()
        for before, new in (((100, 0), (72, 30)), ((250, 31), (5, 72)), ((300, 0), (0, 1))):
            got = []
            for run in (step, graph.replay):
                lens.copy_(torch.tensor(before, dtype=torch.int32))
                nl.copy_(torch.tensor(new, dtype=torch.int32))
                o.fill_(float("nan"))
                l.fill_(float("nan"))
                run()
                st.synchronize()
                assert lens.tolist() == [a + b for a, b in zip(before, new)]
                got.append((o.clone(), l.clone()))
            assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1]), new
            assert not torch.isnan(got[1][0]).any() and not torch.isnan(got[1][1].float()).any()
            pos = positions([a + b for a, b in zip(before, new)], new, R)
            dead = torch.from_numpy(pos < 0).to(DEV)[:, None, :].expand(B, H, R)
            assert torch.count_nonzero(got[1][0][dead]).item() == 0
            assert torch.isneginf(got[1][1].float()[dead]).all()
            assert torch.isfinite(got[1][1].float()[~dead]).all()


# l. 16-bit pools through the new entry point: the sibling's launch and the sibling's bits.
@pytest.mark.parametrize("prec,D", [(P.FP16, 128), (P.BF16, 64), (P.FP16, 72)])
def test_16_bit_pools_take_the_siblings_path(gpu, prec, D):
    B, H, Hkv, R, _, _, page, lens, new = RAGGED
    Q, Ks, Vs, _, _, _ = prefill_problem(B, H, Hkv, R, D, prec, lens, new)
    pc = Cache(Ks, Vs, prec, page).struct()
    o0, l0, n0 = forward(Q, pc, Hkv, prec, 300, new, call=mfa.paged_prefill_forward)
    o1, l1, n1 = forward(Q, pc, Hkv, prec, 300, new)
    assert n0 == n1 == [prefill_kernel_name(prec, D)]
    assert not torch.isnan(o1).any()
    assert torch.equal(o0, o1) and torch.equal(l0, l1)
