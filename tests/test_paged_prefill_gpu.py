"""GPU tests of the paged prefill (mfa_paged_prefill_forward; attention_prefill_paged.hip
mfa_paged_prefill_kernel).  A dense per-sequence cache is scattered into a pool through a shuffled
block table with spare pages; every pool slot that belongs to no sequence (unused pages, slots
past a sequence's length in its last page) holds NaN, and so do output and logsumexp before the
call, so anything read from outside a sequence, and any row left unwritten, shows.  The reference
is the oracle run once per sequence on the stored (rounded) values, row q's keys given as the
half-open range [0, t_q + 1); rows with a visible key are compared at the tolerances of
test_forward_v2_gpu.py::check (the same tile body, the same unit-Gaussian data), the others must
be exact zeros with L at its floor."""
import numpy as np
import pytest
import torch

import mfa_amd as mfa
from harness import TORCH_DTYPE, to_device
from paged_rig import DEAD_LENS, DEAD_NEW, DEAD_R, DEV, Cache, P, decode_check, i32, positions
from paged_rig import prefill_check, prefill_descriptor, prefill_forward, prefill_kernel_name
from paged_rig import prefill_problem

pytestmark = pytest.mark.gpu


def forward(*args, **kw):
    """One call on NaN-filled outputs; returns (O, L, launched kernel names)."""
    o, l, log, _ = prefill_forward(*args, **kw)
    return o, l, [r["name"] for r in log]


def run_case(B, H, Hkv, R, D, prec, page, lens, new_lens=None, causal=True, **kw):
    Q, Ks, Vs, O, L, pos = prefill_problem(B, H, Hkv, R, D, prec, lens, new_lens, causal)
    cache = Cache(Ks, Vs, prec, page, **kw)
    o, l, names = forward(Q, cache.struct(), Hkv, prec, max(max(lens), 1), new_lens, causal)
    assert names == [prefill_kernel_name(prec, D)], names
    prefill_check(o, l, O, L, pos, prec,
                  f"B{B} H{H}/{Hkv} R{R} D{D} page {page} lens {lens} new {new_lens}")
    return o, l


# 1. A prefix; a pure prompt (n == len); a chunk smaller than a wave in a second, partial 128-row
#    block's batch; a partial last tile; a length that ends mid-page.
RAGGED = (3, 4, 2, 160, 128, P.FP16, 64, (300, 160, 97), (160, 160, 33))


def test_ragged_causal_fp16(gpu):
    run_case(*RAGGED)


# 2. The smallest page: a 64-key tile's two segments come from two pages, far apart once shuffled.
def test_bf16_smallest_page(gpu):
    run_case(2, 8, 2, 70, 64, P.BF16, 32, (200, 31), (70, 31), spare=40, seed=5)


# 3. D 256 (32-key tiles), MQA, two row blocks.
def test_fp16_d256_mqa(gpu):
    run_case(2, 4, 1, 130, 256, P.FP16, 128, (260, 129), None)


# 4. Head dimensions that are not a tile width.
@pytest.mark.parametrize("D,prec", [(72, P.FP16), (96, P.BF16)])
def test_odd_head_dims(gpu, D, prec):
    run_case(1, 2, 2, 45, D, prec, 64, (77,), (45,))


# 5. No mask: every live row sees all len_b keys.
def test_unmasked(gpu):
    run_case(2, 4, 2, 140, 128, P.FP16, 64, (200, 150), (140, 20), causal=False)


# 6. Rows without a visible key (paged_rig.DEAD_LENS / DEAD_NEW).
@pytest.mark.parametrize("lpi", [None, False], ids=["L-fp16", "L-fp32"])
def test_dead_rows(gpu, lpi):
    B, H, Hkv, R, D, prec, page = 5, 2, 1, DEAD_R, 64, P.FP16, 32
    Q, Ks, Vs, O, L, pos = prefill_problem(B, H, Hkv, R, D, prec, DEAD_LENS, DEAD_NEW)
    # new_lens 0 and -3: no row; seq_lens 0: no key; new_lens 33 > seq_lens 20: rows 0..12 lie
    # before key 0 and rows 33.. are not the sequence's; R + 9 is clamped to R.
    assert [(p >= 0).sum() for p in pos] == [0, 0, 20, 0, R]
    assert pos[2, 13] == 0 and pos[2, 32] == 19 and pos[4, 0] == 50
    o, l, _ = forward(Q, Cache(Ks, Vs, prec, page).struct(), Hkv, prec, 90, DEAD_NEW, lpi=lpi)
    prefill_check(o, l, O, L, pos, prec, f"dead rows lpi={lpi}")


def test_lengths_above_the_cap_are_clamped(gpu):
    # Caches of 96 and 64 keys, cap 64 (max_seq_len): lengths (500, 64) read as (64, 64).
    B, H, Hkv, R, D, prec, page = 2, 2, 1, 40, 64, P.FP16, 32
    Q, Ks, Vs, O, L, pos = prefill_problem(B, H, Hkv, R, D, prec, (64, 64), (40, 9))
    pad = np.full((Hkv, 32, D), 0.5, np.float32)
    cache = Cache([np.concatenate([Ks[0], pad], 1), Ks[1]], [np.concatenate([Vs[0], pad], 1), Vs[1]],
                  prec, page, lens=(64, 64))
    o, l, _ = forward(Q, cache.struct(), Hkv, prec, 64, (40, 9))
    cache.lens = i32((500, 64))
    o2, l2, _ = forward(Q, cache.struct(), Hkv, prec, 64, (40, 9))
    assert torch.equal(o, o2) and torch.equal(l, l2)
    prefill_check(o2, l2, O, L, pos, prec, "clamped")


# 7. The arithmetic does not depend on the paging.
def test_bit_identical_across_pagings(gpu):
    B, H, Hkv, R, D, prec, lens, new = 2, 4, 2, 160, 128, P.FP16, (300, 97), (160, 33)
    Q, Ks, Vs, O, L, pos = prefill_problem(B, H, Hkv, R, D, prec, lens, new)
    o0, l0, _ = forward(Q, Cache(Ks, Vs, prec, 32, spare=9, seed=3).struct(), Hkv, prec, 300, new)
    prefill_check(o0, l0, O, L, pos, prec, "page 32")
    o1, l1, _ = forward(Q, Cache(Ks, Vs, prec, 256, shuffle=False).struct(), Hkv, prec, 300, new)
    assert torch.equal(o0, o1) and torch.equal(l0, l1)
    # One page per sequence over a dense [B, C_alloc, H_kv, D] tensor.
    alloc, dense = 512, []
    for xs in (Ks, Vs):
        t = np.full((B, alloc, Hkv, D), np.nan, np.float32)
        for b, c in enumerate(lens):
            t[b, :c] = xs[b].transpose(1, 0, 2)
        dense.append(to_device(t, prec))
    table = torch.arange(B, dtype=torch.int32, device=DEV).reshape(B, 1)
    pc = mfa.PagedKVCache.make(prec, alloc, 1, B, Hkv, D, dense[0], dense[1], table, i32(lens),
                               strides=(alloc * Hkv * D, D, Hkv * D))
    o2, l2, _ = forward(Q, pc, Hkv, prec, 300, new)
    assert torch.equal(o0, o2) and torch.equal(l0, l2)


# 8. ... nor on what else is in the batch.
def test_bit_identical_alone_and_in_a_batch(gpu):
    B, H, Hkv, R, D, prec, page, lens, new = RAGGED
    Q, Ks, Vs, _, _, _ = prefill_problem(B, H, Hkv, R, D, prec, lens, new)
    o, l, _ = forward(Q, Cache(Ks, Vs, prec, page).struct(), Hkv, prec, 300, new)
    for b in (0, 2):
        ob, lb, _ = forward(Q[b:b + 1], Cache(Ks[b:b + 1], Vs[b:b + 1], prec, page, seed=9).struct(),
                            Hkv, prec, 300, new[b:b + 1])
        assert torch.equal(o[b:b + 1], ob) and torch.equal(l[b:b + 1], lb), b


# 9. Table entries of logical pages no key lies in are never used.
def test_unused_table_entries_may_be_out_of_range(gpu):
    B, H, Hkv, R, D, prec, page, lens, new = 2, 4, 2, 70, 64, P.FP16, 32, (200, 31), (70, 31)
    Q, Ks, Vs, O, L, pos = prefill_problem(B, H, Hkv, R, D, prec, lens, new)
    clean = Cache(Ks, Vs, prec, page)
    o0, l0, _ = forward(Q, clean.struct(), Hkv, prec, 200, new)
    prefill_check(o0, l0, O, L, pos, prec, "clean table")
    for fill in (-7, clean.num_pages + 5):
        dirty = Cache(Ks, Vs, prec, page, table_fill=fill)
        assert (dirty.table_np == fill).sum() >= 7     # sequence 1's pages 1.., and the extra column
        o1, l1, _ = forward(Q, dirty.struct(), Hkv, prec, 200, new)
        assert torch.equal(o0, o1) and torch.equal(l0, l1), fill


# 10. The query as the [B, R, H * D] output of a projection.
def test_projection_view_of_the_query(gpu):
    B, H, Hkv, R, D, prec, page, lens, new = RAGGED
    Q, Ks, Vs, _, _, _ = prefill_problem(B, H, Hkv, R, D, prec, lens, new)
    pc = Cache(Ks, Vs, prec, page).struct()
    o0, l0, _ = forward(Q, pc, Hkv, prec, 300, new)
    brhd = to_device(Q, prec).permute(0, 2, 1, 3).contiguous()       # [B, R, H, D]
    o1, l1, _ = forward(Q, pc, Hkv, prec, 300, new, q=brhd, q_strides=(R * H * D, D, H * D, 1))
    assert torch.equal(o0, o1) and torch.equal(l0, l1)


# 11. Append, prefill and decode over one cache struct.
def test_round_trip_with_the_writer(gpu):
    B, H, Hkv, R, D, prec, page = 3, 4, 2, 96, 128, P.FP16, 64
    lens, new = (250, 96, 40), (96, 96, 7)
    Q, Ks, Vs, O, L, pos = prefill_problem(B, H, Hkv, R, D, prec, lens, new, seed=4)
    # The cache before the chunk: the prefixes scattered by the host, NaN everywhere else.
    cache = Cache(Ks, Vs, prec, page)
    for b in range(B):
        for t in range(lens[b] - new[b], lens[b]):
            cache.k[cache.table_np[b, t // page], :, t % page] = float("nan")
            cache.v[cache.table_np[b, t // page], :, t % page] = float("nan")
    # The chunk's rows [B, H_kv, R, D]: row r < n_b is key lens[b] - n_b + r.
    kn, vn = (np.zeros((B, Hkv, R, D), np.float32) for _ in range(2))
    for b in range(B):
        kn[b, :, :new[b]] = Ks[b][:, lens[b] - new[b]:]
        vn[b, :, :new[b]] = Vs[b][:, lens[b] - new[b]:]
    pc, nl = cache.struct(), i32(new)
    mfa.paged_kv_append(mfa.PagedAppendDescriptor.make(prec, B, Hkv, R, D, 256),
                        to_device(kn, prec), to_device(vn, prec), pc, new_lens=nl)
    o, l, _ = forward(Q, pc, Hkv, prec, 256, new)
    prefill_check(o, l, O, L, pos, prec, "append -> prefill")
    # The decode call over the same lengths at uniform R = 7: its rows are the last 7 of each chunk.
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
    decode_check(od, ld, Od, Ld, lens, "decode rows")


# 12. lens += n, append, prefill as one graph, replayed with new device values.
def test_graph_replay_reads_new_lengths_and_rows(gpu):
    B, H, Hkv, R, D, prec, page, cap = 2, 4, 2, 72, 128, P.FP16, 64, 384
    rng = np.random.default_rng(12)
    max_pages, num_pages = cap // page, 2 * (cap // page) + 3
    # Finite values in every slot: what a step does not append is the prefix it reads.
    k, v = (to_device(rng.standard_normal((num_pages, Hkv, page, D)).astype(np.float32), prec)
            for _ in range(2))
    table = torch.from_numpy(rng.permutation(num_pages)[:B * max_pages].reshape(B, max_pages)
                             .astype(np.int32)).to(DEV)
    lens, nl = i32((0, 0)), i32((0, 0))
    pc = mfa.PagedKVCache.make(prec, page, max_pages, num_pages, Hkv, D, k, v, table, lens)
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
        mfa.paged_prefill_forward(desc, q, pc, o, new_lens=nl, logsumexp=l, stream=st.cuda_stream)

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


# 13. 64-bit page offsets.
def test_pool_beyond_2_31_bytes(gpu):
    # 128 KiB pages, 16400 of them (2.1 GiB per pool, untouched but for the used pages): the
    # sequence's three pages are the pool's last three, past a 32-bit byte offset.
    B, H, Hkv, R, D, prec, page, lens, num_pages = 1, 2, 1, 40, 256, P.FP16, 256, (700,), 16400
    Q, Ks, Vs, O, L, pos = prefill_problem(B, H, Hkv, R, D, prec, lens)
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
    pc = mfa.PagedKVCache.make(prec, page, 3, num_pages, Hkv, D, pools[0], pools[1], table, i32(lens))
    o, l, _ = forward(Q, pc, Hkv, prec, lens[0])
    prefill_check(o, l, O, L, pos, prec, "pool beyond 2^31 bytes")


# 14. What ran is what the plan named.
def test_launch_log_names_the_plan(gpu):
    for case in (RAGGED, (2, 4, 1, 130, 256, P.FP16, 128, (260, 129), None)):
        B, H, Hkv, R, D, prec, page, lens, new = case
        Q, Ks, Vs, _, _, _ = prefill_problem(B, H, Hkv, R, D, prec, lens, new)
        cache = Cache(Ks, Vs, prec, page)
        _, _, names = forward(Q, cache.struct(), Hkv, prec, max(lens), new)
        plan = mfa.paged_prefill_plan(prefill_descriptor(Q.shape, Hkv, prec, max(lens)), cache.struct())
        assert names == [r["name"] for r in plan], (names, plan)
        assert plan[0]["workgroups"] == B * H * -(-R // 128)
