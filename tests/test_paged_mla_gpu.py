"""GPU tests of the paged MLA decode and the latent append (mfa_paged_mla_decode_forward,
mfa_paged_latent_append; attention_mla_latent.hip mfa_mla_latent_paged_kernel, paged_append.hip).
A dense per-sequence latent is scattered into a pool through a shuffled block table with spare
pages; every pool slot that belongs to no sequence (unused pages, slots past a sequence's length
in its last page) holds NaN, and so do output and logsumexp before the call, so anything read
from outside a sequence, and any row left unwritten, shows.  The reference is the oracle on the
exact decompressed K = latent·W_k, V = latent·W_v (oracle_lib.gemm), one oracle call per sequence
with row q's keys given as the half-open range [0, limit_q + 1).  Rows with a visible key are held
to test_mla_absorbed_gpu.py's tolerances (the same tile body on the same inputs: O 5e-2 FP16 /
1e-1 BF16, L 3e-2 / 1e-1); the others must be exact zeros with L at its floor."""
import functools

import numpy as np
import pytest
import torch

import mfa_amd as mfa
import oracle_lib as ol
from harness import to_device
from paged_rig import DEV, LatentCache, P, i32, mla_check, mla_descriptor, positions, tag
from test_mla_absorbed_gpu import make_inputs

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def problem(B, H, R, D, latent, prec, lens, causal=False, seed=0):
    """Stored-value Q [B, H, R, D], per-sequence latents [len_b, latent], W_k, W_v, the oracle's
    O / L and the rows' limits, computed once per case.  One oracle call per sequence."""
    C = max(max(lens), 1)
    lat, wk, wv, Q = make_inputs(B, H, R, C, D, latent, prec, seed + R + sum(lens))
    lats = [lat.reshape(B, C, latent)[b, :max(c, 0)] for b, c in enumerate(lens)]
    pos = positions(lens, None, R, causal, decode=True)
    O = np.zeros((B, H, R, D), np.float32)
    L = np.zeros((B, H, R), np.float32)
    for b, c in enumerate(lens):
        if c <= 0 or not (pos[b] >= 0).any():
            continue
        K = ol.gemm(lats[b], wk).reshape(c, H, D).transpose(1, 0, 2)
        V = ol.gemm(lats[b], wv).reshape(c, H, D).transpose(1, 0, 2)
        ranges = np.zeros((1, H, R, 2), np.uint32)
        ranges[0, :, :, 1] = (pos[b] + 1).astype(np.uint32)[None, :]
        r = ol.attention(Q[b:b + 1], K[None], V[None], ranges=ranges)
        O[b], L[b] = r["O"][0], r["L"][0]
    for a in [Q, wk, wv, O, L, pos] + lats:
        a.setflags(write=False)
    return Q, lats, wk, wv, O, L, pos


def forward(Q, wk, wv, pc, latent, prec, max_seq_len, causal=False, lpi=None):
    """One call on NaN-filled outputs; returns (O, L, launched kernel names)."""
    B, H, R, D = Q.shape
    desc = mla_descriptor(Q.shape, latent, prec, max_seq_len, causal, lpi)
    o = torch.full((B, H, R, D), float("nan"), dtype=torch.float32, device=DEV)
    l = torch.full((B, H, R), float("nan"), dtype=torch.float32 if lpi is False else torch.float16,
                   device=DEV)
    mfa.last_launches()
    mfa.paged_mla_decode_forward(desc, to_device(Q, prec), to_device(wk, prec), to_device(wv, prec),
                                 pc, o, logsumexp=l)
    torch.cuda.synchronize()
    return o, l, [r["name"] for r in mfa.last_launches()]


def run_case(B, H, R, D, latent, prec, page, lens, causal=False, max_seq_len=None, lpi=None, **kw):
    Q, lats, wk, wv, O, L, pos = problem(B, H, R, D, latent, prec, lens, causal)
    cache = LatentCache(lats, prec, page, **kw)
    msl = max(max(lens), 1) if max_seq_len is None else max_seq_len
    o, l, names = forward(Q, wk, wv, cache.struct(), latent, prec, msl, causal, lpi)
    assert names[1:] == [f"mfa_mla_latent_paged_kernel<{tag(prec)}, {latent}>",
                         f"mfa_mla_latent_merge_kernel<{tag(prec)}, {latent}, 1>"], names
    mla_check(o, l, O, L, pos, prec,
              f"B{B} H{H} R{R} D{D} latent {latent} {tag(prec)} page {page} lens {lens} causal {causal}")
    return o, l


# 1. Ragged and unmasked, one row: two splits of 160 keys at max_seq_len 300 — a sequence over
#    both, one of less than two tiles, one that ends exactly on a page.
@pytest.mark.parametrize("prec", [P.FP16, P.BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("latent", [256, 512])
def test_ragged_unmasked_single_row(gpu, latent, prec):
    run_case(3, 4, 1, 64, latent, prec, 64, (300, 33, 64))


# 2. The smallest page and multi-row causal: 8 splits of 128 keys; sequence 1's rows have limits
#    125..129, so rows 0-2 see split 0 only, rows 3-4 reach into split 1, later splits are empty.
def test_smallest_page_multi_row_causal(gpu):
    run_case(2, 16, 5, 128, 512, P.BF16, 32, (1000, 130), causal=True, max_seq_len=1000, spare=9,
             seed=5)


# 3. Rows without a visible key: an empty sequence, and one shorter than R.
@pytest.mark.parametrize("lpi", [None, False], ids=["L-fp16", "L-fp32"])
def test_dead_rows(gpu, lpi):
    lens, R = (0, 3, 40), 5
    pos = positions(lens, None, R, decode=True)
    assert [(p >= 0).sum() for p in pos] == [0, 3, 5] and list(pos[1]) == [-1, -1, 0, 1, 2]
    run_case(3, 4, R, 64, 256, P.FP16, 32, lens, causal=True, lpi=lpi)


# 4. The arithmetic does not depend on the paging.
def test_bit_identical_across_pagings(gpu):
    B, H, R, D, latent, prec, lens = 2, 4, 3, 64, 256, P.FP16, (300, 97)
    Q, lats, wk, wv, O, L, pos = problem(B, H, R, D, latent, prec, lens, True)
    o0, l0, _ = forward(Q, wk, wv, LatentCache(lats, prec, 32, spare=9, seed=3).struct(), latent, prec,
                        300, True)
    mla_check(o0, l0, O, L, pos, prec, "page 32")
    o1, l1, _ = forward(Q, wk, wv, LatentCache(lats, prec, 256, shuffle=False).struct(), latent, prec,
                        300, True)
    assert torch.equal(o0, o1) and torch.equal(l0, l1)
    # One page per sequence over a dense [B, C_alloc, latent] tensor.
    alloc = 512
    t = np.full((B, alloc, latent), np.nan, np.float32)
    for b, c in enumerate(lens):
        t[b, :c] = lats[b]
    table = torch.arange(B, dtype=torch.int32, device=DEV).reshape(B, 1)
    pc = mfa.PagedLatentCache.make(prec, alloc, 1, B, latent, to_device(t, prec), table, i32(lens),
                                   strides=(alloc * latent, latent))
    o2, l2, _ = forward(Q, wk, wv, pc, latent, prec, 300, True)
    assert torch.equal(o0, o2) and torch.equal(l0, l2)


# 5. ... nor on what else is in the batch.  Two rows per head, so the query projection is the
#    general GEMM alone and in the batch (with one row, a batch takes the decode projection kernel
#    and a single sequence the GEMM, which round Q~ differently); at max_seq_len 300 both calls
#    split the keys in two (the tile count, not the batch, limits the split).
def test_bit_identical_alone_and_in_a_batch(gpu):
    B, H, R, D, latent, prec, page, lens = 3, 4, 2, 64, 256, P.FP16, 64, (300, 33, 64)
    Q, lats, wk, wv, O, L, pos = problem(B, H, R, D, latent, prec, lens, True)
    o, l, _ = forward(Q, wk, wv, LatentCache(lats, prec, page).struct(), latent, prec, 300, True)
    mla_check(o, l, O, L, pos, prec, "batch")
    for b in (0, 2):
        ob, lb, _ = forward(Q[b:b + 1], wk, wv, LatentCache(lats[b:b + 1], prec, page, seed=9).struct(),
                            latent, prec, 300, True)
        assert torch.equal(o[b:b + 1], ob) and torch.equal(l[b:b + 1], lb), b


# 6. Every length at max_seq_len: the dense absorbed call on the same rows splits the keys the
#    same way (8 splits), projects Q~ with the same kernel and merges with the same kernel.
def test_bit_identical_to_the_dense_route(gpu):
    B, H, R, D, latent, prec, S = 2, 16, 1, 128, 512, P.BF16, 1024
    Q, lats, wk, wv, O, L, pos = problem(B, H, R, D, latent, prec, (S, S))
    o, l, names = forward(Q, wk, wv, LatentCache(lats, prec, 64).struct(), latent, prec, S)
    mla_check(o, l, O, L, pos, prec, "full lengths")
    assert names[0] == "mfa_mla_qproj_kernel<BF16>"
    base = mfa.AttentionDescriptor.make(low_precision=True, precision=prec)
    od = torch.full((B, H, R, D), float("nan"), dtype=torch.float32, device=DEV)
    ld = torch.full((B, H, R), float("nan"), dtype=torch.float16, device=DEV)
    dense = to_device(np.concatenate(lats), prec)                       # [B * S, latent]
    mfa.last_launches()
    mfa.mla_forward_absorbed(base, dense, to_device(wk, prec), to_device(wv, prec),
                             to_device(Q, prec), od, B, H, R, S, D, latent, prec, logsumexp=ld)
    torch.cuda.synchronize()
    ran = [r["name"] for r in mfa.last_launches()]
    assert ran == ["mfa_mla_qproj_kernel<BF16>", "mfa_mla_latent_kernel<BF16, 512>",
                   "mfa_mla_latent_merge_kernel<BF16, 512, 1>"], ran
    assert torch.equal(o, od) and torch.equal(l, ld)


# 7. Lengths above the cap are clamped; table entries of pages no key lies in are never used.
def test_lengths_above_the_cap_are_clamped(gpu):
    # Caches of 96 and 64 keys, cap 64 (max_seq_len): lengths (500, 64) read as (64, 64).
    B, H, R, D, latent, prec, page = 2, 4, 3, 64, 256, P.FP16, 32
    Q, lats, wk, wv, O, L, pos = problem(B, H, R, D, latent, prec, (64, 64), True)
    pad = np.full((32, latent), 0.5, np.float32)
    cache = LatentCache([np.concatenate([lats[0], pad]), lats[1]], prec, page, lens=(64, 64))
    o, l, _ = forward(Q, wk, wv, cache.struct(), latent, prec, 64, True)
    cache.lens = i32((500, 64))
    o2, l2, _ = forward(Q, wk, wv, cache.struct(), latent, prec, 64, True)
    assert torch.equal(o, o2) and torch.equal(l, l2)
    mla_check(o2, l2, O, L, pos, prec, "clamped")


def test_unused_table_entries_may_be_out_of_range(gpu):
    B, H, R, D, latent, prec, page, lens = 2, 4, 1, 64, 256, P.FP16, 32, (200, 31)
    Q, lats, wk, wv, O, L, pos = problem(B, H, R, D, latent, prec, lens)
    clean = LatentCache(lats, prec, page)
    o0, l0, _ = forward(Q, wk, wv, clean.struct(), latent, prec, 200)
    mla_check(o0, l0, O, L, pos, prec, "clean table")
    for fill in (-7, clean.num_pages + 5):
        dirty = LatentCache(lats, prec, page, table_fill=fill)
        assert (dirty.table_np == fill).sum() >= 7     # sequence 1's pages 1.., and the extra column
        o1, l1, _ = forward(Q, wk, wv, dirty.struct(), latent, prec, 200)
        assert torch.equal(o0, o1) and torch.equal(l0, l1), fill


# 8. The latent append: ragged rows out of a wider projection output, bits unchanged, nothing
#    else written.
@pytest.mark.parametrize("prec", [P.FP16, P.BF16], ids=["fp16", "bf16"])
def test_latent_append_writes_only_its_rows(gpu, prec):
    B, R, latent, page, max_pages, cap = 7, 4, 256, 32, 3, 64        # the table spans 96 keys
    lens = (10, 5, 7, 40, 33, 2, 66)       # after the append
    new = (3, 0, -2, 9, 1, 4, 4)           # 9 > R: R rows; (2, 4): rows 0-1 lie before key 0;
    rng = np.random.default_rng(8)         # (66, 4): rows 2-3 lie at or past the cap
    num_pages = B * max_pages + 2
    dt = torch.float16 if prec == P.FP16 else torch.bfloat16
    sentinel = 0x7e55 if prec == P.FP16 else 0x7fd5                   # NaN payloads
    pool = torch.full((num_pages, page, latent), sentinel, dtype=torch.int16, device=DEV).view(dt)
    table_np = rng.permutation(num_pages)[:B * max_pages].reshape(B, max_pages).astype(np.int32)
    table, dl, dn = torch.from_numpy(table_np).to(DEV), i32(lens), i32(new)
    wide = to_device(rng.standard_normal((B, R, latent + 64)).astype(np.float32), prec)
    rows = wide[:, :, 32:32 + latent]                                 # strides (R * 320, 320)
    pc = mfa.PagedLatentCache.make(prec, page, max_pages, num_pages, latent, pool, table, dl)
    want = pool.view(torch.int16).clone()
    written = 0
    for b in range(B):
        n = min(max(new[b], 0), R)
        for r in range(n):
            t = lens[b] - n + r
            if 0 <= t < cap:
                want[int(table_np[b, t // page]), t % page] = rows[b, r].view(torch.int16)
                written += 1
    assert written == 3 + 0 + 0 + 4 + 1 + 2 + 2
    mfa.last_launches()
    mfa.paged_latent_append(mfa.PagedLatentAppendDescriptor.make(prec, B, R, latent, cap), rows, pc,
                            new_lens=dn)
    torch.cuda.synchronize()
    ran = mfa.last_launches()
    assert [r["name"] for r in ran] == [f"mfa_paged_append_kernel<{tag(prec)}, 0>"]
    assert ran[0]["workgroups"] == -(-B * R // 4)
    assert torch.equal(pool.view(torch.int16), want)
    assert dl.tolist() == list(lens) and dn.tolist() == list(new)
    assert torch.equal(table.cpu(), torch.from_numpy(table_np))


# 9. Append, then decode, over one cache struct.
def test_round_trip_with_the_writer(gpu):
    B, H, R, D, latent, prec, page, lens = 3, 4, 3, 64, 512, P.BF16, 64, (250, 96, 40)
    Q, lats, wk, wv, O, L, pos = problem(B, H, R, D, latent, prec, lens, True, seed=4)
    cache = LatentCache(lats, prec, page)
    for b in range(B):                                  # the cache before the R new tokens
        for t in range(lens[b] - R, lens[b]):
            cache.pool[int(cache.table_np[b, t // page]), t % page] = float("nan")
    new_rows = to_device(np.stack([lats[b][lens[b] - R:] for b in range(B)]), prec)
    pc = cache.struct()
    mfa.paged_latent_append(mfa.PagedLatentAppendDescriptor.make(prec, B, R, latent, 256), new_rows,
                            pc)
    o, l, _ = forward(Q, wk, wv, pc, latent, prec, 256, True)
    mla_check(o, l, O, L, pos, prec, "append -> decode")


# 10. lens += n, append, decode as one graph, replayed with new device values.
def test_graph_replay_reads_new_lengths(gpu):
    B, H, R, D, latent, prec, page, cap = 2, 4, 4, 64, 256, P.FP16, 64, 384
    rng = np.random.default_rng(12)
    max_pages, num_pages = cap // page, 2 * (cap // page) + 3
    # Finite values in every slot: what a step does not append is the prefix it reads.
    pool = to_device(rng.standard_normal((num_pages, page, latent)).astype(np.float32), prec)
    table = torch.from_numpy(rng.permutation(num_pages)[:B * max_pages].reshape(B, max_pages)
                             .astype(np.int32)).to(DEV)
    lens, nl = i32((0, 0)), i32((0, 0))
    pc = mfa.PagedLatentCache.make(prec, page, max_pages, num_pages, latent, pool, table, lens)
    s = np.sqrt(1.0 / latent)
    q = to_device(rng.standard_normal((B, H, R, D)).astype(np.float32), prec)
    wk, wv = (to_device((rng.standard_normal((latent, H * D)) * s).astype(np.float32), prec)
              for _ in range(2))
    rows = to_device(rng.standard_normal((B, R, latent)).astype(np.float32), prec)
    desc = mla_descriptor((B, H, R, D), latent, prec, cap, causal=True)
    adesc = mfa.PagedLatentAppendDescriptor.make(prec, B, R, latent, cap)
    o = torch.empty((B, H, R, D), dtype=torch.float32, device=DEV)
    l = torch.empty((B, H, R), dtype=torch.float16, device=DEV)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()

    def step():
        lens.add_(nl)
        mfa.paged_latent_append(adesc, rows, pc, new_lens=nl, stream=st.cuda_stream)
        mfa.paged_mla_decode_forward(desc, q, wk, wv, pc, o, logsumexp=l, stream=st.cuda_stream)

    with torch.cuda.stream(st):
        step()   # warm-up outside the capture
        st.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            step()
        for before, new in (((100, 0), (4, 2)), ((250, 31), (1, 4)), ((300, 0), (3, 0))):
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
            pos = positions([a + b for a, b in zip(before, new)], None, R, decode=True)
            dead = torch.from_numpy(pos < 0).to(DEV)[:, None, :].expand(B, H, R)
            assert dead.any() or min(a + b for a, b in zip(before, new)) >= R
            assert torch.count_nonzero(got[1][0][dead]).item() == 0
            assert torch.isneginf(got[1][1].float()[dead]).all()
            assert torch.isfinite(got[1][1].float()[~dead]).all()


# 11. What ran is what the plan named: a split shape and an unsplit one.
@pytest.mark.parametrize("R,lens,nsplit", [(1, (300, 33), 2), (5, (100, 7), 1)],
                         ids=["split", "unsplit"])
def test_launch_log_names_the_plan(gpu, R, lens, nsplit):
    B, H, D, latent, prec, page = 2, 4, 64, 256, P.FP16, 32
    Q, lats, wk, wv, _, _, _ = problem(B, H, R, D, latent, prec, lens, R > 1)
    cache = LatentCache(lats, prec, page)
    _, _, names = forward(Q, wk, wv, cache.struct(), latent, prec, max(lens), R > 1)
    plan = mfa.paged_mla_decode_plan(mla_descriptor(Q.shape, latent, prec, max(lens), R > 1),
                                     cache.struct())
    assert names == [r["name"] for r in plan] and len(plan) == 3, (names, plan)
    assert plan[1]["workgroups"] == -(-H * R // 32) * B * nsplit
    assert plan[2]["workgroups"] == B * H * R
