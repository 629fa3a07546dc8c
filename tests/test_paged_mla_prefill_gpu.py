"""GPU tests of the paged MLA prefill (mfa_paged_mla_prefill_forward; attention_mla_latent.hip
mfa_mla_latent_prefill_kernel).  The setting is test_paged_mla_gpu.py's: a dense per-sequence
latent scattered into a pool through a shuffled block table with spare pages, NaN in every pool
slot that belongs to no sequence and in output and logsumexp before the call, so anything read
from outside a sequence, and any row left unwritten, shows.  Here the rows are ragged: sequence b
brings n_b of the R query rows, row q < n_b at key position len_b - n_b + q, and query rows
q >= n_b hold NaN.  The reference is the oracle on the exact decompressed K = latent·W_k,
V = latent·W_v, one call per sequence, row q's keys given as the half-open range [0, limit_q + 1).
Live rows are held to test_mla_absorbed_gpu.py's tolerances (the same tile body and the same
16-bit Õ: O 5e-2 FP16 / 1e-1 BF16, L 3e-2 / 1e-1); dead rows must be exact zeros with L at its
floor."""
import functools

import numpy as np
import pytest
import torch

import mfa_amd as mfa
import oracle_lib as ol
from harness import maxerr, seen, to_device
from paged_rig import DEV, LatentCache, P, i32, mla_check, mla_descriptor, positions, tag
from test_mla_absorbed_gpu import make_inputs

pytestmark = pytest.mark.gpu


def oracle(Q, lats, wk, wv, pos):
    """O [B, H, R, D] and L [B, H, R] of rows with the limits pos; one oracle call per sequence.
    Dead rows are left at zero here and are not compared with these values."""
    B, H, R, D = Q.shape
    O = np.zeros((B, H, R, D), np.float32)
    L = np.zeros((B, H, R), np.float32)
    for b in range(B):
        c = lats[b].shape[0]
        if c == 0 or not (pos[b] >= 0).any():
            continue
        K = ol.gemm(lats[b], wk).reshape(c, H, D).transpose(1, 0, 2)
        V = ol.gemm(lats[b], wv).reshape(c, H, D).transpose(1, 0, 2)
        ranges = np.zeros((1, H, R, 2), np.uint32)
        ranges[0, :, :, 1] = (pos[b] + 1).astype(np.uint32)[None, :]
        r = ol.attention(Q[b:b + 1], np.ascontiguousarray(K)[None], np.ascontiguousarray(V)[None],
                         ranges=ranges)
        O[b], L[b] = r["O"][0], r["L"][0]
    return O, L


@functools.lru_cache(maxsize=None)
def problem(B, H, R, D, latent, prec, lens, new=None, causal=True, seed=0):
    """Stored-value Q [B, H, R, D], per-sequence latents [len_b, latent], W_k, W_v, the oracle's
    O / L and the rows' limits, computed once per case and left unchanged."""
    C = max(max(lens), 1)
    lat, wk, wv, Q = make_inputs(B, H, R, C, D, latent, prec, seed + R + sum(lens))
    lats = [lat.reshape(B, C, latent)[b, :max(c, 0)] for b, c in enumerate(lens)]
    pos = positions(lens, new, R, causal)
    O, L = oracle(Q, lats, wk, wv, pos)
    for a in [Q, wk, wv, O, L, pos] + lats:
        a.setflags(write=False)
    return Q, lats, wk, wv, O, L, pos


def poisoned(Q, new):
    """Q with NaN in the rows q >= n_b, which the call must never use."""
    if new is None:
        return Q
    Qd = Q.copy()
    for b, n in enumerate(new):
        Qd[b, :, min(max(n, 0), Q.shape[2]):] = np.nan
    return Qd


def forward(Q, wk, wv, pc, latent, prec, max_seq_len, new=None, causal=True, lpi=None):
    """One call on NaN-filled outputs; returns (O, L, launched kernel names)."""
    B, H, R, D = Q.shape
    desc = mla_descriptor(Q.shape, latent, prec, max_seq_len, causal, lpi)
    o = torch.full((B, H, R, D), float("nan"), dtype=torch.float32, device=DEV)
    l = torch.full((B, H, R), float("nan"), dtype=torch.float32 if lpi is False else torch.float16,
                   device=DEV)
    mfa.last_launches()
    mfa.paged_mla_prefill_forward(desc, to_device(poisoned(Q, new), prec), to_device(wk, prec),
                                  to_device(wv, prec), pc, o, new_lens=i32(new), logsumexp=l)
    torch.cuda.synchronize()
    return o, l, [r["name"] for r in mfa.last_launches()]


def run_case(B, H, R, D, latent, prec, page, lens, new=None, causal=True, max_seq_len=None,
             lpi=None, **kw):
    Q, lats, wk, wv, O, L, pos = problem(B, H, R, D, latent, prec, lens, new, causal)
    cache = LatentCache(lats, prec, page, **kw)
    msl = max(max(lens), 1) if max_seq_len is None else max_seq_len
    o, l, names = forward(Q, wk, wv, cache.struct(), latent, prec, msl, new, causal, lpi)
    assert len(names) == 3 and names[1] == f"mfa_mla_latent_prefill_kernel<{tag(prec)}, {latent}>"
    mla_check(o, l, O, L, pos, prec, f"B{B} H{H} R{R} D{D} latent {latent} {tag(prec)} page {page} "
                                     f"lens {lens} new {new} causal {causal}")
    return o, l


# 1. A ragged causal chunk behind prefixes.  R = 40 is no multiple of 32, so query blocks span
#    head boundaries; sequence 2 brings no row; sequence 1's rows have limits 26..32, which lie
#    in the first tile and reach into the second.
@pytest.mark.parametrize("prec", [P.FP16, P.BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("latent", [256, 512])
def test_ragged_causal_chunk_behind_prefixes(gpu, latent, prec):
    lens, new = (100, 33, 64), (40, 7, 0)
    pos = positions(lens, new, 40, True)
    assert [(p >= 0).sum() for p in pos] == [40, 7, 0] and pos[0, 0] == 60 and pos[1, 0] == 26
    run_case(3, 4, 40, 64, latent, prec, 32, lens, new)


# 2. The smallest lengths and the clamps.
@pytest.mark.parametrize("lpi", [None, False], ids=["L-fp16", "L-fp32"])
def test_smallest_lengths_and_clamps(gpu, lpi):
    R = 9
    # n_b > len_b: rows 0-3 lie before key 0.
    assert list(positions((5,), (9,), R, True)[0]) == [-1, -1, -1, -1, 0, 1, 2, 3, 4]
    run_case(1, 4, R, 64, 256, P.FP16, 32, (5,), (9,), lpi=lpi)
    # An empty sequence next to a live one; new_lens of -3 and of R + 5 are clamped to 0 and R.
    lens, new = (0, 40, 40, 12), (3, -3, R + 5, 4)
    pos = positions(lens, new, R, True)
    assert [(p >= 0).sum() for p in pos] == [0, 0, 9, 4] and pos[2, 0] == 31
    run_case(4, 4, R, 64, 256, P.FP16, 32, lens, new, lpi=lpi)
    # Every sequence empty: nothing is loaded, every row is written.
    run_case(2, 4, R, 64, 256, P.FP16, 32, (0, 0), (4, 0), lpi=lpi)


@pytest.mark.parametrize("lpi", [None, False], ids=["L-fp16", "L-fp32"])
def test_lengths_above_the_cap_are_clamped(gpu, lpi):
    # Caches of 96 and 64 keys, cap 64 (max_seq_len): lengths (500, 64) read as (64, 64).
    B, H, R, D, latent, prec, page = 2, 4, 9, 64, 256, P.FP16, 32
    new = (9, 5)
    Q, lats, wk, wv, O, L, pos = problem(B, H, R, D, latent, prec, (64, 64), new)
    pad = np.full((32, latent), 0.5, np.float32)
    cache = LatentCache([np.concatenate([lats[0], pad]), lats[1]], prec, page, lens=(64, 64))
    o, l, _ = forward(Q, wk, wv, cache.struct(), latent, prec, 64, new, lpi=lpi)
    cache.lens = i32((500, 64))
    o2, l2, _ = forward(Q, wk, wv, cache.struct(), latent, prec, 64, new, lpi=lpi)
    assert torch.equal(o, o2) and torch.equal(l, l2)
    mla_check(o2, l2, O, L, pos, prec, "clamped")


# 3. Further variants.
def test_without_new_lens_every_row_is_live(gpu):
    run_case(2, 4, 40, 64, 256, P.BF16, 32, (100, 40), None)


@pytest.mark.parametrize("new", [None, (40, 7, 0)], ids=["uniform", "ragged"])
def test_unmasked(gpu, new):
    # Every live row sees all of its sequence; a row before key 0 is dead all the same.
    lens = (100, 33, 5)
    pos = positions(lens, new, 40, False)
    assert pos[0].tolist() == [99] * 40
    if new is None:
        assert (pos[2] >= 0).sum() == 5 and pos[2, 39] == 4
    run_case(3, 4, 40, 64, 256, P.FP16, 32, lens, new, causal=False)


@pytest.mark.parametrize("D", [72, 128])
def test_head_dims_at_latent_512(gpu, D):
    run_case(2, 4, 40, D, 512, P.BF16, 32, (100, 33), (40, 7))


def test_sequence_ends_on_a_page_boundary(gpu):
    # 256-key pages: sequence 0 fills its page exactly, sequence 1 two pages, sequence 2 part of one.
    run_case(3, 4, 20, 64, 256, P.FP16, 256, (256, 512, 70), (20, 3, 11))


# 4. The arithmetic does not depend on the paging ...
def test_bit_identical_across_pagings(gpu):
    B, H, R, D, latent, prec, lens, new = 2, 4, 40, 64, 256, P.FP16, (300, 97), (40, 13)
    Q, lats, wk, wv, O, L, pos = problem(B, H, R, D, latent, prec, lens, new)
    o0, l0, _ = forward(Q, wk, wv, LatentCache(lats, prec, 32, spare=9, seed=3).struct(), latent, prec,
                        300, new)
    mla_check(o0, l0, O, L, pos, prec, "page 32")
    o1, l1, _ = forward(Q, wk, wv, LatentCache(lats, prec, 256, shuffle=False).struct(), latent, prec,
                        300, new)
    assert torch.equal(o0, o1) and torch.equal(l0, l1)
    # One page per sequence over a dense [B, C_alloc, latent] tensor.
    alloc = 512
    t = np.full((B, alloc, latent), np.nan, np.float32)
    for b, c in enumerate(lens):
        t[b, :c] = lats[b]
    table = torch.arange(B, dtype=torch.int32, device=DEV).reshape(B, 1)
    pc = mfa.PagedLatentCache.make(prec, alloc, 1, B, latent, to_device(t, prec), table, i32(lens),
                                   strides=(alloc * latent, latent))
    o2, l2, _ = forward(Q, wk, wv, pc, latent, prec, 300, new)
    assert torch.equal(o0, o2) and torch.equal(l0, l2)


#    ... nor on what else is in the batch: also with one row, where the decode call projects a
#    batch and a single sequence with different kernels.
@pytest.mark.parametrize("R,new", [(40, (40, 7, 0)), (1, (1, 0, 1))], ids=["R40", "R1"])
def test_bit_identical_alone_and_in_a_batch(gpu, R, new):
    B, H, D, latent, prec, page, lens = 3, 4, 64, 256, P.FP16, 64, (300, 33, 64)
    Q, lats, wk, wv, O, L, pos = problem(B, H, R, D, latent, prec, lens, new)
    o, l, _ = forward(Q, wk, wv, LatentCache(lats, prec, page).struct(), latent, prec, 300, new)
    mla_check(o, l, O, L, pos, prec, "batch")
    for b in (0, 2):
        ob, lb, _ = forward(Q[b:b + 1], wk, wv, LatentCache(lats[b:b + 1], prec, page, seed=9).struct(),
                            latent, prec, 300, new[b:b + 1])
        assert torch.equal(o[b:b + 1], ob) and torch.equal(l[b:b + 1], lb), b


# 5. With len = n = R the KV-cache diagonal is the dense call's top-left one, and at <= 224 keys
#    the dense call does not split: the same projection, the same tile body on the same tiles, the
#    same epilogue and the same output GEMM.
def test_bit_identical_to_the_dense_call(gpu):
    B, H, R, D, latent, prec = 2, 4, 200, 64, 512, P.FP16
    Q, lats, wk, wv, O, L, pos = problem(B, H, R, D, latent, prec, (R, R), (R, R))
    o, l, names = forward(Q, wk, wv, LatentCache(lats, prec, 32).struct(), latent, prec, R, (R, R))
    mla_check(o, l, O, L, pos, prec, "len = n = R")
    base = mfa.AttentionDescriptor.make(low_precision=True, precision=prec, causal=True)
    od = torch.full((B, H, R, D), float("nan"), dtype=torch.float32, device=DEV)
    ld = torch.full((B, H, R), float("nan"), dtype=torch.float16, device=DEV)
    dense = to_device(np.concatenate(lats), prec)                       # [B * R, latent]
    mfa.last_launches()
    mfa.mla_forward_absorbed(base, dense, to_device(wk, prec), to_device(wv, prec),
                             to_device(Q, prec), od, B, H, R, R, D, latent, prec, logsumexp=ld)
    torch.cuda.synchronize()
    ran = [r["name"] for r in mfa.last_launches()]
    assert ran == [names[0], "mfa_mla_latent_kernel<F16, 512>", names[2]], (ran, names)
    assert torch.equal(o, od) and torch.equal(l, ld)


# 6. Uniform rows: the decode call computes the same rows by its split route, which keeps Õ in
#    FP32 up to the merge, so the two agree within the tolerances and not bit for bit.
def test_agrees_with_the_decode_call(gpu):
    B, H, R, D, latent, prec, page, lens = 2, 4, 5, 64, 256, P.FP16, 32, (130, 64)
    Q, lats, wk, wv, O, L, pos = problem(B, H, R, D, latent, prec, lens, None)
    cache = LatentCache(lats, prec, page)
    o, l, _ = forward(Q, wk, wv, cache.struct(), latent, prec, 130)
    mla_check(o, l, O, L, pos, prec, "prefill")
    od = torch.full_like(o, float("nan"))
    ld = torch.full_like(l, float("nan"))
    mfa.paged_mla_decode_forward(mla_descriptor(Q.shape, latent, prec, 130), to_device(Q, prec),
                                 to_device(wk, prec), to_device(wv, prec), cache.struct(), od,
                                 logsumexp=ld)
    torch.cuda.synchronize()
    eo, el = maxerr(o, od), maxerr(l, ld)
    print(f"prefill vs decode: O {eo:.3e} (bound 5e-2); L {el:.3e} (bound 3e-2)")
    assert eo < 5e-2 and el < 3e-2


# 7. Table entries of pages no key lies in are never used.
def test_unused_table_entries_may_be_out_of_range(gpu):
    B, H, R, D, latent, prec, page, lens, new = 2, 4, 9, 64, 256, P.FP16, 32, (200, 31), (9, 4)
    Q, lats, wk, wv, O, L, pos = problem(B, H, R, D, latent, prec, lens, new)
    clean = LatentCache(lats, prec, page)
    o0, l0, _ = forward(Q, wk, wv, clean.struct(), latent, prec, 200, new)
    mla_check(o0, l0, O, L, pos, prec, "clean table")
    for fill in (-7, clean.num_pages + 5):
        dirty = LatentCache(lats, prec, page, table_fill=fill)
        assert (dirty.table_np == fill).sum() >= 7     # sequence 1's pages 1.., and the extra column
        o1, l1, _ = forward(Q, wk, wv, dirty.struct(), latent, prec, 200, new)
        assert torch.equal(o0, o1) and torch.equal(l0, l1), fill


# 8. Append, prefill and decode over one cache struct ...
def test_round_trip_with_the_writer_and_the_decode_call(gpu):
    B, H, R, D, latent, prec, page = 3, 4, 12, 64, 512, P.BF16, 64
    lens, new = (250, 96, 40), (12, 5, 0)
    Q, lats, wk, wv, O, L, pos = problem(B, H, R, D, latent, prec, lens, new, seed=4)
    cache = LatentCache(lats, prec, page)
    rows = np.zeros((B, R, latent), np.float32)
    for b in range(B):                                  # the cache before the n_b new tokens
        for q in range(new[b]):
            t = lens[b] - new[b] + q
            rows[b, q] = lats[b][t]
            cache.pool[int(cache.table_np[b, t // page]), t % page] = float("nan")
    pc, dn = cache.struct(), i32(new)
    mfa.paged_latent_append(mfa.PagedLatentAppendDescriptor.make(prec, B, R, latent, 256),
                            to_device(rows, prec), pc, new_lens=dn)
    o, l, _ = forward(Q, wk, wv, pc, latent, prec, 256, new)
    mla_check(o, l, O, L, pos, prec, "append -> prefill")
    # One decode row per sequence on the same struct: the last key's view of the whole sequence.
    Q1 = np.ascontiguousarray(Q[:, :, :1])
    od = torch.full((B, H, 1, D), float("nan"), dtype=torch.float32, device=DEV)
    ld = torch.full((B, H, 1), float("nan"), dtype=torch.float16, device=DEV)
    mfa.paged_mla_decode_forward(mla_descriptor(Q1.shape, latent, prec, 256), to_device(Q1, prec),
                                 to_device(wk, prec), to_device(wv, prec), pc, od, logsumexp=ld)
    torch.cuda.synchronize()
    p1 = positions(lens, None, 1, True)
    O1, L1 = oracle(Q1, lats, wk, wv, p1)
    mla_check(od, ld, O1, L1, p1, prec, "append -> prefill -> decode")


#    ... and lens += n, append, prefill as one graph, replayed with new device values; each replay
#    is held to the oracle on what the cache then holds.
def test_graph_replay_reads_new_lengths_and_rows(gpu):
    B, H, R, D, latent, prec, page, cap = 2, 4, 8, 64, 256, P.FP16, 64, 192
    rng = np.random.default_rng(12)
    max_pages, num_pages = cap // page, 2 * (cap // page) + 3
    # Finite values in every slot: what a step does not append is the prefix it reads.
    pool_np = seen(rng.standard_normal((num_pages, page, latent)).astype(np.float32), prec)
    table_np = rng.permutation(num_pages)[:B * max_pages].reshape(B, max_pages).astype(np.int32)
    pool, table = to_device(pool_np, prec), torch.from_numpy(table_np).to(DEV)
    lens, nl = i32((0, 0)), i32((0, 0))
    pc = mfa.PagedLatentCache.make(prec, page, max_pages, num_pages, latent, pool, table, lens)
    s = np.sqrt(1.0 / latent)
    Q = seen(rng.standard_normal((B, H, R, D)).astype(np.float32), prec)
    wk, wv = (seen((rng.standard_normal((latent, H * D)) * s).astype(np.float32), prec)
              for _ in range(2))
    rows_np = seen(rng.standard_normal((B, R, latent)).astype(np.float32), prec)
    q, dwk, dwv, rows = (to_device(x, prec) for x in (Q, wk, wv, rows_np))
    desc = mla_descriptor((B, H, R, D), latent, prec, cap)
    adesc = mfa.PagedLatentAppendDescriptor.make(prec, B, R, latent, cap)
    o = torch.empty((B, H, R, D), dtype=torch.float32, device=DEV)
    l = torch.empty((B, H, R), dtype=torch.float16, device=DEV)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()

    def step():
        lens.add_(nl)
        mfa.paged_latent_append(adesc, rows, pc, new_lens=nl, stream=st.cuda_stream)
        mfa.paged_mla_prefill_forward(desc, q, dwk, dwv, pc, o, new_lens=nl, logsumexp=l,
                                      stream=st.cuda_stream)

    with torch.cuda.stream(st):
        step()   # warm-up outside the capture (nothing appended: new_lens is zero)
        st.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            step()
        for before, new in (((100, 0), (8, 3)), ((150, 31), (1, 8)), ((64, 5), (0, 6))):
            after = [a + n for a, n in zip(before, new)]
            lats = []
            for b in range(B):                     # the host's copy of what the append writes
                for r in range(new[b]):
                    t = after[b] - new[b] + r
                    pool_np[table_np[b, t // page], t % page] = rows_np[b, r]
                lats.append(np.stack([pool_np[table_np[b, t // page], t % page]
                                      for t in range(after[b])]))
            pos = positions(after, new, R, True)
            Oref, Lref = oracle(Q, lats, wk, wv, pos)
            got = []
            for run in (step, graph.replay):
                lens.copy_(torch.tensor(before, dtype=torch.int32))
                nl.copy_(torch.tensor(new, dtype=torch.int32))
                o.fill_(float("nan"))
                l.fill_(float("nan"))
                run()
                st.synchronize()
                assert lens.tolist() == after
                got.append((o.clone(), l.clone()))
            assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1]), new
            mla_check(got[1][0], got[1][1], Oref, Lref, pos, prec, f"replay {before} + {new}")
    assert torch.equal(pool.cpu().float(), torch.from_numpy(pool_np))


# 9. What ran is what the plan named.
@pytest.mark.parametrize("R", [1, 40])
def test_launch_log_names_the_plan(gpu, R):
    B, H, D, latent, prec, page, lens = 2, 4, 64, 256, P.FP16, 32, (100, 33)
    new = (R, min(R, 7))
    Q, lats, wk, wv, _, _, _ = problem(B, H, R, D, latent, prec, lens, new)
    cache = LatentCache(lats, prec, page)
    _, _, names = forward(Q, wk, wv, cache.struct(), latent, prec, max(lens), new)
    plan = mfa.paged_mla_prefill_plan(mla_descriptor(Q.shape, latent, prec, max(lens)), cache.struct())
    assert names == [r["name"] for r in plan] and len(plan) == 3, (names, plan)
    assert plan[1]["name"] == "mfa_mla_latent_prefill_kernel<F16, 256>"
    assert plan[1]["workgroups"] == B * -(-H * R // 32)
