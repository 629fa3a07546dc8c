"""GPU tests of the causal sliding window of the paged K/V calls (MFA_SPARSITY_CAUSAL_WINDOW:
mfa_paged_decode_forward, mfa_paged_prefill_forward, mfa_quantized_paged_prefill_forward).  Row q
at key position t_q attends to keys t_q - W <= j <= t_q.  Caches, NaN fill of everything outside
the sequences (pools, outputs, L), data and tolerances are those of test_paged_decode_gpu.py,
test_paged_prefill_gpu.py and test_paged_prefill_kv8_gpu.py: the builders and `check` functions
of paged_rig.py.  The reference is the oracle, once per sequence on the stored values, row
q's keys given as the sparse range [max(0, t_q - W), t_q + 1).  Beyond the oracle: a window that
covers everything gives the CAUSAL call's bits, and pages wholly below the window may hold NaN
and stale table entries (the page-release contract of include/mfa/mfa.h)."""
import functools

import numpy as np
import pytest
import torch

import mfa_amd as mfa
import oracle_lib as ol
import paged_rig as rig
from harness import seen, to_device
from paged_rig import DEAD_LENS, DEAD_NEW, DEAD_R, DEV, NAN, ZP, Cache, Cache8, P, positions
from paged_rig import cache_of, decode_check, decode_forward, prefill_check

pytestmark = pytest.mark.gpu

HUGE = 2 ** 31 - 1


def window_ref(Q, Ks, Vs, pos, W):
    """The oracle's O [B, H, R, D] and L [B, H, R]: one call per sequence, row q's keys the range
    [max(0, pos - W), pos + 1); rows with pos < 0 keep zeros (they are checked as dead rows)."""
    B, H, R, D = Q.shape
    O = np.zeros((B, H, R, D), np.float32)
    L = np.zeros((B, H, R), np.float32)
    for b in range(B):
        live = pos[b] >= 0
        if not live.any():
            continue
        Hkv = Ks[b].shape[0]
        ranges = np.zeros((1, Hkv, R, 2), np.uint32)
        ranges[0, :, :, 0] = np.where(live, np.maximum(pos[b] - W, 0), 0)[None, :]
        ranges[0, :, :, 1] = np.where(live, pos[b] + 1, 0)[None, :]
        r = ol.attention(Q[b:b + 1], Ks[b][None], Vs[b][None], ranges=ranges)
        O[b], L[b] = r["O"][0], r["L"][0]
    return O, L


# ---------------------------------------------------------------------------------- decode
def decode_positions(lens, R):
    return positions(lens, None, R)


@functools.lru_cache(maxsize=None)
def decode_problem(B, H, Hkv, R, D, prec, lens, W, kv8=False):
    """test_paged_decode_gpu.py::problem's data with the window's oracle, once per case."""
    Q, Ks, Vs, quant, _, _ = rig.decode_problem(B, H, Hkv, R, D, prec, lens, kv8)
    O, L = window_ref(Q, Ks, Vs, decode_positions(lens, R), W)
    O.setflags(write=False)
    L.setflags(write=False)
    return Q, Ks, Vs, quant, O, L


# (B, H, Hkv, R, D, prec, page, lens, W, max_seq_len)
# 1. 16-row form: the window crosses a page edge (288), its lower edge 259 is no tile start, and
#    one sequence is shorter than W.
DEC16 = (3, 4, 2, 1, 128, P.FP16, 32, (300, 97, 33), 40, 300)
# 2. 32-row form, two row tiles: rows late in a tile meet leading tiles that are wholly masked.
DEC32 = (2, 2, 2, 40, 64, P.BF16, 32, (200, 40), 5, 200)
# 3. Split path: three splits of 512 keys from a moved base; one sequence shorter than the span.
SPLIT = (3, 8, 2, 1, 64, P.BF16, 64, (5000, 1600, 700), 1500, 8192)


def run_decode(case, kv8=False):
    B, H, Hkv, R, D, prec, page, lens, W, msl = case
    Q, Ks, Vs, quant, O, L = decode_problem(B, H, Hkv, R, D, prec, lens, W, kv8)
    cache = cache_of(Ks, Vs, prec, page, quant)
    o, l, names = decode_forward(Q, cache, prec, msl, W=W)
    assert names[0].startswith(rig.decode_kernel_form(H, Hkv, R)), names
    assert names[0].endswith(", 1>" if kv8 else ", 0>"), names
    decode_check(o, l, O, L, lens, f"window {case} kv8={kv8} {names}")
    return o, l, names


@pytest.mark.parametrize("kv8", [False, True], ids=["fp16", "int8"])
def test_decode_16_row_form(gpu, kv8):
    _, _, names = run_decode(DEC16, kv8)
    assert len(names) == 1, names          # 72 keys of span: one split, merged in the workgroup


@pytest.mark.parametrize("kv8", [False, True], ids=["bf16", "int8"])
def test_decode_32_row_form_with_leading_masked_tiles(gpu, kv8):
    _, _, names = run_decode(DEC32, kv8)
    assert len(names) == 1, names


@pytest.mark.parametrize("kv8", [False, True], ids=["bf16", "int8"])
def test_decode_split_path(gpu, kv8):
    _, _, names = run_decode(SPLIT, kv8)
    assert names[1:] == ["mfa_decode_merge_kernel"], names
    # The grid is the span's (1532 keys: 3 splits), not the cap's.
    B, H, Hkv, R, D, prec, page, lens, W, msl = SPLIT
    base = mfa.AttentionDescriptor.make(low_precision=True, precision=prec, causal_window=W)
    plan = mfa.paged_decode_plan(mfa.PagedDecodeDescriptor.make(base, B, H, R, D, msl, Hkv=Hkv))
    assert plan[0]["workgroups"] == 3 * B * Hkv, plan


def test_decode_window_zero_returns_the_rows_own_value(gpu):
    B, H, Hkv, R, D, prec, page, lens, _, msl = DEC16
    Q, Ks, Vs, _, O, L = decode_problem(B, H, Hkv, R, D, prec, lens, 0)
    o, l, _ = decode_forward(Q, Cache(Ks, Vs, prec, page), prec, msl, W=0)
    own = np.stack([np.stack([Vs[b][h % Hkv, lens[b] - R:lens[b]] for h in range(H)])
                    for b in range(B)])
    decode_check(o, l, own, L, lens, "W = 0 against the stored V rows")
    decode_check(o, l, O, L, lens, "W = 0 against the oracle")
    # A second shape with several rows per sequence (32-row form).
    B, H, Hkv, R, D, prec, page, lens, _, msl = DEC32
    Q, Ks, Vs, _, O, L = decode_problem(B, H, Hkv, R, D, prec, lens, 0)
    o, l, _ = decode_forward(Q, Cache(Ks, Vs, prec, page), prec, msl, W=0)
    own = np.stack([np.stack([Vs[b][h % Hkv, lens[b] - R:lens[b]] for h in range(H)])
                    for b in range(B)])
    decode_check(o, l, own, L, lens, "W = 0, 40 rows, against the stored V rows")


@pytest.mark.parametrize("case,kv8", [(DEC16, False), (DEC16, True), (DEC32, False), (SPLIT, False)],
                         ids=["16rows", "16rows-int8", "32rows", "split"])
def test_decode_huge_window_is_the_causal_call(gpu, case, kv8):
    B, H, Hkv, R, D, prec, page, lens, _, msl = case
    Q, Ks, Vs, quant, _, _ = rig.decode_problem(B, H, Hkv, R, D, prec, lens, kv8)
    cache = cache_of(Ks, Vs, prec, page, quant)
    o0, l0, n0 = decode_forward(Q, cache, prec, msl, causal=True)
    o1, l1, n1 = decode_forward(Q, cache, prec, msl, W=HUGE)
    assert n0 == n1, (n0, n1)
    assert not torch.isnan(o0).any() and not torch.isnan(l0.float()).any()
    assert torch.equal(o0, o1) and torch.equal(l0, l1)


def release_pages(cache, table_np, lens, los, page):
    """Every logical page wholly below los[b]: its pool page NaN in K and V, its table entry
    pointed at a NaN-filled page no sequence owns.  Returns the number of pages released."""
    owned = {int(table_np[b, j]) for b, c in enumerate(lens) for j in range(-(-c // page))}
    spare = min(set(range(cache.num_pages)) - owned)
    assert torch.isnan(cache.k[spare].float()).all() and torch.isnan(cache.v[spare].float()).all()
    table = table_np.copy()
    n = 0
    for b, lo in enumerate(los):
        for j in range(max(lo, 0) // page):          # pages with (j + 1) * page <= lo
            cache.k[int(table_np[b, j])] = NAN
            cache.v[int(table_np[b, j])] = NAN
            table[b, j] = spare
            n += 1
    cache.table = torch.from_numpy(table).to(DEV)
    return n


@pytest.mark.parametrize("case", [DEC16, SPLIT], ids=["16rows", "split"])
def test_decode_pages_below_the_window_are_never_read(gpu, case):
    B, H, Hkv, R, D, prec, page, lens, W, msl = case
    Q, Ks, Vs, _, O, L = decode_problem(B, H, Hkv, R, D, prec, lens, W)
    cache = Cache(Ks, Vs, prec, page)
    o0, l0, _ = decode_forward(Q, cache, prec, msl, W=W)
    los = [max(0, max(0, c - R) - W) for c in lens]
    n = release_pages(cache, cache.table.cpu().numpy(), lens, los, page)
    assert n >= (8 if case is DEC16 else 54 + 1), n
    o1, l1, _ = decode_forward(Q, cache, prec, msl, W=W)
    assert torch.isfinite(o1).all() and torch.isfinite(l1.float()).all()
    assert torch.equal(o0, o1) and torch.equal(l0, l1)
    decode_check(o1, l1, O, L, lens, f"released pages {case}")


def test_decode_graph_replay_moves_the_base(gpu):
    # lens += 1 -> decode as one graph.  W 40, R 1: the base (len - 41) & ~31 is 32 at length 104
    # and 64 from 105 on, so the replays cross the move; sequence 1 crosses a page edge (257).
    B, H, Hkv, R, D, prec, page, cap, W = 2, 8, 2, 1, 128, P.FP16, 32, 320, 40
    Q, Ks, Vs, _, _, _ = rig.decode_problem(B, H, Hkv, R, D, prec, (cap, cap))
    cache = Cache(Ks, Vs, prec, page, lens=(103, 255))
    pc = cache.struct()
    base = mfa.AttentionDescriptor.make(low_precision=True, precision=prec, causal_window=W)
    desc = mfa.PagedDecodeDescriptor.make(base, B, H, R, D, cap, Hkv=Hkv)
    q = to_device(Q, prec)
    o = torch.empty((B, H, R, D), dtype=torch.float32, device=DEV)
    l = torch.empty((B, H, R), dtype=torch.float16, device=DEV)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()

    def decode():
        mfa.paged_decode_forward(desc, q, pc, o, l, stream=st.cuda_stream)

    def step():
        cache.lens.add_(1)
        decode()

    with torch.cuda.stream(st):
        decode()   # warm-up outside the capture
        st.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            step()
        cache.lens.copy_(torch.tensor((103, 255), dtype=torch.int32))
        for k in range(1, 4):
            lens = (103 + k, 255 + k)
            o.fill_(NAN)
            l.fill_(NAN)
            graph.replay()
            st.synchronize()
            assert cache.lens.tolist() == list(lens)
            go, gl = o.clone(), l.clone()
            o.fill_(NAN)
            l.fill_(NAN)
            decode()   # eager, at the same lengths
            st.synchronize()
            assert torch.equal(o, go) and torch.equal(l, gl), lens
            Kb, Vb = [k_[:, :n] for k_, n in zip(Ks, lens)], [v[:, :n] for v, n in zip(Vs, lens)]
            Or, Lr = window_ref(Q, Kb, Vb, decode_positions(lens, R), W)
            decode_check(go, gl, Or, Lr, lens, f"replay {lens}")


# --------------------------------------------------------------------------------- prefill
def prefill_forward(Q, pc, Hkv, prec, max_seq_len, new_lens=None, W=None, causal=False, **kw):
    """One prefill call on NaN-filled outputs; returns (O, L, launched kernel names)."""
    o, l, log, _ = rig.prefill_forward(Q, pc, Hkv, prec, max_seq_len, new_lens, causal, W=W, **kw)
    return o, l, [r["name"] for r in log]


def window_kernel(prec, D, kv8=False):
    return rig.prefill_kernel_name(prec, D, kv8, window=True)


@functools.lru_cache(maxsize=None)
def prefill_problem(B, H, Hkv, R, D, prec, lens, new_lens, W):
    """test_paged_prefill_gpu.py::problem's data with the window's oracle, once per case."""
    Q, Ks, Vs, _, _, pos = rig.prefill_problem(B, H, Hkv, R, D, prec, lens, new_lens)
    O, L = window_ref(Q, Ks, Vs, pos, W)
    O.setflags(write=False)
    L.setflags(write=False)
    return Q, Ks, Vs, O, L, pos


# (B, H, Hkv, R, D, prec, page, lens, new_lens, W)
# 8. Two 128-row blocks and a window below the block height: the second block starts past key 0,
#    every block has rows whose leading tiles are wholly masked; a pure prompt; a short chunk.
TWO_BLOCKS = (3, 4, 2, 160, 128, P.FP16, 64, (300, 160, 97), (160, 160, 33), 70)
# 9. D 256 (32-key tiles), BF16, the smallest page, W one short of a tile.
D256 = (2, 4, 1, 64, 256, P.BF16, 32, (130, 64), None, 31)


def run_prefill(case, **kw):
    B, H, Hkv, R, D, prec, page, lens, new, W = case
    Q, Ks, Vs, O, L, pos = prefill_problem(B, H, Hkv, R, D, prec, lens, new, W)
    cache = Cache(Ks, Vs, prec, page, **kw)
    o, l, names = prefill_forward(Q, cache.struct(), Hkv, prec, max(lens), new, W)
    assert names == [window_kernel(prec, D)], names
    prefill_check(o, l, O, L, pos, prec, f"window prefill {case}")
    return o, l


def test_prefill_two_blocks_window_below_the_block_height(gpu):
    run_prefill(TWO_BLOCKS)


def test_prefill_d256_bf16(gpu):
    run_prefill(D256, spare=9, seed=5)


@pytest.mark.parametrize("W", [0, 1, 33])
def test_prefill_small_windows_bf16_d64(gpu, W):
    # The BF16 / FP32-score path of the body, a 64-key tile from two pages, and rows whose every
    # tile but the last is wholly masked (W = 0: each row sees its own key only).
    run_prefill((2, 8, 2, 70, 64, P.BF16, 32, (200, 31), (70, 31), W), spare=40, seed=5)


@pytest.mark.parametrize("lpi", [None, False], ids=["L-fp16", "L-fp32"])
def test_prefill_dead_rows_under_the_window(gpu, lpi):
    B, H, Hkv, R, D, prec, page, W = 5, 2, 1, DEAD_R, 64, P.FP16, 32, 10
    Q, Ks, Vs, O, L, pos = prefill_problem(B, H, Hkv, R, D, prec, DEAD_LENS, DEAD_NEW, W)
    assert [(p >= 0).sum() for p in pos] == [0, 0, 20, 0, R]
    o, l, _ = prefill_forward(Q, Cache(Ks, Vs, prec, page).struct(), Hkv, prec, 90,
                              DEAD_NEW, W, lpi=lpi)
    prefill_check(o, l, O, L, pos, prec, f"window dead rows lpi={lpi}")


@pytest.mark.parametrize("case", [TWO_BLOCKS, D256], ids=["fp16-128", "bf16-256"])
def test_prefill_huge_window_is_the_causal_call(gpu, case):
    B, H, Hkv, R, D, prec, page, lens, new, _ = case
    Q, Ks, Vs, _, _, _ = rig.prefill_problem(B, H, Hkv, R, D, prec, lens, new)
    pc = Cache(Ks, Vs, prec, page).struct()
    o0, l0, n0 = prefill_forward(Q, pc, Hkv, prec, max(lens), new, causal=True)
    o1, l1, n1 = prefill_forward(Q, pc, Hkv, prec, max(lens), new, HUGE)
    assert n0 == [rig.prefill_kernel_name(prec, D)] and n1 == [window_kernel(prec, D)], (n0, n1)
    assert not torch.isnan(o0).any() and not torch.isnan(l0.float()).any()
    assert torch.equal(o0, o1) and torch.equal(l0, l1)


def prefill_los(lens, new, R, W):
    return [max(0, max(0, c - (R if new is None else min(max(new[b], 0), R))) - W)
            for b, c in enumerate(lens)]


@pytest.mark.parametrize("case", [TWO_BLOCKS, (1, 2, 1, 40, 64, P.BF16, 32, (500,), (40,), 100)],
                         ids=["two-blocks", "long-prefix"])
def test_prefill_pages_below_the_window_are_never_read(gpu, case):
    B, H, Hkv, R, D, prec, page, lens, new, W = case
    Q, Ks, Vs, O, L, pos = prefill_problem(B, H, Hkv, R, D, prec, lens, new, W)
    cache = Cache(Ks, Vs, prec, page)
    o0, l0, _ = prefill_forward(Q, cache.struct(), Hkv, prec, max(lens), new, W)
    n = release_pages(cache, cache.table_np, lens, prefill_los(lens, new, R, W), page)
    assert n == (1 if case is TWO_BLOCKS else 11), n
    o1, l1, _ = prefill_forward(Q, cache.struct(), Hkv, prec, max(lens), new, W)
    assert not torch.isnan(o1).any() and not torch.isnan(l1.float()).any()
    assert torch.equal(o0, o1) and torch.equal(l0, l1)
    prefill_check(o1, l1, O, L, pos, prec, f"released pages {case}")


@pytest.mark.parametrize("prec,D", [(P.FP16, 128), (P.FP16, 256), (P.BF16, 64)],
                         ids=["f16-128", "f16-256", "bf16-64"])
def test_int8_prefill_is_the_16_bit_window_call_on_the_decoded_pool(gpu, prec, D):
    """The header's contract under the window: with power-of-two scales the quantised call equals,
    bit for bit, the 16-bit call on pools holding q - zp at softmax scale scale * k_scale, with O
    multiplied by v_scale (test_paged_prefill_kv8_gpu.py::test_exact_decode_of_the_pool's
    construction).  INT8 pools cannot be NaN-poisoned, so the page-release property of the INT8
    kernel rests on this identity with the 16-bit kernel, whose release test poisons the pages,
    plus the loop bounds (t0, klo, the tile-mask rule) the two kernels share word for word."""
    B, H, Hkv, R, _, _, page, lens, new, W = TWO_BLOCKS
    ks, vs, zps = 2.0 ** -5, 2.0 ** -4, (3, -128)
    Q, qk, qv, _, _, _, _ = rig.prefill8_problem(B, H, Hkv, R, D, prec, lens, new, scales=(ks, vs),
                                                 zps=zps, oracle=False)
    scale = np.float32(D ** -0.5)
    o8, l8, n8 = prefill_forward(Q, Cache8(qk, qv, page, (ks, vs), zps).struct(), Hkv, prec, 300,
                                 new, W, scale=float(scale),
                                 call=mfa.quantized_paged_prefill_forward)
    assert n8 == [window_kernel(prec, D, kv8=True)], n8
    ints = [[q.astype(np.float32) - z for q in qs] for qs, z in zip((qk, qv), zps)]
    assert all(np.array_equal(seen(x, prec), x) for xs in ints for x in xs)   # exact in 16 bits
    o16, l16, n16 = prefill_forward(Q, Cache(ints[0], ints[1], prec, page).struct(), Hkv, prec,
                                    300, new, W, scale=float(scale * np.float32(ks)))
    assert n16 == [window_kernel(prec, D)], n16
    assert not torch.isnan(o8).any() and not torch.isnan(l8.float()).any()
    assert torch.equal(o8, o16 * vs)
    assert torch.equal(l8, l16)


def test_int8_prefill_against_the_oracle(gpu):
    B, H, Hkv, R, D, prec, page, lens, new, W = TWO_BLOCKS
    Q, qk, qv, scales, _, _, pos = rig.prefill8_problem(B, H, Hkv, R, D, prec, lens, new,
                                                        oracle=False)
    Ks, Vs = ([(q.astype(np.float32) - ZP) * np.float32(s) for q in qs]
              for qs, s in zip((qk, qv), scales))
    O, L = window_ref(Q, Ks, Vs, pos, W)
    o, l, names = prefill_forward(Q, Cache8(qk, qv, page, scales).struct(), Hkv, prec, 300, new,
                                  W, call=mfa.quantized_paged_prefill_forward)
    assert names == [window_kernel(prec, D, kv8=True)], names
    prefill_check(o, l, O, L, pos, prec, "int8 window prefill")
