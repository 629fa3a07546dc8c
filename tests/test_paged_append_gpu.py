"""GPU tests of the paged KV-cache append (mfa_paged_kv_append; csrc/paged_append.hip
mfa_paged_append_kernel).  Each pool lies inside a larger allocation with a guard band of one
page on either side; pools and guards are pre-filled with a fixed pseudo-random byte pattern,
the expected allocation is built on the CPU from the same pattern by a plain scatter of the
stored bytes (the input's bits, or the CPU oracle's INT8 quantisation of them), and the
comparison is byte equality of the whole allocation, so a stray write anywhere shows."""
import numpy as np
import pytest
import torch

import mfa_amd as mfa
import oracle_lib as ol
from harness import TORCH_DTYPE, maxerr, seen, to_device

pytestmark = pytest.mark.gpu

P = mfa.Precision
DEV = "cuda:0"


def pattern(nbytes, seed):
    return np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8)


def shuffled_table(B, max_pages, num_pages, seed=1):
    ids = np.random.default_rng(seed).permutation(num_pages)[:B * max_pages]
    return ids.reshape(B, max_pages).astype(np.int32)


class Rig:
    """K and V pools inside guarded allocations, on the device and as the CPU model."""

    def __init__(self, prec, cprec, B, Hkv, D, page, table, num_pages, layout="hs",
                 scales=(1.0, 1.0), zps=(0, 0), seed=7):
        self.prec, self.cprec, self.B, self.Hkv, self.D, self.page = prec, cprec, B, Hkv, D, page
        self.table_np = np.asarray(table, np.int32).reshape(B, -1)
        self.max_pages, self.num_pages = self.table_np.shape[1], num_pages
        self.es = 1 if cprec == P.INT8 else 2
        # [page][kv head][slot][d], or [page][slot][kv head][d].
        self.strides = (Hkv * page * D, page * D, D) if layout == "hs" else (page * Hkv * D, D, Hkv * D)
        self.guard = self.strides[0] * self.es                  # one page
        total = 2 * self.guard + num_pages * self.guard
        self.host = [pattern(total, seed), pattern(total, seed + 1)]
        self.dev = [torch.from_numpy(h.copy()).to(DEV) for h in self.host]
        self.table = torch.from_numpy(self.table_np).to(DEV)
        self.lens = torch.zeros(B, dtype=torch.int32, device=DEV)
        self.scales = tuple(float(np.float32(s)) for s in scales)
        self.zps = zps

    def struct(self, pools=None):
        k, v = (a[self.guard:] for a in (self.dev if pools is None else pools))
        return mfa.PagedKVCache.make(self.cprec, self.page, self.max_pages, self.num_pages,
                                     self.Hkv, self.D, k, v, self.table, self.lens,
                                     strides=self.strides, k_scale=self.scales[0],
                                     v_scale=self.scales[1], k_zero_point=self.zps[0],
                                     v_zero_point=self.zps[1])

    def stored(self, x, which):
        """The bytes the pool must hold for the rows x [B, H_kv, R, D]: uint8 [B, H_kv, R, D * es]."""
        x = x.contiguous()
        B, Hkv, R, D = x.shape
        if self.cprec == P.INT8:
            q = ol.quantize(x.float().cpu().numpy(), ol.INT8, self.scales[which], self.zps[which])
            return q.reshape(B, Hkv, R, D)
        return x.view(torch.int16).cpu().numpy().view(np.uint8).reshape(B, Hkv, R, 2 * D)

    def scatter(self, which, rows, lens, new_lens, cap):
        """The CPU model of one append into self.host[which]."""
        R = rows.shape[2]
        a = self.host[which]
        for b in range(self.B):
            n = R if new_lens is None else min(max(int(new_lens[b]), 0), R)
            for r in range(n):
                t = int(lens[b]) - n + r
                if t < 0 or t >= cap:
                    continue
                pg = min(max(int(self.table_np[b, t // self.page]), 0), self.num_pages - 1)
                for h in range(self.Hkv):
                    off = self.guard + self.es * (pg * self.strides[0] + h * self.strides[1] +
                                                  (t % self.page) * self.strides[2])
                    a[off:off + rows.shape[3]] = rows[b, h, r]

    def append(self, k, v, lens, max_seq_len, new_lens=None, set_lens=True, model=True):
        """lens: the lengths after the append.  Device call, then the CPU model."""
        R = k.shape[2]
        if set_lens:
            self.lens.copy_(torch.tensor(lens, dtype=torch.int32))
        nl = None if new_lens is None else torch.tensor(new_lens, dtype=torch.int32, device=DEV)
        desc = mfa.PagedAppendDescriptor.make(self.prec, self.B, self.Hkv, R, self.D, max_seq_len)
        mfa.paged_kv_append(desc, k, v, self.struct(), new_lens=nl)
        torch.cuda.synchronize()
        if model:
            cap = min(max_seq_len, self.max_pages * self.page)
            self.scatter(0, self.stored(k, 0), lens, new_lens, cap)
            self.scatter(1, self.stored(v, 1), lens, new_lens, cap)
        return desc

    def check(self, what=""):
        for i, name in enumerate("KV"):
            got = self.dev[i].cpu().numpy()
            bad = np.flatnonzero(got != self.host[i])
            assert bad.size == 0, (f"{what}: {name} allocation differs in {bad.size} bytes, first at "
                                   f"{bad[0]} (pool starts at {self.guard}, ends at "
                                   f"{got.size - self.guard})")


def rows(B, Hkv, R, D, prec, seed, scale=1.0):
    """Random new rows [B, H_kv, R, D] on the device in `prec`."""
    x = np.random.default_rng(seed).standard_normal((B, Hkv, R, D)).astype(np.float32) * scale
    return to_device(x, prec)


# ------------------------------------------------------------------ 1. 16-bit scatter
@pytest.mark.parametrize("prec", [P.FP16, P.BF16], ids=["f16", "bf16"])
def test_16bit_scatter(gpu, prec):
    # Lengths after the append (34, 5, 3): positions 29..33 straddle a page boundary, 0..4 start
    # a sequence, and -2, -1 (rows 0 and 1 of the last sequence) are dropped.
    B, Hkv, R, D, page = 3, 2, 5, 72, 32
    rig = Rig(prec, prec, B, Hkv, D, page, shuffled_table(B, 2, 9), 9)
    rig.append(rows(B, Hkv, R, D, prec, 1), rows(B, Hkv, R, D, prec, 2), (34, 5, 3), 64)
    rig.check("straddle / start / negative positions")
    # The model itself: 5 + 5 + 3 rows written, not 15.
    changed = np.count_nonzero(rig.host[0] != pattern(rig.host[0].size, 7))
    assert 12 * Hkv * D * 2 < changed <= 13 * Hkv * D * 2


@pytest.mark.parametrize("prec", [P.FP16, P.BF16], ids=["f16", "bf16"])
def test_16bit_decode_step(gpu, prec):
    B, Hkv, R, D, page = 2, 1, 1, 256, 128
    rig = Rig(prec, prec, B, Hkv, D, page, shuffled_table(B, 3, 7), 7)
    rig.append(rows(B, Hkv, R, D, prec, 3), rows(B, Hkv, R, D, prec, 4), (129, 300), 384)
    rig.check("decode step")


# ------------------------------------------------------------------ 2. INT8 bit-exactness
@pytest.mark.parametrize("prec", [P.FP16, P.BF16], ids=["f16", "bf16"])
def test_int8_ties_and_saturation(gpu, prec):
    # Inputs on a 0.125 grid in [-40, 40] over scale 0.25: quotients on a 0.5 grid up to +-160.
    B, Hkv, R, D, page = 2, 2, 7, 64, 32
    rng = np.random.default_rng(5)
    xs = [seen(rng.integers(-320, 321, (B, Hkv, R, D)).astype(np.float32) * 0.125, prec)
          for _ in range(2)]
    for x in xs:
        quo = x.astype(np.float64) / 0.25
        ties = np.mean(np.abs(quo - np.floor(quo) - 0.5) == 0.0)
        sat = np.mean(np.abs(quo) > 131.0)            # past either end whatever the zero point
        assert ties >= 0.25 and sat >= 0.05, (ties, sat)
    rig = Rig(prec, P.INT8, B, Hkv, D, page, shuffled_table(B, 2, 6), 6, scales=(0.25, 0.25),
              zps=(3, -7))
    rig.append(to_device(xs[0], prec), to_device(xs[1], prec), (40, 7), 64)
    rig.check("ties and saturation")


@pytest.mark.parametrize("prec", [P.FP16, P.BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("D", [128, 80])
def test_int8_normal_inputs(gpu, prec, D):
    B, Hkv, R, page = 3, 2, 5, 32
    k, v = rows(B, Hkv, R, D, prec, 11), rows(B, Hkv, R, D, prec, 12, scale=3.0)
    scales = tuple(np.float32(float(x.float().abs().max()) / 120.0) for x in (k, v))
    rig = Rig(prec, P.INT8, B, Hkv, D, page, shuffled_table(B, 2, 8), 8, scales=scales, zps=(3, 3))
    rig.append(k, v, (34, 5, 64), 64)
    rig.check(f"normal inputs D {D}")


def test_int8_zero_point_at_the_edge(gpu):
    B, Hkv, R, D, page, prec = 2, 1, 4, 32, 32, P.FP16
    k, v = rows(B, Hkv, R, D, prec, 13), rows(B, Hkv, R, D, prec, 14)
    rig = Rig(prec, P.INT8, B, Hkv, D, page, shuffled_table(B, 1, 3), 3, scales=(0.02, 0.02),
              zps=(128, -128))
    rig.append(k, v, (4, 30), 32)
    rig.check("zero points 128 / -128")
    kq = rig.stored(k, 0).view(np.int8)
    assert kq.min() < 127 and kq.max() == 127          # the negative inputs are still resolved


# ------------------------------------------------------------------ 3. ragged new_lens
@pytest.mark.parametrize("cprec", [P.FP16, P.INT8], ids=["f16", "i8"])
def test_ragged_new_lens(gpu, cprec):
    B, Hkv, R, D, page, prec = 5, 2, 6, 64, 32, P.FP16
    rig = Rig(prec, cprec, B, Hkv, D, page, shuffled_table(B, 3, 17), 17, scales=(0.03, 0.04),
              zps=(3, -5) if cprec == P.INT8 else (0, 0))
    before = [h.copy() for h in rig.host]
    new_lens = (0, 6, 2, 9, -1)                        # 9 counts as 6, -1 as 0
    rig.append(rows(B, Hkv, R, D, prec, 21), rows(B, Hkv, R, D, prec, 22), (10, 40, 33, 70, 5), 96,
               new_lens=new_lens)
    rig.check("ragged")
    # The model itself: 6 + 2 + 6 rows x 2 kv heads x D elements changed at most, none for the
    # sequences with 0 rows (their pages hold the pattern).
    for h, b in zip(rig.host, before):
        assert 0 < np.count_nonzero(h != b) <= 14 * Hkv * D * rig.es
        for seq in (0, 4):
            for pg in rig.table_np[seq]:
                lo = rig.guard + pg * rig.guard
                assert np.array_equal(h[lo:lo + rig.guard], b[lo:lo + rig.guard])


# ------------------------------------------------------------------ 4. bounds
@pytest.mark.parametrize("max_seq_len", [50, 100], ids=["max_seq_len", "table-span"])
def test_rows_past_the_cap_are_dropped(gpu, max_seq_len):
    # Two pages of 32 keys per sequence: the cap is min(max_seq_len, 64).  Lengths 54 / 68 / 50
    # with R 8: positions 46..53, 60..67, 42..49; those at or past the cap are dropped.
    B, Hkv, R, D, page, prec = 3, 2, 8, 64, 32, P.FP16
    rig = Rig(prec, prec, B, Hkv, D, page, shuffled_table(B, 2, 8), 8)
    before = rig.host[0].copy()
    rig.append(rows(B, Hkv, R, D, prec, 31), rows(B, Hkv, R, D, prec, 32), (54, 68, 50),
               max_seq_len)
    rig.check(f"cap {min(max_seq_len, 64)}")
    kept = {50: 4 + 0 + 8, 100: 8 + 4 + 8}[max_seq_len]
    assert np.count_nonzero(rig.host[0] != before) <= kept * Hkv * D * 2
    assert np.count_nonzero(rig.host[0] != before) > (kept - 1) * Hkv * D * 2


def test_out_of_range_table_entries_stay_in_the_pools(gpu):
    # Entries -1 and num_pages, for pages that get written: the rows land in page 0 and in page
    # num_pages - 1.  (Both are within one page of the pool, so the guard bands would take the
    # writes of a kernel that did not clamp.)
    B, Hkv, R, D, page, prec, num_pages = 2, 2, 4, 64, 32, P.FP16, 5
    table = np.array([[2, -1], [num_pages, 3]], np.int32)
    rig = Rig(prec, prec, B, Hkv, D, page, table, num_pages)
    before = [h.copy() for h in rig.host]
    rig.append(rows(B, Hkv, R, D, prec, 41), rows(B, Hkv, R, D, prec, 42), (36, 4), 64)
    rig.check("clamped page ids")
    g = rig.guard
    for h, b in zip(rig.host, before):
        assert not np.array_equal(h[g:2 * g], b[g:2 * g])                    # page 0
        assert not np.array_equal(h[g * num_pages:g * (num_pages + 1)],      # the last page
                                  b[g * num_pages:g * (num_pages + 1)])


# ------------------------------------------------------------------ 5. layouts
@pytest.mark.parametrize("cprec", [P.FP16, P.INT8], ids=["f16", "i8"])
def test_projection_buffer_views_and_slot_major_pool(gpu, cprec):
    # K and V as BSHD views of one [B, R, 2 * H_kv * D] projection output, at different base
    # offsets; the pool laid out [page][slot][kv head][d].
    B, Hkv, R, D, page, prec = 2, 3, 5, 80, 32, P.FP16
    buf = to_device(np.random.default_rng(51).standard_normal((B, R, 2 * Hkv * D)), prec)
    k = buf[..., :Hkv * D].view(B, R, Hkv, D).permute(0, 2, 1, 3)
    v = buf[..., Hkv * D:].view(B, R, Hkv, D).permute(0, 2, 1, 3)
    assert k.stride() == (R * 2 * Hkv * D, D, 2 * Hkv * D, 1) and v.data_ptr() != k.data_ptr()
    rig = Rig(prec, cprec, B, Hkv, D, page, shuffled_table(B, 2, 6), 6, layout="sh",
              scales=(0.03, 0.04), zps=(3, -5) if cprec == P.INT8 else (0, 0))
    rig.append(k, v, (34, 5), 64)
    rig.check("projection views, slot-major pool")


# ------------------------------------------------------------------ 6. a pool beyond 2^31 bytes
def test_pool_beyond_2_31_bytes(gpu):
    # 128 KiB pages, 16400 of them (2.1 GiB per pool, untouched but for its first and last
    # pages): the sequence's page is the pool's last, past a 32-bit byte offset.
    B, Hkv, R, D, page, prec, num_pages = 1, 1, 3, 256, 256, P.FP16, 16400
    pb = Hkv * page * D * 2
    k, v = rows(B, Hkv, R, D, prec, 61), rows(B, Hkv, R, D, prec, 62)
    table = torch.tensor([[num_pages - 1]], dtype=torch.int32, device=DEV)
    lens = torch.tensor([200], dtype=torch.int32, device=DEV)
    pools, want = [], []
    for i, x in enumerate((k, v)):
        pool = torch.empty(num_pages * pb, dtype=torch.uint8, device=DEV)
        first, last = pattern(pb, 70 + i), pattern(pb, 80 + i)
        pool[:pb] = torch.from_numpy(first).to(DEV)
        pool[-pb:] = torch.from_numpy(last).to(DEV)
        bits = x.view(torch.int16).cpu().numpy().view(np.uint8).reshape(R, 2 * D)
        for r in range(R):
            t = 200 - R + r
            last[t * 2 * D:(t + 1) * 2 * D] = bits[r]
        pools.append(pool)
        want.append((first, last))
    cache = mfa.PagedKVCache.make(prec, page, 1, num_pages, Hkv, D, pools[0], pools[1], table, lens)
    mfa.paged_kv_append(mfa.PagedAppendDescriptor.make(prec, B, Hkv, R, D, page), k, v, cache)
    torch.cuda.synchronize()
    for pool, (first, last) in zip(pools, want):
        assert np.array_equal(pool[:pb].cpu().numpy(), first)
        assert np.array_equal(pool[-pb:].cpu().numpy(), last)


# ------------------------------------------------------------------ 7. round trip with the reader
def decode(rig, q, lens_B, R, causal, pools=None):
    """mfa_paged_decode_forward over the rig's first lens_B sequences; (O, L)."""
    _, H, _, D = q.shape
    base = mfa.AttentionDescriptor.make(low_precision=True, precision=rig.prec, causal=causal)
    desc = mfa.PagedDecodeDescriptor.make(base, lens_B, H, R, D, rig.max_pages * rig.page,
                                          Hkv=rig.Hkv)
    o = torch.full((lens_B, H, R, D), float("nan"), dtype=torch.float32, device=DEV)
    l = torch.full((lens_B, H, R), float("nan"), dtype=torch.float16, device=DEV)
    mfa.paged_decode_forward(desc, q, rig.struct(pools), o, l)
    torch.cuda.synchronize()
    return o, l


def check_oracle(o, l, O, L, what):
    """The tolerances of test_paged_decode_gpu.py::check."""
    on, ln = o.cpu().numpy(), l.float().cpu().numpy()
    eo, el = maxerr(on, O), maxerr(ln, L)
    omax, lmax = max(1.0, float(np.abs(O).max())), float(np.abs(L).max())
    print(f"{what}: O err {eo:.3e} (bound {2e-3 * omax:.3e}) L err {el:.3e} "
          f"(bound {7e-3 + 2 ** -11 * lmax:.3e})")
    assert np.isfinite(on).all() and np.isfinite(ln).all()
    assert eo < 2e-3 * omax
    assert el < 7e-3 + 2 ** -11 * lmax


@pytest.mark.parametrize("cprec", [P.FP16, P.INT8], ids=["f16", "i8"])
def test_round_trip_with_the_reader(gpu, cprec):
    B, H, Hkv, D, page, prec, ZP = 2, 8, 2, 128, 64, P.FP16, 3
    rng = np.random.default_rng(71)
    # What each append brings: a ragged prefill chunk, then two decode steps.
    steps = [(70, (70, 33), (70, 33)), (1, None, (71, 34)), (1, None, (72, 35))]
    new = [[seen(rng.standard_normal((B, Hkv, R, D)).astype(np.float32), prec) for _ in "KV"]
           for R, _, _ in steps]
    i8 = cprec == P.INT8
    scales = tuple(np.float32(max(float(np.abs(s[i]).max()) for s in new) / 120.0)
                   for i in range(2)) if i8 else (1.0, 1.0)
    rig = Rig(prec, cprec, B, Hkv, D, page, shuffled_table(B, 2, 6), 6, scales=scales,
              zps=(ZP, ZP) if i8 else (0, 0))
    # The values the reader sees: per sequence [Hkv, len, D], grown by the same rule.
    seqs = [[np.zeros((Hkv, 0, D), np.float32) for _ in range(B)] for _ in "KV"]

    def stored_values(x, which):
        if not i8:
            return x
        q = ol.quantize(x, ol.INT8, rig.scales[which], ZP).view(np.int8).reshape(x.shape)
        return (q.astype(np.float32) - ZP) * np.float32(rig.scales[which])

    for (R, new_lens, lens), kv in zip(steps, new):
        rig.append(to_device(kv[0], prec), to_device(kv[1], prec), lens, 2 * page, new_lens=new_lens)
        rig.check(f"append R {R}")
        for which in range(2):
            sv = stored_values(kv[which], which)
            for b in range(B):
                n = R if new_lens is None else new_lens[b]
                seqs[which][b] = np.concatenate([seqs[which][b], sv[b, :, :n]], axis=1)
        assert [s.shape[1] for s in seqs[0]] == list(lens)
        host_pools = [torch.from_numpy(h).to(DEV) for h in rig.host]
        if R > 1:   # the chunk: CAUSAL with the matching R on the full-length sequence
            nb, causal = 1, True
        else:
            nb, causal = B, False
        Q = seen(rng.standard_normal((nb, H, R, D)).astype(np.float32), prec)
        q = to_device(Q, prec)
        o, l = decode(rig, q, nb, R, causal)
        o2, l2 = decode(rig, q, nb, R, causal, pools=host_pools)
        assert torch.equal(o, o2) and torch.equal(l, l2), f"R {R}: differs from the host-filled pool"
        # Keys == rows for the chunk, so the oracle's top-left diagonal is the cache's.
        ref = [ol.attention(Q[b:b + 1], seqs[0][b][None], seqs[1][b][None], causal=causal)
               for b in range(nb)]
        check_oracle(o, l, np.concatenate([r["O"] for r in ref]),
                     np.concatenate([r["L"] for r in ref]), f"{cprec.name} R {R} lens {lens}")


# ------------------------------------------------------------------ 8. graph
@pytest.mark.parametrize("cprec", [P.FP16, P.INT8], ids=["f16", "i8"])
def test_graph_of_lens_append_decode(gpu, cprec):
    # lens += 1 -> append (R 1) -> decode captured once and replayed with new rows in the static
    # buffers: pool bytes and O after each replay equal the eager sequence of the same steps.
    B, H, Hkv, D, page, prec, start = 2, 8, 2, 128, 64, P.FP16, (100, 63)
    rig = Rig(prec, cprec, B, Hkv, D, page, shuffled_table(B, 2, 6), 6, scales=(0.03, 0.04),
              zps=(3, -5) if cprec == P.INT8 else (0, 0))
    rig.append(rows(B, Hkv, 100, D, prec, 81), rows(B, Hkv, 100, D, prec, 82), start, 2 * page,
               new_lens=start)                           # real values under every key read below
    rig.check("prefix")
    initial = [d.clone() for d in rig.dev]
    feed = [(rows(B, Hkv, 1, D, prec, 90 + i), rows(B, Hkv, 1, D, prec, 95 + i),
             rows(B, H, 1, D, prec, 100 + i)) for i in range(3)]
    k, v, q = (torch.empty_like(t) for t in feed[0])
    o = torch.empty((B, H, 1, D), dtype=torch.float32, device=DEV)
    l = torch.empty((B, H, 1), dtype=torch.float16, device=DEV)
    base = mfa.AttentionDescriptor.make(low_precision=True, precision=prec)
    ddesc = mfa.PagedDecodeDescriptor.make(base, B, H, 1, D, 2 * page, Hkv=Hkv)
    adesc = mfa.PagedAppendDescriptor.make(prec, B, Hkv, 1, D, 2 * page)
    pc = rig.struct()
    st = torch.cuda.Stream()
    torch.cuda.synchronize()

    def step():
        rig.lens.add_(1)
        mfa.paged_kv_append(adesc, k, v, pc, stream=st.cuda_stream)
        mfa.paged_decode_forward(ddesc, q, pc, o, l, stream=st.cuda_stream)

    def reset():
        rig.lens.copy_(torch.tensor(start, dtype=torch.int32))
        for d, i in zip(rig.dev, initial):
            d.copy_(i)

    def load(i):
        for dst, src in zip((k, v, q), feed[i]):
            dst.copy_(src)

    with torch.cuda.stream(st):
        load(0)
        step()                                           # warm-up: nothing allocates under capture
        st.synchronize()
        reset()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            step()
        reset()                                          # capture ran nothing; start clean anyway
        replayed = []
        for i in range(3):
            load(i)
            o.fill_(float("nan"))
            graph.replay()
            st.synchronize()
            replayed.append(([d.clone() for d in rig.dev], o.clone(), l.clone(), rig.lens.clone()))
        reset()
        for i in range(3):
            load(i)
            o.fill_(float("nan"))
            step()
            st.synchronize()
            pools, ro, rl, rlens = replayed[i]
            assert torch.equal(rig.lens, rlens) and rlens.tolist() == [start[0] + i + 1, start[1] + i + 1]
            assert all(torch.equal(a, b) for a, b in zip(rig.dev, pools)), f"pool bytes, step {i}"
            assert torch.isfinite(o).all()
            assert torch.equal(o, ro) and torch.equal(l, rl), f"O / L, step {i}"
            # ... and the CPU model of the same step.
            lens = (start[0] + i + 1, start[1] + i + 1)
            rig.scatter(0, rig.stored(feed[i][0], 0), lens, None, 2 * page)
            rig.scatter(1, rig.stored(feed[i][1], 1), lens, None, 2 * page)
            rig.check(f"eager step {i}")


# ------------------------------------------------------------------ 9. launch log
@pytest.mark.parametrize("cprec", [P.FP16, P.INT8], ids=["f16", "i8"])
def test_launch_log_names_the_plan(gpu, cprec):
    B, Hkv, R, D, page, prec = 2, 2, 3, 64, 32, P.FP16
    rig = Rig(prec, cprec, B, Hkv, D, page, shuffled_table(B, 2, 5), 5, scales=(0.03, 0.04))
    mfa.last_launches()
    desc = rig.append(rows(B, Hkv, R, D, prec, 111), rows(B, Hkv, R, D, prec, 112), (34, 3), 64)
    got = mfa.last_launches()
    plan = mfa.paged_kv_append_plan(desc, rig.struct())
    assert len(plan) == 1 and plan[0]["name"] == \
        f"mfa_paged_append_kernel<F16, {1 if cprec == P.INT8 else 0}>"
    assert [r["name"] for r in got] == [r["name"] for r in plan], (got, plan)
    assert got[0]["workgroups"] == plan[0]["workgroups"] and got[0]["threads"] == 256
