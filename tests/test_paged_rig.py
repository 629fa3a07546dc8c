"""CPU tests of tests/paged_rig.py's numpy layer.  Every paged GPU test rests on two things the
rig builds: a cache whose slots outside the sequences hold a poison value, reached through a block
table, and the key position of every query row.  Checked here against a gather and a brute-force
loop, for 16-bit K/V, INT8 K/V and latent pools."""
import numpy as np
import pytest

from paged_rig import DEAD_LENS, DEAD_NEW, DEAD_R, positions, scatter

LENS, PAGE, SPARE = (97, 0, 64), 32, 3
OPTIONS = [dict(shuffle=True), dict(shuffle=False), dict(shuffle=True, seed=5, table_fill=10 ** 6)]


def sequences(kind):
    """(seqs, fill): per-sequence arrays for scatter() and the poison of that kind of pool."""
    rng = np.random.default_rng(3)
    if kind == "latent":
        return ([rng.standard_normal((c, 16)).astype(np.float32) for c in LENS],), np.nan
    if kind == "int8":
        # Bytes 0..126 only, so that no owned slot holds the fill byte 0x7f.
        return tuple([rng.integers(0, 0x7f, (2, c, 8), dtype=np.int8) for c in LENS]
                     for _ in range(2)), 0x7f
    return tuple([rng.standard_normal((2, c, 8)).astype(np.float32) for c in LENS]
                 for _ in range(2)), np.nan


@pytest.mark.parametrize("opts", OPTIONS, ids=["shuffled", "in-order", "table-fill"])
@pytest.mark.parametrize("kind", ["16-bit", "int8", "latent"])
def test_scatter_layout(kind, opts):
    seqs, fill = sequences(kind)
    pools, table = scatter(seqs, PAGE, spare=SPARE, fill=fill, **opts)
    table_fill = opts.get("table_fill", 0)
    npg = [-(-c // PAGE) for c in LENS]
    num_pages = sum(npg) + SPARE
    assert len(pools) == len(seqs) and table.dtype == np.int32
    assert table.shape == (len(LENS), max(1, max(npg)) + (1 if table_fill else 0))
    owned = [int(table[b, j]) for b in range(len(LENS)) for j in range(npg[b])]
    assert len(set(owned)) == len(owned) == sum(npg)
    assert all(0 <= i < num_pages for i in owned)
    if not opts["shuffle"]:
        assert owned == list(range(sum(npg)))
    for b in range(len(LENS)):
        assert (table[b, npg[b]:] == table_fill).all()
    for pool, xs in zip(pools, seqs):
        assert pool.shape == (num_pages,) + xs[0].shape[:-2] + (PAGE, xs[0].shape[-1])
        assert pool.dtype == (np.int8 if kind == "int8" else np.float32)
        unowned = np.ones(pool.shape, bool)
        for b, c in enumerate(LENS):
            got = np.concatenate([pool[table[b, j]] for j in range(npg[b])] or
                                 [pool[0][..., :0, :]], axis=-2)[..., :c, :]
            assert np.array_equal(got, xs[b])            # the gather returns the sequence exactly
            for j in range(npg[b]):
                unowned[table[b, j], ..., :min(PAGE, c - j * PAGE), :] = False
        assert unowned.sum() == pool.size - sum(x.size for x in xs)
        assert unowned[[i for i in range(num_pages) if i not in owned]].all()   # the spare pages
        poison = (pool == 0x7f) if kind == "int8" else np.isnan(pool)
        assert np.array_equal(poison, unowned)           # the fill in every such slot, and no other


def test_random_fill_changes_only_unowned_slots():
    seqs, _ = sequences("int8")
    (k0, v0), t0 = scatter(seqs, PAGE, spare=SPARE, fill=0x7f)
    (k1, v1), t1 = scatter(seqs, PAGE, spare=SPARE, fill="random")
    assert np.array_equal(t0, t1)
    for clean, noisy in ((k0, k1), (v0, v1)):
        owned = clean != 0x7f
        assert np.array_equal(clean[owned], noisy[owned])
        assert len(np.unique(noisy[~owned])) > 200       # bytes of the whole range


def brute_force(lens, new_lens, R, causal, cap, decode):
    out = []
    for b, c in enumerate(lens):
        c = max(c, 0)
        if cap is not None:
            c = min(c, cap)
        n = R
        if new_lens is not None:
            n = min(max(new_lens[b], 0), R)
        row = []
        for q in range(R):
            t = c - n + q
            if q >= n or c == 0 or (t < 0 and (causal or not decode)):
                row.append(-1)                 # not the sequence's row, no key, or before key 0
            else:
                row.append(t if causal else c - 1)
        out.append(row)
    return np.array(out, np.int64).reshape(len(lens), R)


@pytest.mark.parametrize("lens,new_lens,R", [
    (DEAD_LENS, DEAD_NEW, DEAD_R),                 # new_lens 0, negative, above R, above len; len 0
    ((300, 160, 97), (160, 160, 33), 160),
    ((260, 129), None, 130),
    ((0, 3, 40), None, 5),
    ((5,), (9,), 9),
    ((0, 0), (4, 0), 9),
], ids=["dead", "ragged", "uniform", "short", "before-key-0", "empty"])
def test_positions_equal_a_brute_force_loop(lens, new_lens, R):
    for causal in (True, False):
        for cap in (None, 64):
            for decode in (False, True):
                got = positions(lens, new_lens, R, causal, cap, decode)
                assert got.dtype == np.int64 and got.shape == (len(lens), R)
                assert np.array_equal(got, brute_force(lens, new_lens, R, causal, cap, decode)), \
                    (causal, cap, decode)
    assert np.array_equal(positions(lens, new_lens, R), positions(lens, new_lens, R, True, None))


def test_positions_of_the_dead_row_set():
    pos = positions(DEAD_LENS, DEAD_NEW, DEAD_R)
    assert [(p >= 0).sum() for p in pos] == [0, 0, 20, 0, DEAD_R]
    assert pos[2, 13] == 0 and pos[2, 32] == 19 and pos[4, 0] == 50
