"""CPU tests of the causal sliding window of the paged K/V calls (MFA_SPARSITY_CAUSAL_WINDOW = 4 in
include/mfa/mfa.h; paged_kv_mask and decode_paged_span in csrc): which calls serve the value and
which reject it, the decode plan's span-sized split layout, the plain-causal limit of a huge
window, and the Python keyword.  The plan query runs the real dispatcher with launches recorded,
and a rejected call returns before anything touches a device, so no GPU is needed.  The GPU twin
is test_paged_window_gpu.py."""
import ctypes
import re

import pytest

import mfa_amd as mfa
from harness import paged_cache as cache, paged_cache_full as full

P = mfa.Precision
K = mfa.KernelType
OK, INVALID_DESCRIPTOR, UNSUPPORTED, INVALID_ARGUMENT = 0, 1, 2, 4  # mfa_status_t
CAUSAL_WINDOW = 4


def base(prec=P.FP16, **kw):
    return mfa.AttentionDescriptor.make(low_precision=True, precision=prec, **kw)


def decode_desc(B=2, H=8, Hkv=2, R=1, D=128, prec=P.FP16, max_seq_len=1000, **kw):
    return mfa.PagedDecodeDescriptor.make(base(prec, **kw), B, H, R, D, max_seq_len, Hkv=Hkv)


def prefill_desc(B=2, H=8, Hkv=2, R=300, D=128, prec=P.FP16, max_seq_len=1000, **kw):
    return mfa.PagedPrefillDescriptor.make(base(prec, **kw), B, H, R, D, max_seq_len, Hkv=Hkv)


def rows(plan):
    return [(r["name"], r["threads"], r["lds_bytes"], r["workgroups"]) for r in plan]


def last_error():
    return mfa.lib.mfa_last_error().decode()


def decode_status(d, c):
    return mfa.lib.mfa_paged_decode_forward(ctypes.byref(d), 0x100000, None, ctypes.byref(c),
                                            0x200000, None, None)


def prefill_status(fn, d, c):
    return fn(ctypes.byref(d), 0x100000, None, None, ctypes.byref(c), 0x200000, None, None)


def test_the_header_and_the_python_enum_agree():
    text = open(mfa.HEADER_PATH).read()
    assert re.search(r"MFA_SPARSITY_CAUSAL_WINDOW\s*=\s*4\b", text)
    assert re.search(r"MFA_SPARSITY_SLIDING_WINDOW\s*=\s*2\b", text)
    assert int(mfa.Sparsity.causalWindow) == CAUSAL_WINDOW
    assert "Page release" in text and "no reference counterpart" in text.lower()


def test_python_keyword_sets_the_new_value_and_leaves_the_old_ones():
    d = mfa.AttentionDescriptor.make(causal_window=1000)
    assert d.sparsity_pattern == CAUSAL_WINDOW and d.window_size == 1000
    d = mfa.AttentionDescriptor.make(causal_window=0)
    assert d.sparsity_pattern == CAUSAL_WINDOW and d.window_size == 0
    d = mfa.AttentionDescriptor.make(causal=True, window=64)
    assert d.sparsity_pattern == int(mfa.Sparsity.slidingWindow) == 2 and d.window_size == 64
    assert mfa.AttentionDescriptor.make(window=64).sparsity_pattern == 2
    assert mfa.AttentionDescriptor.make(causal=True).sparsity_pattern == int(mfa.Sparsity.causal)
    for kw in ({"causal": True}, {"window": 8}):
        with pytest.raises(ValueError):
            mfa.AttentionDescriptor.make(causal_window=8, **kw)


def test_the_three_paged_calls_and_their_plans_serve_the_value():
    d = decode_desc(causal_window=100)
    assert decode_status(decode_desc(B=0, causal_window=100), full(d)) == OK   # past every mask rule
    for c in (cache(d), cache(d, prec=P.INT8, k_scale=0.02, v_scale=0.03)):
        assert mfa.paged_decode_plan(d, c)[0]["name"].startswith("mfa_fwd_decode16_paged_kernel<")
    assert mfa.paged_decode_plan(decode_desc(R=5, causal_window=100))[0]["name"].startswith(
        "mfa_fwd_decode_paged_kernel<")
    p = prefill_desc(causal_window=100)
    empty = prefill_desc(B=0, causal_window=100)
    for fn in (mfa.lib.mfa_paged_prefill_forward, mfa.lib.mfa_quantized_paged_prefill_forward):
        assert prefill_status(fn, empty, full(p)) == OK
    assert [r["name"] for r in mfa.paged_prefill_plan(p, cache(p))] == \
        ["mfa_paged_window_prefill_kernel<F16, 128, 64>"]
    assert [r["name"] for r in mfa.quantized_paged_prefill_plan(p, cache(p))] == \
        ["mfa_paged_window_prefill_kernel<F16, 128, 64>"]
    c8 = cache(p, prec=P.INT8, k_scale=0.02, v_scale=0.03)
    assert [r["name"] for r in mfa.quantized_paged_prefill_plan(p, c8)] == \
        ["mfa_paged_window_prefill_kv8_kernel<F16, 128, 64>"]
    # INT8 pools stay the quantised entry's alone, under the window too.
    assert prefill_status(mfa.lib.mfa_paged_prefill_forward, p,
                          full(p, prec=P.INT8, k_scale=0.02, v_scale=0.03)) == UNSUPPORTED


@pytest.mark.parametrize("prec,tag", [(P.FP16, "F16"), (P.BF16, "BF16")])
@pytest.mark.parametrize("D,DP,BK", [(64, 64, 64), (128, 128, 64), (256, 256, 32)])
def test_window_prefill_instantiations_resolve(prec, tag, D, DP, BK):
    p = prefill_desc(D=D, prec=prec, causal_window=7)
    plain = prefill_desc(D=D, prec=prec, causal=True)
    for c8 in (False, True):
        kw = {"prec": P.INT8, "k_scale": 0.02, "v_scale": 0.03} if c8 else {}
        got = mfa.quantized_paged_prefill_plan(p, cache(p, **kw))
        want = mfa.quantized_paged_prefill_plan(plain, cache(plain, **kw))
        mid = "_kv8" if c8 else ""
        assert [r["name"] for r in got] == [f"mfa_paged_window_prefill{mid}_kernel<{tag}, {DP}, {BK}>"]
        # The same launch geometry as the causal kernel of the shape.
        assert [r[1:] for r in rows(got)] == [r[1:] for r in rows(want)]


def test_sliding_window_and_sparse_masks_stay_unsupported_on_the_paged_calls():
    d, p = decode_desc(), prefill_desc()
    for kw in ({"window": 64}, {"causal": True, "window": 64},
               {"sparse_mask": mfa.MaskType.sparseRanges},
               {"causal_window": 64, "sparse_mask": mfa.MaskType.sparseRanges}):
        assert decode_status(decode_desc(**kw), full(d)) == UNSUPPORTED, kw
        for fn in (mfa.lib.mfa_paged_prefill_forward, mfa.lib.mfa_quantized_paged_prefill_forward):
            assert prefill_status(fn, prefill_desc(**kw), full(p)) == UNSUPPORTED, kw
    for fn, dd in ((mfa.paged_decode_plan, decode_desc(window=64)),
                   (mfa.paged_prefill_plan, prefill_desc(window=64)),
                   (mfa.quantized_paged_prefill_plan, prefill_desc(window=64))):
        with pytest.raises(mfa.MFAError) as e:
            fn(dd)
        assert e.value.status == UNSUPPORTED
    # Values past the enum stay unknown.
    bad = decode_desc()
    bad.base.sparsity_pattern = 5
    assert decode_status(bad, full(d)) == UNSUPPORTED


def names_the_value(msg):
    return "MFA_SPARSITY_CAUSAL_WINDOW" in msg


def test_paged_mla_calls_reject_the_value_by_name():
    b = base(P.BF16, causal_window=64)
    d = mfa.PagedMLADecodeDescriptor.make(b, 2, 16, 1, 128, 512, 1024, P.BF16)
    c = mfa.PagedLatentCache.make(P.BF16, 64, 16, 32, 512)
    c.pool, c.block_table, c.seq_lens = 0x300000, 0x500000, 0x600000
    for fn in (mfa.lib.mfa_paged_mla_decode_forward, mfa.lib.mfa_paged_mla_prefill_forward):
        args = [ctypes.byref(d), 0x100000, 0x110000, 0x120000]
        if fn is mfa.lib.mfa_paged_mla_prefill_forward:
            args.append(None)   # new_lens
        st = fn(*args, ctypes.byref(c), 0x200000, None, None)
        assert st == UNSUPPORTED and names_the_value(last_error()), last_error()
    for plan in (mfa.paged_mla_decode_plan, mfa.paged_mla_prefill_plan):
        with pytest.raises(mfa.MFAError) as e:
            plan(d)
        assert e.value.status == UNSUPPORTED and names_the_value(str(e.value))


def test_dense_multihead_calls_reject_the_value_by_name():
    d = mfa.MultiHeadDescriptor.make(base(causal_window=64), 1, 4, 256, 128)
    for kind in (K.forward, K.backwardQuery, K.backwardKeyValue):
        with pytest.raises(mfa.MFAError) as e:
            mfa.multihead_plan(d, kind)
        assert e.value.status == UNSUPPORTED and names_the_value(str(e.value)), kind
    buf = mfa.AttentionBuffers()
    for f in ("Q", "K", "V", "O", "L", "D", "dO", "dV", "dK", "dQ"):
        setattr(buf, f, 0x100000)
    for fn in ("mfa_multihead_forward", "mfa_multihead_backward", "mfa_multihead_backward_query",
               "mfa_multihead_backward_key_value"):
        st = getattr(mfa.lib, fn)(ctypes.byref(d), ctypes.byref(buf), None)
        assert st == UNSUPPORTED and names_the_value(last_error()), (fn, st, last_error())
    # Was: INVALID_DESCRIPTOR "unknown sparsity pattern"; values past the enum still are.
    d.base.sparsity_pattern = 5
    with pytest.raises(mfa.MFAError) as e:
        mfa.multihead_plan(d)
    assert e.value.status == INVALID_DESCRIPTOR


def test_quantized_calls_reject_the_value_by_name():
    b = mfa.AttentionDescriptor.make(64, 512, 128, low_precision_intermediates=True,
                                     causal_window=64)
    d = mfa.quantized_descriptor(b, P.FP16, P.INT8, P.INT8, B=1, H=4)
    q = mfa.QuantizedTensor()
    q.data, q.precision, q.scale = 0x100000, int(P.FP16), 1.0
    k = mfa.QuantizedTensor()
    k.data, k.precision, k.scale = 0x200000, int(P.INT8), 0.02
    ref = ctypes.byref
    lib = mfa.lib
    calls = {
        "forward": lambda: lib.mfa_quantized_forward(ref(d), ref(q), ref(k), ref(k), 0x300000,
                                                     0x400000, None, None),
        "from_float": lambda: lib.mfa_quantized_forward_from_float(
            ref(d), 0x100000, 0x200000, 0x200000, int(P.FP16), int(P.FP16), int(P.FP16),
            int(P.INT8), 0, 0, 0x300000, 0x400000, None, None),
        "backward_query": lambda: lib.mfa_quantized_backward_query(
            ref(d), ref(q), ref(k), ref(k), 0x300000, 0x500000, 0x400000, 0x600000, 0x700000, None),
        "backward_key_value": lambda: lib.mfa_quantized_backward_key_value(
            ref(d), ref(q), ref(k), ref(k), 0x500000, 0x400000, 0x700000, 0x600000, 0x800000, None),
    }
    for name, call in calls.items():
        st = call()
        assert st == UNSUPPORTED and names_the_value(last_error()), (name, st, last_error())
    for kind in (K.forward, K.backwardQuery, K.backwardKeyValue):
        with pytest.raises(mfa.MFAError) as e:
            mfa.quantized_plan(d, kind)
        assert e.value.status == UNSUPPORTED and names_the_value(str(e.value)), kind


def test_mla_forwards_reject_the_value_by_name():
    d = mfa.MLADescriptor()
    d.base = base(P.FP16, causal_window=64)
    d.batch_size, d.num_heads = 1, 4
    d.sequence_length_q, d.sequence_length_kv = 64, 512
    d.head_dim, d.kv_latent_dim = 128, 512
    d.precision = int(P.FP16)
    st = mfa.lib.mfa_mla_forward(ctypes.byref(d), 0x100000, 0x110000, 0x120000, 0x130000, 0x140000,
                                 0x150000, 0x200000, 0x210000, None)
    assert st == UNSUPPORTED and names_the_value(last_error()), last_error()
    st = mfa.lib.mfa_mla_forward_absorbed(ctypes.byref(d), 0x100000, 0x110000, 0x120000, 0x130000,
                                          0x140000, 0x200000, 0x210000, None)
    assert st == UNSUPPORTED and names_the_value(last_error()), last_error()


# ------------------------------------------------------------------ the decode plan's span
def test_decode_layout_follows_the_window_not_the_cache():
    # span = min(cap, W + R + 31) = 1032 keys: the grid of the causal call over max_seq_len 1032,
    # whatever the cache's own cap (32768: 32 splits of 1024 keys per unit without the window).
    kw = dict(B=2, H=8, Hkv=2, R=1, D=128)
    for prec8 in (False, True):
        ckw = {"prec": P.INT8, "k_scale": 0.02, "v_scale": 0.03} if prec8 else {}
        win = decode_desc(max_seq_len=32768, causal_window=1000, **kw)
        ref = decode_desc(max_seq_len=1032, causal=True, **kw)
        far = decode_desc(max_seq_len=32768, causal=True, **kw)
        got = rows(mfa.paged_decode_plan(win, cache(win, page=256, **ckw)))
        assert got == rows(mfa.paged_decode_plan(ref, cache(ref, page=256, **ckw)))
        assert [r[0].split("<")[0] for r in got] == ["mfa_fwd_decode16_paged_kernel",
                                                    "mfa_decode_merge_kernel"]
        whole = rows(mfa.paged_decode_plan(far, cache(far, page=256, **ckw)))
        assert whole[0][3] > 8 * got[0][3], (whole, got)


def test_decode_span_in_one_split_is_fused():
    # W + R + 31 = 300 + 4 + 31 = 335 keys: fewer than 32 tiles, one split, no merge launch.
    kw = dict(B=2, H=8, Hkv=2, R=4, D=64, prec=P.BF16)
    win = decode_desc(max_seq_len=32768, causal_window=300, **kw)
    ref = decode_desc(max_seq_len=335, causal=True, **kw)
    got = rows(mfa.paged_decode_plan(win, cache(win, page=256)))
    assert got == rows(mfa.paged_decode_plan(ref, cache(ref, page=256)))
    assert len(got) == 1 and got[0][3] == 2 * 2          # B x H_kv units, one split each
    # The 32-row form as well.
    win = decode_desc(max_seq_len=32768, causal_window=300, **{**kw, "R": 5})
    ref = decode_desc(max_seq_len=336, causal=True, **{**kw, "R": 5})
    got = rows(mfa.paged_decode_plan(win, cache(win, page=256)))
    assert got == rows(mfa.paged_decode_plan(ref, cache(ref, page=256)))
    assert [r[0] for r in got] == ["mfa_fwd_decode_paged_kernel<BF16, 64, 0>"]


@pytest.mark.parametrize("W", [2 ** 32 - 1, 2 ** 31 - 1, 2 ** 30, 32768, 32768 - 1 - 31])
def test_a_window_that_covers_the_cap_plans_the_causal_call(W):
    # W + R + 31 >= cap: exactly the causal call's layout (and 64-bit arithmetic for the sum).
    for R in (1, 5):
        kw = dict(B=1, H=8, Hkv=2, R=R, D=128, max_seq_len=32768)
        win, ref = decode_desc(causal_window=W, **kw), decode_desc(causal=True, **kw)
        assert win.base.window_size == W
        assert rows(mfa.paged_decode_plan(win, cache(win, page=256))) == \
            rows(mfa.paged_decode_plan(ref, cache(ref, page=256)))
    p, pr = prefill_desc(causal_window=W), prefill_desc(causal=True)
    assert [r[1:] for r in rows(mfa.paged_prefill_plan(p, cache(p)))] == \
        [r[1:] for r in rows(mfa.paged_prefill_plan(pr, cache(pr)))]


def test_the_span_never_exceeds_the_caches_own_cap():
    # The layout follows min(max_seq_len, pages x page size, W + R + 31): a short table wins.
    d = decode_desc(B=1, max_seq_len=32768, causal_window=4096)
    short = mfa.PagedKVCache.make(P.FP16, 64, 7, 8, 2, 128)      # 448 keys at most
    assert [r["name"] for r in mfa.paged_decode_plan(d, short)] == \
        ["mfa_fwd_decode16_paged_kernel<F16, 128, 0>"]
