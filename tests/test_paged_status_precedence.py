"""What the paged K/V entry points (mfa_paged_decode_forward, mfa_paged_prefill_forward,
mfa_quantized_paged_prefill_forward, mfa_paged_kv_append) return for a call that is wrong in two
ways.  They share one cache checker
(PagedCacheView in csrc/mfa_api.cpp), and a shared checker can reorder its callers' checks without
any single-fault test noticing.  The order pinned here: descriptor nulls, INVALID_DESCRIPTOR
shape errors, UNSUPPORTED descriptor and cache rules, the empty call's success, null buffers,
alignment.  The forwards share one front end as well (paged_kv_forward) and apply their two size
limits in different orders, pinned per entry point at the end.  Every call is rejected on the
host, so no GPU is needed."""
import ctypes

import pytest

import mfa_amd as mfa
from harness import paged_cache_full as full

P = mfa.Precision
INVALID_DESCRIPTOR, UNSUPPORTED, INVALID_ARGUMENT = 1, 2, 4  # mfa_status_t


def _base(**kw):
    return mfa.AttentionDescriptor.make(low_precision=True, precision=P.FP16, **kw)


def _decode_desc(B=2, H=8, Hkv=2, R=1, D=128, **kw):
    return mfa.PagedDecodeDescriptor.make(_base(**kw), B, H, R, D, 1000, Hkv=Hkv)


def _prefill_desc(B=2, H=8, Hkv=2, R=300, D=128, **kw):
    return mfa.PagedPrefillDescriptor.make(_base(**kw), B, H, R, D, 1000, Hkv=Hkv)


def _append_desc(B=2, Hkv=2, R=1, D=128):
    return mfa.PagedAppendDescriptor.make(P.FP16, B, Hkv, R, D, 1000)


def _ref(x):
    return ctypes.byref(x) if x is not None else None


def _decode_call(d, c, first):
    return mfa.lib.mfa_paged_decode_forward(_ref(d), first, None, _ref(c), 0x200000, None, None)


def _prefill_call(d, c, first):
    return mfa.lib.mfa_paged_prefill_forward(_ref(d), first, None, None, _ref(c), 0x200000, None,
                                             None)


def _qprefill_call(d, c, first):
    return mfa.lib.mfa_quantized_paged_prefill_forward(_ref(d), first, None, None, _ref(c),
                                                       0x200000, None, None)


def _append_call(d, c, first):
    return mfa.lib.mfa_paged_kv_append(_ref(d), first, 0x200000, None, None, None, _ref(c), None)


ENTRY = {"decode": (_decode_desc, _decode_call), "prefill": (_prefill_desc, _prefill_call),
         "qprefill": (_prefill_desc, _qprefill_call), "append": (_append_desc, _append_call)}
ALL, FORWARDS = ("decode", "prefill", "qprefill", "append"), ("decode", "prefill", "qprefill")


def _edit(**fields):
    def apply(c):
        for k, v in fields.items():
            setattr(c, k, v)
    return apply


def _stride1_and_no_lens(c):
    c.seq_lens = None
    c.strides[1] += 4


# (name, entries, descriptor arguments, cache arguments, cache edit, null descriptor,
#  null first buffer, status, message part)
CASES = [
    ("null descriptor, page size 48", ALL, {}, {}, _edit(page_size=48), True, False,
     INVALID_ARGUMENT, "null descriptor or cache"),
    ("D = 0, page size 48", ALL, {"D": 0}, {}, _edit(page_size=48), False, False,
     INVALID_DESCRIPTOR, "empty shape"),
    ("H % Hkv, FP32 cache", FORWARDS, {"H": 8, "Hkv": 3}, {"prec": P.FP32}, None, False, False,
     INVALID_DESCRIPTOR, "heads over"),
    # An empty call does not excuse a bad cache.
    ("B = 0, page size 48", ALL, {"B": 0}, {}, _edit(page_size=48), False, False,
     UNSUPPORTED, "page size 48"),
    ("R = 0, FP32 cache", ALL, {"R": 0}, {"prec": P.FP32}, None, False, False,
     UNSUPPORTED, "cache precision 0"),
    ("first buffer null, k_pool misaligned", ALL, {}, {}, _edit(k_pool=0x300008), False, True,
     INVALID_ARGUMENT, "requires"),
    ("seq_lens null, stride 1 misaligned", ALL, {}, {}, _stride1_and_no_lens, False, False,
     UNSUPPORTED, "cache stride 1"),
    ("v_pool misaligned, D = 264", ALL, {"D": 264}, {}, _edit(v_pool=0x400002), False, False,
     UNSUPPORTED, "head dimension 264"),
    ("window mask, null query", FORWARDS, {"window": 64}, {}, None, False, True,
     UNSUPPORTED, "masks other than causal"),
]


@pytest.mark.parametrize("entry,case", [(e, c) for c in CASES for e in c[1]],
                         ids=lambda v: v if isinstance(v, str) else v[0])
def test_two_faults_return_the_earlier_phases_status(entry, case):
    _, _, dkw, ckw, edit, null_desc, null_first, want, part = case
    make, call = ENTRY[entry]
    d = make(**dkw)
    c = full(d, **ckw)
    if edit:
        edit(c)
    st = call(None if null_desc else d, c, None if null_first else 0x100000)
    msg = mfa.lib.mfa_last_error().decode()
    assert st == want, (st, msg)
    assert part in msg, msg


# B 65536, H 8, Hkv 2, R 4096: B * H * R = 2^31 query rows, one too many for every forward, and
# 65536 x 2 x 512 units, too many for decode's grid.  Decode checks its grid first, the prefills
# the rows (their block count, 2^24 here, can only exceed its limit when the rows do).
FIRST_LIMIT = {"decode": "units exceed the grid", "prefill": "too many query rows",
               "qprefill": "too many query rows"}


@pytest.mark.parametrize("entry", FORWARDS)
def test_both_size_limits_broken_returns_the_calls_first(entry):
    make, call = ENTRY[entry]
    d = make(B=65536, H=8, Hkv=2, R=4096, D=128)
    st = call(d, full(d), 0x100000)
    msg = mfa.lib.mfa_last_error().decode()
    assert st == UNSUPPORTED, (st, msg)
    assert FIRST_LIMIT[entry] in msg, msg
    assert msg.startswith({"decode": "paged decode:", "prefill": "paged prefill:",
                           "qprefill": "quantized paged prefill:"}[entry]), msg
