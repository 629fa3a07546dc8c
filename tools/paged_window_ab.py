#!/usr/bin/env python3
"""Timing of the causal-window paged decode (MFA_SPARSITY_CAUSAL_WINDOW) at a long length, whole
call (kernel plus merge pass): HIP events on one stream after warm-up, best of 5 rounds of 20
calls, the sides alternating round by round in one process (tools/dec_paged_ab.py's method).  Per
shape (B, H, H_kv, R, D, page, len, W), FP16 or INT8 pools, an identity-free shuffled table:
  (w)  the windowed call over sequences of `len` keys (cap = len);
  (s)  the causal call over sequences of W + R keys (cap = W + R): the same number of keys read;
  (c)  the causal call over the `len` keys.
One line per shape: microseconds, w / s, c / w, and the GB/s of (w) on the bytes of W + R + 1 keys.
A library without the window (the parent of the change that added it) prints (s) and (c) alone:
run both libraries alternately (MFA_LIB selects one) and compare (w) of one with (s) of the other.
    python tools/paged_window_ab.py [f16|i8|all]"""
import os
import sys

import torch

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_REPO, "metal-flash-attention-plus_amd", "python"))
import mfa_amd as mfa  # noqa: E402

P = mfa.Precision
dev = torch.device("cuda:0")
st = torch.cuda.Stream()
g = torch.Generator(device=dev).manual_seed(5)

SHAPES = [(8, 32, 8, 1, 128, 256, 32768, 4096), (8, 32, 8, 4, 128, 256, 32768, 1024),
          (32, 16, 16, 1, 128, 256, 8192, 1024)]


def timed(calls):
    """Best-of-5 microseconds per call of each callable, alternating round by round."""
    best = [1e9] * len(calls)
    with torch.cuda.stream(st):
        for c in calls:
            for _ in range(5):
                c()
        torch.cuda.synchronize()
        for _ in range(5):
            for i, c in enumerate(calls):
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(20):
                    c()
                e1.record(st)
                torch.cuda.synchronize()
                best[i] = min(best[i], e0.elapsed_time(e1) / 20 * 1e3)
    return best


def bench(B, H, Hkv, R, D, page, C, W, kv8):
    prec, es = P.FP16, 1 if kv8 else 2
    n = C // page
    q = (torch.rand((B, H, R, D), generator=g, device=dev) * 2 - 1).half()
    if kv8:
        kp, vp = (torch.randint(-127, 128, (B * n, Hkv, page, D), generator=g, device=dev,
                                dtype=torch.int8) for _ in range(2))
    else:
        kp, vp = ((torch.rand((B * n, Hkv, page, D), generator=g, device=dev) * 2 - 1).half()
                  for _ in range(2))
    table = torch.randperm(B * n, generator=torch.Generator().manual_seed(11)).view(B, n) \
        .to(torch.int32).to(dev).contiguous()
    o = torch.empty((B, H, R, D), dtype=torch.float32, device=dev)
    l = torch.empty((B, H, R), dtype=torch.float16, device=dev)
    short = W + R

    def call(lens, cap, **mask):
        base = mfa.AttentionDescriptor.make(low_precision=True, precision=prec, **mask)
        desc = mfa.PagedDecodeDescriptor.make(base, B, H, R, D, cap, Hkv=Hkv)
        cache = mfa.PagedKVCache.make(P.INT8 if kv8 else prec, page, n, B * n, Hkv, D, kp, vp, table,
                                      torch.full((B,), lens, dtype=torch.int32, device=dev),
                                      k_scale=0.01, v_scale=0.02)
        return lambda: mfa.paged_decode_forward(desc, q, cache, o, l, stream=st.cuda_stream)

    calls = [call(short, short, causal=True), call(C, C, causal=True)]
    window = True
    try:
        w = call(C, C, causal_window=W)
        with torch.cuda.stream(st):
            w()
        calls.append(w)
    except (mfa.MFAError, TypeError):
        window = False
    torch.cuda.synchronize()
    t = timed(calls)
    head = f"B{B} H{H}/{Hkv} R{R} D{D} p{page} len{C} W{W} {'I8' if kv8 else 'F16'}:"
    tail = f"causal len {short} {t[0]:7.1f} us | causal len {C} {t[1]:7.1f} us"
    if window:
        byts = 2.0 * B * Hkv * (W + R + 1) * D * es + B * H * R * (D * 2 + D * 4 + 2)
        mfa.last_launches()
        with torch.cuda.stream(st):
            calls[2]()
        torch.cuda.synchronize()
        names = [r["name"] for r in mfa.last_launches()]
        print(f"{head} window {t[2]:7.1f} us {byts / t[2] / 1e3:5.0f} GB/s | {tail} | window/short "
              f"x{t[2] / t[0]:5.3f}  long/window x{t[1] / t[2]:5.2f} {names}", flush=True)
    else:
        print(f"{head} window unsupported | {tail}", flush=True)


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    print(f"# {os.environ.get('TAG', 'lib')} set={which}", flush=True)
    for kv8 in (False, True):
        if which in ("all", "i8" if kv8 else "f16"):
            for shape in SHAPES:
                bench(*shape, kv8=kv8)
