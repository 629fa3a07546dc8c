#!/usr/bin/env python3
"""A/B of the paged decode call (mfa_paged_decode_forward) against the contiguous decode route
on the same values, whole call (kernel plus merge pass): HIP events on one stream after warm-up,
best of 5 rounds of 20 calls, the sides alternating round by round in one process.  Per shape:
  (a)  the contiguous route on a dense cache (16-bit: MFA_DECODE_KV16=1; INT8: the quantized entry);
  (b)  the paged call on the same values scattered over a shuffled block table, pages of 32 and
       of 256 keys, every length equal to C;
  (c)  the paged call (256-key pages) with ragged lengths, uniform in [C/8, C] (fixed seed),
       as GB/s on the bytes those lengths need.
One line per shape: microseconds, the paged/contiguous time ratios, GB/s.  Run it twice for the
repeat spread.  MFA_LIB selects the library.
    MFA_DEV=1 python tools/dec_paged_ab.py [f16|i8|all]"""
import os
import sys

if os.environ.get("MFA_DEV") != "1":
    sys.exit("dec_paged_ab.py: needs MFA_DEV=1 (the contiguous route switch is a development switch)")

import torch

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_REPO, "metal-flash-attention-plus_amd", "python"))
import mfa_amd as mfa  # noqa: E402

P = mfa.Precision
ROOF = 8e12
dev = torch.device("cuda:0")
st = torch.cuda.Stream()
g = torch.Generator(device=dev).manual_seed(5)

# (B, H, H_kv, R, C, D): the main set of dec_kv16_ab.py; the INT8 caches take four of them.
F16 = [(32, 16, 16, 1, 8192, 128), (32, 16, 16, 16, 8192, 128), (8, 32, 8, 1, 16384, 128),
       (1, 32, 8, 4, 65536, 128), (8, 32, 4, 1, 16384, 256)]
I8 = [F16[0], F16[2], F16[3], F16[4]]


def scatter(dense, page, seed):
    """[B, Hkv, C, D] -> pool [B·C/page, Hkv, page, D] through a shuffled table [B, C/page]."""
    B, Hkv, C, D = dense.shape
    n = C // page
    # (contiguous(): at B = 1 the reshape is a view, and empty_like would keep its strides)
    pages = dense.view(B, Hkv, n, page, D).permute(0, 2, 1, 3, 4).reshape(B * n, Hkv, page, D).contiguous()
    perm = torch.randperm(B * n, generator=torch.Generator().manual_seed(seed)).to(dev)
    pool = torch.empty_like(pages)
    pool[perm] = pages
    return pool, perm.view(B, n).to(torch.int32).contiguous()


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


def bench(B, H, Hkv, R, C, D, kv8):
    prec, es = P.FP16, 1 if kv8 else 2
    q = (torch.rand((B, H, R, D), generator=g, device=dev) * 2 - 1).half()
    if kv8:
        k, v = (torch.randint(-127, 128, (B, Hkv, C, D), generator=g, device=dev, dtype=torch.int8)
                for _ in range(2))
    else:
        k, v = ((torch.rand((B, Hkv, C, D), generator=g, device=dev) * 2 - 1).half() for _ in range(2))
    o = torch.empty((B, H, R, D), dtype=torch.float32, device=dev)
    l = torch.empty((B, H, R), dtype=torch.float16, device=dev)
    ks, vs = 0.01, 0.02
    if kv8:
        qbase = mfa.AttentionDescriptor.make(R, C, D, low_precision_intermediates=True)
        qdesc = mfa.quantized_descriptor(qbase, prec, P.INT8, P.INT8, B=B, H=H, Hkv=Hkv)
        tq = mfa.quantized_tensor(q, prec)
        tk, tv = mfa.quantized_tensor(k, P.INT8, scale=ks), mfa.quantized_tensor(v, P.INT8, scale=vs)
        qa = mfa.QuantizedAttention()
        dense = lambda: qa.forward(qdesc, tq, tk, tv, o, l, stream=st.cuda_stream)
    else:
        os.environ["MFA_DECODE_KV16"] = "1"
        base = mfa.AttentionDescriptor.make(low_precision=True, precision=prec)
        mdesc = mfa.MultiHeadDescriptor.make(base, B, H, R, D, Hkv=Hkv, C=C)
        mha = mfa.MultiHeadAttention()
        dense = lambda: mha.forward(mdesc, q, k, v, o, l, stream=st.cuda_stream)
    pbase = mfa.AttentionDescriptor.make(low_precision=True, precision=prec)
    pdesc = mfa.PagedDecodeDescriptor.make(pbase, B, H, R, D, C, Hkv=Hkv)
    full = torch.full((B,), C, dtype=torch.int32, device=dev)
    ragged = torch.randint(C // 8, C + 1, (B,), generator=torch.Generator().manual_seed(7),
                           dtype=torch.int32).to(dev)
    calls, keep = [dense], []
    for page, lens in ((32, full), (256, full), (256, ragged)):
        kp, table = scatter(k, page, 11)
        vp, _ = scatter(v, page, 11)
        cache = mfa.PagedKVCache.make(P.INT8 if kv8 else prec, page, C // page, B * (C // page),
                                      Hkv, D, kp, vp, table, lens, k_scale=ks, v_scale=vs)
        keep.append(cache)
        calls.append(lambda c=cache: mfa.paged_decode_forward(pdesc, q, c, o, l, stream=st.cuda_stream))
    # The sides compute the same values: max |O - O_contiguous| at full lengths, checked once
    # (0 when the split layouts agree: the arithmetic order is the same).
    with torch.cuda.stream(st):
        dense()
        torch.cuda.synchronize()
        o0 = o.clone()
        same = []
        for c in calls[1:3]:
            o.zero_()
            c()
            torch.cuda.synchronize()
            same.append(float((o - o0).abs().max()))
    mfa.last_launches()
    calls[1]()
    torch.cuda.synchronize()
    kern = mfa.last_launches()[0]["name"]
    a, b32, b256, rag = timed(calls)
    io = B * H * R * (D * 2 + D * 4 + 2)
    byts = 2.0 * B * Hkv * C * D * es + io
    rbytes = 2.0 * int(ragged.sum().item()) * Hkv * D * es + io
    gb = lambda n, us: n / us / 1e3
    print(f"B{B} H{H}/{Hkv} R{R} C{C} D{D} {'I8' if kv8 else 'F16'}: contiguous {a:7.1f} us "
          f"{gb(byts, a):5.0f} GB/s | paged p32 {b32:7.1f} us x{b32 / a:5.3f}  p256 {b256:7.1f} us "
          f"x{b256 / a:5.3f} {gb(byts, b256):5.0f} GB/s | ragged p256 {rag:7.1f} us "
          f"{gb(rbytes, rag):5.0f} GB/s {gb(rbytes, rag) * 1e9 / ROOF:4.2f} of roof "
          f"(mean len {ragged.float().mean().item() / C:4.2f} C) | max|dO| {same} [{kern}]", flush=True)


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    print(f"# {os.environ.get('TAG', 'lib')} set={which}", flush=True)
    if which in ("f16", "all"):
        for shape in F16:
            bench(*shape, kv8=False)
    if which in ("i8", "all"):
        for shape in I8:
            bench(*shape, kv8=True)
