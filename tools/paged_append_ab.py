#!/usr/bin/env python3
"""A/B of the paged KV-cache append (mfa_paged_kv_append) against what a caller can do without
it, whole call: HIP events on one stream after warm-up, best of 5 rounds of 20 calls, the sides
alternating round by round in one process.  Per shape and pool type:
  (a)  mfa_paged_kv_append (one launch for K and V);
  (b)  a PyTorch index_put_ scatter of K and of V into the same pools with page / slot indices
       precomputed on the device (not timed); for INT8 pools preceded by the torch expression of
       the quantisation (FP32 divide, round half away from zero, zero point, clamp, to int8);
  (c)  the roof: one torch.Tensor.copy_ that moves the bytes (a) reads plus writes.
Both sides are checked once to leave the same pool bytes.  One line per shape: microseconds,
the torch/append time ratio and, for the prefill chunk, GB/s (the R = 1 shapes are launch-bound).
Run it twice for the repeat spread.  MFA_LIB selects the library.
    python tools/paged_append_ab.py [f16|i8|all]"""
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
PAGE = 256

# (B, H_kv, R, D, length after the append): two decode steps and a prefill chunk.
SHAPES = [(32, 8, 1, 128, 1024), (256, 8, 1, 128, 1024), (8, 8, 2048, 128, 2048)]


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


def bench(B, Hkv, R, D, length, kv8):
    prec = P.FP16
    max_pages = -(-length // PAGE)
    num_pages = B * max_pages
    k, v = ((torch.rand((B, Hkv, R, D), generator=g, device=dev) * 2 - 1).half() for _ in range(2))
    ks, vs, kz, vz = 0.01, 0.02, 3, -5
    pdt = torch.int8 if kv8 else torch.float16
    pools = [torch.zeros((num_pages, Hkv, PAGE, D), dtype=pdt, device=dev) for _ in range(4)]
    table = torch.randperm(num_pages, generator=torch.Generator().manual_seed(11)).to(dev) \
        .view(B, max_pages).to(torch.int32).contiguous()
    lens = torch.full((B,), length, dtype=torch.int32, device=dev)
    cache = mfa.PagedKVCache.make(P.INT8 if kv8 else prec, PAGE, max_pages, num_pages, Hkv, D,
                                  pools[0], pools[1], table, lens, k_scale=ks, v_scale=vs,
                                  k_zero_point=kz, v_zero_point=vz)
    desc = mfa.PagedAppendDescriptor.make(prec, B, Hkv, R, D, length)
    append = lambda: mfa.paged_kv_append(desc, k, v, cache, stream=st.cuda_stream)

    # The torch side: page and slot of every (sequence, row), computed on the device, once.
    t = (lens.long() - R).view(B, 1) + torch.arange(R, device=dev).view(1, R)
    page_idx = torch.gather(table.long(), 1, t // PAGE).reshape(-1)
    slot_idx = (t % PAGE).reshape(-1)

    def quant(x, s, z):
        y = x.float() / s
        r = torch.sign(y) * torch.floor(torch.abs(y) + 0.5)
        return torch.clamp(r + z, -128, 127).to(torch.int8)

    def scatter_index_put():   # (indexed assignment is index_put_)
        for pool, x, s, z in ((pools[2], k, ks, kz), (pools[3], v, vs, vz)):
            rows = x.permute(0, 2, 1, 3).reshape(B * R, Hkv, D)
            pool[page_idx, :, slot_idx] = quant(rows, s, z) if kv8 else rows

    moved = 2 * B * Hkv * R * D * (2 + (1 if kv8 else 2))      # bytes read + written by (a)
    a_src = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
    a_dst = torch.empty_like(a_src)
    roof = lambda: a_dst.copy_(a_src)

    with torch.cuda.stream(st):
        append()
        scatter_index_put()
        torch.cuda.synchronize()
        same = torch.equal(pools[0], pools[2]) and torch.equal(pools[1], pools[3])
        filled = int(torch.count_nonzero(pools[0]).item()) > 0
    mfa.last_launches()
    append()
    torch.cuda.synchronize()
    kern = mfa.last_launches()[0]["name"]
    a, b, c = timed([append, scatter_index_put, roof])
    gb = lambda us: moved / us / 1e3
    tail = f" | append {gb(a):5.0f} GB/s, scatter {gb(b):5.0f}, copy_ {gb(c):5.0f}" if R > 1 else ""
    print(f"B{B} Hkv{Hkv} R{R} D{D} F16->{'I8' if kv8 else 'F16'}: append {a:7.1f} us | torch "
          f"scatter {b:7.1f} us x{b / a:5.2f} | copy_ of {moved / 1e6:6.2f} MB {c:7.1f} us "
          f"x{c / a:5.2f}{tail} | same bytes {same and filled} [{kern}]", flush=True)


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    print(f"# {os.environ.get('TAG', 'lib')} set={which}", flush=True)
    for kv8 in (False, True):
        if which in ("i8" if kv8 else "f16", "all"):
            for shape in SHAPES:
                bench(*shape, kv8=kv8)
