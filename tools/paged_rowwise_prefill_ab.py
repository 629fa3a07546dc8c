"""Row-wise INT8 paged prefill against the per-tensor INT8 call over the same bytes (MI355X).

Causal FP16 prompts, B 4, H 32 / H_kv 8, n = len = 4096, page 256, D in {128, 64, 256}; a shuffled
block table.  The two calls alternate in one process; device events around CALLS calls, REPEATS
repeats after a warm-up: median [min..max].  Every row-wise scale equals the per-tensor one, so the
two outputs are also compared (the time does not depend on the scale values).

    python tools/paged_rowwise_prefill_ab.py > profiles/paged_rowwise_prefill.txt"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                                "metal-flash-attention-plus_amd", "python"))
import mfa_amd as mfa  # noqa: E402

P = mfa.Precision
DEV = "cuda:0"
B, H, HKV, N, PAGE, CALLS, REPEATS = 4, 32, 8, 4096, 256, 10, 9


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / CALLS


def main():
    assert torch.cuda.is_available(), "needs the MI355X"
    print("Row-wise INT8 paged prefill against the per-tensor INT8 call (MI355X, gfx950).")
    print(f"FP16 queries, causal; B {B}, H {H}, H_kv {HKV}, n = len = {N}, page {PAGE}; both calls "
          f"alternated in one process;\ndevice events around {CALLS} calls, {REPEATS} repeats after a "
          "warm-up: median [min..max].  Bytes: 2*D per (key, kv head), +8 row-wise.\n")
    for D in (128, 64, 256):
        g = torch.Generator(device=DEV).manual_seed(D)
        pages = B * N // PAGE
        kp, vp = (torch.randint(-127, 128, (pages, HKV, PAGE, D), dtype=torch.int8, device=DEV,
                                generator=g) for _ in range(2))
        table = torch.randperm(pages, device=DEV, generator=g).to(torch.int32).view(B, N // PAGE)
        lens = torch.full((B,), N, dtype=torch.int32, device=DEV)
        sk, sv = 0.01, 0.02
        c = mfa.PagedKVCache.make(P.INT8, PAGE, N // PAGE, pages, HKV, D, kp, vp, table, lens,
                                  k_scale=sk, v_scale=sv, k_zero_point=0, v_zero_point=0)
        s = mfa.PagedKVScales.make(PAGE, HKV,
                                   torch.full((pages, HKV, PAGE), sk, dtype=torch.float32, device=DEV),
                                   torch.full((pages, HKV, PAGE), sv, dtype=torch.float32, device=DEV))
        q = torch.randn((B, H, N, D), dtype=torch.float16, device=DEV, generator=g)
        base = mfa.AttentionDescriptor.make(low_precision=True, precision=P.FP16, causal=True)
        desc = mfa.PagedPrefillDescriptor.make(base, B, H, N, D, N, Hkv=HKV)
        out = [torch.empty((B, H, N, D), dtype=torch.float32, device=DEV) for _ in range(2)]
        l = torch.empty((B, H, N), dtype=torch.float16, device=DEV)
        pt = lambda: mfa.quantized_paged_prefill_forward(desc, q, c, out[0], logsumexp=l)
        rw = lambda: mfa.paged_prefill_forward_rowwise(desc, q, c, s, out[1], logsumexp=l)
        print("plan per-tensor:", [r["name"] for r in mfa.quantized_paged_prefill_plan(desc, c)])
        plan = mfa.paged_prefill_rowwise_plan(desc, c, s)
        print("plan row-wise:  ", [r["name"] for r in plan], "LDS", plan[0]["lds_bytes"],
              "->", 160 * 1024 // plan[0]["lds_bytes"], "workgroup(s) per CU by LDS")
        pt(), rw()
        torch.cuda.synchronize()
        diff = (out[0] - out[1]).abs().max().item()
        t = [[], []]
        for _ in range(REPEATS):
            t[0].append(timed(pt))
            t[1].append(timed(rw))
        m = [statistics.median(x) for x in t]
        tf = 4.0 * B * H * D * N * (N + 1) / 2 / 1e6   # useful causal FLOPs / 1e6 -> TFLOP/s by us
        print(f"prefill B{B} H{H}/{HKV} D{D} n {N} page {PAGE}: "
              f"per-tensor {m[0]:.1f} us [{min(t[0]):.1f}..{max(t[0]):.1f}] ({tf / m[0]:.0f} TFLOP/s)  "
              f"row-wise {m[1]:.1f} us [{min(t[1]):.1f}..{max(t[1]):.1f}] ({tf / m[1]:.0f} TFLOP/s)  "
              f"ratio {m[1] / m[0]:.4f}  byte floor {(2 * D + 8) / (2 * D):.4f}  "
              f"max |O_rw - O_pt| {diff:.2e}", flush=True)


if __name__ == "__main__":
    main()
