#!/usr/bin/env python3
"""A/B of the paged prefill over INT8 pools (mfa_quantized_paged_prefill_forward) against the
16-bit paged prefill on pools of the same shape, whole call: HIP events on one stream after
warm-up, best of 5 rounds of 10 calls, the sides alternating round by round in one process
(tools/paged_prefill_ab.py's method).  Per shape and page size (256 and 32 keys, shuffled block
table), all causal:
  (A)  mfa_quantized_paged_prefill_forward on INT8 pools (widened on load);
  (B)  mfa_paged_prefill_forward on FP16 pools holding the same keys.
Prefill is MFMA-bound: halving the K/V bytes cannot make A faster than B; A / B is the price of
the widening.  One `row` line per shape and page size: microseconds, A's TFLOP/s on the visible
(query, key) pairs, max |O_A - O_B| (the two pools hold the same values up to the quantisation)
and the NaN counts.  Run it twice for the repeat spread, then
    python tools/paged_prefill_kv8_ab.py --summary RUN1 RUN2
prints the table: mean times, the spread |t1 - t2| / mean of each side, A / B, and whether A / B
exceeds 1 by more than twice the larger spread.  MFA_LIB selects the library.
    python tools/paged_prefill_kv8_ab.py [--quick]"""
import os
import sys

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (B, H, H_kv, R, prefix, D): the first three shapes of DESIGN.md's paged-prefill table.
SHAPES = [(8, 32, 8, 2048, 0, 128), (8, 32, 8, 512, 8192, 128), (32, 32, 8, 128, 4096, 128)]
QUICK = [(2, 4, 2, 256, 0, 128), (2, 4, 2, 128, 384, 128)]


def summary(paths):
    runs = []
    for p in paths:
        rows = {}
        for line in open(p):
            if line.startswith("row "):
                kv = dict(f.split("=", 1) for f in line.split()[1:])
                rows[(kv["shape"], kv["page"])] = kv
        runs.append(rows)
    print("shape page | A us (spread) | B us (spread) | A/B | A TFLOP/s | A/B - 1 > 2 x spread")
    for key in runs[0]:
        if any(key not in r for r in runs):
            continue
        spreads, mean = {}, {}
        for side in "AB":
            ts = [float(r[key][side + "_us"]) for r in runs]
            mean[side] = sum(ts) / len(ts)
            spreads[side] = (max(ts) - min(ts)) / mean[side]
        tf = sum(float(r[key]["A_tflops"]) for r in runs) / len(runs)
        sp = max(spreads["A"], spreads["B"])
        behind = mean["A"] / mean["B"] - 1 > 2 * sp
        print(f"{key[0]} p{key[1]} | {mean['A']:9.1f} ({spreads['A'] * 100:4.1f} %) | "
              f"{mean['B']:9.1f} ({spreads['B'] * 100:4.1f} %) | {mean['A'] / mean['B']:5.3f} | "
              f"{tf:6.1f} | {'yes' if behind else 'no'}")


if len(sys.argv) > 1 and sys.argv[1] == "--summary":
    summary(sys.argv[2:])
    sys.exit(0)

import torch  # noqa: E402

sys.path.insert(0, os.path.join(_REPO, "metal-flash-attention-plus_amd", "python"))
import mfa_amd as mfa  # noqa: E402

P = mfa.Precision
dev = torch.device("cuda:0")
st = torch.cuda.Stream()
g = torch.Generator(device=dev).manual_seed(5)
ZP = 3


def scatter(dense, page, seed):
    """[B, Hkv, C, D] -> pool [B·C/page, Hkv, page, D] through a shuffled table [B, C/page]."""
    B, Hkv, C, D = dense.shape
    n = C // page
    pages = dense.view(B, Hkv, n, page, D).permute(0, 2, 1, 3, 4).reshape(B * n, Hkv, page, D).contiguous()
    perm = torch.randperm(B * n, generator=torch.Generator().manual_seed(seed)).to(dev)
    pool = torch.empty_like(pages)
    pool[perm] = pages
    return pool, perm.view(B, n).to(torch.int32).contiguous()


def timed(calls, n):
    """Best-of-5 microseconds per call of each callable, alternating round by round."""
    best = [1e12] * len(calls)
    with torch.cuda.stream(st):
        for c in calls:
            for _ in range(3):
                c()
        torch.cuda.synchronize()
        for _ in range(5):
            for i, c in enumerate(calls):
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(n):
                    c()
                e1.record(st)
                torch.cuda.synchronize()
                best[i] = min(best[i], e0.elapsed_time(e1) / n * 1e3)
    return best


def bench(B, H, Hkv, R, prefix, D, n):
    prec = P.FP16
    C = prefix + R                      # keys per sequence after the chunk
    Ca = -(-C // 256) * 256             # allocated: whole pages
    q = (torch.rand((B, H, R, D), generator=g, device=dev) * 2 - 1).half()
    k, v = ((torch.rand((B, Hkv, Ca, D), generator=g, device=dev) * 2 - 1).half() for _ in range(2))
    # The INT8 side's bytes: scale = amax / 120, zero point 3.
    scales = [float(x.abs().max()) / 120.0 for x in (k, v)]
    k8, v8 = ((torch.round(x.float() / s) + ZP).clamp(-128, 127).to(torch.int8)
              for x, s in zip((k, v), scales))
    oa, ob = (torch.empty((B, H, R, D), dtype=torch.float32, device=dev) for _ in range(2))
    l = torch.empty((B, H, R), dtype=torch.float16, device=dev)
    base = mfa.AttentionDescriptor.make(low_precision=True, precision=prec, causal=True)
    pdesc = mfa.PagedPrefillDescriptor.make(base, B, H, R, D, C, Hkv=Hkv)
    lens = torch.full((B,), C, dtype=torch.int32, device=dev)
    pairs = B * (R * prefix + R * (R + 1) // 2)
    flops = 4.0 * D * pairs * H
    tag = f"B{B}_H{H}/{Hkv}_R{R}_pre{prefix}_D{D}"
    for page in (256, 32):
        kp, table = scatter(k, page, 11)
        vp, _ = scatter(v, page, 11)
        kp8, _ = scatter(k8, page, 11)
        vp8, _ = scatter(v8, page, 11)
        c16 = mfa.PagedKVCache.make(prec, page, Ca // page, B * (Ca // page), Hkv, D, kp, vp, table,
                                    lens)
        c8 = mfa.PagedKVCache.make(P.INT8, page, Ca // page, B * (Ca // page), Hkv, D, kp8, vp8,
                                   table, lens, k_scale=scales[0], v_scale=scales[1],
                                   k_zero_point=ZP, v_zero_point=ZP)
        A = lambda: mfa.quantized_paged_prefill_forward(pdesc, q, c8, oa, logsumexp=l,
                                                        stream=st.cuda_stream)
        Bc = lambda: mfa.paged_prefill_forward(pdesc, q, c16, ob, logsumexp=l,
                                               stream=st.cuda_stream)
        torch.cuda.synchronize()   # the operands were made on the default stream
        with torch.cuda.stream(st):
            mfa.last_launches()
            A()
            torch.cuda.synchronize()
            kern = mfa.last_launches()[0]["name"]
            Bc()
            torch.cuda.synchronize()
            diff = float((oa - ob).abs().max())
            nans = f"{int(torch.isnan(oa).sum())}/{int(torch.isnan(ob).sum())}"
        t = timed([A, Bc], n)
        print(f"row shape={tag} page={page} A_us={t[0]:.1f} B_us={t[1]:.1f} "
              f"A_over_B={t[0] / t[1]:.3f} A_tflops={flops / t[0] / 1e6:.1f} maxdiff_AB={diff:.2e} "
              f"nan_A/B={nans} kern={kern.replace(' ', '')}", flush=True)
        del kp, vp, kp8, vp8, table


if __name__ == "__main__":
    quick = "--quick" in sys.argv
    print(f"# paged_prefill_kv8_ab {os.environ.get('TAG', 'lib')} {'quick' if quick else 'full'}",
          flush=True)
    for shape in (QUICK if quick else SHAPES):
        bench(*shape, n=4 if quick else 10)
