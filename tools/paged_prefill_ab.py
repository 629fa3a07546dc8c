#!/usr/bin/env python3
"""A/B of the paged prefill call (mfa_paged_prefill_forward) against what a caller had before it,
whole call: HIP events on one stream after warm-up, best of 5 rounds of N calls, the sides
alternating round by round in one process.  Per shape and page size (256 and 32 keys, shuffled
block table), all causal:
  (A)  the paged prefill call;
  (B)  mfa_paged_decode_forward with the same arguments at uniform R — the only gather-free
       alternative, kernel plus merge pass.  It cannot take a ragged chunk: on the ragged shape it
       runs the chunk padded to R rows per sequence (lengths R), the work a caller would give it;
  (C)  prefix-0 shapes only, where the two diagonals coincide: mfa_multihead_forward causal on a
       dense copy of the same K/V (the tuned kernel: the roof).  Ragged shape: padded to R, as (B).
One `row` line per shape and page size: microseconds, A's TFLOP/s on the visible (query, key)
pairs, max |O_A - O_B| over the rows both compute and the NaN counts of the two outputs.  Run it twice for the repeat spread, then
    python tools/paged_prefill_ab.py --summary RUN1 RUN2
prints the table: mean times, the spread |t1 - t2| / mean of each side, B/A and A/C, and whether
A beats B by more than twice the larger spread.  MFA_LIB selects the library.
    python tools/paged_prefill_ab.py [--quick | --short]
--short runs the crossover set instead: chunks of 16 to 512 rows over prefixes of 8192 and 32768
keys, where (B) splits the keys over workgroups and (A) does not."""
import os
import sys

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (B, H, H_kv, R, prefix, D, ragged)
SHAPES = [(8, 32, 8, 2048, 0, 128, False), (8, 32, 8, 512, 8192, 128, False),
          (32, 32, 8, 128, 4096, 128, False), (4, 32, 4, 1024, 0, 256, False),
          (8, 32, 8, 2048, 0, 128, True)]
# Short chunks over long prefixes, where the decode call's split-KV takes over (--short).
SHORT = [(8, 32, 8, 64, 8192, 128, False), (8, 32, 8, 16, 8192, 128, False),
         (1, 32, 8, 128, 32768, 128, False), (1, 32, 8, 32, 32768, 128, False),
         (1, 32, 8, 512, 32768, 128, False)]
QUICK = [(2, 4, 2, 256, 0, 128, False), (2, 4, 2, 128, 384, 128, True)]


def summary(paths):
    runs = []
    for p in paths:
        rows = {}
        for line in open(p):
            if line.startswith("row "):
                kv = dict(f.split("=", 1) for f in line.split()[1:])
                rows[(kv["shape"], kv["page"])] = kv
        runs.append(rows)
    print("shape page | A us (spread) | B us (spread) B/A | C us (spread) A/C | A TFLOP/s | A beats B by > 2 x spread")
    for key in runs[0]:
        if any(key not in r for r in runs):
            continue
        spreads, mean = {}, {}
        for side in "ABC":
            ts = [float(r[key][side + "_us"]) for r in runs]
            if any(t != t for t in ts):
                mean[side] = float("nan")
                continue
            mean[side] = sum(ts) / len(ts)
            spreads[side] = (max(ts) - min(ts)) / mean[side]
        tf = sum(float(r[key]["A_tflops"]) for r in runs) / len(runs)
        sp = max(spreads["A"], spreads["B"])
        win = (mean["B"] - mean["A"]) / mean["A"] > 2 * sp
        c = (f"{mean['C']:9.1f} ({spreads['C'] * 100:4.1f} %) {mean['A'] / mean['C']:5.2f}"
             if mean["C"] == mean["C"] else "        -           -")
        print(f"{key[0]} p{key[1]} | {mean['A']:9.1f} ({spreads['A'] * 100:4.1f} %) | "
              f"{mean['B']:9.1f} ({spreads['B'] * 100:4.1f} %) {mean['B'] / mean['A']:5.2f} | {c} | "
              f"{tf:6.1f} | {'yes' if win else 'NO'}")


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


def bench(B, H, Hkv, R, prefix, D, ragged, n):
    prec = P.FP16
    C = prefix + R                      # keys per sequence after the chunk
    Ca = -(-C // 256) * 256             # allocated: whole pages
    q = (torch.rand((B, H, R, D), generator=g, device=dev) * 2 - 1).half()
    k, v = ((torch.rand((B, Hkv, Ca, D), generator=g, device=dev) * 2 - 1).half() for _ in range(2))
    oa, ob, oc = (torch.empty((B, H, R, D), dtype=torch.float32, device=dev) for _ in range(3))
    l = torch.empty((B, H, R), dtype=torch.float16, device=dev)
    base = mfa.AttentionDescriptor.make(low_precision=True, precision=prec, causal=True)
    pdesc = mfa.PagedPrefillDescriptor.make(base, B, H, R, D, C, Hkv=Hkv)
    ddesc = mfa.PagedDecodeDescriptor.make(base, B, H, R, D, C, Hkv=Hkv)
    mdesc = mfa.MultiHeadDescriptor.make(base, B, H, R, D, Hkv=Hkv, C=C)
    mha = mfa.MultiHeadAttention()
    full = torch.full((B,), C, dtype=torch.int32, device=dev)
    if ragged:
        new = torch.randint(R // 8, R + 1, (B,), generator=torch.Generator().manual_seed(7),
                            dtype=torch.int32)
    else:
        new = torch.full((B,), R, dtype=torch.int32)
    lens_a = (new + prefix).to(dev)
    new_d = new.to(dev)
    # Visible (query, key) pairs of A: row q of n rows behind a prefix sees prefix + q + 1 keys.
    pairs = sum(int(x) * prefix + int(x) * (int(x) + 1) // 2 for x in new.tolist())
    flops = 4.0 * D * pairs * H
    tag = f"B{B}_H{H}/{Hkv}_R{R}_pre{prefix}_D{D}" + ("_ragged" if ragged else "")
    for page in (256, 32):
        kp, table = scatter(k, page, 11)
        vp, _ = scatter(v, page, 11)
        mk = lambda lens: mfa.PagedKVCache.make(prec, page, Ca // page, B * (Ca // page), Hkv, D,
                                                kp, vp, table, lens)
        ca, cb = mk(lens_a), mk(full)
        A = lambda: mfa.paged_prefill_forward(pdesc, q, ca, oa, new_lens=new_d if ragged else None,
                                              logsumexp=l, stream=st.cuda_stream)
        Bc = lambda: mfa.paged_decode_forward(ddesc, q, cb, ob, l, stream=st.cuda_stream)
        calls = [A, Bc]
        if prefix == 0:
            calls.append(lambda: mha.forward(mdesc, q, k, v, oc, l, stream=st.cuda_stream))
        # The sides compute the same rows (ragged: the sequences with all R rows).
        torch.cuda.synchronize()   # the operands were made on the default stream
        with torch.cuda.stream(st):
            mfa.last_launches()
            A()
            torch.cuda.synchronize()
            kern = mfa.last_launches()[0]["name"]
            Bc()
            torch.cuda.synchronize()
            same = (new == R).to(dev)
            diff = float((oa - ob)[same].abs().max()) if bool(same.any()) else float("nan")
            nans = f"{int(torch.isnan(oa).sum())}/{int(torch.isnan(ob[same]).sum())}"
        t = timed(calls, n) + [float("nan")]
        print(f"row shape={tag} page={page} A_us={t[0]:.1f} B_us={t[1]:.1f} C_us={t[2]:.1f} "
              f"A_tflops={flops / t[0] / 1e6:.1f} maxdiff_AB={diff:.2e} nan_A/B={nans} kern={kern.replace(' ', '')}",
              flush=True)
        del kp, vp, table


if __name__ == "__main__":
    quick, short = "--quick" in sys.argv, "--short" in sys.argv
    print(f"# paged_prefill_ab {os.environ.get('TAG', 'lib')} "
          f"{'quick' if quick else 'short' if short else 'full'}", flush=True)
    for shape in (QUICK if quick else SHORT if short else SHAPES):
        # Enough calls per round for a window of tens of milliseconds.
        bench(*shape, n=4 if quick else 10)
