#!/usr/bin/env python3
"""A/B of the paged MLA decode call (mfa_paged_mla_decode_forward) against what a caller had
before it, whole call: HIP events on one stream after warm-up, best of 5 rounds of 10 calls, the
sides alternating round by round in one process.  Per shape and page size (256 and 32 keys,
shuffled block table), BF16, latent 512, D 128, H 16:
  (A)  the paged call, every sequence at the full length;
  (B)  mfa_mla_forward_absorbed on a dense copy of the same latent rows at the same uniform
       length — without the gather a caller of (B) also pays.  Unmasked; on the causal shape (A)
       alone is causal (the dense call's diagonal is the top-left one, another problem).
One `row` line per shape and page size: microseconds, max |O_A - O_B| (unmasked shapes: the two
run the same tile body over the same splits, so 0 is expected) and the NaN counts.  Run it twice
for the repeat spread, then
    python tools/paged_mla_ab.py --summary RUN1 RUN2
prints the table: mean times, the spread |t1 - t2| / mean of each side, A/B, and whether A is
within twice the larger spread of B.  MFA_LIB selects the library.
    python tools/paged_mla_ab.py [--quick]"""
import os
import sys

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (B, H, R, keys, D, latent, causal for A)
SHAPES = [(32, 16, 1, 4096, 128, 512, False), (8, 16, 1, 32768, 128, 512, False),
          (32, 16, 4, 4096, 128, 512, True)]
QUICK = [(2, 16, 1, 1024, 128, 512, False), (2, 16, 4, 512, 128, 512, True)]


def summary(paths):
    runs = []
    for p in paths:
        rows = {}
        for line in open(p):
            if line.startswith("row "):
                kv = dict(f.split("=", 1) for f in line.split()[1:])
                rows[(kv["shape"], kv["page"])] = kv
        runs.append(rows)
    print("shape page | A us (spread) | B us (spread) | A/B | A within 2 x spread of B")
    for key in runs[0]:
        if any(key not in r for r in runs):
            continue
        spreads, mean = {}, {}
        for side in "AB":
            ts = [float(r[key][side + "_us"]) for r in runs]
            mean[side] = sum(ts) / len(ts)
            spreads[side] = (max(ts) - min(ts)) / mean[side]
        sp = max(spreads["A"], spreads["B"])
        within = (mean["A"] - mean["B"]) / mean["B"] <= 2 * sp
        print(f"{key[0]} p{key[1]} | {mean['A']:9.1f} ({spreads['A'] * 100:4.1f} %) | "
              f"{mean['B']:9.1f} ({spreads['B'] * 100:4.1f} %) | {mean['A'] / mean['B']:5.3f} | "
              f"{'yes' if within else 'NO'}")


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
    """[B, C, latent] -> pool [B·C/page, page, latent] through a shuffled table [B, C/page]."""
    B, C, lat = dense.shape
    n = C // page
    pages = dense.view(B * n, page, lat)
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


def bench(B, H, R, C, D, lat, causal, n):
    prec = P.BF16
    rnd = lambda *s: torch.randn(s, generator=g, device=dev)
    q = rnd(B, H, R, D).bfloat16()
    wk, wv = ((rnd(lat, H * D) * lat ** -0.5).bfloat16() for _ in range(2))
    dense = rnd(B, C, lat).bfloat16()
    oa, ob = (torch.empty((B, H, R, D), dtype=torch.float32, device=dev) for _ in range(2))
    la, lb = (torch.empty((B, H, R), dtype=torch.float16, device=dev) for _ in range(2))
    base_a = mfa.AttentionDescriptor.make(low_precision=True, precision=prec, causal=causal)
    base_b = mfa.AttentionDescriptor.make(low_precision=True, precision=prec)
    desc = mfa.PagedMLADecodeDescriptor.make(base_a, B, H, R, D, lat, C, prec)
    lens = torch.full((B,), C, dtype=torch.int32, device=dev)
    tag = f"B{B}_H{H}_R{R}_C{C}_D{D}_lat{lat}" + ("_causalA" if causal else "")
    for page in (256, 32):
        pool, table = scatter(dense, page, 11)
        pc = mfa.PagedLatentCache.make(prec, page, C // page, B * (C // page), lat, pool, table, lens)
        A = lambda: mfa.paged_mla_decode_forward(desc, q, wk, wv, pc, oa, logsumexp=la,
                                                 stream=st.cuda_stream)
        Bc = lambda: mfa.mla_forward_absorbed(base_b, dense, wk, wv, q, ob, B, H, R, C, D, lat, prec,
                                              logsumexp=lb, stream=st.cuda_stream)
        torch.cuda.synchronize()   # the operands were made on the default stream
        with torch.cuda.stream(st):
            mfa.last_launches()
            A()
            torch.cuda.synchronize()
            kern = "+".join(r["name"] for r in mfa.last_launches())
            Bc()
            torch.cuda.synchronize()
            diff = float("nan") if causal else float((oa - ob).abs().max())
            nans = f"{int(torch.isnan(oa).sum())}/{int(torch.isnan(ob).sum())}"
        t = timed([A, Bc], n)
        print(f"row shape={tag} page={page} A_us={t[0]:.1f} B_us={t[1]:.1f} maxdiff_AB={diff:.2e} "
              f"nan_A/B={nans} kern={kern.replace(' ', '')}", flush=True)
        del pool, table


if __name__ == "__main__":
    quick = "--quick" in sys.argv
    print(f"# paged_mla_ab {os.environ.get('TAG', 'lib')} {'quick' if quick else 'full'}", flush=True)
    for shape in (QUICK if quick else SHAPES):
        bench(*shape, n=4 if quick else 10)
