#!/usr/bin/env python3
"""A/B of the paged MLA prefill call (mfa_paged_mla_prefill_forward) against the two calls a
caller had before it, whole call: HIP events on one stream after warm-up, best of 5 rounds of 10
calls, the sides alternating round by round in one process (tools/paged_mla_ab.py's method).
Per shape and page size (256 and 32 keys, shuffled block table), BF16, latent 512, D 128, H 16,
causal, every sequence `prefix + R` keys long:
  (A)  the prefill call;
  (B)  mfa_paged_mla_decode_forward with the same arguments (uniform shapes only: it takes
       exactly R rows of every sequence);
  (C)  at prefix 0 and uniform rows only, mfa_mla_forward_absorbed, causal, on a dense copy of the
       same latent rows — without the gather a caller of (C) also pays.
The ragged shape draws n_b from [R / 8, R] and has side A alone.
One `row` line per shape and page size: microseconds, max |O_A - O_B|, whether O_A equals O_C bit
for bit (expected where C does not split the keys) and the NaN count of O_A.  Run it twice for
the repeat spread, then
    python tools/paged_mla_prefill_ab.py --summary RUN1 RUN2
prints the table: mean times, the spread |t1 - t2| / mean of each side, A/B and A/C, and the two
expectations — A faster than B by more than twice the spread, A within twice the spread of C.
MFA_LIB selects the library.
    python tools/paged_mla_prefill_ab.py [--quick]"""
import os
import sys

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (B, H, R, prefix, D, latent, ragged)
SHAPES = [(8, 16, 2048, 0, 128, 512, False), (8, 16, 512, 8192, 128, 512, False),
          (32, 16, 128, 4096, 128, 512, False), (8, 16, 2048, 0, 128, 512, True),
          # Short chunks over long prefixes: where the decode call's key split stays ahead.
          (8, 16, 16, 8192 - 16, 128, 512, False), (8, 16, 64, 8192 - 64, 128, 512, False),
          (1, 16, 128, 32768 - 128, 128, 512, False)]
QUICK = [(2, 16, 256, 0, 128, 512, False), (2, 16, 64, 512, 128, 512, False),
         (2, 16, 256, 0, 128, 512, True)]


def summary(paths):
    runs = []
    for p in paths:
        rows = {}
        for line in open(p):
            if line.startswith("row "):
                kv = dict(f.split("=", 1) for f in line.split()[1:])
                rows[(kv["shape"], kv["page"])] = kv
        runs.append(rows)
    print("shape page | A us (spread) | B us (spread) | C us (spread) | A/B | A/C | "
          "A faster than B by > 2 x spread | A within 2 x spread of C")
    for key in runs[0]:
        if any(key not in r for r in runs):
            continue
        spreads, mean = {}, {}
        for side in "ABC":
            ts = [float(r[key][side + "_us"]) for r in runs]
            if any(t != t for t in ts):
                continue
            mean[side] = sum(ts) / len(ts)
            spreads[side] = (max(ts) - min(ts)) / mean[side]
        cell = lambda s: (f"{mean[s]:9.1f} ({spreads[s] * 100:4.1f} %)" if s in mean
                          else "        - (   - %)")
        ab = ac = faster = within = "-"
        if "B" in mean:
            sp = max(spreads["A"], spreads["B"])
            ab = f"{mean['A'] / mean['B']:5.3f}"
            faster = "yes" if (mean["B"] - mean["A"]) / mean["B"] > 2 * sp else "NO"
        if "C" in mean:
            sp = max(spreads["A"], spreads["C"])
            ac = f"{mean['A'] / mean['C']:5.3f}"
            within = "yes" if (mean["A"] - mean["C"]) / mean["C"] <= 2 * sp else "NO"
        print(f"{key[0]} p{key[1]} | {cell('A')} | {cell('B')} | {cell('C')} | {ab} | {ac} | "
              f"{faster} | {within}")


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


def bench(B, H, R, prefix, D, lat, ragged, n):
    prec = P.BF16
    C = prefix + R
    CA = -(-C // 256) * 256              # allocated keys per sequence: whole 256-key pages
    rnd = lambda *s: torch.randn(s, generator=g, device=dev)
    q = rnd(B, H, R, D).bfloat16()
    wk, wv = ((rnd(lat, H * D) * lat ** -0.5).bfloat16() for _ in range(2))
    paged = rnd(B, CA, lat).bfloat16()
    dense = paged[:, :C].contiguous()    # side C's operand: the C keys of every sequence
    oa, ob, oc = (torch.empty((B, H, R, D), dtype=torch.float32, device=dev) for _ in range(3))
    la, lb, lc = (torch.empty((B, H, R), dtype=torch.float16, device=dev) for _ in range(3))
    base = mfa.AttentionDescriptor.make(low_precision=True, precision=prec, causal=True)
    desc = mfa.PagedMLADecodeDescriptor.make(base, B, H, R, D, lat, C, prec)
    new = None
    lens = torch.full((B,), C, dtype=torch.int32, device=dev)
    if ragged:
        new = torch.randint(R // 8, R + 1, (B,), generator=torch.Generator().manual_seed(3))
        new = new.to(torch.int32).to(dev)
        lens = (new + prefix).contiguous()
    tag = f"B{B}_H{H}_R{R}_prefix{prefix}_D{D}_lat{lat}" + ("_ragged" if ragged else "")
    for page in (256, 32):
        pool, table = scatter(paged, page, 11)
        pc = mfa.PagedLatentCache.make(prec, page, CA // page, B * (CA // page), lat, pool, table,
                                       lens)
        A = lambda: mfa.paged_mla_prefill_forward(desc, q, wk, wv, pc, oa, new_lens=new,
                                                  logsumexp=la, stream=st.cuda_stream)
        Bc = lambda: mfa.paged_mla_decode_forward(desc, q, wk, wv, pc, ob, logsumexp=lb,
                                                  stream=st.cuda_stream)
        Cc = lambda: mfa.mla_forward_absorbed(base, dense, wk, wv, q, oc, B, H, R, C, D, lat, prec,
                                              logsumexp=lc, stream=st.cuda_stream)
        sides = [A] + ([] if ragged else [Bc]) + ([Cc] if prefix == 0 and not ragged else [])
        torch.cuda.synchronize()   # the operands were made on the default stream
        diff, same = float("nan"), "-"
        with torch.cuda.stream(st):
            mfa.last_launches()
            A()
            torch.cuda.synchronize()
            kern = "+".join(r["name"] for r in mfa.last_launches())
            if Bc in sides:
                Bc()
                torch.cuda.synchronize()
                diff = float((oa - ob).abs().max())
            if Cc in sides:
                Cc()
                torch.cuda.synchronize()
                same = str(bool(torch.equal(oa, oc) and torch.equal(la, lc)))
            nans = int(torch.isnan(oa).sum())
        t = dict(zip("ABC", [float("nan")] * 3))
        for side, us in zip([s for s, c in zip("ABC", (A, Bc, Cc)) if c in sides], timed(sides, n)):
            t[side] = us
        print(f"row shape={tag} page={page} A_us={t['A']:.1f} B_us={t['B']:.1f} C_us={t['C']:.1f} "
              f"maxdiff_AB={diff:.2e} A_equals_C={same} nan_A={nans} kern={kern.replace(' ', '')}",
              flush=True)
        del pool, table


if __name__ == "__main__":
    quick = "--quick" in sys.argv
    print(f"# paged_mla_prefill_ab {os.environ.get('TAG', 'lib')} {'quick' if quick else 'full'}",
          flush=True)
    for shape in (QUICK if quick else SHAPES):
        bench(*shape, n=4 if quick else 10)
