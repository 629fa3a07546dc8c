#!/usr/bin/env python3
"""A/B of the paged MLA prefill with a RoPE key part (mfa_paged_mla_rope_prefill_forward) against
the no-rope prefill on the same latent cache, by tools/paged_mla_prefill_ab.py's method (whole
call, HIP events, best of 5 rounds of 10 calls, the sides alternating in one process; BF16, latent
512, D 128, H 16, causal, every sequence prefix + R keys, 256- and 32-key pages, shuffled table):
  (A)  the rope call, rope rows fused behind the latent rows (token stride 576) or in a pool of
       their own (the latent pool then dense, token stride 512);
  (B)  mfa_paged_mla_prefill_forward over the same latent cache struct.
A reads 576 / 512 of B's cache bytes and issues 33 / 32 of its MFMA work in the attention kernel.
One `row` line per shape, layout and page size; run it twice, then
    python tools/paged_mla_rope_prefill_ab.py --summary RUN1 RUN2
prints mean times, the spread |t1 - t2| / mean of each side, A / B and the bound
A / B <= 1.125 + twice the larger spread.  MFA_LIB selects the library.
    python tools/paged_mla_rope_prefill_ab.py [--quick]"""
import os
import sys


def summary(paths):
    runs = [{(kv["shape"], kv["page"]): kv for kv in
             (dict(f.split("=", 1) for f in line.split()[1:]) for line in open(p) if line.startswith("row "))}
            for p in paths]
    print("shape page | A us (spread) | B us (spread) | A/B | bound | inside")
    worst = 0.0
    for key in runs[0]:
        if any(key not in r for r in runs):
            continue
        mean, spread = {}, {}
        for side in "AB":
            ts = [float(r[key][side + "_us"]) for r in runs]
            mean[side] = sum(ts) / len(ts)
            spread[side] = (max(ts) - min(ts)) / mean[side]
        ab, bound = mean["A"] / mean["B"], 1.125 + 2 * max(spread.values())
        worst = max(worst, ab)
        print(f"{key[0]} p{key[1]} | {mean['A']:9.1f} ({spread['A'] * 100:4.1f} %) | "
              f"{mean['B']:9.1f} ({spread['B'] * 100:4.1f} %) | {ab:5.3f} | {bound:5.3f} | "
              f"{'yes' if ab <= bound else 'NO'}")
    print(f"largest A/B {worst:5.3f}")


if len(sys.argv) > 1 and sys.argv[1] == "--summary":
    summary(sys.argv[2:])
    sys.exit(0)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from paged_mla_prefill_ab import QUICK, SHAPES, P, dev, g, mfa, scatter, st, timed, torch  # noqa: E402

ROPE = 64


def bench(B, H, R, prefix, D, lat, ragged, n):
    prec, C = P.BF16, prefix + R
    CA = -(-C // 256) * 256              # allocated keys per sequence: whole 256-key pages
    rnd = lambda *s: torch.randn(s, generator=g, device=dev)
    q, qr = rnd(B, H, R, D).bfloat16(), rnd(B, H, R, ROPE).bfloat16()
    wk, wv = ((rnd(lat, H * D) * lat ** -0.5).bfloat16() for _ in range(2))
    rows = rnd(B, CA, lat + ROPE).bfloat16()                     # [latent | rope] per key
    oa, ob = (torch.empty((B, H, R, D), dtype=torch.float32, device=dev) for _ in range(2))
    la, lb = (torch.empty((B, H, R), dtype=torch.float16, device=dev) for _ in range(2))
    base = mfa.AttentionDescriptor.make(low_precision=True, precision=prec, causal=True)
    desc = mfa.PagedMLADecodeDescriptor.make(base, B, H, R, D, lat, C, prec)
    lens = torch.full((B,), C, dtype=torch.int32, device=dev)
    for page in (256, 32):
        pool, table = scatter(rows, page, 11)
        n_pages = B * (CA // page)
        for layout in ("fused", "separate"):
            tag = f"B{B}_H{H}_R{R}_prefix{prefix}_D{D}_lat{lat}_{layout}"
            if layout == "fused":
                lp, rp, strides = pool, pool[..., lat:], (page * (lat + ROPE), lat + ROPE)
                rc = mfa.PagedRopeCache.make(page, rp, strides=strides)
            else:
                lp, rp, strides = pool[..., :lat].contiguous(), pool[..., lat:].contiguous(), None
                rc = mfa.PagedRopeCache.make(page, rp)
            pc = mfa.PagedLatentCache.make(prec, page, CA // page, n_pages, lat, lp, table, lens,
                                           strides=strides)
            A = lambda: mfa.paged_mla_rope_prefill_forward(desc, q, qr, wk, wv, pc, rc, oa,
                                                           logsumexp=la, stream=st.cuda_stream)
            Bc = lambda: mfa.paged_mla_prefill_forward(desc, q, wk, wv, pc, ob, logsumexp=lb,
                                                       stream=st.cuda_stream)
            torch.cuda.synchronize()   # the operands were made on the default stream
            with torch.cuda.stream(st):
                mfa.last_launches()
                A()
                torch.cuda.synchronize()
                kern = "+".join(r["name"] for r in mfa.last_launches())
                Bc()
                torch.cuda.synchronize()
                nans = f"{int(torch.isnan(oa).sum())}/{int(torch.isnan(ob).sum())}"
            t = timed([A, Bc], n)
            print(f"row shape={tag} page={page} A_us={t[0]:.1f} B_us={t[1]:.1f} nan_A/B={nans} "
                  f"kern={kern.replace(' ', '')}", flush=True)
            del lp, rp
        del pool, table


if __name__ == "__main__":
    quick = "--quick" in sys.argv
    print(f"# paged_mla_rope_prefill_ab {os.environ.get('TAG', 'lib')} {'quick' if quick else 'full'}",
          flush=True)
    for shape in (QUICK[:2] if quick else SHAPES[:3]):   # the prefill table's first six rows
        bench(*shape, n=4 if quick else 10)
