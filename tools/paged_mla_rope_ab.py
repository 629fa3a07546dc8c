#!/usr/bin/env python3
"""A/B of the paged MLA decode with a RoPE key part (mfa_paged_mla_rope_decode_forward) against
the no-rope call on the same latent cache, by tools/paged_mla_ab.py's method (whole call, HIP
events, best of 5 rounds of 10 calls, the sides alternating in one process; BF16, latent 512,
D 128, H 16, 256- and 32-key pages, shuffled table):
  (A)  the rope call, rope rows fused behind the latent rows (token stride 576) or in a pool of
       their own (the latent pool then dense, token stride 512);
  (B)  mfa_paged_mla_decode_forward over the same latent cache struct.
A reads 576 / 512 of B's bytes per key and issues 17 / 16 of its QK MFMA work.  One `row` line per
shape, layout and page size; run it twice, then
    python tools/paged_mla_rope_ab.py --summary RUN1 RUN2
prints paged_mla_ab.py's table (mean times, spreads, A/B).  MFA_LIB selects the library.
    python tools/paged_mla_rope_ab.py [--quick]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from paged_mla_ab import QUICK, SHAPES, P, dev, g, mfa, scatter, st, timed, torch  # noqa: E402  (--summary exits there)

ROPE = 64


def bench(B, H, R, C, D, lat, causal, n):
    prec = P.BF16
    rnd = lambda *s: torch.randn(s, generator=g, device=dev)
    q, qr = rnd(B, H, R, D).bfloat16(), rnd(B, H, R, ROPE).bfloat16()
    wk, wv = ((rnd(lat, H * D) * lat ** -0.5).bfloat16() for _ in range(2))
    rows = rnd(B, C, lat + ROPE).bfloat16()                      # [latent | rope] per key
    oa, ob = (torch.empty((B, H, R, D), dtype=torch.float32, device=dev) for _ in range(2))
    la, lb = (torch.empty((B, H, R), dtype=torch.float16, device=dev) for _ in range(2))
    base = mfa.AttentionDescriptor.make(low_precision=True, precision=prec, causal=causal)
    desc = mfa.PagedMLADecodeDescriptor.make(base, B, H, R, D, lat, C, prec)
    lens = torch.full((B,), C, dtype=torch.int32, device=dev)
    for page in (256, 32):
        pool, table = scatter(rows, page, 11)
        n_pages = B * (C // page)
        for layout in ("fused", "separate"):
            tag = f"B{B}_H{H}_R{R}_C{C}_D{D}_lat{lat}" + ("_causal" if causal else "") + "_" + layout
            if layout == "fused":
                lp, rp, strides = pool, pool[..., lat:], (page * (lat + ROPE), lat + ROPE)
                rc = mfa.PagedRopeCache.make(page, rp, strides=strides)
            else:
                lp, rp, strides = pool[..., :lat].contiguous(), pool[..., lat:].contiguous(), None
                rc = mfa.PagedRopeCache.make(page, rp)
            pc = mfa.PagedLatentCache.make(prec, page, C // page, n_pages, lat, lp, table, lens,
                                           strides=strides)
            A = lambda: mfa.paged_mla_rope_decode_forward(desc, q, qr, wk, wv, pc, rc, oa, logsumexp=la,
                                                          stream=st.cuda_stream)
            Bc = lambda: mfa.paged_mla_decode_forward(desc, q, wk, wv, pc, ob, logsumexp=lb,
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
    print(f"# paged_mla_rope_ab {os.environ.get('TAG', 'lib')} {'quick' if quick else 'full'}", flush=True)
    for shape in (QUICK if quick else SHAPES):
        bench(*shape, n=4 if quick else 10)
