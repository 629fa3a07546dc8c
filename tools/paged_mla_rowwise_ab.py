#!/usr/bin/env python3
"""A/B of the paged MLA decode over a row-wise INT8 latent cache
(mfa_paged_mla_decode_forward_rowwise) against the 16-bit call on the same rows, whole call, by
paged_mla_ab.py's method (HIP events on one stream after warm-up, best of 5 rounds of 10 calls,
the sides alternating round by round in one process).  Per shape and page size (256 and 32 keys,
shuffled block table), BF16, latent 512, D 128, H 16, unmasked, every sequence at the full length:
  (A)  the row-wise call on INT8 bytes and per-token FP32 scales (amax / 127 of rows whose
       magnitudes spread over four octaves);
  (B)  mfa_paged_mla_decode_forward on the pool of scale * q rounded to BF16.
One `row` line per shape and page size: microseconds, max |O_A - O_B| (0 is expected: the two
run the same tile body on the same LDS image) and the NaN counts.  Run it twice for the repeat
spread, then
    python tools/paged_mla_rowwise_ab.py --summary RUN1 RUN2
prints paged_mla_ab.py's table.  MFA_LIB selects the library (a build with
-DMFA_MLA_RW8_DIST=2 measures the other prefetch distance).
    python tools/paged_mla_rowwise_ab.py [--quick]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from paged_mla_ab import P, dev, g, mfa, scatter, st, timed, torch  # noqa: E402  (--summary ends here)

# (B, H, R, keys, D, latent)
SHAPES = [(32, 16, 1, 4096, 128, 512), (8, 16, 1, 32768, 128, 512)]
QUICK = [(2, 16, 1, 1024, 128, 512), (2, 16, 1, 1024, 128, 256)]


def bench(B, H, R, C, D, lat, n):
    prec = P.BF16
    rnd = lambda *s: torch.randn(s, generator=g, device=dev)
    q = rnd(B, H, R, D).bfloat16()
    wk, wv = ((rnd(lat, H * D) * lat ** -0.5).bfloat16() for _ in range(2))
    x = rnd(B, C, lat) * torch.exp2(4 * torch.rand((B, C, 1), generator=g, device=dev) - 2)
    scale = x.abs().amax(-1, keepdim=True) / 127.0
    q8 = torch.clamp(torch.round(x / scale), -127, 127).to(torch.int8)
    dense = (scale * q8.float()).bfloat16()
    oa, ob = (torch.empty((B, H, R, D), dtype=torch.float32, device=dev) for _ in range(2))
    la, lb = (torch.empty((B, H, R), dtype=torch.float16, device=dev) for _ in range(2))
    base = mfa.AttentionDescriptor.make(low_precision=True, precision=prec)
    desc = mfa.PagedMLADecodeDescriptor.make(base, B, H, R, D, lat, C, prec)
    lens = torch.full((B,), C, dtype=torch.int32, device=dev)
    tag = f"B{B}_H{H}_R{R}_C{C}_D{D}_lat{lat}"
    for page in (256, 32):
        n_pages = B * (C // page)
        pool16, table = scatter(dense, page, 11)
        pool8, _ = scatter(q8, page, 11)
        spool, _ = scatter(scale, page, 11)
        pc16 = mfa.PagedLatentCache.make(prec, page, C // page, n_pages, lat, pool16, table, lens)
        pc8 = mfa.PagedLatentCache.make(P.INT8, page, C // page, n_pages, lat, pool8, table, lens)
        sc = mfa.PagedLatentScales.make(page, spool)
        A = lambda: mfa.paged_mla_decode_forward_rowwise(desc, q, wk, wv, pc8, sc, oa, logsumexp=la,
                                                         stream=st.cuda_stream)
        Bc = lambda: mfa.paged_mla_decode_forward(desc, q, wk, wv, pc16, ob, logsumexp=lb,
                                                  stream=st.cuda_stream)
        torch.cuda.synchronize()   # the operands were made on the default stream
        with torch.cuda.stream(st):
            mfa.last_launches()
            A()
            torch.cuda.synchronize()
            kern = "+".join(r["name"] for r in mfa.last_launches())
            Bc()
            torch.cuda.synchronize()
            diff = float((oa - ob).abs().max())
            nans = f"{int(torch.isnan(oa).sum())}/{int(torch.isnan(ob).sum())}"
        t = timed([A, Bc], n)
        print(f"row shape={tag} page={page} A_us={t[0]:.1f} B_us={t[1]:.1f} maxdiff_AB={diff:.2e} "
              f"nan_A/B={nans} kern={kern.replace(' ', '')}", flush=True)
        del pool16, pool8, spool, table


if __name__ == "__main__":
    quick = "--quick" in sys.argv
    print(f"# paged_mla_rowwise_ab {os.environ.get('TAG', 'lib')} {'quick' if quick else 'full'}",
          flush=True)
    for shape in (QUICK if quick else SHAPES):
        bench(*shape, n=4 if quick else 10)
