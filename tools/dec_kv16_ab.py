#!/usr/bin/env python3
"""A/B of the 16-bit K/V decode route (MFA_DECODE_KV16=1) against the kernels the same call ran
before (MFA_DECODE_KV16=0), whole call (kernel plus merge pass): HIP events on one stream after
warm-up, best of 5 rounds of 20 calls, the two routes alternating round by round in one process.
One line per shape: microseconds of both, their ratio, and GB/s of the routed call with its
fraction of the 8 TB/s roof (bytes: K + V once per kv head, plus Q, O and L).  Run it twice for
the repeat spread.  MFA_LIB selects the library.
    MFA_DEV=1 python tools/dec_kv16_ab.py [main|keys|rows|units|d64|all]"""
import os
import sys

if os.environ.get("MFA_DEV") != "1":
    sys.exit("dec_kv16_ab.py: needs MFA_DEV=1 (the route switch is a development switch)")

import torch

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_REPO, "metal-flash-attention-plus_amd", "python"))
import mfa_amd as mfa  # noqa: E402

P = mfa.Precision
ROOF = 8e12
dev = torch.device("cuda:0")
st = torch.cuda.Stream()
g = torch.Generator(device=dev).manual_seed(5)

# (B, H, H_kv, R, C, D)
MAIN = [(32, 16, 16, 1, 8192, 128), (32, 16, 16, 16, 8192, 128), (8, 32, 8, 1, 16384, 128),
        (1, 32, 8, 4, 65536, 128), (8, 32, 4, 1, 16384, 256)]
# The bound on keys: S_kv 512 .. 4096 at one row and at 16 rows per kv head.
KEYS = [(32, 16, 16, R, C, 128) for R in (1, 16) for C in (512, 1024, 2048, 4096)] + \
       [(8, 32, 8, 1, C, 128) for C in (512, 1024, 2048, 4096)]
# The bound on rows per kv head: 8 .. 64 (above 16: the 32-row form).
ROWS = [(8, 32, 8, R, 8192, 128) for R in (2, 4, 6, 8, 12, 16)] + \
       [(8, 32, 4, R, 8192, 256) for R in (1, 2, 3, 4, 8)]
# Rows per kv head (above 16: the 32-row form) against the number of (batch, kv head) units:
# 512 units (B32 H16/16), 256 (B32 H32/8), 128 (B16 H32/8).
UNITS = [(32, 16, 16, R, C, 128) for C in (4096, 8192) for R in (24, 32, 48, 64)] + \
        [(B, 32, 8, R, 8192, 128) for B in (32, 16) for R in (1, 4, 6, 8, 12, 16)] + \
        [(32, 32, 4, R, 8192, 256) for R in (3, 4, 8)]
# D = 64 (the three-slot ring).
D64 = [(32, 16, 16, 1, 8192, 64), (32, 16, 16, 16, 8192, 64), (8, 32, 8, 1, 16384, 64),
       (1, 32, 8, 4, 65536, 64)]
SETS = {"main": MAIN, "keys": KEYS, "rows": ROWS, "units": UNITS, "d64": D64,
        "all": MAIN + KEYS + ROWS + UNITS + D64}


def bench(B, H, Hkv, R, C, D, dtype=torch.float16):
    prec = P.FP16 if dtype == torch.float16 else P.BF16
    q = (torch.rand((B, H, R, D), generator=g, device=dev) * 2 - 1).to(dtype)
    k = (torch.rand((B, Hkv, C, D), generator=g, device=dev) * 2 - 1).to(dtype)
    v = (torch.rand((B, Hkv, C, D), generator=g, device=dev) * 2 - 1).to(dtype)
    o = torch.empty((B, H, R, D), dtype=torch.float32, device=dev)
    l = torch.empty((B, H, R), dtype=torch.float16, device=dev)
    base = mfa.AttentionDescriptor.make(low_precision=True, precision=prec)
    desc = mfa.MultiHeadDescriptor.make(base, B, H, R, D, Hkv=Hkv, C=C)
    mha = mfa.MultiHeadAttention()
    best, names = {"1": 1e9, "0": 1e9}, {}
    with torch.cuda.stream(st):
        for sw in ("1", "0"):
            os.environ["MFA_DECODE_KV16"] = sw
            mfa.last_launches()
            for _ in range(5):
                mha.forward(desc, q, k, v, o, l, stream=st.cuda_stream)
            torch.cuda.synchronize()
            names[sw] = mfa.last_launches()[-1]["name"] if sw == "0" else \
                [r["name"] for r in mfa.last_launches()][-2:]
        for _ in range(5):
            for sw in ("1", "0"):
                os.environ["MFA_DECODE_KV16"] = sw
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(20):
                    mha.forward(desc, q, k, v, o, l, stream=st.cuda_stream)
                e1.record(st)
                torch.cuda.synchronize()
                best[sw] = min(best[sw], e0.elapsed_time(e1) / 20)
    byts = 2.0 * B * Hkv * C * D * 2 + B * H * R * (D * 2 + D * 4 + 2)
    on, off = best["1"] * 1e3, best["0"] * 1e3
    gbs = byts / best["1"] / 1e6
    kern = next((n for n in names["1"] if "fwd_decode" in n), names["1"][-1])
    print(f"B{B} H{H}/{Hkv} R{R} C{C} D{D} {'F16' if dtype == torch.float16 else 'BF16'}: "
          f"on {on:7.1f} us  off {off:7.1f} us  off/on {off / on:5.2f}  "
          f"{gbs:5.0f} GB/s {gbs * 1e9 / ROOF:4.2f} of roof  [{kern} | {names['0']}]", flush=True)


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    print(f"# {os.environ.get('TAG', 'lib')} set={which}", flush=True)
    for shape in SETS[which]:
        bench(*shape)
