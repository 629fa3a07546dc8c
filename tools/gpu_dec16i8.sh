#!/bin/bash
# 16-row decode for INT8 too: decode tests, then default vs MFA_DECODE16=4 (INT8 on the 32-row
# kernel), interleaved, same library.
set -o pipefail
OUT=${OUT:?set OUT to the directory the logs and bench lines go to}
mkdir -p "$OUT"
export MFA_DEV=1
timeout -k 10 300 python -u -m pytest -x -q --timeout 120 --timeout-method thread \
  tests/test_quant_gpu.py -k "decode" > $OUT/dec16i8_tests.log 2>&1 || { tail -40 $OUT/dec16i8_tests.log; exit 1; }
tail -1 $OUT/dec16i8_tests.log
for i in 1 2 3; do
  for v in d16 d32; do
    unset MFA_DECODE16
    [ $v = d32 ] && export MFA_DECODE16=4
    timeout -k 10 200 python -u bench.py --full --no-c5 --no-mla > $OUT/x_$v$i.json 2> $OUT/x_$v$i.err || { tail -20 $OUT/x_$v$i.err; exit 1; }
  done
done
python - "$OUT" <<'PY'
import json, sys
out = sys.argv[1]
for v in ("d16", "d32"):
    row = []
    for i in (1, 2, 3):
        r = json.loads(open(f"{out}/x_{v}{i}.json").read().strip().splitlines()[-1])["int8_decode"]
        row.append("q1 %.4f q1i4 %.4f q16 %.4f" % (r["s_q1"]["ms"], r["s_q1_int4"]["ms"], r["s_q16"]["ms"]))
    print(v, " | ".join(row))
PY
