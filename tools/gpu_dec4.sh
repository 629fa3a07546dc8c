#!/bin/bash
# INT4 decode: parity tests, then the decode bench lines.
set -o pipefail
OUT=${OUT:?set OUT to the directory the logs and bench lines go to}
mkdir -p "$OUT"
timeout -k 10 300 python -u -m pytest -x -q --timeout 120 --timeout-method thread \
  tests/test_quant_gpu.py -k "decode" > $OUT/dec4_tests.log 2>&1 || { tail -40 $OUT/dec4_tests.log; exit 1; }
tail -2 $OUT/dec4_tests.log
timeout -k 10 400 python -u bench.py --full --no-c5 --no-mla > $OUT/dec4_bench.json 2> $OUT/dec4_bench.err || { tail -20 $OUT/dec4_bench.err; exit 1; }
python - "$OUT" <<'PY'
import json, sys
out = sys.argv[1]
r = json.loads(open(f"{out}/dec4_bench.json").read().strip().splitlines()[-1])
print(json.dumps(r.get("int8_decode"), indent=1))
PY
