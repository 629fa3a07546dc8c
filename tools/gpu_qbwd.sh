#!/bin/bash
# GPU check of the on-load quantised backwardQuery (and forward): parity tests, then the bench.
set -o pipefail
OUT=${OUT:?set OUT to the directory the logs and bench lines go to}
mkdir -p "$OUT"
timeout -k 10 500 python -u -m pytest -x -v --timeout 120 --timeout-method thread \
  tests/test_quant_gpu.py tests/test_plan_gpu.py > $OUT/qbwd_tests.log 2>&1 || { tail -60 $OUT/qbwd_tests.log; exit 1; }
tail -3 $OUT/qbwd_tests.log
timeout -k 10 400 python -u bench.py --full > $OUT/qbwd_bench.json 2> $OUT/qbwd_bench.err || { tail -20 $OUT/qbwd_bench.err; exit 1; }
python - "$OUT" <<'PY'
import json, sys
out = sys.argv[1]
r = json.loads(open(f"{out}/qbwd_bench.json").read().strip().splitlines()[-1])
print(json.dumps(r["int8_fwd_bwd_d256"], indent=1))
print("C2", r["value"], "C5", r["fwd_bwd_d256"]["tflops"])
PY
