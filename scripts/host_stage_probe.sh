#!/bin/bash
# host stages around the device path for C2 and C4
set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
cd $GRAFT_REPO_ROOT
for cfg in C2 C4; do
  timeout -k 10 300 python bench.py --full --config $cfg --steps 2 --warmup 1 --no-cpu-baseline > $OUT/v.json 2> $OUT/v.err || { tail -3 $OUT/v.err; exit 1; }
  python - $cfg "$OUT/v.json" <<'PY'
import json,sys
d=json.loads(open(sys.argv[2]).read().strip().split("\n")[-1])
print(sys.argv[1], {k:(round(v,2) if isinstance(v,float) else v) for k,v in d["host_stages_ms"].items()}, flush=True)
PY
done
