#!/bin/bash
# C5 subset (48 x 50 kb = 2304 pairs of the 32-bit tile): built default against the variant lib $1, interleaved
set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
cd $GRAFT_REPO_ROOT
V=$PWD/seqrush_amd/libseqrush_amd_$1.so
show() { python - "$1" "$2" <<'PY'
import json,sys
d=json.loads(open(sys.argv[2]).read().strip().split("\n")[-1])
r=d["roofline"]
print(sys.argv[1], "| ms/step", round(d["ms_per_step"],2), "align", round(r["kernel_ms"],2), "build", d["config"]["workspace"].get("kernel_build"), flush=True)
PY
}
run() { name=$1; shift; env "$@" timeout -k 10 400 python bench.py --full --config C5 --nseq 48 --steps 3 --warmup 1 --no-cpu-baseline --no-host-stages > $OUT/v.json 2> $OUT/v.err && show "C5/48 $name" $OUT/v.json || { echo "$name FAILED"; tail -3 $OUT/v.err; }; }
for rep in 1 2 3; do run default SR_X=$rep; run $1 SEQRUSH_AMD_LIB=$V; done
