#!/bin/bash
# repeated interleaved A/B of two variant libs ($1 = reference, $2 = candidate) on C2 (4x), C4 (2x), C3 (2x); parity of the candidate first
set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
cd $GRAFT_REPO_ROOT
A=$PWD/seqrush_amd/libseqrush_amd_$1.so; B=$PWD/seqrush_amd/libseqrush_amd_$2.so
show() { python - "$1" "$2" <<'PY'
import json,sys
d=json.loads(open(sys.argv[2]).read().strip().split("\n")[-1])
r=d["roofline"]
print(sys.argv[1], "| ms/step", round(d["ms_per_step"],2), "align", round(r["kernel_ms"],2), "build", d["config"]["workspace"].get("kernel_build"), flush=True)
PY
}
run() { cfg=$1; name=$2; shift; shift; env "$@" timeout -k 10 200 python bench.py --full --config $cfg --steps 10 --warmup 3 --no-cpu-baseline --no-host-stages > $OUT/v.json 2> $OUT/v.err && show "$cfg $name" $OUT/v.json || { echo "$cfg $name FAILED"; tail -3 $OUT/v.err; }; }
SEQRUSH_AMD_LIB=$B timeout -k 10 300 python scripts/gpu_parity_quick.py > $OUT/quick.log 2>&1; echo "quick $2 rc=$?"; tail -1 $OUT/quick.log
grep -q "ALL OK" $OUT/quick.log || { grep -n "MISMATCH\|Error\|error" $OUT/quick.log | head; exit 1; }
run C2 "warm" SEQRUSH_AMD_LIB=$A
for rep in 1 2 3 4; do run C2 "$1" SEQRUSH_AMD_LIB=$A; run C2 "$2" SEQRUSH_AMD_LIB=$B; done
for rep in 1 2; do run C4 "$1" SEQRUSH_AMD_LIB=$A; run C4 "$2" SEQRUSH_AMD_LIB=$B; done
for rep in 1 2; do run C3 "$1" SEQRUSH_AMD_LIB=$A; run C3 "$2" SEQRUSH_AMD_LIB=$B; done
