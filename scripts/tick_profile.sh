#!/bin/bash
# tick profile incl. the control section's parts (variant lib $1)
set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
cd $GRAFT_REPO_ROOT
V=$PWD/seqrush_amd/libseqrush_amd_${1:-ctlprof}.so
show() { python - "$1" "$2" <<'PY'
import json,sys
d=json.loads(open(sys.argv[2]).read().strip().split("\n")[-1])
r=d["roofline"]; k=d["kernels"]
tp=k.get("ticks_pair") or 1
print(sys.argv[1], "ms/step", round(d["ms_per_step"],2), "align", round(r["kernel_ms"],2), d["config"]["workspace"].get("kernel_build"), {x: round(100.0*k[x]/tp,1) for x in k if x.startswith(("tk_","ticks_b","ticks_br")) and k[x]}, flush=True)
PY
}
run() { cfg=$1; name=$2; shift; shift; env "$@" timeout -k 10 200 python bench.py --full --config $cfg --steps 3 --warmup 1 --no-cpu-baseline --no-host-stages > $OUT/v.json 2> $OUT/v.err && show "$cfg $name" $OUT/v.json || { echo "$cfg $name FAILED"; tail -3 $OUT/v.err; }; }
run C2 "ticks" SR_PROFILE_TICKS=1 SEQRUSH_AMD_LIB=$V
run C2 "ticks 512 pairs/4 waves" SR_PROFILE_TICKS=1 SEQRUSH_AMD_LIB=$V SR_NWG=256
run C4 "ticks" SR_PROFILE_TICKS=1 SEQRUSH_AMD_LIB=$V
