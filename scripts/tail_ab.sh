#!/bin/bash
# A/B of the tail launch on one GPU: scripts/tail_ab.sh PARENT_TREE [part...]
# PARENT_TREE is a built checkout of the parent commit (its own library, Python package and bench.py: the host side of the
# library changed, so the parent cannot be a variant library of this tree); runs of the two sides are interleaved.
# parts (default: all): timeline c2 others full variants trace.  Lines in the format of profiles/mirror_ab.log go to
# $OUT/tail_ab.log, the timelines to $OUT/tail_timeline_{before,after}.log.  Every GPU step has its own time limit and the
# script ends at the first step that fails.
set -o pipefail
PARENT=$(cd "$1" && pwd) || { echo "usage: scripts/tail_ab.sh PARENT_TREE [part...]"; exit 2; }
shift
PARTS=${*:-timeline c2 others full variants trace}
cd "$(dirname "$0")/.."
ROOT=$PWD
OUT=${OUT:-$ROOT/bench_out}
mkdir -p "$OUT"
LOG=$OUT/tail_ab.log
show() { python - "$1" "$2" <<'PY' | tee -a "$LOG"
import json, sys
d = json.loads(open(sys.argv[2]).read().strip().split("\n")[-1])
w = d["config"]["workspace"]
r = d.get("roofline") or {}
c = d.get("kernels") or {}
keys = ("mirror_pairs", "mirror_ties", "row_bytes_loaded", "row_bytes_stored", "bp_passes", "base_tiles", "wf_cells", "breakpoint_searches",
        "united_bases")
print(sys.argv[1], "| ms/step", round(d["ms_per_step"], 3), "| align kernel ms", r.get("kernel_ms"), "| build", w.get("kernel_build"),
      w.get("source_digest"), "| partners", w.get("mirror_partners"), "| tail_threads", w.get("tail_threads"), "|", w.get("knobs"),
      "|", {k: c[k] for k in keys if k in c}, flush=True)
PY
}
# run LABEL TREE SECONDS [VAR=value ...] -- bench arguments
run() {
    local label=$1 tree=$2 secs=$3; shift 3
    local envs=()
    while [ "$1" != "--" ]; do envs+=("$1"); shift; done
    shift
    (cd "$tree" && env "${envs[@]}" timeout -k 10 "$secs" python bench.py "$@") > "$OUT/v.json" 2> "$OUT/v.err" \
        || { echo "$label FAILED rc=$?" | tee -a "$LOG"; tail -5 "$OUT/v.err"; exit 1; }
    show "$label" "$OUT/v.json"
}
FULL="--full --no-cpu-baseline --no-h2h --no-host-stages"
for part in $PARTS; do
    case $part in
    timeline)
        SR_TAIL=0 timeout -k 10 120 python scripts/tail_timeline.py > "$OUT/tail_timeline_before.log" || { echo "timeline before FAILED"; exit 1; }
        timeout -k 10 120 python scripts/tail_timeline.py > "$OUT/tail_timeline_after.log" || { echo "timeline after FAILED"; exit 1; }
        head -4 "$OUT/tail_timeline_before.log" "$OUT/tail_timeline_after.log" ;;
    c2)
        run "C2 default-args warm" "$PARENT" 200 X=0 -- --gpus 1
        for rep in 1 2 3 4; do
            run "C2 default-args parent" "$PARENT" 200 X=0 -- --gpus 1
            run "C2 default-args candidate" "$ROOT" 200 X=0 -- --gpus 1
        done
        run "C2 default-args candidate SR_TAIL=0" "$ROOT" 200 SR_TAIL=0 -- --gpus 1 ;;
    others)
        for rep in 1 2; do
            run "C4 default-args parent" "$PARENT" 300 X=0 -- --gpus 1 --config C4
            run "C4 default-args candidate" "$ROOT" 300 X=0 -- --gpus 1 --config C4
        done
        for rep in 1 2; do
            run "C3 default-args parent" "$PARENT" 200 X=0 -- --gpus 1 --config C3
            run "C3 default-args candidate" "$ROOT" 200 X=0 -- --gpus 1 --config C3
        done
        for rep in 1 2; do
            run "C5 nseq 32 parent" "$PARENT" 300 X=0 -- --gpus 1 --config C5 --nseq 32 --steps 2 --warmup 1
            run "C5 nseq 32 candidate" "$ROOT" 300 X=0 -- --gpus 1 --config C5 --nseq 32 --steps 2 --warmup 1
        done ;;
    full)
        run "C2 full parent" "$PARENT" 300 X=0 -- $FULL --config C2
        run "C2 full candidate" "$ROOT" 300 X=0 -- $FULL --config C2 ;;
    variants)
        run "C2 default-args candidate" "$ROOT" 200 SR_TAIL_ROUNDS=2 -- --gpus 1
        run "C2 default-args candidate" "$ROOT" 200 SR_TAIL_ROUNDS=32 -- --gpus 1
        run "C2 default-args candidate" "$ROOT" 200 SR_TAIL_THREADS=512 -- --gpus 1
        run "C2 default-args candidate" "$ROOT" 200 SR_TAIL=all -- --gpus 1 ;;
    trace)
        # kernel trace with statistics, one run per side, nothing else collected in the same run
        for side in parent candidate; do
            tree=$ROOT; [ $side = parent ] && tree=$PARENT
            rm -rf "$OUT/trace_$side"
            (cd /tmp && timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace_$side" -- \
                python "$tree/bench.py" --gpus 1 > "$OUT/trace_$side.json" 2> "$OUT/trace_$side.log") || { echo "trace $side FAILED"; tail -5 "$OUT/trace_$side.log"; exit 1; }
            cp "$(find "$OUT/trace_$side" -name '*kernel_stats.csv' | head -1)" "$OUT/tail_${side}_kernel_stats.csv"
            echo "# kernel trace $side:" | tee -a "$LOG"
            grep sr_align_blk_kernel "$OUT/tail_${side}_kernel_stats.csv" | tee -a "$LOG"
        done ;;
    esac
done
