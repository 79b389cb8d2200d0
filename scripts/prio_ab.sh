#!/bin/bash
# A/B of the rotating tile priority on one GPU: scripts/prio_ab.sh PARENT_TREE [part...]
# PARENT_TREE is a built checkout of the parent commit (its own library, Python package and bench.py: the kernel arguments
# and the counters changed, so the parent cannot be a variant library of this tree); runs of the two sides are interleaved.
# parts (default: timeline c2): timeline c2 full others dump trace variants.  Lines in the format of profiles/tail_ab.log go to
# $OUT/prio_ab.log, the timelines to $OUT/prio_timeline_{before,after}.log.  Every GPU step has its own time limit and the
# script ends at the first step that fails.
# REPS (default 4): repetitions per side of the c2 and variants parts.
# variants: VARIANTS="name ..." are libraries seqrush_amd/libseqrush_amd_NAME.so of THIS tree (scripts/build_variant.sh),
# interleaved with the default library.
set -o pipefail
PARENT=$(cd "$1" && pwd) || { echo "usage: scripts/prio_ab.sh PARENT_TREE [part...]"; exit 2; }
shift
PARTS=${*:-timeline c2}
cd "$(dirname "$0")/.."
ROOT=$PWD
OUT=${OUT:-$ROOT/bench_out}
mkdir -p "$OUT"
LOG=$OUT/prio_ab.log
show() { python - "$1" "$2" <<'PY' | tee -a "$LOG"
import json, sys
d = json.loads(open(sys.argv[2]).read().strip().split("\n")[-1])
w = d["config"]["workspace"]
r = d.get("roofline") or {}
print(sys.argv[1], "| ms/step", round(d["ms_per_step"], 3), "| align kernel ms", r.get("kernel_ms"), "| build", w.get("kernel_build"),
      w.get("source_digest"), "| tile_prio", w.get("tile_prio"), "shift", w.get("prio_epoch_shift"), "|", w.get("knobs"), flush=True)
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
for part in $PARTS; do
    case $part in
    timeline)
        SR_TILE_PRIO=0 timeout -k 10 120 python scripts/tail_timeline.py > "$OUT/prio_timeline_before.log" || { echo "timeline before FAILED"; exit 1; }
        timeout -k 10 120 python scripts/tail_timeline.py > "$OUT/prio_timeline_after.log" || { echo "timeline after FAILED"; exit 1; }
        head -4 "$OUT/prio_timeline_before.log" "$OUT/prio_timeline_after.log" ;;
    c2)
        run "C2 default-args warm" "$PARENT" 200 X=0 -- --gpus 1
        for rep in $(seq "${REPS:-4}"); do
            run "C2 default-args parent" "$PARENT" 200 X=0 -- --gpus 1
            run "C2 default-args candidate" "$ROOT" 200 X=0 -- --gpus 1
            run "C2 default-args candidate" "$ROOT" 200 SR_TILE_PRIO=0 -- --gpus 1
        done ;;
    full)
        # the alignment kernel's own time (hipEvents), two runs per side
        for rep in 1 2; do
            run "C2 full parent" "$PARENT" 300 X=0 -- --full --no-cpu-baseline --no-h2h --no-host-stages --config C2
            run "C2 full candidate" "$ROOT" 300 X=0 -- --full --no-cpu-baseline --no-h2h --no-host-stages --config C2
        done ;;
    variants)
        for rep in $(seq "${REPS:-4}"); do
            run "C2 default-args candidate" "$ROOT" 200 X=0 -- --gpus 1
            for v in $VARIANTS; do
                run "C2 default-args variant $v" "$ROOT" 200 "SEQRUSH_AMD_LIB=$ROOT/seqrush_amd/libseqrush_amd_$v.so" -- --gpus 1
            done
        done ;;
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
    dump)
        # what the timed path hands back, both sides: the files must be byte for byte equal
        rm -rf "$OUT/dump_parent" "$OUT/dump_candidate"
        run "C2 dump parent" "$PARENT" 200 X=0 -- --gpus 1 --dump-outputs "$OUT/dump_parent"
        run "C2 dump candidate" "$ROOT" 200 X=0 -- --gpus 1 --dump-outputs "$OUT/dump_candidate"
        n=0
        for f in "$OUT"/dump_parent/*; do
            cmp "$f" "$OUT/dump_candidate/$(basename "$f")" || { echo "dump DIFFERS: $(basename "$f")" | tee -a "$LOG"; exit 1; }
            n=$((n + 1))
        done
        echo "# --dump-outputs: $n files byte for byte equal" | tee -a "$LOG" ;;
    trace)
        # kernel trace with statistics, one run per side, nothing else collected in the same run
        for side in parent candidate; do
            tree=$ROOT; [ $side = parent ] && tree=$PARENT
            rm -rf "$OUT/trace_$side"
            (cd /tmp && timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace_$side" -- \
                python "$tree/bench.py" --gpus 1 > "$OUT/trace_$side.json" 2> "$OUT/trace_$side.log") || { echo "trace $side FAILED"; tail -5 "$OUT/trace_$side.log"; exit 1; }
            cp "$(find "$OUT/trace_$side" -name '*kernel_stats.csv' | head -1)" "$OUT/prio_${side}_kernel_stats.csv"
            echo "# kernel trace $side:" | tee -a "$LOG"
            grep sr_align_blk_kernel "$OUT/prio_${side}_kernel_stats.csv" | tee -a "$LOG"
        done ;;
    esac
done
