#!/usr/bin/env python3
"""iterative_bench.py -- `-x tree:3,3,0.1` against `--iterative` with the same spec on one GPU: one JSON line per config.

    python scripts/iterative_bench.py [--configs C4,C2] [--reps 3] [--no-profile] [--out DIR]

Per config:
  plain_ms / iterative_ms     host clock around align + unite (sr_ctx_run / sr_ctx_run_iterative) ending in a device
                              synchronise; the pair list and workspace are loaded before the clock starts; median of --reps
                              after one warm-up run
  tree_entries, random_entries, random_processed, random_aligned, random_skipped, checks, windows, post_tree, final_components
  same_partition_as_plain     whether the iterative run ended with the plain run's partition (true when nothing was skipped)
  phase2_*_ms                 from a child run of the iterative mode alone under `rocprofv3 --kernel-trace --stats`: kernels
                              that start after phase 1's component count; `chain` = the guarded unite + root count + decide
                              kernels, `align` = orientation + dequeue-order + alignment kernels; chain_over_align = their ratio
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SPEC = "tree:3,3,0.1"
CHAIN = ("sr_iter_unite_kernel", "sr_count_roots_kernel", "sr_iter_decide_kernel")


def records(cfg):
    from seqrush_amd import synth
    return {"C2": synth.config_c2, "C4": synth.config_c4}[cfg]()


def timed(fn, reps):
    fn()                                           # warm-up: code objects, first use of the workspace
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def measure(cfg, reps):
    import numpy as np
    from seqrush_amd.seqrush import Context, Params, SeqSet
    ss = SeqSet(records(cfg))
    plain = Context(0)
    plain.load(ss, Params(sparsification=SPEC))

    def run_plain():
        plain.reset_uf(); plain.run(); plain.sync()
    plain_ms = timed(run_plain, reps)
    plain_labels = plain.download_labels()
    plain_pairs = plain.num_pairs
    plain.close()
    it = Context(0)
    it.load_iterative(ss, Params(sparsification=SPEC))

    def run_iter():
        it.run_iterative(); it.sync()
    iter_ms = timed(run_iter, reps)
    st = it.iterative_stats()
    labels = it.download_labels()
    it.close()
    out = dict(config=cfg, spec=SPEC, plain_pairs=plain_pairs, plain_ms=round(plain_ms, 2), iterative_ms=round(iter_ms, 2),
               speedup=round(plain_ms / max(iter_ms, 1e-9), 3))
    for k in ("tree_entries", "random_entries", "random_processed", "random_aligned", "checks", "windows", "post_tree",
              "final_components", "stabilized"):
        out[k] = st[k]
    out["random_skipped"] = st["random_entries"] - st["random_processed"]
    out["same_partition_as_plain"] = bool(np.array_equal(labels, plain_labels))
    return out


def child(cfg):
    """the iterative run alone, once, for the profiler"""
    import torch  # noqa: F401  (same HIP runtime order as the suite)
    from seqrush_amd.seqrush import Context, Params, SeqSet
    ctx = Context(0)
    ctx.load_iterative(SeqSet(records(cfg)), Params(sparsification=SPEC))
    ctx.run_iterative(); ctx.sync()
    print(json.dumps(ctx.iterative_stats()["windows"]))
    ctx.close()


def profile(cfg, outdir):
    d = os.path.join(outdir, f"rocprof_{cfg}")
    os.makedirs(d, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "iter", "--",
           sys.executable, os.path.abspath(__file__), "--child", cfg]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        return dict(profile_error=f"rocprofv3 exit {r.returncode}: {r.stderr[-400:]}")
    files = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getmtime)
    if not files:
        return dict(profile_error="no kernel_trace.csv")
    rows = list(csv.DictReader(open(files[-1])))
    rows.sort(key=lambda x: int(x["Start_Timestamp"]))
    first = next((i for i, x in enumerate(rows) if "sr_count_roots_kernel" in x["Kernel_Name"]), None)
    if first is None:
        return dict(profile_error="no root count kernel in the trace")
    chain = align = 0
    n_chain = 0
    for x in rows[first + 1:]:
        dt = (int(x["End_Timestamp"]) - int(x["Start_Timestamp"])) * 1e-6
        name = x["Kernel_Name"]
        if any(k in name for k in CHAIN):
            chain += dt; n_chain += 1
        elif "sr_align" in name or "sr_orient" in name or "rocprim" in name or "sr_order" in name:
            align += dt
    return dict(phase2_chain_ms=round(chain, 3), phase2_chain_kernels=n_chain, phase2_align_ms=round(align, 3),
                chain_over_align=round(chain / align, 4) if align else None, trace=os.path.relpath(files[-1], ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C4,C2")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    import torch  # noqa: F401
    for cfg in a.configs.split(","):
        out = measure(cfg, a.reps)
        if not a.no_profile:
            out.update(profile(cfg, a.out))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
