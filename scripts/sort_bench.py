#!/usr/bin/env python3
"""sort_bench.py -- the Ygs layout (--sort) stage on one GPU: one JSON line per graph.

    python scripts/sort_bench.py [--configs C2[,C4]] [--reps 5] [--no-host]

Per graph (aligned, united and induced on the device, compacted -- the graph `--sort` receives):
  nodes, steps, terms_per_iter, iterations, subrounds_per_iter
  sgd_device_ms      hipEvents around the SGD launches, median of --reps after one warm-up
  sgd_host_twin_ms   the same schedule on one host thread (bit-identical positions; checked)
  sgd_sequential_ms  the yardstick: every term applied at once
  groom_ms, topo_ms, write_ms
  sort_stage_ms      host-clock wall time of the whole sort stage of one sr_ctx_build_gfa_sorted call (everything after
                     induction and compaction: parameters and tables, device buffers and copies, SGD, orderings, groom,
                     topological sort, path verification, GFA writing), median of --reps after one warm-up
  sort_parts_ms      SGD + groom + topo + write only (the part of the stage the slots above name)
  quality_*          mean | |pos_b - pos_a| - len(a) | over consecutive steps (src/bin/measure_layout_quality.rs:100-200) of
                     the unsorted graph, the device sort and the sequential yardstick's sort
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401  (first HIP runtime in the process, as in the test suite)

from seqrush_amd import synth  # noqa: E402
from seqrush_amd.seqrush import Context, Params, SeqSet, SortParams, graph_stats, sgd_layout, sort_gfa, sort_stats  # noqa: E402


def quality(text):
    """the overall MAE of the statistics stage, on the device"""
    d = graph_stats(text, 0)
    return d["total_abs"] / max(d["total_pairs"], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip the host twin and the sequential yardstick")
    a = ap.parse_args()
    for cfg in a.configs.split(","):
        recs = {"C2": synth.config_c2, "C4": synth.config_c4}[cfg]()
        ss = SeqSet(recs)
        ctx = Context(0)
        ctx.load(ss, Params())
        ctx.run()
        ctx.sync()
        unsorted = ctx.build_gfa(compact=True)[0]
        stage = []
        for _ in range(a.reps + 1):
            sorted_text = ctx.build_gfa(compact=True, sort=SortParams(device=0))[0]
            st = sort_stats()
            stage.append(st)
        ctx.close()
        stage = stage[1:]
        dev = [sgd_layout(unsorted, device=0) for _ in range(a.reps + 1)]
        sgd_ms = []
        for _ in range(a.reps):
            sgd_layout(unsorted, device=0)
            sgd_ms.append(sort_stats()["sgd_ms"])
        st = sort_stats()
        out = dict(config=cfg, nodes=int(st["nodes"]), steps=int(st["steps"]), terms_per_iter=int(st["terms_per_iter"]),
                   iterations=int(st["iterations"]), subrounds_per_iter=int(st["subrounds_per_iter"]),
                   sgd_device_ms=round(statistics.median(sgd_ms), 3),
                   groom_ms=round(statistics.median(s["groom_ms"] for s in stage), 3),
                   topo_ms=round(statistics.median(s["topo_ms"] for s in stage), 3),
                   write_ms=round(statistics.median(s["write_ms"] for s in stage), 3),
                   sort_stage_ms=round(statistics.median(s["stage_ms"] for s in stage), 3),
                   sort_parts_ms=round(statistics.median(s["sgd_ms"] + s["groom_ms"] + s["topo_ms"] + s["write_ms"]
                                                         for s in stage), 3),
                   reproducible=all(d.tobytes() == dev[0].tobytes() for d in dev))
        out["quality_unsorted"] = round(quality(unsorted), 4)
        out["quality_device"] = round(quality(sorted_text), 4)
        if not a.no_host:
            twin = sgd_layout(unsorted, device=-1)
            out["sgd_host_twin_ms"] = round(sort_stats()["sgd_ms"], 3)
            out["device_equals_twin"] = twin.tobytes() == dev[0].tobytes()
            sgd_layout(unsorted, device=-2)
            out["sgd_sequential_ms"] = round(sort_stats()["sgd_ms"], 3)
            out["twin_over_device"] = round(out["sgd_host_twin_ms"] / max(out["sgd_device_ms"], 1e-9), 1)
            out["quality_sequential"] = round(quality(sort_gfa(unsorted, device=-2)), 4)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
