#!/usr/bin/env python3
"""layout_bench.py -- the 2-D layout stage (--layout) on one GPU: one JSON line per graph.

    python scripts/layout_bench.py [--configs C2,C5like] [--reps 5] [--no-host]

Per graph (aligned, united and induced on the device, compacted -- the graph `--layout` receives):
  nodes, steps, terms_per_iter, iterations, subrounds_per_iter, terms_per_round
  sgd_device_ms       hipEvents around the SGD launches, median of --reps after one warm-up
  stage_ms            host-clock wall time of one sr_layout_gfa call (parse, tables, buffers, copies, SGD), same runs
  terms_per_second    terms_per_iter * iterations / sgd_device_ms
  sgd_host_twin_ms    the same schedule on one host thread (bit-identical end points; checked)
  sgd_sequential_ms   the yardstick: every term applied at once
  stress_*            sampled path stress (sr_layout_quality, 200 000 draws) of the initial state, the device layout and
                      the yardstick's
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402,F401  (first HIP runtime in the process, as in the test suite)

import layout_helpers as lh  # noqa: E402  (the restatement's initial state)
import sort_helpers as sh  # noqa: E402
from seqrush_amd import synth  # noqa: E402
from seqrush_amd.seqrush import Context, Params, SeqSet, layout_gfa, layout_quality, layout_resolve, layout_stats  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C5like")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip the host twin and the sequential yardstick")
    a = ap.parse_args()
    for cfg in a.configs.split(","):
        recs = {"C2": synth.config_c2, "C5like": synth.config_c5_like}[cfg]()
        ctx = Context(0)
        ctx.load(SeqSet(recs), Params())
        ctx.run()
        ctx.sync()
        text = ctx.build_gfa(compact=True)[0]
        ctx.close()

        def stress(xy):
            return layout_quality(text, xy, seed=1, samples=200000)["stress"]
        dev = layout_gfa(text, device=0)                       # warm-up
        runs = []
        for _ in range(a.reps):
            again = layout_gfa(text, device=0)
            runs.append(layout_stats())
            assert again.tobytes() == dev.tobytes(), "device layout differs run to run"
        st = runs[0]
        sgd_ms = statistics.median(r["sgd_ms"] for r in runs)
        out = dict(config=cfg, nodes=int(st["nodes"]), steps=int(st["steps"]), terms_per_iter=int(st["terms_per_iter"]),
                   iterations=int(st["iterations"]), subrounds_per_iter=int(st["subrounds_per_iter"]),
                   terms_per_round=int(layout_resolve(text)["terms_per_round"]),
                   sgd_device_ms=round(sgd_ms, 3), stage_ms=round(statistics.median(r["stage_ms"] for r in runs), 3),
                   terms_per_second=round(st["terms_per_iter"] * st["iterations"] / (sgd_ms * 1e-3)),
                   stress_initial=stress(lh.initial_state(sh.Gfa.parse(text))),
                   stress_device=stress(dev))
        if not a.no_host:
            twin = layout_gfa(text, device=-1)
            out["sgd_host_twin_ms"] = round(layout_stats()["sgd_ms"], 3)
            out["device_equals_twin"] = twin.tobytes() == dev.tobytes()
            seq = layout_gfa(text, device=-2)
            out["sgd_sequential_ms"] = round(layout_stats()["sgd_ms"], 3)
            out["stress_sequential"] = stress(seq)
            out["twin_over_device"] = round(out["sgd_host_twin_ms"] / max(out["sgd_device_ms"], 1e-9), 1)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
