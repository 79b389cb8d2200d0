#!/usr/bin/env python3
"""The statistics stage (--stats) on the device against its host twin on one thread, one JSON line per input:
  device_us / twin_us        the stage (device: hipEvents from the first kernel to the last; twin: host clock over the same
                             five sections), median of --reps after a warm-up
  device_kernel_us / twin_kernel_us   the same per section: steps, nodes, similarity, layout, topology
  similarity_ratio           twin / device for the similarity section
  wall_device_ms / wall_twin_ms   graph_stats() end to end: parsing, tables, buffers, copies and the stage
The inputs are the compacted graphs of C2 and of config_c5_like, induced on the device; device and twin must agree.

    python scripts/stats_bench.py [--inputs c2,c5_like] [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from seqrush_amd import synth                                   # noqa: E402
from seqrush_amd.seqrush import Context, Params, SeqSet, graph_stats, STATS_KERNELS         # noqa: E402

INPUTS = {
    "c1": synth.config_c1,
    "c2": synth.config_c2,
    "c5_like": lambda: synth.config_c5_like(16, 6000),
}


def runs(text, device, reps):
    graph_stats(text, device)
    out, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        out.append(graph_stats(text, device))
        wall.append((time.perf_counter() - t0) * 1e3)
    med = lambda f: statistics.median(f(d) for d in out)         # noqa: E731
    return out[0], med(lambda d: d["stats_us"]), {k: med(lambda d: d["kernel_us"][k]) for k in STATS_KERNELS}, statistics.median(wall)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="c2,c5_like")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ns = ap.parse_args()
    for name in ns.inputs.split(","):
        recs = INPUTS[name]()
        ctx = Context(ns.device)
        ctx.load(SeqSet(recs), Params())
        ctx.run()
        ctx.sync()
        text = ctx.build_gfa(compact=True)[0]
        ctx.close()
        dev, dev_us, dev_k, dev_wall = runs(text, ns.device, ns.reps)
        twin, twin_us, twin_k, twin_wall = runs(text, -1, ns.reps)
        for k in ("length", "depth_bp", "total_abs", "total_sq", "tips", "components"):
            assert dev[k] == twin[k], k
        assert (dev["shared"] == twin["shared"]).all()
        pair_updates = int(sum(int(c) * (int(c) + 1) // 2 for c in dev["paths_on"]))
        row = {"input": name, "nodes": dev["nodes"], "edges": dev["edges"], "paths": dev["paths"], "steps": dev["steps"],
               "similarity_pair_updates": pair_updates, "device_us": dev_us, "twin_us": twin_us, "device_kernel_us": dev_k,
               "twin_kernel_us": twin_k, "similarity_ratio": round(twin_k["similarity"] / max(dev_k["similarity"], 1), 2),
               "wall_device_ms": round(dev_wall, 3), "wall_twin_ms": round(twin_wall, 3)}
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
