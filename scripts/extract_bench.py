#!/usr/bin/env python3
"""The extract stage (--extract-*) on the device against its host twin on one thread, one JSON line per input, region set and
option set:
  device_us / twin_us        the stage (device: hipEvents from the first kernel to the end of the emission, with the
                             synchronisations of the merge rounds inside; twin: host clock over its sections), median of
                             --reps after a warm-up
  device_kernel_us / twin_kernel_us   per group: positions, seeds, context, merge, numbering, emission
  stage_ratio                twin / device for the stage
  wall_device_ms / wall_twin_ms   extract() end to end: parsing the GFA and the regions, tables, buffers, copies, the stage
                             and the result tables (not the GFA text, which is formed by the same code for both)
The inputs are the compacted graphs of C2 (64 paths) and of config_c5_like(16, 6000), induced on the device, and the
synthetic graph of 256 paths through 33 333 bubbles of scripts/variants_bench.py.  The region sets are seeded: one locus of
5 kb, a hundred loci of 1 kb over all paths, and one whole path; the option sets are the defaults and the defaults with two
steps of context.  Device and twin must agree on every table, every counter and the output bytes before a time is reported.

    python scripts/extract_bench.py [--inputs c2,c5_like,synthetic] [--reps 3] [--out profiles/extract_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from seqrush_amd import synth                                   # noqa: E402
from seqrush_amd.seqrush import Context, Params, SeqSet, Extract, EXTRACT_KERNELS, EXTRACT_COUNTERS         # noqa: E402
from lift_bench import path_lengths                             # noqa: E402
from variants_bench import synthetic                            # noqa: E402

INPUTS = {
    "c1": synth.config_c1,
    "c2": synth.config_c2,
    "c5_like": lambda: synth.config_c5_like(16, 6000),
    "synthetic": None,
}
TABLES = ("level", "node_old", "edge_from", "edge_to", "sub_path", "sub_start", "sub_end", "sub_off", "sub_steps")
OPTIONS = {"default": {}, "context_2": dict(context_steps=2)}


def region_sets(text, seed=23):
    """name -> region strings"""
    rng = np.random.default_rng(seed)
    paths = [(name, L) for name, L in path_lengths(text) if L]

    def locus(size):
        name, L = paths[int(rng.integers(0, len(paths)))]
        a = int(rng.integers(0, max(1, L - size)))
        return f"{name}:{a}-{min(L, a + size)}"
    return {"one_5kb": (locus(5000),), "hundred_1kb": tuple(locus(1000) for _ in range(100)), "whole_path": (paths[0][0],)}


def runs(text, regions, device, reps, **kw):
    with Extract(text, regions, None, device, **kw) as v:
        first, out = v.as_dict(), v.gfa()
    us, kernel, wall = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        with Extract(text, regions, None, device, **kw) as v:
            s = v.p.contents
            us.append(int(s.extract_us))
            kernel.append([int(x) for x in s.kernel_us])
        wall.append((time.perf_counter() - t0) * 1e3)
    return first, out, statistics.median(us), {k: statistics.median(r[i] for r in kernel) for i, k in enumerate(EXTRACT_KERNELS)}, statistics.median(wall)


def same(dev, twin, dev_out, twin_out, what):
    for k in EXTRACT_COUNTERS + ("sub_names",):
        assert dev[k] == twin[k], f"{what}: device and twin differ in {k}"
    for k in TABLES:
        assert dev[k].shape == twin[k].shape and (dev[k] == twin[k]).all(), f"{what}: device and twin differ in {k}"
    assert dev_out == twin_out, f"{what}: device and twin differ in the output bytes"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="c2,c5_like,synthetic")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the rows to this file as a JSON list")
    ns = ap.parse_args()
    rows = []
    for name in ns.inputs.split(","):
        make = INPUTS[name]
        if make is None:
            text = synthetic()
        else:
            ctx = Context(ns.device)
            ctx.load(SeqSet(make()), Params())
            ctx.run()
            ctx.sync()
            text = ctx.build_gfa(compact=True)[0]
            ctx.close()
        for rname, regions in region_sets(text).items():
            for oname, kw in OPTIONS.items():
                what = f"{name} {rname} {oname}"
                twin, twin_out, twin_us, twin_k, twin_wall = runs(text, regions, -1, ns.reps, **kw)
                dev, dev_out, dev_us, dev_k, dev_wall = runs(text, regions, ns.device, ns.reps, **kw)
                same(dev, twin, dev_out, twin_out, what)
                row = {"input": name, "region_set": rname, "options": oname, **{k: dev[k] for k in EXTRACT_COUNTERS}, "device_us": dev_us, "twin_us": twin_us,
                       "device_kernel_us": dev_k, "twin_kernel_us": twin_k, "stage_ratio": round(twin_us / max(dev_us, 1), 2),
                       "wall_device_ms": round(dev_wall, 3), "wall_twin_ms": round(twin_wall, 3),
                       "not_measured": "counters; an early exit of the context loop; other defaults of merge_distance and merge_rounds; --gpus 2"}
                rows.append(row)
                print(json.dumps(row), flush=True)
    if ns.out:
        with open(ns.out, "w") as fh:
            json.dump(rows, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
