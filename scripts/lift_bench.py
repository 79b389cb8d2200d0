#!/usr/bin/env python3
"""The lift stage (--lift) on the device against its host twin on one thread, one JSON line per input:
  device_us / twin_us        the stage (device: hipEvents from the first kernel to the end of the download; twin: host clock
                             over its sections), median of --reps after a warm-up
  device_kernel_us / twin_kernel_us   per group: positions, first_visits, locate, short_pairs, long_pairs (the twin walks
                             every pair in one loop, booked under short_pairs, and has no locate group of its own)
  stage_ratio                twin / device for the stage
  wall_device_ms / wall_twin_ms   lift() end to end: parsing the GFA and the BED, tables, buffers, copies and the stage
  short_pairs / long_pairs   the pairs each of the two pair kernels took at the default short_steps
  all_short_us / all_long_us the short_pairs and long_pairs groups when one kernel takes every pair (short_steps = 2^64 - 1
                             and 0)
The inputs are the compacted graphs of C2 (64 paths) and of config_c5_like(16, 6000), induced on the device, and the
synthetic graph of 256 paths through 33 333 bubbles of scripts/variants_bench.py.  The queries are seeded: half of them
one base, half 1 to 5 kb (cut at the end of their path), over all paths, against every path.  Device and twin must agree
on every field and on the output bytes before a time is reported.

    python scripts/lift_bench.py [--inputs c2,c5_like,synthetic] [--reps 3] [--out profiles/lift_bench.json]
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
from seqrush_amd.seqrush import Context, Params, SeqSet, Lift, LIFT_KERNELS         # noqa: E402
from variants_bench import synthetic                            # noqa: E402

INPUTS = {
    "c1": (synth.config_c1, 1000),
    "c2": (synth.config_c2, 10000),
    "c5_like": (lambda: synth.config_c5_like(16, 6000), 10000),
    "synthetic": (None, 2000),
}
FIELDS = ("q_path", "q_start", "q_end", "target_path", "tstart", "tend", "covered", "rev_bp")


def path_lengths(text):
    """name and length of every path, from the text"""
    ln, out = {}, []
    for line in text.split("\n"):
        f = line.split("\t")
        if f[0] == "S":
            ln[f[1]] = len(f[2])
        elif f[0] == "P":
            out.append((f[1], sum(ln[s[:-1]] for s in f[2].split(",")) if f[2] else 0))
    return out


def queries(text, n, seed=20):
    rng = np.random.default_rng(seed)
    paths = [(name, L) for name, L in path_lengths(text) if L]
    rows = []
    for k in range(n):
        name, L = paths[int(rng.integers(0, len(paths)))]
        a = int(rng.integers(0, L))
        b = a + 1 if k % 2 == 0 else min(L, a + int(rng.integers(1000, 5001)))
        rows.append(f"{name}\t{a}\t{b}\tq{k}\n")
    return "".join(rows)


def runs(text, bed, device, reps, **kw):
    with Lift(text, bed, device, **kw) as v:
        first, out = v.as_dict(), v.bed()
    us, kernel, wall = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        with Lift(text, bed, device, **kw) as v:
            s = v.p.contents
            us.append(int(s.lift_us))
            kernel.append([int(x) for x in s.kernel_us])
        wall.append((time.perf_counter() - t0) * 1e3)
    return first, out, statistics.median(us), {k: statistics.median(r[i] for r in kernel) for i, k in enumerate(LIFT_KERNELS)}, statistics.median(wall)


def same(dev, twin, dev_out, twin_out, what):
    for k in ("queries", "targets", "paths", "unknown", "out_of_range", "mapped", "labels"):
        assert dev[k] == twin[k], f"{what}: device and twin differ in {k}"
    for k in FIELDS:
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
        make, n_queries = INPUTS[name]
        if make is None:
            text = synthetic()
        else:
            ctx = Context(ns.device)
            ctx.load(SeqSet(make()), Params())
            ctx.run()
            ctx.sync()
            text = ctx.build_gfa(compact=True)[0]
            ctx.close()
        bed = queries(text, n_queries)
        twin, twin_out, twin_us, twin_k, twin_wall = runs(text, bed, -1, ns.reps)
        dev, dev_out, dev_us, dev_k, dev_wall = runs(text, bed, ns.device, ns.reps)
        same(dev, twin, dev_out, twin_out, name)
        split = {}
        for key, short, group in (("all_short_us", 2 ** 64 - 1, "short_pairs"), ("all_long_us", 0, "long_pairs")):
            d, out, _, k, _ = runs(text, bed, ns.device, ns.reps, short_steps=short)
            same(d, twin, out, twin_out, f"{name} short_steps={short}")
            split[key] = k[group]
        nodes = sum(1 for line in text.split("\n") if line.startswith("S\t"))
        steps = sum(line.count(",") + 1 for line in text.split("\n") if line.startswith("P\t"))
        row = {"input": name, "nodes": nodes, "steps": steps, "paths": dev["paths"], "queries": dev["queries"], "targets": dev["targets"],
               "mapped": dev["mapped"], "short_pairs": dev["short_pairs"], "long_pairs": dev["long_pairs"], "device_us": dev_us, "twin_us": twin_us,
               "device_kernel_us": dev_k, "twin_kernel_us": twin_k, "stage_ratio": round(twin_us / max(dev_us, 1), 2),
               "wall_device_ms": round(dev_wall, 3), "wall_twin_ms": round(twin_wall, 3), **split,
               "not_measured": "a path-major first-visit table; counters; --gpus 2"}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if ns.out:
        with open(ns.out, "w") as fh:
            json.dump(rows, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
