#!/usr/bin/env python3
"""The growth stage (--growth) on the device against its host twin on one thread, one JSON line per input:
  device_us / twin_us        the stage (device: hipEvents from the first kernel to the end of the download; twin: host clock
                             over the same four sections), median of --reps after a warm-up
  device_kernel_us / twin_kernel_us   the same per section: presence, histogram, ranks, growth
  growth_ratio / stage_ratio twin / device for the growth section and for the stage
  dense_kernel_us            the device sections of the same library built with the LDS copy of the node lengths stored
                             densely (`make -C seqrush_amd/csrc growth-dense`: row stride 64 dwords instead of the padded
                             65), measured by a child process that loads that library; absent if it is not built
  wall_device_ms / wall_twin_ms   growth() end to end: parsing, tables, buffers, copies and the stage
The inputs are the compacted graphs of C2 (64 paths) and of config_c5_like(16, 6000), induced on the device, every path its
own group, and a synthetic graph of 256 one-path groups on 100 000 nodes (three quarters of it shared by a random half of
the groups) that is closer to the size the stage is for.  Device and twin must agree on every table before a time is
reported.  There is one kernel variant, so there is no variant to force; the dense build is the evidence for its LDS layout.

    python scripts/growth_bench.py [--inputs c2,c5_like,synthetic] [--reps 5] [--permutations 1000] [--out profiles/growth_bench.json]
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from seqrush_amd import synth                                   # noqa: E402
from seqrush_amd.seqrush import Context, Params, SeqSet, growth, GROWTH_KERNELS         # noqa: E402

DENSE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "seqrush_amd", "libseqrush_amd_growthdense.so")
INPUTS = {
    "c1": synth.config_c1,
    "c2": synth.config_c2,
    "c5_like": lambda: synth.config_c5_like(16, 6000),
}


def synthetic(V=100000, G=256, seed=5):
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 41, size=V)
    out = ["H\tVN:Z:1.0\n"] + [f"S\t{v + 1}\t{'ACGT'[v % 4] * int(lens[v])}\n" for v in range(V)]
    shared = rng.random(V) < 0.75
    for g in range(G):
        on = np.flatnonzero((shared & (rng.random(V) < 0.5)) | (rng.random(V) < 0.002)) + 1
        out.append(f"P\tg{g}\t" + ",".join(f"{v}+" for v in on) + "\t*\n")
    return "".join(out)


def runs(text, device, reps, permutations):
    growth(text, device, permutations=permutations)
    out, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        out.append(growth(text, device, permutations=permutations))
        wall.append((time.perf_counter() - t0) * 1e3)
    med = lambda f: statistics.median(f(d) for d in out)         # noqa: E731
    return out[0], med(lambda d: d["growth_us"]), {k: med(lambda d: d["kernel_us"][k]) for k in GROWTH_KERNELS}, statistics.median(wall)


def digest(d):
    return hashlib.sha256(b"".join(d[k].tobytes() for k in ("pan", "core", "perm", "bp_by_groups"))).hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="c2,c5_like,synthetic")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--permutations", type=int, default=1000)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the rows to this file as a JSON list")
    ap.add_argument("--measure", default=None, metavar="GFA", help="(child) measure the loaded library on this GFA file only")
    ns = ap.parse_args()
    if ns.measure:
        d, us, k, _ = runs(open(ns.measure).read(), ns.device, ns.reps, ns.permutations)
        print(json.dumps(dict(digest=digest(d), us=us, kernel_us=k)))
        return
    rows = []
    for name in ns.inputs.split(","):
        if name == "synthetic":
            text = synthetic()
        else:
            ctx = Context(ns.device)
            ctx.load(SeqSet(INPUTS[name]()), Params())
            ctx.run()
            ctx.sync()
            text = ctx.build_gfa(compact=True)[0]
            ctx.close()
        dev, dev_us, dev_k, dev_wall = runs(text, ns.device, ns.reps, ns.permutations)
        twin, twin_us, twin_k, twin_wall = runs(text, -1, ns.reps, ns.permutations)
        for k in ("pan", "core", "perm", "bp_by_groups"):
            assert (dev[k] == twin[k]).all(), f"device and twin differ in {k}"
        nodes = sum(1 for line in text.split("\n") if line.startswith("S\t"))
        row = {"input": name, "nodes": nodes, "length": dev["length"], "groups": dev["groups"], "permutations": dev["permutations"],
               "exhaustive": dev["exhaustive"], "variant": dev["variant"], "device_us": dev_us, "twin_us": twin_us,
               "device_kernel_us": dev_k, "twin_kernel_us": twin_k,
               "growth_ratio": round(twin_k["growth"] / max(dev_k["growth"], 1), 2), "stage_ratio": round(twin_us / max(dev_us, 1), 2),
               "wall_device_ms": round(dev_wall, 3), "wall_twin_ms": round(twin_wall, 3)}
        if os.path.exists(DENSE):
            tmp = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"growth_bench_{os.getpid()}_{name}.gfa")
            with open(tmp, "w") as fh:
                fh.write(text)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--measure", tmp, "--reps", str(ns.reps), "--device", str(ns.device),
                                "--permutations", str(ns.permutations)], capture_output=True, text=True,
                               env=dict(os.environ, SEQRUSH_AMD_LIB=DENSE), timeout=600)
            os.unlink(tmp)
            if r.returncode != 0:
                raise SystemExit("the dense build failed: " + r.stderr[-2000:])
            dense = json.loads(r.stdout.strip().split("\n")[-1])
            assert dense["digest"] == digest(dev), "the dense build differs"
            row.update(dense_us=dense["us"], dense_kernel_us=dense["kernel_us"])
        rows.append(row)
        print(json.dumps(row), flush=True)
    if ns.out:
        with open(ns.out, "w") as fh:
            json.dump(rows, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
