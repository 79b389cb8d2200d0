#!/usr/bin/env python3
"""The path-by-bin stage (--bin / --viz) on the device against two yardsticks, one JSON line per input and setting:
  device_us / device_steps_us   the stage and its step kernel by hipEvents, median of --reps after a warm-up
  twin_us / twin_steps_us       the host twin on one thread, host clock over the same sections
  plain_us / plain_steps_us     the same kernels built without the wave-level run reduction (`make -C seqrush_amd/csrc
                                bin-plain`), measured by a child process that loads that library; absent if it is not built
  wall_device_ms / wall_twin_ms path_bins() end to end: parsing, tables, buffers, copies and the stage
The inputs are the compacted, sorted graphs of C2 and of config_c5_like(16, 6000), induced on the device; the settings are
--bin-count 1500 (rows in LDS), --bin-width 1 (global atomics) and --bin-count 16 (the most contended case).  Device, twin and plain build must agree.

    python scripts/bin_bench.py [--inputs c2,c5_like] [--reps 5] [--out profiles/bin_bench.json]
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from seqrush_amd import synth                                   # noqa: E402
from seqrush_amd.seqrush import Context, Params, SeqSet, SortParams, graph_stats, path_bins         # noqa: E402

INPUTS = {
    "c1": synth.config_c1,
    "c2": synth.config_c2,
    "c5_like": lambda: synth.config_c5_like(16, 6000),
}
# the third setting is not a use case: 64 lanes of a wave on one or two addresses, where the run reduction has the most to remove
SETTINGS = (("bin_count_1500", dict(bins=1500)), ("bin_width_1", dict(bin_width=1)), ("bin_count_16", dict(bins=16)))
PLAIN = os.path.join(ROOT, "seqrush_amd", "libseqrush_amd_binplain.so")


def runs(text, device, reps, kw):
    path_bins(text, device, **kw)
    out, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        out.append(path_bins(text, device, **kw))
        wall.append((time.perf_counter() - t0) * 1e3)
    digest = hashlib.sha256(out[0]["cov"].tobytes() + out[0]["inv"].tobytes()).hexdigest()[:16]
    return dict(us=statistics.median(d["bin_us"] for d in out), steps_us=statistics.median(d["kernel_us"]["steps"] for d in out),
                scan_us=statistics.median(d["kernel_us"]["scan"] for d in out),
                download_us=statistics.median(d["kernel_us"]["download"] for d in out),
                wall_ms=round(statistics.median(wall), 3), digest=digest, bins=out[0]["bins"], paths=out[0]["paths"],
                length=out[0]["length"], depth_bp=int(out[0]["cov"].sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="c2,c5_like")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the rows to this file as a JSON list")
    ap.add_argument("--measure", default=None, metavar="GFA", help="(child) measure the loaded library on this GFA file only")
    ns = ap.parse_args()
    if ns.measure:
        text = open(ns.measure).read()
        print(json.dumps({name: runs(text, ns.device, ns.reps, kw) for name, kw in SETTINGS}))
        return
    rows = []
    for name in ns.inputs.split(","):
        ctx = Context(ns.device)
        ctx.load(SeqSet(INPUTS[name]()), Params())
        ctx.run()
        ctx.sync()
        text = ctx.build_gfa(compact=True, sort=SortParams(device=ns.device))[0]
        ctx.close()
        steps = int(graph_stats(text, -1)["steps"])
        plain = None
        if os.path.exists(PLAIN):
            tmp = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"bin_bench_{os.getpid()}_{name}.gfa")
            with open(tmp, "w") as fh:
                fh.write(text)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--measure", tmp, "--reps", str(ns.reps), "--device", str(ns.device)],
                               capture_output=True, text=True, env=dict(os.environ, SEQRUSH_AMD_LIB=PLAIN), timeout=600)
            os.unlink(tmp)
            if r.returncode != 0:
                raise SystemExit("the plain build failed: " + r.stderr[-2000:])
            plain = json.loads(r.stdout.strip().split("\n")[-1])
        for sname, kw in SETTINGS:
            dev, twin = runs(text, ns.device, ns.reps, kw), runs(text, -1, ns.reps, kw)
            assert dev["digest"] == twin["digest"], "device and twin differ"
            row = {"input": name, "setting": sname, "length": dev["length"], "paths": dev["paths"], "bins": dev["bins"],
                   "steps": steps, "depth_bp": dev["depth_bp"],
                   "device_us": dev["us"], "device_scan_us": dev["scan_us"], "device_steps_us": dev["steps_us"],
                   "device_download_us": dev["download_us"], "twin_us": twin["us"], "twin_steps_us": twin["steps_us"],
                   "wall_device_ms": dev["wall_ms"], "wall_twin_ms": twin["wall_ms"]}
            if plain:
                assert plain[sname]["digest"] == dev["digest"], "the plain build differs"
                row.update(plain_us=plain[sname]["us"], plain_steps_us=plain[sname]["steps_us"])
            rows.append(row)
            print(json.dumps(row), flush=True)
    if ns.out:
        with open(ns.out, "w") as fh:
            json.dump(rows, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
