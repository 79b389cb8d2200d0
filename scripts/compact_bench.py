#!/usr/bin/env python3
"""Compaction on the host against compaction on the device (--compact-on), one JSON line per input:
  host_compaction_ms   sr_graph_compact + sr_graph_renumber on the host (stats of sr_compact_gfa device=-1: the greedy
                       procedure alone, no parsing or writing), median of --reps after a warm-up
  tables_on_host_ms    the table formulation in index order on the host (device=-2), same clock
  ctx_device_ms / ctx_copy_ms / rounds / jumps   stats of Context.build_gfa(compact_on="device"): hipEvents around the
                       rounds and the renumbering, host clock around the final download (the induced graph is on the device)
  text_device_ms / text_copy_ms   the same through sr_compact_gfa(device): upload of the parsed graph included in copy
  build_gfa_*_ms       wall time of Context.build_gfa: no compaction, compaction on the host, compaction on the device

    python scripts/compact_bench.py [--inputs c2,c5_like] [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from seqrush_amd import synth                                   # noqa: E402
from seqrush_amd.seqrush import Context, Params, SeqSet, compact_gfa, compact_stats         # noqa: E402

INPUTS = {
    "c1": synth.config_c1,
    "c2": synth.config_c2,
    "c5_like": lambda: synth.config_c5_like(16, 6000),
}


def med(f, reps):
    """median over reps of (wall ms, what f returned) by wall ms, after one warm-up call"""
    f()
    runs = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = f()
        runs.append(((time.perf_counter() - t0) * 1e3, r))
    runs.sort(key=lambda x: x[0])
    return runs[len(runs) // 2]


def stat_med(f, key, reps):
    f()
    return statistics.median(f()[key] for _ in range(reps)) / 1e3


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
        plain = ctx.build_gfa(compact=False)[0]
        row = {"input": name, "sequences": len(recs), "steps": sum(len(s) for _, s in recs), "nodes_induced": plain.count("\nS\t")}

        def text(device):
            st = {}
            compact_gfa(plain, device, st)
            return st
        row["host_compaction_ms"] = round(stat_med(lambda: text(-1), "compact_us", ns.reps), 3)
        row["tables_on_host_ms"] = round(stat_med(lambda: text(-2), "compact_us", ns.reps), 3)
        row["text_device_ms"] = round(stat_med(lambda: text(ns.device), "compact_us", ns.reps), 3)
        row["text_copy_ms"] = round(stat_med(lambda: text(ns.device), "copy_us", ns.reps), 3)

        def on_device():
            ctx.build_gfa(compact=True, compact_on="device")
            return compact_stats()
        row["build_gfa_nocompact_ms"] = round(med(lambda: ctx.build_gfa(compact=False), ns.reps)[0], 3)
        row["build_gfa_host_ms"] = round(med(lambda: ctx.build_gfa(compact=True, compact_on="host"), ns.reps)[0], 3)
        wall, st = med(on_device, ns.reps)
        row["build_gfa_device_ms"] = round(wall, 3)
        row["ctx_device_ms"], row["ctx_copy_ms"] = st["compact_us"] / 1e3, st["copy_us"] / 1e3
        for k in ("rounds", "host_rounds", "jumps", "chains", "longest_list"):
            row[k] = st[k]
        assert ctx.build_gfa(compact=True, compact_on="device") == ctx.build_gfa(compact=True, compact_on="host")
        ctx.close()
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
