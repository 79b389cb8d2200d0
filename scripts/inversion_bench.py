#!/usr/bin/env python3
"""--patch-inversions against the plain run on one GPU: wall time of align + unite (host clock, after a warm-up run, median
of 3), scan ms, patch-align ms, alignment-kernel ms, jobs, accepted, nodes.  One JSON line per input.  With --join N a third
run per input uses --inversion-join N: its scan ms is the joined instances' beside the plain instances', and it adds the
jobs rejected by site cost, the islands absorbed and the host ms of the patch pass.
usage: inversion_bench.py [--n 8] [--len 6000] [--c5-subset 0] [-k 16] [--join 0]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from seqrush_amd import synth                                   # noqa: E402
from seqrush_amd.seqrush import Context, Params, SeqSet         # noqa: E402


def one(recs, k, patch, reps=3, join=0):
    ss = SeqSet(recs)
    ctx = Context(0)
    p = Params()
    p.c.min_match_len = k
    ctx.load(ss, p)
    if patch:
        ctx.enable_inversions(join_below=join)
    walls = []
    for i in range(reps + 1):
        ctx.reset_uf(); ctx.sync()
        t0 = time.perf_counter()
        ctx.run(); ctx.sync()
        if i:
            walls.append((time.perf_counter() - t0) * 1e3)
    out = dict(patch=patch, join=join, wall_ms=round(statistics.median(walls), 2), align_ms=round(ctx.kernel_ms(0), 2),
               batches=ctx.num_batches, nodes=ctx.build_gfa(compact=False)[1])
    if patch:
        st = ctx.inversion_stats()
        out.update(scan_ms=round(st["scan_ms"], 3), patch_align_ms=round(st["patch_align_ms"], 3), jobs=st["candidates"],
                   accepted=st["accepted"], sites=st["sites"], scan_over_align=round(st["scan_ms"] / max(ctx.kernel_ms(0), 1e-9), 5))
        if join:
            js = ctx.inversion_join_stats()
            out.update(rejected=st["rejected_score"] + st["rejected_divergence"], rejected_site_cost=js["rejected_site_cost"],
                       islands_absorbed=js["islands_absorbed"], host_ms=round(js["host_us"] / 1e3, 3),
                       patch_batches=st["patch_batches"])
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--len", type=int, default=6000)
    ap.add_argument("--c5-subset", type=int, default=0, help="also run the first N sequences of config_c5 (50 kb each)")
    ap.add_argument("-k", type=int, default=16)
    ap.add_argument("--join", type=int, default=0, help="also run with --inversion-join N")
    ns = ap.parse_args()
    inputs = [(f"c5_like_{ns.n}x{ns.len}", synth.config_c5_like(ns.n, ns.len))]
    if ns.c5_subset:
        inputs.append((f"c5_first_{ns.c5_subset}", synth.config_c5(ns.c5_subset)))
    for name, recs in inputs:
        for patch, join in ((False, 0), (True, 0)) + (((True, ns.join),) if ns.join else ()):
            print(json.dumps(dict(input=name, k=ns.k, **one(recs, ns.k, patch, join=join))), flush=True)


if __name__ == "__main__":
    main()
