#!/usr/bin/env python3
"""--extend measured, one JSON line per row:
  (a) stage    the spell and seed groups on the device (hipEvents) against the host twin on one thread (host clock), on the
               graph of all but the last --new sequences of C2, uncompacted and compacted, and of config_c5_like(16, 6000),
               compacted; the merged bytes and the seeded labels must agree before a time is reported
  (b) end_to_end   C2 split 60 + 4: plan + load_extend + run + sync + graph against load + run + sync + graph of all 64 on a
               host clock, the pair counts beside the times; the two GFA texts must be the same bytes
Every time is the median of --reps runs after one warm-up.

    python scripts/extend_bench.py [--reps 3] [--new 4] [--out profiles/extend_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from seqrush_amd import synth                                   # noqa: E402
from seqrush_amd.seqrush import Context, ExtendPlan, HostUnionFind, Params, SeqSet, extend_seed_host     # noqa: E402

NOT_MEASURED = ("hardware counters of the two groups; the alternative mapping of the seed (one wave per step, for long nodes): "
                "not built; a full-size C5 split")


def build(recs, device, compact):
    ctx = Context(device)
    ctx.load(SeqSet(recs), Params())
    ctx.run(); ctx.sync()
    text = ctx.build_gfa(compact=compact)[0]
    pairs = ctx.num_pairs
    ctx.close()
    return text, pairs


def device_stage(text, new, device):
    with ExtendPlan(text, new, device=device) as plan:
        ctx = Context(device)
        ctx.load_extend(plan, Params())
        ctx.sync()
        st, lab, recs = ctx.extend_stats(), ctx.download_labels(), plan.records
        ctx.close()
    return st, lab, recs


def twin_stage(text, new):
    with ExtendPlan(text, new, device=-1) as plan:
        uf = HostUnionFind(plan.seqset.total_length)
        t0 = time.perf_counter()
        cnt = extend_seed_host(plan, uf)
        seed_us = (time.perf_counter() - t0) * 1e6
        return dict(plan.stats(), seed_us=int(seed_us + 0.5), **cnt), uf.canonical_labels(), plan.records


def stage_row(name, recs, n_new, compact, device, reps):
    text, _ = build(recs[:-n_new], device, compact)
    new = recs[-n_new:]
    dev, dev_lab, dev_recs = device_stage(text, new, device)            # warm-up and the comparison
    twin, twin_lab, twin_recs = twin_stage(text, new)
    assert dev_recs == twin_recs == [(n, bytes(s)) for n, s in recs], "merged bytes differ"
    assert np.array_equal(dev_lab, twin_lab), "seeded labels differ"
    assert (dev["unions_attempted"], dev["unions_joined"]) == (twin["unions_attempted"], twin["unions_joined"])
    d = [device_stage(text, new, device)[0] for _ in range(reps)]
    t = [twin_stage(text, new)[0] for _ in range(reps)]
    med = lambda rows, k: statistics.median(r[k] for r in rows)     # noqa: E731
    return {"row": "stage", "input": name, "compacted": compact, "old_paths": dev["old_paths"], "old_bases": dev["old_bases"],
            "old_steps": dev["old_steps"], "unions_attempted": dev["unions_attempted"], "unions_joined": dev["unions_joined"],
            "device_spell_us": med(d, "spell_us"), "device_seed_us": med(d, "seed_us"), "twin_spell_us": med(t, "spell_us"),
            "twin_seed_us": med(t, "seed_us"), "not_measured": NOT_MEASURED}


def end_to_end_row(recs, n_new, device, reps):
    old_text, old_pairs = build(recs[:-n_new], device, False)

    def one_shot():
        t0 = time.perf_counter()
        text, pairs = build(recs, device, False)
        return (time.perf_counter() - t0) * 1e3, text, pairs

    def extend():
        t0 = time.perf_counter()
        with ExtendPlan(old_text, recs[-n_new:], device=device) as plan:
            ctx = Context(device)
            ctx.load_extend(plan, Params())
            ctx.run(); ctx.sync()
            text = ctx.build_gfa(compact=False)[0]
            ms = (time.perf_counter() - t0) * 1e3
            st = ctx.extend_stats()
            ctx.close()
        return ms, text, st

    _, want, all_pairs = one_shot()
    _, got, st = extend()
    assert got == want, "the extended graph is not the one-shot graph"
    a = [one_shot()[0] for _ in range(reps)]
    b = [extend()[0] for _ in range(reps)]
    return {"row": "end_to_end", "input": f"c2 {len(recs) - n_new}+{n_new}", "one_shot_pairs": all_pairs, "extend_pairs": st["pairs_after"],
            "old_pairs": old_pairs, "one_shot_ms": round(statistics.median(a), 3), "extend_ms": round(statistics.median(b), 3),
            "spell_us": st["spell_us"], "seed_us": st["seed_us"], "not_measured": NOT_MEASURED}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--new", type=int, default=4)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the rows to this file as a JSON list")
    ns = ap.parse_args()
    c2, c5 = synth.config_c2(), synth.config_c5_like(16, 6000)
    rows = []
    for row in (lambda: stage_row("c2", c2, ns.new, False, ns.device, ns.reps), lambda: stage_row("c2", c2, ns.new, True, ns.device, ns.reps),
                lambda: stage_row("c5_like", c5, ns.new, True, ns.device, ns.reps), lambda: end_to_end_row(c2, ns.new, ns.device, ns.reps)):
        rows.append(row())
        print(json.dumps(rows[-1]), flush=True)
    if ns.out:
        with open(ns.out, "w") as fh:
            json.dump(rows, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
