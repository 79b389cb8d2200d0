#!/usr/bin/env python3
"""The variants stage (--vcf) on the device against its host twin on one thread, one JSON line per input:
  device_us / twin_us        the stage (device: hipEvents from the first kernel to the end of the download, the two counts
                             that come back in between included; twin: host clock over its sections), median of --reps
                             after a warm-up
  device_kernel_us / twin_kernel_us   per group: anchors, scan, emit, hash, sort_classes, genotypes (the twin has no scan and
                             no hash: it walks each path once and compares allele bytes directly, so those slots are 0)
  stage_ratio                twin / device for the stage
  wall_device_ms / wall_twin_ms   variants() end to end: parsing, tables, buffers, copies, the stage and the host work over
                             its output (the allele arena and the final numbering)
The inputs are the compacted graphs of C2 (64 paths) and of config_c5_like(16, 6000), induced on the device, against their
first path, and a synthetic graph of 256 paths through 33 333 bubbles (100 000 nodes; SNPs and every fifth a deletion) that
is closer to the size the stage is for.  Device and twin must agree on every field and on the VCF bytes before a time is
reported.

    python scripts/variants_bench.py [--inputs c2,c5_like,synthetic] [--reps 3] [--out profiles/variants_bench.json]
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
from seqrush_amd.seqrush import Context, Params, SeqSet, Variants, VARIANTS_KERNELS         # noqa: E402

INPUTS = {
    "c1": synth.config_c1,
    "c2": synth.config_c2,
    "c5_like": lambda: synth.config_c5_like(16, 6000),
}


def synthetic(B=33333, P=256, seed=5):
    """spine node 3k + 1, reference allele 3k + 2, other allele 3k + 3 (absent in every fifth bubble: a deletion)"""
    rng = np.random.default_rng(seed)
    out = ["H\tVN:Z:1.0\n"]
    base = rng.integers(0, 4, size=B)
    for k in range(B):
        out.append(f"S\t{3 * k + 1}\t{'ACGT'[k % 4] * int(1 + k % 8)}\nS\t{3 * k + 2}\t{'ACGT'[base[k]]}\nS\t{3 * k + 3}\t{'ACGT'[(base[k] + 1 + k % 3) % 4]}\n")
    out.append(f"S\t{3 * B + 1}\tACGT\n")
    freq = rng.random(B) * 0.6
    k3 = 3 * np.arange(B)
    for p in range(P):
        alt = (rng.random(B) < freq) & (p > 0)
        mid = np.where(alt, k3 + 3, k3 + 2)
        steps = np.stack([k3 + 1, mid], axis=1)
        keep = np.stack([np.ones(B, dtype=bool), ~(alt & (np.arange(B) % 5 == 4))], axis=1)
        ids = np.append(steps[keep], 3 * B + 1)
        out.append(f"P\tg{p}\t" + ",".join(f"{v}+" for v in ids.tolist()) + "\t*\n")
    return "".join(out)


def runs(text, device, reps):
    with Variants(text, device) as v:
        first, vcf = v.as_dict(), v.vcf()
    us, kernel, wall = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        with Variants(text, device) as v:
            s = v.p.contents
            us.append(int(s.variants_us))
            kernel.append([int(x) for x in s.kernel_us])
        wall.append((time.perf_counter() - t0) * 1e3)
    return first, vcf, statistics.median(us), {k: statistics.median(r[i] for r in kernel) for i, k in enumerate(VARIANTS_KERNELS)}, statistics.median(wall)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="c2,c5_like,synthetic")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the rows to this file as a JSON list")
    ns = ap.parse_args()
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
        dev, dev_vcf, dev_us, dev_k, dev_wall = runs(text, ns.device, ns.reps)
        twin, twin_vcf, twin_us, twin_k, twin_wall = runs(text, -1, ns.reps)
        for k in ("ref_path", "ref_len", "ref_seq", "paths", "anchors", "traversals", "sites", "alleles"):
            assert dev[k] == twin[k], f"device and twin differ in {k}"
        for k in ("breaks", "skipped", "site_start", "site_end", "site_alleles", "gt"):
            assert dev[k].shape == twin[k].shape and (dev[k] == twin[k]).all(), f"device and twin differ in {k}"
        assert dev_vcf == twin_vcf, "device and twin differ in the VCF bytes"
        nodes = sum(1 for line in text.split("\n") if line.startswith("S\t"))
        steps = sum(line.count(",") + 1 for line in text.split("\n") if line.startswith("P\t"))
        row = {"input": name, "nodes": nodes, "steps": steps, "paths": dev["paths"], "ref_len": dev["ref_len"], "anchors": dev["anchors"],
               "traversals": dev["traversals"], "sites": dev["sites"], "breaks": int(dev["breaks"].sum()), "skipped": int(dev["skipped"].sum()),
               "hash_collision_sites": dev["hash_collision_sites"], "device_us": dev_us, "twin_us": twin_us, "device_kernel_us": dev_k,
               "twin_kernel_us": twin_k, "stage_ratio": round(twin_us / max(dev_us, 1), 2), "wall_device_ms": round(dev_wall, 3),
               "wall_twin_ms": round(twin_wall, 3), "not_measured": "one wave per long allele in the hash group (not built); a look-back carry in the scans (not built)"}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if ns.out:
        with open(ns.out, "w") as fh:
            json.dump(rows, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
