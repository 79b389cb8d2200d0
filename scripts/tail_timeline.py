#!/usr/bin/env python3
"""Per-workgroup timeline of one C2 step of the blocked alignment kernel: how many workgroups of the main
launch are alive over time, and what the last ones to exit were doing.

Runs under SR_PROFILE_TICKS=1 (the instrumented instance writes, per workgroup, the 100 MHz ticks of its first dequeue, of
the start of its last alignment and of its exit, and how many alignments it ran).  SR_TAIL=0 in the environment gives the
timeline without the tail launch, SR_TAIL unset the one with it:

    SR_TAIL=0 python scripts/tail_timeline.py > profiles/tail_timeline_before.log
    python scripts/tail_timeline.py > profiles/tail_timeline_after.log

The instrumented instance is about 10 % slower than the production one; the two logs compare like with like."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TICKS_PER_MS = 100e6 / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseq", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    os.environ["SR_PROFILE_TICKS"] = "1"
    import bench
    from seqrush_amd.seqrush import SeqSet, Params, Context

    recs, spars, workload, _ = bench.build_config("C2", args.nseq, None)
    ctx = Context(0)
    ctx.load(SeqSet(recs), Params(sparsification=spars))
    rep = ctx.workspace_report()
    for _ in range(args.warmup + 1):
        ctx.reset_uf(); ctx.run(); ctx.sync()
    ms, cnt, deferred = ctx.kernel_ms(0), ctx.counters(), ctx.tail_deferred()
    tl = ctx.tail_timeline().astype(np.int64)
    ctx.close()
    print(f"# {workload}")
    print(f"# knobs {rep['knobs']} | workgroups {rep['workgroups']} x {rep['threads_per_workgroup']} threads | tail_threads "
          f"{rep['tail_threads']} | mirror_partners {rep['mirror_partners']} | build {rep['kernel_build']} {rep['source_digest']}")
    print(f"# alignment kernels (main + tail launch, instrumented instance): {ms:.2f} ms | mirror_pairs {cnt['mirror_pairs']} "
          f"mirror_ties {cnt['mirror_ties']} deferred to the tail launch {deferred}")
    if len(tl) == 0 or not tl[:, 2].any():
        print("no timeline: the load did not run the instrumented instance")
        return 1
    tl = tl[tl[:, 2] > 0]
    t0 = tl[:, 0].min()
    first, last, end = ((tl[:, k] - t0) / TICKS_PER_MS for k in range(3))
    n, own = tl[:, 3] & 0xffffffff, (tl[:, 3] >> 32) & 1
    span = end.max()
    print(f"# main launch: first dequeue to last exit {span:.2f} ms; the rest of the {ms:.2f} ms is launch latency and the tail launch")
    print("# workgroups alive (dequeued, not yet exited) at the start of each 1 ms bin, and those running their last alignment")
    print("ms\talive\tin_last_alignment\tof_those_own_secondary")
    for b in range(int(np.ceil(span)) + 1):
        alive = (first <= b) & (end > b)
        inlast = alive & (last <= b) & (n > 0)
        print(f"{b}\t{int(alive.sum())}\t{int(inlast.sum())}\t{int((inlast & (own == 1)).sum())}")
    print("# alignments per workgroup: " + ", ".join(f"{k}: {int((n == k).sum())}" for k in sorted(set(n.tolist()))))
    print("# the last 16 workgroups to exit")
    print("workgroup\texit_ms\talignments\tlast_was_own_tied_secondary\tlast_alignment_ms")
    for i in np.argsort(end)[-16:]:
        print(f"{i}\t{end[i]:.2f}\t{n[i]}\t{own[i]}\t{end[i] - last[i]:.2f}")
    half = span - np.sort(end)[max(0, len(end) - 1 - len(end) // 100)]
    print(f"# the last 1 % of the workgroups exit over the final {half:.2f} ms of the main launch")
    return 0


if __name__ == "__main__":
    sys.exit(main())
