#!/usr/bin/env python3
"""Per-workgroup timeline of one C2 step of the blocked alignment kernel: how many workgroups of the main
launch are alive over time, and what the last ones to exit were doing.

Runs under SR_PROFILE_TICKS=1 (the instrumented instance writes, per workgroup, the 100 MHz ticks of its first dequeue, of
the start of its last alignment and of its exit, and how many alignments it ran).  SR_TAIL=0 in the environment gives the
timeline without the tail launch, SR_TAIL unset the one with it:

    SR_TAIL=0 python scripts/tail_timeline.py > profiles/tail_timeline_before.log
    python scripts/tail_timeline.py > profiles/tail_timeline_after.log

It also prints who ends when by the workgroup's rank among the workgroups of its CU (the rotating tile priority, DESIGN.md 4.1;
SR_TILE_PRIO=0 is the scheduling before it: ranks are taken, every wave's tile code runs at priority 0):

    SR_TILE_PRIO=0 python scripts/tail_timeline.py > profiles/prio_timeline_before.log
    python scripts/tail_timeline.py > profiles/prio_timeline_after.log

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
    ptl = ctx.prio_timeline().astype(np.int64)
    ctx.close()
    print(f"# {workload}")
    print(f"# knobs {rep['knobs']} | workgroups {rep['workgroups']} x {rep['threads_per_workgroup']} threads | tail_threads "
          f"{rep['tail_threads']} | mirror_partners {rep['mirror_partners']} | build {rep['kernel_build']} {rep['source_digest']}")
    print(f"# alignment kernels (main + tail launch, instrumented instance): {ms:.2f} ms | mirror_pairs {cnt['mirror_pairs']} "
          f"mirror_ties {cnt['mirror_ties']} deferred to the tail launch {deferred}")
    if len(tl) == 0 or not tl[:, 2].any():
        print("no timeline: the load did not run the instrumented instance")
        return 1
    keep = tl[:, 2] > 0
    tl = tl[keep]
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
    if len(ptl) == len(keep) and keep.any():
        # who finishes when: by the rank among the workgroups of the CU (arrival order on the CU the hardware ids name,
        # sr_prio_rule.h) and, for comparison, by blockIdx / CUs (dispatch order only if the dispatcher goes round the CUs)
        ptl = ptl[keep]
        end1 = (ptl[:, 0] - t0) / TICKS_PER_MS
        rank, idx, arr = ptl[:, 1], ptl[:, 2], ptl[:, 3]
        wg_cu = int(rep["prio_workgroups_per_cu"])
        cus = max(1, int(rep["workgroups"]) // max(1, int(rep["workgroups_per_cu"])))
        wid = np.nonzero(keep)[0]
        per_cu = np.bincount(idx)
        print(f"# tile_prio {rep['tile_prio']} | prio_epoch_shift {rep['prio_epoch_shift']} | workgroups per CU of the rule {wg_cu} | "
              f"table entries used {int((per_cu > 0).sum())}, arrivals per entry min {int(per_cu[per_cu > 0].min())} max {int(per_cu.max())} "
              f"| ranks_taken {cnt['prio_ranks_taken']} max_cu_arrivals {cnt['prio_max_cu_arrivals']}")
        for name, key in (("rank on the CU", rank), ("blockIdx / CUs", wid // cus), ("blockIdx % 8", wid % 8)):
            print(f"# by {name}: workgroups, median / 10 % / 90 % end of the first alignment, median / max end of the last one (ms)")
            print("group\tworkgroups\tfirst_end_median\tfirst_end_p10\tfirst_end_p90\tlast_end_median\tlast_end_max")
            for g in sorted(set(key.tolist())):
                m = (key == g) & (n > 0)
                if not m.any():
                    continue
                print(f"{g}\t{int(m.sum())}\t{np.median(end1[m]):.2f}\t{np.percentile(end1[m], 10):.2f}\t"
                      f"{np.percentile(end1[m], 90):.2f}\t{np.median(end[m]):.2f}\t{end[m].max():.2f}")
        print("# rank against blockIdx / CUs (rows: rank, columns: blockIdx / CUs)")
        for g in sorted(set(rank.tolist())):
            print(f"{g}\t" + "\t".join(str(int(((rank == g) & (wid // cus == q)).sum())) for q in sorted(set((wid // cus).tolist()))))
        slow = np.argsort(end)[-16:]
        print("# the last 16 workgroups to exit: workgroup, rank, blockIdx / CUs")
        print("\t".join(f"{wid[i]}:{rank[i]}:{wid[i] // cus}" for i in slow))
    return 0


if __name__ == "__main__":
    sys.exit(main())
