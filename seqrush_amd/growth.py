"""`python -m seqrush_amd.growth graph.gfa [-o out.tsv] [--device N|-1] [--permutations N] [--seed N] [--group-by ...]` -- the
pangenome growth curves of any GFA with S / L / P lines and numeric node ids: how the pangenome and
the core grow as genomes are added, over sampled (or, for up to 8 groups, all) orders, with the closed-form expectation and
a Heaps' law fit."""
import argparse
import sys

from ._lib import SeqRushError
from .seqrush import Growth, GROWTH_GROUP_BY


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m seqrush_amd.growth", description="pangenome growth curves of a GFA")
    ap.add_argument("gfa")
    ap.add_argument("-o", "--output", default=None, metavar="FILE", help="the report (default: standard output)")
    ap.add_argument("--device", type=int, default=0, help="HIP device ordinal; -1 = the host twin (same integers)")
    ap.add_argument("--permutations", type=int, default=1000, metavar="N")
    ap.add_argument("--seed", type=int, default=9399220, metavar="N")
    ap.add_argument("--group-by", choices=GROWTH_GROUP_BY, default="path")
    ns = ap.parse_args(argv)
    try:
        with open(ns.gfa) as fh:
            text = fh.read()
        with Growth(text, ns.device, ns.group_by, ns.permutations, ns.seed) as g:
            report = g.report()
        if ns.output:
            with open(ns.output, "w") as fh:
                fh.write(report)
        else:
            sys.stdout.write(report)
    except (SeqRushError, OSError) as e:
        print(f"Error: {e}", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
