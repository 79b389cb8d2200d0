"""`python -m seqrush_amd.extract graph.gfa [-r REGION]... [-b in.bed] [-o sub.gfa] [--context-steps N] [--merge-distance N]
[--merge-rounds N] [--device N|-1]` -- the subgraph of regions of paths of any GFA with S / L / P lines and numeric node ids
(DESIGN.md section 19): the graph of one locus alone, with every path's allele through it, as GFA for every other tool."""
import argparse
import sys

from ._lib import SeqRushError
from .seqrush import Extract


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m seqrush_amd.extract", description="cut the subgraph of path intervals out of a GFA")
    ap.add_argument("gfa")
    ap.add_argument("-r", "--region", action="append", default=[], metavar="REGION", help="NAME or NAME:START-END, 0-based, half-open (repeatable)")
    ap.add_argument("-b", "--bed", default=None, metavar="IN.bed", help="regions as BED lines: name start end")
    ap.add_argument("-o", "--output", default=None, metavar="FILE", help="the extracted graph (default: standard output)")
    ap.add_argument("--context-steps", type=int, default=0, metavar="N", help="grow the regions' nodes by N L lines")
    ap.add_argument("--merge-distance", type=int, default=100000, metavar="N", help="close a gap of at most N bases between two kept steps of a path")
    ap.add_argument("--merge-rounds", type=int, default=3, metavar="N", help="rounds of gap closing")
    ap.add_argument("--device", type=int, default=0, help="HIP device ordinal; -1 = the host twin (same bytes)")
    ns = ap.parse_args(argv)
    try:
        with open(ns.gfa) as fh:
            text = fh.read()
        bed = None
        if ns.bed is not None:
            with open(ns.bed) as fh:
                bed = fh.read()
        with Extract(text, tuple(ns.region), bed, ns.device, ns.context_steps, ns.merge_distance, ns.merge_rounds) as v:
            out = v.gfa()
        if ns.output:
            with open(ns.output, "w") as fh:
                fh.write(out)
        else:
            sys.stdout.write(out)
    except (SeqRushError, OSError) as e:
        print(f"Error: {e}", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
