"""`python -m seqrush_amd.lift graph.gfa -b in.bed [-o out.bed] [--to NAME] [--min-covered N] [--device N|-1]` -- the BED
intervals of paths of any GFA with S / L / P lines and numeric node ids, projected onto its other paths (DESIGN.md section
17): where a gene, exon or peak of one haplotype lies in every other one, as BED with the covered bases and the strand."""
import argparse
import sys

from ._lib import SeqRushError
from .seqrush import Lift


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m seqrush_amd.lift", description="project BED intervals of a path of a GFA onto its other paths")
    ap.add_argument("gfa")
    ap.add_argument("-b", "--bed", required=True, metavar="IN.bed", help="the intervals: name start end [label ...], 0-based, half-open")
    ap.add_argument("-o", "--output", default=None, metavar="FILE", help="the lifted intervals (default: standard output)")
    ap.add_argument("--to", default=None, metavar="NAME", help="the one target path (default: every other path)")
    ap.add_argument("--min-covered", type=int, default=1, metavar="N", help="leave out targets with fewer than N lifted bases")
    ap.add_argument("--device", type=int, default=0, help="HIP device ordinal; -1 = the host twin (same bytes)")
    ns = ap.parse_args(argv)
    try:
        with open(ns.gfa) as fh:
            text = fh.read()
        with open(ns.bed) as fh:
            bed = fh.read()
        with Lift(text, bed, ns.device, ns.to, ns.min_covered) as v:
            out = v.bed()
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
