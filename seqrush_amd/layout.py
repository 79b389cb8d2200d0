"""`python -m seqrush_amd.layout graph.gfa -o graph.lay.tsv [--svg graph.svg] [--device N|-1|-2] [--seed N] [--iter-max N]`
-- the 2-D path-guided SGD layout of any GFA with S / L / P lines and numeric node ids: two end
points per node as TSV, and the drawing as SVG."""
import argparse
import sys

from ._lib import SeqRushError
from .seqrush import layout_gfa, layout_svg, layout_tsv


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m seqrush_amd.layout", description="reproducible 2-D layout of a GFA")
    ap.add_argument("gfa")
    ap.add_argument("-o", "--output", required=True, help="TSV: idx, X, Y; rows 2v and 2v + 1 are the end points of the v-th node")
    ap.add_argument("--svg", default=None, help="also draw the layout to this file")
    ap.add_argument("--device", type=int, default=0,
                    help="HIP device ordinal; -1 = the host twin (same bits), -2 = the sequential yardstick")
    ap.add_argument("--seed", type=int, default=9399220)
    ap.add_argument("--iter-max", type=int, default=30)
    ns = ap.parse_args(argv)
    try:
        with open(ns.gfa) as fh:
            text = fh.read()
        xy = layout_gfa(text, seed=ns.seed, iter_max=ns.iter_max, device=ns.device)
        with open(ns.output, "w") as fh:
            fh.write(layout_tsv(xy))
        if ns.svg:
            with open(ns.svg, "w") as fh:
                fh.write(layout_svg(text, xy))
    except (SeqRushError, OSError) as e:
        print(f"Error: {e}", file=sys.stderr)
        return 1
    print(f"Layout written to {ns.output}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
