"""`python -m seqrush_amd.stats graph.gfa [--device N|-1]` -- the statistics report of any GFA with
S / L / P lines and numeric node ids: summary, depth, base pairs by path count, path similarity, layout error, topology."""
import argparse
import sys

from ._lib import SeqRushError
from .seqrush import graph_stats_report


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m seqrush_amd.stats", description="exact statistics of a GFA")
    ap.add_argument("gfa")
    ap.add_argument("--device", type=int, default=0, help="HIP device ordinal; -1 = the host twin (same integers)")
    ns = ap.parse_args(argv)
    try:
        with open(ns.gfa) as fh:
            text = fh.read()
        sys.stdout.write(graph_stats_report(text, ns.device))
    except (SeqRushError, OSError) as e:
        print(f"Error: {e}", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
