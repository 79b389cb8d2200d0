"""`python -m seqrush_amd.viz graph.gfa [-o out.png] [--tsv out.tsv] [--device N|-1]` -- the path-by-bin coverage (DESIGN.md
section 13) of any GFA with S / L / P lines and numeric node ids: the table `odgi bin` writes as TSV, the picture `odgi viz`
draws as PNG."""
import argparse
import sys

from ._lib import SeqRushError
from .seqrush import PathBins, VIZ_MODES


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m seqrush_amd.viz", description="paths over bins of a GFA's sequence")
    ap.add_argument("gfa")
    ap.add_argument("-o", "--output", default=None, metavar="FILE.png", help="the picture")
    ap.add_argument("--tsv", default=None, metavar="FILE", help="the table")
    ap.add_argument("--device", type=int, default=0, help="HIP device ordinal; -1 = the host twin (same integers)")
    ap.add_argument("--bin-width", type=int, default=0, metavar="W", help="bin width in bp")
    ap.add_argument("--bin-count", "--viz-width", dest="bin_count", type=int, default=0, metavar="N",
                    help="number of bins = pixels across (default 1500)")
    ap.add_argument("--viz-path-height", type=int, default=10, metavar="H")
    ap.add_argument("--viz-path-gap", type=int, default=1, metavar="G")
    ap.add_argument("--viz-mode", choices=VIZ_MODES, default="path")
    ap.add_argument("--viz-depth-max", type=int, default=4, metavar="D")
    ns = ap.parse_args(argv)
    if ns.bin_width and ns.bin_count:
        print("Error: --bin-width and --bin-count exclude each other", file=sys.stderr)
        return 1
    if not ns.output and not ns.tsv:
        print("Error: give -o FILE.png, --tsv FILE or both", file=sys.stderr)
        return 1
    try:
        with open(ns.gfa) as fh:
            text = fh.read()
        kw = dict(bin_width=ns.bin_width) if ns.bin_width else dict(bins=ns.bin_count or 1500)
        with PathBins(text, ns.device, **kw) as pb:
            if ns.tsv:
                with open(ns.tsv, "w") as fh:
                    fh.write(pb.tsv())
            if ns.output:
                data = pb.png(mode=ns.viz_mode, path_height=ns.viz_path_height, path_gap=ns.viz_path_gap,
                              depth_max=ns.viz_depth_max)
                with open(ns.output, "wb") as fh:
                    fh.write(data)
    except (SeqRushError, OSError) as e:
        print(f"Error: {e}", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
