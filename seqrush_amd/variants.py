"""`python -m seqrush_amd.variants graph.gfa [-o out.vcf] [--ref NAME] [--device N|-1] [--max-allele-len N]` -- the variant
sites of any GFA with S / L / P lines and numeric node ids against one of its paths, as VCF: where
the other paths differ from it, and the allele every path carries at each site."""
import argparse
import sys

from ._lib import SeqRushError
from .seqrush import Variants


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m seqrush_amd.variants", description="variant sites of a GFA against one of its paths")
    ap.add_argument("gfa")
    ap.add_argument("-o", "--output", default=None, metavar="FILE", help="the VCF (default: standard output)")
    ap.add_argument("--ref", default=None, metavar="NAME", help="the reference path (default: the first path)")
    ap.add_argument("--device", type=int, default=0, help="HIP device ordinal; -1 = the host twin (same bytes)")
    ap.add_argument("--max-allele-len", type=int, default=10000, metavar="N", help="0: no limit")
    ns = ap.parse_args(argv)
    try:
        with open(ns.gfa) as fh:
            text = fh.read()
        with Variants(text, ns.device, ns.ref, ns.max_allele_len) as v:
            vcf = v.vcf()
        if ns.output:
            with open(ns.output, "w") as fh:
                fh.write(vcf)
        else:
            sys.stdout.write(vcf)
    except (SeqRushError, OSError) as e:
        print(f"Error: {e}", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
