"""`python -m seqrush_amd` -- thin CLI with the reference's flag surface for the hot path
(src/seqrush.rs:17-152, src/main.rs:4-7).  Everything that computes runs on the GPU."""
import argparse
import os
import subprocess
import sys

from .seqrush import Args, run_seqrush, run_seqrush_rank, check_inversion_join
from ._lib import SeqRushError


def main(argv=None):
    ap = argparse.ArgumentParser(prog="seqrush", description="MI355X-native seqrush hot path")
    ap.add_argument("-s", "--sequences", required=True)
    ap.add_argument("-o", "--output", default="output.gfa")
    ap.add_argument("-k", "--min-match-length", type=int, default=0)
    ap.add_argument("-t", "--threads", type=int, default=4)
    ap.add_argument("-S", "--scores", default="0,5,8,2,24,1")
    ap.add_argument("--orientation-scores", default="0,1,1,1")
    ap.add_argument("-d", "--max-divergence", type=float, default=None)
    ap.add_argument("-x", "--sparsify", dest="sparsification", default="none")
    ap.add_argument("-p", "--paf", default=None)
    ap.add_argument("--output-alignments", default=None)
    ap.add_argument("--no-compact", action="store_true")
    ap.add_argument("--compact-on", choices=("host", "device"), default="host",
                    help="where compaction + renumbering run: the host procedure, or per-handle tables on the GPU (same bytes)")
    ap.add_argument("--no-sort", action="store_true")
    ap.add_argument("--sort", action="store_true",
                    help="Ygs layout: path-guided SGD on the GPU (reproducible), grooming, topological sort")
    ap.add_argument("--sort-seed", type=int, default=9399220)
    ap.add_argument("--sgd-iter-max", type=int, default=100)
    ap.add_argument("--skip-sgd", action="store_true")
    ap.add_argument("--skip-groom", action="store_true")
    ap.add_argument("--skip-topo", action="store_true")
    ap.add_argument("--aligner", default="allwave")
    ap.add_argument("--iterative", action="store_true",
                    help="tree pairs first, then random pairs in chunks of 10 until 10 component counts in a row are unchanged")
    ap.add_argument("--patch-inversions", action="store_true",
                    help="realign large two-sided CIGAR gaps with the query segment reverse-complemented and unite the good ones")
    ap.add_argument("--inversion-min-size", type=int, default=0, help="gap threshold of --patch-inversions (0 = 2 * -k)")
    ap.add_argument("--inversion-join", type=int, default=0,
                    help="with --patch-inversions: join gaps across match islands shorter than N and accept a patch against "
                         "what the main alignment paid for the gap (0 = off; N <= -k is the sensible range)")
    ap.add_argument("--stats", default=None, metavar="FILE",
                    help="write the statistics report of the final GFA (summary, depth, path similarity, layout error) to FILE")
    ap.add_argument("--layout", default=None, metavar="FILE",
                    help="write the 2-D path-guided SGD layout of the final GFA (two end points per node) to FILE as TSV")
    ap.add_argument("--layout-svg", default=None, metavar="FILE", help="draw the same layout to FILE as SVG")
    ap.add_argument("--layout-seed", type=int, default=9399220)
    ap.add_argument("--layout-iter-max", type=int, default=30)
    ap.add_argument("--bin", default=None, metavar="FILE",
                    help="write the path-by-bin coverage table of the final GFA (what `odgi bin` writes) to FILE as TSV")
    ap.add_argument("--bin-width", type=int, default=None, metavar="W", help="bin width of --bin in bp")
    ap.add_argument("--bin-count", type=int, default=None, metavar="N", help="number of bins of --bin (default 1500)")
    ap.add_argument("--viz", default=None, metavar="FILE.png",
                    help="draw the paths of the final GFA over bins of its sequence (what `odgi viz` draws) to FILE.png")
    ap.add_argument("--viz-width", type=int, default=None, metavar="N", help="bins = pixels across (default 1500)")
    ap.add_argument("--viz-path-height", type=int, default=None, metavar="H", help="rows per path (default 10)")
    ap.add_argument("--viz-path-gap", type=int, default=None, metavar="G", help="white rows between paths (default 1)")
    ap.add_argument("--viz-mode", choices=("path", "strand", "depth"), default=None,
                    help="path: coverage in the path's colour; strand: reverse bins red; depth: grey by mean coverage")
    ap.add_argument("--viz-depth-max", type=int, default=None, metavar="D", help="depth mode: the mean coverage drawn black (default 4)")
    ap.add_argument("--growth", default=None, metavar="FILE",
                    help="write the pangenome growth curves of the final GFA (`odgi heaps`, `panacus histgrowth`) to FILE as TSV")
    ap.add_argument("--growth-permutations", type=int, default=None, metavar="N", help="orders of the groups sampled (default 1000)")
    ap.add_argument("--growth-seed", type=int, default=None, metavar="N", help="seed of the sampled orders (default 9399220)")
    ap.add_argument("--growth-group-by", choices=("path", "sample", "haplotype"), default=None,
                    help="path: every path a genome; sample / haplotype: paths grouped by their PanSN prefix")
    ap.add_argument("--vcf", default=None, metavar="FILE",
                    help="write the variant sites of the final GFA against one of its paths (`vg deconstruct`) to FILE as VCF")
    ap.add_argument("--vcf-ref", default=None, metavar="NAME", help="the reference path (default: the first path)")
    ap.add_argument("--vcf-max-allele-len", type=int, default=None, metavar="N",
                    help="traversals with a longer allele or reference span are skipped (default 10000; 0: no limit)")
    ap.add_argument("--lift", default=None, metavar="IN.bed",
                    help="project the BED intervals of paths of the final GFA onto its other paths (`odgi position`); needs --lift-out")
    ap.add_argument("--lift-out", default=None, metavar="FILE", help="the lifted intervals, as BED")
    ap.add_argument("--lift-to", default=None, metavar="NAME", help="the one target path (default: every other path)")
    ap.add_argument("--lift-min-covered", type=int, default=None, metavar="N",
                    help="leave out targets with fewer than N lifted bases (default 1)")
    ap.add_argument("--extract-region", action="append", default=None, metavar="REGION",
                    help="cut the subgraph of NAME or NAME:START-END of a path out of the final GFA (`odgi extract`; repeatable); needs --extract-out")
    ap.add_argument("--extract-bed", default=None, metavar="FILE", help="regions to extract, as BED lines")
    ap.add_argument("--extract-out", default=None, metavar="FILE", help="the extracted graph, as GFA")
    ap.add_argument("--extract-context-steps", type=int, default=None, metavar="N", help="grow the regions' nodes by N L lines (default 0)")
    ap.add_argument("--extract-merge-distance", type=int, default=None, metavar="N",
                    help="close a gap of at most N bases between two kept steps of a path (default 100000)")
    ap.add_argument("--extract-merge-rounds", type=int, default=None, metavar="N", help="rounds of gap closing (default 3)")
    ap.add_argument("--extend", default=None, metavar="FILE.gfa",
                    help="add the sequences of -s to this graph: its paths are kept as they are and only the pairs that touch a "
                         "new sequence are aligned")
    ap.add_argument("-v", "--verbose", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--gpus", type=int, default=1,
                    help="GPUs of this node: the pair list is sharded, one process per GPU (torch.distributed.run, RCCL)")
    ns = ap.parse_args(argv)
    if ns.sort and ns.no_sort:
        print("Error: --sort and --no-sort exclude each other", file=sys.stderr)
        return 1
    if ns.compact_on == "device" and ns.no_compact:
        print("Error: --compact-on device and --no-compact exclude each other", file=sys.stderr)
        return 1
    # the rules of seqrush_mi355x: an option of --bin / --viz needs its flag, and a given value is a positive integer
    # (--viz-path-gap: non-negative)
    given = {f: getattr(ns, f.lstrip("-").replace("-", "_")) for f in
             ("--bin-width", "--bin-count", "--viz-width", "--viz-path-height", "--viz-path-gap", "--viz-mode", "--viz-depth-max")}
    for flag, v in given.items():
        if v is None:
            continue
        owner = flag[:5]
        if getattr(ns, owner[2:]) is None:
            print(f"Error: {flag} is an option of {owner}: give both", file=sys.stderr)
            return 1
        low = 0 if flag == "--viz-path-gap" else 1
        if flag != "--viz-mode" and not low <= v <= (0xffffffff if owner == "--viz" else 2 ** 64 - 1):
            print(f"Error: {flag} needs a {'non-negative' if low == 0 else 'positive'} integer, got '{v}'", file=sys.stderr)
            return 1
    for flag in ("--growth-permutations", "--growth-seed", "--growth-group-by"):
        v = getattr(ns, flag.lstrip("-").replace("-", "_"))
        if v is None:
            continue
        if ns.growth is None:
            print(f"Error: {flag} is an option of --growth: give both", file=sys.stderr)
            return 1
        low = 0 if flag == "--growth-seed" else 1
        if flag != "--growth-group-by" and not low <= v <= 2 ** 64 - 1:
            print(f"Error: {flag} needs a {'non-negative' if low == 0 else 'positive'} integer, got '{v}'", file=sys.stderr)
            return 1
    for flag in ("--vcf-ref", "--vcf-max-allele-len"):
        v = getattr(ns, flag.lstrip("-").replace("-", "_"))
        if v is None:
            continue
        if ns.vcf is None:
            print(f"Error: {flag} is an option of --vcf: give both", file=sys.stderr)
            return 1
        if flag == "--vcf-max-allele-len" and not 0 <= v <= 2 ** 64 - 1:
            print(f"Error: {flag} needs a non-negative integer, got '{v}'", file=sys.stderr)
            return 1
    if ns.lift is not None and ns.lift_out is None:
        print("Error: --lift needs --lift-out FILE: the lifted intervals have nowhere to go", file=sys.stderr)
        return 1
    for flag in ("--lift-out", "--lift-to", "--lift-min-covered"):
        v = getattr(ns, flag.lstrip("-").replace("-", "_"))
        if v is None:
            continue
        if ns.lift is None:
            print(f"Error: {flag} is an option of --lift: give both", file=sys.stderr)
            return 1
        if flag == "--lift-min-covered" and not 0 <= v <= 2 ** 64 - 1:
            print(f"Error: {flag} needs a non-negative integer, got '{v}'", file=sys.stderr)
            return 1
    asked = ns.extract_region is not None or ns.extract_bed is not None
    if asked and ns.extract_out is None:
        print("Error: --extract-region / --extract-bed need --extract-out FILE: the extracted graph has nowhere to go", file=sys.stderr)
        return 1
    if ns.extract_out is not None and not asked:
        print("Error: --extract-out needs --extract-region REGION or --extract-bed FILE: there is nothing to extract", file=sys.stderr)
        return 1
    for flag in ("--extract-context-steps", "--extract-merge-distance", "--extract-merge-rounds"):
        v = getattr(ns, flag.lstrip("-").replace("-", "_"))
        if v is None:
            continue
        if not asked:
            print(f"Error: {flag} is an option of --extract-region / --extract-bed: give both", file=sys.stderr)
            return 1
        if not 0 <= v <= 2 ** 64 - 1:
            print(f"Error: {flag} needs a non-negative integer, got '{v}'", file=sys.stderr)
            return 1
    if ns.bin_width is not None and ns.bin_count is not None:
        print("Error: --bin-width and --bin-count exclude each other", file=sys.stderr)
        return 1
    if ns.iterative and (ns.paf is not None or ns.gpus > 1):
        # before any rank starts: the stop rule is global and sequential, and -p has no alignment stage to stop
        print(f"Error: --iterative cannot be combined with {'-p' if ns.paf is not None else '--gpus N > 1'}", file=sys.stderr)
        return 1
    if ns.patch_inversions and (ns.iterative or ns.paf is not None):
        print(f"Error: --patch-inversions cannot be combined with {'--iterative' if ns.iterative else '-p'}", file=sys.stderr)
        return 1
    if ns.patch_inversions and (ns.inversion_min_size or 2 * ns.min_match_length) <= 0:
        print("Error: --patch-inversions needs -k or --inversion-min-size (a threshold of 0 would call every complementary "
              "SNP an inversion)", file=sys.stderr)
        return 1
    try:
        check_inversion_join(ns)
    except SeqRushError as e:
        print(f"Error: {e}", file=sys.stderr)
        return 1
    if ns.extend is not None:
        # before any device work: each of these would compose in principle, none is verified
        for on, what in ((ns.iterative, "--iterative"), (ns.paf is not None, "-p"), (ns.patch_inversions, "--patch-inversions"),
                         (ns.gpus > 1, "--gpus N > 1")):
            if on:
                print(f"Error: --extend cannot be combined with {what}", file=sys.stderr)
                return 1
    if ns.gpus > 1 and "RANK" not in os.environ:
        # start one process per GPU BEFORE anything here touches the GPU (never exec from a process that has)
        port = os.environ.get("MASTER_PORT", str(29400 + os.getpid() % 2000))
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ns.gpus),
               "--master-addr", "127.0.0.1", "--master-port", port, "-m", "seqrush_amd"] + list(argv if argv is not None else sys.argv[1:])
        env = dict(os.environ)
        env["PYTHONPATH"] = os.path.dirname(os.path.dirname(os.path.abspath(__file__))) + os.pathsep + env.get("PYTHONPATH", "")
        return subprocess.call(cmd, env=env)
    args = Args(sequences=ns.sequences, output=ns.output, min_match_length=ns.min_match_length,
                threads=ns.threads, scores=ns.scores, orientation_scores=ns.orientation_scores,
                max_divergence=ns.max_divergence, sparsification=ns.sparsification, paf=ns.paf,
                output_alignments=ns.output_alignments, no_compact=ns.no_compact, compact_on=ns.compact_on, no_sort=ns.no_sort,
                sort=ns.sort, sort_seed=ns.sort_seed, sgd_iter_max=ns.sgd_iter_max, skip_sgd=ns.skip_sgd,
                skip_groom=ns.skip_groom, skip_topo=ns.skip_topo,
                aligner=ns.aligner, verbose=ns.verbose, device=ns.device, gpus=ns.gpus, iterative=ns.iterative,
                patch_inversions=ns.patch_inversions, inversion_min_size=ns.inversion_min_size,
                inversion_join=ns.inversion_join, stats=ns.stats, layout=ns.layout, layout_svg=ns.layout_svg,
                layout_seed=ns.layout_seed, layout_iter_max=ns.layout_iter_max, bin=ns.bin, bin_width=ns.bin_width or 0,
                bin_count=ns.bin_count or 0, viz=ns.viz, viz_width=ns.viz_width or 1500,
                viz_path_height=ns.viz_path_height or 10, viz_path_gap=1 if ns.viz_path_gap is None else ns.viz_path_gap,
                viz_mode=ns.viz_mode or "path", viz_depth_max=ns.viz_depth_max or 4, growth=ns.growth,
                growth_permutations=ns.growth_permutations or 1000,
                growth_seed=9399220 if ns.growth_seed is None else ns.growth_seed, growth_group_by=ns.growth_group_by or "path", vcf=ns.vcf, vcf_ref=ns.vcf_ref,
                vcf_max_allele_len=10000 if ns.vcf_max_allele_len is None else ns.vcf_max_allele_len, extend=ns.extend,
                lift=ns.lift, lift_out=ns.lift_out, lift_to=ns.lift_to, lift_min_covered=1 if ns.lift_min_covered is None else ns.lift_min_covered,
                extract_regions=tuple(ns.extract_region or ()), extract_bed=ns.extract_bed, extract_out=ns.extract_out,
                extract_context_steps=ns.extract_context_steps or 0,
                extract_merge_distance=100000 if ns.extract_merge_distance is None else ns.extract_merge_distance,
                extract_merge_rounds=3 if ns.extract_merge_rounds is None else ns.extract_merge_rounds)
    try:
        if ns.gpus > 1:
            if int(os.environ.get("WORLD_SIZE", "1")) != ns.gpus:
                raise ValueError(f"--gpus {ns.gpus} but WORLD_SIZE={os.environ.get('WORLD_SIZE')}")
            run_seqrush_rank(args)
        else:
            run_seqrush(args)
    except (SeqRushError, ValueError) as e:
        print(f"Error: {e}", file=sys.stderr)
        if ns.gpus > 1:
            _leave_ranks()
        return 1
    except BaseException:
        if ns.gpus > 1:                 # any other failure of a rank: the same quick exit
            import traceback
            traceback.print_exc()
            _leave_ranks()
        raise
    return 0


def _leave_ranks():
    """A rank that failed (load error, device fault bits from ctx.sync()) leaves at once with a non-zero code instead of
    finalising the interpreter with a live process group: the other ranks may already sit in the label all-gather or a
    barrier, and torch.distributed.run ends them as soon as one worker has failed -- not after the RCCL timeout."""
    sys.stderr.flush(); sys.stdout.flush()
    os._exit(1)


if __name__ == "__main__":
    sys.exit(main())
