"""Host-side mirror of the reference's production entry points for the hot path.

Reference (pangenome/seqrush): ``Args`` src/seqrush.rs:17-152, ``Sequence``
:272-277, ``load_sequences`` :1801-1837, ``SeqRush::new`` :308-336,
``build_graph`` :433-458, ``align_and_unite_with_allwave`` :611-757,
``run_seqrush`` :1839-1853.  Everything that computes calls the C ABI
(``include/seqrush_amd.h``); there is no Python or CPU alignment path.
"""
import ctypes as C
import dataclasses
from typing import List, Optional, Sequence as Seq

import numpy as np

from . import _lib
from ._lib import (ParamsC, SeqSetC, AlignmentsC, SortParamsC, IterStatsC, InvParamsC, InvStatsC, InvJobC, InvSiteC, GraphStatsC,
                   LayoutParamsC, BinParamsC, PathBinsC, VizParamsC, GrowthParamsC, GrowthC, VariantParamsC, VariantsC, ExtendStatsC, LiftParamsC, LiftC, ExtractParamsC, ExtractC, check,
                   SeqRushError)

SR_MEM_HIGH, SR_MEM_ULTRALOW = 0, 3


# --------------------------------------------------------------------------- args
@dataclasses.dataclass
class Args:
    """Flag surface of the reference CLI that the hot path reads (src/seqrush.rs:17-152)."""
    sequences: str = ""                     # -s
    output: str = "output.gfa"              # -o
    min_match_length: int = 0               # -k
    threads: int = 4                        # -t (host threads; the device path ignores it)
    scores: str = "0,5,8,2,24,1"            # -S
    orientation_scores: str = "0,1,1,1"     # --orientation-scores
    max_divergence: Optional[float] = None  # -d
    sparsification: str = "none"            # -x
    paf: Optional[str] = None               # -p: replay alignments from a PAF file instead of aligning
    output_alignments: Optional[str] = None  # --output-alignments
    no_compact: bool = False                # --no-compact (default: compact + renumber, bidirected_gfa_writer.rs:39-51)
    compact_on: str = "host"                # added: --compact-on host|device: where compaction + renumbering run
    no_sort: bool = True                    # --no-sort: the unsorted graph
    sort: bool = False                      # added: --sort, the Ygs layout (the reference's default); wins over no_sort
    sort_seed: int = 9399220                # added: --sort-seed, seed of the counter-based SGD draws
    sgd_iter_max: int = 100                 # --sgd-iter-max (the reference's hidden flag)
    skip_sgd: bool = False                  # --skip-sgd / --skip-groom / --skip-topo (src/seqrush.rs:90-99)
    skip_groom: bool = False
    skip_topo: bool = False
    aligner: str = "allwave"
    verbose: bool = False
    device: int = 0                         # added: HIP device ordinal
    shard_rank: int = 0                     # added: multi-GPU pair shard
    shard_count: int = 1
    gpus: int = 1                           # added: --gpus N, one process per GPU under torch.distributed.run
    iterative: bool = False                 # --iterative: tree pairs, then random pairs until the components are stable
    patch_inversions: bool = False          # added: --patch-inversions, realign large two-sided CIGAR gaps on the other strand
    inversion_min_size: int = 0             # added: --inversion-min-size N (0 = 2 * min_match_length)
    inversion_join: int = 0                 # added: --inversion-join J: join gaps across match islands shorter than J (0 = off)
    stats: Optional[str] = None             # added: --stats FILE: the statistics report of the final GFA
    layout: Optional[str] = None            # added: --layout FILE: 2-D layout of the final GFA as TSV
    layout_svg: Optional[str] = None        # added: --layout-svg FILE: the same layout drawn as SVG
    layout_seed: int = 9399220              # added: --layout-seed N
    layout_iter_max: int = 30               # added: --layout-iter-max N
    bin: Optional[str] = None               # added: --bin FILE: path-by-bin coverage of the final GFA as TSV
    bin_width: int = 0                      # added: --bin-width W | --bin-count N (neither: 1500 bins)
    bin_count: int = 0
    viz: Optional[str] = None               # added: --viz FILE.png: the same table drawn, --viz-width bins wide
    viz_width: int = 1500
    viz_path_height: int = 10
    viz_path_gap: int = 1
    viz_mode: str = "path"                  # path | strand | depth
    viz_depth_max: int = 4
    growth: Optional[str] = None            # added: --growth FILE: pangenome growth curves of the final GFA as TSV
    growth_permutations: int = 1000         # added: --growth-permutations N
    growth_seed: int = 9399220              # added: --growth-seed N
    growth_group_by: str = "path"           # added: --growth-group-by path | sample | haplotype
    vcf: Optional[str] = None               # added: --vcf FILE: variant sites of the final GFA against one path as VCF
    vcf_ref: Optional[str] = None           # added: --vcf-ref NAME: the reference path (default: the first)
    vcf_max_allele_len: int = 10000         # added: --vcf-max-allele-len N (0: no limit)
    lift: Optional[str] = None              # added: --lift IN.bed: intervals of paths of the final GFA to project onto its other paths
    lift_out: Optional[str] = None          # added: --lift-out FILE: where the lifted intervals go (required with --lift)
    lift_to: Optional[str] = None           # added: --lift-to NAME: the one target path (default: every path)
    lift_min_covered: int = 1               # added: --lift-min-covered N
    extract_regions: tuple = ()             # added: --extract-region REGION (repeatable): NAME or NAME:START-END of paths of the final GFA
    extract_bed: Optional[str] = None       # added: --extract-bed FILE: regions as BED lines
    extract_out: Optional[str] = None       # added: --extract-out FILE: where the extracted GFA goes (required with a region or a BED)
    extract_context_steps: int = 0          # added: --extract-context-steps N
    extract_merge_distance: int = 100000    # added: --extract-merge-distance N
    extract_merge_rounds: int = 3           # added: --extract-merge-rounds N
    extend: Optional[str] = None            # added: --extend FILE.gfa: add the sequences of -s to this graph


@dataclasses.dataclass
class AlignmentScores:
    """src/seqrush.rs:154-250"""
    match_score: int
    mismatch_penalty: int
    gap1_open: int
    gap1_extend: int
    gap2_open: Optional[int] = None
    gap2_extend: Optional[int] = None

    @staticmethod
    def parse(scores_str: str) -> "AlignmentScores":
        p = ParamsC()
        L = _lib.load()
        L.sr_default_params(C.byref(p))
        check(L.sr_parse_scores(scores_str.encode(), C.byref(p)))
        two = p.gap_open2 >= 0
        return AlignmentScores(p.match_score, p.mismatch_penalty, p.gap_open1, p.gap_ext1,
                               p.gap_open2 if two else None, p.gap_ext2 if two else None)

    @staticmethod
    def parse_orientation(scores_str: str) -> "AlignmentScores":
        p = ParamsC()
        L = _lib.load()
        L.sr_default_params(C.byref(p))
        check(L.sr_parse_orientation_scores(scores_str.encode(), C.byref(p)))
        return AlignmentScores(p.ori_match, p.ori_mismatch, p.ori_gap_open, p.ori_gap_ext)


@dataclasses.dataclass
class Sequence:
    """src/seqrush.rs:272-277"""
    id: str
    data: bytes
    offset: int = 0


def load_sequences(file_path: str) -> List[Sequence]:
    """FASTA loader with the reference's exact record rules (src/seqrush.rs:1801-1837):
    id = first whitespace token after '>', lines trimmed and concatenated verbatim,
    offset = running sum, records with an empty id are dropped."""
    sequences: List[Sequence] = []
    current_id = ""
    current = bytearray()
    offset = 0
    with open(file_path, "rb") as fh:
        text = fh.read()
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    ws = b" \t\n\r\x0b\x0c"
    for line in lines:
        if line.endswith(b"\r"):
            line = line[:-1]
        if line.startswith(b">"):
            if current_id:
                sequences.append(Sequence(current_id, bytes(current), offset))
                offset += len(current)
                current = bytearray()
            toks = line[1:].split()
            current_id = toks[0].decode() if toks else ""
        else:
            current.extend(line.strip(ws))
    if current_id:
        sequences.append(Sequence(current_id, bytes(current), offset))
    return sequences


# --------------------------------------------------------------------------- C ABI wrappers
class SeqSet:
    """Owns the buffers behind an ``sr_seqset``."""

    def __init__(self, records: Seq):
        """records: iterable of (name, bytes) or Sequence"""
        names, datas = [], []
        for r in records:
            if isinstance(r, Sequence):
                names.append(r.id); datas.append(bytes(r.data))
            else:
                names.append(r[0]); datas.append(bytes(r[1]))
        self.names = names
        self.lengths = [len(d) for d in datas]
        self._bases = b"".join(datas)
        self._offsets = np.zeros(len(datas) + 1, dtype=np.uint64)
        np.cumsum(self.lengths, out=self._offsets[1:])
        self._names_c = (C.c_char_p * max(1, len(names)))(*[n.encode() for n in names])
        self.c = SeqSetC(len(datas), self._bases, self._offsets.ctypes.data_as(C.POINTER(C.c_uint64)),
                         C.cast(self._names_c, C.POINTER(C.c_char_p)))

    @property
    def n(self):
        return len(self.names)

    @property
    def total_length(self):
        return int(self._offsets[-1])

    def offset(self, i):
        return int(self._offsets[i])

    def seq(self, i):
        return self._bases[int(self._offsets[i]): int(self._offsets[i + 1])]


class Params:
    """``sr_params`` with the reference defaults (src/seqrush.rs:33-75)."""

    def __init__(self, **kw):
        self.c = ParamsC()
        _lib.load().sr_default_params(C.byref(self.c))
        for k, v in kw.items():
            self.set(k, v)

    def set(self, k, v):
        if k == "scores":
            check(_lib.load().sr_parse_scores(v.encode(), C.byref(self.c)))
        elif k == "orientation_scores":
            check(_lib.load().sr_parse_orientation_scores(v.encode(), C.byref(self.c)))
        elif k == "sparsification":
            check(_lib.load().sr_parse_sparsification(v.encode(), C.byref(self.c)))
        elif k == "max_divergence":
            self.c.max_divergence = -1.0 if v is None else float(v)
        else:
            if not hasattr(self.c, k):
                raise AttributeError(k)
            setattr(self.c, k, v)

    @staticmethod
    def from_args(args: Args) -> "Params":
        p = Params(scores=args.scores, orientation_scores=args.orientation_scores,
                   sparsification=args.sparsification, max_divergence=args.max_divergence)
        p.c.min_match_len = args.min_match_length
        p.c.device = args.device
        p.c.shard_rank, p.c.shard_count = args.shard_rank, args.shard_count
        return p


class Alignments:
    """Owned ``sr_alignments`` (Seam 1 result)."""

    def __init__(self, ptr):
        self._p = ptr
        a = ptr.contents
        n = int(a.n)
        self.n = n

        def arr(p, dt, m):
            return np.ctypeslib.as_array(p, shape=(max(m, 1),))[:m].astype(dt, copy=True)
        self.query_idx = arr(a.query_idx, np.uint32, n)
        self.target_idx = arr(a.target_idx, np.uint32, n)
        self.is_reverse = arr(a.is_reverse, np.uint8, n)
        self.score = arr(a.score, np.int32, n)
        self.query_start = arr(a.query_start, np.uint64, n)
        self.query_end = arr(a.query_end, np.uint64, n)
        self.target_start = arr(a.target_start, np.uint64, n)
        self.target_end = arr(a.target_end, np.uint64, n)
        self.cigar_off = arr(a.cigar_off, np.uint64, n + 1)
        self.cigar_ops = arr(a.cigar_ops, np.uint32, int(self.cigar_off[-1]) if n else 0)

    def cigar(self, i: int) -> str:
        ops = self.cigar_ops[int(self.cigar_off[i]): int(self.cigar_off[i + 1])]
        return "".join(f"{int(o) >> 4}{'=XID'[int(o) & 3]}" for o in ops)

    def raw_cigar_bytes(self, i: int) -> bytes:
        """per-column raw WFA2 alphabet (M X I D), i.e. allwave's ``cigar_bytes``"""
        ops = self.cigar_ops[int(self.cigar_off[i]): int(self.cigar_off[i + 1])]
        tr = {0: b"M", 1: b"X", 2: b"D", 3: b"I"}   # undo the I<->D swap of src/wfa.rs:25-31
        return b"".join(tr[int(o) & 3] * (int(o) >> 4) for o in ops)

    def write_paf(self, seqset: SeqSet, path: str):
        check(_lib.load().sr_write_paf(self._p, C.byref(seqset.c), path.encode()))

    def append_paf(self, seqset: SeqSet, path: str, tag: Optional[str] = None):
        """append the records to `path`, each with one more tag column (e.g. "sr:Z:inv")"""
        check(_lib.load().sr_append_paf_tagged(self._p, C.byref(seqset.c), path.encode(), tag.encode() if tag else None))

    def close(self):
        if self._p:
            _lib.load().sr_alignments_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """Resident device context (``sr_ctx``): what ``bench.py`` times."""

    def __init__(self, device: int = 0):
        self.L = _lib.load()
        self._h = C.c_void_p()
        check(self.L.sr_ctx_create(device, C.byref(self._h)))
        self.seqset = None

    def set_stream(self, stream_ptr: int):
        check(self.L.sr_ctx_set_stream(self._h, C.c_void_p(stream_ptr)))

    def load(self, seqset: SeqSet, params: Params):
        self.seqset = seqset
        check(self.L.sr_ctx_load(self._h, C.byref(seqset.c), C.byref(params.c)))

    def load_pairs(self, seqset: SeqSet, params: Params, pairs):
        """explicit ordered (query, target) pair list instead of the all-vs-all enumeration"""
        self.seqset = seqset
        q = np.ascontiguousarray([a for a, _ in pairs], dtype=np.uint32)
        t = np.ascontiguousarray([b for _, b in pairs], dtype=np.uint32)
        check(self.L.sr_ctx_load_pairs(self._h, C.byref(seqset.c), C.byref(params.c),
                                       q.ctypes.data_as(C.POINTER(C.c_uint32)), t.ctypes.data_as(C.POINTER(C.c_uint32)),
                                       len(pairs)))

    def load_extend(self, plan: "ExtendPlan", params: Params):
        """--extend: the plan's merged set with only the pairs that touch a new sequence, and the union-find seeded with the
        partition the input graph stands for (enqueued; reset_uf() on such a context means init + seed)"""
        self.seqset = plan.seqset
        check(self.L.sr_ctx_load_extend(self._h, plan._h, C.byref(params.c)))

    def extend_stats(self) -> dict:
        """sr_extend_stats of the loaded extend context (syncs the stream)"""
        st = ExtendStatsC()
        check(self.L.sr_ctx_extend_stats(self._h, C.byref(st)))
        return {f: int(getattr(st, f)) for f, _ in ExtendStatsC._fields_}

    def pairs(self):
        """this rank's (query, target) pair list after sparsification and sharding"""
        q = C.POINTER(C.c_uint32)(); t = C.POINTER(C.c_uint32)(); cnt = C.c_uint64()
        check(self.L.sr_ctx_pairs(self._h, C.byref(q), C.byref(t), C.byref(cnt)))
        m = int(cnt.value)
        qa = np.ctypeslib.as_array(q, shape=(max(m, 1),))[:m].copy()
        ta = np.ctypeslib.as_array(t, shape=(max(m, 1),))[:m].copy()
        self.L.sr_free(C.cast(q, C.c_void_p)); self.L.sr_free(C.cast(t, C.c_void_p))
        return list(zip(qa.tolist(), ta.tolist()))

    @property
    def num_batches(self):
        return int(self.L.sr_ctx_num_batches(self._h))

    def workspace_report(self):
        import json
        return json.loads(self.L.sr_ctx_workspace_report(self._h).decode() or "{}")

    def run(self):
        """align + unite of the whole shard, batch after batch (PAF context: unite only)"""
        check(self.L.sr_ctx_run(self._h))

    def align_all(self, unite: bool = False) -> "Alignments":
        p = C.POINTER(AlignmentsC)()
        check(self.L.sr_ctx_align_all(self._h, 1 if unite else 0, C.byref(p)))
        return Alignments(p)

    def orientation_scores(self):
        """(forward, reverse-complement) orientation scores of the last alignment stage over this rank's pairs"""
        n = self.num_pairs
        fw = np.zeros(max(n, 1), dtype=np.int32); rv = np.zeros(max(n, 1), dtype=np.int32)
        check(self.L.sr_ctx_orientation_scores(self._h, fw.ctypes.data_as(C.POINTER(C.c_int32)), rv.ctypes.data_as(C.POINTER(C.c_int32))))
        return fw[:n], rv[:n]

    def pair_results(self):
        """(score, is_reverse, n_cigar_ops) arrays over this rank's pairs; resident for every batch"""
        n = self.num_pairs
        sc = np.zeros(max(n, 1), dtype=np.int32); rv = np.zeros(max(n, 1), dtype=np.uint8); co = np.zeros(max(n, 1), dtype=np.uint32)
        check(self.L.sr_ctx_pair_results(self._h, sc.ctypes.data_as(C.POINTER(C.c_int32)),
                                         rv.ctypes.data_as(C.POINTER(C.c_uint8)), co.ctypes.data_as(C.POINTER(C.c_uint32))))
        return sc[:n], rv[:n], co[:n]

    def load_iterative(self, seqset: SeqSet, params: Params, keep_alignments: bool = False):
        """--iterative: sequences + tree entries + random entries (a -x other than tree: becomes tree:3,3,0.1,16)"""
        self.seqset = seqset
        check(self.L.sr_ctx_load_iterative(self._h, C.byref(seqset.c), C.byref(params.c), 1 if keep_alignments else 0))

    def run_iterative(self):
        """phase 1 (every tree entry) and phase 2 (random entries in chunks of 10 until 10 checks saw no change)"""
        check(self.L.sr_ctx_run_iterative(self._h))

    def iterative_stats(self):
        """stats of the last iterative run -> dict (sr_iter_stats fields + check_counts: the per-check component counts)"""
        st = IterStatsC()
        check(self.L.sr_ctx_iterative_stats(self._h, C.byref(st), None, 0))
        cc = np.zeros(max(int(st.checks), 1), dtype=np.uint64)
        check(self.L.sr_ctx_iterative_stats(self._h, C.byref(st), cc.ctypes.data_as(C.POINTER(C.c_uint64)), int(st.checks)))
        d = {f: getattr(st, f) for f, _ in IterStatsC._fields_ if f != "reserved"}
        d["stabilized"], d["tree_defaulted"] = bool(d["stabilized"]), bool(d["tree_defaulted"])
        d["check_counts"] = [int(x) for x in cc[:int(st.checks)]]
        return d

    def iterative_alignments(self) -> "Alignments":
        """the processed alignments of the last iterative run, in processing order (load with keep_alignments=True)"""
        p = C.POINTER(AlignmentsC)()
        check(self.L.sr_ctx_iterative_alignments(self._h, C.byref(p)))
        return Alignments(p)

    def enable_inversions(self, min_size: int = 0, keep_alignments: bool = False, on: bool = True, join_below: int = 0):
        """--patch-inversions for the next run() / align_all(unite=True) of the loaded context (min_size 0 = 2 * -k);
        join_below = J of --inversion-join (0 = the plain rule)"""
        if not on:
            check(self.L.sr_ctx_enable_inversions(self._h, None))
            return
        if not 0 <= int(join_below) < 2 ** 32:
            raise SeqRushError(-1, f"inversion join length out of range: {join_below}")
        ip = InvParamsC(int(min_size), 1 if keep_alignments else 0, int(join_below))
        check(self.L.sr_ctx_enable_inversions(self._h, C.byref(ip)))

    def inversion_stats(self):
        """sr_inv_stats of the last run -> dict"""
        st = InvStatsC()
        check(self.L.sr_ctx_inversion_stats(self._h, C.byref(st)))
        return {f: getattr(st, f) for f, _ in InvStatsC._fields_}

    def inversion_join_stats(self):
        """sr_ctx_inversion_join_stats of the last run -> dict"""
        out = (C.c_uint64 * 4)()
        check(self.L.sr_ctx_inversion_join_stats(self._h, out))
        return dict(islands_absorbed=int(out[0]), rejected_site_cost=int(out[1]), host_us=int(out[2]))

    def inversion_jobs(self):
        """the jobs of the last run (pair order, then CIGAR order) -> list of dicts of the sr_inv_job fields"""
        p = C.POINTER(InvJobC)(); cnt = C.c_uint64()
        check(self.L.sr_ctx_inversion_jobs(self._h, C.byref(p), C.byref(cnt)))
        out = [{f: int(getattr(p[i], f)) for f, _ in InvJobC._fields_ if f != "reserved"} for i in range(cnt.value)]
        self.L.sr_free(C.cast(p, C.c_void_p))
        return out

    def inversion_alignments(self) -> "Alignments":
        """the accepted patches of the last run (enable with keep_alignments=True), forward-strand query coordinates"""
        p = C.POINTER(AlignmentsC)()
        check(self.L.sr_ctx_inversion_alignments(self._h, C.byref(p)))
        return Alignments(p)

    def load_paf(self, seqset: SeqSet, params: Params, paf_path: str):
        """`seqrush -p`: replay the records of a PAF file (then unite()); there is no alignment stage"""
        self.seqset = seqset
        check(self.L.sr_ctx_load_paf(self._h, C.byref(seqset.c), C.byref(params.c), paf_path.encode()))

    def build_gfa(self, compact: bool = False, sort: "Optional[SortParams]" = None, compact_on: str = "host"):
        """graph induction on the device from this context's union-find (+ compaction and
        renumbering, src/bidirected_gfa_writer.rs:39-51) + GFA text;
        -> (gfa_text, n_nodes, n_edges), byte-identical to build_gfa(seqset, download_labels(), compact).
        sort: SortParams -> the Ygs layout before the writer (src/bidirected_gfa_writer.rs:53-117)
        compact_on: "host" (sr_compact.cpp) or "device": compaction by tables on this context's device, straight from
        the induced arrays (sr_compact.hip; the same bytes; compact_stats() afterwards)"""
        mode = compact_mode(compact, compact_on)
        out = C.c_void_p(); nn = C.c_uint64(); ne = C.c_uint64()
        if sort is None:
            check(self.L.sr_ctx_build_gfa_opts(self._h, C.byref(self.seqset.c), mode, C.byref(out),
                                               C.byref(nn), C.byref(ne)))
        else:
            check(self.L.sr_ctx_build_gfa_sorted(self._h, C.byref(self.seqset.c), mode, C.byref(sort.c),
                                                 C.byref(out), C.byref(nn), C.byref(ne)))
        text = C.cast(out, C.c_char_p).value.decode()
        self.L.sr_free(out)
        return text, int(nn.value), int(ne.value)

    def reset_uf(self):
        check(self.L.sr_ctx_reset_uf(self._h))

    def align(self):
        check(self.L.sr_ctx_align(self._h))

    def unite(self):
        check(self.L.sr_ctx_unite(self._h))

    def sync(self):
        check(self.L.sr_ctx_sync(self._h))

    def alignments(self) -> Alignments:
        p = C.POINTER(AlignmentsC)()
        check(self.L.sr_ctx_alignments(self._h, C.byref(p)))
        return Alignments(p)

    @property
    def uf_size(self):
        return int(self.L.sr_ctx_uf_size(self._h))

    @property
    def num_pairs(self):
        return int(self.L.sr_ctx_num_pairs(self._h))

    @property
    def dp_cells(self):
        return int(self.L.sr_ctx_dp_cells(self._h))

    def download_uf(self) -> np.ndarray:
        out = np.zeros(self.uf_size, dtype=np.uint64)
        check(self.L.sr_ctx_download_uf(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out

    def download_labels(self) -> np.ndarray:
        out = np.zeros(self.uf_size, dtype=np.uint64)
        check(self.L.sr_ctx_download_labels(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out

    def labels_device(self, dev_ptr: int):
        check(self.L.sr_ctx_labels_device(self._h, C.c_void_p(dev_ptr)))

    def merge_labels(self, dev_ptr: int, count: int):
        check(self.L.sr_ctx_merge_labels(self._h, C.c_void_p(dev_ptr), count))

    def labels_device_u32(self, dev_ptr: int):
        check(self.L.sr_ctx_labels_device_u32(self._h, C.c_void_p(dev_ptr)))

    def merge_labels_u32(self, dev_ptr: int, count: int):
        check(self.L.sr_ctx_merge_labels_u32(self._h, C.c_void_p(dev_ptr), count))

    @property
    def align_kernel(self) -> str:
        n = self.L.sr_ctx_align_kernel(self._h)
        return n.decode() if n else ""

    def kernel_ms(self, which: int) -> float:
        ms = C.c_float()
        check(self.L.sr_ctx_kernel_ms(self._h, which, C.byref(ms)))
        return float(ms.value)

    def counters(self):
        """device counters of the last align / unite (include/seqrush_amd.h sr_ctx_counters_all): every name maps to ONE slot"""
        out = (C.c_uint64 * 54)()
        n = self.L.sr_ctx_counters_all(self._h, out, 54)
        if n < 0:
            check(n)
        return dict(row_bytes_loaded=int(out[16]), row_bytes_stored=int(out[17]), tk_recompute=int(out[18]),
                    wf_cells=int(out[0]), wf_steps=int(out[1]), base_segments=int(out[2]),
                    breakpoint_searches=int(out[3]), united_bases=int(out[4]), match_runs=int(out[5]),
                    ticks_orientation=int(out[6]), ticks_breakpoint=int(out[7]), ticks_base=int(out[8]),
                    bp_passes=int(out[9]), ticks_pair=int(out[10]), tk_pass=int(out[11]),
                    tk_barrier=int(out[12]), tk_setup_first=int(out[13]), tk_phase2=int(out[14]),
                    tk_tail=int(out[15]), bp_filter_units=int(out[19]), bp_candidates=int(out[20]),
                    bp_exact_units=int(out[21]), bp_rounds=int(out[22]), tk_backtrace=int(out[23]), tk_emit=int(out[24]),
                    tk_ctl_section=int(out[25]), tk_ctl_mak=int(out[26]), tk_ctl_segments=int(out[27]), tk_p2_list=int(out[28]),
                    tk_p2_filter=int(out[29]), tk_p2_exact=int(out[30]), tk_p2_replay=int(out[31]),
                    st_wait_cycles=int(out[32]), st_body_cycles=int(out[33]), st_tiles=int(out[34]), st_ext_iters=int(out[35]),
                    lds_row_bytes=int(out[36]), base_requeues=int(out[37]),
                    # blocked kernel: secondaries written as their primary's transposed CIGAR / aligned after all (a tie, a
                    # reverse strand or an error in the primary)
                    mirror_pairs=int(out[38]), mirror_ties=int(out[39]),
                    bounds_first=[int(out[40]), int(out[41]), int(out[42]), int(out[43])],
                    experiment=[int(out[44]), int(out[45]), int(out[46]), int(out[47])],
                    # blocked kernel: the base-case histories' share of row_bytes_*, base-case tiles and level-diagonals as executed
                    hist_bytes_loaded=int(out[44]), hist_bytes_stored=int(out[45]), base_tiles=int(out[46]),
                    base_level_diagonals=int(out[47]),
                    # replay of tied secondaries: tied primaries whose depth-0 search was tie-sensitive / whose
                    # ties all sit in base-case backtraces; secondaries that took breakpoints from their primary's records;
                    # searches they did not run
                    mirror_tie_top=int(out[48]), mirror_tie_base_only=int(out[49]), mirror_replays=int(out[50]),
                    replay_cached_searches=int(out[51]),
                    # rotating tile priority: workgroups of the main launches that took a rank on their CU, the
                    # largest arrival count of a CU in one launch
                    prio_ranks_taken=int(out[52]), prio_max_cu_arrivals=int(out[53]))

    def tail_deferred(self) -> int:
        """secondaries handed to the tail launch in the last pass (sr_ctx_tail_deferred; syncs)"""
        v = C.c_uint64()
        check(self.L.sr_ctx_tail_deferred(self._h, C.byref(v)))
        return int(v.value)

    def tail_timeline(self):
        """[workgroups, 4] uint64 of the instrumented instance's last main launch (sr_ctx_tail_timeline): ticks of the first
        dequeue, of the start of the last alignment, of the exit; alignments | last-was-own-secondary << 32"""
        cap = int(self.workspace_report().get("workgroups", 0))
        out = np.zeros((max(cap, 1), 4), dtype=np.uint64)
        n = self.L.sr_ctx_tail_timeline(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64)), cap)
        if n < 0:
            check(n)
        return out[:n]

    def prio_timeline(self):
        """[workgroups, 4] uint64, the second record of the same launch (sr_ctx_prio_timeline): tick of the end of the first
        alignment, rank among the workgroups of the CU, the CU's index in the arrival table, arrival count"""
        cap = int(self.workspace_report().get("workgroups", 0))
        out = np.zeros((max(cap, 1), 4), dtype=np.uint64)
        n = self.L.sr_ctx_prio_timeline(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64)), cap)
        if n < 0:
            check(n)
        return out[:n]

    def close(self):
        if self._h:
            self.L.sr_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SortParams:
    """``sr_sort_params``: the Ygs layout's settings (zero fields are derived from the graph, YgsParams::from_graph
    src/ygs_sort.rs:50-95); device >= 0: SGD on that GPU, -1: host twin (bit-identical), -2: sequential yardstick"""

    HOST_TWIN, SEQUENTIAL = -1, -2

    def __init__(self, **kw):
        self.c = SortParamsC()
        _lib.load().sr_sort_params_default(C.byref(self.c))
        for k, v in kw.items():
            if not hasattr(self.c, k):
                raise AttributeError(k)
            setattr(self.c, k, int(v) if isinstance(v, bool) else v)

    @staticmethod
    def from_args(args: Args) -> "SortParams":
        return SortParams(seed=args.sort_seed, iter_max=args.sgd_iter_max, skip_sgd=args.skip_sgd,
                          skip_groom=args.skip_groom, skip_topo=args.skip_topo, device=args.device)

    def as_dict(self):
        return {f: getattr(self.c, f) for f, _ in SortParamsC._fields_}


def _sort_params(params) -> SortParams:
    return params if isinstance(params, SortParams) else SortParams(**params)


def sort_gfa(text: str, **params) -> str:
    """the Ygs layout of any GFA with S / L / P lines and numeric node ids (the reference's sort_gfa binary);
    params: sr_sort_params fields (device=-1 for the host twin).  -> sorted GFA text"""
    L = _lib.load()
    sp = _sort_params(params)
    out = C.c_void_p(); nn = C.c_uint64(); ne = C.c_uint64()
    check(L.sr_sort_gfa(text.encode(), C.byref(sp.c), C.byref(out), C.byref(nn), C.byref(ne)))
    res = C.cast(out, C.c_char_p).value.decode()
    L.sr_free(out)
    return res


COMPACT_STATS = ("rounds", "host_rounds", "chains", "longest_list", "jumps", "compact_us", "copy_us", "reserved")


def compact_mode(compact: bool, compact_on: str) -> int:
    """the C ABI's `compact` argument: 0 none, 1 on the host, 2 on the context's device"""
    if compact_on not in ("host", "device"):
        raise SeqRushError(-1, f"compact_on must be 'host' or 'device', not {compact_on!r}")
    if compact_on == "device" and not compact:
        raise SeqRushError(-1, "--compact-on device and --no-compact exclude each other")
    return 0 if not compact else (2 if compact_on == "device" else 1)


def compact_gfa(text: str, device: int = -1, stats: Optional[dict] = None) -> str:
    """compact() + renumbering of any GFA with S / L / P lines and numeric node ids -> GFA text.  device: -1 the greedy
    host procedure (sr_compact.cpp), -2 the table formulation on the host, >= 0 the same in HIP on that device; all
    three return the same bytes.  stats: a dict that receives COMPACT_STATS"""
    L = _lib.load()
    out = C.c_void_p(); nn = C.c_uint64(); ne = C.c_uint64()
    st = (C.c_uint64 * 8)()
    check(L.sr_compact_gfa(text.encode(), device, C.byref(out), C.byref(nn), C.byref(ne), st))
    res = C.cast(out, C.c_char_p).value.decode()
    L.sr_free(out)
    if stats is not None:
        stats.update(zip(COMPACT_STATS, (int(v) for v in st)))
    return res


def compact_stats() -> dict:
    """COMPACT_STATS of this thread's last compaction by tables (compact_gfa, Context.build_gfa(compact_on="device"))"""
    st = (C.c_uint64 * 8)()
    check(_lib.load().sr_compact_stats(st))
    return dict(zip(COMPACT_STATS, (int(v) for v in st)))


SR_STATS_DEVICE_HOST = -1
STATS_KERNELS = ("steps", "nodes", "similarity", "layout", "topology")


class _GraphStats:
    """an owned sr_graph_stats"""

    def __init__(self, text: str, device: int):
        self.L = _lib.load()
        self.p = C.POINTER(GraphStatsC)()
        check(self.L.sr_graph_stats_gfa(text.encode(), int(device), C.byref(self.p)))

    def close(self):
        if self.p:
            self.L.sr_graph_stats_free(self.p)
            self.p = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def as_dict(self) -> dict:
        s = self.p.contents
        V, P = int(s.nodes), int(s.paths)

        def arr(ptr, n, dt):
            return np.ctypeslib.as_array(ptr, shape=(max(n, 1),))[:n].astype(dt, copy=True)

        def sq(parts):
            return (int(parts[0]) << 32) + (int(parts[1]) << 17) + int(parts[2])
        d = {k: int(getattr(s, k)) for k in ("length", "nodes", "edges", "paths", "steps", "rev_steps", "depth_bp", "self_loops",
                                             "tips", "components", "total_pairs", "total_abs", "total_len", "stats_us")}
        d["depth"], d["paths_on"] = arr(s.depth, V, np.uint32), arr(s.paths_on, V, np.uint32)
        d["bp_by_paths"], d["nodes_by_paths"] = arr(s.bp_by_paths, P + 1, np.uint64), arr(s.nodes_by_paths, P + 1, np.uint64)
        d["shared"] = arr(s.shared, P * P, np.uint64).reshape(P, P)
        d["path_pairs"], d["path_abs"], d["path_len"] = (arr(q, P, np.uint64) for q in (s.path_pairs, s.path_abs, s.path_len))
        d["path_sq_parts"] = arr(s.path_sq, 3 * P, np.uint64).reshape(P, 3)
        d["path_sq"] = [sq(row) for row in d["path_sq_parts"]]
        d["total_sq_parts"] = [int(v) for v in s.total_sq]
        d["total_sq"] = sq(s.total_sq)
        d["kernel_us"] = dict(zip(STATS_KERNELS, (int(v) for v in s.kernel_us)))
        return d

    def report(self, names) -> str:
        arr = (C.c_char_p * max(1, len(names)))(*[n.encode() for n in names])
        out = C.c_void_p()
        check(self.L.sr_graph_stats_report(self.p, C.cast(arr, C.POINTER(C.c_char_p)), C.byref(out)))
        res = C.cast(out, C.c_char_p).value.decode()
        self.L.sr_free(out)
        return res


def _path_names(text: str):
    """the names of the P lines the library's parser reads as paths, in order"""
    names = []
    for line in text.split("\n"):
        f = line.rstrip("\r").split("\t")
        if f[0][:1] == "P" and len(f) >= 3:
            names.append(f[1])
    return names


def graph_stats(text: str, device: int = 0) -> dict:
    """exact integer statistics of any GFA with S / L / P lines and numeric node ids.  device >= 0:
    HIP kernels on that device, -1: the host twin (the same integers).  -> dict: length, nodes, edges, paths, steps,
    rev_steps, depth_bp, self_loops, tips, components; depth / paths_on (per node, ascending id), bp_by_paths /
    nodes_by_paths (index = number of paths), shared (P x P shared base pairs), path_pairs / path_abs / path_len /
    path_sq (per path; path_sq as Python ints, path_sq_parts the three split sums), total_*; stats_us, kernel_us"""
    with _GraphStats(text, device) as gs:
        return gs.as_dict()


def _graph_stats_report(text: str, device: int):
    with _GraphStats(text, device) as gs:
        s = gs.p.contents
        return gs.report(_path_names(text)), dict(stats_us=int(s.stats_us))


def graph_stats_report(text: str, device: int = 0) -> str:
    """the TSV report of graph_stats(text, device), formatted by the library (the only place where a float is formed)"""
    return _graph_stats_report(text, device)[0]


def stats_sq_sums_host(values):
    """tests: the split sum of squares of values below 2^32 -> (sum a^2, sum a b, sum b^2) with e = a 2^16 + b"""
    a = np.ascontiguousarray(values, dtype=np.uint64)
    out = (C.c_uint64 * 3)()
    check(_lib.load().sr_stats_sq_sums_host(a.ctypes.data_as(C.POINTER(C.c_uint64)), len(a), out))
    return tuple(int(v) for v in out)


SR_BIN_DEVICE_HOST = -1
BIN_KERNELS = ("scan", "steps", "download")
VIZ_MODES = ("path", "strand", "depth")


def _viz_params(mode="path", path_height=10, path_gap=1, depth_max=4) -> VizParamsC:
    if mode not in VIZ_MODES:
        raise SeqRushError(-1, f"viz mode must be one of {', '.join(VIZ_MODES)}, not {mode!r}")
    for k, v in (("path_height", path_height), ("path_gap", path_gap), ("depth_max", depth_max)):
        if not 0 <= int(v) < 2 ** 32:
            raise SeqRushError(-1, f"viz {k} must be in 0 .. 2^32 - 1")
    return VizParamsC(VIZ_MODES.index(mode), int(path_height), int(path_gap), int(depth_max))


class PathBins:
    """an owned sr_path_bins: the path-by-bin tables of a GFA text and the outputs the library
    forms from them.  names default to the names of the text's P lines"""

    def __init__(self, text: str, device: int = 0, bin_width: int = 0, bins: int = 0):
        for k, v in (("bin_width", bin_width), ("bins", bins)):
            if not 0 <= int(v) < 2 ** 64:
                raise SeqRushError(-1, f"{k} must be in 0 .. 2^64 - 1")
        self.L = _lib.load()
        self.p = C.POINTER(PathBinsC)()
        self.names = _path_names(text)
        prm = BinParamsC(int(bin_width), int(bins))
        check(self.L.sr_path_bins_gfa(text.encode(), C.byref(prm), int(device), C.byref(self.p)))

    def close(self):
        if self.p:
            self.L.sr_path_bins_free(self.p)
            self.p = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _names(self, names):
        names = self.names if names is None else list(names)
        if len(names) != int(self.p.contents.paths):
            raise SeqRushError(-1, "path bins: one name per path is needed")
        arr = (C.c_char_p * max(1, len(names)))(*[n.encode() for n in names])
        return C.cast(arr, C.POINTER(C.c_char_p)), arr

    def as_dict(self) -> dict:
        s = self.p.contents
        P, B = int(s.paths), int(s.bins)

        def arr(ptr):
            return np.ctypeslib.as_array(ptr, shape=(max(P * B, 1),))[:P * B].astype(np.uint64, copy=True).reshape(P, B)
        d = {k: int(getattr(s, k)) for k in ("length", "paths", "bins", "bin_width", "bin_us")}
        d["cov"], d["inv"] = arr(s.cov), arr(s.inv)
        d["kernel_us"] = dict(zip(BIN_KERNELS, (int(v) for v in s.kernel_us)))
        return d

    def tsv(self, names=None) -> str:
        ptr, _keep = self._names(names)
        out = C.c_void_p()
        check(self.L.sr_path_bins_tsv(self.p, ptr, C.byref(out)))
        return _take_text(out)

    def rgb(self, names=None, **viz) -> np.ndarray:
        ptr, _keep = self._names(names)
        vp = _viz_params(**viz)
        out = C.c_void_p(); w = C.c_uint32(); h = C.c_uint32()
        check(self.L.sr_path_bins_rgb(self.p, ptr, C.byref(vp), C.byref(out), C.byref(w), C.byref(h)))
        n = w.value * h.value * 3
        img = np.frombuffer(C.string_at(out, n), dtype=np.uint8).reshape(h.value, w.value, 3).copy()
        self.L.sr_free(out)
        return img

    def png(self, names=None, **viz) -> bytes:
        ptr, _keep = self._names(names)
        vp = _viz_params(**viz)
        out = C.c_void_p(); n = C.c_uint64()
        check(self.L.sr_path_bins_png(self.p, ptr, C.byref(vp), C.byref(out), C.byref(n)))
        data = C.string_at(out, n.value)
        self.L.sr_free(out)
        return data


def path_bins(text: str, device: int = 0, bin_width: int = 0, bins: int = 0) -> dict:
    """path-by-bin coverage of any GFA with S / L / P lines and numeric node ids: give exactly one of
    bin_width (bp) and bins (a count; the width is ceil(length / bins)).  device >= 0: HIP kernels on that device, -1: the host
    twin (the same integers).  -> dict: length, paths, bins, bin_width; cov / inv (uint64 [paths, bins]: base pairs of the bin
    covered by the path's steps / by its reverse steps); bin_us, kernel_us"""
    with PathBins(text, device, bin_width, bins) as pb:
        return pb.as_dict()


def path_bins_tsv(text: str, device: int = 0, bin_width: int = 0, bins: int = 0) -> str:
    """the table of path_bins() as TSV (one row per covered cell, bins 1-based), formatted by the library"""
    with PathBins(text, device, bin_width, bins) as pb:
        return pb.tsv()


def path_bins_rgb(text: str, device: int = 0, bin_width: int = 0, bins: int = 0, **viz) -> np.ndarray:
    """the table of path_bins() as an image -> uint8 [height, width = bins, 3].  viz: mode ("path", "strand", "depth"),
    path_height, path_gap, depth_max"""
    with PathBins(text, device, bin_width, bins) as pb:
        return pb.rgb(**viz)


def path_bins_png(text: str, device: int = 0, bin_width: int = 0, bins: int = 0, **viz) -> bytes:
    """the image of path_bins_rgb() as the bytes of a PNG file"""
    with PathBins(text, device, bin_width, bins) as pb:
        return pb.png(**viz)


def write_bins(text: str, args: "Args"):
    """the --bin / --viz stage of both Python front ends on the final GFA text"""
    if args.bin:
        if args.bin_width and args.bin_count:
            raise SeqRushError(-1, "--bin-width and --bin-count exclude each other")
        kw = dict(bin_width=args.bin_width) if args.bin_width else dict(bins=args.bin_count or 1500)
        with PathBins(text, args.device, **kw) as pb:
            with open(args.bin, "w") as fh:
                fh.write(pb.tsv())
            us = int(pb.p.contents.bin_us)
        print(f"Bins written to {args.bin}")
        if args.verbose:
            print(f"Bin stage: {us} us on device {args.device}")
    if args.viz:
        with PathBins(text, args.device, bins=args.viz_width) as pb:
            data = pb.png(mode=args.viz_mode, path_height=args.viz_path_height, path_gap=args.viz_path_gap,
                          depth_max=args.viz_depth_max)
            us = int(pb.p.contents.bin_us)
        with open(args.viz, "wb") as fh:
            fh.write(data)
        print(f"Visualization written to {args.viz}")
        if args.verbose:
            print(f"Bin stage: {us} us on device {args.device}")


SR_GROWTH_DEVICE_HOST = -1
GROWTH_KERNELS = ("presence", "histogram", "ranks", "growth")
GROWTH_GROUP_BY = ("path", "sample", "haplotype")


def growth_groups(names, mode="path"):
    """groups of paths from their names -> (group_of: uint32 [paths], group names).  mode "path": every path its own
    group; "sample" / "haplotype": the PanSN prefix before the first / second '#' (a name without that many is its own
    key); groups are numbered by first appearance"""
    if mode not in GROWTH_GROUP_BY:
        raise SeqRushError(-1, f"group_by must be one of {', '.join(GROWTH_GROUP_BY)}, not {mode!r}")
    L = _lib.load()
    names = list(names)
    arr = (C.c_char_p * max(1, len(names)))(*[n.encode() for n in names])
    group_of = np.zeros(max(1, len(names)), dtype=np.uint32)
    n = C.c_uint32()
    out = C.POINTER(C.c_char_p)()
    check(L.sr_growth_groups(C.cast(arr, C.POINTER(C.c_char_p)), len(names), GROWTH_GROUP_BY.index(mode),
                             group_of.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(n), C.byref(out)))
    group_names = [out[i].decode() for i in range(n.value)]
    L.sr_free(C.cast(out, C.c_void_p))
    return group_of[:len(names)].copy(), group_names


def growth_expected(bp_by_groups):
    """closed-form E pan(k), E core(k), k = 1..G, over all orders of the groups -> two float64 arrays [G]"""
    bp = np.ascontiguousarray(bp_by_groups, dtype=np.uint64)
    G = len(bp) - 1
    pan, core = np.zeros(max(G, 1)), np.zeros(max(G, 1))
    check(_lib.load().sr_growth_expected(bp.ctypes.data_as(C.POINTER(C.c_uint64)), G, _pd(pan), _pd(core)))
    return pan[:G], core[:G]


def growth_fit(pan_exp):
    """Heaps' law fit of new(k) = pan_exp(k) - pan_exp(k - 1) ~ kappa k^-alpha -> (alpha, kappa, points); points < 2: no fit"""
    pe = np.ascontiguousarray(pan_exp, dtype=np.float64)
    a, k, n = C.c_double(), C.c_double(), C.c_uint32()
    check(_lib.load().sr_growth_fit(_pd(pe), len(pe), C.byref(a), C.byref(k), C.byref(n)))
    return a.value, k.value, n.value


class Growth:
    """an owned sr_growth: the growth curves of a GFA text.  group_by names the grouping of the
    text's P lines; group_of / n_groups give one directly instead"""

    def __init__(self, text: str, device: int = 0, group_by: str = "path", permutations: int = 1000, seed: int = 9399220,
                 group_of=None, n_groups: Optional[int] = None):
        for k, v in (("permutations", permutations), ("seed", seed)):
            if not 0 <= int(v) < 2 ** 64:
                raise SeqRushError(-1, f"{k} must be in 0 .. 2^64 - 1")
        self.L = _lib.load()
        self.p = C.POINTER(GrowthC)()
        self.group_names = None
        if group_of is None and group_by != "path":
            group_of, self.group_names = growth_groups(_path_names(text), group_by)
        elif group_by not in GROWTH_GROUP_BY:
            raise SeqRushError(-1, f"group_by must be one of {', '.join(GROWTH_GROUP_BY)}, not {group_by!r}")
        ptr, G = None, 0
        if group_of is not None:
            group_of = np.ascontiguousarray(group_of, dtype=np.uint32)
            G = int(n_groups) if n_groups is not None else (int(group_of.max()) + 1 if len(group_of) else 0)
            keep = group_of if len(group_of) else np.zeros(1, dtype=np.uint32)
            ptr = keep.ctypes.data_as(C.POINTER(C.c_uint32))
        prm = GrowthParamsC(int(seed), int(permutations))
        check(self.L.sr_growth_gfa(text.encode(), ptr, G, C.byref(prm), int(device), C.byref(self.p)))

    def close(self):
        if self.p:
            self.L.sr_growth_free(self.p)
            self.p = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def as_dict(self) -> dict:
        s = self.p.contents
        R, G = int(s.permutations), int(s.groups)

        def arr(ptr, n, dt):
            return np.ctypeslib.as_array(ptr, shape=(max(n, 1),))[:n].astype(dt, copy=True)
        d = {k: int(getattr(s, k)) for k in ("length", "paths", "groups", "permutations", "exhaustive", "variant", "seed", "growth_us")}
        d["pan"], d["core"] = arr(s.pan, R * G, np.uint64).reshape(R, G), arr(s.core, R * G, np.uint64).reshape(R, G)
        d["perm"] = arr(s.perm, R * G, np.uint32).reshape(R, G)
        d["bp_by_groups"] = arr(s.bp_by_groups, G + 1, np.uint64)
        d["kernel_us"] = dict(zip(GROWTH_KERNELS, (int(v) for v in s.kernel_us)))
        return d

    def report(self) -> str:
        out = C.c_void_p()
        check(self.L.sr_growth_report(self.p, C.byref(out)))
        return _take_text(out)


def growth(text: str, device: int = 0, group_by: str = "path", permutations: int = 1000, seed: int = 9399220, **groups) -> dict:
    """growth curves of any GFA with S / L / P lines and numeric node ids.  device >= 0: HIP kernels
    on that device, -1: the host twin (the same integers).  -> dict: length, paths, groups, permutations (run), exhaustive,
    variant, seed; pan / core (uint64 [permutations, groups]: base pairs on at least one / on all of the first k groups of
    each permutation), perm (uint32, the group at each rank), bp_by_groups (uint64 [groups + 1]); growth_us, kernel_us"""
    with Growth(text, device, group_by, permutations, seed, **groups) as g:
        return g.as_dict()


def growth_report(text: str, device: int = 0, group_by: str = "path", permutations: int = 1000, seed: int = 9399220, **groups) -> str:
    """the TSV report of growth(): expectations, the Heaps' law fit and mean / sd / min / max over the permutations per k,
    formatted by the library (the only place where a float is formed)"""
    with Growth(text, device, group_by, permutations, seed, **groups) as g:
        return g.report()


def write_growth(text: str, args: "Args"):
    """the --growth stage of both Python front ends on the final GFA text"""
    with Growth(text, args.device, args.growth_group_by, args.growth_permutations, args.growth_seed) as g:
        with open(args.growth, "w") as fh:
            fh.write(g.report())
        us = int(g.p.contents.growth_us)
    print(f"Growth written to {args.growth}")
    if args.verbose:
        print(f"Growth stage: {us} us on device {args.device}")


SR_VARIANTS_DEVICE_HOST = -1
VARIANTS_KERNELS = ("anchors", "scan", "emit", "hash", "sort_classes", "genotypes")


class Variants:
    """an owned sr_variants: the variant sites of a GFA text against one of its paths"""

    def __init__(self, text: str, device: int = 0, ref: Optional[str] = None, max_allele_len: int = 10000,
                 hash_mask: int = 2 ** 64 - 1):
        for k, v in (("max_allele_len", max_allele_len), ("hash_mask", hash_mask)):
            if not 0 <= int(v) < 2 ** 64:
                raise SeqRushError(-1, f"{k} must be in 0 .. 2^64 - 1")
        self.L = _lib.load()
        self.p = C.POINTER(VariantsC)()
        self.names = _path_names(text)
        prm = VariantParamsC(None if ref is None else ref.encode(), int(max_allele_len), int(hash_mask), 0)
        check(self.L.sr_variants_gfa(text.encode(), C.byref(prm), int(device), C.byref(self.p)))

    def close(self):
        if self.p:
            self.L.sr_variants_free(self.p)
            self.p = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def as_dict(self) -> dict:
        s = self.p.contents
        P, NS = int(s.paths), int(s.sites)

        def arr(ptr, n, dt):
            return np.ctypeslib.as_array(ptr, shape=(max(n, 1),))[:n].astype(dt, copy=True)
        d = {k: int(getattr(s, k)) for k in ("ref_path", "ref_len", "paths", "anchors", "traversals", "sites", "hash_collision_sites",
                                             "variant", "variants_us")}
        d["breaks"], d["skipped"] = arr(s.breaks, P, np.uint64), arr(s.skipped, P, np.uint64)
        d["site_start"], d["site_end"] = arr(s.site_start, NS, np.uint64), arr(s.site_end, NS, np.uint64)
        d["site_alleles"] = arr(s.site_alleles, NS, np.uint32)
        n_alt = int(d["site_alleles"].sum())
        off = arr(s.allele_off, n_alt + 1, np.uint64)
        arena = C.string_at(s.alleles, int(off[-1]))
        flat = [arena[int(off[k]):int(off[k + 1])] for k in range(n_alt)]
        d["alleles"], k = [], 0
        for n in d["site_alleles"]:
            d["alleles"].append(flat[k:k + int(n)])
            k += int(n)
        d["gt"] = arr(s.gt, NS * P, np.int32).reshape(NS, P)
        d["ref_seq"] = C.string_at(s.ref_seq, int(s.ref_len))
        d["kernel_us"] = dict(zip(VARIANTS_KERNELS, (int(v) for v in s.kernel_us)))
        return d

    def vcf(self) -> str:
        arr = (C.c_char_p * max(1, len(self.names)))(*[n.encode() for n in self.names])
        out = C.c_void_p()
        check(self.L.sr_variants_vcf(self.p, C.cast(arr, C.POINTER(C.c_char_p)), C.byref(out)))
        return _take_text(out)


def variants(text: str, device: int = 0, ref: Optional[str] = None, max_allele_len: int = 10000, hash_mask: int = 2 ** 64 - 1) -> dict:
    """variant sites of any GFA with S / L / P lines and numeric node ids against its path `ref` (default: the first;
    DESIGN.md section 15).  device >= 0: HIP kernels on that device, -1: the host twin (the same integers and bytes).  ->
    dict: ref_path, ref_len, ref_seq, paths, anchors, traversals, sites, hash_collision_sites; breaks / skipped (uint64
    [paths]); site_start / site_end (uint64 [sites]), site_alleles, alleles (per site the list of its ALT alleles, bytes);
    gt (int32 [sites, paths], -1 = no call); variants_us, kernel_us"""
    with Variants(text, device, ref, max_allele_len, hash_mask) as v:
        return v.as_dict()


def variants_vcf(text: str, device: int = 0, ref: Optional[str] = None, max_allele_len: int = 10000, hash_mask: int = 2 ** 64 - 1) -> str:
    """the VCF text of variants(), formatted by the library"""
    with Variants(text, device, ref, max_allele_len, hash_mask) as v:
        return v.vcf()


def write_vcf(text: str, args: "Args"):
    """the --vcf stage of both Python front ends on the final GFA text"""
    with Variants(text, args.device, args.vcf_ref, args.vcf_max_allele_len) as v:
        with open(args.vcf, "w") as fh:
            fh.write(v.vcf())
        us = int(v.p.contents.variants_us)
    print(f"VCF written to {args.vcf}")
    if args.verbose:
        print(f"Variants stage: {us} us on device {args.device}")


SR_LIFT_DEVICE_HOST = -1
LIFT_KERNELS = ("positions", "first_visits", "locate", "short_pairs", "long_pairs")


class Lift:
    """an owned sr_lift: the BED intervals of paths of a GFA text projected onto its other paths"""

    def __init__(self, text: str, bed: str, device: int = 0, to: Optional[str] = None, min_covered: int = 1, short_steps: int = 8):
        for k, v in (("min_covered", min_covered), ("short_steps", short_steps)):
            if not 0 <= int(v) < 2 ** 64:
                raise SeqRushError(-1, f"{k} must be in 0 .. 2^64 - 1")
        self.L = _lib.load()
        self.p = C.POINTER(LiftC)()
        self.names = _path_names(text)
        prm = LiftParamsC(None if to is None else to.encode(), int(min_covered), int(short_steps), 0)
        check(self.L.sr_lift_gfa(text.encode(), bed.encode(), C.byref(prm), int(device), C.byref(self.p)))

    def close(self):
        if self.p:
            self.L.sr_lift_free(self.p)
            self.p = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def as_dict(self) -> dict:
        s = self.p.contents
        Q, T = int(s.queries), int(s.targets)

        def arr(ptr, n, dt):
            return np.ctypeslib.as_array(ptr, shape=(max(n, 1),))[:n].astype(dt, copy=True)
        d = {k: int(getattr(s, k)) for k in ("queries", "targets", "paths", "unknown", "out_of_range", "mapped", "variant", "to_named",
                                             "min_covered", "short_pairs", "long_pairs", "lift_us")}
        d["q_path"], d["q_start"], d["q_end"] = arr(s.q_path, Q, np.uint32), arr(s.q_start, Q, np.uint64), arr(s.q_end, Q, np.uint64)
        off = arr(s.label_off, Q + 1, np.uint64)
        arena = C.string_at(s.labels, int(off[-1]))
        d["labels"] = [arena[int(off[k]):int(off[k + 1])].decode() for k in range(Q)]
        d["target_path"] = arr(s.target_path, T, np.uint32)
        for k in ("tstart", "tend", "covered", "rev_bp"):
            d[k] = arr(getattr(s, k), Q * T, np.uint64).reshape(Q, T)
        d["kernel_us"] = dict(zip(LIFT_KERNELS, (int(v) for v in s.kernel_us)))
        return d

    def bed(self) -> str:
        arr = (C.c_char_p * max(1, len(self.names)))(*[n.encode() for n in self.names])
        out = C.c_void_p()
        check(self.L.sr_lift_bed(self.p, C.cast(arr, C.POINTER(C.c_char_p)), C.byref(out)))
        return _take_text(out)


def lift(text: str, bed: str, device: int = 0, to: Optional[str] = None, min_covered: int = 1, short_steps: int = 8) -> dict:
    """the BED intervals `bed` (name start end [label ...], 0-based, half-open) of paths of any GFA with S / L / P lines and
    numeric node ids, projected onto every path or onto the path `to`.  device >= 0: HIP kernels on
    that device, -1: the host twin (the same integers).  -> dict: queries, targets, paths, unknown, out_of_range, mapped;
    q_path / q_start / q_end / labels per query; target_path; tstart / tend / covered / rev_bp (uint64 [queries, targets],
    all 0 where unmapped); short_pairs, long_pairs, lift_us, kernel_us"""
    with Lift(text, bed, device, to, min_covered, short_steps) as v:
        return v.as_dict()


def lift_bed(text: str, bed: str, device: int = 0, to: Optional[str] = None, min_covered: int = 1, short_steps: int = 8) -> str:
    """the lifted intervals of lift() as BED text, formatted by the library"""
    with Lift(text, bed, device, to, min_covered, short_steps) as v:
        return v.bed()


def check_lift(args: "Args"):
    """--lift needs --lift-out and the other way round; before any device work"""
    if args.lift and not args.lift_out:
        raise SeqRushError(-1, "--lift needs --lift-out FILE: the lifted intervals have nowhere to go")
    for flag, on in (("--lift-out", args.lift_out), ("--lift-to", args.lift_to), ("--lift-min-covered", args.lift_min_covered != 1)):
        if on and not args.lift:
            raise SeqRushError(-1, f"{flag} is an option of --lift: give both")


def write_lift(text: str, args: "Args"):
    """the --lift stage of both Python front ends on the final GFA text"""
    try:
        with open(args.lift) as fh:
            bed = fh.read()
    except OSError as e:
        raise SeqRushError(-8, f"cannot read {args.lift}: {e.strerror}")
    with Lift(text, bed, args.device, args.lift_to, args.lift_min_covered) as v:
        with open(args.lift_out, "w") as fh:
            fh.write(v.bed())
        s = v.p.contents
        line = (f"Lift stage: {int(s.lift_us)} us on device {args.device}, {int(s.queries)} queries x {int(s.targets)} targets, "
                f"{int(s.mapped)} mapped, {int(s.unknown)} unknown, {int(s.out_of_range)} out of range")
    print(f"Lifted intervals written to {args.lift_out}")
    if args.verbose:
        print(line)


SR_EXTRACT_DEVICE_HOST = -1
EXTRACT_KERNELS = ("positions", "seeds", "context", "merge", "numbering", "emission")
EXTRACT_COUNTERS = ("regions", "unknown", "out_of_range", "in_nodes", "in_edges", "in_steps", "in_paths", "nodes", "edges", "subpaths", "steps",
                    "bases", "seeds", "by_context", "by_merge", "merge_rounds_run")


class Extract:
    """an owned sr_extract: the subgraph of regions of paths of a GFA text"""

    def __init__(self, text: str, regions=(), bed: Optional[str] = None, device: int = 0, context_steps: int = 0, merge_distance: int = 100000,
                 merge_rounds: int = 3):
        for k, v in (("context_steps", context_steps), ("merge_distance", merge_distance), ("merge_rounds", merge_rounds)):
            if not 0 <= int(v) < 2 ** 64:
                raise SeqRushError(-1, f"{k} must be in 0 .. 2^64 - 1")
        if isinstance(regions, str):
            regions = (regions,)
        self.L = _lib.load()
        self.p = C.POINTER(ExtractC)()
        self.names = _path_names(text)
        regs = [str(r).encode() for r in regions]
        arr = (C.c_char_p * max(1, len(regs)))(*regs)
        prm = ExtractParamsC(int(context_steps), int(merge_distance), int(merge_rounds), 0)
        check(self.L.sr_extract_gfa(text.encode(), None if bed is None else bed.encode(), C.cast(arr, C.POINTER(C.c_char_p)), len(regs),
                                    C.byref(prm), int(device), C.byref(self.p)))

    def close(self):
        if self.p:
            self.L.sr_extract_free(self.p)
            self.p = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def as_dict(self) -> dict:
        s = self.p.contents

        def arr(ptr, n, dt):
            return np.ctypeslib.as_array(ptr, shape=(max(n, 1),))[:n].astype(dt, copy=True)
        d = {k: int(getattr(s, k)) for k in EXTRACT_COUNTERS + ("variant", "extract_us")}
        d["level"] = arr(s.level, d["in_nodes"], np.uint32)
        d["node_old"] = arr(s.node_old, d["nodes"], np.uint32)
        d["edge_from"], d["edge_to"] = arr(s.edge_from, d["edges"], np.uint32), arr(s.edge_to, d["edges"], np.uint32)
        d["sub_path"] = arr(s.sub_path, d["subpaths"], np.uint32)
        d["sub_start"], d["sub_end"] = arr(s.sub_start, d["subpaths"], np.uint64), arr(s.sub_end, d["subpaths"], np.uint64)
        d["sub_off"] = arr(s.sub_off, d["subpaths"] + 1, np.uint64)
        d["sub_steps"] = arr(s.sub_steps, d["steps"], np.uint32)
        d["sub_names"] = [f"{self.names[int(p)]}:{int(a)}-{int(b)}" for p, a, b in zip(d["sub_path"], d["sub_start"], d["sub_end"])]
        d["kernel_us"] = dict(zip(EXTRACT_KERNELS, (int(v) for v in s.kernel_us)))
        return d

    def gfa(self) -> str:
        out = C.c_void_p()
        check(self.L.sr_extract_text(self.p, C.byref(out)))
        return _take_text(out)


def extract(text: str, regions=(), bed: Optional[str] = None, device: int = 0, context_steps: int = 0, merge_distance: int = 100000,
            merge_rounds: int = 3) -> dict:
    """the subgraph of any GFA with S / L / P lines and numeric node ids that the regions (`NAME` or `NAME:START-END`
    strings, and / or the lines of the BED text `bed`) of its paths touch, grown by context_steps L lines and closed over
    gaps of at most merge_distance bases in merge_rounds rounds.  device >= 0: HIP kernels on that
    device, -1: the host twin (the same integers and bytes).  -> dict: the counters of sr_extract; level (uint32
    [in_nodes], all ones = not kept); node_old; edge_from / edge_to; sub_path / sub_start / sub_end / sub_off / sub_steps
    and sub_names; extract_us, kernel_us"""
    with Extract(text, regions, bed, device, context_steps, merge_distance, merge_rounds) as v:
        return v.as_dict()


def extract_gfa(text: str, regions=(), bed: Optional[str] = None, device: int = 0, context_steps: int = 0, merge_distance: int = 100000,
                merge_rounds: int = 3) -> str:
    """the subgraph of extract() as GFA text, formatted by the library"""
    with Extract(text, regions, bed, device, context_steps, merge_distance, merge_rounds) as v:
        return v.gfa()


def extract_line(s, device) -> str:
    """the one line of -v, from an ExtractC"""
    return (f"Extract stage: {int(s.extract_us)} us on device {device}, {int(s.regions)} regions, {int(s.unknown)} unknown, "
            f"{int(s.out_of_range)} out of range, {int(s.seeds)} seeds + {int(s.by_context)} by context + {int(s.by_merge)} by merge in "
            f"{int(s.merge_rounds_run)} rounds = {int(s.nodes)} of {int(s.in_nodes)} nodes, {int(s.edges)} edges, {int(s.subpaths)} subpaths, "
            f"{int(s.steps)} steps, {int(s.bases)} bases")


def check_extract(args: "Args"):
    """a region or a BED needs --extract-out and the other way round; before any device work"""
    asked = bool(args.extract_regions) or bool(args.extract_bed)
    if asked and not args.extract_out:
        raise SeqRushError(-1, "--extract-region / --extract-bed need --extract-out FILE: the extracted graph has nowhere to go")
    if args.extract_out and not asked:
        raise SeqRushError(-1, "--extract-out needs --extract-region REGION or --extract-bed FILE: there is nothing to extract")
    for flag, on in (("--extract-context-steps", args.extract_context_steps != 0), ("--extract-merge-distance", args.extract_merge_distance != 100000),
                     ("--extract-merge-rounds", args.extract_merge_rounds != 3)):
        if on and not asked:
            raise SeqRushError(-1, f"{flag} is an option of --extract-region / --extract-bed: give both")


def write_extract(text: str, args: "Args"):
    """the --extract-* stage of both Python front ends on the final GFA text"""
    bed = None
    if args.extract_bed:
        try:
            with open(args.extract_bed) as fh:
                bed = fh.read()
        except OSError as e:
            raise SeqRushError(-8, f"cannot read {args.extract_bed}: {e.strerror}")
    with Extract(text, tuple(args.extract_regions), bed, args.device, args.extract_context_steps, args.extract_merge_distance,
                 args.extract_merge_rounds) as v:
        with open(args.extract_out, "w") as fh:
            fh.write(v.gfa())
        line = extract_line(v.p.contents, args.device)
    print(f"Extracted graph written to {args.extract_out}")
    if args.verbose:
        print(line)


LAYOUT_STATS =("sgd_ms", "terms_per_iter", "iterations", "subrounds_per_iter", "nodes", "steps", "stage_ms")


def _layout_params(params) -> LayoutParamsC:
    if isinstance(params, LayoutParamsC):
        return params
    lp = LayoutParamsC()
    _lib.load().sr_layout_params_default(C.byref(lp))
    for k, v in params.items():
        if k == "reserved" or not hasattr(lp, k):
            raise AttributeError(k)
        setattr(lp, k, v)
    return lp


def _n_segments(text: str) -> int:
    return sum(1 for line in text.split("\n") if line.startswith("S\t"))


def _pd(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _xy(xy, n=None):
    a = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1)
    if a.size % 4 or (n is not None and a.size != 4 * n):
        raise SeqRushError(-1, "a layout has 4 values per node: x0 y0 x1 y1")
    return a, a.size // 4


def _take_text(out) -> str:
    res = C.cast(out, C.c_char_p).value.decode()
    _lib.load().sr_free(out)
    return res


def layout_gfa(text: str, n_nodes: Optional[int] = None, **params) -> np.ndarray:
    """the 2-D path-guided SGD layout of any GFA with S / L / P lines and numeric node ids.
    params: sr_layout_params fields (device >= 0: that GPU, -1: the host twin with the same bits, -2: the sequential
    yardstick).  -> float64 array [nodes, 4]: x0 y0 x1 y1 per node in ascending id order.  n_nodes: the number of nodes
    the caller expects (default: the S lines of text)"""
    lp = _layout_params(params)
    n = _n_segments(text) if n_nodes is None else int(n_nodes)
    out = np.zeros(max(4 * n, 1), dtype=np.float64)
    check(_lib.load().sr_layout_gfa(text.encode(), C.byref(lp), _pd(out), n))
    return out[:4 * n].reshape(n, 4)


def layout_tsv(xy) -> str:
    """`idx X Y` rows of a layout (two per node), formatted by the library"""
    a, n = _xy(xy)
    out = C.c_void_p()
    check(_lib.load().sr_layout_tsv(_pd(a), n, C.byref(out)))
    return _take_text(out)


def layout_svg(text: str, xy) -> str:
    """the layout drawn as SVG: one line per node, one thin line per L line of text; formatted by the library"""
    a, n = _xy(xy)
    out = C.c_void_p()
    check(_lib.load().sr_layout_svg(text.encode(), _pd(a), n, C.byref(out)))
    return _take_text(out)


def layout_quality(text: str, xy, seed: int = 1, samples: int = 200000) -> dict:
    """sampled path stress and mean node length error of a layout (host, double) -> dict(stress, node_len_err, pairs)"""
    a, n = _xy(xy)
    out = np.zeros(4, dtype=np.float64)
    check(_lib.load().sr_layout_quality(text.encode(), _pd(a), n, int(seed), int(samples), _pd(out)))
    return dict(stress=float(out[0]), node_len_err=float(out[1]), pairs=int(out[2]))


def layout_stats() -> dict:
    """LAYOUT_STATS of the calling thread's last layout_gfa"""
    out = (C.c_double * 7)()
    n = _lib.load().sr_layout_stats(out, 7)
    if n < 0:
        check(n)
    return {k: float(out[i]) for i, k in enumerate(LAYOUT_STATS)}


def layout_resolve(text: str, **params) -> dict:
    """tests: the parameters layout_gfa resolves for text"""
    lp = _layout_params(params)
    res = LayoutParamsC()
    check(_lib.load().sr_layout_resolve(text.encode(), C.byref(lp), C.byref(res)))
    return {f: getattr(res, f) for f, _ in LayoutParamsC._fields_ if f != "reserved"}


def layout_select(text: str, k: int, t0: int, count: int, cooling: bool = False, **params):
    """tests: the selection of terms t0 .. t0 + count - 1 of iteration k -> list of (i, j, d), None for a skipped draw"""
    lp = _layout_params(params)
    i = np.zeros(max(count, 1), dtype=np.uint32); j = np.zeros(max(count, 1), dtype=np.uint32)
    d = np.zeros(max(count, 1), dtype=np.float64)
    check(_lib.load().sr_layout_select_host(text.encode(), C.byref(lp), k, t0, count, 1 if cooling else 0,
                                            i.ctypes.data_as(C.POINTER(C.c_uint32)), j.ctypes.data_as(C.POINTER(C.c_uint32)), _pd(d)))
    return [None if int(i[q]) == 0xffffffff else (int(i[q]), int(j[q]), float(d[q])) for q in range(count)]


def write_layout(text: str, args: "Args"):
    """the --layout / --layout-svg stage of both Python front ends on the final GFA text"""
    xy = layout_gfa(text, seed=args.layout_seed, iter_max=args.layout_iter_max, device=args.device)
    if args.layout:
        with open(args.layout, "w") as fh:
            fh.write(layout_tsv(xy))
    if args.layout_svg:
        with open(args.layout_svg, "w") as fh:
            fh.write(layout_svg(text, xy))
    print(f"Layout written to {args.layout or args.layout_svg}")
    if args.verbose:
        st = layout_stats()
        print(f"Layout stage: SGD {st['sgd_ms']:.3f} ms, stage {st['stage_ms']:.3f} ms on device {args.device}")


def sgd_layout(text: str, **params) -> np.ndarray:
    """the path-guided SGD positions of a GFA's nodes (ascending id order) -> float64 array"""
    L = _lib.load()
    sp = _sort_params(params)
    n = sum(1 for line in text.split("\n") if line.startswith("S\t"))
    out = np.zeros(max(n, 1), dtype=np.float64)
    check(L.sr_sgd_layout(text.encode(), C.byref(sp.c), out.ctypes.data_as(C.POINTER(C.c_double)), n))
    return out[:n]


def sgd_tables(text: str, **params):
    """resolved parameters and tables of the SGD on a GFA -> (dict of sr_sort_params, etas, zetas, prefix_theta,
    prefix_cooling)"""
    L = _lib.load()
    sp = _sort_params(params)
    res = SortParamsC()
    sizes = (C.c_uint64 * 4)()
    check(L.sr_sgd_tables(text.encode(), C.byref(sp.c), C.byref(res), sizes, None, None, None, None))
    arrs = [np.zeros(max(int(sizes[i]), 1), dtype=np.float64) for i in (0, 1, 2, 2)]
    ptr = [a.ctypes.data_as(C.POINTER(C.c_double)) for a in arrs]
    check(L.sr_sgd_tables(text.encode(), C.byref(sp.c), C.byref(res), sizes, *ptr))
    d = {f: getattr(res, f) for f, _ in SortParamsC._fields_}
    return d, arrs[0][:int(sizes[0])], arrs[1][:int(sizes[1])], arrs[2][:int(sizes[2])], arrs[3][:int(sizes[2])]


def sort_stats():
    """the calling thread's last sort: dict of sgd_ms, groom_ms, topo_ms, write_ms, terms_per_iter, iterations,
    subrounds_per_iter, nodes, steps, stage_ms (host-clock wall time of the whole stage, everything included)"""
    out = (C.c_double * 10)()
    n = _lib.load().sr_sort_stats(out, 10)
    if n < 0:
        check(n)
    keys = ("sgd_ms", "groom_ms", "topo_ms", "write_ms", "terms_per_iter", "iterations", "subrounds_per_iter", "nodes", "steps",
            "stage_ms")
    return {k: float(out[i]) for i, k in enumerate(keys)}


def build_gfa(seqset: SeqSet, labels: np.ndarray, compact: bool = False):
    """Graph induction + GFA text from canonical labels (consumer A9; --no-sort, with or without --no-compact).
    -> (gfa_text, n_nodes, n_edges)"""
    L = _lib.load()
    labels = np.ascontiguousarray(labels, dtype=np.uint64)
    out = C.c_void_p(); nn = C.c_uint64(); ne = C.c_uint64()
    check(L.sr_build_gfa_opts(C.byref(seqset.c), labels.ctypes.data_as(C.POINTER(C.c_uint64)), 1 if compact else 0,
                              C.byref(out), C.byref(nn), C.byref(ne)))
    text = C.cast(out, C.c_char_p).value.decode()
    L.sr_free(out)
    return text, int(nn.value), int(ne.value)


def build_gfa_from_nodes(seqset: SeqSet, nodes: np.ndarray, compact: bool = False):
    """Graph induction from a RAW uf_rush node array with the reference's root rule (src/bidirected_builder.rs:46-48,
    176-182: node base = base at the offset of the component's union-find root).  -> (gfa_text, n_nodes, n_edges)"""
    L = _lib.load()
    nodes = np.ascontiguousarray(nodes, dtype=np.uint64)
    out = C.c_void_p(); nn = C.c_uint64(); ne = C.c_uint64()
    check(L.sr_build_gfa_from_nodes(C.byref(seqset.c), nodes.ctypes.data_as(C.POINTER(C.c_uint64)), 1 if compact else 0,
                                    C.byref(out), C.byref(nn), C.byref(ne)))
    text = C.cast(out, C.c_char_p).value.decode()
    L.sr_free(out)
    return text, int(nn.value), int(ne.value)


class HostUnionFind:
    """uf_rush node array on the host (sr_uf_*_host: same packing / halving / rank / tie rule as uf_rush lib.rs:112-208,
    one thread): SeqRush::new state, unite, merge of gathered canonical label arrays, canonical labels."""

    def __init__(self, total_len: int):
        self.n = 2 * total_len + 2
        self.nodes = np.zeros(self.n, dtype=np.uint64)
        check(_lib.load().sr_uf_init_host(self._p(self.nodes), self.n, total_len))

    @staticmethod
    def _p(a):
        return a.ctypes.data_as(C.POINTER(C.c_uint64))

    def unite(self, x: int, y: int) -> bool:
        r = _lib.load().sr_uf_unite_host(self._p(self.nodes), self.n, x, y)
        if r < 0:
            check(r)
        return r == 1

    def merge_labels(self, label_arrays):
        lab = np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=np.uint64) for a in label_arrays]))
        assert len(lab) % self.n == 0
        check(_lib.load().sr_uf_merge_labels_host(self._p(self.nodes), self.n, self._p(lab), len(lab) // self.n))

    def canonical_labels(self) -> np.ndarray:
        out = np.zeros(self.n, dtype=np.uint64)
        check(_lib.load().sr_uf_canonical_labels_host(self._p(self.nodes), self.n, self._p(out)))
        return out


class ExtendPlan:
    """Owned ``sr_extend_plan``: the paths of a GFA spelled back into sequences (device >= 0: on that GPU; -1: plain loops),
    followed by the new records, and the tables that seed the union-find with the graph's partition."""

    def __init__(self, gfa_text: str, new_records=(), device: int = -1):
        self.L = _lib.load()
        self._h = C.c_void_p()
        new = new_records if isinstance(new_records, SeqSet) else SeqSet(list(new_records))
        check(self.L.sr_extend_plan_gfa(gfa_text.encode(), C.byref(new.c) if new.n else None, device, C.byref(self._h)))
        m = self.L.sr_extend_plan_seqs(self._h).contents
        n = int(m.n)
        off = [int(m.offsets[i]) for i in range(n + 1)]
        raw = C.string_at(C.cast(C.byref(m, SeqSetC.bases.offset), C.POINTER(C.c_void_p))[0], off[n]) if off[n] else b""
        self.n_old = int(self.L.sr_extend_plan_n_old(self._h))
        self.records = [(m.names[i].decode(), raw[off[i]: off[i + 1]]) for i in range(n)]
        self.seqset = SeqSet(self.records)          # a copy with the same bytes: what build_gfa() of a context reads

    def stats(self) -> dict:
        st = ExtendStatsC()
        check(self.L.sr_extend_plan_stats(self._h, C.byref(st)))
        return {f: int(getattr(st, f)) for f, _ in ExtendStatsC._fields_}

    def pair_list(self, pairs):
        """the pair filter: the (query, target) pairs that touch a new sequence, in the order given"""
        q = np.ascontiguousarray([a for a, _ in pairs] or [0], dtype=np.uint32)
        t = np.ascontiguousarray([b for _, b in pairs] or [0], dtype=np.uint32)
        PU = C.POINTER(C.c_uint32)
        qo, to, cnt = PU(), PU(), C.c_uint64()
        check(self.L.sr_extend_pair_list(self._h, q.ctypes.data_as(PU), t.ctypes.data_as(PU), len(pairs), C.byref(qo), C.byref(to),
                                         C.byref(cnt)))
        out = [(int(qo[i]), int(to[i])) for i in range(cnt.value)]
        self.L.sr_free(C.cast(qo, C.c_void_p)); self.L.sr_free(C.cast(to, C.c_void_p))
        return out

    def close(self):
        if self._h:
            self.L.sr_extend_plan_free(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def extend_seed_host(plan: ExtendPlan, uf: "HostUnionFind") -> dict:
    """the host twin of the seed on a HostUnionFind of the plan's merged set -> dict(unions_attempted, unions_joined)"""
    st = (C.c_uint64 * 2)()
    check(_lib.load().sr_extend_seed_host(plan._h, uf._p(uf.nodes), uf.n, st))
    return dict(unions_attempted=int(st[0]), unions_joined=int(st[1]))


def check_extend(args: "Args"):
    """the refusals of --extend that need no device: each would compose in principle, none is verified"""
    if not args.extend:
        return
    for on, what in ((args.iterative, "--iterative"), (args.paf is not None, "-p"), (args.patch_inversions, "--patch-inversions"),
                     (args.gpus > 1 or args.shard_count > 1, "--gpus N > 1")):
        if on:
            raise SeqRushError(-6, f"--extend cannot be combined with {what}")


def extend_report(st: dict) -> str:
    """the -v line of --extend"""
    return (f"Extend: {st['old_paths']} paths {st['old_bases']} bases {st['old_steps']} steps + {st['new_sequences']} sequences, "
            f"pairs {st['pairs_after']} of {st['pairs_before']}, unions {st['unions_joined']} of {st['unions_attempted']}, "
            f"spell_us={st['spell_us']} seed_us={st['seed_us']}")


def uf_find(nodes: np.ndarray, x: int) -> int:
    nodes = np.ascontiguousarray(nodes, dtype=np.uint64)
    return int(_lib.load().sr_uf_find(nodes.ctypes.data_as(C.POINTER(C.c_uint64)), len(nodes), x))


# --------------------------------------------------------------------------- SeqRush
class SeqRush:
    """Mirror of ``SeqRush`` (src/seqrush.rs:298-336, 433-458) over the device path."""

    def __init__(self, sequences: List[Sequence], device: int = 0, extend_plan: "Optional[ExtendPlan]" = None):
        self.extend_plan = extend_plan                       # --extend: `sequences` is its merged set
        for s in sequences:                                  # :310-317
            if len(s.data) == 0:
                raise ValueError(
                    f"Empty sequences are not allowed: sequence '{s.id}' has length 0")
        off = 0
        for s in sequences:
            s.offset = off
            off += len(s.data)
        self.sequences = sequences
        self.total_length = off
        self.seqset = SeqSet(sequences)
        self.ctx = Context(device)
        self.labels = None
        self.alignments = None

    def align_and_unite(self, args: Args):
        """align_and_unite_with_allwave (src/seqrush.rs:611-757) on the device"""
        check_extend(args)
        if args.iterative and args.paf is not None:
            raise SeqRushError(-6, "--iterative cannot be combined with -p (there is no alignment stage to stop)")
        if args.patch_inversions and (args.iterative or args.paf is not None):
            raise SeqRushError(-6, f"--patch-inversions cannot be combined with {'--iterative' if args.iterative else '-p'}")
        if args.patch_inversions and (args.inversion_min_size or 2 * args.min_match_length) == 0:
            raise SeqRushError(-1, "--patch-inversions needs -k or --inversion-min-size: a threshold of 0 would call every "
                                   "complementary SNP an inversion")
        check_inversion_join(args)
        if args.paf is not None:                      # align_and_unite_from_paf (src/seqrush.rs:510-609)
            print(f"Reading alignments from PAF file: {args.paf}")
            self.ctx.load_paf(self.seqset, Params.from_args(args), args.paf)
            self.ctx.run()
            self.ctx.sync()
            self.labels = self.ctx.download_labels()
            self.ctx.sync()
            return
        if args.aligner.lower() != "allwave":
            raise SeqRushError(-6, f"aligner '{args.aligner}' is out of scope; only 'allwave'")
        params = Params.from_args(args)
        if args.iterative:
            return self._align_and_unite_iterative(args, params)
        n = len(self.sequences)
        if self.extend_plan is not None:
            self.ctx.load_extend(self.extend_plan, params)
            self.seqset = self.ctx.seqset
            print(f"Total sequence pairs: {n * n} (sparsification: {args.sparsification})")
            print(f"Extending {self.extend_plan.n_old} paths by {n - self.extend_plan.n_old} sequences: {self.ctx.num_pairs} pairs to align")
        else:
            self.ctx.load(self.seqset, params)
            print(f"Total sequence pairs: {n * n} (sparsification: {args.sparsification})")
        if args.patch_inversions:
            self.ctx.enable_inversions(args.inversion_min_size, keep_alignments=bool(args.output_alignments),
                                       join_below=args.inversion_join)
        if args.output_alignments:
            al = self.ctx.align_all(unite=True)         # batches: align, copy the CIGARs out, unite
            print(f"Writing alignments to {args.output_alignments}")
            al.write_paf(self.seqset, args.output_alignments)
            al.close()
            append_inversion_paf(self.ctx, self.seqset, args.output_alignments, args.patch_inversions)
        else:
            self.ctx.run()
        self.ctx.sync()
        if self.extend_plan is not None:
            self.extend_stats = self.ctx.extend_stats()
            if args.verbose:
                print(extend_report(self.extend_stats))
        if args.patch_inversions:
            st = self.ctx.inversion_stats()
            self.inversion_stats = st
            print(f"Patched inversions: {st['accepted']} of {st['candidates']} candidate gaps")
            if args.verbose and args.inversion_join:
                js = self.ctx.inversion_join_stats()
                self.inversion_join_stats = js
                print(inversion_join_report(js))
        self.labels = self.ctx.download_labels()
        self.ctx.sync()

    def _align_and_unite_iterative(self, args: Args, params: Params):
        """align_and_unite_iterative (src/seqrush.rs:867-1132) on the device, with the reference's messages"""
        import sys
        if args.shard_count != 1:
            raise SeqRushError(-6, "--iterative cannot be sharded over GPUs (its stop rule is global and sequential)")
        print("Using iterative alignment with stabilization detection")
        if params.c.sparsify_kind != SR_SPARSE_TREE:
            print("Note: Iterative mode works best with tree sampling. Using default tree:3,3,0.1,16", file=sys.stderr)
        self.ctx.load_iterative(self.seqset, params, keep_alignments=bool(args.output_alignments))
        st = self.ctx.iterative_stats()
        print(f"Processing {st['tree_entries']} tree pairs (k={st['tree_k_nearest']}, k_far={st['tree_k_farthest']}) + "
              f"{st['random_entries']} random pairs (frac={rust_f64(st['tree_rand_frac'])})")
        if args.output_alignments:
            print(f"Writing alignments to {args.output_alignments}")
        print("\nPhase 1: Processing tree pairs (k-nearest + k-farthest)...")
        self.ctx.run_iterative()
        self.ctx.sync()
        st = self.ctx.iterative_stats()
        for line in iterative_report(st, args.verbose):
            print(line)
        if args.output_alignments:
            al = self.ctx.iterative_alignments()
            al.write_paf(self.seqset, args.output_alignments)
            al.close()
        self.labels = self.ctx.download_labels()
        self.ctx.sync()
        self.iterative_stats = st

    def build_graph(self, args: Args):
        print(f"Building graph with {len(self.sequences)} sequences "
              f"(total length: {self.total_length})")
        self.align_and_unite(args)
        self.write_gfa(args)

    def write_gfa(self, args: Args):
        # Args.sort selects the Ygs layout whatever no_sort says: no_sort defaults to True for the Python API, and both
        # CLIs refuse `--sort --no-sort` before anything runs
        if not args.no_sort and not args.sort:
            raise SeqRushError(-6, "only --no-sort output is implemented by default (the reference's unseeded Ygs layout "
                                   "is not reproducible run to run, SURVEY 0.4); pass --sort for the Ygs layout; "
                                   "compaction runs unless --no-compact")
        sort = SortParams.from_args(args) if args.sort else None
        # graph induction on the device, compaction on the host or (--compact-on device) on the device, Ygs: SGD on the
        # device, groom + topological sort on the host
        where = {"compact_on": "device"} if args.compact_on == "device" else {}     # (the default call is unchanged)
        if args.compact_on not in ("host", "device"):
            raise SeqRushError(-1, f"compact_on must be 'host' or 'device', not {args.compact_on!r}")
        text, _, _ = self.ctx.build_gfa(compact=not args.no_compact, sort=sort, **where)
        if args.verbose and args.compact_on == "device":
            print("Compaction on device: " + " ".join(f"{k}={v}" for k, v in list(compact_stats().items())[:7]))
        with open(args.output, "w") as fh:
            fh.write(text)
        if args.stats:
            # the stage parses the text just written (keeping the tables on the device: DESIGN.md section 7 item 5)
            report, st = _graph_stats_report(text, args.device)
            with open(args.stats, "w") as fh:
                fh.write(report)
            print(f"Statistics written to {args.stats}")
            if args.verbose:
                print(f"Statistics stage: {st['stats_us']} us on device {args.device}")
        if args.layout or args.layout_svg:
            write_layout(text, args)
        if args.bin or args.viz:
            write_bins(text, args)
        if args.growth:
            write_growth(text, args)
        if args.vcf:
            write_vcf(text, args)
        if args.lift:
            write_lift(text, args)
        if args.extract_out:
            write_extract(text, args)


def run_seqrush(args: Args):
    """src/seqrush.rs:1839-1853"""
    check_lift(args)
    check_extract(args)
    sequences = load_sequences(args.sequences)
    print(f"Loaded {len(sequences)} sequences")
    plan = None
    if args.extend:
        check_extend(args)
        try:
            with open(args.extend) as fh:
                text = fh.read()
        except OSError as e:
            raise SeqRushError(-8, f"cannot read {args.extend}: {e.strerror}")
        plan = ExtendPlan(text, sequences, device=args.device)
        print(f"Extending {args.extend}: {plan.n_old} paths")
        sequences = [Sequence(name, data) for name, data in plan.records]
    sr = SeqRush(sequences, device=args.device, extend_plan=plan)
    sr.build_graph(args)
    print(f"Graph written to {args.output}")
    return sr


def run_seqrush_rank(args: Args):
    """One rank of `--gpus N` (started by torch.distributed.run, one process per GPU): this rank's cost-balanced
    shard of the pair list -> private forest -> ONE all-gather of canonical labels (u32 while 2N+2 < 2^32; RCCL over
    xGMI) -> replay-unite on every rank -> rank 0 induces the graph and writes the GFA."""
    import os
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    local = int(os.environ.get("LOCAL_RANK", "0"))
    single_dev = os.environ.get("SR_BENCH_SINGLE_DEVICE") == "1"      # testing: all ranks on GPU 0, gloo
    dev = 0 if single_dev else local
    torch.cuda.set_device(dev)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if single_dev:
        dist.init_process_group("gloo")
    else:
        dist.init_process_group("nccl", device_id=torch.device("cuda", dev))
    args.device, args.shard_rank, args.shard_count = dev, rank, world
    sequences = load_sequences(args.sequences)
    if rank == 0:
        print(f"Loaded {len(sequences)} sequences")
        print(f"Building graph with {len(sequences)} sequences (total length: {sum(len(s.data) for s in sequences)})")
    if os.environ.get("SR_TEST_FAIL_RANK") == str(rank):       # test hook: a rank that fails before the collective
        raise SeqRushError(-1, f"SR_TEST_FAIL_RANK: rank {rank} fails on purpose")
    sr = SeqRush(sequences, device=dev)
    ctx = sr.ctx
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    if args.paf is not None:
        ctx.load_paf(sr.seqset, Params.from_args(args), args.paf)
        ctx.run()
    else:
        ctx.load(sr.seqset, Params.from_args(args))
        if rank == 0:
            n = len(sequences)
            print(f"Total sequence pairs: {n * n} (sparsification: {args.sparsification})")
        if args.patch_inversions:               # a job stays on the rank that owns its pair and lands in that rank's forest
            ctx.enable_inversions(args.inversion_min_size, keep_alignments=bool(args.output_alignments),
                                  join_below=args.inversion_join)
        if args.output_alignments:
            al = ctx.align_all(unite=True)
            al.write_paf(sr.seqset, f"{args.output_alignments}.rank{rank}")
            al.close()
            append_inversion_paf(ctx, sr.seqset, f"{args.output_alignments}.rank{rank}", args.patch_inversions)
        else:
            ctx.run()
    ctx.sync()
    if args.patch_inversions and args.paf is None:
        st = ctx.inversion_stats()
        js = ctx.inversion_join_stats()
        tot = torch.tensor([st["accepted"], st["candidates"], js["islands_absorbed"], js["rejected_site_cost"], js["host_us"]],
                           dtype=torch.int64, device="cpu" if single_dev else "cuda")
        dist.all_reduce(tot)
        if rank == 0:
            print(f"Patched inversions: {int(tot[0])} of {int(tot[1])} candidate gaps")
            if args.verbose and args.inversion_join:
                print(inversion_join_report(dict(islands_absorbed=int(tot[2]), rejected_site_cost=int(tot[3]), host_us=int(tot[4]))))
    ufn = ctx.uf_size
    u32 = ufn < (1 << 32)
    ldt = torch.int32 if u32 else torch.int64
    lab = torch.empty(ufn, dtype=ldt, device="cuda")
    gathered = torch.empty(ufn * world, dtype=ldt, device="cuda")
    (ctx.labels_device_u32 if u32 else ctx.labels_device)(lab.data_ptr())
    torch.cuda.synchronize()
    if single_dev:
        parts = [torch.empty(ufn, dtype=ldt) for _ in range(world)]
        dist.all_gather(parts, lab.cpu())
        gathered.copy_(torch.cat(parts))
    else:
        dist.all_gather_into_tensor(gathered, lab)
    (ctx.merge_labels_u32 if u32 else ctx.merge_labels)(gathered.data_ptr(), world)
    ctx.sync()
    dist.barrier()
    if rank == 0:
        if args.output_alignments:
            with open(args.output_alignments, "wb") as out:
                for r in range(world):
                    part = f"{args.output_alignments}.rank{r}"
                    with open(part, "rb") as fh:
                        out.write(fh.read())
                    os.remove(part)
            print(f"Writing alignments to {args.output_alignments}")
        sr.write_gfa(args)
        print(f"Graph written to {args.output}")
    dist.barrier()
    dist.destroy_process_group()
    return sr


SR_SPARSE_TREE = 4


def check_inversion_join(args: "Args"):
    """the refusals of --inversion-join that need no device"""
    if args.inversion_join < 0:
        raise SeqRushError(-1, f"--inversion-join needs a non-negative integer, got {args.inversion_join}")
    if args.inversion_join and not args.patch_inversions:
        raise SeqRushError(-1, "--inversion-join is an option of --patch-inversions: give both")
    if args.inversion_join and args.inversion_join > (args.inversion_min_size or 2 * args.min_match_length):
        raise SeqRushError(-1, f"--inversion-join {args.inversion_join} is above the gap threshold of --patch-inversions "
                               f"({args.inversion_min_size or 2 * args.min_match_length}): an island would be a candidate by itself")


def inversion_join_report(js: dict) -> str:
    """the -v line of --inversion-join"""
    return (f"Inversion join: {js['islands_absorbed']} match islands absorbed into candidate gaps, "
            f"{js['rejected_site_cost']} jobs rejected by site cost")


def append_inversion_paf(ctx: Context, seqset: SeqSet, path: str, on: bool = True):
    """--output-alignments with --patch-inversions: the accepted patches after the main records, tagged sr:Z:inv"""
    if not on or ctx.inversion_stats()["candidates"] == 0:
        return
    al = ctx.inversion_alignments()
    al.append_paf(seqset, path, "sr:Z:inv")
    al.close()


def _ops_array(ops):
    a = np.ascontiguousarray(ops, dtype=np.uint32)
    return a, a.ctypes.data_as(C.POINTER(C.c_uint32))


def _sites(p, n):
    return [dict(query_start=int(p[i].query_start), query_end=int(p[i].query_end), target_start=int(p[i].target_start),
                 target_end=int(p[i].target_end), kind=int(p[i].kind), candidate=bool(p[i].candidate)) for i in range(n)]


def inversion_sites_host(ops, min_size: int):
    """the gaps of one alignment (ops in the sr_alignments encoding, (len << 4) | 0 '=' 1 X 2 I 3 D) -> list of dicts;
    kind 1 divergent, 2 query-only, 3 target-only (src/cigar_analysis.rs:23-128)"""
    L = _lib.load()
    a, ap = _ops_array(ops)
    p = C.POINTER(InvSiteC)(); cnt = C.c_uint64()
    check(L.sr_inversion_sites_host(ap, len(a), int(min_size), C.byref(p), C.byref(cnt)))
    out = _sites(p, cnt.value)
    L.sr_free(C.cast(p, C.c_void_p))
    return out


def inversion_candidate(qgap: int, tgap: int, min_size: int) -> bool:
    r = _lib.load().sr_inversion_candidate(int(qgap), int(tgap), int(min_size))
    if r < 0:
        check(r)
    return r == 1


def inversion_sites_host_join(ops, min_size: int, join_below: int, scores: str = "0,5,8,2,24,1"):
    """the joined rule over one alignment -> (list of site dicts, list of site costs)"""
    L = _lib.load()
    a, ap = _ops_array(ops)
    prm = Params(scores=scores)
    p = C.POINTER(InvSiteC)(); pc = C.POINTER(C.c_int32)(); cnt = C.c_uint64()
    check(L.sr_inversion_sites_host_join(ap, len(a), int(min_size), int(join_below), C.byref(prm.c), C.byref(p), C.byref(pc),
                                         C.byref(cnt)))
    out = _sites(p, cnt.value), [int(pc[i]) for i in range(cnt.value)]
    L.sr_free(C.cast(p, C.c_void_p)); L.sr_free(C.cast(pc, C.c_void_p))
    return out


def inversion_accept_site(patch_score: int, site_cost: int) -> bool:
    return _lib.load().sr_inversion_accept_site(int(patch_score), int(site_cost)) == 1


def inversion_scan_device_join(cigars, min_size: int, join_below: int, scores: str = "0,5,8,2,24,1", score=None, max_score=None,
                               device: int = 0):
    """tests: the joined device scan over a list of op arrays -> ([(alignment index, site dict, site cost)] in job order,
    dict(scanned, sites, candidates, islands))"""
    L = _lib.load()
    off = np.zeros(len(cigars) + 1, dtype=np.uint64)
    np.cumsum([len(c) for c in cigars], out=off[1:])
    a, ap = _ops_array(np.concatenate([np.asarray(c, dtype=np.uint32) for c in cigars]) if len(cigars) else [])
    prm = Params(scores=scores)
    i32p = lambda v: None if v is None else np.ascontiguousarray(v, dtype=np.int32)      # noqa: E731
    sc, mx = i32p(score), i32p(max_score)
    ptr = lambda v: None if v is None else v.ctypes.data_as(C.POINTER(C.c_int32))        # noqa: E731
    p = C.POINTER(InvSiteC)(); ow = C.POINTER(C.c_uint64)(); pc = C.POINTER(C.c_int32)(); cnt = C.c_uint64()
    st = (C.c_uint64 * 4)()
    check(L.sr_inversion_scan_device_join(device, ap, off.ctypes.data_as(C.POINTER(C.c_uint64)), len(cigars), int(min_size),
                                          int(join_below), C.byref(prm.c), ptr(sc), ptr(mx), C.byref(p), C.byref(ow), C.byref(pc),
                                          C.byref(cnt), st))
    sites = _sites(p, cnt.value)
    out = [(int(ow[i]), sites[i], int(pc[i])) for i in range(cnt.value)]
    for q in (p, ow, pc):
        L.sr_free(C.cast(q, C.c_void_p))
    return out, dict(scanned=int(st[0]), sites=int(st[1]), candidates=int(st[2]), islands=int(st[3]))


def inversion_accept(patch_score: int, main_score: int) -> bool:
    return _lib.load().sr_inversion_accept(int(patch_score), int(main_score)) == 1


def inversion_scan_device(cigars, min_size: int, device: int = 0):
    """tests: the device scan over a list of op arrays -> [(alignment index, site dict)] in job order"""
    L = _lib.load()
    off = np.zeros(len(cigars) + 1, dtype=np.uint64)
    np.cumsum([len(c) for c in cigars], out=off[1:])
    a, ap = _ops_array(np.concatenate([np.asarray(c, dtype=np.uint32) for c in cigars]) if len(cigars) else [])
    p = C.POINTER(InvSiteC)(); ow = C.POINTER(C.c_uint64)(); cnt = C.c_uint64()
    check(L.sr_inversion_scan_device(device, ap, off.ctypes.data_as(C.POINTER(C.c_uint64)), len(cigars), int(min_size),
                                     C.byref(p), C.byref(ow), C.byref(cnt)))
    sites = _sites(p, cnt.value)
    out = [(int(ow[i]), sites[i]) for i in range(cnt.value)]
    L.sr_free(C.cast(p, C.c_void_p)); L.sr_free(C.cast(ow, C.c_void_p))
    return out


def _take(L, p, shape, dtype):
    """copy a malloc'ed result array into numpy and sr_free it"""
    out = np.ctypeslib.as_array(p, shape=(max(1, int(np.prod(shape))),))[: int(np.prod(shape))].astype(dtype, copy=True).reshape(shape)
    L.sr_free(C.cast(p, C.c_void_p))
    return out


def sketch_device(seqset: SeqSet, kmer: int, device: int = 0):
    """tests: the sketch and Jaccard stages of `tree:` selection as the load path runs them -> (sketch (n, 1000) u64 with the
    unwritten entries still 2^64-1, sketch_n (n,) u32, shared (n, n) u32, denom (n, n) u32)"""
    L = _lib.load()
    sk = C.POINTER(C.c_uint64)(); skn = C.POINTER(C.c_uint32)(); sh = C.POINTER(C.c_uint32)(); dn = C.POINTER(C.c_uint32)()
    check(L.sr_sketch_device(device, C.byref(seqset.c), int(kmer), C.byref(sk), C.byref(skn), C.byref(sh), C.byref(dn)))
    n = seqset.n
    return (_take(L, sk, (n, 1000), np.uint64), _take(L, skn, (n,), np.uint32), _take(L, sh, (n, n), np.uint32),
            _take(L, dn, (n, n), np.uint32))


def knn_select_device(shared, denom, k_nearest: int, k_farthest: int, device: int = 0) -> np.ndarray:
    """tests: the selection stage on given (n, n) shared / denom matrices -> sel (n, n) u8, bit 0 nearest, bit 1 farthest"""
    L = _lib.load()
    sh = np.ascontiguousarray(shared, dtype=np.uint32); dn = np.ascontiguousarray(denom, dtype=np.uint32)
    n = sh.shape[0]
    if sh.shape != (n, n) or dn.shape != (n, n):
        raise ValueError("shared / denom must be square and of one shape")
    p = C.POINTER(C.c_uint8)()
    u32p = C.POINTER(C.c_uint32)
    check(L.sr_knn_select_device(device, sh.ctypes.data_as(u32p), dn.ctypes.data_as(u32p), n, int(k_nearest), int(k_farthest),
                                 C.byref(p)))
    return _take(L, p, (n, n), np.uint8)


def rust_f64(x: float) -> str:
    """an f64 the way Rust's Display prints it: shortest round-trip digits, never an exponent, no '.0' on integers"""
    import decimal
    r = repr(float(x))
    if r in ("inf", "-inf", "nan"):
        return {"inf": "inf", "-inf": "-inf", "nan": "NaN"}[r]
    s = format(decimal.Decimal(r), "f")
    if "." in s:
        s = s.rstrip("0").rstrip(".")
    return s


def iterative_report(st: dict, verbose: bool = False):
    """the reference's stdout lines after phase 1 (src/seqrush.rs:1024-1131) from iterative_stats(); the per-pair
    progress lines of its -v phase 1 are not printed"""
    out = [f"Phase 1 complete: {st['post_tree']} components after tree pairs",
           "\nPhase 2: Processing random pairs with early stopping..."]
    prev = st["post_tree"]
    nchk = len(st["check_counts"])
    for k, c in enumerate(st["check_counts"]):
        if verbose:
            out.append(f"  After {(k + 1) * 10} random pairs: {c} components (prev: {prev})")
        stop = st["stabilized"] and k == nchk - 1
        if stop:
            m, r = (k + 1) * 10, st["random_entries"]
            out.append(f"Graph stabilized after {m} random pairs ({c} components)")
            out.append(f"Skipped {r - m} random pairs ({rust_f64((r - m) / r * 100.0)}% reduction)")
        prev = c
    out.append(f"\nFinal component count: {st['final_components']}")
    return out


def uf_count_components_host(nodes: np.ndarray, total_len: int) -> int:
    """count_components (src/seqrush.rs:341-353) of a SeqRush node array on the host: roots among nodes [0, 2T)"""
    nodes = np.ascontiguousarray(nodes, dtype=np.uint64)
    out = C.c_uint64()
    check(_lib.load().sr_uf_count_components_host(nodes.ctypes.data_as(C.POINTER(C.c_uint64)), len(nodes), total_len,
                                                  C.byref(out)))
    return int(out.value)


def iterative_stop_host(counts, post_tree: int) -> int:
    """the stop rule over per-check counts -> checks consumed when it fired (0 = it never fired)"""
    counts = [int(c) for c in counts]
    arr = np.ascontiguousarray(counts or [0], dtype=np.uint64)
    out = C.c_uint64()
    check(_lib.load().sr_iterative_stop_host(arr.ctypes.data_as(C.POINTER(C.c_uint64)), len(counts), post_tree, C.byref(out)))
    return int(out.value)


def iterative_pair_lists(n: int, sel, params: Params):
    """the two entry lists of --iterative for an n*n k-NN selection (sel[i, j]: j picked by i; None = none)
    -> (tree [(i, j)], random [(i, j)])"""
    L = _lib.load()
    selp = None
    if sel is not None:
        sel = np.ascontiguousarray(sel, dtype=np.uint8).reshape(-1)
        assert len(sel) == n * n
        selp = sel.ctypes.data_as(C.POINTER(C.c_uint8))
    P = lambda: C.POINTER(C.c_uint32)()     # noqa: E731
    ti, tj, ri, rj = P(), P(), P(), P()
    tc, rc = C.c_uint64(), C.c_uint64()
    check(L.sr_iterative_pair_lists(n, selp, C.byref(params.c), C.byref(ti), C.byref(tj), C.byref(tc), C.byref(ri), C.byref(rj),
                                    C.byref(rc)))
    tree = [(int(ti[k]), int(tj[k])) for k in range(tc.value)]
    rnd = [(int(ri[k]), int(rj[k])) for k in range(rc.value)]
    for a in (ti, tj, ri, rj):
        L.sr_free(C.cast(a, C.c_void_p))
    return tree, rnd


def pair_list(n: int, params: Params):
    """This rank's ordered (query, target) pair list (host only)."""
    L = _lib.load()
    q = C.POINTER(C.c_uint32)(); t = C.POINTER(C.c_uint32)(); cnt = C.c_uint64()
    check(L.sr_pair_list(n, C.byref(params.c), C.byref(q), C.byref(t), C.byref(cnt)))
    m = int(cnt.value)
    out = [(int(q[i]), int(t[i])) for i in range(m)]
    L.sr_free(C.cast(q, C.c_void_p)); L.sr_free(C.cast(t, C.c_void_p))
    return out


MIRROR_NONE, MIRROR_SECONDARY = 0xffffffff, 0x80000000


def mirror_map(pairs, batch_first=None, workgroups=0):
    """The blocked kernel's mirror partners of an ordered pair list that runs in the given batches (host only;
    include/seqrush_amd.h sr_mirror_map) -> (entries, primaries): entries[i] = partner's index inside i's batch, | MIRROR_SECONDARY
    on the pair that is not aligned by itself, MIRROR_NONE = no partner.  batch_first: nbatch + 1 pair indices, None = one batch;
    workgroups: what the launch has -- a batch with no more pairs than that gets no partners (0: pair every batch)"""
    L = _lib.load()
    m = len(pairs)
    q = np.ascontiguousarray([a for a, _ in pairs] or [0], dtype=np.uint32)
    t = np.ascontiguousarray([b for _, b in pairs] or [0], dtype=np.uint32)
    out = np.zeros(max(m, 1), dtype=np.uint32)
    n = C.c_uint64()
    PU = C.POINTER(C.c_uint32)
    bf = None if batch_first is None else np.ascontiguousarray(batch_first, dtype=np.uint32)
    check(L.sr_mirror_map(q.ctypes.data_as(PU), t.ctypes.data_as(PU), m, None if bf is None else bf.ctypes.data_as(PU),
                          0 if bf is None else len(bf) - 1, int(workgroups), out.ctypes.data_as(PU), C.byref(n)))
    return [int(x) for x in out[:m]], int(n.value)
