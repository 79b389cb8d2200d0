"""Inputs of the resident-context tests (test_resident_host.py, test_resident_gpu.py) and the oracle's answers on them.

The resident context is loaded again and again by a long-running host, on a stream the host
chooses.  What a reload can get wrong only shows when consecutive loads DIFFER: another kernel family, another alphabet,
other sizes, other optional buffers.  So the inputs here are the smallest shapes that still take each path, chosen to differ
from their neighbours in the reload chain, and test_resident_host.py asserts that they do, from the oracle alone.

  A   6 x 400 bp SNP family with reverse-complemented members, default penalties, plain ACGT: the blocked kernel with every
      optional device buffer (orientation kernel and sorted dequeue order, mirror partners, tail list, three batches)
  B   3 x 790 bp with N runs, an IUPAC code and a soft-masked stretch, penalties that have no blocked instance: the
      level-per-pass kernel on 4-bit symbols, no knobs, one batch.  (The alphabet cases of test_gpu_parity.py are 900 bp long;
      three of those hold more bases than A, and B has to be smaller than A in every size, so each is cut to 790 bp.)
  C   4 x 300 bp, as a PAF file written from the oracle's alignments (load_paf)
  D   the `never` case of test_iterative_gpu.CASES (load_iterative)
  EI  the smallest inversion family of inversion_helpers with an accepted patch (enable_inversions)
  EX  the smallest split family of extend_inputs, its first half as the oracle's graph (load_extend)
  P   an explicit pair list over C's family (load_pairs)
  F   the failing loads: a set with an empty record, a pair list with an index out of range

Every oracle answer is computed once per process (functools.lru_cache) and handed out read-only."""
import functools

import numpy as np

import extend_inputs as ei
import inversion_helpers as ih
import oracle_binding as ob
from seqrush_amd import synth
from test_gpu_parity import ALPHA_CASES, oracle_params
from test_iterative_gpu import CASES as ITER_CASES, restate as iter_restate

# knobs a load reads; the GPU module clears all of them before it sets those of an input
KNOBS = ("SR_PREORIENT", "SR_TAIL", "SR_TAIL_THREADS", "SR_TAIL_ROUNDS", "SR_CIGAR_ARENA_OPS", "SR_NWG", "SR_ALIGN_THREADS",
         "SR_NO_MIRROR", "SR_ALIGN_IMPL", "SR_NO_REORDER", "SR_MIRROR_REPLAY", "SR_NO_FUSED_UNITE")

A_N, A_LEN, A_BATCH_PAIRS = 6, 400, 12
# the arena holds A_BATCH_PAIRS pairs of (|q| + |t| + 2) reserved ops (the rule of test_batched_cigar_arena): 36 pairs -> 3 batches.
# Partners exist only in a batch with more pairs than workgroups, and the tail launch only beside a main launch narrower than
# the widest instance: 4 workgroups of 256 threads
A_ENV = {"SR_PREORIENT": "1", "SR_TAIL": "all", "SR_CIGAR_ARENA_OPS": str(A_BATCH_PAIRS * (2 * A_LEN + 2) + 100),
         "SR_NWG": "4", "SR_ALIGN_THREADS": "256"}
B_LEN = 790
B_KW = {"scores": "0,4,6,2,24,1"}                  # no blocked instance (test_raw_byte_alphabet_on_fallback_kernel...)
EI_NAME = "inv"
EX_FAMILY, EX_K = "indel8", 0
P_PAIRS = ((0, 1), (3, 2), (2, 2), (1, 0), (2, 3), (0, 3))


def input_a():
    return synth.snp_family(A_N, A_LEN, 0.05, 1701, rc_every=3)


def input_b():
    recs = ALPHA_CASES["n-runs"]()[:3]             # N runs and an R; the second record gets the soft-masked stretch
    return [(n, (s[:150] + s[150:420].lower() + s[420:] if i == 1 else s)[:B_LEN]) for i, (n, s) in enumerate(recs)]


def input_c():
    return synth.snp_family(4, 300, 0.04, 1703, rc_every=2)


def input_d():
    mk, spec, k = ITER_CASES["never"]
    return mk(), spec, k


def input_ei():
    return list(ih.inputs(EI_NAME))


def input_ex():
    recs = ei.FAMILIES[EX_FAMILY]()
    return recs, len(recs) // 2


def input_f_empty():
    return [("a", b"ACGTACGTAC"), ("b", b"")]


F_BAD_PAIRS = [(0, 1), (0, 9)]


# ------------------------------------------------------------------ the oracle, once
def _ro(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def _runs(raw: bytes):
    """run-length (letter, length) of a per-column raw CIGAR"""
    out = []
    for b in raw:
        if out and out[-1][0] == b:
            out[-1][1] += 1
        else:
            out.append([b, 1])
    return out


def full_oracle(recs, pairs=None, **kw):
    """every pair aligned and united on the oracle -> what the device results are compared with: pairs, score, is_reverse,
    nops (run-length ops per CIGAR), cigar (= X I D strings), labels, gfa, gfa_compact, united_bases and match_runs (the
    bases and the number of the match runs of at least -k bases over all CIGARs: counters 4 and 5 of a pass)"""
    o = ob.OracleSeqRush(records=recs)
    op = oracle_params(**kw)
    n, k = o.n, kw.get("min_match_len", 0)
    plist = [(q, t) for q in range(n) for t in range(n)] if pairs is None else [tuple(p) for p in pairs]
    sc, rv, nops, cig, united, mruns = [], [], [], [], 0, 0
    for q, t in plist:
        a = o.align_pair(op, q, t)
        runs = _runs(a["cigar"])
        sc.append(a["score"]); rv.append(int(a["is_reverse"])); nops.append(len(runs))
        cig.append(ob.cigar_bytes_to_string(a["cigar"]))
        good = [ln for ch, ln in runs if ch == ord("M") and ln >= k]
        united += sum(good); mruns += len(good)
    if pairs is None:
        o.align_and_unite(op)
    else:
        o.align_and_unite_list(op, plist)
    gfa, nn, ne = o.gfa(canonical=True)
    out = dict(recs=list(recs), n=n, total_len=int(o.total_length), uf_size=2 * int(o.total_length) + 2, pairs=plist,
               score=_ro(np.array(sc, dtype=np.int32)), is_reverse=_ro(np.array(rv, dtype=np.uint8)),
               nops=_ro(np.array(nops, dtype=np.uint32)), cigar=cig, labels=_ro(o.canonical_labels()), gfa=gfa, nodes=nn, edges=ne,
               gfa_compact=ob.compact_gfa(gfa)[0], united_bases=united, match_runs=mruns)
    o.close()
    return out


def paf_text(recs, res):
    """the oracle's alignments as PAF lines in the layout sr_write_paf uses (12 columns, AS:i:, cg:Z:)"""
    lines = []
    for (q, t), sc, rv, cg in zip(res["pairs"], res["score"], res["is_reverse"], res["cigar"]):
        lq, lt = len(recs[q][1]), len(recs[t][1])
        ops = ih.letters_to_ops(cg)
        matches, alen = sum(o >> 4 for o in ops if o & 15 == 0), sum(o >> 4 for o in ops)
        lines.append(f"{recs[q][0]}\t{lq}\t0\t{lq}\t{'-' if rv else '+'}\t{recs[t][0]}\t{lt}\t0\t{lt}\t{matches}\t{alen}\t255\t"
                     f"AS:i:{int(sc)}\tcg:Z:{cg}")
    return "\n".join(lines) + "\n"


@functools.lru_cache(maxsize=None)
def oracle(name):
    """name: A, B, C, P (full_oracle, C with the key `paf`), D (test_iterative_gpu.restate + sizes), EI (inversion_helpers.restate
    + sizes and the plain run), EX (full_oracle of the whole family + `old_gfa`, the oracle's graph of the first half, and m)"""
    if name == "A":
        return full_oracle(input_a())
    if name == "B":
        return full_oracle(input_b(), **B_KW)
    if name == "C":
        res = full_oracle(input_c())
        res["paf"] = paf_text(input_c(), res)
        return res
    if name == "P":
        return full_oracle(input_c(), pairs=P_PAIRS)
    if name == "D":
        recs, spec, k = input_d()
        ref = dict(iter_restate(recs, spec, k))
        total = sum(len(s) for _, s in recs)
        ref.update(recs=recs, spec=spec, k=k, n=len(recs), total_len=total, uf_size=2 * total + 2,
                   pairs=[p for i, j in ref["tree"] + ref["random"] for p in ((i, i), (i, j), (j, i), (j, j))], labels=_ro(ref["labels"]))
        return ref
    if name == "EI":
        recs = input_ei()
        ref = dict(ih.restate(EI_NAME))
        total = sum(len(s) for _, s in recs)
        plain = full_oracle(recs, min_match_len=ih.K)
        ref.update(recs=recs, n=len(recs), total_len=total, uf_size=2 * total + 2, pairs=plain["pairs"], plain=plain,
                   is_reverse=plain["is_reverse"], labels=_ro(ref["labels"]))
        return ref
    if name == "EX":
        recs, m = input_ex()
        res = full_oracle(recs, min_match_len=EX_K)
        res["m"] = m
        res["old_gfa"] = full_oracle(recs[:m], min_match_len=EX_K)["gfa"]
        n = len(recs)
        res["ext_pairs"] = [(q, t) for q, t in res["pairs"] if not (q < m and t < m)]
        assert len(res["ext_pairs"]) == n * n - m * m
        return res
    raise KeyError(name)


# the reload chain of test_resident_gpu.py: successful loads by name, failing ones as F-empty / F-pair
CHAIN = ("A", "B", "F-empty", "C", "A", "D", "EI", "B", "EX", "F-pair", "A")


def chain_loads():
    """the chain without its failing loads: what the context holds, one after the other"""
    return [x for x in CHAIN if not x.startswith("F-")]


def sizes(name):
    r = oracle(name)
    pairs = r["ext_pairs"] if name == "EX" else r["pairs"]
    return dict(n=r["n"], total_len=r["total_len"], uf_size=r["uf_size"], pairs=len(pairs))
