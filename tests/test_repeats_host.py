"""CPU tests (-m "not gpu") on low-complexity, repeat and palindromic inputs (tests/repeat_inputs.py): the oracle is the
yardstick of the device suite (test_repeats_gpu.py), so it is pinned on these inputs first -- scores against the
independent Gotoh DP, CIGARs that cost their score -- together with the host consumers of a partition (graph induction,
compaction, the Ygs sort) on graphs with self-loops and self-reverse-complement edges.  Every assertion is exact."""
import hashlib

import numpy as np
import pytest

import oracle_binding as ob
import repeat_inputs as ri
import sort_helpers as sh
from seqrush_amd import synth
from seqrush_amd.seqrush import SeqSet, build_gfa, build_gfa_from_nodes, sgd_layout, sort_gfa
from conftest import canon_gfa
from test_oracle_golden import P1, P2, consumption

TWIN = -1
# the five penalty sets of test_oracle_golden.test_wfa_optimal_vs_gotoh_random
PENS = [P1, P2, ob.Penalties.of(0, 1, 1, 1), ob.Penalties.of(0, 4, 6, 2, 12, 1), ob.Penalties.of(0, 3, 0, 1)]
ORI = ob.Penalties.of(0, 1, 1, 1)                      # the default --orientation-scores


# ------------------------------------------------------------------------------------------ 1. oracle scores and CIGARs
@pytest.mark.parametrize("family", sorted(ri.SMALL_FAMILIES))
def test_oracle_optimal_on_every_pair(family):
    """every ordered pair of the family under five penalty sets: plain WFA (full history), biWFA and the score-only WFA
    give the Gotoh DP's score; both CIGARs consume both sequences and cost that score.  For the mutated families at least
    one pair has two different co-optimal CIGARs (full history != biWFA under 0,5,8,2,24,1): the inputs do hold the ties
    the device must break like the oracle's biWFA"""
    recs = ri.SMALL_FAMILIES[family]()
    differ = 0
    for qn, q in recs:
        for tn, t in recs:
            for pen in PENS:
                g = ob.gotoh(q, t, pen)
                cig = {}
                for mode in (ob.MEM_HIGH, ob.MEM_ULTRALOW):
                    raw, s = ob.wfa_align(q, t, pen, mode)
                    assert s == g, (qn, tn, mode)
                    assert consumption(raw) == (len(q), len(t)), (qn, tn, mode)
                    assert ob.cigar_score(raw, q, t, pen) == g, (qn, tn, mode)
                    cig[mode] = raw
                assert ob.wfa_score(q, t, pen) == g, (qn, tn)
                differ += pen is P2 and cig[ob.MEM_HIGH] != cig[ob.MEM_ULTRALOW]
    if family in ri.MUTATED_FAMILIES:
        assert differ >= 1, "no pair of this family has two co-optimal CIGARs: pick another seed"


def test_palindromes_score_equally_on_both_strands_and_stay_forward():
    """orientation at equality: a query equal to its own reverse complement scores the same forward and reverse against
    every target, and the forward strand wins ("reverse iff strictly lower").  The near-palindromes put the two scores one
    apart, in both directions.  On every pair of the family the oracle's strand is the one the two scores dictate"""
    pal = ri.palindromes()
    d = dict(pal)
    idx = {n: i for i, (n, _) in enumerate(pal)}
    o = ob.OracleSeqRush(records=pal)
    op = ob.default_params()
    fwd, rev, strand = {}, {}, {}
    for qn, q in pal:
        for tn, t in pal:
            fwd[qn, tn] = ob.wfa_score(q, t, ORI)
            rev[qn, tn] = ob.wfa_score(synth.reverse_complement(q), t, ORI)
            strand[qn, tn] = o.align_pair(op, idx[qn], idx[tn])["is_reverse"]
            assert strand[qn, tn] == (rev[qn, tn] < fwd[qn, tn]), (qn, tn)
    for qn in ri.PALINDROMIC:
        assert d[qn] == synth.reverse_complement(d[qn])
        for tn, _ in pal:
            assert fwd[qn, tn] == rev[qn, tn] and strand[qn, tn] is False, (qn, tn)
    # near1 against near2: two mismatches forward, one reverse -> the reverse strand wins by one
    assert (fwd["near1", "near2"], rev["near1", "near2"], strand["near1", "near2"]) == (2, 1, True)
    assert (fwd["near2", "near1"], rev["near2", "near1"], strand["near2", "near1"]) == (2, 1, True)
    # near1 against near1b: one mismatch forward, two reverse -> the forward strand wins by one
    assert (fwd["near1", "near1b"], rev["near1", "near1b"], strand["near1", "near1b"]) == (1, 2, False)
    assert (fwd["near1b", "near1"], rev["near1b", "near1"], strand["near1b", "near1"]) == (1, 2, False)
    for n in ("near1", "near2", "near1b"):
        assert (fwd[n, n], rev[n, n], strand[n, n]) == (0, 2, False)


# ------------------------------------------------------------------------------------------ 2. partition and host consumers
def _oracle(recs, k=0, threads=8):
    o = ob.OracleSeqRush(records=recs)
    p = ob.default_params()
    p.min_match_len, p.threads = k, threads
    o.align_and_unite(p)
    return o


def self_edges(gfa):
    """(self-loop L lines x +/- x same sign, L lines that are their own reverse complement: x + x - or x - x +)"""
    L = [l.split("\t") for l in gfa.split("\n") if l.startswith("L\t")]
    return sum(f[1] == f[3] and f[2] == f[4] for f in L), sum(f[1] == f[3] and f[2] != f[4] for f in L)


@pytest.mark.parametrize("family", sorted(ri.SMALL_FAMILIES))
@pytest.mark.parametrize("k", [0, 8])
def test_partition_does_not_depend_on_the_thread_count(family, k):
    """a few huge components, united from many pairs at once: 1 thread and 8 give the same partition"""
    if family == "homopolymers_1500" and k:
        k = 1499                                        # (run length == k for the A x 1499 self pair)
    recs = ri.SMALL_FAMILIES[family]()
    assert np.array_equal(_oracle(recs, k, 1).canonical_labels(), _oracle(recs, k, 8).canonical_labels())


@pytest.mark.parametrize("name", sorted(ri.graph_cases()))
def test_host_induction_and_compaction_match_oracle_on_repeat_graphs(name):
    """sr_build_gfa, sr_build_gfa_opts(compact=1) and sr_build_gfa_from_nodes on the oracle's labels / forest equal the
    oracle's graph and its compaction on graphs with a self-loop edge ("loops") and with an edge that is its own reverse
    complement ("selfrc": k1 == k2 in the edge table)"""
    recs, k = ri.graph_cases()[name]
    o = _oracle(recs, k)
    labels = o.canonical_labels()
    ss = SeqSet(recs)
    g_prod, nn, ne = build_gfa(ss, labels)
    g_orc, on, oe = o.gfa(canonical=True)
    assert (nn, ne) == (on, oe) and g_prod == g_orc
    assert canon_gfa(g_prod) == canon_gfa(o.gfa(canonical=True, faithful_scan=True)[0])
    loops, selfrc = self_edges(g_prod)
    if name == "loops":
        assert loops >= 1
    if name == "selfrc":
        assert selfrc >= 1
    gc_prod, cn, ce = build_gfa(ss, labels, compact=True)
    gc_orc, con, coe = ob.compact_gfa(g_orc)
    assert (cn, ce) == (con, coe) and canon_gfa(gc_prod) == canon_gfa(gc_orc)
    assert cn < nn
    o1 = _oracle(recs, k, threads=1)                   # a sequentially built forest: the reference's root rule
    gn_prod = build_gfa_from_nodes(ss, o1.nodes())
    gn_orc = o1.gfa(canonical=False)
    assert gn_prod == gn_orc
    gnc_prod, gnn, gne = build_gfa_from_nodes(ss, o1.nodes(), compact=True)
    gnc_orc, gon, goe = ob.compact_gfa(gn_orc[0])
    assert (gnn, gne) == (gon, goe) and canon_gfa(gnc_prod) == canon_gfa(gnc_orc)
    # every path of both graphs still spells its input
    for text in (g_prod, gc_prod):
        g = sh.Gfa.parse(text)
        assert {n: g.spell(st) for n, st in g.paths} == {n: s.decode() for n, s in recs}


# ------------------------------------------------------------------------------------------ 3. host sort on cyclic graphs
def _cyclic_graphs():
    out = {}
    for name, (recs, k) in ri.graph_cases().items():
        if name != "micro_k8":
            out[name] = (recs, _oracle(recs, k).gfa(canonical=True)[0])
    for name, recs in ri.tiny_cyclic_sets().items():
        g = _oracle(recs).gfa(canonical=True)[0]
        out["tiny_" + name] = (recs, g)
        out["tiny_" + name + "_compact"] = (recs, ob.compact_gfa(g)[0])
    return out


@pytest.mark.parametrize("name", sorted(_cyclic_graphs()))
def test_host_twin_sgd_and_sort_on_cyclic_graphs(name):
    """paths that visit one node many times, self-loops, self-reverse-complement edges: the host twin's SGD equals the
    Python restatement bit for bit, and the sorted graph is the same graph"""
    recs, text = _cyclic_graphs()[name]
    g = sh.Gfa.parse(text)
    for tpr in (7, 64):
        want = sh.sgd_batched(g, seed=9, iter_max=3, terms_per_round=tpr)
        got = sgd_layout(g.text(), device=TWIN, seed=9, iter_max=3, terms_per_round=tpr)
        assert got.tobytes() == want.tobytes(), tpr
    spell = {n: s.decode() for n, s in recs}
    sh.check_same_graph(g, g, want_spellings=spell)
    after = sh.Gfa.parse(sort_gfa(g.text(), device=TWIN))
    sh.check_same_graph(g, after, want_spellings=spell)
    assert sort_gfa(g.text(), device=TWIN) == sort_gfa(g.text(), device=TWIN)


# ------------------------------------------------------------------------------------------ 4. the generators
def _digest(recs):
    return hashlib.sha256(b"\0".join(n.encode() + b"\1" + s for n, s in recs)).hexdigest()


def test_generators_are_deterministic():
    for name, mk in ri.SMALL_FAMILIES.items():
        assert mk() == mk(), name
    assert ri.long_satellite() == ri.long_satellite()
    assert ri.sketch_set(with_long=True) == ri.sketch_set(with_long=True) and ri.iterative_family() == ri.iterative_family()
    assert [ri.random_repeat_set(s) for s in range(12)] == [ri.random_repeat_set(s) for s in range(12)]
    assert len({_digest(ri.random_repeat_set(s)[0]) for s in range(12)}) == 12
    # what the families promise
    homo = dict(ri.homopolymers() + ri.homopolymers_1500())
    for L in ri.HOMO_L + (1500,):
        for d in ri.HOMO_D:
            if L - d >= 1:
                assert homo[f"A{L}"] == b"A" * L and homo[f"A{L - d}"] == b"A" * (L - d)
    assert homo["N64"] == b"N" * 64
    lens = {n: len(s) for n, s in ri.microsatellites()}
    assert (lens["ACx58"] - lens["ACx50"], lens["CAGx45"] - lens["CAGx40"], lens["CAGx45p"] - lens["CAGx40"]) == (16, 15, 17)
    assert sorted(len(u) for u in ri.MICRO_UNITS) == [2, 3, 4, 6]
    assert [len(s) > 800 for _, s in ri.satellite()] == [True] * 5 and sum(n.endswith("rc") for n, _ in ri.satellite()) == 1
    assert all(set(s) <= set(b"AT") for _, s in ri.two_letter())
    long = ri.long_satellite()
    assert all(32000 < len(s) <= 57000 for _, s in long["ring34k"]) and all(11000 < len(s) < 13000 for _, s in long["deep12k"])
    for s in range(12):
        recs, k = ri.random_repeat_set(s)
        assert 2 <= len(recs) <= 6 and all(1 <= len(q) <= 450 for _, q in recs) and k in (0, 1, 5, 20)
    assert len(ri.iterative_family()) >= 12
    sk = dict(ri.sketch_set())
    assert sk["cag_a"] == sk["cag_b"] == sk["cag_c"] and set(sk["allN"]) == {ord("N")} and len(sk["short"]) < 16
    assert len(set(sk["homo"])) == 1
