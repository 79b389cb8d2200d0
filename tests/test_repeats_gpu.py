"""GPU parity tests (-m gpu) on low-complexity, repeat and palindromic inputs (tests/repeat_inputs.py).  On random
sequence an optimal alignment is locally unique; here whole bands of diagonals carry equal offsets, many diagonals meet at
one score in the breakpoint search, sequences equal their own reverse complement, sketches are tiny or exactly equal and a
few union-find roots take all the unites -- so what is compared with the oracle bit for bit (check_parity: CIGAR bytes,
strand, score, partition, canonical GFA, fused run against align + unite; every pair, no sampling) is the kernels' choice
between equal candidates.  Each case asserts from the context's report that it ran on the instance it is meant for."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_binding as ob
import repeat_inputs as ri
import sort_helpers as sh
from seqrush_amd.seqrush import Context, Params, SeqSet, build_gfa, sgd_layout, sort_gfa
from conftest import canon_gfa
from test_gpu_parity import check_parity, run_gpu
from test_iterative_gpu import expand, restate, run_product
from test_repeats_host import self_edges

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWIN = -1
BLK, BFS = "sr_align_blk_kernel", "sr_align_bfs_kernel"
FAMILIES = sorted(ri.SMALL_FAMILIES)


def report(recs, **kw):
    """the context's own account of how it will run these records under the current environment"""
    ctx = Context(0)
    ctx.load(SeqSet(recs), Params(**kw))
    rep = ctx.workspace_report()
    ctx.close()
    assert rep["kernel_build"] == ("default" if not os.environ.get("SEQRUSH_AMD_LIB") else rep["kernel_build"])
    return rep


def symbol_bits(recs):
    return 2 if all(set(s) <= set(b"ACGT") for _, s in recs) else 4


# (scores, environment) -> (kernel, block_levels, offset_bytes, ring_cell_bytes) the report must state
INSTANCES = {
    "default": ({}, {}, (BLK, 10, 2, 2)),
    "generic5": ({}, {"SR_BLK_LEVELS": "5"}, (BLK, 5, 2, 2)),
    "one-piece": ({"scores": "0,5,8,2"}, {}, (BLK, 10, 2, 2)),
    "level-2p": ({"scores": "0,4,6,2,12,1"}, {}, (BFS, 1, 2, 2)),
    "level-1p": ({"scores": "0,3,4,1"}, {}, (BFS, 1, 2, 2)),
    "level-wide": ({"scores": "0,3,40,1"}, {}, (BFS, 1, 2, 2)),
    "deep-scope": ({"scores": "0,5,8,2,60,1"}, {}, (BLK, 5, 2, 2)),
    "int32-ring16": ({}, {"SR_FORCE_INT32": "1", "SR_RING_U16": "1"}, (BLK, 10, 4, 2)),
    "int32-ring32": ({}, {"SR_FORCE_INT32": "1", "SR_RING_U16": "0"}, (BLK, 10, 4, 4)),
}


# ------------------------------------------------------------------------------------------ 1. families x kernel instances
@pytest.mark.parametrize("instance", list(INSTANCES))
@pytest.mark.parametrize("family", FAMILIES)
def test_family_on_kernel_instance(gpu, monkeypatch, family, instance):
    """wavefront ties (M / I1 / D1 / I2 / D2 predecessors at equal offsets), the breakpoint's walk-order field, extension
    that runs long on every diagonal across 16-symbol words into both sequence ends, clean gaps of 15 / 16 / 17 around the
    two gap pieces' crossover: every family through every alignment kernel instance"""
    kw, env, (kernel, levels, osz, rsz) = INSTANCES[instance]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    recs = ri.SMALL_FAMILIES[family]()
    rep = report(recs, **kw)
    assert (rep["block_levels"], rep["offset_bytes"], rep["ring_cell_bytes"]) == (levels, osz, rsz), rep
    assert rep["kernel_impl"] == (2 if kernel == BLK else 1) and rep["symbol_bits"] == symbol_bits(recs)
    assert rep["symbol_bits"] == (4 if family == "homopolymers" else 2)
    al, _, cnt = check_parity(recs, **kw)
    assert cnt["align_kernel"] == kernel
    assert al.n == len(recs) ** 2


@pytest.mark.parametrize("env", [{"SR_NWG": "1"}, {"SR_NWG": "2", "SR_POISON_ROWS": "37"}], ids=["1wg", "2wg-poisoned"])
@pytest.mark.parametrize("family", FAMILIES)
def test_state_carried_between_pairs(gpu, monkeypatch, family, env):
    """one or two workgroups align every pair one after the other: a repeat pair leaves plausible offsets behind in the ring,
    the LDS tables and the registers; rows poisoned with a plausible offset before the run"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    recs = ri.SMALL_FAMILIES[family]()
    rep = report(recs)
    assert rep["workgroups"] == int(env["SR_NWG"]) and rep["block_levels"] == 10, rep
    _, _, cnt = check_parity(recs)
    assert cnt["align_kernel"] == BLK


@pytest.mark.parametrize("threads", ["64", "512"])
@pytest.mark.parametrize("family", [f for f in FAMILIES if f != "homopolymers"])
def test_workgroup_sizes(gpu, monkeypatch, family, threads):
    """one-wave workgroups (the lean build: 2-bit symbols only, hence not the family with an N member) and 8 waves"""
    monkeypatch.setenv("SR_ALIGN_THREADS", threads)
    recs = ri.SMALL_FAMILIES[family]()
    rep = report(recs)
    assert rep["threads_per_workgroup"] == int(threads) and rep["block_levels"] == 10 and rep["symbol_bits"] == 2, rep
    _, _, cnt = check_parity(recs)
    assert cnt["align_kernel"] == BLK


def test_workgroup_size_512_with_4bit_symbols(gpu, monkeypatch):
    monkeypatch.setenv("SR_ALIGN_THREADS", "512")
    recs = ri.homopolymers()
    rep = report(recs)
    assert rep["threads_per_workgroup"] == 512 and rep["symbol_bits"] == 4, rep
    check_parity(recs)


# ------------------------------------------------------------------------------------------ 2. orientation
ORIENT_REGIMES = {"in-kernel": {"SR_PREORIENT": "0"}, "orient-kernel": {"SR_PREORIENT": "1"},
                  "orient-kernel-no-kbits": {"SR_PREORIENT": "1", "SR_NO_KBITS": "1"}}
_STRANDS = {}


@pytest.mark.parametrize("regime", list(ORIENT_REGIMES))
@pytest.mark.parametrize("family", ["palindromes", "satellite", "two_letter"])
def test_orientation_at_and_next_to_equality(gpu, monkeypatch, family, regime):
    """a sequence equal to its own reverse complement scores the same on both strands: forward must win.  (AT)n and (ACGT)n
    put every 8-mer of the reverse complement into the target's set (reverse bound 0: no early decision), the
    near-palindromes put the two scores one apart (both ways).  Orientation inside the alignment kernel, as its own
    kernel, and without the 8-mer bound: strands and scores equal the oracle's in every regime and hence each other's"""
    for k, v in ORIENT_REGIMES[regime].items():
        monkeypatch.setenv(k, v)
    recs = ri.SMALL_FAMILIES[family]()
    names = [n for n, _ in recs]
    al, _, _ = check_parity(recs)
    strand = {(names[int(q)], names[int(t)]): bool(r) for q, t, r in zip(al.query_idx, al.target_idx, al.is_reverse)}
    if family == "palindromes":
        for q in ri.PALINDROMIC:
            assert not any(strand[q, t] for t in names), q
        assert strand["near1", "near2"] and strand["near2", "near1"]                 # reverse lower by one
        assert not strand["near1", "near1b"] and not strand["near1b", "near1"]       # forward lower by one
        assert not strand["near1", "near1"]
    if family == "satellite":
        rcm = [n for n in names if n.endswith("rc")]
        assert all(strand[q, t] == ((q in rcm) != (t in rcm)) for q in names for t in names)
    key = (family, tuple(al.is_reverse.tolist()), tuple(al.score.tolist()))
    assert _STRANDS.setdefault(family, key) == key, "the orientation regimes disagree with each other"
    # other orientation penalties move where the two strands tie
    check_parity(recs, orientation_scores="0,2,3,1")


# ------------------------------------------------------------------------------------------ 3. -k
@pytest.mark.parametrize("k", [0, 1, 8, 64])
@pytest.mark.parametrize("family", ["microsatellites", "satellite"])
def test_min_match_len_on_repeats(gpu, family, k):
    """run length == k is the boundary of the unite: microsatellite units between substitutions give many match runs of
    exactly one length"""
    _, _, cnt = check_parity(ri.SMALL_FAMILIES[family](), min_match_len=k)
    assert cnt["match_runs"] > 0


# ------------------------------------------------------------------------------------------ 4. long pairs
@pytest.mark.parametrize("env", [{}, {"SR_NWG": "1"}], ids=["default", "1wg"])
def test_34kb_satellite_pair_on_the_16bit_ring(gpu, monkeypatch, env):
    """32-bit searches whose ring is 16 bits per cell (the packed tile), on satellite arrays: off-diagonal extension runs
    for a whole unit at every multiple of 171"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    recs = ri.long_satellite()["ring34k"]
    rep = report(recs)
    assert (rep["offset_bytes"], rep["ring_cell_bytes"], rep["block_levels"]) == (4, 2, 10), rep
    check_parity(recs)


def test_12kb_satellite_pair_deep_levels(gpu):
    """~10 % divergence: a search thousands of levels deep (past SR_DEEP_INT16, where creeping NULLs are reset) on arrays
    whose shifted diagonals stay alive"""
    recs = ri.long_satellite()["deep12k"]
    rep = report(recs)
    assert (rep["offset_bytes"], rep["ring_cell_bytes"], rep["block_levels"]) == (2, 2, 10), rep
    al, _, _ = check_parity(recs)
    assert max(int(x) for x in al.score) > 2 * 3000


# ------------------------------------------------------------------------------------------ 5. bounds-checked build
def test_bounds_checked_build_on_repeats(gpu):
    """the -DSR_BOUNDS instance of the blocked kernel: homopolymer, microsatellite, palindrome and satellite families run
    clean (no SR_DEV_ERR_ADDRESS) and equal the oracle.  A subprocess, because the library is chosen at load time."""
    lib = os.path.join(ROOT, "seqrush_amd", "libseqrush_amd_bounds.so")
    assert os.path.exists(lib), "build() did not make libseqrush_amd_bounds.so"
    code = ("import sys; sys.path.insert(0, 'tests'); import torch; import test_gpu_parity as t; import repeat_inputs as ri\n"
            "from seqrush_amd.seqrush import SeqSet, Params, Context\n"
            "c = Context(0); c.load(SeqSet(ri.palindromes()), Params()); assert c.workspace_report()['kernel_build'] == 'bounds'; c.close()\n"
            "for f in ('homopolymers', 'homopolymers_1500', 'microsatellites', 'palindromes', 'satellite'):\n"
            "    t.check_parity(ri.SMALL_FAMILIES[f]())\n"
            "print('bounds build clean')\n")
    for nwg in ("", "2"):
        env = dict(os.environ, SEQRUSH_AMD_LIB=lib)
        if nwg:
            env["SR_NWG"] = nwg
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and "bounds build clean" in r.stdout, (r.stdout[-800:], r.stderr[-1500:])


# ------------------------------------------------------------------------------------------ 6. sparsification
@pytest.mark.parametrize("with_long", [False, True], ids=["low-complexity", "with-1000-kmer-members"])
@pytest.mark.parametrize("spec", ["tree:2,1,0.1,4", "tree:3,3,0.1", "tree:2,2,0.0,32", "tree:1", "connectivity:0.9", "auto"])
def test_sparsified_pair_lists_on_degenerate_sketches(gpu, spec, with_long):
    """sketches with one distinct k-mer (homopolymer), none (all N, shorter than k) and byte-identical members, whose
    Jaccard fractions are exactly equal so that sr_knn_select_kernel's "lower index first" decides; with members of more
    than 1 000 distinct k-mers the sketch cut and the short sketches meet in one Jaccard walk.  The pair list equals the
    oracle's and so does the partition over it"""
    recs = ri.sketch_set(with_long=with_long)
    ss = SeqSet(recs); ctx = Context(0); ctx.load(ss, Params(sparsification=spec))
    pairs = ctx.pairs()
    o = ob.OracleSeqRush(records=recs)
    assert pairs == o.sparsified_pairs(spec)
    assert all((q, q) in set(pairs) for q in range(len(recs)))
    ctx.run(); ctx.sync(); labels = ctx.download_labels(); ctx.close()
    op = ob.default_params(); op.threads = 8
    o.align_and_unite_list(op, pairs)
    assert np.array_equal(labels, o.canonical_labels())
    if spec.startswith("tree:"):
        assert len(pairs) < len(recs) ** 2


# ------------------------------------------------------------------------------------------ 7. induction, compaction, sort
@pytest.mark.parametrize("name", sorted(ri.graph_cases()))
def test_device_induction_compaction_and_sort_on_repeat_graphs(gpu, name):
    """a few huge components (heavy contention on a few union-find roots), self-loop edges and edges equal to their own
    reverse complement (k1 == k2 in gi_edge_insert), paths that visit one node hundreds of times: device induction ==
    host induction on the downloaded labels byte for byte == the oracle canonically, with and without compaction; the
    device SGD is bit-identical to the host twin; the sorted graph is the same graph"""
    recs, k = ri.graph_cases()[name]
    ss = SeqSet(recs); ctx = Context(0); ctx.load(ss, Params(min_match_len=k)); ctx.run(); ctx.sync()
    dev = ctx.build_gfa()
    devc = ctx.build_gfa(compact=True)
    labels = ctx.download_labels()
    ctx.close()
    assert dev == build_gfa(ss, labels) and devc == build_gfa(ss, labels, compact=True)
    o = ob.OracleSeqRush(records=recs)
    op = ob.default_params(); op.threads = 8; op.min_match_len = k
    o.align_and_unite(op)
    assert np.array_equal(labels, o.canonical_labels())
    g_orc = o.gfa(canonical=True)
    assert canon_gfa(dev[0]) == canon_gfa(g_orc[0]) and dev[1:] == g_orc[1:]
    c_orc = ob.compact_gfa(g_orc[0])
    assert canon_gfa(devc[0]) == canon_gfa(c_orc[0]) and devc[1:] == c_orc[1:]
    loops, selfrc = self_edges(dev[0])
    assert name != "loops" or loops >= 1
    assert name != "selfrc" or selfrc >= 1
    spell = {n: s.decode() for n, s in recs}
    for text in (dev[0], devc[0]):
        for kw in ({}, {"terms_per_round": 64, "iter_max": 10}):
            assert sgd_layout(text, device=0, **kw).tobytes() == sgd_layout(text, device=TWIN, **kw).tobytes(), kw
        before = sh.Gfa.parse(text)
        out = sort_gfa(text, device=0)
        sh.check_same_graph(before, sh.Gfa.parse(out), want_spellings=spell)
        assert out == sort_gfa(text, device=TWIN)


# ------------------------------------------------------------------------------------------ 8. iterative mode
@pytest.mark.parametrize("spec,k", [("tree:1,0,1.0", 0), ("tree:1,1,1.0,8", 5)])
def test_iterative_on_a_repeat_family(gpu, spec, k):
    """--iterative over 14 satellite arrays (every fourth reverse-complemented) against the restatement over the oracle:
    entries, component counts after every check, the stop, labels and graph"""
    recs = ri.iterative_family()
    assert len(recs) >= 12
    ref = restate(recs, spec, k)
    st, labels, gfa, _ = run_product(recs, spec, k)
    assert (st["tree_entries"], st["random_entries"]) == (len(ref["tree"]), len(ref["random"]))
    assert st["pairs"] == expand(ref["tree"]) + expand(ref["random"])
    assert st["post_tree"] == ref["post_tree"] and st["check_counts"] == ref["check_counts"]
    assert st["checks"] == len(ref["check_counts"]) > 0
    assert st["stabilized"] == ref["stabilized"] and st["random_processed"] == ref["processed"]
    assert st["final_components"] == ref["final"]
    assert np.array_equal(labels, ref["labels"])
    assert canon_gfa(gfa) == canon_gfa(ref["gfa"])


# ------------------------------------------------------------------------------------------ 9. seeded mixtures
@pytest.mark.parametrize("seed", list(range(12)))
def test_randomised_repeat_sets(gpu, seed):
    """seeded mixtures of the families: 2-6 members of length 1..400, mutated, truncated, reverse-complemented, through
    every phase of the default kernels, then device induction against host induction"""
    recs, k = ri.random_repeat_set(seed)
    al, labels, cnt = check_parity(recs, min_match_len=k)
    ss = SeqSet(recs); ctx = Context(0); ctx.load(ss, Params(min_match_len=k)); ctx.align(); ctx.unite(); ctx.sync()
    dev = ctx.build_gfa(); ctx.close()
    assert dev == build_gfa(ss, labels)
