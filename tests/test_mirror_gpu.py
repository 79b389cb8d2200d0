"""GPU tests (-m gpu) of mirrored emission: the blocked kernel aligns one of (q, t), (t, q) and writes the other
as the transposed CIGAR unless a tie-break decided something in the first.  Results must be bit for bit what they are with
SR_NO_MIRROR=1 and what the CPU oracle gives: strand, score, raw CIGAR bytes of every pair, the partition; the counters that
describe the alignment as the oracle counts it ([0]..[5]) must not move, the rows loaded and stored must fall.  Inputs and the
oracle's answers (once per process): tests/mirror_inputs.py.

A batch with no more pairs than the launch has workgroups gets no partners (sr_pairs.cpp mirror_map: every pair has a
workgroup of its own there and mirroring could only lengthen the launch), and these inputs have 25 to 64 pairs on a GPU
with a thousand workgroup slots.  So every case that is about mirroring runs with fewer workgroups than pairs (SR_NWG=8
unless the case sets its own): that is what "mirroring on" means for an input of this size.
test_a_workgroup_per_pair_means_no_partners runs the same inputs without the cap."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import mirror_inputs as mi
import oracle_binding as ob
from seqrush_amd.seqrush import SeqSet, Params, Context
from test_gpu_parity import oracle_params

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("SR_NO_MIRROR", "SR_NWG", "SR_BLK_LEVELS", "SR_FORCE_INT32", "SR_ALIGN_THREADS", "SR_POISON_ROWS", "SR_CIGAR_ARENA_OPS",
         "SR_PREORIENT", "SR_ALIGN_IMPL", "SR_NO_FUSED_UNITE")
MIRROR_ON = {"SR_NWG": "8"}           # fewer workgroups than any of the inputs has pairs
ORACLE_COUNTED = ("wf_cells", "wf_steps", "base_segments", "breakpoint_searches", "united_bases", "match_runs")


def run_ctx(recs, kw, fused=True, pairs=None):
    """one context, one pass (sr_ctx_run, or align + unite when not fused) -> everything the comparisons need"""
    ss = SeqSet(recs)
    ctx = Context(0)
    if pairs is None:
        ctx.load(ss, Params(**kw))
    else:
        ctx.load_pairs(ss, Params(**kw), pairs)
    rep = ctx.workspace_report()
    if fused:
        ctx.run()
    else:
        ctx.align(); ctx.unite()
    ctx.sync()
    al = ctx.alignments()
    out = dict(pairs=[(int(al.query_idx[i]), int(al.target_idx[i])) for i in range(al.n)],
               cigar=[al.raw_cigar_bytes(i) for i in range(al.n)], rev=[bool(x) for x in al.is_reverse[:al.n]],
               score=[int(x) for x in al.score[:al.n]], labels=ctx.download_labels(), cnt=ctx.counters(), rep=rep,
               kernel=ctx.align_kernel, ori=[x.tolist() for x in ctx.orientation_scores()])
    al.close(); ctx.close()
    return out


def set_env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def on_and_off(monkeypatch, recs, kw, env, oracle, fused=True):
    """the input with mirroring on and off under the same knobs: equal to each other and to the oracle; -> (on, off)"""
    env = dict(MIRROR_ON, **env)
    set_env(monkeypatch, env)
    on = run_ctx(recs, kw, fused)
    set_env(monkeypatch, dict(env, SR_NO_MIRROR="1"))
    off = run_ctx(recs, kw, fused)
    assert on["kernel"] == off["kernel"] == "sr_align_blk_kernel"
    assert off["rep"]["mirror_partners"] == 0 and off["cnt"]["mirror_pairs"] == 0 and off["cnt"]["mirror_ties"] == 0
    assert off["rep"]["knobs"].get("SR_NO_MIRROR") == "1" and "SR_NO_MIRROR" not in on["rep"]["knobs"]
    for i, (q, t) in enumerate(on["pairs"]):
        oa = oracle.pairs[q, t]
        for r, what in ((on, "mirroring on"), (off, "SR_NO_MIRROR=1")):
            assert r["rev"][i] == oa["is_reverse"], (what, q, t)
            assert r["score"][i] == oa["score"], (what, q, t)
            assert r["cigar"][i] == oa["cigar"], f"{what}: CIGAR differs from the oracle's on pair ({q},{t})"
    assert on["pairs"] == off["pairs"] and on["cigar"] == off["cigar"]
    # the orientation scores a mirrored secondary gets from its primary are what its own orientation search finds
    assert on["ori"] == off["ori"]
    assert np.array_equal(on["labels"], oracle.canonical_labels()) and np.array_equal(off["labels"], oracle.canonical_labels())
    for k in ORACLE_COUNTED:
        assert on["cnt"][k] == off["cnt"][k], (k, on["cnt"][k], off["cnt"][k])
    c = on["cnt"]
    assert c["mirror_pairs"] + c["mirror_ties"] == on["rep"]["mirror_partners"]
    return on, off


def row_bytes(r):
    return r["cnt"]["row_bytes_loaded"] + r["cnt"]["row_bytes_stored"]


def test_input_a(gpu, monkeypatch):
    """all three kinds of tie occur: the non-transposable pairs must all take the fallback, the others may mirror"""
    o = mi.oracle_once("A")
    nt = o.non_transposable()
    assert len(nt) >= 3
    on, off = on_and_off(monkeypatch, mi.input_a(), {}, {}, o)
    print("input A: non-transposable", len(nt), "mirror_pairs", on["cnt"]["mirror_pairs"], "mirror_ties", on["cnt"]["mirror_ties"],
          "row bytes on/off", row_bytes(on), row_bytes(off))
    assert on["rep"]["mirror_partners"] == 15
    assert on["cnt"]["mirror_ties"] >= len(nt)
    assert on["cnt"]["mirror_pairs"] >= 1
    assert row_bytes(on) < row_bytes(off)


def test_substitutions_only(gpu, monkeypatch):
    on, off = on_and_off(monkeypatch, mi.subst_only(), {}, {}, mi.oracle_once("subst"))
    assert on["cnt"]["mirror_pairs"] + on["cnt"]["mirror_ties"] == 28
    assert on["cnt"]["mirror_pairs"] > 0
    assert row_bytes(on) < row_bytes(off)


@pytest.mark.parametrize("pre", ["auto", "0", "1"])
def test_reverse_strand_pairs_are_never_mirrored(gpu, monkeypatch, pre):
    """one reverse-complemented member: its pairs align on the reverse strand and are aligned both ways, with the
    orientation inside the alignment kernel and as its own kernel"""
    o = mi.oracle_once("rc")
    rev_unordered = {(min(q, t), max(q, t)) for q, t in o.reverse_pairs()}
    assert len(rev_unordered) == 4
    on, off = on_and_off(monkeypatch, mi.one_reversed(), {}, {} if pre == "auto" else {"SR_PREORIENT": pre}, o)
    assert on["rep"]["mirror_partners"] == 10
    assert on["cnt"]["mirror_ties"] >= len(rev_unordered) + len(o.non_transposable())
    assert on["cnt"]["mirror_pairs"] <= 10 - len(rev_unordered)


ONE_PIECE = "0,5,8,2"
VARIANTS = {
    "nwg1": ({"SR_NWG": "1"}, {}),
    "nwg2": ({"SR_NWG": "2"}, {}),
    "levels5": ({"SR_BLK_LEVELS": "5"}, {}),
    "one-piece": ({}, {"scores": ONE_PIECE}),
    "int32": ({"SR_FORCE_INT32": "1"}, {}),
    "threads64": ({"SR_ALIGN_THREADS": "64", "SR_NWG": "3"}, {}),
    "preorient": ({"SR_PREORIENT": "1"}, {}),
    "min-match": ({}, {"min_match_len": 12}),
    "divergence": ({}, {"max_divergence": mi.A_DIVERGENCE}),
    "poison": ({"SR_POISON_ROWS": "37", "SR_NWG": "2"}, {}),
}


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_input_a_varied(gpu, monkeypatch, name):
    """Input A under the knobs and parameters that change what a workgroup carries from a primary through emission or
    fallback into its next pair (one and two workgroups for 36 pairs), the tile (5-level instance, one-piece penalties,
    32-bit searches, one-wave workgroups), the orientation route, the unite filter and what the rows held before"""
    env, kw = VARIANTS[name]
    o = mi.oracle_once("A", tuple(sorted(kw.items())))
    on, off = on_and_off(monkeypatch, mi.input_a(), kw, env, o)
    assert on["cnt"]["mirror_ties"] >= len(o.non_transposable()) and on["cnt"]["mirror_pairs"] >= 1
    if name == "nwg1":
        assert on["rep"]["workgroups"] == 1
    if name == "levels5":
        assert on["rep"]["block_levels"] == 5
    if name == "int32":
        assert on["rep"]["offset_bytes"] == 4
    if name == "threads64":
        assert on["rep"]["threads_per_workgroup"] == 64 and on["rep"]["wave_build"] == 1
    if name == "divergence":                      # the bound rejects some pairs and keeps others
        plain = mi.oracle_once("A")
        assert not np.array_equal(o.canonical_labels(), plain.canonical_labels())
        assert 0 < on["cnt"]["united_bases"] < run_ctx(mi.input_a(), {})["cnt"]["united_bases"]


@pytest.mark.parametrize("name", ["A", "rc"])
def test_a_workgroup_per_pair_means_no_partners(gpu, monkeypatch, name):
    """no cap on the workgroups: every pair of these inputs has a workgroup of its own, the launch lasts as long as its
    longest pair and a primary that aligned its secondary after itself would double it -- the load gives no pair a partner
    and the run is the one without mirroring"""
    set_env(monkeypatch, {})
    o = mi.oracle_once(name)
    r = run_ctx(mi.SETS[name](), {})
    assert r["rep"]["workgroups"] == len(r["pairs"]) and r["rep"]["mirror_partners"] == 0
    assert r["cnt"]["mirror_pairs"] == 0 and r["cnt"]["mirror_ties"] == 0
    assert r["cigar"] == [o.pairs[p]["cigar"] for p in r["pairs"]]
    assert np.array_equal(r["labels"], o.canonical_labels())


def test_unfused_path_equals_run(gpu, monkeypatch):
    """align() + unite() (sr_unite_kernel walks the mirrored CIGARs like any other) against sr_ctx_run (the workgroup unites
    the primary's runs and adds the secondary's tallies)"""
    o = mi.oracle_once("A")
    on_u, off_u = on_and_off(monkeypatch, mi.input_a(), {}, {}, o, fused=False)
    set_env(monkeypatch, MIRROR_ON)
    on_f = run_ctx(mi.input_a(), {}, fused=True)
    assert on_f["cnt"]["mirror_pairs"] >= 1
    assert on_f["cigar"] == on_u["cigar"] and np.array_equal(on_f["labels"], on_u["labels"])
    for k in ORACLE_COUNTED:
        assert on_f["cnt"][k] == on_u["cnt"][k] == off_u["cnt"][k], k


def bounds_child(path):
    """(child process, SEQRUSH_AMD_LIB = the bounds-checked library)"""
    oracle = pickle.load(open(path, "rb"))

    class MP:                                           # the two monkeypatch calls set_env uses
        @staticmethod
        def delenv(k, raising=False):
            os.environ.pop(k, None)

        @staticmethod
        def setenv(k, v):
            os.environ[k] = v
    for env in ({}, {"SR_NWG": "2"}):
        on, off = on_and_off(MP, mi.input_a(), {}, env, oracle)
        assert on["rep"]["kernel_build"] == "bounds" and on["cnt"]["mirror_pairs"] >= 1
        assert on["cnt"]["bounds_first"][0] == 0
    print("bounds build clean")


def test_bounds_checked_build(gpu, tmp_path):
    """the -DSR_BOUNDS instance on Input A, all workgroups and two: no access outside the workgroup's extent (it would
    raise SR_DEV_ERR_ADDRESS in the child).  A subprocess, because the library is chosen at load time"""
    lib = os.path.join(ROOT, "seqrush_amd", "libseqrush_amd_bounds.so")
    assert os.path.exists(lib), "build() did not make libseqrush_amd_bounds.so"
    path = tmp_path / "oracle.pkl"
    path.write_bytes(pickle.dumps(mi.oracle_once("A")))
    code = f"import sys; sys.path.insert(0, 'tests'); import test_mirror_gpu as t; t.bounds_child({str(path)!r})"
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(env, SEQRUSH_AMD_LIB=lib), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "bounds build clean" in r.stdout, (r.stdout[-800:], r.stderr[-1500:])


def test_explicit_list_on_the_device(gpu, monkeypatch):
    """the host test's list -- a secondary ahead of its primary, copies of both, an unpaired pair, self pairs -- on Input A"""
    from seqrush_amd.seqrush import mirror_map
    pairs = [(3, 1), (0, 2), (1, 3), (4, 4), (1, 3), (2, 0), (0, 5), (3, 1), (2, 2)]
    recs = mi.input_a()
    o = mi.oracle_once("A")
    oo = ob.OracleSeqRush(records=recs)
    oo.align_and_unite_list(oracle_params(), pairs)
    want_labels = oo.canonical_labels(); oo.close()
    for env in ({"SR_NWG": "2"}, {"SR_NWG": "1"}, {"SR_NWG": "2", "SR_NO_MIRROR": "1"}, {}):
        set_env(monkeypatch, env)
        r = run_ctx(recs, {}, pairs=pairs)
        assert r["pairs"] == pairs
        for i, (q, t) in enumerate(pairs):
            assert r["cigar"][i] == o.pairs[q, t]["cigar"] and r["score"][i] == o.pairs[q, t]["score"], (env, q, t)
        assert np.array_equal(r["labels"], want_labels)
        want = 0 if env.get("SR_NO_MIRROR") or not env else mirror_map(pairs, workgroups=int(env["SR_NWG"]))[1]
        assert want == (2 if env in ({"SR_NWG": "2"}, {"SR_NWG": "1"}) else 0)
        assert r["rep"]["mirror_partners"] == want == r["cnt"]["mirror_pairs"] + r["cnt"]["mirror_ties"]


def test_forced_batches_on_the_device(gpu, monkeypatch):
    """SR_CIGAR_ARENA_OPS cuts the list into batches that share the arena one after the other: partners in different batches
    are aligned on their own, the others mirror inside their batch (indices relative to the batch).  The host test's list in
    batches of two, then all 36 pairs in batches of about 13"""
    from seqrush_amd.seqrush import mirror_map
    recs = mi.input_a()
    o = mi.oracle_once("A")
    longest = max(len(s) for _, s in recs)
    split = [(0, 1), (0, 2), (1, 0), (2, 0), (1, 2), (2, 1)]
    for pairs, per_batch, env in ((split, 2, {"SR_NWG": "1"}), (None, 13, {"SR_NWG": "4"}), (None, 13, {"SR_NWG": "1"})):
        set_env(monkeypatch, dict(env, SR_CIGAR_ARENA_OPS=str(per_batch * (2 * longest + 2))))
        ss = SeqSet(recs); ctx = Context(0)
        if pairs is None:
            ctx.load(ss, Params())
        else:
            ctx.load_pairs(ss, Params(), pairs)
        rep = ctx.workspace_report()
        al = ctx.align_all(unite=True); ctx.sync()
        cnt = ctx.counters()
        if pairs is not None:
            assert ctx.num_batches == 3 and rep["mirror_partners"] == mirror_map(pairs, [0, 2, 4, 6], workgroups=1)[1] == 1
        else:
            assert ctx.num_batches >= 3 and 0 < rep["mirror_partners"] < 15
            assert cnt["mirror_pairs"] >= 1
            assert np.array_equal(ctx.download_labels(), o.canonical_labels())
        assert cnt["mirror_pairs"] + cnt["mirror_ties"] == rep["mirror_partners"]
        for i in range(al.n):
            oa = o.pairs[int(al.query_idx[i]), int(al.target_idx[i])]
            assert al.raw_cigar_bytes(i) == oa["cigar"] and int(al.score[i]) == oa["score"] and bool(al.is_reverse[i]) == oa["is_reverse"]
        al.close(); ctx.close()
