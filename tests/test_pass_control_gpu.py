"""GPU tests (-m gpu) of the blocked kernel's wave-0 section between two passes (sr_pass_rule.h, blk_setup of sr_blk_pass.inc,
the control and base-case sections of sr_align_blk.inc): the pass tables and the max_ak stores are written one (aligner,
level) pair per lane, 64 / B aligners per step, the phase-1 walk and the base cases' reach scan run on values read in one
batch.  None of it may change a result, so every case is bit-equality with the CPU oracle -- strand, score, raw CIGAR bytes,
canonical labels -- and the counts the oracle has of its own: breakpoint searches and base cases from its trace.  The
level count (wf_steps) is block-granular on the device and the cell count (wf_cells) includes the orientation and follows
the device's rules for a search's and a base case's last block; the oracle's trace carries neither.  Both are what this
change re-sums (cells_l, by LDS adds per (aligner, level) lane), so every case compares them with the figures the kernel
of the commit before this change gave on the same input and knobs (tests/golden/pass_control_counts.json, recorded on an
MI355X): an error common to every shape would show there.  (On the seam input the device's alignment cells are
368 391 023 and the cells of the oracle's traced alignments 368 039 913; the reverse aligner's level that the device counts
when a search ends with the forward aligner one level ahead explains 55 592 of the difference, the rest is not explained.)

Inputs are the smallest that reach each seam:
 * chunk seams -- two pairs whose recursions have levels of 3 and 4 searched segments (6 and 8 aligners: either side of the
   lane step at B = 10), of exactly 16, of 29 (16 + a ragged chunk of 13) and of 56 (three full chunks and one of 8).  The
   blocked kernel's translation unit sets SR_BFS_MAXACT to 16 segments (sr_align_blk.hip; the 32 of sr_internal.h is the
   level kernel's), so a full chunk -- BJ_MAX = 32 aligners, six lane steps at B = 10 -- is a level of 16 segments, and a
   level of 32 segments would be two such chunks one after the other, which the level of 56 contains.  The precondition is
   asserted on the oracle's trace;
 * the max_ak ring wrap inside a block -- a generic-instance penalty set whose ring depth is no multiple of B = 5;
 * base cases -- batches of 16 jobs and the re-queue (SR_TEST_BASE_LEVELS);
 * every instance shape on one small family."""
import json
import os
import pickle
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest

import deep_inputs as di
import instance_matrix as im
import mirror_inputs as mi
import oracle_binding as ob
import test_mirror_gpu as tm
import test_replay_gpu as tr
from seqrush_amd import synth
from test_gpu_parity import oracle_params

pytestmark = pytest.mark.gpu

ROOT = tm.ROOT
MAIN256 = {"SR_ALIGN_THREADS": "256"}
PRIO_KNOBS = ("SR_TILE_PRIO", "SR_WG_PER_CU", "SR_TEST_BASE_LEVELS", "SR_BFS_BASE_JOBS", "SR_RING_U16")
GENERIC_WRAP = "0,5,8,2,13,1"            # 5-level instance, ring of scope + B + 1 = 15 + 5 + 1 = 21 levels: a block wraps inside
_CACHE = {}
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "pass_control_counts.json")))


def clear(mp):
    tr.clear(mp)
    for k in PRIO_KNOBS:
        mp.delenv(k, raising=False)


def run(mp, recs, kw, env, pairs=None):
    clear(mp)
    tm.set_env(mp, env)
    for k, v in env.items():
        mp.setenv(k, v)
    return tm.run_ctx(recs, kw, pairs=pairs)


def _sim(L, seed, sub):
    a = synth.base_sequence(L, seed)
    return synth.to_bytes(a), synth.to_bytes(synth.substitute(a, sub, seed + 1))


def seam_records():
    """pair (0, 1): 1.5 kb of unrelated sequence in front of 4 kb at 4 % substitutions -- the recursion's levels search 1, 2, 3
    and 4 segments; pair (2, 3): the same two parts in front of 10 kb at 30 % -- 1, 2, 4, 8, 16, 29 and 56 segments"""
    u = (di.unique(1500, 9101), di.unique(1500, 9102))
    x = _sim(4000, 13200, 0.04)
    z = _sim(10000, 19300, 0.3)
    return [("a0", u[0] + x[0]), ("a1", u[1] + x[1]), ("b0", u[0] + x[0] + z[0]), ("b1", u[1] + x[1] + z[1])]


SEAM_PAIRS = [(0, 1), (2, 3)]


class PairsOracle:
    """the oracle's answers on an explicit pair list, computed once: alignments, labels, and from the trace of every pair the
    searched segments per recursion level, the base cases and the wavefront cells"""

    def __init__(self, recs, pairs, kw):
        o = ob.OracleSeqRush(records=recs)
        op = oracle_params(**kw)
        self.pairs = {(q, t): o.align_pair(op, q, t) for q, t in pairs}
        o.align_and_unite_list(op, pairs)
        self.labels = o.canonical_labels().copy()
        o.close()
        self.levels, self.searches, self.bases, self.cells = {}, 0, 0, 0
        for q, t in pairs:
            a = self.pairs[q, t]
            qs = synth.reverse_complement(recs[q][1]) if a["is_reverse"] else recs[q][1]
            cig, sc, tr_ = ob.wfa_align_traced(qs, recs[t][1], op.pen)
            assert cig == a["cigar"] and sc == a["score"]
            self.cells += int(ob.lib().sro_wfa_last_cells())
            c = Counter(x["depth"] for x in tr_ if x["kind"] == ob.TRACE_SEARCH)
            self.levels[q, t] = [c[d] for d in sorted(c)]
            self.searches += sum(c.values())
            self.bases += sum(1 for x in tr_ if x["kind"] == ob.TRACE_BASE)


def oracle_for(key, recs, pairs, kw):
    k = (key, tuple(sorted(kw.items())))
    if k not in _CACHE:
        _CACHE[k] = PairsOracle(recs, pairs, kw)
    return _CACHE[k]


def all_pairs(n):
    return [(q, t) for q in range(n) for t in range(n)]


def check(r, o, what, golden=None):
    """bit-equality with the oracle, the oracle's own counts, and cells and levels as the previous kernel counted them
    (golden: the key of the recorded figures, by default `what`; False: a run that has none)"""
    assert r["kernel"] == "sr_align_blk_kernel", what
    assert sorted(r["pairs"]) == sorted(o.pairs), what
    for i, (q, t) in enumerate(r["pairs"]):
        oa = o.pairs[q, t]
        assert r["rev"][i] == oa["is_reverse"], (what, q, t)
        assert r["score"][i] == oa["score"], (what, q, t)
        assert r["cigar"][i] == oa["cigar"], f"{what}: CIGAR differs from the oracle's on pair ({q},{t})"
    assert np.array_equal(r["labels"], o.labels), what
    c = r["cnt"]
    # (orientation in a kernel of its own: counter [6] holds its cells, the rest of wf_cells is the alignments')
    separate = r["rep"]["orientation_route"] != "in-kernel"
    align_cells = c["wf_cells"] - c["ticks_orientation"] if separate else None
    print(what, "searches", c["breakpoint_searches"], o.searches, "base cases", c["base_segments"], o.bases, "wf_cells", c["wf_cells"],
          "orientation", c["ticks_orientation"], "alignment cells", align_cells, "oracle", o.cells, "levels", c["wf_steps"],
          "passes", c["bp_passes"], "requeues", c["base_requeues"], "build", r["rep"]["kernel_build"], flush=True)
    assert c["breakpoint_searches"] == o.searches, (what, c["breakpoint_searches"], o.searches)
    assert c["base_segments"] == o.bases, (what, c["base_segments"], o.bases)
    if golden is not False:
        g = GOLDEN[golden or what]
        assert c["wf_cells"] == g["wf_cells"], (what, c["wf_cells"], g["wf_cells"])
        assert c["wf_steps"] == g["wf_steps"], (what, c["wf_steps"], g["wf_steps"])
    return c


def same_counts(a, b, what, keys=tm.ORACLE_COUNTED):
    for k in keys:
        assert a["cnt"][k] == b["cnt"][k], (what, k, a["cnt"][k], b["cnt"][k])


# ------------------------------------------------------------------------------------------ chunk seams
def test_chunk_seams(gpu, monkeypatch):
    recs = seam_records()
    o = oracle_for("seams", recs, SEAM_PAIRS, {})
    small, big = o.levels[0, 1], o.levels[2, 3]
    # the precondition, from the oracle's segment counts: 6 and 8 aligners, a full chunk, a ragged second chunk, > 32 segments
    assert 3 in small and 4 in small, small
    assert 16 in big and any(16 < n < 32 and n % 16 for n in big) and any(n > 32 for n in big), big
    r10 = run(monkeypatch, recs, {}, dict(MAIN256), pairs=SEAM_PAIRS)
    assert r10["rep"]["block_levels"] == 10
    check(r10, o, "B = 10")
    r5 = run(monkeypatch, recs, {}, dict(MAIN256, SR_BLK_LEVELS="5"), pairs=SEAM_PAIRS)
    assert r5["rep"]["block_levels"] == 5
    check(r5, o, "B = 5")
    same_counts(r10, r5, "B = 10 against B = 5", ("wf_cells", "base_segments", "breakpoint_searches", "united_bases", "match_runs"))
    r1 = run(monkeypatch, recs, {}, dict(MAIN256, SR_NWG="1"), pairs=SEAM_PAIRS)
    check(r1, o, "one workgroup", "B = 10")
    same_counts(r10, r1, "one workgroup")
    # orientation in its own kernel: the same alignments, the same counts
    rp = run(monkeypatch, recs, {}, dict(MAIN256, SR_PREORIENT="1"), pairs=SEAM_PAIRS)
    assert rp["rep"]["orientation_route"] != "in-kernel"
    check(rp, o, "orientation kernel", "B = 10")
    same_counts(r10, rp, "orientation kernel", ("wf_steps", "base_segments", "breakpoint_searches", "united_bases", "match_runs"))


# ------------------------------------------------------------------------------------------ max_ak ring wrap
def small_family():
    return im.family(5150)


def family_oracle(kw):
    recs = small_family()
    return recs, oracle_for("family", recs, all_pairs(len(recs)), kw)


def test_max_ak_ring_wraps_inside_a_block(gpu, monkeypatch):
    kw = {"scores": GENERIC_WRAP}
    recs, o = family_oracle(kw)
    pen = im.parse_pen(GENERIC_WRAP)
    assert (pen.scope + 5 + 1) % 5 != 0 and min(a["score"] for (q, t), a in o.pairs.items() if q != t) > 2 * (pen.scope + 5 + 1)
    r = run(monkeypatch, recs, kw, dict(MAIN256, SR_NWG="3"))
    assert r["rep"]["block_levels"] == 5 and r["rep"]["ring_depth_m"] % 5 != 0, r["rep"]
    check(r, o, "generic_wrap")


# ------------------------------------------------------------------------------------------ base cases
@pytest.mark.parametrize("name", ["batch16", "requeue", "batch3"])
def test_base_case_batches(gpu, monkeypatch, name):
    recs = seam_records()
    o = oracle_for("seams", recs, SEAM_PAIRS, {})
    assert o.bases > 2 * 16
    env = {"batch16": {}, "requeue": {"SR_TEST_BASE_LEVELS": "20"}, "batch3": {"SR_BFS_BASE_JOBS": "3"}}[name]
    r = run(monkeypatch, recs, {}, dict(MAIN256, **env), pairs=SEAM_PAIRS)
    c = check(r, o, name)
    assert (c["base_requeues"] > 0) == (name == "requeue"), c["base_requeues"]
    assert c["base_tiles"] > 0


# ------------------------------------------------------------------------------------------ instance shapes
ROUNDS = {"SR_TAIL_ROUNDS": "64"}
SHAPES = {
    "threads64": ({"SR_ALIGN_THREADS": "64", "SR_NWG": "3"}, {}),
    "threads128": ({"SR_ALIGN_THREADS": "128", "SR_NWG": "3"}, {}),
    "threads256": (dict(MAIN256, SR_NWG="3"), {}),
    "threads512": ({"SR_ALIGN_THREADS": "512", "SR_NWG": "3"}, {}),
    "threads1024": ({"SR_NWG": "3"}, {}),                              # (few pairs: the load gives every workgroup 1 024 threads)
    "levels5": (dict(MAIN256, SR_BLK_LEVELS="5", SR_NWG="3"), {}),
    "one_piece": (dict(MAIN256, SR_NWG="3"), {"scores": im.ONE_PIECE}),
    "int32": (dict(MAIN256, SR_FORCE_INT32="1", SR_NWG="3"), {}),
    "one_workgroup": (dict(MAIN256, SR_NWG="1"), {}),
    "prio_on": (dict(MAIN256, SR_NWG="3", **ROUNDS), {}),
    "prio_off": (dict(MAIN256, SR_NWG="3", SR_TILE_PRIO="0", **ROUNDS), {}),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_instance_shapes(gpu, monkeypatch, name):
    env, kw = SHAPES[name]
    recs, o = family_oracle(kw)
    r = run(monkeypatch, recs, kw, env)
    check(r, o, name)
    if name == "levels5":
        assert r["rep"]["block_levels"] == 5
    if name == "int32":
        assert r["rep"]["offset_bytes"] == 4
    if name.startswith("threads"):
        assert r["rep"]["threads_per_workgroup"] == int(name[7:]), r["rep"]["threads_per_workgroup"]
    if name in ("prio_on", "prio_off"):
        assert r["rep"]["tile_prio"] == (1 if name == "prio_on" else 0)


def bounds_child(path):
    """(child process, SEQRUSH_AMD_LIB = the bounds-checked library)"""
    o = pickle.load(open(path, "rb"))

    class MP:
        @staticmethod
        def delenv(k, raising=False):
            os.environ.pop(k, None)

        @staticmethod
        def setenv(k, v):
            os.environ[k] = v
    recs = small_family()
    for env, golden in ((dict(MAIN256, SR_NWG="3"), "threads256"), (dict(MAIN256, SR_NWG="1", SR_TEST_BASE_LEVELS="20"), False),
                        (dict(MAIN256, SR_BLK_LEVELS="5", SR_NWG="3"), "levels5")):
        r = run(MP, recs, {}, env)
        check(r, o, "bounds %s" % env, golden)
        assert r["rep"]["kernel_build"] == "bounds" and r["cnt"]["bounds_first"][0] == 0
    print("bounds build clean")


def test_bounds_checked_build(gpu, tmp_path):
    """the -DSR_BOUNDS instance (an access outside a workgroup's extent raises SR_DEV_ERR_ADDRESS in the child).  A subprocess,
    because the library is chosen at load time"""
    lib = os.path.join(ROOT, "seqrush_amd", "libseqrush_amd_bounds.so")
    assert os.path.exists(lib), "build() did not make libseqrush_amd_bounds.so"
    recs, o = family_oracle({})
    path = tmp_path / "oracle.pkl"
    path.write_bytes(pickle.dumps(o))
    code = f"import sys; sys.path.insert(0, 'tests'); import test_pass_control_gpu as t; t.bounds_child({str(path)!r})"
    drop = tm.KNOBS + ("SR_TAIL", "SR_TAIL_THREADS", "SR_TAIL_ROUNDS", "SR_MIRROR_REPLAY") + PRIO_KNOBS
    env = {k: v for k, v in os.environ.items() if k not in drop}
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(env, SEQRUSH_AMD_LIB=lib), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "bounds build clean" in r.stdout, (r.stdout[-800:], r.stderr[-1500:])
