"""GPU tests (-m gpu) of the replay of a tied secondary (DESIGN.md 4.3 "Replay"): a primary that has a partner keeps one record
per breakpoint search; when a tie makes its workgroup align the secondary after all, the secondary takes the transposed
breakpoint of every search whose record carries no tie bit and searches only the others (base cases are always recomputed).
Results must be bit for bit what they are without the replay (SR_MIRROR_REPLAY=0), without mirroring (SR_NO_MIRROR=1) and what
the CPU oracle gives -- strand, score, raw CIGAR bytes, orientation scores, canonical labels -- and the counters that describe
the alignment as the oracle counts it must not move, while the passes as executed fall.

Inputs and oracle answers: tests/mirror_inputs.py; comparisons: the helpers of tests/test_mirror_gpu.py and
tests/test_tail_launch.py.  The main launch is pinned to the production shape (SR_ALIGN_THREADS=256) unless a case is about
another instance, and runs with fewer workgroups than pairs (what gives these small inputs partners at all)."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import mirror_inputs as mi
import test_mirror_gpu as tm
import test_tail_launch as tl

pytestmark = pytest.mark.gpu

ROOT = tm.ROOT
MAIN256 = tl.MAIN256
REPLAY_COUNTERS = ("mirror_tie_top", "mirror_tie_base_only", "mirror_replays", "replay_cached_searches")


def clear(mp):
    tl.clear(mp)
    mp.delenv("SR_MIRROR_REPLAY", raising=False)


def same_results(r, ref, what):
    for k in ("pairs", "rev", "score", "cigar", "ori"):
        assert r[k] == ref[k], (what, k)
    assert np.array_equal(r["labels"], ref["labels"]), what
    for k in tm.ORACLE_COUNTED + ("mirror_pairs", "mirror_ties"):
        assert r["cnt"][k] == ref["cnt"][k], (what, k, r["cnt"][k], ref["cnt"][k])


def three_ways(mp, name, kw, env, fused=True):
    """the input with the replay (mirroring on), with SR_MIRROR_REPLAY=0 and with SR_NO_MIRROR=1 under the same knobs: all equal
    to the oracle (tm.on_and_off) and to each other, the oracle-counted counters too -> (replay, no_replay, no_mirror)"""
    clear(mp)
    name, recs, o = mi.resolve(name, kw)                     # a name of mi.SETS, or (key, records, oracle function)
    on, off = tm.on_and_off(mp, recs, kw, env, o, fused)
    clear(mp)
    tm.set_env(mp, dict(tm.MIRROR_ON, **dict(env, SR_MIRROR_REPLAY="0")))
    r0 = tm.run_ctx(recs, kw, fused)
    clear(mp)
    same_results(on, r0, "replay against SR_MIRROR_REPLAY=0")
    assert r0["rep"]["mirror_replay"] == 0 and r0["rep"]["knobs"].get("SR_MIRROR_REPLAY") == "0"
    assert off["rep"]["mirror_replay"] == 0                      # no partners, no records
    assert r0["cnt"]["mirror_replays"] == 0 and r0["cnt"]["replay_cached_searches"] == 0
    assert off["cnt"]["mirror_replays"] == 0 and off["cnt"]["replay_cached_searches"] == 0
    # where the ties sit does not depend on the replay
    assert on["cnt"]["mirror_tie_top"] == r0["cnt"]["mirror_tie_top"] and on["cnt"]["mirror_tie_base_only"] == r0["cnt"]["mirror_tie_base_only"]
    print(name, kw, env, {k: on["cnt"][k] for k in REPLAY_COUNTERS + ("mirror_pairs", "mirror_ties")}, "bp_passes", on["cnt"]["bp_passes"],
          "without the replay", r0["cnt"]["bp_passes"], "searches", on["cnt"]["breakpoint_searches"])
    return on, r0, off, o


def replayed(on, r0):
    """the run replayed something and ran fewer passes for it"""
    assert on["rep"]["mirror_replay"] == 1 and "SR_MIRROR_REPLAY" not in on["rep"]["knobs"]
    assert on["cnt"]["mirror_replays"] >= 1 and on["cnt"]["replay_cached_searches"] >= 1
    assert on["cnt"]["bp_passes"] < r0["cnt"]["bp_passes"]
    assert on["cnt"]["mirror_replays"] <= on["cnt"]["mirror_ties"]


@pytest.mark.parametrize("nwg", ["1", "2", "4"])
def test_input_a(gpu, monkeypatch, nwg):
    """7 non-transposable pairs, 8 ties on the device.  One workgroup runs all 21 alignments in sequence: every replay is
    followed by an ordinary pair (a primary that records, or an unpaired self pair) whose result must be right -- stale records
    and solved marks must not reach it"""
    on, r0, off, o = three_ways(monkeypatch, "A", {}, dict(MAIN256, SR_NWG=nwg))
    assert on["rep"]["mirror_partners"] == 15 and on["rep"]["workgroups"] == int(nwg) and on["rep"]["threads_per_workgroup"] == 256
    assert on["cnt"]["mirror_ties"] >= len(o.non_transposable()) == 7
    replayed(on, r0)
    # no reverse strands, no errors on this input: every tied primary replays unless its depth-0 search was tie-sensitive,
    # and that one takes the old path (inline or the tail launch)
    assert on["cnt"]["mirror_replays"] == on["cnt"]["mirror_ties"] - on["cnt"]["mirror_tie_top"]
    assert on["cnt"]["mirror_tie_top"] >= 1                   # (this input has such pairs: 5 of its 8 ties)
    assert on["cnt"]["mirror_tie_top"] + on["cnt"]["mirror_tie_base_only"] <= on["cnt"]["mirror_ties"]


@pytest.mark.parametrize("pre", ["auto", "0", "1"])
def test_reverse_strand_secondaries_are_not_replayed(gpu, monkeypatch, pre):
    env = dict(MAIN256, **({} if pre == "auto" else {"SR_PREORIENT": pre}))
    on, r0, off, o = three_ways(monkeypatch, "rc", {}, env)
    rev_unordered = {(min(q, t), max(q, t)) for q, t in o.reverse_pairs()}
    assert len(rev_unordered) == 4 and on["rep"]["mirror_partners"] == 10
    assert on["cnt"]["mirror_replays"] <= on["cnt"]["mirror_ties"] - len(rev_unordered)


def test_substitutions_only(gpu, monkeypatch):
    """(almost) no ties: the run is the one without the replay"""
    on, r0, off, o = three_ways(monkeypatch, "subst", {}, MAIN256)
    assert on["rep"]["mirror_replay"] == 1
    assert on["cnt"]["mirror_replays"] <= on["cnt"]["mirror_ties"] < on["cnt"]["mirror_pairs"]
    if on["cnt"]["mirror_ties"] == 0:
        assert on["cnt"]["bp_passes"] == r0["cnt"]["bp_passes"] and on["cnt"]["replay_cached_searches"] == 0


def test_defer_all_keeps_full_alignments(gpu, monkeypatch):
    """SR_TAIL=all: every tied secondary goes to the tail launch and is aligned in full there"""
    clear(monkeypatch)
    on, o = tl.baseline(monkeypatch, "A", {}, MAIN256)
    clear(monkeypatch)
    r = tl.run_tail(monkeypatch, mi.input_a(), {}, dict(MAIN256, SR_TAIL="all"))
    tl.same(r, on)
    assert r["rep"]["mirror_replay"] == 1 and r["rep"]["tail_threads"] == 1024
    assert r["cnt"]["mirror_replays"] == 0 and r["cnt"]["replay_cached_searches"] == 0
    assert r["deferred"] == r["cnt"]["mirror_ties"] >= 7


INSTANCES = {
    "one-piece": (MAIN256, {"scores": tm.ONE_PIECE}),
    "int32": (dict(MAIN256, SR_FORCE_INT32="1"), {}),
    "levels5": (dict(MAIN256, SR_BLK_LEVELS="5"), {}),
    "threads64": ({"SR_ALIGN_THREADS": "64", "SR_NWG": "3"}, {}),
    "poison": (dict(MAIN256, SR_POISON_ROWS="37", SR_NWG="2"), {}),
    "wide": ({}, {}),                      # the 1 024-thread instance the load picks for so few pairs
}


@pytest.mark.parametrize("name", sorted(INSTANCES))
def test_instances(gpu, monkeypatch, name):
    env, kw = INSTANCES[name]
    on, r0, off, o = three_ways(monkeypatch, "A", kw, env)
    if name == "int32":
        assert on["rep"]["offset_bytes"] == 4 and on["rep"]["ring_cell_bytes"] == 2
    if name == "levels5":
        assert on["rep"]["block_levels"] == 5
    if name == "threads64":
        assert on["rep"]["threads_per_workgroup"] == 64 and on["rep"]["wave_build"] == 1
    if name == "wide":
        assert on["rep"]["threads_per_workgroup"] > 256
    assert on["cnt"]["mirror_ties"] >= len(o.non_transposable())
    if on["rep"]["mirror_replay"]:
        replayed(on, r0)
    else:
        assert on["cnt"]["mirror_replays"] == 0


def test_unfused_path(gpu, monkeypatch):
    on_u, r0_u, off_u, o = three_ways(monkeypatch, "A", {}, MAIN256, fused=False)
    replayed(on_u, r0_u)
    clear(monkeypatch)
    tm.set_env(monkeypatch, dict(tm.MIRROR_ON, **MAIN256))
    on_f = tm.run_ctx(mi.input_a(), {}, fused=True)
    same_results(on_f, on_u, "fused against align() + unite()")
    assert on_f["cnt"]["mirror_replays"] >= 1


def test_forced_batches(gpu, monkeypatch):
    """batches of about 13 pairs: records are a workgroup's and belong to the primary it has just aligned -- nothing of one
    batch's primary may reach a pair of the next batch (one workgroup takes them all in turn)"""
    recs = mi.input_a()
    o = mi.oracle_once("A")
    longest = max(len(s) for _, s in recs)
    for nwg in ("1", "4"):
        env = dict(MAIN256, SR_NWG=nwg, SR_CIGAR_ARENA_OPS=str(13 * (2 * longest + 2)))
        clear(monkeypatch)
        r = tl.run_tail(monkeypatch, recs, {}, env, batches=True)
        clear(monkeypatch)
        r0 = tl.run_tail(monkeypatch, recs, {}, dict(env, SR_MIRROR_REPLAY="0"), batches=True)
        monkeypatch.delenv("SR_MIRROR_REPLAY", raising=False)
        off = tl.run_tail(monkeypatch, recs, {}, dict(env, SR_NO_MIRROR="1"), batches=True)
        for x in (r, r0, off):
            for i, p in enumerate(x["pairs"]):
                assert (x["cigar"][i], x["score"][i], x["rev"][i]) == (o.pairs[p]["cigar"], o.pairs[p]["score"], o.pairs[p]["is_reverse"]), p
            assert np.array_equal(x["labels"], o.canonical_labels())
        same_results(r, r0, "batches")
        for k in tm.ORACLE_COUNTED:
            assert r["cnt"][k] == off["cnt"][k], k
        assert r["rep"]["batches"] >= 3 and 0 < r["rep"]["mirror_partners"] < 15
        assert r["cnt"]["mirror_pairs"] + r["cnt"]["mirror_ties"] == r["rep"]["mirror_partners"]
        assert r["cnt"]["mirror_replays"] >= 1 and r["cnt"]["bp_passes"] < r0["cnt"]["bp_passes"]
        assert r0["cnt"]["mirror_replays"] == 0
    clear(monkeypatch)


def bounds_child(path):
    """(child process, SEQRUSH_AMD_LIB = the bounds-checked library)"""
    oracle = pickle.load(open(path, "rb"))

    class MP:
        @staticmethod
        def delenv(k, raising=False):
            os.environ.pop(k, None)

        @staticmethod
        def setenv(k, v):
            os.environ[k] = v
    for nwg in ("1", "2"):
        clear(MP)
        on, off = tm.on_and_off(MP, mi.input_a(), {}, dict(MAIN256, SR_NWG=nwg), oracle)
        assert on["rep"]["kernel_build"] == "bounds" and on["rep"]["mirror_replay"] == 1
        assert on["cnt"]["mirror_replays"] >= 1 and on["cnt"]["replay_cached_searches"] >= 1
        assert on["cnt"]["bounds_first"][0] == 0
    print("bounds build clean")


def test_bounds_checked_build(gpu, tmp_path):
    """the -DSR_BOUNDS instance with replays on one and two workgroups: no access outside a workgroup's extent (it would raise
    SR_DEV_ERR_ADDRESS in the child)"""
    lib = os.path.join(ROOT, "seqrush_amd", "libseqrush_amd_bounds.so")
    assert os.path.exists(lib), "build() did not make libseqrush_amd_bounds.so"
    path = tmp_path / "oracle.pkl"
    path.write_bytes(pickle.dumps(mi.oracle_once("A")))
    code = f"import sys; sys.path.insert(0, 'tests'); import test_replay_gpu as t; t.bounds_child({str(path)!r})"
    env = {k: v for k, v in os.environ.items() if k not in tm.KNOBS + tl.TAIL_KNOBS + ("SR_MIRROR_REPLAY",)}
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(env, SEQRUSH_AMD_LIB=lib), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "bounds build clean" in r.stdout, (r.stdout[-800:], r.stderr[-1500:])
