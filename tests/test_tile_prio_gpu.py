"""GPU tests (-m gpu) of the rotating tile priority of the blocked kernel (sr_prio_rule.h): the workgroups
of a CU take a rank at kernel start and run the tile code of a pass at an s_setprio level that goes round by rank and wall
time.  Issue priority cannot change a result, so every case is bit-equality of three runs: the default, SR_TILE_PRIO=0 (all
tile code at priority 0, no clock read) and the CPU oracle -- strand, score, raw CIGAR bytes, orientation scores, canonical
labels, and between the two device runs the counters that count as the oracle counts.

The small inputs have few enough pairs for the load to give every workgroup 1 024 threads -- one workgroup per CU, where the
rule is off; the cases that are about the rule pin the production shape (SR_ALIGN_THREADS=256) as tests/test_tail_launch.py
does."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import mirror_inputs as mi
import test_mirror_gpu as tm
import test_replay_gpu as tr
import tie_inputs as ti
from seqrush_amd import synth

pytestmark = pytest.mark.gpu

ROOT = tm.ROOT
PRIO_KNOBS = ("SR_TILE_PRIO", "SR_WG_PER_CU")
MAIN256 = {"SR_ALIGN_THREADS": "256"}
# a batch rotates only while its alignments are at most SR_TAIL_ROUNDS x its workgroups (the short-list rule): two or three
# workgroups run 20 to 40 alignments here, so the cases raise the bound to keep the rotation on
ROUNDS = {"SR_TAIL_ROUNDS": "64"}
_ORACLE = {}


def clear(mp):
    tr.clear(mp)
    for k in PRIO_KNOBS:
        mp.delenv(k, raising=False)


def family(name):
    return list(ti.records(name)), ti.oracle_once(name)


def snp_40x300():
    """40 x 300 bp, 3 % substitutions: 1 600 ordered pairs, more than the 1 024 workgroup slots of the device"""
    if "snp" not in _ORACLE:
        recs = synth.snp_family(40, 300, 0.03, 4100)
        _ORACLE["snp"] = (recs, mi.OracleOnce(recs, {}))
    return _ORACLE["snp"]


def run(mp, recs, env):
    clear(mp)
    tm.set_env(mp, env)
    return tm.run_ctx(recs, {})


def three_runs(mp, recs, oracle, env, prio_wg):
    """default and SR_TILE_PRIO=0 under env, both against the oracle and against each other -> (default, knob)"""
    on = run(mp, recs, env)
    off = run(mp, recs, dict(env, SR_TILE_PRIO="0"))
    assert on["kernel"] == off["kernel"] == "sr_align_blk_kernel"
    for r, what in ((on, "default"), (off, "SR_TILE_PRIO=0")):
        for i, (q, t) in enumerate(r["pairs"]):
            oa = oracle.pairs[q, t]
            assert r["rev"][i] == oa["is_reverse"], (what, q, t)
            assert r["score"][i] == oa["score"], (what, q, t)
            assert r["cigar"][i] == oa["cigar"], f"{what}: CIGAR differs from the oracle's on pair ({q},{t})"
        assert np.array_equal(r["labels"], oracle.canonical_labels()), what
        assert r["rep"]["prio_workgroups_per_cu"] == prio_wg, (what, r["rep"])
        assert r["rep"]["prio_epoch_shift"] == 11
        # every workgroup of the (one) main launch took a rank; no CU's count can exceed the launch
        assert r["cnt"]["prio_ranks_taken"] == r["rep"]["workgroups"], (what, r["cnt"]["prio_ranks_taken"], r["rep"]["workgroups"])
        assert 1 <= r["cnt"]["prio_max_cu_arrivals"] <= r["rep"]["workgroups"]
    for k in ("pairs", "rev", "score", "cigar", "ori"):
        assert on[k] == off[k], k
    assert np.array_equal(on["labels"], off["labels"])
    for k in tm.ORACLE_COUNTED + ("mirror_pairs", "mirror_ties"):
        assert on["cnt"][k] == off["cnt"][k], (k, on["cnt"][k], off["cnt"][k])
    assert on["rep"]["tile_prio"] == (1 if prio_wg > 1 else 0) and "SR_TILE_PRIO" not in on["rep"]["knobs"]
    assert off["rep"]["tile_prio"] == 0 and off["rep"]["knobs"].get("SR_TILE_PRIO") == "0"
    print(env, "workgroups", on["rep"]["workgroups"], "x", on["rep"]["threads_per_workgroup"], "prio_wg", prio_wg, "ranks",
          on["cnt"]["prio_ranks_taken"], "max arrivals", on["cnt"]["prio_max_cu_arrivals"], "mirror_pairs", on["cnt"]["mirror_pairs"],
          "mirror_ties", on["cnt"]["mirror_ties"], "replays", on["cnt"]["mirror_replays"])
    return on, off


@pytest.mark.parametrize("name", ["deep_ties", "unequal_blocks_800"])
def test_two_workgroups_many_alignments(gpu, monkeypatch, name):
    """two persistent workgroups run the whole family: several alignments each, ties, fallback secondaries and replays"""
    recs, o = family(name)
    on, off = three_runs(monkeypatch, recs, o, dict(MAIN256, SR_NWG="2", **ROUNDS), 4)
    assert on["rep"]["workgroups"] == 2 and on["rep"]["threads_per_workgroup"] == 256
    assert on["cnt"]["mirror_pairs"] >= 1 and on["cnt"]["mirror_ties"] >= len(o.non_transposable()) >= 2


def test_more_pairs_than_workgroup_slots(gpu, monkeypatch):
    """1 600 pairs: the full launch of the device (every CU holds its four workgroups), mirroring active"""
    recs, o = snp_40x300()
    on, off = three_runs(monkeypatch, recs, o, {}, 4)
    assert len(on["pairs"]) == 1600 > on["rep"]["workgroups"] >= 256 and on["rep"]["threads_per_workgroup"] == 256
    assert on["rep"]["mirror_partners"] == 40 * 39 // 2 and on["cnt"]["mirror_pairs"] >= 1
    # (a uniform histogram over the CUs is not asserted: pairs this small let early workgroups exit before late ones arrive)


INSTANCES = {
    # knobs, workgroups per CU the rule runs with (16 waves per CU)
    "threads512": ({"SR_ALIGN_THREADS": "512", "SR_NWG": "3"}, 2),
    "threads64": ({"SR_ALIGN_THREADS": "64", "SR_NWG": "3"}, 16),
    "threads128": ({"SR_ALIGN_THREADS": "128", "SR_NWG": "3"}, 8),
    "levels5": (dict(MAIN256, SR_BLK_LEVELS="5", SR_NWG="3"), 4),
    "int32": (dict(MAIN256, SR_FORCE_INT32="1", SR_NWG="3"), 4),
    "three_per_cu": (dict(MAIN256, SR_WG_PER_CU="3", SR_NWG="3"), 3),
    # one workgroup per CU: the rule is off whatever the knob says
    "threads1024": ({"SR_NWG": "3"}, 1),
}


@pytest.mark.parametrize("name", sorted(INSTANCES))
def test_other_instances(gpu, monkeypatch, name):
    env, prio_wg = INSTANCES[name]
    recs, o = family("unequal_blocks_800")
    on, off = three_runs(monkeypatch, recs, o, dict(env, **ROUNDS), prio_wg)
    if name == "threads1024":
        assert on["rep"]["threads_per_workgroup"] == 1024 and on["rep"]["tile_prio"] == 0
    if name == "levels5":
        assert on["rep"]["block_levels"] == 5
    if name == "int32":
        assert on["rep"]["offset_bytes"] == 4


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
    on, off = three_runs(MP, list(ti.records("deep_ties")), o, dict(MAIN256, SR_NWG="2", **ROUNDS), 4)
    assert on["rep"]["kernel_build"] == "bounds" and on["rep"]["tile_prio"] == 1
    assert on["cnt"]["bounds_first"][0] == 0 and off["cnt"]["bounds_first"][0] == 0
    print("bounds build clean")


def test_bounds_checked_build(gpu, tmp_path):
    """one case on the -DSR_BOUNDS instance (an access outside a workgroup's extent raises SR_DEV_ERR_ADDRESS in the child).  A
    subprocess, because the library is chosen at load time"""
    lib = os.path.join(ROOT, "seqrush_amd", "libseqrush_amd_bounds.so")
    assert os.path.exists(lib), "build() did not make libseqrush_amd_bounds.so"
    path = tmp_path / "oracle.pkl"
    path.write_bytes(pickle.dumps(ti.oracle_once("deep_ties")))
    code = f"import sys; sys.path.insert(0, 'tests'); import test_tile_prio_gpu as t; t.bounds_child({str(path)!r})"
    drop = tm.KNOBS + ("SR_TAIL", "SR_TAIL_THREADS", "SR_TAIL_ROUNDS", "SR_MIRROR_REPLAY") + PRIO_KNOBS
    env = {k: v for k, v in os.environ.items() if k not in drop}
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(env, SEQRUSH_AMD_LIB=lib), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "bounds build clean" in r.stdout, (r.stdout[-800:], r.stderr[-1500:])
