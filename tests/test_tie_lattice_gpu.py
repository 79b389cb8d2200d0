"""GPU tests (-m gpu) of mirrored emission, the tail launch and the replay on the tie lattice
(tests/tie_inputs.py): every family through the mirrored paths -- emitted by symmetry, aligned after the primary, deferred to
the tail launch, replayed from the primary's records -- and through the kernel instances, bit for bit against the CPU oracle,
against SR_NO_MIRROR=1 and against SR_MIRROR_REPLAY=0 (strand, score, raw CIGAR bytes, orientation scores, canonical labels,
the oracle-counted counters: the helpers of test_mirror_gpu.py, test_replay_gpu.py and test_tail_launch.py assert those), and
within the bounds the CPU census of the same inputs gives (test_tie_lattice_host.py): a pair the oracle cannot transpose must
be aligned, a search below a tie must be searched.

Every family has 25 to 64 ordered pairs; SR_NWG stays below that (8 unless a case sets its own), without which a launch this
small gets no partners at all."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import mirror_inputs as mi
import test_mirror_gpu as tm
import test_replay_gpu as tr
import test_tail_launch as tl
import tie_inputs as ti
from seqrush_amd.seqrush import SeqSet, Params, Context

pytestmark = pytest.mark.gpu

ROOT = tm.ROOT
MAIN256 = tl.MAIN256


def inp(name):
    """a family as the helpers take it: (key, records, oracle answers under a parameter tuple)"""
    return ("tie:" + name, ti.records(name), lambda kt: ti.oracle_once(name, kt))


def census_bounds(r, name, kw, o, full=True):
    """what the CPU census says about a run with mirroring on.  full: all partners of the all-vs-all list exist (one batch)"""
    c = ti.census(name, kw.get("scores", ti.DEFAULT_SCORES))
    n, cnt = o.n, r["cnt"]
    rev = {(min(q, t), max(q, t)) for q, t in o.reverse_pairs()}
    nt = c.non_transposable()
    assert len(c.pairs) + len(rev) == n * (n - 1) // 2
    assert cnt["mirror_pairs"] + cnt["mirror_ties"] == r["rep"]["mirror_partners"]
    assert cnt["mirror_pairs"] <= len(c.pairs) - len(nt), "a pair the oracle cannot transpose was emitted by symmetry"
    per_pair = sorted((c.replayable(q, t) for q, t in c.pairs), reverse=True)
    assert cnt["mirror_replays"] <= cnt["mirror_ties"] - (len(rev) if full else 0)
    assert cnt["replay_cached_searches"] <= sum(per_pair[:cnt["mirror_replays"]]), "a search below a tie was taken from a record"
    if full:
        assert r["rep"]["mirror_partners"] == n * (n - 1) // 2
        assert cnt["mirror_ties"] >= len(nt) + len(rev)
        if name in ti.FORWARD:
            assert cnt["mirror_pairs"] >= 1
    print(name, kw, "census: forward pairs", len(c.pairs), "non-transposable", len(nt), "reverse", len(rev), "| device: mirror_pairs",
          cnt["mirror_pairs"], "mirror_ties", cnt["mirror_ties"], "replays", cnt["mirror_replays"], "cached", cnt["replay_cached_searches"],
          "of at most", sum(per_pair[:cnt["mirror_replays"]]))
    return c


def lattice(mp, name, kw, env, fused=True):
    on, r0, off, o = tr.three_ways(mp, inp(name), kw, env, fused)
    assert len(on["pairs"]) == o.n * o.n > int(on["rep"]["workgroups"])
    census_bounds(on, name, kw, o)
    census_bounds(r0, name, kw, o)
    return on, r0, off, o


@pytest.mark.parametrize("name", sorted(ti.FAMILIES))
def test_production_shape(gpu, monkeypatch, name):
    on, r0, off, o = lattice(monkeypatch, name, {}, MAIN256)
    assert on["rep"]["threads_per_workgroup"] == 256 and on["rep"]["symbol_bits"] == 2 and on["rep"]["mirror_replay"] == 1
    if name == "deep_ties":
        tr.replayed(on, r0)


INSTANCES = {
    "one-piece": (MAIN256, {"scores": ti.ONE_PIECE}),
    "int32": (dict(MAIN256, SR_FORCE_INT32="1"), {}),
    "levels5": (dict(MAIN256, SR_BLK_LEVELS="5"), {}),
    "threads64": ({"SR_ALIGN_THREADS": "64", "SR_NWG": "3"}, {}),
    "wide": ({}, {}),                                    # the load's own choice for so few pairs
    "nwg1": (dict(MAIN256, SR_NWG="1"), {}),
    "preorient0": (dict(MAIN256, SR_PREORIENT="0"), {}),
    "preorient1": (dict(MAIN256, SR_PREORIENT="1"), {}),
}


@pytest.mark.parametrize("inst", sorted(INSTANCES))
@pytest.mark.parametrize("name", ["deep_ties", "equal_blocks_16"])
def test_instances(gpu, monkeypatch, name, inst):
    env, kw = INSTANCES[inst]
    on, r0, off, o = lattice(monkeypatch, name, kw, env)
    rep = on["rep"]
    if inst == "int32":
        assert rep["offset_bytes"] == 4
    if inst == "levels5":
        assert rep["block_levels"] == 5
    if inst == "threads64":
        assert rep["threads_per_workgroup"] == 64 and rep["wave_build"] == 1
    if inst == "wide":
        assert rep["threads_per_workgroup"] > 256
    if inst == "nwg1":
        assert rep["workgroups"] == 1
    if inst.startswith("preorient"):
        assert rep["knobs"].get("SR_PREORIENT") == inst[-1]
    if name == "deep_ties":
        if rep["mirror_replay"]:
            tr.replayed(on, r0)
        else:
            assert on["cnt"]["mirror_replays"] == 0


@pytest.mark.parametrize("threads", ["512", "1024"])
@pytest.mark.parametrize("name", ["deep_ties", "equal_blocks_16"])
def test_tail_launch_takes_every_tie(gpu, monkeypatch, name, threads):
    """SR_TAIL=all: every tied secondary is aligned in full by the wide launch, nothing is replayed"""
    r, o = tl.tail_case(monkeypatch, inp(name), {}, MAIN256, {"SR_TAIL": "all", "SR_TAIL_THREADS": threads})
    assert r["rep"]["tail_threads"] == int(threads) and r["rep"]["threads_per_workgroup"] == 256
    c = census_bounds(r, name, {}, o)
    assert r["deferred"] == r["cnt"]["mirror_ties"] >= len(c.non_transposable()) >= 4
    assert r["cnt"]["mirror_replays"] == 0 and r["cnt"]["replay_cached_searches"] == 0


def test_deep_ties_unfused(gpu, monkeypatch):
    on_u, r0_u, off_u, o = lattice(monkeypatch, "deep_ties", {}, MAIN256, fused=False)
    tr.replayed(on_u, r0_u)
    tr.clear(monkeypatch)
    tm.set_env(monkeypatch, dict(tm.MIRROR_ON, **MAIN256))
    on_f = tm.run_ctx(list(ti.records("deep_ties")), {}, fused=True)
    tr.same_results(on_f, on_u, "fused against align() + unite()")
    assert on_f["cnt"]["mirror_replays"] >= 1


def test_deep_ties_forced_batches(gpu, monkeypatch):
    """batches of about 13 pairs: partners in different batches are aligned on their own, records never cross a batch"""
    recs = list(ti.records("deep_ties"))
    o = ti.oracle_once("deep_ties")
    longest = max(len(s) for _, s in recs)
    env = dict(MAIN256, SR_NWG="4", SR_CIGAR_ARENA_OPS=str(13 * (2 * longest + 2)))
    tr.clear(monkeypatch)
    r = tl.run_tail(monkeypatch, recs, {}, env, batches=True)
    tr.clear(monkeypatch)
    r0 = tl.run_tail(monkeypatch, recs, {}, dict(env, SR_MIRROR_REPLAY="0"), batches=True)
    monkeypatch.delenv("SR_MIRROR_REPLAY", raising=False)
    off = tl.run_tail(monkeypatch, recs, {}, dict(env, SR_NO_MIRROR="1"), batches=True)
    for x in (r, r0, off):
        for i, p in enumerate(x["pairs"]):
            assert (x["cigar"][i], x["score"][i], x["rev"][i]) == (o.pairs[p]["cigar"], o.pairs[p]["score"], o.pairs[p]["is_reverse"]), p
        assert np.array_equal(x["labels"], o.canonical_labels())
    tr.same_results(r, r0, "batches")
    for k in tm.ORACLE_COUNTED:
        assert r["cnt"][k] == off["cnt"][k], k
    assert r["rep"]["batches"] >= 3 and 0 < r["rep"]["mirror_partners"] < 15 and off["rep"]["mirror_partners"] == 0
    census_bounds(r, "deep_ties", {}, o, full=False)
    assert r0["cnt"]["mirror_replays"] == 0 and r["cnt"]["bp_passes"] <= r0["cnt"]["bp_passes"]
    tr.clear(monkeypatch)


BOUNDS_FAMILIES = ("deep_ties", "unequal_blocks_800")


def bounds_child(path):
    """(child process, SEQRUSH_AMD_LIB = the bounds-checked library)"""
    oracles = pickle.load(open(path, "rb"))

    class MP:
        @staticmethod
        def delenv(k, raising=False):
            os.environ.pop(k, None)

        @staticmethod
        def setenv(k, v):
            os.environ[k] = v
    for name in BOUNDS_FAMILIES:
        tr.clear(MP)
        on, off = tm.on_and_off(MP, list(ti.records(name)), {}, MAIN256, oracles[name])
        assert on["rep"]["kernel_build"] == "bounds" and on["rep"]["mirror_replay"] == 1
        assert on["cnt"]["mirror_pairs"] >= 1 and on["cnt"]["mirror_ties"] >= len(oracles[name].non_transposable()) >= 5
        if name == "deep_ties":
            assert on["cnt"]["mirror_replays"] >= 1 and on["cnt"]["replay_cached_searches"] >= 1
        assert on["cnt"]["bounds_first"][0] == 0 and off["cnt"]["bounds_first"][0] == 0
    print("bounds build clean")


def test_bounds_checked_build(gpu, tmp_path):
    """the -DSR_BOUNDS instance on the two families with the most replays: no access outside a workgroup's extent (it would
    raise SR_DEV_ERR_ADDRESS in the child).  A subprocess, because the library is chosen at load time"""
    lib = os.path.join(ROOT, "seqrush_amd", "libseqrush_amd_bounds.so")
    assert os.path.exists(lib), "build() did not make libseqrush_amd_bounds.so"
    path = tmp_path / "oracle.pkl"
    path.write_bytes(pickle.dumps({name: ti.oracle_once(name) for name in BOUNDS_FAMILIES}))
    code = f"import sys; sys.path.insert(0, 'tests'); import test_tie_lattice_gpu as t; t.bounds_child({str(path)!r})"
    env = {k: v for k, v in os.environ.items() if k not in tm.KNOBS + tl.TAIL_KNOBS + ("SR_MIRROR_REPLAY",)}
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(env, SEQRUSH_AMD_LIB=lib), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "bounds build clean" in r.stdout, (r.stdout[-800:], r.stderr[-1500:])


def test_an_n_member_means_no_partners(gpu, monkeypatch):
    """one N in one member: the set takes the 4-bit symbol build, where the reference's complement is no involution -- no pair
    gets a partner, and the run is the oracle's"""
    recs = list(ti.records("equal_blocks_16"))
    nm, s = recs[3]
    recs[3] = (nm, s[:400] + b"N" + s[401:])
    o = mi.OracleOnce(recs, {})
    tr.clear(monkeypatch)
    tm.set_env(monkeypatch, dict(tm.MIRROR_ON, **MAIN256))
    r = tm.run_ctx(recs, {})
    assert r["rep"]["symbol_bits"] == 4 and r["rep"]["mirror_partners"] == 0 and r["rep"]["tail_threads"] == 0
    assert r["cnt"]["mirror_pairs"] == 0 and r["cnt"]["mirror_ties"] == 0 and r["cnt"]["mirror_replays"] == 0
    for i, p in enumerate(r["pairs"]):
        assert (r["cigar"][i], r["score"][i], r["rev"][i]) == (o.pairs[p]["cigar"], o.pairs[p]["score"], o.pairs[p]["is_reverse"]), p
    assert np.array_equal(r["labels"], o.canonical_labels())


def test_a_paf_context_has_no_partners(gpu, monkeypatch, tmp_path):
    """`-p`: the records of a PAF file are united as they stand, (t, q) beside (q, t); there is no alignment stage, so no
    partners and no tail launch.  A PAF load writes no workspace report: its keys are absent, the counters are 0"""
    recs = list(ti.records("equal_blocks_16"))
    o = ti.oracle_once("equal_blocks_16")
    tr.clear(monkeypatch)
    tm.set_env(monkeypatch, dict(tm.MIRROR_ON, **MAIN256))
    ss = SeqSet(recs)
    ctx = Context(0)
    ctx.load(ss, Params())
    assert ctx.workspace_report()["mirror_partners"] == 15
    ctx.run(); ctx.sync()
    al = ctx.alignments()
    paf = tmp_path / "lattice.paf"
    al.write_paf(ss, str(paf))
    al.close(); ctx.close()
    assert len(paf.read_text().strip().split("\n")) == 36
    ctx = Context(0)
    ctx.load_paf(ss, Params(), str(paf))
    rep = ctx.workspace_report()
    assert rep.get("mirror_partners", 0) == 0 and rep.get("tail_threads", 0) == 0
    ctx.run(); ctx.sync()
    cnt = ctx.counters()
    assert cnt["mirror_pairs"] == 0 and cnt["mirror_ties"] == 0 and cnt["mirror_replays"] == 0 and ctx.tail_deferred() == 0
    assert ctx.align_kernel == ""
    assert np.array_equal(ctx.download_labels(), o.canonical_labels())
    ctx.close()
