"""GPU tests (-m gpu) of the blocked kernel's tail launch: a primary whose secondary has to be aligned after all
puts it on a list when the queue is dry (SR_TAIL=all: always), and a second, wide launch of the same kernel aligns the list.
Results must be bit for bit what they are without the list (SR_TAIL=0), without mirroring (SR_NO_MIRROR=1) and what the CPU
oracle gives: strand, score, raw CIGAR bytes, orientation scores, canonical labels, the oracle-counted counters.

Inputs, oracle answers and the comparison of the two runs without a tail launch: tests/mirror_inputs.py and the helpers of
tests/test_mirror_gpu.py (mirroring needs fewer workgroups than pairs: SR_NWG).  These inputs have few enough pairs for the
load to give every workgroup 1 024 threads, which leaves nothing wider for a tail launch; the cases pin the main launch to
the production shape (SR_ALIGN_THREADS=256) so that the tail shape is chosen as it is on a full-size list."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import mirror_inputs as mi
import test_mirror_gpu as tm
from seqrush_amd.seqrush import SeqSet, Params, Context

pytestmark = pytest.mark.gpu

ROOT = tm.ROOT
TAIL_KNOBS = ("SR_TAIL", "SR_TAIL_THREADS", "SR_TAIL_ROUNDS")
MAIN256 = {"SR_ALIGN_THREADS": "256"}
_BASE = {}


def clear(mp):
    for k in TAIL_KNOBS:
        mp.delenv(k, raising=False)


def collect(ctx, rep, al):
    out = dict(pairs=[(int(al.query_idx[i]), int(al.target_idx[i])) for i in range(al.n)],
               cigar=[al.raw_cigar_bytes(i) for i in range(al.n)], rev=[bool(x) for x in al.is_reverse[:al.n]],
               score=[int(x) for x in al.score[:al.n]], labels=ctx.download_labels(), cnt=ctx.counters(), rep=rep,
               ori=[x.tolist() for x in ctx.orientation_scores()], deferred=ctx.tail_deferred())
    al.close(); ctx.close()
    return out


def run_tail(mp, recs, kw, env, fused=True, pairs=None, batches=False):
    """tm.run_ctx under env (mirroring on, their knobs and these cleared first), plus what only the tail launch has;
    batches: the pass that takes a list cut into several batches (align_all)"""
    clear(mp)
    tm.set_env(mp, dict(tm.MIRROR_ON, **env))
    ss = SeqSet(recs)
    ctx = Context(0)
    if pairs is None:
        ctx.load(ss, Params(**kw))
    else:
        ctx.load_pairs(ss, Params(**kw), pairs)
    rep = ctx.workspace_report()
    if batches:
        al = ctx.align_all(unite=True); ctx.sync()
        return collect(ctx, rep, al)
    if fused:
        ctx.run()
    else:
        ctx.align(); ctx.unite()
    ctx.sync()
    return collect(ctx, rep, ctx.alignments())


def baseline(mp, name, kw, env, fused=True):
    """the input under env with SR_TAIL=0, mirroring on and off: both equal to the oracle (tm.on_and_off asserts it).
    Computed once per (input, parameters, knobs) and shared unchanged"""
    name, recs, o = mi.resolve(name, kw)                     # a name of mi.SETS, or (key, records, oracle function)
    key = (name, tuple(sorted(kw.items())), tuple(sorted(env.items())), fused)
    if key not in _BASE:
        clear(mp)
        on, off = tm.on_and_off(mp, recs, kw, dict(env, SR_TAIL="0"), o, fused)
        assert on["rep"]["tail_threads"] == 0 and on["rep"]["knobs"].get("SR_TAIL") == "0"
        _BASE[key] = (on, o)
    return _BASE[key]


def same(r, on):
    """the run with a tail launch against the one without"""
    for k in ("pairs", "rev", "score", "cigar", "ori"):
        assert r[k] == on[k], k
    assert np.array_equal(r["labels"], on["labels"])
    for k in tm.ORACLE_COUNTED + ("mirror_pairs", "mirror_ties"):
        assert r["cnt"][k] == on["cnt"][k], (k, r["cnt"][k], on["cnt"][k])
    assert r["cnt"]["mirror_pairs"] + r["cnt"]["mirror_ties"] == r["rep"]["mirror_partners"] == on["rep"]["mirror_partners"]
    assert 0 <= r["deferred"] <= r["cnt"]["mirror_ties"]


def tail_case(mp, name, kw, env, tail_env, fused=True):
    on, o = baseline(mp, name, kw, env, fused)
    name, recs, _ = mi.resolve(name, kw)
    r = run_tail(mp, recs, kw, dict(env, **tail_env), fused)
    same(r, on)
    print(name, kw, env, tail_env, "tail_threads", r["rep"]["tail_threads"], "mirror_pairs", r["cnt"]["mirror_pairs"], "mirror_ties",
          r["cnt"]["mirror_ties"], "deferred", r["deferred"])
    return r, o


@pytest.mark.parametrize("nwg", ["1", "2", "8"])
def test_input_a_defer_all(gpu, monkeypatch, nwg):
    """every fallback secondary goes through the list; at one and two workgroups the tail grid is smaller than the list and
    its workgroups loop"""
    r, o = tail_case(monkeypatch, "A", {}, dict(MAIN256, SR_NWG=nwg), {"SR_TAIL": "all"})
    assert r["rep"]["tail_threads"] == 1024 and r["rep"]["threads_per_workgroup"] == 256
    assert r["deferred"] == r["cnt"]["mirror_ties"] >= len(o.non_transposable()) >= 7
    assert r["cnt"]["mirror_pairs"] >= 1
    if nwg != "8":
        assert r["rep"]["workgroups"] == int(nwg) < r["deferred"]


@pytest.mark.parametrize("threads", ["256", "512", "1024"])
def test_forced_tail_shapes(gpu, monkeypatch, threads):
    r, o = tail_case(monkeypatch, "A", {}, MAIN256, {"SR_TAIL": "all", "SR_TAIL_THREADS": threads})
    assert r["rep"]["tail_threads"] == int(threads)
    assert r["deferred"] == r["cnt"]["mirror_ties"] >= len(o.non_transposable())


SHAPES = {
    "one-piece": (MAIN256, {"scores": tm.ONE_PIECE}, 512),
    "int32": (dict(MAIN256, SR_FORCE_INT32="1"), {}, 512),
    "levels5": (dict(MAIN256, SR_BLK_LEVELS="5"), {}, 0),
    "threads64": ({"SR_ALIGN_THREADS": "64", "SR_NWG": "3"}, {}, 0),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_tail_shape_by_instance(gpu, monkeypatch, name):
    """the widest instance the plan has: 512 threads for one-piece penalties and for 32-bit searches on the uint16 ring, none
    for the 5-level instance and the one-wave build -- there nothing is deferred and the run is the one without a list"""
    env, kw, want = SHAPES[name]
    r, o = tail_case(monkeypatch, "A", kw, env, {"SR_TAIL": "all"})
    assert r["rep"]["tail_threads"] == want
    if name == "int32":
        assert r["rep"]["offset_bytes"] == 4 and r["rep"]["ring_cell_bytes"] == 2
    if want:
        assert r["deferred"] == r["cnt"]["mirror_ties"] >= len(o.non_transposable())
    else:
        assert r["deferred"] == 0 and r["cnt"]["mirror_ties"] >= len(o.non_transposable())


def test_default_rule(gpu, monkeypatch):
    """SR_TAIL unset: 21 alignments on 4 workgroups are within SR_TAIL_ROUNDS, so a secondary is deferred when its primary ends
    after the queue ran dry -- how many do depends on timing, the results do not"""
    r, o = tail_case(monkeypatch, "A", {}, dict(MAIN256, SR_NWG="4"), {})
    assert r["rep"]["tail_threads"] == 1024 and "SR_TAIL" not in r["rep"]["knobs"]
    # one round at most: the batch is beyond the rule, no list, nothing deferred
    r1, _ = tail_case(monkeypatch, "A", {}, dict(MAIN256, SR_NWG="4"), {"SR_TAIL_ROUNDS": "1"})
    assert r1["rep"]["tail_threads"] == 1024 and r1["deferred"] == 0


@pytest.mark.parametrize("pre", ["auto", "0", "1"])
def test_reverse_strand_secondaries(gpu, monkeypatch, pre):
    """secondaries of reverse-strand pairs are deferred and aligned on the reverse strand in the tail launch, with the
    orientation inside the alignment kernel and as its own kernel (strand and orientation scores are then inputs)"""
    env = dict(MAIN256, **({} if pre == "auto" else {"SR_PREORIENT": pre}))
    r, o = tail_case(monkeypatch, "rc", {}, env, {"SR_TAIL": "all"})
    rev_unordered = {(min(q, t), max(q, t)) for q, t in o.reverse_pairs()}
    assert r["deferred"] == r["cnt"]["mirror_ties"] >= len(rev_unordered) == 4
    assert sum(r["rev"]) == len(o.reverse_pairs()) == 8


def test_substitutions_only_and_no_partners(gpu, monkeypatch):
    """few or no ties: the tail launch finds a short or empty list and leaves every output as the main launch wrote it; a list
    without partners has no tail launch at all"""
    r, _ = tail_case(monkeypatch, "subst", {}, MAIN256, {"SR_TAIL": "all"})
    assert r["rep"]["tail_threads"] == 1024 and r["deferred"] == r["cnt"]["mirror_ties"]
    tail_case(monkeypatch, "subst", {}, MAIN256, {})
    pairs = [(q, t) for q in range(8) for t in range(q + 1, 8)]
    o = mi.oracle_once("subst")
    for env in ({"SR_TAIL": "all"}, {"SR_TAIL": "0"}):
        p = run_tail(monkeypatch, mi.subst_only(), {}, dict(MAIN256, **env), pairs=pairs)
        assert p["rep"]["mirror_partners"] == 0 and p["rep"]["tail_threads"] == 0 and p["deferred"] == 0
        assert p["cigar"] == [o.pairs[x]["cigar"] for x in pairs] and p["score"] == [o.pairs[x]["score"] for x in pairs]


def test_forced_batches(gpu, monkeypatch):
    """batches of about 13 pairs share the arena one after the other: list indices are relative to the batch, the three queue
    words are reset per batch, the deferred count is the sum over the batches"""
    recs = mi.input_a()
    o = mi.oracle_once("A")
    longest = max(len(s) for _, s in recs)
    env = dict(MAIN256, SR_NWG="4", SR_CIGAR_ARENA_OPS=str(13 * (2 * longest + 2)))
    on = run_tail(monkeypatch, recs, {}, dict(env, SR_TAIL="0"), batches=True)
    off = run_tail(monkeypatch, recs, {}, dict(env, SR_TAIL="0", SR_NO_MIRROR="1"), batches=True)
    for r in (on, off):
        assert r["deferred"] == 0 and r["rep"]["tail_threads"] == 0
        for i, p in enumerate(r["pairs"]):
            assert (r["cigar"][i], r["score"][i], r["rev"][i]) == (o.pairs[p]["cigar"], o.pairs[p]["score"], o.pairs[p]["is_reverse"]), p
        assert np.array_equal(r["labels"], o.canonical_labels())
    assert on["ori"] == off["ori"] and off["rep"]["mirror_partners"] == 0
    r = run_tail(monkeypatch, recs, {}, dict(env, SR_TAIL="all"), batches=True)
    same(r, on)
    for k in tm.ORACLE_COUNTED:
        assert r["cnt"][k] == off["cnt"][k], k
    assert r["rep"]["batches"] >= 3 and 0 < r["rep"]["mirror_partners"] < 15 and r["rep"]["tail_threads"] == 1024
    assert r["deferred"] == r["cnt"]["mirror_ties"] >= 1
    print("forced batches:", r["rep"]["batches"], "batches, partners", r["rep"]["mirror_partners"], "deferred", r["deferred"])


def test_unfused_path_equals_run(gpu, monkeypatch):
    """align() + unite(): the tail launch sits between the main launch and sr_unite_kernel"""
    ru, _ = tail_case(monkeypatch, "A", {}, MAIN256, {"SR_TAIL": "all"}, fused=False)
    rf, _ = tail_case(monkeypatch, "A", {}, MAIN256, {"SR_TAIL": "all"}, fused=True)
    assert ru["deferred"] == rf["deferred"] >= 7
    assert ru["cigar"] == rf["cigar"] and np.array_equal(ru["labels"], rf["labels"])
    for k in tm.ORACLE_COUNTED:
        assert ru["cnt"][k] == rf["cnt"][k], k


def test_poisoned_rows(gpu, monkeypatch):
    """the tail launch reuses workspace slots the main launch dirtied, on top of rows that held plausible offsets"""
    r, _ = tail_case(monkeypatch, "A", {}, dict(MAIN256, SR_POISON_ROWS="37", SR_NWG="2"), {"SR_TAIL": "all"})
    assert r["deferred"] == r["cnt"]["mirror_ties"] >= 7


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
    env = dict(MAIN256, SR_NWG="2")
    clear(MP)
    on, _ = tm.on_and_off(MP, mi.input_a(), {}, dict(env, SR_TAIL="0"), oracle)
    r = run_tail(MP, mi.input_a(), {}, dict(env, SR_TAIL="all"))
    same(r, on)
    assert r["rep"]["kernel_build"] == "bounds" and r["rep"]["tail_threads"] == 1024
    assert r["deferred"] == r["cnt"]["mirror_ties"] >= 7
    assert r["cnt"]["bounds_first"][0] == 0 and on["cnt"]["bounds_first"][0] == 0
    print("bounds build clean")


def test_bounds_checked_build(gpu, tmp_path):
    """the -DSR_BOUNDS instance, main and tail launch on two workgroup slots: no access outside a workgroup's extent"""
    lib = os.path.join(ROOT, "seqrush_amd", "libseqrush_amd_bounds.so")
    assert os.path.exists(lib), "build() did not make libseqrush_amd_bounds.so"
    path = tmp_path / "oracle.pkl"
    path.write_bytes(pickle.dumps(mi.oracle_once("A")))
    code = f"import sys; sys.path.insert(0, 'tests'); import test_tail_launch as t; t.bounds_child({str(path)!r})"
    env = {k: v for k, v in os.environ.items() if k not in tm.KNOBS + TAIL_KNOBS}
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(env, SEQRUSH_AMD_LIB=lib), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "bounds build clean" in r.stdout, (r.stdout[-800:], r.stderr[-1500:])
