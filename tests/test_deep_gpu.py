"""GPU parity tests (-m gpu) of deep searches on the packed 16-bit tiles (tests/deep_inputs.py): one-sided gaps and unrelated
pairs, thousands of levels with most diagonals off the matrix, on int16 rows and -- SR_FORCE_INT32=1 -- on the 16-bit ring
of 32-bit searches.  That is where a NULL cell creeps (sr_blk_tile.inc, q4_renull): tiles past SR_DEEP_INT16 /
SR_DEEP_RING16 levels reset the chain sources and the M[s - x] sources of a block, not its gap-open sources, and ADVICE.md
(round 4) estimates that a NULL could still reach the valid range near level 6 600 / 3 300.  Every case runs past that
estimate (test_deep_host.py shows which few cannot, and how deep those run) and must equal the CPU oracle bit for bit:
CIGAR bytes, strand, score, partition, GFA, and sr_ctx_run against align + unite (test_gpu_parity.check_parity).  The
bounds-checked build runs first: it drops an offending access instead of performing it and reports it."""
import functools
import os
import pickle
import subprocess
import sys

import pytest

import deep_inputs as di
import oracle_binding as ob
from seqrush_amd.seqrush import SeqSet, Params, Context
from test_gpu_parity import check_parity, oracle_params

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = {"ring16": {"SR_FORCE_INT32": "1"}, "int16": {}, "int32": {"SR_FORCE_INT32": "1", "SR_RING_U16": "0"}}
CELLS = {"ring16": (4, 2), "int16": (2, 2), "int32": (4, 4)}                       # offset_bytes, ring_cell_bytes
REGIMES = {"default": {}, "1wg": {"SR_NWG": "1"}, "2wg-poison": {"SR_NWG": "2", "SR_POISON_ROWS": "37"}}
KNOBS = ("SR_FORCE_INT32", "SR_RING_U16", "SR_NWG", "SR_POISON_ROWS")


class OracleOnce:
    """the oracle's answers on one input under one penalty set, computed once and shared, unchanged, by every regime that
    runs the input (and, pickled, by the child process of the bounds-checked build): what check_parity asks of an
    OracleSeqRush"""

    def __init__(self, recs, kw):
        o = ob.OracleSeqRush(records=recs)
        op = oracle_params(**kw)
        n = len(recs)
        self.pairs = {(q, t): o.align_pair(op, q, t) for q in range(n) for t in range(n)}
        o.align_and_unite(op)
        self.labels = o.canonical_labels()
        self.gfa_out = o.gfa(canonical=True)
        o.close()

    def align_pair(self, op, q, t):
        return self.pairs[q, t]

    def align_and_unite(self, op):
        return None

    def canonical_labels(self):
        v = self.labels.view(); v.flags.writeable = False
        return v

    def gfa(self, canonical=True):
        assert canonical
        return self.gfa_out


@functools.lru_cache(maxsize=None)
def oracle_once(name, scores):
    return OracleOnce(di.SETS[name](), {} if scores == di.DEFAULT else {"scores": scores})


def run_case(instance, name, scores, regime, oracle=None, expect_build="default"):
    """one input on one instance of the tile under one regime (environment already set): the report shows the instance,
    the build and every knob, the result equals the oracle's, and the deepest pair ran as deep as the case promises"""
    recs = di.SETS[name]()
    kw = {} if scores == di.DEFAULT else {"scores": scores}
    ctx = Context(0); ctx.load(SeqSet(recs), Params(**kw))
    rep = ctx.workspace_report(); ctx.close()
    # the 16-bit ring exists for the exact 10-level instance only (sr_host.cpp plan_kernel, u16_ok): forced 32-bit searches of
    # the generic 5-level instance keep int32 rows -- the unpacked tile, run here as the same inputs' cross-check
    generic = rep["kernel_impl"] == 2 and rep["block_levels"] == 5
    assert generic == (scores == di.GENERIC), rep
    assert (rep["offset_bytes"], rep["ring_cell_bytes"]) == (CELLS["int32"] if instance == "ring16" and generic else CELLS[instance]), rep
    if expect_build != "default" or not os.environ.get("SEQRUSH_AMD_LIB"):       # (an A/B library names its own build)
        assert rep["kernel_build"] == expect_build, rep
    want = dict(ENV[instance], **regime)
    assert {k: v for k, v in rep["knobs"].items() if k in KNOBS} == want, rep["knobs"]
    al, labels, cnt = check_parity(recs, oracle=oracle if oracle is not None else oracle_once(name, scores), **kw)
    deepest = max(int(x) for x in al.score) // 2
    if (instance, name, scores) in di.CASES:                                      # the packed tiles
        assert deepest >= di.levels_needed(instance, name, scores), (instance, name, scores, deepest)
    if name in di.GAP:
        assert max(int(x) for x in al.score) == di.gap_score(scores, di.GAP[name])
    return al, cnt


def set_env(monkeypatch, instance, regime):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(ENV[instance], **regime).items():
        monkeypatch.setenv(k, v)


# ------------------------------------------------------------------------------------------ bounds-checked build first
def bounds_child(path):
    """(child process, SEQRUSH_AMD_LIB = the bounds-checked library) one case with all workgroups and with two"""
    instance, name, oracle = pickle.load(open(path, "rb"))
    for regime in ({}, {"SR_NWG": "2"}):
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(dict(ENV[instance], **regime))
        run_case(instance, name, di.DEFAULT, regime, oracle=oracle, expect_build="bounds")
    print("bounds build clean")


@pytest.mark.parametrize("instance,name", [("ring16", s) for s in di.RING16_SETS] + [("int16", s) for s in di.INT16_SETS])
def test_bounds_checked_build_on_deep_sets(gpu, tmp_path, instance, name):
    """the -DSR_BOUNDS instance of the blocked kernel on every ring16 and int16 set, SR_NWG unset and 2: no row or LDS-window
    address outside the workgroup's extent (SR_DEV_ERR_ADDRESS would raise in the child; SR_BOUNDS_DETAIL=1 names the first
    offender in the message) and results equal to the oracle's.  A subprocess, because the library is chosen at load time"""
    lib = os.path.join(ROOT, "seqrush_amd", "libseqrush_amd_bounds.so")
    assert os.path.exists(lib), "build() did not make libseqrush_amd_bounds.so"
    path = tmp_path / "case.pkl"
    path.write_bytes(pickle.dumps((instance, name, oracle_once(name, di.DEFAULT))))
    code = f"import sys; sys.path.insert(0, 'tests'); import test_deep_gpu as t; t.bounds_child({str(path)!r})"
    env = dict(os.environ, SEQRUSH_AMD_LIB=lib, SR_BOUNDS_DETAIL="1")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "bounds build clean" in r.stdout, (r.stdout[-800:], r.stderr[-1500:])


# ------------------------------------------------------------------------------------------ production build
@pytest.mark.parametrize("regime", sorted(REGIMES))
@pytest.mark.parametrize("name", di.RING16_SETS)
def test_ring16_deep(gpu, monkeypatch, name, regime):
    """C5's instance -- the packed tile on the 16-bit ring of 32-bit searches -- at least 4 800 levels per side; with one
    workgroup the pairs follow each other in one ring (deep_then_shallow: a search of 40 levels after one of 5 500), with
    two the rows are poisoned with a plausible offset before the run"""
    set_env(monkeypatch, "ring16", REGIMES[regime])
    al, cnt = run_case("ring16", name, di.DEFAULT, REGIMES[regime])
    assert cnt["align_kernel"] == "sr_align_blk_kernel"


@pytest.mark.parametrize("regime", ["default", "1wg"])
@pytest.mark.parametrize("name", di.INT16_SETS)
def test_int16_deep(gpu, monkeypatch, name, regime):
    """int16 rows, no knob: gaps of 20 000 and 18 000 (9 000 levels per side and more) and unrelated pairs"""
    set_env(monkeypatch, "int16", REGIMES[regime])
    al, cnt = run_case("int16", name, di.DEFAULT, REGIMES[regime])
    assert cnt["align_kernel"] == "sr_align_blk_kernel"


def test_int32_rows_cross_check(gpu, monkeypatch):
    """the unpacked tile on int32 rows has no creep: a mismatch here as well as above is not the packed path's"""
    set_env(monkeypatch, "int32", {})
    al, cnt = run_case("int32", "prefix12k", di.DEFAULT, {})
    assert cnt["align_kernel"] == "sr_align_blk_kernel"


@pytest.mark.parametrize("instance", ["int16", "ring16"])
@pytest.mark.parametrize("scores", [di.ONE_PIECE, di.GENERIC])
@pytest.mark.parametrize("name", di.PENALTY_SETS)
def test_penalty_instances_deep(gpu, monkeypatch, name, scores, instance):
    """the one-piece exact instance (twice the depth at the same size: 8 + 2 x 8 000 on prefix9k) and the generic
    blocked instance (o2 + e2 = 14 is no multiple of five), on int16 rows and with SR_FORCE_INT32=1: the exact instance then
    runs the packed tile on the 16-bit ring, the generic one -- which has no 16-bit ring -- the 32-bit tile on int32 rows"""
    set_env(monkeypatch, instance, {})
    al, cnt = run_case(instance, name, scores, {})
    assert cnt["align_kernel"] == "sr_align_blk_kernel"


def test_level_per_pass_kernel_deep(gpu, monkeypatch):
    """0,4,6,2,24,1 has no blocked instance: the level-per-pass kernel on a gap of 8 000"""
    set_env(monkeypatch, "int16", {})
    al, cnt = run_case("int16", "prefix9k", di.LEVEL_KERNEL, {})
    assert cnt["align_kernel"] == "sr_align_bfs_kernel"
    assert max(int(x) for x in al.score) == 24 + 8000
