"""GPU parity tests (-m gpu) of the base cases' backward-cone clipping (blk_setup of the blocked kernel,
seqrush_amd/csrc/sr_base_cone.h): a leaf of the biWFA recursion computes and stores, per level, only the diagonals from which
its end cell is still within reach.  Every case goes through check_parity -- strand, score, CIGAR bytes, partition and
canonical GFA against the oracle, every pair -- on inputs chosen to put the optimal path on the cone's edges: one long gap
at the very start, the very end and mid-sequence (both gap pieces, ends in I2 / D2), ragged lengths (k_end != 0), jobs that
are re-queued with the loose worst-case cone, history regions left dirty by the previous pair or poisoned before the run,
the 32-bit instances and the bounds-checked library."""
import os
import subprocess
import sys

import pytest

from seqrush_amd import synth
from seqrush_amd.seqrush import Context, Params, SeqSet
from test_gpu_parity import check_parity

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLK = "sr_align_blk_kernel"
_CACHE = {}


def _seq(L, seed):
    return synth.to_bytes(synth.base_sequence(L, seed))


def _snps(s, every, seed):
    b = bytearray(s)
    for i in range(seed % every, len(b), every):
        b[i] = {65: 67, 67: 71, 71: 84, 84: 65}[b[i]]
    return bytes(b)


def whole_pair_sets():
    """pairs of 150 - 600 bp whose score stays below 250: one breakpoint, then both halves are base cases"""
    if "whole" not in _CACHE:
        out = {}
        for L in (150, 333, 600):
            a = _seq(L, 9100 + L)
            out[f"{L}bp"] = [("a", a), ("b", _snps(a, 41, 3)), ("c", _snps(a, 29, 11)[:L - 7] + b"ACGTTGCA"),
                             ("d", a[:L // 3] + a[L // 3 + 9:])]
        _CACHE["whole"] = out
    return _CACHE["whole"]


def long_gap_sets():
    """a 400 bp sequence against copies with ONE long insertion / deletion (120 - 200 bp: beyond the first gap piece,
    near the reach limit of a 250-level base case) at the very start, the very end and mid-sequence"""
    if "gaps" not in _CACHE:
        a = _seq(400, 9201)
        ins = _seq(200, 9202)
        out = {}
        for g in (120, 163, 200):
            out[f"del{g}"] = [("a", a), ("start", a[g:]), ("end", a[:-g]), ("mid", a[:137] + a[137 + g:])]
            out[f"ins{g}"] = [("a", a), ("start", ins[:g] + a), ("end", a + ins[:g]), ("mid", a[:211] + ins[:g] + a[211:])]
        out["gap+snps"] = [("a", a), ("b", _snps(a[:90] + a[90 + 150:], 37, 5)), ("c", _snps(a[:300] + ins[:140] + a[300:], 43, 2))]
        _CACHE["gaps"] = out
    return _CACHE["gaps"]


def ragged_set():
    """plen != tlen: truncations at either end, one sequence several times the other"""
    if "ragged" not in _CACHE:
        a = _seq(900, 9301)
        _CACHE["ragged"] = [("a", a), ("head", a[:180]), ("tail", _snps(a[610:], 53, 1)), ("mid", a[300:520]),
                            ("rc", synth.reverse_complement(a[100:760])), ("tiny", a[400:431])]
    return _CACHE["ragged"]


def family_3x2kb():
    """5 % substitutions and indels: the segments split, base cases begin and end in gap components"""
    if "fam" not in _CACHE:
        _CACHE["fam"] = synth.indel_family(3, 2000, 0.04, 0.01, 9401)
    return _CACHE["fam"]


def _blocked(recs, levels=10, **kw):
    ctx = Context(0)
    ctx.load(SeqSet(recs), Params(**kw))
    rep = ctx.workspace_report()
    ctx.close()
    assert rep["kernel_impl"] == 2 and rep["block_levels"] == levels, rep
    return rep


@pytest.mark.parametrize("name", ["150bp", "333bp", "600bp"])
def test_whole_pair_base_cases(gpu, name):
    recs = whole_pair_sets()[name]
    _blocked(recs)
    al, _, cnt = check_parity(recs)
    assert cnt["align_kernel"] == BLK and cnt["base_segments"] > 0
    assert max(int(x) for x in al.score) <= 250


@pytest.mark.parametrize("scores", ["0,5,8,2,24,1", "0,5,8,2", "0,5,8,2,13,1"], ids=["default", "one-piece", "generic5"])
@pytest.mark.parametrize("name", ["del120", "del163", "del200", "ins120", "ins163", "ins200", "gap+snps"])
def test_one_long_gap_on_the_cones_edge(gpu, name, scores):
    recs = long_gap_sets()[name]
    _blocked(recs, levels=5 if scores == "0,5,8,2,13,1" else 10, scores=scores)
    _, _, cnt = check_parity(recs, scores=scores)
    assert cnt["align_kernel"] == BLK and cnt["base_segments"] > 0


def test_ragged_lengths(gpu):
    recs = ragged_set()
    _blocked(recs)
    _, _, cnt = check_parity(recs)
    assert cnt["align_kernel"] == BLK and cnt["base_segments"] > 0


ENVS = {
    "default": {},
    "requeue": {"SR_TEST_BASE_LEVELS": "20"},                      # every job outgrows two blocks: searched again, loose cone
    "requeue-30": {"SR_TEST_BASE_LEVELS": "30"},
    "1wg": {"SR_NWG": "1"},                                        # the history region is dirty from the previous pair
    "poisoned": {"SR_NWG": "2", "SR_POISON_ROWS": "37"},           # nothing reads what nobody wrote
    "int32-ring16": {"SR_FORCE_INT32": "1", "SR_RING_U16": "1", "SR_NWG": "3"},
    "int32-ring32": {"SR_FORCE_INT32": "1", "SR_RING_U16": "0"},
}


@pytest.mark.parametrize("env", list(ENVS))
def test_3x2kb_family(gpu, monkeypatch, env):
    for k, v in ENVS[env].items():
        monkeypatch.setenv(k, v)
    recs = family_3x2kb()
    rep = _blocked(recs)
    if env.startswith("int32"):
        assert rep["offset_bytes"] == 4 and rep["ring_cell_bytes"] == (2 if env == "int32-ring16" else 4), rep
    _, _, cnt = check_parity(recs)
    assert cnt["align_kernel"] == BLK and cnt["base_segments"] > 0
    assert (cnt["base_requeues"] > 0) == env.startswith("requeue")
    # the histories' share of the row bytes, the base cases' tiles and level-diagonals as executed (counters[44..47])
    assert 0 < cnt["hist_bytes_stored"] < cnt["row_bytes_stored"] and 0 < cnt["hist_bytes_loaded"] < cnt["row_bytes_loaded"]
    assert cnt["base_tiles"] > 0 and 0 < cnt["base_level_diagonals"] < cnt["wf_cells"]


@pytest.mark.parametrize("env", ["requeue", "1wg", "poisoned", "int32-ring16"])
def test_long_gaps_under_the_same_regimes(gpu, monkeypatch, env):
    for k, v in ENVS[env].items():
        monkeypatch.setenv(k, v)
    for name in ("del163", "ins200", "gap+snps"):
        check_parity(long_gap_sets()[name])
    check_parity(ragged_set())


def test_bounds_checked_library(gpu):
    """the -DSR_BOUNDS instance: every history row access tested against the workgroup's extent (a subprocess, because the
    library is chosen at load time)"""
    lib = os.path.join(ROOT, "seqrush_amd", "libseqrush_amd_bounds.so")
    assert os.path.exists(lib), "build() did not make libseqrush_amd_bounds.so"
    code = ("import sys; sys.path.insert(0, 'tests'); import test_gpu_parity as t; import test_base_cone_gpu as c\n"
            "from seqrush_amd.seqrush import SeqSet, Params, Context\n"
            "x = Context(0); x.load(SeqSet(c.family_3x2kb()), Params()); assert x.workspace_report()['kernel_build'] == 'bounds'; x.close()\n"
            "t.check_parity(c.family_3x2kb())\n"
            "t.check_parity(c.ragged_set())\n"
            "for n in ('del200', 'ins200', 'gap+snps'):\n"
            "    t.check_parity(c.long_gap_sets()[n])\n"
            "print('bounds build clean')\n")
    for extra in ({}, {"SR_NWG": "1", "SR_TEST_BASE_LEVELS": "20"}):
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, SEQRUSH_AMD_LIB=lib, **extra),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "bounds build clean" in r.stdout, (r.stdout[-800:], r.stderr[-1500:])
