"""Device side of the long-sequence seams (-m gpu): both sides of every length seam of every alphabet (DESIGN.md section 3;
tests/long_inputs.py) against the CPU oracle.  Every case first holds the load's workspace report against
long_inputs.plan() -- kernel family, offset and ring cell width, symbol bits, threads, workgroups per CU, dynamic LDS and
the orientation route -- so a dispatch change that moves a seam fails here instead of silently testing another instance,
and then runs test_gpu_parity.check_parity: raw CIGAR bytes, strand and score of every pair, partition, GFA, and a second
run on the same context.

Measured on an MI355X, wall time of a whole case (both runs of check_parity, downloads, GFA; the oracle's answers are
shared and mostly computed by the first case that needs them):
  yardstick test_gpu_parity.py::test_50kb_pair_int32_offsets[60000-env4], same session      0.23 s
  slowest blocked-kernel case   off16-s2-32000 (first case of the module: device warm-up)    0.30 s
                                blocked-s2-102368-ragged (longest blocked load)              0.27 s
  slowest level-kernel case     admitted-s2-177456 (two runs: 0.46 s, 0.52 s)                0.52 s
                                blocked-s2-102369-rc-ragged                                  0.33 s
Every blocked case is within 1.3 times the yardstick (allowed: three times), every level-kernel case within 2.4 times
(allowed: ten times); the child process of the bounds-checked build takes 3 s, the whole module 13 s.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import long_inputs as li
import oracle_binding as ob
import seqrush_amd as sa
from seqrush_amd import synth
from seqrush_amd.seqrush import Context, Params, SeqSet
from test_gpu_parity import check_parity

pytestmark = pytest.mark.gpu

REUSE = {"SR_NWG": "1", "SR_POISON_ROWS": "37"}        # one workgroup takes all four pairs in turn on poisoned rows


@functools.lru_cache(maxsize=None)
def cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def loaded_report(recs):
    ctx = Context(0)
    ctx.load(SeqSet(recs), Params())
    rep, name = ctx.workspace_report(), ctx.align_kernel
    ctx.close()
    return rep, name


def run_case(setenv, case, extra=None):
    """one load of a case under its knobs (+ extra): the report reads what plan() says, the result equals the oracle's"""
    knobs = dict(case.knobs, **(extra or {}))
    for k, v in knobs.items():
        setenv(k, v)
    recs = li.recs_of(case)
    p = li.plan(case.L, case.bits, npairs=4, cus=cus(), knobs=knobs)
    assert p.refused is None
    rep, name = loaded_report(recs)
    bad = li.plan_mismatches(rep, name, p)
    assert not bad, (bad, rep)
    assert rep["pairs"] == 4 and rep["batches"] == 1
    if "SR_NWG" in knobs:
        assert rep["workgroups"] == int(knobs["SR_NWG"]), rep
    al, _, cnt = check_parity(recs, oracle=li.oracle_once(case.name))
    assert cnt["align_kernel"] == name and al.n == 4
    assert cnt["breakpoint_searches"] > 0 and cnt["base_segments"] > 0
    return p, rep, cnt


@pytest.mark.parametrize("case", li.CASES, ids=lambda c: c.name)
def test_both_sides_of_every_seam(gpu, monkeypatch, case):
    """every admitted length either side of every seam; the orientation seams under SR_PREORIENT=1, where the report
    must show the orientation kernel's rings on the lower side and none on the upper one"""
    p, rep, _ = run_case(monkeypatch.setenv, case)
    if case.seam == "orient":
        lower = case.L == [s.L for s in li.SEAMS if (s.name, s.bits) == ("orient", case.bits)][0]
        assert rep["orientation_route"] == ("orient-blk" if lower else "in-kernel")
        assert (rep["orientation_ring_bytes"] > 0) == lower and rep["orientation_ring_bytes"] == p.orientation_ring_bytes


def _case_at(bits, L, rc=None):
    return [c for c in li.CASES if (c.bits, c.L) == (bits, L) and not c.knobs and (rc is None or c.rc == rc)][0]


@pytest.mark.parametrize("bits,L", sorted(li.LAST_BLOCKED.items()) + sorted(li.LEVEL_LENGTH.items()),
                         ids=lambda v: str(v))
def test_one_workgroup_on_poisoned_rows(gpu, monkeypatch, bits, L):
    """the last blocked length and one level-kernel length of every alphabet once more with SR_NWG=1 and poisoned rows: one
    workgroup aligns all four pairs in turn and starts each from what the previous pair left in LDS and in the rows"""
    run_case(monkeypatch.setenv, _case_at(bits, L), extra=REUSE)


@pytest.mark.parametrize("bits,L", [(4, li.LAST_BLOCKED[4]), (8, li.LAST_BLOCKED[8])], ids=lambda v: str(v))
def test_256_threads_at_the_window_edge(gpu, monkeypatch, bits, L):
    """the 256-thread builds have smaller static tables than the 512-thread ones the plan picks: the four copies of the
    same load lie elsewhere in the window.  The reverse-complemented case: the copy at the top of the window is extended"""
    p, rep, _ = run_case(monkeypatch.setenv, _case_at(bits, L, rc=True), extra={"SR_ALIGN_THREADS": "256"})
    assert p.threads_per_workgroup == 256 and rep["threads_per_workgroup"] == 256


@pytest.mark.parametrize("bits", [2, 4, 8])
def test_short_pair_inside_a_full_size_window(gpu, bits):
    """an explicit pair list at the last blocked length whose sequences 2 and 3 are a 300-base pair: window and plan are
    those of the long pair"""
    case = _case_at(bits, li.LAST_BLOCKED[bits], rc=True)
    recs = li.recs_of(case) + li.short_pair(bits)
    pairs = [(0, 1), (1, 0), (2, 3), (3, 2)]
    ctx = Context(0)
    ctx.load_pairs(SeqSet(recs), Params(), pairs)
    rep, name = ctx.workspace_report(), ctx.align_kernel
    bad = li.plan_mismatches(rep, name, li.plan(case.L, bits, npairs=4, cus=cus()))
    assert not bad, (bad, rep)
    assert ctx.pairs() == pairs
    ctx.run(); ctx.sync()
    al, labels = ctx.alignments(), ctx.download_labels()
    ctx.close()
    o = li.OracleByPieces(recs, pairs=pairs, rev_first=True)
    for i, (q, t) in enumerate(pairs):
        oa = o.align_pair(None, q, t)
        assert al.raw_cigar_bytes(i) == oa["cigar"], f"CIGAR differs on pair ({q},{t})"
        assert bool(al.is_reverse[i]) == oa["is_reverse"] and int(al.score[i]) == oa["score"]
    assert o.pairs[0, 1]["is_reverse"] and not o.pairs[2, 3]["is_reverse"]
    assert np.array_equal(labels, o.canonical_labels())


def test_bounds_checked_build_on_the_longest_2bit_loads(gpu):
    """the -DSR_BOUNDS instance of the 2-bit blocked kernel (libseqrush_amd_bounds.so: every row access tested against the
    workgroup's extent, every LDS window of a live cell of the packed tile against the staged sequences) on the longest
    load of the 16-bit ring (57 000: the packed tile's largest offsets and highest window addresses) and on the longest
    blocked load (102 368: the longest rows), reverse strand extended in both: clean (no SR_DEV_ERR_ADDRESS) and equal to
    the oracle.  A subprocess, because the library is chosen at load time."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "seqrush_amd", "libseqrush_amd_bounds.so")
    assert os.path.exists(lib), "build() did not make libseqrush_amd_bounds.so"
    code = ("import os, sys; sys.path.insert(0, 'tests'); import test_gpu_parity as t; import long_inputs as li\n"
            "from seqrush_amd.seqrush import SeqSet, Params, Context\n"
            "for L, rows in ((57000, 2), (102368, 4)):\n"
            "    recs = list(li.pair(L, 2, 8970, rc=True))\n"
            "    oracle = li.OracleByPieces(recs, rev_first=True)\n"
            "    for nwg in (None, '1'):\n"                   # as many workgroups as pairs; one that takes all four in turn
            "        if nwg: os.environ['SR_NWG'] = nwg\n"
            "        else: os.environ.pop('SR_NWG', None)\n"
            "        c = Context(0); c.load(SeqSet(recs), Params()); rep = c.workspace_report(); c.close()\n"
            "        assert rep['kernel_build'] == 'bounds' and rep['kernel_impl'] == 2 and rep['ring_cell_bytes'] == rows, rep\n"
            "        assert rep['workgroups'] == (1 if nwg else 4), rep\n"
            "        t.check_parity(recs, oracle=oracle)\n"
            "print('bounds build clean')\n")
    env = dict(os.environ, SEQRUSH_AMD_LIB=lib)
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "bounds build clean" in r.stdout, (r.stdout[-800:], r.stderr[-1500:])


def test_thread_rule_just_below_20kb_of_copies(gpu):
    """a 2-bit load of 20 000 bases with fewer pairs than CUs: 20 048 bytes of copies beside the 34 KB of static tables of
    the 1 024-thread shape leave two workgroups per CU, so the load runs 512 threads -- the window in which
    instance_matrix.dispatch still answers (copies <= 20 KB) and says 1 024 (test_long_seams_host._dispatch_window)"""
    recs = list(li.pair(20000, 2, 8999))
    p = li.plan(20000, 2, npairs=4, cus=cus())
    assert (p.threads_per_workgroup, p.workgroups_per_cu, p.lds_dynamic_bytes) == (512, 2, 20048)
    rep, name = loaded_report(recs)
    bad = li.plan_mismatches(rep, name, p)
    assert not bad, (bad, rep)
    check_parity(recs, oracle=li.OracleByPieces(recs))


@pytest.mark.parametrize("bits", [2, 4, 8])
def test_first_refused_length(gpu, bits):
    """one symbol past the last admitted length: SR_ERR_UNSUPPORTED with the LDS message, and the context serves the next
    load.  The blocked kernel's other refusal (4 GB of rows per workgroup) cannot be reached below the LDS limit:
    test_long_seams_host.test_row_workspace_refusal_is_out_of_reach has the arithmetic (0.68 GB at most)"""
    L = li.FIRST_REFUSED[bits]
    assert li.plan(L, bits).refused == li.LDS_REFUSAL and li.plan(L - 1, bits).refused is None
    recs = list(li.pair(L, bits, 8990 + bits))
    assert max(len(s) for _, s in recs) == L
    ctx = Context(0)
    with pytest.raises(sa.SeqRushError) as e:
        ctx.load(SeqSet(recs), Params())
    assert e.value.code == li.SR_ERR_UNSUPPORTED and li.LDS_REFUSAL in str(e.value), str(e.value)
    assert str(L - 1) in str(e.value)                       # the message names the limit of every alphabet
    small = synth.config_c1()
    ctx.load(SeqSet(small), Params())
    ctx.run(); ctx.sync()
    labels = ctx.download_labels()
    ctx.close()
    o = ob.OracleSeqRush(records=small)
    o.align_and_unite(ob.default_params())
    assert np.array_equal(labels, o.canonical_labels())
    o.close()
