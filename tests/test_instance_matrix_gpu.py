"""Device side of the instance matrix (-m gpu): every compiled instance of the two alignment kernel templates, reached by
its recipe from tests/instance_matrix.py, against the CPU oracle (check_parity: CIGAR bytes, strand, score, partition, GFA;
every pair) -- and the penalty lattice either side of every dispatch boundary.  Each case reads from the context's
workspace report which instance ran and holds it against the restatement, so a dispatch change that reroutes a recipe
fails the case instead of silently testing another kernel."""
import os
import subprocess
import sys

import pytest

import instance_matrix as im
import repeat_inputs as ri
import seqrush_amd as sa
from seqrush_amd import synth
from seqrush_amd.seqrush import Context, Params, SeqSet
from test_gpu_parity import check_parity

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REUSE = {"SR_NWG": "2", "SR_POISON_ROWS": "37"}        # two workgroups take all pairs in turn, rows start from plausible offsets
_FAMILIES = {}


def cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def matrix_family(seed, bits):
    if (seed, bits) not in _FAMILIES:
        recs = im.lift(im.family(seed), bits, seed)
        assert im.symbol_bits(recs) == bits
        _FAMILIES[(seed, bits)] = recs
    return _FAMILIES[(seed, bits)]


def loaded_report(recs, **kw):
    ctx = Context(0)
    ctx.load(SeqSet(recs), Params(**kw))
    rep, name = ctx.workspace_report(), ctx.align_kernel
    ctx.close()
    return rep, name


def run_and_identify(setenv, recs, knobs, scores=im.DEFAULT_SCORES, ori=im.DEFAULT_ORI, extra_env=None):
    """one load under `knobs`: the report must read what the restatement says for this shape, then parity with the
    oracle.  -> (Dispatch, counters, alignments)"""
    for k, v in dict(knobs, **(extra_env or {})).items():
        setenv(k, v)
    kw = {}
    if scores != im.DEFAULT_SCORES:
        kw["scores"] = scores
    if ori != im.DEFAULT_ORI:
        kw["orientation_scores"] = ori
    d = im.dispatch(scores, ori, bits=im.symbol_bits(recs), maxlen=max(len(s) for _, s in recs), npairs=len(recs) ** 2,
                    cus=cus(), knobs=knobs)
    rep, name = loaded_report(recs, **kw)
    bad = im.report_mismatches(rep, d, name)
    assert not bad, (bad, rep)
    if extra_env and "SR_NWG" in extra_env:
        assert rep["workgroups"] == int(extra_env["SR_NWG"]), rep
    al, _, cnt = check_parity(recs, **kw)
    assert cnt["align_kernel"] == name
    # from the device: the level kernel always counts a pair's ticks, the blocked kernel only in its profiling instance
    assert (cnt["ticks_pair"] > 0) == (d.kernel_impl == 1 or d.instance.prof), (cnt["ticks_pair"], d.instance)
    return d, cnt, al


@pytest.mark.parametrize("row", range(len(im.INSTANCE_ROWS)), ids=[im.instance_id(i) for i in im.INSTANCES])
def test_instance(gpu, monkeypatch, row):
    """one case per reachable instance: a family of 5 sequences of 1.2-2.5 kb (substitutions, indels up to 40, a truncated
    and a reverse-complemented member; N runs / soft masking / IUPAC codes for the 4- and 8-bit builds), once as it is and
    once with two workgroups on poisoned rows.  The searches recurse (breakpoints) and end in base cases."""
    inst, recipe = im.INSTANCE_ROWS[row]
    recs = matrix_family(row % 4, recipe["bits"])
    for extra in (None, REUSE):
        d, cnt, al = run_and_identify(monkeypatch.setenv, recs, recipe["knobs"], recipe["scores"], extra_env=extra)
        assert d.instance == inst, (d.instance, inst)
        assert cnt["breakpoint_searches"] > 0 and cnt["base_segments"] > 0
        assert al.n == len(recs) ** 2


def test_table_has_a_case_per_reachable_instance():
    assert len(im.INSTANCE_ROWS) == len(set(im.INSTANCES)) == 138 - len(im.UNREACHABLE)


@pytest.mark.parametrize("recipe,threads", im.SUBSTITUTIONS, ids=[str(i) for i in range(len(im.SUBSTITUTIONS))])
def test_requested_shape_without_a_build(gpu, monkeypatch, recipe, threads):
    """a requested thread count that has no build: the report names the shape that runs (run_and_identify holds the whole
    report against the restatement) and the result equals the oracle's"""
    recs = matrix_family(1, recipe["bits"])
    d, cnt, _ = run_and_identify(monkeypatch.setenv, recs, recipe["knobs"], recipe["scores"])
    assert d.threads_per_workgroup == threads and cnt["breakpoint_searches"] > 0


# ------------------------------------------------------------------------------------------ penalty lattice
@pytest.mark.parametrize("name", list(im.LATTICE))
def test_lattice(gpu, monkeypatch, name):
    """every lattice set on the 2-bit build: kernel, block depth, lazy I/D rows and narrow / wide as the table expects (and
    as the restatement derives), results equal to the oracle's; the set beyond the device ring is refused with the host's message"""
    scores, kernel, levels, lazy, wide = im.LATTICE[name]
    recs = matrix_family(2, 2)
    if kernel == "refused":
        with pytest.raises(sa.SeqRushError) as e:
            loaded_report(recs, scores=scores)
        assert e.value.code == -6 and im.UNSUPPORTED_SCOPE_MSG in str(e.value)
        return
    d, cnt, _ = run_and_identify(monkeypatch.setenv, recs, {"SR_ALIGN_THREADS": "256"}, scores)
    assert (d.kernel_impl, d.block_levels, d.lazy_id_rows, d.wide) == (2 if kernel == "blk" else 1, levels, lazy, wide)
    assert cnt["breakpoint_searches"] > 0 and cnt["base_segments"] > 0


@pytest.mark.parametrize("knobs", [{"SR_ALIGN_THREADS": "512"},
                                   {"SR_FORCE_INT32": "1", "SR_ALIGN_THREADS": "256"},
                                   {"SR_FORCE_INT32": "1", "SR_RING_U16": "0"}], ids=["int16", "int32-ring16", "int32-ring32"])
@pytest.mark.parametrize("name", im.NEW_EXACT)
def test_exact_instance_second_piece_15_and_20(gpu, monkeypatch, name, knobs):
    """the exact tile reads M[s - o2 - e2] as two runs of five rows; at 15 and 20 those runs are neither the block below
    nor the default's rows: int16 rows, the 16-bit ring of 32-bit searches, int32 rows; plain and with reused, poisoned rows"""
    scores = im.LATTICE[name][0]
    for extra in (None, REUSE):
        d, cnt, _ = run_and_identify(monkeypatch.setenv, matrix_family(3, 2), knobs, scores, extra_env=extra)
        assert d.block_levels == 10 and d.instance.two and cnt["breakpoint_searches"] > 0


@pytest.mark.parametrize("name", im.NEW_EXACT)
def test_exact_instance_second_piece_deep_search(gpu, monkeypatch, name):
    """one pair of 12.5 kb whose score passes 3 000 levels: the ring of 50 / 60 rows wraps many times and the
    deep-level reset runs with these row distances"""
    recs = synth.indel_family(2, 12500, 0.08, 0.004, 7411, max_indel=40)
    d, cnt, al = run_and_identify(monkeypatch.setenv, recs, {"SR_ALIGN_THREADS": "256"}, im.LATTICE[name][0])
    assert d.block_levels == 10 and max(int(s) for s in al.score) > 3000


# ------------------------------------------------------------------------------------------ orientation lattice
def orientation_family():
    recs = matrix_family(0, 2)[:4]
    pal = dict(ri.palindromes())
    return recs + [("pal", pal["pal"]), ("pal_mid", pal["pal_mid"])]


@pytest.mark.parametrize("route", ["1", "0"], ids=["orient-kernel", "in-kernel"])
@pytest.mark.parametrize("ori", [o for o in im.ORI_LATTICE if o != "0,1,76,1"])
def test_orientation_lattice(gpu, monkeypatch, ori, route):
    """every orientation set through its own kernel (SR_PREORIENT=1: the blocked wave kernel for 0,1,1,1, level by level
    otherwise) and through the in-kernel passes, on a family with reverse-complemented members and palindromes; sets the
    blocked path refuses run the level kernel.  Strand and score of every pair equal the oracle's (check_parity)."""
    blocked, want_route = im.ORI_LATTICE[ori]
    recs = orientation_family()
    d, cnt, al = run_and_identify(monkeypatch.setenv, recs, {"SR_PREORIENT": route, "SR_ALIGN_THREADS": "256"}, ori=ori)
    assert (d.kernel_impl == 2) == blocked
    assert d.orient_route == (want_route if route == "1" else "in-kernel")
    assert any(bool(r) for r in al.is_reverse) and not all(bool(r) for r in al.is_reverse)


# ------------------------------------------------------------------------------------------ bounds-checked build
def bounds_cells():
    """(knobs, scores, ori) the bounds-checked build runs: the 2-bit cells of the blocked kernel's workgroup build (the one
    libseqrush_amd_bounds.so replaces), the new exact-instance lattice cases, and the deepest orientation ring in-kernel"""
    cells = [(r["knobs"], r["scores"], im.DEFAULT_ORI) for i, r in im.INSTANCE_ROWS
             if i.family == "blk" and i.bits == 2 and i.build == "wg4"]
    for name in im.NEW_EXACT:
        for knobs in ({"SR_ALIGN_THREADS": "256"}, {"SR_FORCE_INT32": "1", "SR_ALIGN_THREADS": "256"}, {"SR_FORCE_INT32": "1", "SR_RING_U16": "0"}):
            cells.append((knobs, im.LATTICE[name][0], im.DEFAULT_ORI))
    cells.append(({"SR_PREORIENT": "0", "SR_ALIGN_THREADS": "256"}, im.DEFAULT_SCORES, "0,1,76,1"))
    return cells


def run_bounds_cells():
    """body of the subprocess of test_bounds_build_runs_the_blocked_cells_clean (the library is chosen at load time)"""
    cells = bounds_cells()
    for n, (knobs, scores, ori) in enumerate(cells):
        for k in list(os.environ):
            if k.startswith("SR_"):
                del os.environ[k]

        def setenv(k, v):
            os.environ[k] = v
        recs = matrix_family(n % 4, 2)
        rep, _ = loaded_report(recs)
        assert rep["kernel_build"] == "bounds", rep
        d, cnt, _ = run_and_identify(setenv, recs, knobs, scores, ori, extra_env=REUSE if n % 2 else None)
        assert d.kernel_impl == 2
        print("cell", n, im.instance_id(d.instance), "clean", flush=True)
    print("bounds cells clean:", len(cells))


def test_bounds_build_runs_the_blocked_cells_clean(gpu):
    """-DSR_BOUNDS instance of the 2-bit blocked kernel: every row and LDS access of these cells stays inside the workgroup's
    extent (a violation sets SR_DEV_ERR_ADDRESS, which sr_ctx_sync raises) and the results equal the oracle's"""
    lib = os.path.join(ROOT, "seqrush_amd", "libseqrush_amd_bounds.so")
    assert os.path.exists(lib), "build() did not make libseqrush_amd_bounds.so"
    code = "import sys; sys.path.insert(0, 'tests'); import test_instance_matrix_gpu as t; t.run_bounds_cells()"
    env = {k: v for k, v in os.environ.items() if not k.startswith("SR_")}
    env["SEQRUSH_AMD_LIB"] = lib
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "bounds cells clean: %d" % len(bounds_cells()) in r.stdout, (r.stdout[-1500:], r.stderr[-2500:])
