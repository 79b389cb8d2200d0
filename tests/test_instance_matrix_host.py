"""Host side of the instance matrix (no GPU): the oracle is pinned against the Gotoh DP on every set of the penalty
lattice before any device test leans on it there; the inputs really exercise the second gap piece; the dispatch
restatement of tests/instance_matrix.py equals the library's srk_align_blk_supports over an exhaustive grid; and the
instance table equals the set of alignment kernel instantiations in the built library."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import instance_matrix as im
import oracle_binding as ob
import repeat_inputs as ri
from seqrush_amd import synth, _lib


# ------------------------------------------------------------------------------------------ inputs
def host_pairs():
    """(pattern, text) pairs of at most a few hundred bases: seeded indel families (indels up to 40, one member
    reverse-complemented), clean single gaps of 1 / 17 / 90 bases, and members of the repeat families"""
    pairs = []
    for seed, L in ((11, 150), (12, 300), (13, 300)):
        fam = [s for _, s in synth.indel_family(3, L, 0.03, 0.02, 8100 + seed, max_indel=40)]
        fam[2] = synth.reverse_complement(fam[2])
        fam.append(synth.reverse_complement(fam[0]))                # related to fam[2] on the same strand
        pairs += [(a, b) for i, a in enumerate(fam) for j, b in enumerate(fam) if i != j and (i + j) % 2 == 1]
    base = synth.to_bytes(synth.base_sequence(320, 8200))
    for gap in (1, 17, 90):
        cut = base[:130] + base[130 + gap:]
        pairs += [(base, cut), (cut, base)]
    pairs.append((base[:100] + base[101:200] + base[240:], base))    # gaps of 1 and 40 in one pair
    for name in ("microsatellites", "palindromes", "two_letter"):
        recs = [s for _, s in ri.SMALL_FAMILIES[name]()][:4]
        recs = [s[:300] for s in recs]
        pairs += [(recs[i], recs[j]) for i in range(len(recs)) for j in range(len(recs)) if i < j]
    return pairs


PAIRS = host_pairs()
RUNNABLE = {k: v for k, v in im.LATTICE.items() if v[1] != "refused"}


def oracle_pen(scores):
    r, pen = ob.parse_scores(scores)
    assert r == 0
    return pen


@pytest.fixture(scope="module")
def oracle_cigars():
    """lattice set -> [(pattern, text, full-memory CIGAR, biWFA CIGAR)], each checked against the DP on the way"""
    out = {}
    for name, row in RUNNABLE.items():
        pen = oracle_pen(row[0])
        rows = []
        for a, b in PAIRS:
            g = ob.gotoh(a, b, pen)
            both = []
            for mode in (ob.MEM_HIGH, ob.MEM_ULTRALOW):
                raw, s = ob.wfa_align(a, b, pen, mode)
                assert s == g, (name, mode, s, g, len(a), len(b))
                assert ob.cigar_score(raw, a, b, pen) == s, (name, mode)
                assert raw.count(b"M") + raw.count(b"X") + raw.count(b"D") == len(a), (name, mode)
                assert raw.count(b"M") + raw.count(b"X") + raw.count(b"I") == len(b), (name, mode)
                both.append(raw)
            rows.append((a, b, both[0], both[1]))
        out[name] = rows
    return out


def test_oracle_equals_gotoh_on_the_whole_lattice(oracle_cigars):
    """full-memory WFA and biWFA scores equal the O(nm) DP, every CIGAR scores what it claims and consumes both lengths
    (asserted while the fixture builds), on every runnable lattice set"""
    assert set(oracle_cigars) == set(RUNNABLE) and all(len(v) == len(PAIRS) for v in oracle_cigars.values())
    assert len(PAIRS) >= 30 and max(max(len(a), len(b)) for a, b in PAIRS) <= 500


def test_the_second_gap_piece_matters(oracle_cigars):
    """a two-piece set whose second piece never prices a gap of the inputs would be a one-piece test in disguise: for every
    set with a crossover some oracle CIGAR holds a gap run longer than it; where the second piece is cheaper at every
    length a gap of one base exists.  (e2 >= e1 with o2 >= o1 has no crossover: the second piece can never win.)"""
    checked = 0
    for name, rows in oracle_cigars.items():
        pen = im.parse_pen(RUNNABLE[name][0])
        if not pen.two:
            continue
        x = im.crossover(pen)
        if x is None:
            assert pen.e2 >= pen.e1 and pen.o2 >= pen.o1
            continue
        runs = [r for _, _, hi, lo in rows for r in im.gap_runs(hi) + im.gap_runs(lo)]
        if x == 1:
            assert 1 in runs, name
        else:
            assert max(runs) > x, (name, x, max(runs))
            assert min(runs) < x, (name, x)                          # and the first piece prices some gap too
        checked += 1
    assert checked >= 14


def test_lattice_expectations_follow_from_the_restatement():
    """the lattice table's expected column is what the restatement gives for a small 2-bit load"""
    for name, (scores, kernel, levels, lazy, wide) in im.LATTICE.items():
        if kernel == "refused":
            with pytest.raises(ValueError, match="scope > 127"):
                im.dispatch(scores)
            continue
        d = im.dispatch(scores, knobs={"SR_ALIGN_THREADS": "256"})
        assert (d.kernel_impl, d.block_levels, d.lazy_id_rows, d.wide) == (2 if kernel == "blk" else 1, levels, lazy, wide), (name, d)
    for ori, (blocked, route) in im.ORI_LATTICE.items():
        d = im.dispatch(ori_scores=ori, knobs={"SR_PREORIENT": "1"})
        assert (d.kernel_impl == 2, d.orient_route) == (blocked, route), (ori, d)
        assert im.dispatch(ori_scores=ori, knobs={"SR_PREORIENT": "0"}).orient_route == "in-kernel"


def test_lattice_has_both_sides_of_every_boundary():
    got = {name: im.dispatch(row[0], knobs={"SR_ALIGN_THREADS": "256"}) for name, row in RUNNABLE.items()}
    seconds = {im.second_piece(im.parse_pen(RUNNABLE[n][0])) for n, d in got.items() if d.two_piece and d.block_levels == 10}
    assert seconds == {10, 15, 20, 25}
    sides = lambda f: {f(d) for d in got.values()}
    assert sides(lambda d: d.kernel_impl) == {1, 2} and sides(lambda d: d.block_levels) == {1, 5, 10}
    assert sides(lambda d: (d.kernel_impl, d.lazy_id_rows)) == {(1, 0), (2, 0), (2, 1)}
    assert sides(lambda d: (d.kernel_impl, d.wide)) == {(1, False), (1, True), (2, False)}


# ------------------------------------------------------------------------------------------ restatement == library
class SrPen(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("x", "o1", "e1", "o2", "e2", "two", "scope")]

    @staticmethod
    def of(p: im.Pen):
        return SrPen(p.x, p.o1, p.e1, p.o2, p.e2, int(p.two), p.scope)


def mk(x, o1, e1, o2=None, e2=None):
    two = o2 is not None
    return im.Pen(x, o1, e1, o2 if two else 0, e2 if two else 0, two, max(x, o1 + e1, o2 + e2 if two else 0) + 1)


def test_block_depth_equals_srk_align_blk_supports_on_a_grid():
    """exhaustive, no sampling: x 1..12, o1 0..12, e1 1..3, one piece and two pieces with o2 0..80 and e2 1..3, under four
    orientation sets (the default, one with e1 = 2, the last whose scope fits the blocked ring and the first that does not) -- about 450 000
    combinations through ctypes; the function is host code and the library loads without a GPU"""
    L = _lib.load()
    f = L.srk_align_blk_supports
    f.argtypes = [C.POINTER(SrPen), C.POINTER(SrPen)]
    f.restype = C.c_int
    n = 0
    seen = set()
    for ori in (mk(1, 1, 1), mk(1, 2, 2), mk(1, 77, 1), mk(1, 76, 1)):
        co = SrPen.of(ori)
        for x in range(1, 13):
            for o1 in range(0, 13):
                for e1 in (1, 2, 3):
                    pens = [mk(x, o1, e1)] + [mk(x, o1, e1, o2, e2) for o2 in range(0, 81) for e2 in (1, 2, 3)]
                    for p in pens:
                        if p.scope > im.MAX_SCOPE:
                            continue
                        cp = SrPen.of(p)
                        want, have = im.blk_levels(p, ori), f(C.byref(cp), C.byref(co))
                        assert want == have, (p, ori, want, have)
                        seen.add(have)
                        n += 1
    assert n > 300000 and seen == {0, 5, 10}


def test_launcher_substitutions_are_stated():
    """requested shapes that have no build: the restatement (and, since this change, the load itself) names the shape
    that runs, and that shape is a row of the table"""
    for recipe, threads in im.SUBSTITUTIONS:
        d = im.dispatch(recipe["scores"], bits=recipe["bits"], npairs=25, knobs=recipe["knobs"])
        assert d.threads_per_workgroup == threads and d.instance in im.INSTANCES, (recipe, d)


def test_every_recipe_reaches_its_instance():
    """each row's recipe, through the restatement, lands on the row's own instance -- and on no other row's"""
    assert len(set(im.INSTANCES)) == len(im.INSTANCES)
    for inst, recipe in im.INSTANCE_ROWS:
        d = im.dispatch(recipe["scores"], bits=recipe["bits"], npairs=25, knobs=recipe["knobs"])
        assert d.instance == inst, (im.instance_id(inst), d)
    for inst, why in im.UNREACHABLE:
        assert inst not in im.INSTANCES and why


# ------------------------------------------------------------------------------------------ completeness guard
def kernel_symbols():
    """demangled symbols of the built library (`nm -C`, else ROCm's llvm-nm)"""
    lib = _lib.LIB_PATH
    tools = [shutil.which("nm"), shutil.which("llvm-nm"), "/opt/rocm/llvm/bin/llvm-nm", "/opt/rocm/lib/llvm/bin/llvm-nm"]
    for tool in tools:
        if tool and os.path.exists(tool):
            r = subprocess.run([tool, "-C", lib], capture_output=True, text=True)
            if r.returncode == 0 and "sr_align_blk_kernel" in r.stdout:
                return r.stdout
    return None


def test_instance_table_is_complete():
    """the table (reachable rows + rows listed as unreachable) equals the sr_align_blk_kernel<...> / sr_align_bfs_kernel<...>
    instantiations of the built library, read from its demangled host-side kernel symbols: a new instance without a row
    fails here, on a machine without a GPU"""
    text = kernel_symbols()
    assert text is not None, "neither nm nor llvm-nm could list the symbols of " + _lib.LIB_PATH
    built = im.instances_in_symbols(text)
    table = set(im.INSTANCES) | {inst for inst, _ in im.UNREACHABLE}
    assert len(table) == len(im.INSTANCES) + len(im.UNREACHABLE)
    missing = sorted(im.instance_id(i) for i in built - table)
    stale = sorted(im.instance_id(i) for i in table - built)
    assert not missing and not stale, {"built without a row": missing, "rows without a build": stale}
    by = lambda fam: sum(1 for i in built if i.family == fam)
    assert (by("blk"), by("bfs")) == (66, 72)
