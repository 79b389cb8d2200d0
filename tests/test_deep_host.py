"""CPU tests (-m "not gpu") on the deep one-sided-gap inputs (tests/deep_inputs.py): before any device time is spent they
show that the inputs reach the level counts test_deep_gpu.py relies on and that the oracle alone is right on them -- its
score is the closed form of the one gap, the independent O(nm) Gotoh DP's score, and the cost of its own CIGAR.  Every
assertion is exact."""
import functools
import os
import re
from concurrent.futures import ThreadPoolExecutor

import pytest

import deep_inputs as di
import oracle_binding as ob
from seqrush_amd import synth
from conftest import usable_cpus

GOTOH_CELLS = 10 ** 8            # |q| |t| up to which the quadratic DP runs (a second per 10^8 cells): all sets but prefix30k
# closed forms under the other two penalty sets: the sets the device suite runs under them get the oracle's alignment
# (score and CIGAR), the others the oracle's score-only WFA -- the same recurrences without the backtrace, a third of the time
ALIGNED = {(n, di.DEFAULT) for n in di.SETS} | {(n, p) for n in di.PENALTY_SETS for p in (di.ONE_PIECE, di.GENERIC)} | \
          {("prefix9k", di.LEVEL_KERNEL)}
SCORED = {(n, p) for n in di.GAP for p in di.CLOSED_FORM_SCORES} - ALIGNED


def pen_of(scores):
    r, pen = ob.parse_scores(scores)
    assert r == 0
    return pen


def _pair(recs, scores, q, t, align):
    """one ordered pair: the oracle's alignment (or its score alone) and Gotoh's score on the strand the oracle chose"""
    pen = pen_of(scores)
    out = {}
    if align:
        o = ob.OracleSeqRush(records=recs)
        op = ob.default_params(); op.threads = 1; op.pen = pen
        out = o.align_pair(op, q, t)
        o.close()
        qq = synth.reverse_complement(recs[q][1]) if out["is_reverse"] else recs[q][1]
    else:
        qq = recs[q][1]
        out["score"] = ob.wfa_score(qq, recs[t][1], pen)
    tt = recs[t][1]
    out["gotoh"] = ob.gotoh(qq, tt, pen) if len(qq) * len(tt) <= GOTOH_CELLS else None
    out["strand_q"], out["t_seq"] = qq, tt
    return out


@functools.lru_cache(maxsize=None)
def reference():
    """{(set, scores): {(q, t): result}} for every ordered pair of different sequences, computed once for the module (the
    library calls release the GIL: one thread per usable CPU)"""
    jobs = []
    for (name, scores) in sorted(ALIGNED | SCORED):
        recs = di.SETS[name]()
        for q in range(len(recs)):
            for t in range(len(recs)):
                if q != t:
                    jobs.append((name, scores, q, t, recs, (name, scores) in ALIGNED))
    jobs.sort(key=lambda j: -max(len(s) for _, s in j[4]))                  # longest first
    with ThreadPoolExecutor(max_workers=min(16, usable_cpus())) as ex:
        res = list(ex.map(lambda j: _pair(j[4], j[1], j[2], j[3], j[5]), jobs))
    out = {}
    for j, r in zip(jobs, res):
        out.setdefault((j[0], j[1]), {})[(j[2], j[3])] = r
    return out


def test_constructors_are_deterministic_and_small():
    for name, f in di.SETS.items():
        a, b = f(), f()
        assert a == b and f.__name__ == name
        assert 2 <= len(a) <= 3 and len({n for n, _ in a}) == len(a)
        assert all(0 < len(s) <= 32000 and set(s) <= set(b"ACGT") for _, s in a), name       # int16 rows unless forced
    x = dict(di.prefix12k())["x"]
    assert dict(di.suffix12k())["suf"] == x[-1000:] and dict(di.hole12k())["ends"] == x[:1000] + x[-1000:]
    assert dict(di.prefix9k())["x9"] == x[:9000] and dict(di.prefix30k())["pre"] == dict(di.prefix30k())["y30"][:12000]
    pre, snp = dict(di.deep_then_shallow())["pre"], dict(di.deep_then_shallow())["snp"]
    assert len(snp) == len(pre) and 5 <= sum(a != b for a, b in zip(pre, snp)) <= 40
    for name in ("unrelated3k", "unrelated6k", "unrelated8k"):
        (_, u), (_, v) = di.SETS[name]()
        assert len(u) == len(v) == int(name[9]) * 1000 and u != v


def test_copied_constants_are_the_kernels():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "seqrush_amd", "csrc", "sr_blk_tile.inc")).read()
    assert int(re.search(r"#define SR_DEEP_INT16 (\d+)", src).group(1)) == di.SR_DEEP_INT16
    assert int(re.search(r"#define SR_DEEP_RING16 (\d+)", src).group(1)) == di.SR_DEEP_RING16


@pytest.mark.parametrize("scores", di.CLOSED_FORM_SCORES)
@pytest.mark.parametrize("name", sorted(di.GAP))
def test_one_gap_sets_score_the_closed_form(name, scores):
    """target = prefix / suffix of the query, or the query with a hole: the optimum is one gap of g, min(o1 + g e1, o2 + g e2),
    in both orders (insertion and deletion), on the forward strand"""
    ref = reference()[name, scores]
    assert sorted(ref) == [(0, 1), (1, 0)]
    for r in ref.values():
        assert r["score"] == di.gap_score(scores, di.GAP[name]), (name, scores)
        assert not r.get("is_reverse", False)
    assert di.gap_score(di.DEFAULT, 11000) == 24 + 11000 and di.gap_score(di.ONE_PIECE, 8000) == 8 + 16000
    assert di.gap_score(di.GENERIC, 10000) == 13 + 10000 and di.gap_score(di.DEFAULT, 10) == 8 + 20


@pytest.mark.parametrize("name,scores", sorted(ALIGNED | SCORED))
def test_oracle_equals_gotoh_and_its_cigar_costs_its_score(name, scores):
    ref = reference()[name, scores]
    n = len(di.SETS[name]())
    assert len(ref) == n * (n - 1)
    fits = 0
    for (q, t), r in ref.items():
        if r["gotoh"] is not None:
            assert r["score"] == r["gotoh"], (name, scores, q, t)
            fits += 1
        if "cigar" in r:
            assert ob.cigar_score(r["cigar"], r["strand_q"], r["t_seq"], pen_of(scores)) == r["score"], (name, scores, q, t)
    assert fits == len(ref) or name == "prefix30k"


def test_unrelated_sets_are_nothing_but_mismatches_and_gaps():
    """no optimal alignment of two independent sequences holds a long match run: the wavefront never collapses onto a few
    diagonals, and the score is about two per base"""
    for name in ("unrelated3k", "unrelated6k", "unrelated8k"):
        L = int(name[9]) * 1000
        for r in reference()[name, di.DEFAULT].values():
            assert 1.9 * L <= r["score"] <= 2.1 * L
            assert max(len(m) for m in re.split(rb"[XID]+", r["cigar"])) < 40


def test_deep_then_shallow_holds_both():
    ref = reference()["deep_then_shallow", di.DEFAULT]
    assert ref[0, 1]["score"] == ref[1, 0]["score"] == di.gap_score(di.DEFAULT, 11000)
    assert 0 < ref[1, 2]["score"] == ref[2, 1]["score"] < 200                    # a few substitutions
    assert ref[0, 2]["score"] > ref[0, 1]["score"]


@pytest.mark.parametrize("instance,name,scores", di.CASES)
def test_sets_reach_the_deep_regime(instance, name, scores):
    """conditions on the inputs, not measurements: the deepest pair of every case the device suite runs on a packed tile
    runs score // 2 levels per side, past the advisor's estimate (di.NEED) -- or, for the listed cases that cannot at these
    sizes, at least 1000 levels into the reset branch"""
    deepest = max(r["score"] for r in reference()[name, scores].values()) // 2
    assert deepest >= di.levels_needed(instance, name, scores), (instance, name, scores, deepest)
    short = (instance, name, scores) in di.SHORT_OF_ESTIMATE
    assert short == (deepest < di.NEED[instance]), "SHORT_OF_ESTIMATE lists exactly the cases below the estimate"
    assert di.NEED == {"ring16": 3300 + 1500, "int16": 6600 + 1000}
    assert name in (di.RING16_SETS if instance == "ring16" else di.INT16_SETS) or scores != di.DEFAULT
