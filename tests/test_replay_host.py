"""Host tests of the replay of a tied secondary (DESIGN.md 4.3 "Replay", csrc/sr_mirror_rule.h): the transposition of a
breakpoint record, the walk that matches a level's segments against the primary's records (sr_replay_match_host, the twin of
the kernel's loop: the same shared predicates), and the oracle-side precondition the GPU tests lean on.  No GPU."""
import ctypes as C
import random

import mirror_inputs as mi
from seqrush_amd import _lib

M, I1, I2, D1, D2 = range(5)
COMP_T = {M: M, I1: D1, I2: D2, D1: I1, D2: I2}
FIELDS = ("level", "pb", "pe", "tb", "te", "cb", "ce", "bv", "bh", "bcomp", "bsf", "bsr", "tie", "cells_lo", "cells_hi", "passes")
MAXSEG = 4096                      # SR_BFS_MAXSEG (csrc/sr_internal.h)


def L():
    return _lib.load()


def ints(v):
    return (C.c_int * max(1, len(v)))(*v)


def rec(level, pb, pe, tb, te, cb=M, ce=M, bv=1, bh=1, bcomp=M, bsf=10, bsr=12, tie=0, cells=1000, passes=3):
    return [level, pb, pe, tb, te, cb, ce, bv, bh, bcomp, bsf, bsr, tie, cells & 0xffffffff, cells >> 32, passes]


def transpose(r):
    out = (C.c_int * 16)()
    L().sr_replay_transpose_host(ints(r), out)
    return list(out)


def seg_of(r):
    """the segment a record was written for, as the kernel's list holds it"""
    return r[1:7]


def seg_t(r):
    """the segment of the transposed pair that a record speaks about"""
    return seg_of(transpose(r))


def match(recs, segs, level):
    flat_r = [x for r in recs for x in r]
    flat_s = [x for s in segs for x in s]
    out = (C.c_int * max(1, len(segs)))()
    n = L().sr_replay_match_host(ints(flat_r), len(recs), ints(flat_s), len(segs), level, out)
    got = list(out)[:len(segs)]
    assert n == sum(1 for x in got if x >= 0)
    return got


def test_record_layout():
    assert L().sr_replay_record_ints() == len(FIELDS) == 16


def test_transposition_is_an_involution_and_maps_components():
    rng = random.Random(5)
    for _ in range(200):
        r = [rng.randrange(0, 100000) for _ in FIELDS]
        for f in (5, 6, 9):
            r[f] = rng.randrange(5)
        t = transpose(r)
        assert transpose(t) == r
        d, e = dict(zip(FIELDS, r)), dict(zip(FIELDS, t))
        assert (e["pb"], e["pe"], e["tb"], e["te"]) == (d["tb"], d["te"], d["pb"], d["pe"])
        assert (e["bv"], e["bh"]) == (d["bh"], d["bv"])
        for f in ("cb", "ce", "bcomp"):
            assert e[f] == COMP_T[d[f]]
        for f in ("level", "bsf", "bsr", "tie", "cells_lo", "cells_hi", "passes"):
            assert e[f] == d[f]
    assert [COMP_T[c] for c in range(5)] == [transpose(rec(0, 0, 1, 0, 1, cb=c))[5] for c in range(5)]


def level_of(cuts, level, **kw):
    """records of one level of a primary: segments between consecutive (p, t) cut points of one monotone path"""
    return [rec(level, p0, p1, t0, t1, **kw) for (p0, t0), (p1, t1) in zip(cuts[:-1], cuts[1:])]


def test_all_matched():
    recs = level_of([(0, 0), (900, 950), (2100, 2000), (3000, 3100)], 2)
    recs[1][5], recs[1][6], recs[1][9] = I1, D2, I2
    assert match(recs, [seg_t(r) for r in recs], 2) == [0, 1, 2]
    # records of other levels around them are passed over
    before, after = level_of([(0, 0), (3000, 3100)], 0) + level_of([(0, 0), (2100, 2000), (3000, 3100)], 1), level_of([(0, 0), (5, 5)], 3)
    assert match(before + recs + after, [seg_t(r) for r in recs], 2) == [3, 4, 5]
    # the segments of the primary itself (not transposed) are somebody else's
    assert match(recs, [seg_of(r) for r in recs], 2) == [-1, -1, -1]


def test_flagged_search_and_its_children():
    """a tie bit: the segment is searched, and splits where the transposed walk splits -- its two children meet no record"""
    top = level_of([(0, 0), (1000, 1040), (2000, 2100)], 1)
    top[1][12] = 1                                          # the second search was tie-sensitive
    top[0][7], top[0][8] = 400, 420                         # breakpoints (bv, bh) inside the segments
    top[1][7], top[1][8] = 500, 530
    assert match(top, [seg_t(r) for r in top], 1) == [0, -1]
    kids = level_of([(0, 0), (400, 420), (1000, 1040), (1500, 1570), (2000, 2100)], 2)
    segs = [seg_t(r) for r in kids]
    # the secondary's own search of the flagged segment split one diagonal away
    segs[2] = [segs[2][0], segs[2][1] + 1, segs[2][2], segs[2][3], segs[2][4], segs[2][5]]
    segs[3] = [segs[3][0] + 1, segs[3][1], segs[3][2], segs[3][3], segs[3][4], segs[3][5]]
    assert match(top + kids, segs, 2) == [2, 3, -1, -1]
    # ... or at the same place through another component
    segs = [seg_t(r) for r in kids]
    segs[2][5], segs[3][4] = D1, D1
    assert match(top + kids, segs, 2) == [2, 3, -1, -1]


def test_unequal_components_do_not_match():
    recs = level_of([(0, 0), (700, 650), (1500, 1500)], 1)
    segs = [seg_t(r) for r in recs]
    segs[0][4] = D1                                         # begin component
    assert match(recs, segs, 1) == [-1, 1]
    segs = [seg_t(r) for r in recs]
    segs[1][5] = I2                                         # end component
    assert match(recs, segs, 1) == [0, -1]
    # the record's component I1 is the secondary's D1, not its I1
    recs[0][5] = I1
    segs = [seg_t(r) for r in recs]
    assert segs[0][4] == D1 and match(recs, segs, 1) == [0, 1]
    segs[0][4] = I1
    assert match(recs, segs, 1) == [-1, 1]


def test_empty_level_and_missing_records():
    recs = level_of([(0, 0), (700, 650), (1500, 1500)], 1)
    assert match(recs, [], 1) == []
    assert match([], [seg_t(r) for r in recs], 1) == [-1, -1]
    assert match(recs, [seg_t(r) for r in recs], 2) == [-1, -1]          # no record of that level
    # a segment between two records, a record between two segments
    more = level_of([(0, 0), (300, 310), (700, 650), (1100, 1000), (1500, 1500)], 3)
    segs = [seg_t(r) for r in more]
    assert match([more[0], more[2], more[3]], segs, 3) == [0, -1, 1, 2]
    assert match(more, [segs[0], segs[3]], 3) == [0, 3]


def test_level_at_half_the_segment_list():
    n = MAXSEG // 2
    cuts = [(0, 0)]
    rng = random.Random(11)
    for _ in range(n):
        cuts.append((cuts[-1][0] + rng.randrange(1, 40), cuts[-1][1] + rng.randrange(1, 40)))
    recs = level_of(cuts, 7)
    tied = set(rng.sample(range(n), 50))
    for i in tied:
        recs[i][12] = 1
    got = match(recs, [seg_t(r) for r in recs], 7)
    assert got == [-1 if i in tied else i for i in range(n)]


def test_oracle_transposes_exactly_off_the_non_transposable_pairs():
    """the precondition of the GPU tests: on these inputs the oracle's (t, q) CIGAR is the transpose of its (q, t) CIGAR exactly
    on the forward pairs non_transposable() does not list -- Input A has both kinds, the substitution family almost only one"""
    for name, at_least, at_most in (("A", 7, 7), ("subst", 0, 28)):
        o = mi.oracle_once(name)
        nt = set(o.non_transposable())
        assert at_least <= len(nt) <= at_most, (name, len(nt))
        for q in range(o.n):
            for t in range(q + 1, o.n):
                a, b = o.pairs[q, t], o.pairs[t, q]
                assert not a["is_reverse"] and not b["is_reverse"]
                assert (mi.transpose(a["cigar"]) == b["cigar"]) == ((q, t) not in nt), (name, q, t)
                assert a["score"] == b["score"]
