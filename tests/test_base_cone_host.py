"""Host checks of the base cases' backward cone (seqrush_amd/csrc/sr_base_cone.h, used by blk_setup of the blocked kernel).

A base case ends in the cell (k_end = tlen - plen, offset tlen) of its end component within `lj` levels, so a level s only
needs the diagonals from which that end is still within reach: |k - k_end| <= sr_base_cone_reach(lj - 1 - s).  The kernel
clips every level's range to it.  Here a small pure-Python model of the five-component recurrences (same rules as the
tiles: ranges, limits, level 0, extension of M) records the sources of every non-NULL cell and checks, by brute force on
random short pairs, that

 * every ancestor of the end cell lies inside the cone the kernel's formula gives (the formula itself comes from the
   library: one source), for every end component and for one- and two-piece penalties, and
 * a search clipped to the cone reaches the end at the same level and backtraces to the same operations as the
   unclipped one -- also with a loose level budget, as a re-queued job has.
"""
import random

import pytest

from seqrush_amd import _lib

M, I1, D1, I2, D2 = range(5)
NUL = -(1 << 20)

# default, one-piece, and sets the exact (10-level) and generic (5-level) blocked instances serve (tests/instance_matrix.py)
PENALTIES = ["0,5,8,2,24,1", "0,5,8,2", "0,5,8,2,14,1", "0,5,8,2,9,1", "0,5,8,2,13,1", "0,5,8,2,4,1", "0,5,3,2", "0,6,8,2",
             "0,5,7,2", "0,40,8,2", "0,5,8,2,72,1"]


def parse(scores):
    v = [int(x) for x in scores.split(",")]
    two = len(v) == 6
    return dict(x=v[1], o1=v[2], e1=v[3], o2=v[4] if two else 0, e2=v[5] if two else 0, two=two)


def cone_reach(pen, left):
    return int(_lib.load().sr_base_cone_reach(pen["e1"], pen["e2"], 1 if pen["two"] else 0, left))


def fwd_reach(pen, s, begin):
    """kreach of sr_blk_pass.inc"""
    if begin == M:
        r = (s - pen["o1"]) // pen["e1"] if s >= pen["o1"] + pen["e1"] else 0
        if pen["two"] and s >= pen["o2"] + pen["e2"]:
            r = max(r, (s - pen["o2"]) // pen["e2"])
    else:
        r = s // pen["e1"]
        if pen["two"]:
            r = max(r, s // pen["e2"])
    return r


def search(P, T, pen, begin, end, max_levels, lj=None):
    """level by level until component `end` of diagonal tlen - plen holds offset tlen.  lj: clip every level to the cone
    of that budget.  -> (end level or None, cells {(s, comp, k): offset}, sources {(s, comp, k): [(s', comp', k')]})"""
    plen, tlen = len(P), len(T)
    kend = tlen - plen
    cells, srcs = {}, {}

    def get(s, c, k):
        return cells.get((s, c, k), NUL) if s >= 0 else NUL

    for s in range(max_levels):
        R = fwd_reach(pen, s, begin)
        klo, khi = max(-plen, -R), min(tlen, R)
        if lj is not None:
            r = cone_reach(pen, lj - 1 - s)
            klo, khi = max(klo, kend - r), min(khi, kend + r)
        for k in range(klo, khi + 1):
            lim = min(tlen, plen + k)

            def bnd(v):
                return v if 0 <= v <= lim else NUL
            if s == 0:
                if k == 0:
                    cells[(0, begin, 0)] = 0
                    srcs[(0, begin, 0)] = []
                val = {c: get(0, c, k) for c in range(5)}
            else:
                val, sc = {}, {}
                pieces = [(I1, D1, pen["o1"], pen["e1"])] + ([(I2, D2, pen["o2"], pen["e2"])] if pen["two"] else [])
                for ci, cd, o, e in pieces:
                    a = [(s - o - e, M, k - 1), (s - e, ci, k - 1)]
                    val[ci] = bnd(max(get(*q) for q in a) + 1)
                    sc[ci] = a
                    b = [(s - o - e, M, k + 1), (s - e, cd, k + 1)]
                    val[cd] = bnd(max(get(*q) for q in b))
                    sc[cd] = b
                m = bnd(get(s - pen["x"], M, k) + 1)
                sc[M] = [(s - pen["x"], M, k)]
                for c in val:
                    m = max(m, val[c])
                    sc[M].append((s, c, k))
                val[M] = m
                for c, v in val.items():
                    if v >= 0:
                        cells[(s, c, k)] = v
                        srcs[(s, c, k)] = [q for q in sc[c] if get(*q) >= 0]
            m = val.get(M, NUL)
            if m >= 0:                                 # extension
                while m < lim and P[m - k] == T[m]:
                    m += 1
                cells[(s, M, k)] = m
        if klo <= kend <= khi and get(s, end, kend) >= tlen:
            return s, cells, srcs
    return None, cells, srcs


def backtrace(cells, pen, plen, tlen, begin, end, score):
    """bfs_backtrace of sr_align_bfs.inc: same candidates, same order of preference; a cell that is not stored is NULL"""
    def get(s, c, k):
        return cells.get((s, c, k), NUL) if s >= 0 else NUL
    ops = []
    s, k, comp, o = score, tlen - plen, end, tlen
    for _ in range(4 * (plen + tlen) + 64):
        lim = min(tlen, plen + k)

        def bnd(v):
            return v if 0 <= v <= lim else NUL
        if comp == M:
            if s == 0:
                assert begin == M and k == 0
                ops.append(("M", o))
                return ops
            cand = [(bnd(get(s - pen["x"], M, k) + 1), 9)]
            cand += [(bnd(get(s - pen["o1"] - pen["e1"], M, k - 1) + 1), 1), (bnd(get(s - pen["o1"] - pen["e1"], M, k + 1)), 5),
                     (bnd(get(s - pen["e1"], I1, k - 1) + 1), 2), (bnd(get(s - pen["e1"], D1, k + 1)), 6)]
            if pen["two"]:
                cand += [(bnd(get(s - pen["o2"] - pen["e2"], M, k - 1) + 1), 3), (bnd(get(s - pen["o2"] - pen["e2"], M, k + 1)), 7),
                         (bnd(get(s - pen["e2"], I2, k - 1) + 1), 4), (bnd(get(s - pen["e2"], D2, k + 1)), 8)]
            bo, bty = NUL, 0
            for v, ty in cand:                          # bt_best: equal offsets -> the higher type
                if v >= 0 and (v > bo or (v == bo and ty > bty)):
                    bo, bty = v, ty
            assert bty and bo <= o
            ops.append(("M", o - bo))
            o = bo
            ops.append(("X" if bty == 9 else "I" if bty <= 4 else "D", 1))
            if bty == 9:
                o -= 1; s -= pen["x"]
            elif bty <= 4:
                o -= 1; k -= 1
                s -= {1: pen["o1"] + pen["e1"], 2: pen["e1"], 3: pen["o2"] + pen["e2"], 4: pen["e2"]}[bty]
                comp = {1: M, 2: I1, 3: M, 4: I2}[bty]
            else:
                k += 1
                s -= {5: pen["o1"] + pen["e1"], 6: pen["e1"], 7: pen["o2"] + pen["e2"], 8: pen["e2"]}[bty]
                comp = {5: M, 6: D1, 7: M, 8: D2}[bty]
        else:
            if s == 0:
                assert comp == begin and k == 0 and o == 0
                return ops
            ins = comp in (I1, I2)
            go, ge = (pen["o1"], pen["e1"]) if comp in (I1, D1) else (pen["o2"], pen["e2"])
            kk = k - 1 if ins else k + 1
            c_open = bnd(get(s - go - ge, M, kk) + (1 if ins else 0))
            c_ext = bnd(get(s - ge, comp, kk) + (1 if ins else 0))
            ext = c_ext >= 0 and c_ext >= c_open
            assert ext or c_open >= 0
            assert (c_ext if ext else c_open) == o
            ops.append(("I" if ins else "D", 1))
            if ins:
                o -= 1
            k = kk
            if ext:
                s -= ge
            else:
                s -= go + ge; comp = M
        assert s >= 0
    raise AssertionError("backtrace did not end")


def pairs(seed):
    """short random pairs: substitutions, a few short indels, one long gap (start, end or middle), ragged lengths"""
    rng = random.Random(seed)
    out = []
    for i in range(6):
        L = rng.randint(10, 24)
        a = [rng.choice("ACGT") for _ in range(L)]
        b = list(a)
        for _ in range(rng.randint(0, 3)):
            j = rng.randrange(len(b)); b[j] = rng.choice("ACGT")
        kind = i % 6
        g = rng.randint(3, 9)
        if kind == 1:
            b = b[g:]
        elif kind == 2:
            b = b[:-g]
        elif kind == 3:
            j = rng.randrange(1, len(b)); b[j:j] = [rng.choice("ACGT") for _ in range(g)]
        elif kind == 4:
            j = rng.randrange(1, max(2, len(b) - g)); del b[j:j + g]
        elif kind == 5:
            b = b[:max(3, L // 4)]
        if rng.random() < 0.5:
            a, b = b, a
        out.append(("".join(a), "".join(b)))
    return out


def test_formula_is_monotone_and_wide_enough():
    for sc in PENALTIES:
        pen = parse(sc)
        emin = min(pen["e1"], pen["e2"]) if pen["two"] else pen["e1"]
        prev = -1
        for left in range(0, 400):
            r = cone_reach(pen, left)
            assert r >= left // emin and r >= prev
            prev = r
        assert cone_reach(pen, -1) < 0 or cone_reach(pen, -1) <= cone_reach(pen, 0)


@pytest.mark.parametrize("scores", PENALTIES)
def test_ancestors_of_the_end_lie_in_the_cone_and_clipping_changes_nothing(scores):
    pen = parse(scores)
    ends = [M, I1, D1] + ([I2, D2] if pen["two"] else [])
    seen = 0
    for P, T in pairs(sum(map(ord, scores))):
        plen, tlen = len(P), len(T)
        kend = tlen - plen
        for end in ends:
            cap = pen["o1"] + (pen["o2"] if pen["two"] else 0) + (plen + tlen + 2) * max(pen["x"], pen["e1"], pen["e2"]) + 8
            cap = min(cap, 200)
            score, cells, srcs = search(P, T, pen, M, end, cap)
            if score is None:
                continue
            seen += 1
            # closure: every ancestor of the end cell, at the tightest budget (lj = score + 1)
            todo, anc = [(score, end, kend)], set()
            while todo:
                c = todo.pop()
                if c in anc:
                    continue
                anc.add(c)
                todo.extend(srcs.get(c, []))
            for s, c, k in anc:
                assert abs(k - kend) <= cone_reach(pen, score - s), (scores, P, T, end, (s, c, k))
            ops = backtrace(cells, pen, plen, tlen, M, end, score)
            # clipped searches: tight budget, the kernel's rounding to a block, a loose (re-queued) budget
            for lj in (score + 1, ((score + pen["o1"] + 2) // 10 + 1) * 10, score + 57):
                s2, cells2, _ = search(P, T, pen, M, end, lj, lj=lj)
                assert s2 == score, (scores, P, T, end, lj)
                assert backtrace(cells2, pen, plen, tlen, M, end, score) == ops
                assert len(cells2) <= len(cells)
                assert all(cells[c] == v for c, v in cells2.items() if abs(c[2] - kend) <= cone_reach(pen, lj - 1 - c[0]))
    assert seen >= 6
