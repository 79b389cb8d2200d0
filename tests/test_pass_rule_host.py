"""Host checks of the blocked kernel's pass tables (seqrush_amd/csrc/sr_pass_rule.h, used by blk_setup of sr_blk_pass.inc).

blk_setup writes, for the B levels of a pass and every active aligner, the per-level ranges jklo / jkhi (for a base case cut
to the backward cone of its end), the cells of the unclipped and of the clipped ranges, the window of 4-diagonal groups the
aligner's tiles cover, their number and the tile prefix.  The kernel computes the per-level part one (aligner, level) pair
per lane in steps of 64 / B aligners and the per-aligner part from the block's first and last level; the library's host twin
(sr_pass_tables_host) is organised the same way on the same header.  Here it is compared with a plain serial restatement of
the loop blk_setup was before -- one aligner after the other, its levels one after the other, the window from what the loop
left behind -- over a lattice of begin components, lengths, levels either side of the gap-open thresholds, both block
depths, tight and wide windows, the penalty sets the blocked instances serve, base cases from one block of levels up, and
batches of 1 .. BJ_MAX aligners with inactive ones in between (the lane chunks are crossed at 6 -> 7 and 12 -> 13)."""
import ctypes as C
import itertools

import pytest

import instance_matrix as im
from seqrush_amd import _lib

M, I1, I2, D1, D2 = range(5)             # SR_C_* of sr_internal.h
BJ_MAX = 32                              # aligners of a pass (2 x SR_BFS_MAXACT of the workgroup build)
LANES = 64
JOB_INTS = 7
SENTINEL = 123456789
PENALTIES = sorted({v[0] for v in im.LATTICE.values() if v[1] == "blk"} | {im.DEFAULT_SCORES, im.ONE_PIECE})
LENGTHS = (0, 1, 3, 40, 300)


def cdiv(a, b):
    """C's truncating division"""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b > 0) else -q


def kreach(pen, s, begin):
    """kreach of sr_blk_pass.inc as it was"""
    if begin == M:
        r = cdiv(s - pen.o1, pen.e1) if s >= pen.o1 + pen.e1 else 0
        if pen.two and s >= pen.o2 + pen.e2:
            r = max(r, cdiv(s - pen.o2, pen.e2))
    else:
        r = cdiv(s, pen.e1)
        if pen.two:
            r = max(r, cdiv(s, pen.e2))
    return r


def cone_reach(pen, left):
    """sr_cone_reach of sr_base_cone.h"""
    if left < 0:
        return -1
    e = pen.e2 if (pen.two and pen.e2 < pen.e1) else pen.e1
    return left // max(e, 1) + 1


def own(B):
    """KGeo<B>::OWN of sr_blk_rows.inc"""
    return 64 - 2 * (2 if B <= 5 else (B + 3) // 4)


def serial_setup(pen, B, tight, base, s0, job):
    """blk_setup as it was: one aligner, a loop over the block's levels, kwindow, the cone's cut of the window"""
    active, begin, plen, tlen, shift, kend, lj = job
    klo_l, khi_l, cells, ccells = [], [], 0, 0
    Rw = clo0 = chi0 = 0
    for j in range(B):
        Rw = kreach(pen, s0 + j, begin)
        klo, khi = max(-plen, -Rw), min(tlen, Rw)
        cells += khi - klo + 1 if khi >= klo else 0
        if base:
            rb = cone_reach(pen, lj - 1 - (s0 + j))
            klo, khi = max(klo, kend - rb), min(khi, kend + rb)
            if j == 0:
                clo0, chi0 = kend - rb, kend + rb
        klo_l.append(klo); khi_l.append(khi)
        ccells += khi - klo + 1 if khi >= klo else 0
    mg = 1 if tight else pen.scope + 1
    wlo, whi = max(-plen - 1, -Rw - mg), min(tlen + 1, Rw + mg)
    glo, ghi = (wlo + shift) >> 2, (whi + shift) >> 2
    if base:
        wlo, whi = max(wlo, clo0 - 1), min(whi, chi0 + 1)
        glo = (wlo + shift) >> 2
        ghi = (whi + shift) >> 2 if whi >= wlo else glo - 1
    nt = max(0, cdiv(ghi - glo + own(B), own(B)))
    return klo_l, khi_l, cells, ccells, glo, ghi, nt


def twin(pen, B, tight, base, s0, jobs, cells0=5):
    """sr_pass_tables_host on a batch -> (steps, klo[j][a], khi[j][a], cells, ccells, glo, ghi, nt, tstart)"""
    L = _lib.load()
    n = len(jobs)
    IA = lambda k, v=0: (C.c_int * max(k, 1))(*([v] * max(k, 1)))
    pen6 = (C.c_int * 6)(pen.x, pen.o1, pen.e1, pen.o2, pen.e2, 1 if pen.two else 0)
    flat = (C.c_int * max(n * JOB_INTS, 1))(*[v for j in jobs for v in j])
    klo, khi = IA(B * n, SENTINEL), IA(B * n, SENTINEL)
    cells, ccells = (C.c_longlong * max(n, 1))(*([cells0] * max(n, 1))), (C.c_longlong * max(n, 1))(*([cells0] * max(n, 1)))
    glo, ghi, nt, ts = IA(n, SENTINEL), IA(n, SENTINEL), IA(n, SENTINEL), IA(n + 1, SENTINEL)
    steps = L.sr_pass_tables_host(pen6, pen.scope, B, int(tight), int(base), s0, n, flat, klo, khi, cells, ccells, glo, ghi, nt, ts)
    assert steps >= 0
    return (steps, [[klo[j * n + a] for a in range(n)] for j in range(B)], [[khi[j * n + a] for a in range(n)] for j in range(B)],
            [cells[a] - cells0 for a in range(n)], [ccells[a] - cells0 for a in range(n)], list(glo)[:n], list(ghi)[:n], list(nt)[:n],
            list(ts)[:n + 1])


def check_batch(pen, B, tight, base, s0, jobs):
    steps, klo, khi, cells, ccells, glo, ghi, nt, ts = twin(pen, B, tight, base, s0, jobs)
    n = len(jobs)
    per = LANES // B
    assert steps == -(-n // per)
    assert ts[0] == 0
    tiles = 0
    for a, job in enumerate(jobs):
        what = (pen, B, tight, base, s0, a, job)
        if not job[0]:            # inactive: no range written, no cells, an empty window, no tiles
            assert all(klo[j][a] == SENTINEL and khi[j][a] == SENTINEL for j in range(B)), what
            assert (cells[a], ccells[a], glo[a], ghi[a], nt[a]) == (0, 0, 0, -1, 0), what
        else:
            w_klo, w_khi, w_cells, w_ccells, w_glo, w_ghi, w_nt = serial_setup(pen, B, tight, base, s0, job)
            assert [klo[j][a] for j in range(B)] == w_klo and [khi[j][a] for j in range(B)] == w_khi, what
            assert (cells[a], ccells[a]) == (w_cells, w_ccells), what
            assert (glo[a], ghi[a], nt[a]) == (w_glo, w_ghi, w_nt), what
            if not base:
                assert ccells[a] == cells[a], what
            tiles += w_nt
        assert ts[a + 1] == tiles, what
    return steps


def levels_of_interest(pen, B):
    """first levels of blocks whose levels lie below, across and above o1 + e1 and o2 + e2, and far above"""
    marks = {0, pen.o1 + pen.e1, 1000}
    if pen.two:
        marks.add(pen.o2 + pen.e2)
    out = set()
    for m in marks:
        b = m // B * B
        out.update(x for x in (b - B, b, b + B) if x >= 0)
    return sorted(out)


def batches(jobs, sizes):
    """cut a job list into batches of the sizes given (cycled), every fourth aligner of a batch inactive"""
    it, k = iter(sizes), 0
    while k < len(jobs):
        n = next(it)
        b = [list(j) for j in jobs[k:k + n]]
        for a in range(3, len(b), 4):
            b[a][0] = 0
        yield [tuple(j) for j in b]
        k += n


@pytest.mark.parametrize("B", [5, 10])
@pytest.mark.parametrize("scores", PENALTIES)
def test_search_tables_equal_the_serial_setup(scores, B):
    pen = im.parse_pen(scores)
    jobs = [(1, begin, plen, tlen, plen + 29, tlen - plen, 0)
            for begin in (M, I1, D1, I2, D2) for plen in LENGTHS for tlen in LENGTHS]
    seen = 0
    for s0 in levels_of_interest(pen, B):
        for tight in (False, True):
            for b in batches(jobs, itertools.cycle((1, 2, 6, 7, 12, 13, BJ_MAX, 5))):
                check_batch(pen, B, tight, False, s0, b)
                seen += len(b)
    assert seen >= 2 * 125 * 4


@pytest.mark.parametrize("B", [5, 10])
@pytest.mark.parametrize("scores", [im.DEFAULT_SCORES, im.ONE_PIECE, "0,5,8,2,13,1", "0,5,3,2", "0,40,8,2"])
def test_base_case_tables_equal_the_serial_setup(scores, B):
    pen = im.parse_pen(scores)
    empty = 0
    for lj in (B, 2 * B, 3 * B, 10 * B):
        jobs = [(1, begin, plen, tlen, max(plen, tlen) + 40, tlen - plen, lj)
                for begin in (M, I1, D1, I2, D2) for plen in LENGTHS for tlen in LENGTHS]
        for s0 in range(0, lj + B, B):                     # (the last block lies past the job's levels: nothing left of the cone)
            for b in batches(jobs, itertools.cycle((16, 1, 7, 13))):
                check_batch(pen, B, False, True, s0, b)
                _, klo, khi, _, ccells, glo, ghi, nt, _ = twin(pen, B, False, True, s0, b)
                for a, job in enumerate(b):
                    if job[0] and ccells[a] == 0 and ghi[a] < glo[a]:
                        assert nt[a] == 0
                        empty += 1
    assert empty > 0                                      # jobs whose clipped range is empty got no tiles


@pytest.mark.parametrize("B", [5, 10])
def test_lane_chunks(B):
    """1 .. BJ_MAX aligners: whole aligners per step, 64 / B of them; every active (aligner, level) pair is written once"""
    pen = im.parse_pen(im.DEFAULT_SCORES)
    per = LANES // B
    assert per == (6 if B == 10 else 12)
    steps = {}
    for n in range(1, BJ_MAX + 1):
        jobs = [(0 if (a % 5 == 2) else 1, M if a % 2 == 0 else D2, 40 + a, 300 - a, 40 + a + 29, 260 - 2 * a, 0) for a in range(n)]
        steps[n] = check_batch(pen, B, True, False, 3 * B, jobs)
    assert steps[per] == 1 and steps[per + 1] == 2 and steps[2 * per] == 2 and steps[2 * per + 1] == 3
    assert steps[BJ_MAX] == -(-BJ_MAX // per)
    assert int(_lib.load().sr_pass_tile_own(B)) == own(B)
