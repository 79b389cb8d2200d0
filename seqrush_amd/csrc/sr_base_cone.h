// sr_base_cone.h -- the backward cone of a base case (blocked kernel, blk_setup; host twin sr_base_cone_reach in sr_twins.cpp,
// which tests/test_base_cone_host.py checks against a brute-force model of the recurrences), shared like sr_iter_rule.h.
//
// A base case ends in the cell (k_end = tlen - plen, offset tlen) of its end component, at a level below the lj levels it
// was given.  A cell of level s can lie on a path to that end only if the levels that are left, lj - 1 - s, pay for the
// diagonals between it and k_end: every step of the recurrences that changes the diagonal by one -- opening or extending a
// gap, either piece -- costs at least min(e1, e2) levels, mismatches and extension stay on their diagonal.  So
//     |k - k_end| <= (lj - 1 - s) / min(e1, e2)
// for every cell of every component that the end descends from, whatever the end component: the bound is tight for the
// joint range of the five components (a cell of I2 / D2 extends to the end diagonal at e2 per step and closes into M for
// free), and the per-level ranges jklo / jkhi are shared by the components.  The cone is closed under the recurrences: a
// source of a cell of level s lies at level s' <= s - min(e1, e2) when it lies on a neighbour diagonal, and
// (lj - 1 - s) / e + 1 <= (lj - 1 - s') / e.  Any upper bound of the end level serves as lj (a re-queued job carries the
// worst case: a loose cone, still valid).  One diagonal of slack: err wide, never narrow.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SR_CONE_HD __host__ __device__
#else
#define SR_CONE_HD
#endif

// diagonals either side of k_end that a level with `left` levels to go (lj - 1 - s) has to keep; < 0: none (left < 0)
SR_CONE_HD inline int sr_cone_reach(int e1, int e2, bool two, int left) {
    if (left < 0) return -1;
    const int e = (two && e2 < e1) ? e2 : e1;
    return left / (e > 0 ? e : 1) + 1;
}
