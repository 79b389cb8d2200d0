// sr_pass_rule.h -- the tables of one pass of the blocked kernel (blk_setup of sr_blk_pass.inc; host twin sr_pass_tables_host in
// sr_twins.cpp, which tests/test_pass_rule_host.py checks against a serial restatement), shared like sr_base_cone.h.
//
// A pass computes the B levels s0 .. s0+B-1 of every active aligner.  Its tables have a per-level part -- the range
// [klo, khi] of diagonals a level can reach, for a base case intersected with the backward cone of its end, and the cells
// of the range, counted unclipped (what the oracle counts) and clipped (what runs) -- and a per-aligner part that needs the
// whole block: the window of 4-diagonal groups its tiles cover, their count, and the tiles of the aligners before it.
// The per-level part of one aligner does not depend on its other levels, so wave 0 computes it one (aligner, level) pair
// per lane, SR_PASS_LANES / B aligners per step (sr_pass_lane): a depth-0 search (two aligners) is one step of 2 B lanes
// instead of B dependent steps of two.  The per-aligner part takes one lane per aligner and only needs the block's first
// and last level, which it evaluates itself: neither part waits for the other.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SR_PASS_HD __host__ __device__ __forceinline__
#else
#define SR_PASS_HD inline
#endif

#define SR_PASS_LANES 64

// 4-diagonal groups a wave tile of a B-level block owns: 64 lanes less the halo lanes either side (KGeo of sr_blk_rows.inc)
SR_PASS_HD constexpr int sr_pass_own(int B) { return 64 - 2 * (B <= 5 ? 2 : (B + 3) / 4); }

// diagonals either side of 0 that level s of a search that began in component M (from_m) or in a gap component can reach
SR_PASS_HD int sr_pass_reach(int o1, int e1, int o2, int e2, bool two, int s, bool from_m) {
    int r;
    if (from_m) {
        r = (s >= o1 + e1) ? (s - o1) / e1 : 0;
        if (two && s >= o2 + e2) { const int r2 = (s - o2) / e2; r = r2 > r ? r2 : r; }
    } else {
        r = s / e1;
        if (two) { const int r2 = s / e2; r = r2 > r ? r2 : r; }
    }
    return r;
}

// (aligner, level) pair of a lane in step `step`: whole aligners only, B lanes each; false: the lane idles in this step
SR_PASS_HD bool sr_pass_lane(int lane, int step, int B, int &aligner, int &level) {
    const int per = SR_PASS_LANES / B, al = lane / B;
    aligner = step * per + al; level = lane - al * B;
    return al < per;
}
SR_PASS_HD int sr_pass_steps(int njobs, int B) { const int per = SR_PASS_LANES / B; return (njobs + per - 1) / per; }

// one level: reach Rw of the level; cone: the range is intersected with [kend - rb, kend + rb] (rb < 0: nothing).
// cells: the unclipped range's, ccells: the clipped range's (equal without a cone)
SR_PASS_HD void sr_pass_level(int Rw, int plen, int tlen, bool cone, int kend, int rb, int &klo, int &khi, int &cells, int &ccells) {
    klo = -plen > -Rw ? -plen : -Rw; khi = tlen < Rw ? tlen : Rw;
    cells = (khi >= klo) ? khi - klo + 1 : 0;
    if (cone) {
        klo = klo > kend - rb ? klo : kend - rb; khi = khi < kend + rb ? khi : kend + rb;
    }
    ccells = (khi >= klo) ? khi - klo + 1 : 0;
}

// the block: Rw = reach of its LAST level, mg = margin in diagonals (1: tight ring cover, scope + 1: wide), shift = the
// aligner's diagonal offset in its rows, own = groups a tile owns; cone: the window is also cut to the cone of the block's
// FIRST level (rb0, its widest) + 1.  -> groups [glo, ghi] (ghi = glo - 1: none) and the tiles nt that cover them
SR_PASS_HD void sr_pass_window(int Rw, int mg, int plen, int tlen, int shift, bool cone, int kend, int rb0, int own,
                               int &glo, int &ghi, int &nt) {
    int wlo = -plen - 1 > -Rw - mg ? -plen - 1 : -Rw - mg, whi = tlen + 1 < Rw + mg ? tlen + 1 : Rw + mg;
    if (cone) {
        wlo = wlo > kend - rb0 - 1 ? wlo : kend - rb0 - 1; whi = whi < kend + rb0 + 1 ? whi : kend + rb0 + 1;
        glo = (wlo + shift) >> 2; ghi = (whi >= wlo) ? (whi + shift) >> 2 : glo - 1;
    } else { glo = (wlo + shift) >> 2; ghi = (whi + shift) >> 2; }
    nt = (ghi - glo + own) / own;
    nt = nt > 0 ? nt : 0;
}
