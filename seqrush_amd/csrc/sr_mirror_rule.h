// sr_mirror_rule.h -- when the alignment of (t, q) is the transpose of the alignment of (q, t) (blocked kernel: mirrored
// emission, sr_align_blk.inc; host twins sr_mirror_* in sr_twins.cpp, which tests/test_mirror_host.py checks by enumeration),
// shared like sr_base_cone.h.  DESIGN.md section 4.3.
//
// Transposing a pair swaps pattern and text: diagonal k becomes -k, I becomes D, offsets (furthest-reaching points) and
// scores stay.  The rules of oracle/wfa.c see the orientation in exactly two places:
//   1. the M step of the backtrace: candidates with the same (maximum) offset are ranked by their tag,
//        MISMS > D2e > D2o > D1e > D1o > I2e > I2o > I1e > I1o                    (this pair)
//        MISMS > I2e > I2o > I1e > I1o > D2e > D2o > D1e > D1o                    (the transposed pair, in this pair's terms)
//      so the two orders pick different tags iff the maximum is reached by an I tag and by a D tag and not by MISMS;
//   2. the breakpoint choice of a bidirectional overlap call: among the candidates of the smallest value the walk takes the
//      earliest (distance i, component in the order D2 I2 D1 I1 M), then the smallest diagonal; the transposed pair walks
//      I2 D2 I1 D1 M and takes the largest diagonal (its smallest).
// A pair in which neither place ever has to decide is "tie-free": the CIGAR of (t, q) is the CIGAR of (q, t) with I and
// D swapped.  Flagging more than that is allowed (the pair is aligned both ways, as before), flagging less is not.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SR_MIR_HD __host__ __device__
#else
#define SR_MIR_HD
#endif

// SrAlignArgs::mirror, one entry per pair of a batch: the partner's index inside the batch, top bit = this pair is the
// secondary (skipped when dequeued; written or aligned by its primary's workgroup)
#define SR_MIRROR_NONE 0xffffffffu
#define SR_MIRROR_SECONDARY 0x80000000u
// bfs_backtrace's return value: error bits | this bit when an M step was tie-sensitive
#define SR_MIRROR_BT_TIE (1 << 30)

// backtrace tags (oracle/wfa.c: priority = numeric value)
enum { SR_BT_I1_OPEN = 1, SR_BT_I1_EXT = 2, SR_BT_I2_OPEN = 3, SR_BT_I2_EXT = 4,
       SR_BT_D1_OPEN = 5, SR_BT_D1_EXT = 6, SR_BT_D2_OPEN = 7, SR_BT_D2_EXT = 8, SR_BT_MISMS = 9 };

// priority the transposed pair gives the tag (its D is this pair's I)
SR_MIR_HD inline int sr_mirror_bt_rank_t(int tag) { return tag == SR_BT_MISMS ? tag : (tag <= SR_BT_I2_EXT ? tag + 4 : tag - 4); }
// best_tag / best_off: what this pair's order picked (maximum offset, highest tag among equals); best_ins_off: the largest
// offset of any I tag (negative: none).  Among equals a D tag outranks every I tag here, so the orders differ iff a D tag
// won and an I tag reaches the same offset.
SR_MIR_HD inline bool sr_mirror_bt_tie(int best_tag, int best_off, int best_ins_off) {
    return best_tag >= SR_BT_D1_OPEN && best_tag <= SR_BT_D2_EXT && best_ins_off == best_off;
}

// walk rank of a component (sr_internal.h SR_C_*: M 0, I1 1, I2 2, D1 3, D2 4) in a breakpoint call: this pair's, the transposed pair's
SR_MIR_HD inline int sr_mirror_bp_rank(int c) { return c == 4 ? 0 : c == 2 ? 1 : c == 3 ? 2 : c == 1 ? 3 : 4; }
SR_MIR_HD inline int sr_mirror_bp_rank_t(int c) { return c == 2 ? 0 : c == 4 ? 1 : c == 1 ? 2 : c == 3 ? 3 : 4; }
SR_MIR_HD inline int sr_mirror_bp_comp(int rank) { return rank == 0 ? 4 : rank == 1 ? 2 : rank == 2 ? 3 : rank == 3 ? 1 : 0; }
SR_MIR_HD inline int sr_mirror_bp_comp_t(int rank) { return rank == 0 ? 2 : rank == 1 ? 4 : rank == 2 ? 1 : rank == 3 ? 3 : 0; }
// the two packed keys of a candidate (value + bias, walk order, diagonal): the smallest key of a call is the candidate the
// respective walk accepts.  ord = i * 5 + rank < 1024, |k| < 2^30.
SR_MIR_HD inline unsigned long long sr_mirror_bp_key(unsigned val_biased, int i, int c, int k) {
    return ((unsigned long long)val_biased << 42) | ((unsigned long long)(unsigned)(i * 5 + sr_mirror_bp_rank(c)) << 32) |
           (unsigned long long)(unsigned)(k + (1 << 30));
}
SR_MIR_HD inline unsigned long long sr_mirror_bp_key_t(unsigned val_biased, int i, int c, int k) {
    return ((unsigned long long)val_biased << 42) | ((unsigned long long)(unsigned)(i * 5 + sr_mirror_bp_rank_t(c)) << 32) |
           (unsigned long long)(unsigned)((1 << 30) - k);
}
// the call is tie-sensitive iff the two winners name different (component, diagonal) (their value and distance are equal)
SR_MIR_HD inline bool sr_mirror_bp_tie(unsigned long long key, unsigned long long key_t) {
    const int ord = (int)((key >> 32) & 1023ull), ord_t = (int)((key_t >> 32) & 1023ull);
    const int c = sr_mirror_bp_comp(ord % 5), c_t = sr_mirror_bp_comp_t(ord_t % 5);
    const int k = (int)(unsigned)(key & 0xffffffffull) - (1 << 30), k_t = (1 << 30) - (int)(unsigned)(key_t & 0xffffffffull);
    return c != c_t || k != k_t;
}

// ---- replay of a tied secondary from its primary's breakpoints (DESIGN.md 4.3 "Replay") -------------------------------
// A breakpoint search is a function of its segment (pb, pe, tb, te, begin / end component) alone.  By the symmetry above the
// search of the transposed segment finds the transposed breakpoint -- bv <-> bh, component I <-> D, the same two scores --
// unless one of its accepted overlap calls was tie-sensitive (rule 2).  A primary that has a partner therefore keeps one
// record per search; the secondary, when the same workgroup aligns it next, takes the breakpoint of every segment whose
// transposed record exists and carries no tie bit, and searches the others.  Base cases are always recomputed (rule 1).
// Record: SR_BPREC_INTS ints, appended level by level in list order.
#define SR_BPREC_INTS 16
#define SR_BPREC_MAX 2048            // records a workgroup keeps per primary (later searches are not recorded: searched again)
enum { SR_BR_LEVEL = 0, SR_BR_PB, SR_BR_PE, SR_BR_TB, SR_BR_TE, SR_BR_CB, SR_BR_CE, SR_BR_BV, SR_BR_BH, SR_BR_BCOMP, SR_BR_BSF,
       SR_BR_BSR, SR_BR_TIE, SR_BR_CELLS_LO, SR_BR_CELLS_HI, SR_BR_PASSES };
// component of the transposed pair: I1 <-> D1, I2 <-> D2 (sr_internal.h SR_C_*: M 0, I1 1, I2 2, D1 3, D2 4)
SR_MIR_HD inline int sr_mirror_comp_t(int c) { return c == 0 ? 0 : (c <= 2 ? c + 2 : c - 2); }
// field f of the transposed record, read from record r (any pointer-like type): pb/pe <-> tb/te, bv <-> bh, components
// mapped; level, scores, tie bit and tallies as they are.  An involution.
template <typename P>
SR_MIR_HD inline int sr_bprec_t(P r, int f) {
    switch (f) {
    case SR_BR_PB: return r[SR_BR_TB];
    case SR_BR_PE: return r[SR_BR_TE];
    case SR_BR_TB: return r[SR_BR_PB];
    case SR_BR_TE: return r[SR_BR_PE];
    case SR_BR_CB: return sr_mirror_comp_t(r[SR_BR_CB]);
    case SR_BR_CE: return sr_mirror_comp_t(r[SR_BR_CE]);
    case SR_BR_BV: return r[SR_BR_BH];
    case SR_BR_BH: return r[SR_BR_BV];
    case SR_BR_BCOMP: return sr_mirror_comp_t(r[SR_BR_BCOMP]);
    default: return r[f];
    }
}
// Two-pointer walk of a level.  Both lists are in list order; the segments under search of one level are disjoint pieces
// of one monotone path and none is empty, so pb + tb grows strictly along either list (and is the same for a segment and
// its transpose).  One step compares the record at hand with the segment at hand (its first six ints: pb pe tb te cb ce):
//   < 0: the record lies before the segment -> next record;  > 0: behind it -> the segment has no record, next segment;
//   0: same place -> next of both, and the segment is matched iff sr_replay_same().
template <typename P, typename Q>
SR_MIR_HD inline int sr_replay_cmp(P rec, Q seg) { return (rec[SR_BR_PB] + rec[SR_BR_TB]) - (seg[0] + seg[2]); }
template <typename P, typename Q>
SR_MIR_HD inline bool sr_replay_same(P rec, Q seg) {
    return sr_bprec_t(rec, SR_BR_PB) == seg[0] && sr_bprec_t(rec, SR_BR_PE) == seg[1] && sr_bprec_t(rec, SR_BR_TB) == seg[2] &&
           sr_bprec_t(rec, SR_BR_TE) == seg[3] && sr_bprec_t(rec, SR_BR_CB) == seg[4] && sr_bprec_t(rec, SR_BR_CE) == seg[5];
}
