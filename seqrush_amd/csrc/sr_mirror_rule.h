// sr_mirror_rule.h -- when the alignment of (t, q) is the transpose of the alignment of (q, t) (blocked kernel: mirrored
// emission, sr_align_blk.inc; host twins sr_mirror_* in sr_host.cpp, which tests/test_mirror_host.py checks by enumeration),
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
