// sr_inv_rule.h -- the rule of --patch-inversions (the reference's inversion-aware runner, src/inversion_aware_seqrush.rs:118-255
// over src/cigar_analysis.rs:23-147), shared by the device scan (sr_inv.hip) and the host twins (sr_inv_host.cpp), like
// sr_iter_rule.h for the iterative mode.
//   site       a match op ending at (qa, ta) opens a look-ahead over the ops after it, up to the next match op or the end of
//              the CIGAR: qgap = query-only + mismatch columns, tgap = target-only + mismatch columns (cigar_analysis.rs:54-78).
//              A gap before the first match op is never seen; one that runs to the end is.
//   kind       with threshold m: both >= m divergent, else qgap >= m query-only, else tgap >= m target-only, else none (:80-105)
//   candidate  divergent and max(qgap, tgap) / min(qgap, tgap) <= 1.5 (:131-147), here as 2 max <= 3 min in 64 bits: exact
//              for any 32-bit lengths, where the f64 quotient is not
//   threshold  m = min_size if given, else 2 k (inversion_aware_seqrush.rs:163,170); m = 0 is refused (every complementary
//              SNP would be an inversion)
//   job        pattern = reverse complement of the ALIGNED query's [qa, qa + qgap), text = target [ta, ta + tgap), same
//              penalties, orientation forced.  The reference flips the target segment (:272-276); this project flips the
//              query, because its strand flag and unite_matching_region put the reverse strand on the query side.  Own decision.
//              The patch's strand is the negation of the main strand.  With the main alignment on '+' the aligned query is
//              the forward query, forward range [qa, qa + qgap); on '-' it is the reverse complement, forward range
//              [len_q - qa - qgap, len_q - qa).  Either way the patch's first query position in ITS OWN alignment space
//              (forward for a '+' patch, reverse-complement space for a '-' patch, the reference's quirk) is
//              len_q - qa - qgap on '-' patches and the forward start on '+' patches -- the same number.
//   accept     0 <= inv_score < main_score / 2, integer halving (:191); with -d also inv_score <= max_score_for_divergence(
//              min(qgap, tgap), d) (:304-309).  Both fold into one per-job upper bound for the unite kernel's score filter.
// Joined mode (--inversion-join J, J >= 1; own rule, not the reference's): rc(s) against s nearly always matches a few bases
// near the centre, and that island is a match op that splits a real inversion's gap into two one-sided sites.  So:
//   anchor     a match op with len >= J.  Only anchors open and close sites; "match op" above reads "anchor".
//   island     a match op with len < J.  Its columns count towards qgap AND tgap, like X columns.
//   site cost  what the main alignment paid for the site's ops under the run's penalties: X len x; an I or D run
//              min(o1 + len e1, o2 + len e2) (single-piece: o1 + len e1); island 0.  The CIGAR is run-length, so every gap
//              run is one op and the sum over a whole CIGAR is the alignment's score; a site's cost is at most that.
//   accept     0 <= inv_score < site_cost / 2, integer halving, in place of the main-score test: joined SNP clusters pass
//              main / 2 (the whole alignment's score is large next to any one cluster) and fail against what the
//              alignment paid for that very gap.  The -d bound is as above.
//   J = 1      every match op is an anchor: the plain rule's sites, the joined accept test.  J > m is refused: an island of
//              m columns would be a candidate by itself.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SR_INV_HD __host__ __device__
#else
#define SR_INV_HD
#endif

enum { SR_INV_NONE = 0, SR_INV_DIVERGENT = 1, SR_INV_QUERY_ONLY = 2, SR_INV_TARGET_ONLY = 3 };

// one job of the patch pass, as the scan emits it (20 bytes): pair index in the context's list, alignment coordinates
struct SrInvJob { uint32_t pair, qa, qgap, ta, tgap; };

// the joined scan's record (24 bytes): the same, and what the main alignment paid for the site
struct SrInvJobJ { uint32_t pair, qa, qgap, ta, tgap; int32_t cost; };

// penalties as the joined scan needs them (SrPen's fields; two = 0: single-piece)
struct SrInvPen { int32_t x, o1, e1, o2, e2, two; };

SR_INV_HD inline int sr_inv_site_kind(unsigned long long qgap, unsigned long long tgap, unsigned long long m) {
    if (qgap >= m && tgap >= m) return SR_INV_DIVERGENT;
    if (qgap >= m) return SR_INV_QUERY_ONLY;
    if (tgap >= m) return SR_INV_TARGET_ONLY;
    return SR_INV_NONE;
}

SR_INV_HD inline int sr_inv_is_candidate(unsigned long long qgap, unsigned long long tgap, unsigned long long m) {
    if (sr_inv_site_kind(qgap, tgap, m) != SR_INV_DIVERGENT) return 0;
    const unsigned long long hi = qgap > tgap ? qgap : tgap, lo = qgap > tgap ? tgap : qgap;
    return 2ULL * hi <= 3ULL * lo ? 1 : 0;
}

// largest patch score the score rule accepts for a main alignment of score `main_score` (< 0: none)
SR_INV_HD inline int32_t sr_inv_score_bound(int32_t main_score) { return main_score < 0 ? -1 : main_score / 2 - 1; }

SR_INV_HD inline int sr_inv_accept_score(int32_t inv_score, int32_t main_score) {
    return inv_score >= 0 && inv_score <= sr_inv_score_bound(main_score) ? 1 : 0;
}

// ---- joined mode
// op: 0 match, 1 mismatch, anything else a gap run (either side); join_below = J.  An island costs 0.
SR_INV_HD inline int sr_inv_is_anchor(uint32_t op, uint32_t len, uint32_t join_below) { return op == 0 && len >= join_below ? 1 : 0; }

SR_INV_HD inline uint32_t sr_inv_op_cost(uint32_t op, uint32_t len, const SrInvPen &p) {
    if (op == 0) return 0;
    if (op == 1) return len * (uint32_t)p.x;
    const uint32_t c1 = (uint32_t)p.o1 + len * (uint32_t)p.e1;
    if (!p.two) return c1;
    const uint32_t c2 = (uint32_t)p.o2 + len * (uint32_t)p.e2;
    return c1 < c2 ? c1 : c2;
}

// largest patch score the site-cost rule accepts (< 0: none)
SR_INV_HD inline int32_t sr_inv_site_bound(int32_t site_cost) { return site_cost < 0 ? -1 : site_cost / 2 - 1; }

SR_INV_HD inline int sr_inv_accept_site(int32_t inv_score, int32_t site_cost) {
    return inv_score >= 0 && inv_score <= sr_inv_site_bound(site_cost) ? 1 : 0;
}
