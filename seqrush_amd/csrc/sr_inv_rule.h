// sr_inv_rule.h -- the rule of --patch-inversions (the reference's inversion-aware runner, src/inversion_aware_seqrush.rs:118-255
// over src/cigar_analysis.rs:23-147), shared by the device scan (sr_inv.hip) and the host twins (sr_host.cpp), like
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
