// sr_lift_rule.h -- the rule of the interval lift (--lift), shared by the kernels and the host twin of
// sr_lift.hip and by nothing else: the limits, the step of a path that holds a base, what one step of the query path
// contributes to the image of an interval in a target path, and how contributions combine.  Every quantity is a min, a max
// or a sum of integers, so the result does not depend on the order of evaluation and the two executions agree exactly.
//
// Tables: steps[S] = handle (node << 1 | reverse) of every step of every path back to back, node v = 1..V at index v - 1;
// len[V] >= 1; pstart[S] = the offset of a step in the oriented sequence of its own path.
#pragma once
#include <cstdint>
#include "sr_sgd_term.h"

#define SR_LIFT_MAX_PAIRS (1ULL << 26)         // queries x targets above this: SR_ERR_UNSUPPORTED
#define SR_LIFT_MAX_TABLE (1ULL << 28)         // targets x nodes (the first-visit table) above this: SR_ERR_UNSUPPORTED
#define SR_LIFT_VARIANT_HOST 0                 // sr_lift.variant: plain loops on the host
#define SR_LIFT_VARIANT_DEVICE 1
#define SR_LIFT_NONE 0xffffffffu               // first[B][v] of a node the target does not visit

struct SrLiftTables {
    const uint32_t *steps;                     // [S]
    const uint32_t *len;                       // [V]
    const uint64_t *pstart;                    // [S]
};

// the step of the path with steps [a0, a1), a0 < a1, that holds base x < plen: the last s with pstart[s] <= x (pstart
// rises strictly along a path because node lengths are >= 1)
SR_HD static inline uint32_t sr_lift_step_of(const uint64_t *pstart, uint32_t a0, uint32_t a1, uint64_t x) {
    uint32_t lo = a0, hi = a1;
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (pstart[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

// what the contributions of the steps of one (query, target) pair add up to
struct SrLiftAcc { uint64_t lo, hi, covered, rev_bp; };
SR_HD static inline SrLiftAcc sr_lift_empty() { return SrLiftAcc{~0ULL, 0, 0, 0}; }      // the identities of min, max and sum
SR_HD static inline SrLiftAcc sr_lift_join(const SrLiftAcc &a, const SrLiftAcc &b) {
    return SrLiftAcc{a.lo < b.lo ? a.lo : b.lo, a.hi > b.hi ? a.hi : b.hi, a.covered + b.covered, a.rev_bp + b.rev_bp};
}

// step s of the query path, handle (v, r), against the query [start, end) and the target's first step t = first[B][v]
// on the node, handle (v, r'): the overlap [o0, o1) of the query with the step in handle offsets goes to the same offsets
// of the target's handle when the strands agree, else to [len - o1, len - o0).  Nothing (the identities) when the target
// does not visit the node or the overlap is empty.
SR_HD static inline SrLiftAcc sr_lift_step(const SrLiftTables &g, uint32_t s, uint64_t start, uint64_t end, uint32_t t) {
    if (t == SR_LIFT_NONE) return sr_lift_empty();
    const uint32_t h = g.steps[s];
    const uint64_t n = g.len[(h >> 1) - 1], ps = g.pstart[s];
    const uint64_t a = start > ps ? start : ps, b = end < ps + n ? end : ps + n;
    if (a >= b) return sr_lift_empty();
    const uint64_t o0 = a - ps, o1 = b - ps, pt = g.pstart[t];
    const uint32_t sigma = (h ^ g.steps[t]) & 1u;
    const uint64_t lo = sigma ? n - o1 : o0, hi = sigma ? n - o0 : o1;
    return SrLiftAcc{pt + lo, pt + hi, o1 - o0, sigma ? o1 - o0 : 0};
}

// an unmapped pair is all zeros
SR_HD static inline SrLiftAcc sr_lift_finish(const SrLiftAcc &a) { return a.covered ? a : SrLiftAcc{0, 0, 0, 0}; }

// the strand of a mapped pair: reverse iff most of the covered bases map to the other strand
SR_HD static inline bool sr_lift_reverse(uint64_t covered, uint64_t rev_bp) { return 2 * rev_bp > covered; }
