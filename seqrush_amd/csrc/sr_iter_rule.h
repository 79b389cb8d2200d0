// sr_iter_rule.h -- the stop rule of the iterative mode (--iterative, align_and_unite_iterative src/seqrush.rs:1034-1122),
// shared by the device decide kernel (sr_iter.hip) and the host twin sr_iterative_stop_host (sr_twins.cpp), like
// sr_sgd_term.h for the layout.  One check runs after every CHECK_INTERVAL random entries; the count is compared with
// the previous check's (the first check with the count after the tree entries), `stable` grows on equality and resets on
// a change, and the run stops at the check where it reaches STABILITY_THRESHOLD.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SR_ITER_HD __host__ __device__
#else
#define SR_ITER_HD
#endif

#define SR_ITER_CHECK_INTERVAL 10          // random entries between two component counts (:1037)
#define SR_ITER_STABILITY_THRESHOLD 10     // unchanged checks in a row that stop the run (:1036)

struct SrIterState {
    unsigned long long prev;    // count of the previous check (post_tree before the first)
    uint32_t stable;            // unchanged checks in a row
    uint32_t stopped;           // 1 once the rule fired: later unites, counts and decisions of the run do nothing
    uint32_t stop_check;        // 0-based index of the check that fired
    uint32_t pad;
};

// one check: `count` components after check number `check` (0-based, counted over the whole phase 2)
SR_ITER_HD inline void sr_iter_step(SrIterState *s, unsigned long long count, uint32_t check) {
    if (s->stopped) return;
    if (count == s->prev) {
        s->stable += 1;
        if (s->stable >= SR_ITER_STABILITY_THRESHOLD) { s->stopped = 1; s->stop_check = check; return; }   // (break: prev stays)
    } else {
        s->stable = 0;
    }
    s->prev = count;
}
