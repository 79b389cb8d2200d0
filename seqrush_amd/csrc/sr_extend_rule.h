// sr_extend_rule.h -- the rules of --extend, shared by the kernels and the host twin of
// sr_extend.hip: which step spells a base of the old sequences, which byte it spells, which two union-find elements a
// spelled base unites, and which pairs of the merged set are still to be aligned.  Integer arithmetic only, so the two
// executions agree exactly.
//
// Tables: steps[S] = handle (node << 1 | reverse) of every step of every path back to back, node v = 1..V at index
// v - 1; len[V]; sinc[S] = inclusive prefix sums of the step lengths, so step s spells the global base offsets
// [sinc[s - 1], sinc[s]) (the old sequences are the front of the merged set, in path order); anchor[V] = the smallest
// step index on the node.
#pragma once
#include <cstdint>
#include "sr_variants_rule.h"

#define SR_EXTEND_NO_ANCHOR 0xffffffffu        // anchor[] of a node no path visits
#define SR_EXTEND_MAX_BASES (1ULL << 39)       // one lane per base in blocks of 256: the grid stays below 2^31 blocks

SR_HD static inline uint64_t sr_ext_spos(const uint64_t *sinc, uint32_t s) { return s ? sinc[s - 1] : 0; }

// the step that spells global base offset x < sinc[S - 1]: the first s with sinc[s] > x (node lengths are >= 1)
SR_HD static inline uint32_t sr_ext_step_of(const uint64_t *sinc, uint32_t S, uint64_t x) {
    uint32_t lo = 0, hi = S - 1;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (sinc[mid] > x) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// the offset inside a node of `len` bytes that a handle of orientation o reaches at spelled offset j -- and, being its
// own inverse, the spelled offset at which it reaches node offset j
SR_HD static inline uint32_t sr_ext_flip(uint32_t o, uint32_t len, uint32_t j) { return o ? len - 1 - j : j; }

// the byte at global base offset x of the old sequences (sr_var_handle_byte: the project's complement on a reverse step)
SR_HD static inline uint8_t sr_ext_spell(const uint32_t *steps, const uint32_t *len, const uint64_t *sinc, const uint64_t *seq_off,
                                         const uint8_t *seq, uint32_t S, uint64_t x) {
    const uint32_t s = sr_ext_step_of(sinc, S, x), h = steps[s], v = (h >> 1) - 1;
    return sr_var_handle_byte(seq + seq_off[v], len[v], h & 1u, (uint32_t)(x - sr_ext_spos(sinc, s)));
}

// the union of global base offset x: false when its step is the anchor of its node (nothing to unite), else *px / *py =
// the forward-strand elements (Pos << 1) of x and of the base the anchor step spells at the same node offset.  Either
// strand serves: SeqRush::new united the two strands of every base.
SR_HD static inline bool sr_ext_seed_pair(const uint32_t *steps, const uint32_t *len, const uint64_t *sinc, const uint32_t *anchor,
                                          uint32_t S, uint64_t x, uint64_t *px, uint64_t *py) {
    const uint32_t s = sr_ext_step_of(sinc, S, x), h = steps[s], v = (h >> 1) - 1, a = anchor[v];
    if (a == s) return false;
    const uint32_t n = len[v], b = sr_ext_flip(h & 1u, n, (uint32_t)(x - sr_ext_spos(sinc, s)));
    const uint32_t ja = sr_ext_flip(steps[a] & 1u, n, b);
    *px = x << 1;
    *py = (sr_ext_spos(sinc, a) + ja) << 1;
    return true;
}

// the pair filter: a pair between two old sequences was aligned when the input graph was built
SR_HD static inline bool sr_ext_keep_pair(uint32_t q, uint32_t t, uint32_t n_old) { return !(q < n_old && t < n_old); }
