// sr_growth_rule.h -- the rules of the pangenome growth curves (--growth), shared by the kernels
// and the host twin of sr_growth.hip: the limits, the order of the groups in a sampled permutation, the r-th permutation
// in lexicographic order, and the layout of the presence bitset.  Everything here is integer arithmetic, so the two
// executions agree bit for bit.
#pragma once
#include <cstdint>
#include "../../include/seqrush_amd.h"
#include "sr_sgd_term.h"

#define SR_GROWTH_MAX_GROUPS 4096u         // G above this: SR_ERR_UNSUPPORTED (as the paths of the statistics)
#define SR_GROWTH_MAX_CELLS (1ULL << 24)   // permutations asked for x G: two u64 tables of 128 MiB each
#define SR_GROWTH_EXHAUSTIVE_MAX 8u        // G <= this and G! <= permutations asked for: all G! permutations
#define SR_GROWTH_CHUNK_WORDS 64u          // node words per chunk of the growth kernel: one per lane of a wave
#define SR_GROWTH_CHUNK_NODES (SR_GROWTH_CHUNK_WORDS * 64u)
#define SR_GROWTH_VARIANT_HOST 0           // sr_growth.variant: plain loops on the host
#define SR_GROWTH_VARIANT_WAVE 1           // lane = node word, wave = permutation

// node v = 1..V is bit (v - 1) & 63 of word (v - 1) >> 6 of its group's column
SR_HD static inline uint64_t sr_growth_words(uint64_t V) { return (V + 63) >> 6; }
// the nodes of word w that exist: all 64 bits except in the last word
SR_HD static inline uint64_t sr_growth_word_mask(uint64_t V, uint64_t w) {
    const uint64_t left = V - (w << 6);
    return left >= 64 ? ~0ULL : (1ULL << left) - 1;
}

// sampled permutation r orders the groups by (key(r, g), g) ascending
SR_HD static inline uint64_t sr_growth_key(uint64_t seed, uint64_t r, uint64_t g) { return sgd_mix(sgd_mix(seed, r), g); }
SR_HD static inline bool sr_growth_before(uint64_t ka, uint32_t a, uint64_t kb, uint32_t b) { return ka < kb || (ka == kb && a < b); }

// G! for G <= SR_GROWTH_EXHAUSTIVE_MAX
SR_HD static inline uint64_t sr_growth_factorial(uint32_t G) {
    uint64_t f = 1;
    for (uint32_t i = 2; i <= G; i++) f *= i;
    return f;
}
// the r-th permutation of 0..G-1 in lexicographic order (r < G!, G <= SR_GROWTH_EXHAUSTIVE_MAX): the digits of r in the
// factorial number system pick, from the most significant down, among the groups not yet taken in ascending order
SR_HD static inline void sr_growth_unrank(uint64_t r, uint32_t G, uint32_t *out) {
    uint64_t left = 0x76543210ULL;                    // the groups not yet taken, ascending, one per nibble (no indexed array: no scratch)
    uint64_t f = sr_growth_factorial(G);
    for (uint32_t k = 0; k < G; k++) {
        f /= G - k;                                   // (G - k - 1)!
        const uint32_t d = (uint32_t)(r / f);
        r -= d * f;
        out[k] = (uint32_t)(left >> (4 * d)) & 15u;
        left = (left & ((1ULL << (4 * d)) - 1)) | ((left >> (4 * d + 4)) << (4 * d));
    }
}
