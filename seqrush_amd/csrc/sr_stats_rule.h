// sr_stats_rule.h -- the rules of the statistics stage (--stats) that the device kernels
// (sr_stats.hip) and the host twin share, like sr_iter_rule.h and sr_inv_rule.h for theirs: the layout error of one
// consecutive step pair (src/bin/measure_layout_quality.rs:133-161), the split accumulation of its square, and the node
// side an edge end touches.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SR_STATS_HD __host__ __device__
#else
#define SR_STATS_HD
#endif

#define SR_STATS_MAX_PATHS 4096            // bitset words per node <= 64, P x P matrix <= 128 MiB
#define SR_STATS_TILE 64                   // paths per similarity tile = bits of one bitset word = lanes of a wave
#define SR_STATS_CHUNK 64                  // nodes per similarity work item (one load per lane)

// e = | |pos[b] - pos[a]| - len[a] | for the step pair (a, b); pos = cumulative node length in id order
SR_STATS_HD inline uint64_t sr_stats_pair_error(uint64_t pos_a, uint64_t pos_b, uint64_t len_a) {
    const uint64_t d = pos_b > pos_a ? pos_b - pos_a : pos_a - pos_b;
    return d > len_a ? d - len_a : len_a - d;
}

// e^2 reaches 2^62, so a u64 sum of squares overflows on large unsorted graphs.  With e = a 2^16 + b (e < 2^32):
// sq[0] += a^2 (< 2^32), sq[1] += a b (< 2^32), sq[2] += b^2 (< 2^32): each sum fits a u64 for fewer than 2^31 terms,
// and sum e^2 = sq[0] 2^32 + sq[1] 2^17 + sq[2] in 128 bits on the host.
SR_STATS_HD inline void sr_stats_sq_split(uint64_t e, uint64_t *hh, uint64_t *hl, uint64_t *ll) {
    const uint64_t a = e >> 16, b = e & 0xffffu;
    *hh = a * a; *hl = a * b; *ll = b * b;
}

// node side an edge (from, to) touches, as an index 2 * node + (0 left, 1 right): the right side of a forward `from`,
// the left side of a reverse one; the left side of a forward `to`, the right side of a reverse one
SR_STATS_HD inline uint64_t sr_stats_side_from(uint32_t h) { return ((uint64_t)(h >> 1) << 1) | (1u ^ (h & 1u)); }
SR_STATS_HD inline uint64_t sr_stats_side_to(uint32_t h) { return ((uint64_t)(h >> 1) << 1) | (h & 1u); }
