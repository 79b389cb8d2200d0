// sr_extract_rule.h -- the rule of the subgraph extraction (--extract-*; include/seqrush_amd.h "extracting a subgraph",
// DESIGN.md section 19), shared by the kernels of sr_extract.hip and its host twin and by nothing else: when a step is
// touched by a region, when an edge hands a level on, when a gap between two kept steps closes, and where a subpath
// starts and ends.  Integers only, so both executions agree exactly.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SR_EX_HD __host__ __device__ __forceinline__
#else
#define SR_EX_HD inline
#endif

#define SR_EXTRACT_NONE 0xffffffffu                 // level: not kept
#define SR_EXTRACT_MAX_REGIONS (1ULL << 24)
#define SR_EXTRACT_MAX_CONTEXT 65535ULL
#define SR_EXTRACT_MAX_ROUNDS 64ULL

// the step [step_start, step_start + len) and the region [start, end) share a base (len >= 1, start < end)
SR_EX_HD bool sr_extract_touches(uint64_t step_start, uint32_t len, uint64_t start, uint64_t end) {
    return step_start < end && start < step_start + len;
}

// Seeds with the regions of one path sorted by start and pmax[k] = the largest end among the first k + 1 of them: with
// k = the number of regions whose start lies below the step's end, the step is touched iff one of those k ends behind
// the step's start.  A long early region that covers a step which later short ones miss is what the maximum is for.
SR_EX_HD bool sr_extract_seed(const uint64_t *reg_start, const uint64_t *reg_pmax, uint32_t r0, uint32_t r1, uint64_t step_start, uint32_t len) {
    const uint64_t step_end = step_start + len;
    uint32_t lo = r0, hi = r1;                       // the first region of [r0, r1) with start >= step_end
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (reg_start[mid] < step_end) lo = mid + 1; else hi = mid;
    }
    return lo > r0 && reg_pmax[lo - 1] > step_start;
}

// Context round r: the edge (a, b) gives node `to` the level r iff the other end has level r - 1 and `to` has none.  A
// self-loop has both ends on one level and gives nothing.
SR_EX_HD bool sr_extract_hands_on(uint32_t level_from, uint32_t level_to, uint32_t r) {
    return level_from == r - 1 && level_to == SR_EXTRACT_NONE;
}

// Merge: the run of not-kept steps between the kept steps prev and next of one path closes iff its bases are at most D.
// Its bases are what lies between the end of prev and the start of next.
SR_EX_HD bool sr_extract_gap_closes(uint64_t pstart_prev, uint32_t len_prev, uint64_t pstart_next, uint64_t D) {
    return pstart_next - pstart_prev - len_prev <= D;
}

// Subpaths: step s of the path [a0, a1) starts one iff it is kept and the step before it in the path is not, and ends one
// iff it is kept and the step behind it in the path is not.  kept: anything that answers kept[s]
template <class K> SR_EX_HD bool sr_extract_run_starts(const K &kept, uint32_t a0, uint32_t s) { return kept[s] && (s == a0 || !kept[s - 1]); }
template <class K> SR_EX_HD bool sr_extract_run_ends(const K &kept, uint32_t a1, uint32_t s) { return kept[s] && (s + 1 == a1 || !kept[s + 1]); }
