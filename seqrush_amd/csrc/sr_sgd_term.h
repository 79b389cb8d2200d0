// sr_sgd_term.h -- one term of the deterministic path-guided SGD (PG-SGD), shared by the device kernel (sr_sort.hip),
// the host twin and the sequential yardstick (sr_sort.cpp).  Term selection and update follow
// src/path_sgd.rs:388-470 with three changes:
//   * every random draw is a stateless hash of (seed, iteration, term, draw#) instead of a per-thread Xoshiro stream;
//   * the Zipf jump is a binary search in a host-built prefix table of i^-theta instead of DirtyZipfian's power loop;
//   * the caller decides when an update lands (sub-round accumulation or at once), not this function.
// Only + - * /, fabs, fmin and round-to-nearest double -> int64 are used, with FP contraction off, so every execution
// computes the same bits.
#pragma once
#include <cstdint>
#include <cmath>

#pragma clang fp contract(off)

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SR_HD __host__ __device__
#else
#define SR_HD
#endif

// fixed point of the sub-round accumulators: 2^-20 bp (positions stay far below 2^43 bp)
#define SR_SGD_FIX_SHIFT 20
#define SR_SGD_FIX_SCALE 1048576.0
#define SR_SGD_DRAWS 4                               // draws per term: step, coin, direction, rank / Zipf u

struct SgdView {
    // path index: one entry per step (PathIndex::from_graph, src/path_sgd.rs:38-80)
    const uint32_t *step_node;                       // dense node index of the step's handle
    const uint32_t *step_path;
    const uint32_t *step_rank;
    const uint64_t *step_pos;                        // nucleotide offset of the step in its path
    const uint64_t *path_first;                      // first step of each path
    const uint32_t *path_nsteps;
    const double *zetas;                             // zeta table of `theta` (src/path_sgd.rs:266-283)
    const double *prefix[2];                         // prefix sums of i^-theta: [0] theta, [1] the cooling theta
    uint64_t total_steps;
    uint64_t space, space_max, space_quant;
    uint64_t min_term_updates;                       // terms per iteration
    uint64_t zeta_size;
    uint64_t seed;
};

SR_HD static inline uint64_t sgd_mix(uint64_t seed, uint64_t idx) {      // splitmix64 of state seed + (idx + 1) * golden
    uint64_t z = seed + (idx + 1) * 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

SR_HD static inline double sgd_unit(uint64_t r) { return (double)(r >> 11) * (1.0 / 9007199254740992.0); }   // [0, 1)

SR_HD static inline int64_t sgd_fix(double v) {                         // round to nearest even, like llrint
#if defined(__HIP_DEVICE_COMPILE__)
    return (int64_t)__double2ll_rn(v * SR_SGD_FIX_SCALE);
#else
    return (int64_t)llrint(v * SR_SGD_FIX_SCALE);
#endif
}

// zeta index of a jump space (src/path_sgd.rs:404-409)
SR_HD static inline uint64_t sgd_space_idx(const SgdView &v, uint64_t js) {
    uint64_t i = js > v.space_max ? v.space_max + (js - v.space_max) / v.space_quant + 1 : js;
    return i < v.zeta_size - 1 ? i : v.zeta_size - 1;
}

// DirtyZipfian::sample (src/path_sgd.rs:133-145) by table: the first i in [1, js] with prefix[i] >= u * zeta, else js
SR_HD static inline uint64_t sgd_zipf(const double *prefix, uint64_t js, double target) {
    uint64_t lo = 1, hi = js;
    if (prefix[js] < target) return js;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (prefix[mid] >= target) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// Term t of iteration k.  Returns false for a skipped draw (single-step path, rank_a == rank_b, zero distance);
// otherwise the update is x[i] -= *rx, x[j] += *rx.
SR_HD static inline bool sgd_term(const SgdView &v, uint64_t k, uint64_t t, double eta, int cooling, const double *x,
                                  uint32_t *i_out, uint32_t *j_out, double *rx_out) {
    const uint64_t base = (k * v.min_term_updates + t) * SR_SGD_DRAWS;
    const uint64_t r0 = sgd_mix(v.seed, base), r1 = sgd_mix(v.seed, base + 1);
    const uint64_t r2 = sgd_mix(v.seed, base + 2), r3 = sgd_mix(v.seed, base + 3);
    const uint64_t step = r0 % v.total_steps;
    const uint32_t path = v.step_path[step];
    const uint64_t n = v.path_nsteps[path];
    if (n == 1) return false;
    const uint64_t rank_a = v.step_rank[step];
    uint64_t rank_b = rank_a;
    if (cooling || (r1 & 1)) {
        const double *prefix = v.prefix[cooling ? 1 : 0];
        if (rank_a > 0 && ((r2 & 1) || rank_a == n - 1)) {                   // backward
            const uint64_t js = v.space < rank_a ? v.space : rank_a;
            const uint64_t z = sgd_zipf(prefix, js, sgd_unit(r3) * v.zetas[sgd_space_idx(v, js)]);
            rank_b = z < rank_a ? rank_a - z : 0;
        } else if (rank_a < n - 1) {                                         // forward
            const uint64_t js = v.space < n - rank_a - 1 ? v.space : n - rank_a - 1;
            const uint64_t z = sgd_zipf(prefix, js, sgd_unit(r3) * v.zetas[sgd_space_idx(v, js)]);
            rank_b = rank_a + z < n - 1 ? rank_a + z : n - 1;
        }
    } else {
        rank_b = r3 % n;                                                     // uniform rank
    }
    if (rank_a == rank_b) return false;
    const uint64_t first = v.path_first[path];
    const uint64_t sa = first + rank_a, sb = first + rank_b;
    const double pos_a = (double)v.step_pos[sa], pos_b = (double)v.step_pos[sb];
    const double d = fabs(pos_a - pos_b);
    if (d == 0.0) return false;
    const double w = 1.0 / d;
    const double mu = fmin(eta * w, 1.0);
    const uint32_t i = v.step_node[sa], j = v.step_node[sb];
    double dx = x[i] - x[j];
    if (dx == 0.0) dx = 1e-9;
    const double mag = fabs(dx);
    const double delta = mu * (mag - d) / 2.0;
    const double r = delta / mag;
    *i_out = i; *j_out = j; *rx_out = r * dx;
    return true;
}

// apply pass of one node: x += acc * 2^-20 / cnt (cnt > 0)
SR_HD static inline double sgd_apply(double x, int64_t acc, uint32_t cnt) {
    return x + ((double)acc / SR_SGD_FIX_SCALE) / (double)cnt;
}
