// sr_layout_term.h -- one term of the deterministic 2-D path-guided SGD layout (`--layout`), shared by
// the device kernels (sr_layout.hip), the host twin and the sequential yardstick (sr_layout.cpp).  The state is two end
// points per dense node v: end point 2v is the node's start on its forward strand, 2v + 1 its end; each is an (x, y) pair.
// A term picks step a and rank b like sgd_term (sr_sgd_term.h; restated here so that the 1-D bits cannot move), then one
// path-order end of each step: the path position of end 1 is the step's offset plus the node's length, and on a reverse
// step path-order end e is the node's end point 1 - e.  The two end points are pulled to their path distance d in the
// plane.  Only + - * /, fabs, fmin, one correctly rounded square root and round-to-nearest double -> int64 are used, with
// FP contraction off, so every execution computes the same bits.
#pragma once
#include "sr_sgd_term.h"

#pragma clang fp contract(off)

#define SR_LAYOUT_DRAWS 6                            // draws per term: step, coin, direction, rank / Zipf u, end of a, end of b
#define SR_LAYOUT_Y_SALT 0x6c61796f7574ULL           // "layout": stream of the initial y coordinates
#define SR_LAYOUT_SKIP 0xffffffffu

#if defined(__HIPCC__)
typedef double2 sr_xy;                               // one end point = one 16-byte load
#else
struct alignas(16) sr_xy { double x, y; };
#endif

struct LayoutView {
    SgdView s;                                       // path index, tables, seed, terms per iteration
    const uint8_t *step_rev;                         // 1 = the step visits its node on the reverse strand
    const uint32_t *node_len;                        // [dense node] length in bp
};

// per node: the sub-round's sums of both end points in one 64-byte record (a term touches at most two of them)
struct alignas(64) LayoutAcc {
    unsigned long long a[4];                         // ax0 ay0 ax1 ay1: int64 two's complement, units of 2^-20 bp
    unsigned c[2];                                   // contributions per end point
    unsigned pad[6];
};

SR_HD static inline double layout_sqrt(double v) {   // correctly rounded on both sides
#if defined(__HIP_DEVICE_COMPILE__)
    return __dsqrt_rn(v);
#else
    return sqrt(v);
#endif
}

// Selection of term t of iteration k: end points *i_out, *j_out (2 * dense node + end) and their path distance *d_out.
// Returns false for a skipped draw: single-step path, the same end of the same step, zero distance.
SR_HD static inline bool layout_select(const LayoutView &lv, uint64_t k, uint64_t t, int cooling, uint32_t *i_out, uint32_t *j_out,
                                       double *d_out) {
    const SgdView &v = lv.s;
    const uint64_t base = (k * v.min_term_updates + t) * SR_LAYOUT_DRAWS;
    const uint64_t r0 = sgd_mix(v.seed, base), r1 = sgd_mix(v.seed, base + 1);
    const uint64_t r2 = sgd_mix(v.seed, base + 2), r3 = sgd_mix(v.seed, base + 3);
    const uint64_t r4 = sgd_mix(v.seed, base + 4), r5 = sgd_mix(v.seed, base + 5);
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
    const uint32_t ea = (uint32_t)(r4 & 1), eb = (uint32_t)(r5 & 1);
    if (rank_a == rank_b && ea == eb) return false;                          // the other end of the same step holds a node to its length
    const uint64_t first = v.path_first[path];
    const uint64_t sa = first + rank_a, sb = first + rank_b;
    const uint32_t na = v.step_node[sa], nb = v.step_node[sb];
    const double pos_a = (double)(v.step_pos[sa] + (ea ? lv.node_len[na] : 0u));
    const double pos_b = (double)(v.step_pos[sb] + (eb ? lv.node_len[nb] : 0u));
    const double d = fabs(pos_a - pos_b);
    if (d == 0.0) return false;
    *i_out = 2u * na + (lv.step_rev[sa] ? 1u - ea : ea);
    *j_out = 2u * nb + (lv.step_rev[sb] ? 1u - eb : eb);
    *d_out = d;
    return true;
}

// The update of end points pi, pj at path distance d: pi moves by (-*rx, -*ry), pj by (+*rx, +*ry).
SR_HD static inline void layout_update(double eta, double d, sr_xy pi, sr_xy pj, double *rx_out, double *ry_out) {
    const double mu = fmin(eta / d, 1.0);
    double dx = pi.x - pj.x;
    if (dx == 0.0) dx = 1e-9;
    const double dy = pi.y - pj.y;
    const double mag = layout_sqrt(dx * dx + dy * dy);
    const double r = mu * (mag - d) / 2.0 / mag;
    *rx_out = r * dx;
    *ry_out = r * dy;
}

// Term t of iteration k on the state xy.  Returns false for a skipped draw.
SR_HD static inline bool layout_term(const LayoutView &lv, uint64_t k, uint64_t t, double eta, int cooling, const sr_xy *xy,
                                     uint32_t *i_out, uint32_t *j_out, double *rx_out, double *ry_out) {
    double d;
    if (!layout_select(lv, k, t, cooling, i_out, j_out, &d)) return false;
    layout_update(eta, d, xy[*i_out], xy[*j_out], rx_out, ry_out);
    return true;
}
