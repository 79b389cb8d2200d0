// sr_layout.cpp -- the 2-D path-guided SGD layout on the host (`--layout`; include/seqrush_amd.h "2-D layout", DESIGN.md
// section 12): parameters, schedule and initial state on top of sgd_prepare's path index and tables (sr_sort.cpp); the host
// twin of the device SGD and the sequential yardstick (per-term math: sr_layout_term.h); the TSV and SVG writers and the
// quality measure, formed here so that every front end writes the same bytes.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/seqrush_amd.h"
#include "sr_layout.h"
#include "sr_stage_host.h"

#pragma clang fp contract(off)

// Default terms per sub-round: the largest power of two up to an eighth of the end points, within [64, 65 536].  An end point
// moves by the average of its sub-round's contributions, so every further contribution to the same end point in one sub-round
// is a step not taken: the host twin's stress stays within the margin of the yardstick's only while a sub-round holds fewer
// terms than end points (measurements: DESIGN.md section 12).
static uint64_t default_terms_per_round(uint64_t n_nodes) {
    uint64_t r = 64;
    while (r < 65536 && r * 2 <= n_nodes / 4) r *= 2;
    return r;
}
static const uint64_t QUALITY_SALT = 0x7175616c697479ULL;   // "quality": the stream of sr_layout_quality's draws

static const uint32_t N_STATS = 7;
static thread_local double g_stats[N_STATS];
extern "C" int sr_layout_stats(double *out, uint32_t cap) {
    if (!out) return sr_fail(SR_ERR_INVALID, "null argument");
    const uint32_t n = cap < N_STATS ? cap : N_STATS;
    for (uint32_t i = 0; i < n; i++) out[i] = g_stats[i];
    return (int)n;
}

static double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

extern "C" void sr_layout_params_default(sr_layout_params *p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->seed = 9399220;
    p->iter_max = 30;
    p->theta = 0.99;
    p->eps = 0.01;
    p->cooling_start = 0.5;
    p->space_max = 100;
    p->space_quant = 100;
    p->device = 0;
}

// ------------------------------------------------------------------ parameters, schedule, initial state
int layout_prepare(const SrGraph &g, const sr_layout_params &prm, LayoutProblem &p) {
    sr_layout_params d;
    sr_layout_params_default(&d);
    uint64_t alive = 0;
    for (size_t id = 0; id < g.node_seq.size(); id++) alive += g.node_alive[id] ? 1 : 0;
    const uint64_t S = g.steps.size();
    if (alive > (1ULL << 30) || S > (1ULL << 31))
        return sr_fail(SR_ERR_UNSUPPORTED, "layout: more than 2^30 nodes or 2^31 path steps");
    uint64_t max_len = 0;                            // longest path in bp
    for (size_t q = 0; q + 1 < g.path_off.size(); q++) {
        uint64_t len = 0;
        for (uint64_t i = g.path_off[q]; i < g.path_off[q + 1]; i++) {
            const uint32_t id = g.steps[i] >> 1;
            if (id >= g.node_seq.size() || !g.node_alive[id]) return sr_fail(SR_ERR_INVALID, "layout: a path step names a missing node");
            len += g.node_seq[id].size();
        }
        max_len = std::max(max_len, len);
    }
    sr_sort_params sp;
    sr_sort_params_default(&sp);
    sp.seed = prm.seed;
    sp.iter_max = prm.iter_max ? prm.iter_max : d.iter_max;
    sp.theta = prm.theta != 0.0 ? prm.theta : d.theta;
    sp.eps = prm.eps != 0.0 ? prm.eps : d.eps;
    sp.eta_max = prm.eta_max != 0.0 ? prm.eta_max : (double)max_len * (double)max_len;
    sp.cooling_start = prm.cooling_start != 0.0 ? prm.cooling_start : d.cooling_start;
    sp.space = prm.space;
    sp.space_max = prm.space_max ? prm.space_max : d.space_max;
    sp.space_quant = prm.space_quant ? prm.space_quant : d.space_quant;
    sp.min_term_updates = prm.min_term_updates ? prm.min_term_updates : 10 * S;
    sp.terms_per_round = prm.terms_per_round ? prm.terms_per_round : default_terms_per_round(alive);
    if (!(sp.eps > 0) || !(sp.theta > 0) || sp.eta_max < 0) return sr_fail(SR_ERR_INVALID, "layout: theta and eps must be > 0, eta_max >= 0");
    int r = sgd_prepare(g, sp, p.sgd);
    if (r) return r;
    const uint64_t N = p.sgd.n_nodes;
    p.step_rev.resize(S);
    for (uint64_t i = 0; i < S; i++) p.step_rev[i] = (uint8_t)(g.steps[i] & 1u);
    p.node_len.resize(N);
    p.xy0.resize(2 * N);
    for (uint64_t v = 0; v < N; v++) {
        const uint64_t len = g.node_seq[p.sgd.node_id[v]].size();
        if (len > 0xffffffffULL) return sr_fail(SR_ERR_UNSUPPORTED, "layout: a node is longer than 2^32 bp");
        p.node_len[v] = (uint32_t)len;
        for (uint64_t e = 0; e < 2; e++) {
            sr_xy &q = p.xy0[2 * v + e];
            q.x = p.sgd.x0[v] + (e ? (double)len : 0.0);
            q.y = (sgd_unit(sgd_mix(p.sgd.seed ^ SR_LAYOUT_Y_SALT, 2 * v + e)) - 0.5) * (double)len;
        }
    }
    p.view.s = p.sgd.view;
    p.view.step_rev = p.step_rev.data();
    p.view.node_len = p.node_len.data();
    return SR_OK;
}

// ------------------------------------------------------------------ host twin and sequential yardstick
void layout_run_host_twin(const LayoutProblem &p, std::vector<sr_xy> &xy) {
    xy = p.xy0;
    if (!p.sgd.has_terms) return;
    const uint64_t N = p.sgd.n_nodes, M = p.sgd.min_term_updates, R = p.sgd.terms_per_round;
    std::vector<LayoutAcc> acc(N);                   // zeroed; int64 two's complement, wrapping like the device's atomics
    for (uint64_t k = 0; k < p.sgd.iters; k++) {
        const double eta = p.sgd.etas[k];
        const int cooling = k > p.sgd.first_cooling;
        for (uint64_t t0 = 0; t0 < M; t0 += R) {
            const uint64_t t1 = std::min(M, t0 + R);
            for (uint64_t t = t0; t < t1; t++) {
                uint32_t i, j;
                double rx, ry;
                if (!layout_term(p.view, k, t, eta, cooling, xy.data(), &i, &j, &rx, &ry)) continue;
                LayoutAcc &ai = acc[i >> 1], &aj = acc[j >> 1];
                ai.a[(i & 1) * 2] += (uint64_t)sgd_fix(-rx); ai.a[(i & 1) * 2 + 1] += (uint64_t)sgd_fix(-ry); ai.c[i & 1]++;
                aj.a[(j & 1) * 2] += (uint64_t)sgd_fix(rx); aj.a[(j & 1) * 2 + 1] += (uint64_t)sgd_fix(ry); aj.c[j & 1]++;
            }
            for (uint64_t e = 0; e < 2 * N; e++) {
                LayoutAcc &a = acc[e >> 1];
                const unsigned c = a.c[e & 1];
                if (!c) continue;
                xy[e].x = sgd_apply(xy[e].x, (int64_t)a.a[(e & 1) * 2], c);
                xy[e].y = sgd_apply(xy[e].y, (int64_t)a.a[(e & 1) * 2 + 1], c);
                a.a[(e & 1) * 2] = 0; a.a[(e & 1) * 2 + 1] = 0; a.c[e & 1] = 0;
            }
        }
    }
}

void layout_run_sequential(const LayoutProblem &p, std::vector<sr_xy> &xy) {
    xy = p.xy0;
    if (!p.sgd.has_terms) return;
    for (uint64_t k = 0; k < p.sgd.iters; k++) {
        const double eta = p.sgd.etas[k];
        const int cooling = k > p.sgd.first_cooling;
        for (uint64_t t = 0; t < p.sgd.min_term_updates; t++) {
            uint32_t i, j;
            double rx, ry;
            if (!layout_term(p.view, k, t, eta, cooling, xy.data(), &i, &j, &rx, &ry)) continue;
            xy[i].x -= rx; xy[i].y -= ry;
            xy[j].x += rx; xy[j].y += ry;
        }
    }
}

// ------------------------------------------------------------------ C ABI
static sr_layout_params given_or_default(const sr_layout_params *p) {
    sr_layout_params q;
    if (p) q = *p; else sr_layout_params_default(&q);
    return q;
}

static int parse_and_prepare(const char *gfa_in, const sr_layout_params &prm, SrGraph &g, LayoutProblem &lp) {
    std::vector<std::string> names;
    int r = sr_graph_parse_gfa(gfa_in, g, names);
    if (r) return r;
    return layout_prepare(g, prm, lp);
}

extern "C" int sr_layout_gfa(const char *gfa_in, const sr_layout_params *p, double *xy_out, uint64_t n_nodes) {
    if (!gfa_in || (!xy_out && n_nodes)) return sr_fail(SR_ERR_INVALID, "null argument");
    const auto t_all = std::chrono::steady_clock::now();
    const sr_layout_params prm = given_or_default(p);
    if (prm.device < SR_LAYOUT_DEVICE_SEQUENTIAL)
        return sr_fail(SR_ERR_INVALID, "layout: device must be >= 0, -1 (host twin) or -2 (sequential)");
    SrGraph g;
    LayoutProblem lp;
    int r = parse_and_prepare(gfa_in, prm, g, lp);
    if (r) return r;
    const uint64_t N = lp.sgd.n_nodes;
    if (n_nodes != N) return sr_fail(SR_ERR_INVALID, "sr_layout_gfa: n_nodes must be the number of nodes (" + std::to_string(N) + ")");
    for (double &s : g_stats) s = 0;
    std::vector<sr_xy> xy = lp.xy0;
    if (lp.sgd.has_terms) {
        const auto t0 = std::chrono::steady_clock::now();
        if (prm.device >= 0) {
            float ms = 0;
            if ((r = srk_layout_device(lp, prm.device, nullptr, xy, &ms))) return r;
            g_stats[0] = ms;
        } else {
            if (prm.device == SR_LAYOUT_DEVICE_HOST_TWIN) layout_run_host_twin(lp, xy);
            else layout_run_sequential(lp, xy);
            g_stats[0] = ms_since(t0);
        }
    }
    for (uint64_t e = 0; e < 2 * N; e++) { xy_out[2 * e] = xy[e].x; xy_out[2 * e + 1] = xy[e].y; }
    g_stats[1] = (double)lp.sgd.min_term_updates; g_stats[2] = (double)lp.sgd.iters;
    g_stats[3] = (double)((lp.sgd.min_term_updates + lp.sgd.terms_per_round - 1) / lp.sgd.terms_per_round);
    g_stats[4] = (double)N; g_stats[5] = (double)g.steps.size();
    g_stats[6] = ms_since(t_all);
    return SR_OK;
}

extern "C" int sr_layout_resolve(const char *gfa_in, const sr_layout_params *p, sr_layout_params *resolved) {
    if (!gfa_in || !resolved) return sr_fail(SR_ERR_INVALID, "null argument");
    const sr_layout_params prm = given_or_default(p);
    SrGraph g;
    LayoutProblem lp;
    int r = parse_and_prepare(gfa_in, prm, g, lp);
    if (r) return r;
    const SgdProblem &s = lp.sgd;
    *resolved = prm;
    resolved->iter_max = s.iter_max; resolved->theta = s.theta; resolved->eps = s.eps; resolved->eta_max = s.eta_max;
    resolved->cooling_start = s.cooling_start; resolved->space = s.space; resolved->space_max = s.space_max;
    resolved->space_quant = s.space_quant; resolved->min_term_updates = s.min_term_updates; resolved->terms_per_round = s.terms_per_round;
    return SR_OK;
}

extern "C" int sr_layout_select_host(const char *gfa_in, const sr_layout_params *p, uint64_t k, uint64_t t0, uint64_t count, int cooling,
                                     uint32_t *i_out, uint32_t *j_out, double *d_out) {
    if (!gfa_in || !i_out || !j_out || !d_out) return sr_fail(SR_ERR_INVALID, "null argument");
    const sr_layout_params prm = given_or_default(p);
    SrGraph g;
    LayoutProblem lp;
    int r = parse_and_prepare(gfa_in, prm, g, lp);
    if (r) return r;
    for (uint64_t t = 0; t < count; t++) {
        i_out[t] = j_out[t] = SR_LAYOUT_SKIP; d_out[t] = 0.0;
        if (g.steps.empty()) continue;
        uint32_t i, j;
        double d;
        if (layout_select(lp.view, k, t0 + t, cooling != 0, &i, &j, &d)) { i_out[t] = i; j_out[t] = j; d_out[t] = d; }
    }
    return SR_OK;
}

// ------------------------------------------------------------------ outputs
static void appendf(std::string &s, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
static void appendf(std::string &s, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    const int n = vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (n > 0) s.append(buf, std::min((size_t)n, sizeof(buf) - 1));
}

extern "C" int sr_layout_tsv(const double *xy, uint64_t n, char **text) {
    if ((!xy && n) || !text) return sr_fail(SR_ERR_INVALID, "null argument");
    std::string s = "idx\tX\tY\n";
    s.reserve(16 + n * 64);
    for (uint64_t e = 0; e < 2 * n; e++) appendf(s, "%llu\t%.4f\t%.4f\n", (unsigned long long)e, xy[2 * e], xy[2 * e + 1]);
    return sr_give_text(s, text, "out of memory");
}

extern "C" int sr_layout_svg(const char *gfa_in, const double *xy, uint64_t n, char **text) {
    if (!gfa_in || (!xy && n) || !text) return sr_fail(SR_ERR_INVALID, "null argument");
    SrGraph g;
    std::vector<std::string> names;
    int r = sr_graph_parse_gfa(gfa_in, g, names);
    if (r) return r;
    const uint64_t N = g.node_seq.size() - 1;        // the parser maps the S ids to 1..N in ascending order
    if (n != N) return sr_fail(SR_ERR_INVALID, "sr_layout_svg: n must be the number of nodes (" + std::to_string(N) + ")");
    double x0 = 0, y0 = 0, x1 = 0, y1 = 0;
    for (uint64_t e = 0; e < 2 * n; e++) {
        const double x = xy[2 * e], y = xy[2 * e + 1];
        if (!std::isfinite(x) || !std::isfinite(y)) return sr_fail(SR_ERR_INVALID, "sr_layout_svg: a coordinate is not finite");
        if (e == 0) { x0 = x1 = x; y0 = y1 = y; }
        x0 = std::min(x0, x); x1 = std::max(x1, x); y0 = std::min(y0, y); y1 = std::max(y1, y);
    }
    const double span = std::max(std::max(x1 - x0, y1 - y0), 1.0);
    const double mx = 0.02 * (x1 - x0), my = 0.02 * (y1 - y0);       // 2 % of the bounding box, shared between the two sides
    const double wn = span / 400.0, wl = span / 1600.0;              // stroke widths: nodes, links
    std::string s;
    s.reserve(256 + (n + g.edges.size()) * 96);
    appendf(s, "<svg xmlns=\"http://www.w3.org/2000/svg\" viewBox=\"%.4f %.4f %.4f %.4f\">\n", x0 - mx / 2, y0 - my / 2, (x1 - x0) + mx,
            (y1 - y0) + my);
    appendf(s, "<g stroke=\"black\" stroke-width=\"%.4f\">\n", wn);
    for (uint64_t v = 0; v < n; v++)
        appendf(s, "<line x1=\"%.4f\" y1=\"%.4f\" x2=\"%.4f\" y2=\"%.4f\"/>\n", xy[4 * v], xy[4 * v + 1], xy[4 * v + 2], xy[4 * v + 3]);
    appendf(s, "</g>\n<g stroke=\"black\" stroke-width=\"%.4f\">\n", wl);
    for (const auto &e : g.edges) {
        const uint64_t a = 2 * (uint64_t)((e.first >> 1) - 1) + ((e.first & 1) ? 0 : 1);      // out-end of the from-handle
        const uint64_t b = 2 * (uint64_t)((e.second >> 1) - 1) + ((e.second & 1) ? 1 : 0);    // in-end of the to-handle
        appendf(s, "<line x1=\"%.4f\" y1=\"%.4f\" x2=\"%.4f\" y2=\"%.4f\"/>\n", xy[2 * a], xy[2 * a + 1], xy[2 * b], xy[2 * b + 1]);
    }
    s += "</g>\n</svg>\n";
    return sr_give_text(s, text, "out of memory");
}

extern "C" int sr_layout_quality(const char *gfa_in, const double *xy, uint64_t n, uint64_t seed, uint64_t samples, double out[4]) {
    if (!gfa_in || (!xy && n) || !out) return sr_fail(SR_ERR_INVALID, "null argument");
    sr_layout_params prm;
    sr_layout_params_default(&prm);
    prm.seed = seed ^ QUALITY_SALT;
    SrGraph g;
    LayoutProblem lp;
    int r = parse_and_prepare(gfa_in, prm, g, lp);
    if (r) return r;
    const uint64_t N = lp.sgd.n_nodes;
    if (n != N) return sr_fail(SR_ERR_INVALID, "sr_layout_quality: n must be the number of nodes (" + std::to_string(N) + ")");
    double stress = 0.0, pairs = 0.0;
    if (!g.steps.empty())
        for (uint64_t t = 0; t < samples; t++) {
            uint32_t i, j;
            double d;
            if (!layout_select(lp.view, 0, t, 0, &i, &j, &d)) continue;
            const double dx = xy[2 * (uint64_t)i] - xy[2 * (uint64_t)j], dy = xy[2 * (uint64_t)i + 1] - xy[2 * (uint64_t)j + 1];
            const double e = (sqrt(dx * dx + dy * dy) - d) / d;
            stress += e * e;
            pairs += 1.0;
        }
    double len_err = 0.0;
    for (uint64_t v = 0; v < N; v++) {
        const double dx = xy[4 * v + 2] - xy[4 * v], dy = xy[4 * v + 3] - xy[4 * v + 1];
        len_err += fabs(sqrt(dx * dx + dy * dy) - (double)lp.node_len[v]);
    }
    out[0] = pairs > 0 ? stress / pairs : 0.0;
    out[1] = N ? len_err / (double)N : 0.0;
    out[2] = pairs;
    out[3] = 0.0;
    return SR_OK;
}
