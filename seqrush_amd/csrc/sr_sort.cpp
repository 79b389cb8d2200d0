// sr_sort.cpp -- the Ygs layout on the host (src/ygs_sort.rs:96-162; include/seqrush_amd.h "Ygs layout"):
//   path index, parameters and tables of the path-guided SGD (src/path_sgd.rs:38-80, 252-283, 552-575,
//   YgsParams::from_graph src/ygs_sort.rs:50-95); the host twin of the device SGD and the sequential yardstick
//   (per-term math: sr_sgd_term.h); apply_ordering (src/bidirected_ops.rs:1609-...); the BFS groom
//   (src/groom.rs:49-200, 253-300, 613-...) seeded by find_head_nodes (src/bidirected_ops.rs:1317-1345); the
//   head-seeded topological sort exact_odgi_topological_order(true, false) (src/bidirected_ops.rs:1390-1599).
// Neighbours are visited in ascending handle order everywhere the reference iterates a set.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>
#include "../../include/seqrush_amd.h"
#include "sr_sort.h"

#pragma clang fp contract(off)

typedef uint32_t hnd;                                // Handle: node_id << 1 | is_reverse
static inline uint32_t hid(hnd h) { return h >> 1; }
static const double COOLING_THETA = 0.001;           // src/path_sgd.rs:347
static const uint64_t TERMS_PER_ROUND_DEFAULT = 65536;     // 256 workgroups of 256 lanes: one per CU

static const uint32_t N_STATS = 10;
static thread_local double g_stats[N_STATS];
void sr_sort_note_write_ms(double ms) { g_stats[3] = ms; g_stats[9] += ms; }
extern "C" int sr_sort_stats(double *out, uint32_t cap) {
    if (!out) return sr_fail(SR_ERR_INVALID, "null argument");
    const uint32_t n = cap < N_STATS ? cap : N_STATS;
    for (uint32_t i = 0; i < n; i++) out[i] = g_stats[i];
    return (int)n;
}

static double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

extern "C" void sr_sort_params_default(sr_sort_params *p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->seed = 9399220;                               // the reference's first worker seed (src/path_sgd.rs:376)
    p->iter_max = 100;
    p->theta = 0.99;
    p->eps = 0.01;
    p->eta_max = 0.0;
    p->cooling_start = 0.5;
    p->space = 0;
    p->space_max = 100;
    p->space_quant = 100;
    p->min_term_updates = 0;
    p->terms_per_round = 0;
    p->device = 0;
}

static uint64_t graph_node_len(const SrGraph &g, hnd h) { return g.node_seq[hid(h)].size(); }

// ------------------------------------------------------------------ SGD: path index, parameters, tables
int sgd_prepare(const SrGraph &g, const sr_sort_params &prm, SgdProblem &p) {
    if (prm.iter_max < 2) return sr_fail(SR_ERR_INVALID, "sort: iter_max must be >= 2 (the schedule divides by iter_max - 1)");
    if (prm.space_quant == 0) return sr_fail(SR_ERR_INVALID, "sort: space_quant must be > 0");
    const size_t NN = g.node_seq.size();
    std::vector<uint32_t> dense(NN, 0xffffffffu);
    p.node_id.clear(); p.x0.clear();
    uint64_t len = 0;                                // positions seeded with the layout in id order (:200-217)
    for (size_t id = 0; id < NN; id++) {
        if (!g.node_alive[id]) continue;
        dense[id] = (uint32_t)p.node_id.size();
        p.node_id.push_back((uint32_t)id);
        p.x0.push_back((double)len);
        len += g.node_seq[id].size();
    }
    p.n_nodes = p.node_id.size();
    const size_t npaths = g.path_off.size() - 1, S = g.steps.size();
    p.step_node.resize(S); p.step_path.resize(S); p.step_rank.resize(S); p.step_pos.resize(S);
    p.path_first.resize(npaths); p.path_nsteps.resize(npaths);
    uint64_t sum_steps = 0, max_steps = 0, max_len = 0;
    p.has_terms = false;
    for (size_t q = 0; q < npaths; q++) {
        uint64_t pos = 0;
        const uint64_t b = g.path_off[q], e = g.path_off[q + 1];
        if (e - b > 0xffffffffULL) return sr_fail(SR_ERR_UNSUPPORTED, "sort: a path has more than 2^32 steps");
        p.path_first[q] = b; p.path_nsteps[q] = (uint32_t)(e - b);
        for (uint64_t i = b; i < e; i++) {
            const hnd h = g.steps[i];
            if (hid(h) >= NN || !g.node_alive[hid(h)]) return sr_fail(SR_ERR_INVALID, "sort: a path step names a missing node");
            p.step_node[i] = dense[hid(h)]; p.step_path[i] = (uint32_t)q; p.step_rank[i] = (uint32_t)(i - b); p.step_pos[i] = pos;
            pos += graph_node_len(g, h);
        }
        sum_steps += e - b;
        max_steps = std::max(max_steps, e - b);
        max_len = std::max(max_len, pos);
        if (e - b > 1) p.has_terms = true;
    }
    p.seed = prm.seed; p.iter_max = prm.iter_max; p.theta = prm.theta; p.eps = prm.eps; p.cooling_start = prm.cooling_start;
    p.space_max = prm.space_max; p.space_quant = prm.space_quant;
    p.min_term_updates = prm.min_term_updates ? prm.min_term_updates : sum_steps;
    p.eta_max = prm.eta_max > 0 ? prm.eta_max : (double)(max_steps * max_steps);
    p.space = prm.space ? prm.space : max_len;
    if (p.space == 0) p.space = 1;
    if (p.has_terms && !(p.eta_max > 0)) return sr_fail(SR_ERR_INVALID, "sort: eta_max must be > 0");
    // learning-rate schedule, path_linear_sgd_schedule (src/path_sgd.rs:552-575) with iter_with_max_learning_rate = 0
    {
        const double w_min = 1.0 / p.eta_max, w_max = 1.0;
        const double eta_max = 1.0 / w_min, eta_min = p.eps / w_max;
        const double lambda = std::log(eta_max / eta_min) / ((double)p.iter_max - 1.0);
        p.etas.resize(p.iter_max + 1);
        for (uint64_t t = 0; t <= p.iter_max; t++) p.etas[t] = eta_max * std::exp(-lambda * (double)t);
    }
    p.iters = p.iter_max + 1;
    p.first_cooling = (uint64_t)std::floor(p.cooling_start * (double)p.iter_max);
    // zeta table (src/path_sgd.rs:266-283) and one prefix table per theta (entry i: sum_{k <= i} (1/k)^theta)
    {
        const uint64_t zs = (p.space <= p.space_max ? p.space : p.space_max + (p.space - p.space_max) / p.space_quant + 1) + 1;
        p.zetas.assign(zs, 0.0);
        p.prefix_theta.assign(p.space + 1, 0.0);
        p.prefix_cool.assign(p.space + 1, 0.0);
        double z = 0.0, zc = 0.0;
        for (uint64_t i = 1; i <= p.space; i++) {
            z += std::pow(1.0 / (double)i, p.theta);
            zc += std::pow(1.0 / (double)i, COOLING_THETA);
            p.prefix_theta[i] = z; p.prefix_cool[i] = zc;
            if (i <= p.space_max) p.zetas[i] = z;
            if (i >= p.space_max && (i - p.space_max) % p.space_quant == 0) {
                const uint64_t idx = p.space_max + 1 + (i - p.space_max) / p.space_quant;
                if (idx < zs) p.zetas[idx] = z;
            }
        }
    }
    p.terms_per_round = prm.terms_per_round ? prm.terms_per_round : TERMS_PER_ROUND_DEFAULT;
    SgdView &v = p.view;
    v.step_node = p.step_node.data(); v.step_path = p.step_path.data(); v.step_rank = p.step_rank.data();
    v.step_pos = p.step_pos.data(); v.path_first = p.path_first.data(); v.path_nsteps = p.path_nsteps.data();
    v.zetas = p.zetas.data(); v.prefix[0] = p.prefix_theta.data(); v.prefix[1] = p.prefix_cool.data();
    v.total_steps = S; v.space = p.space; v.space_max = p.space_max; v.space_quant = p.space_quant;
    v.min_term_updates = p.min_term_updates; v.zeta_size = p.zetas.size(); v.seed = p.seed;
    return SR_OK;
}

// ------------------------------------------------------------------ SGD: host twin and sequential yardstick
void sgd_run_host_twin(const SgdProblem &p, std::vector<double> &x) {
    x = p.x0;
    if (!p.has_terms) return;
    const uint64_t N = p.n_nodes, M = p.min_term_updates, R = p.terms_per_round;
    std::vector<uint64_t> acc(N, 0);                 // int64 two's complement, wrapping like the device's atomics
    std::vector<uint32_t> cnt(N, 0);
    for (uint64_t k = 0; k < p.iters; k++) {
        const double eta = p.etas[k];
        const int cooling = k > p.first_cooling;
        for (uint64_t t0 = 0; t0 < M; t0 += R) {
            const uint64_t t1 = std::min(M, t0 + R);
            for (uint64_t t = t0; t < t1; t++) {
                uint32_t i, j;
                double rx;
                if (!sgd_term(p.view, k, t, eta, cooling, x.data(), &i, &j, &rx)) continue;
                acc[i] += (uint64_t)sgd_fix(-rx); cnt[i]++;
                acc[j] += (uint64_t)sgd_fix(rx); cnt[j]++;
            }
            for (uint64_t n = 0; n < N; n++) {
                if (!cnt[n]) continue;
                x[n] = sgd_apply(x[n], (int64_t)acc[n], cnt[n]);
                acc[n] = 0; cnt[n] = 0;
            }
        }
    }
}

void sgd_run_sequential(const SgdProblem &p, std::vector<double> &x) {
    x = p.x0;
    if (!p.has_terms) return;
    for (uint64_t k = 0; k < p.iters; k++) {
        const double eta = p.etas[k];
        const int cooling = k > p.first_cooling;
        for (uint64_t t = 0; t < p.min_term_updates; t++) {
            uint32_t i, j;
            double rx;
            if (!sgd_term(p.view, k, t, eta, cooling, x.data(), &i, &j, &rx)) continue;
            const double xi = x[i], xj = x[j];       // src/path_sgd.rs:455-460
            x[i] = xi - rx;
            x[j] = xj + rx;
        }
    }
}

static int sgd_positions(const SgdProblem &p, const sr_sort_params &prm, void *stream, std::vector<double> &x, double *ms) {
    const auto t0 = std::chrono::steady_clock::now();
    if (prm.device >= 0) {
        float dms = 0;
        int r = srk_sgd_device(p, prm.device, stream, x, &dms);
        if (r) return r;
        *ms = dms;
        return SR_OK;
    }
    if (prm.device == SR_SORT_DEVICE_HOST_TWIN) sgd_run_host_twin(p, x);
    else if (prm.device == SR_SORT_DEVICE_SEQUENTIAL) sgd_run_sequential(p, x);
    else return sr_fail(SR_ERR_INVALID, "sort: device must be >= 0, -1 (host twin) or -2 (sequential)");
    *ms = ms_since(t0);
    return SR_OK;
}

// ------------------------------------------------------------------ graph rewrites
// apply_ordering (src/bidirected_ops.rs:1609-...): order[r] (an old node id) becomes id r + 1
static void apply_ordering(SrGraph &g, const std::vector<uint32_t> &order) {
    const size_t NN = g.node_seq.size();
    std::vector<uint32_t> map(NN, 0);
    for (size_t r = 0; r < order.size(); r++) map[order[r]] = (uint32_t)(r + 1);
    std::vector<std::string> ns(order.size() + 1);
    std::vector<uint8_t> na(order.size() + 1, 1);
    na[0] = 0;
    for (size_t r = 0; r < order.size(); r++) ns[r + 1] = std::move(g.node_seq[order[r]]);
    g.node_seq.swap(ns); g.node_alive.swap(na);
    for (auto &e : g.edges) { e.first = (map[hid(e.first)] << 1) | (e.first & 1u); e.second = (map[hid(e.second)] << 1) | (e.second & 1u); }
    for (auto &h : g.steps) h = (map[hid(h)] << 1) | (h & 1u);
}

static std::vector<uint32_t> alive_ids(const SrGraph &g) {
    std::vector<uint32_t> ids;
    for (size_t id = 0; id < g.node_seq.size(); id++) if (g.node_alive[id]) ids.push_back((uint32_t)id);
    return ids;
}

// find_head_nodes (src/bidirected_ops.rs:1317-1345): nodes no stored edge enters (either orientation), forward, ordered by
// (earliest rank in any path, id)
static std::vector<hnd> find_heads(const SrGraph &g) {
    const size_t NN = g.node_seq.size();
    std::vector<uint8_t> has_in(NN, 0);
    for (const auto &e : g.edges) has_in[hid(e.second)] = 1;
    std::vector<uint64_t> first(NN, UINT64_MAX);
    for (size_t q = 0; q + 1 < g.path_off.size(); q++)
        for (uint64_t i = g.path_off[q]; i < g.path_off[q + 1]; i++) {
            const uint32_t id = hid(g.steps[i]);
            first[id] = std::min(first[id], i - g.path_off[q]);
        }
    std::vector<uint32_t> ids;
    for (size_t id = 0; id < NN; id++) if (g.node_alive[id] && !has_in[id]) ids.push_back((uint32_t)id);
    std::stable_sort(ids.begin(), ids.end(), [&](uint32_t a, uint32_t b) { return first[a] < first[b]; });
    std::vector<hnd> heads;
    for (uint32_t id : ids) heads.push_back(id << 1);
    return heads;
}

// per handle: the `to` of every stored edge leaving it, ascending
static void out_adjacency(const SrGraph &g, std::vector<uint64_t> &off, std::vector<hnd> &to) {
    const size_t NH = g.node_seq.size() * 2;
    off.assign(NH + 1, 0);
    for (const auto &e : g.edges) off[e.first + 1]++;
    for (size_t h = 0; h < NH; h++) off[h + 1] += off[h];
    to.resize(g.edges.size());
    std::vector<uint64_t> fill(off.begin(), off.end() - 1);
    for (const auto &e : g.edges) to[fill[e.first]++] = e.second;
    for (size_t h = 0; h < NH; h++) std::sort(to.begin() + off[h], to.begin() + off[h + 1]);
}

static inline uint8_t rc_base(uint8_t b) {           // src/bidirected_graph.rs:73-85
    switch (b) {
    case 'A': case 'a': return 'T'; case 'T': case 't': return 'A';
    case 'C': case 'c': return 'G'; case 'G': case 'g': return 'C';
    case 'N': case 'n': return 'N';
    default: return b;
    }
}

// groom(use_bfs = true) + apply_grooming_with_reorder(reorder = false) (src/groom.rs:49-200, 253-300, 613-...)
static void groom(SrGraph &g) {
    const size_t NN = g.node_seq.size();
    std::vector<uint64_t> off;
    std::vector<hnd> to;
    out_adjacency(g, off, to);
    std::vector<uint8_t> visited(NN, 0), flipped(NN, 0);
    std::vector<hnd> seeds = find_heads(g);
    if (seeds.empty())
        for (size_t id = 0; id < NN; id++) if (g.node_alive[id]) { seeds.push_back((hnd)(id << 1)); break; }
    std::vector<hnd> queue;
    size_t scan = 0;                                  // next component: first unvisited node in id order
    for (;;) {
        if (seeds.empty()) {
            while (scan < NN && (!g.node_alive[scan] || visited[scan])) scan++;
            if (scan == NN) break;
            seeds.push_back((hnd)(scan << 1));
        }
        queue.clear();
        for (hnd s : seeds) {
            if (visited[hid(s)]) continue;
            visited[hid(s)] = 1;
            if (s & 1) flipped[hid(s)] = 1;
            queue.push_back(s);
        }
        for (size_t qi = 0; qi < queue.size(); qi++) {
            const hnd cur = queue[qi];
            for (uint64_t k = off[cur]; k < off[cur + 1]; k++) {
                const hnd next = to[k];
                if (visited[hid(next)]) continue;
                visited[hid(next)] = 1;
                if (next & 1) flipped[hid(next)] = 1;
                queue.push_back(next);
            }
        }
        seeds.clear();
    }
    for (size_t id = 0; id < NN; id++) {
        if (!flipped[id]) continue;
        std::string &s = g.node_seq[id];
        std::reverse(s.begin(), s.end());
        for (auto &c : s) c = (char)rc_base((uint8_t)c);
    }
    auto fl = [&](hnd h) { return flipped[hid(h)] ? (hnd)(h ^ 1u) : h; };
    for (auto &e : g.edges) { e.first = fl(e.first); e.second = fl(e.second); }
    for (auto &h : g.steps) h = fl(h);
}

// exact_odgi_topological_order(use_heads = true, use_tails = false) (src/bidirected_ops.rs:1390-1599): node ids in emission order
static std::vector<uint32_t> topo_order(const SrGraph &g) {
    const size_t NN = g.node_seq.size(), NH = NN * 2, E = g.edges.size();
    std::vector<uint64_t> ooff(NH + 1, 0), ioff(NH + 1, 0);
    for (const auto &e : g.edges) { ooff[e.first + 1]++; ioff[e.second + 1]++; }
    for (size_t h = 0; h < NH; h++) { ooff[h + 1] += ooff[h]; ioff[h + 1] += ioff[h]; }
    std::vector<uint32_t> oedge(E), iedge(E);
    {
        std::vector<uint64_t> of(ooff.begin(), ooff.end() - 1), inf(ioff.begin(), ioff.end() - 1);
        for (uint32_t k = 0; k < E; k++) { oedge[of[g.edges[k].first]++] = k; iedge[inf[g.edges[k].second]++] = k; }
        for (size_t h = 0; h < NH; h++)            // outgoing edges in ascending `to` (the reference sorts all edges)
            std::sort(oedge.begin() + ooff[h], oedge.begin() + ooff[h + 1],
                      [&](uint32_t a, uint32_t b) { return g.edges[a].second < g.edges[b].second; });
    }
    std::vector<uint32_t> unmasked_in(NH, 0);
    for (const auto &e : g.edges) unmasked_in[e.second]++;
    std::vector<uint8_t> masked(E, 0), unvisited(NH, 0), emitted(NN, 0);
    size_t n_unvisited = 0;
    for (size_t id = 0; id < NN; id++)
        if (g.node_alive[id]) { unvisited[id << 1] = unvisited[(id << 1) | 1] = 1; n_unvisited += 2; }
    auto take = [&](hnd h) {                         // unvisited.remove(h), unvisited.remove(h.flip())
        if (unvisited[h]) { unvisited[h] = 0; n_unvisited--; }
        if (unvisited[h ^ 1]) { unvisited[h ^ 1] = 0; n_unvisited--; }
    };
    std::set<hnd> S, seeds;
    for (hnd h : find_heads(g)) { S.insert(h); take(h); }
    std::vector<uint32_t> sorted;
    size_t cursor = 0;                               // unvisited only shrinks: its minimum never moves back
    while (n_unvisited > 0 || !S.empty()) {
        if (S.empty()) {
            bool found = false;
            if (!seeds.empty()) {
                const hnd h = *seeds.begin();
                seeds.erase(seeds.begin());
                if (unvisited[h]) { S.insert(h); take(h); found = true; }
            }
            if (!found && n_unvisited > 0) {
                while (!unvisited[cursor]) cursor++;
                const hnd h = (hnd)cursor;
                S.insert(h); take(h);
            }
        }
        while (!S.empty()) {
            const hnd h = *S.begin();
            S.erase(S.begin());
            if (!emitted[hid(h)]) { emitted[hid(h)] = 1; sorted.push_back(hid(h)); }
            for (uint64_t k = ioff[h]; k < ioff[h + 1]; k++) {
                const uint32_t e = iedge[k];
                if (!masked[e]) { masked[e] = 1; unmasked_in[g.edges[e].second]--; }
            }
            for (uint64_t k = ooff[h]; k < ooff[h + 1]; k++) {
                const uint32_t e = oedge[k];
                if (masked[e]) continue;
                masked[e] = 1;
                const hnd next = g.edges[e].second;
                unmasked_in[next]--;
                if (!unvisited[next]) continue;
                if (unmasked_in[next] == 0) { S.insert(next); take(next); }
                else seeds.insert(next);
            }
        }
    }
    return sorted;
}

static void spell_paths(const SrGraph &g, std::vector<std::string> &out) {
    out.assign(g.path_off.size() - 1, std::string());
    for (size_t q = 0; q + 1 < g.path_off.size(); q++)
        for (uint64_t i = g.path_off[q]; i < g.path_off[q + 1]; i++) {
            const hnd h = g.steps[i];
            const std::string &s = g.node_seq[hid(h)];
            if (h & 1) for (size_t k = s.size(); k-- > 0;) out[q].push_back((char)rc_base((uint8_t)s[k]));
            else out[q] += s;
        }
}

int sr_graph_ygs(SrGraph &g, const sr_sort_params &prm, void *stream) {
    for (double &s : g_stats) s = 0;
    const auto t_all = std::chrono::steady_clock::now();    // slot [9]: the whole stage, verification included
    std::vector<std::string> before, after;
    spell_paths(g, before);
    g_stats[7] = (double)alive_ids(g).size();
    g_stats[8] = (double)g.steps.size();
    if (!prm.skip_sgd) {                             // Y: path_sgd_sort + apply_ordering (src/path_sgd.rs:578-603)
        SgdProblem p;
        int r = sgd_prepare(g, prm, p);
        if (r) return r;
        g_stats[4] = (double)p.min_term_updates;
        g_stats[5] = (double)p.iters;
        g_stats[6] = (double)((p.min_term_updates + p.terms_per_round - 1) / p.terms_per_round);
        if (p.has_terms) {
            std::vector<double> x;
            if ((r = sgd_positions(p, prm, stream, x, &g_stats[0]))) return r;
            std::vector<uint32_t> idx(p.n_nodes);
            for (uint32_t i = 0; i < p.n_nodes; i++) idx[i] = i;
            std::sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return x[a] < x[b] || (x[a] == x[b] && a < b); });
            std::vector<uint32_t> order(p.n_nodes);
            for (size_t r2 = 0; r2 < idx.size(); r2++) order[r2] = p.node_id[idx[r2]];
            apply_ordering(g, order);
        }
    }
    if (!prm.skip_groom) {                           // g
        const auto t0 = std::chrono::steady_clock::now();
        groom(g);
        g_stats[1] = ms_since(t0);
    }
    const auto t0 = std::chrono::steady_clock::now();
    if (!prm.skip_topo) apply_ordering(g, topo_order(g));   // s
    else apply_ordering(g, alive_ids(g));                   // ids dense 1..N whatever ran
    std::sort(g.edges.begin(), g.edges.end());
    g_stats[2] = ms_since(t0);
    spell_paths(g, after);
    for (size_t q = 0; q < before.size(); q++)
        if (before[q] != after[q])
            return sr_fail(SR_ERR_DEVICE_FAULT, "sort: path " + std::to_string(q) + " no longer spells its sequence (internal error)");
    g_stats[9] = ms_since(t_all);
    return SR_OK;
}

// ------------------------------------------------------------------ GFA input
static bool parse_u32(const char *b, const char *e, uint32_t *out) {
    if (b == e) return false;
    uint64_t v = 0;
    for (const char *c = b; c < e; c++) {
        if (*c < '0' || *c > '9') return false;
        v = v * 10 + (uint64_t)(*c - '0');
        if (v >= 0x7fffffffULL) return false;
    }
    *out = (uint32_t)v;
    return true;
}

// S ids are mapped to 1..n in ascending order (every rule of the sort depends on id order only, and the output is
// renumbered anyway), so memory follows the number of S lines, not the largest id
int sr_graph_parse_gfa(const char *text, SrGraph &g, std::vector<std::string> &names) {
    g = SrGraph();
    names.clear();
    g.path_off.assign(1, 0);
    std::vector<std::pair<uint32_t, std::string>> segs;
    std::vector<std::pair<uint32_t, uint32_t>> edges;   // (gfa id << 1 | rev) pairs, ids still unmapped
    std::vector<std::vector<std::pair<uint32_t, int>>> raw_paths;
    const char *p = text;
    uint64_t lineno = 0;
    while (*p) {
        const char *eol = strchr(p, '\n');
        if (!eol) eol = p + strlen(p);
        const char *le = eol;
        if (le > p && le[-1] == '\r') le--;
        lineno++;
        std::vector<std::pair<const char *, const char *>> f;
        for (const char *a = p; a <= le;) {
            const char *b = (const char *)memchr(a, '\t', (size_t)(le - a));
            if (!b) b = le;
            f.push_back({a, b});
            a = b + 1;
        }
        auto bad = [&](const char *why) { return sr_fail(SR_ERR_INVALID, "GFA line " + std::to_string(lineno) + ": " + why); };
        const char kind = (le > p) ? *p : 0;
        if (kind == 'S') {
            uint32_t id;
            if (f.size() < 3 || !parse_u32(f[1].first, f[1].second, &id) || id == 0) return bad("S needs a positive numeric id and a sequence");
            segs.emplace_back(id, std::string(f[2].first, f[2].second));
        } else if (kind == 'L') {
            uint32_t a, b;
            if (f.size() < 5 || !parse_u32(f[1].first, f[1].second, &a) || !parse_u32(f[3].first, f[3].second, &b) ||
                f[2].second - f[2].first != 1 || f[4].second - f[4].first != 1) return bad("L needs from, orient, to, orient");
            const char oa = *f[2].first, ob = *f[4].first;
            if ((oa != '+' && oa != '-') || (ob != '+' && ob != '-')) return bad("orientation must be + or -");
            edges.push_back({(a << 1) | (oa == '-'), (b << 1) | (ob == '-')});
        } else if (kind == 'P') {
            if (f.size() < 3) return bad("P needs a name and steps");
            names.emplace_back(f[1].first, f[1].second);
            raw_paths.emplace_back();
            for (const char *a = f[2].first; a < f[2].second;) {
                const char *b = (const char *)memchr(a, ',', (size_t)(f[2].second - a));
                if (!b) b = f[2].second;
                uint32_t id;
                if (b - a < 2 || (b[-1] != '+' && b[-1] != '-') || !parse_u32(a, b - 1, &id)) return bad("bad path step");
                raw_paths.back().push_back({id, b[-1] == '-'});
                a = b + 1;
            }
        }
        p = *eol ? eol + 1 : eol;
    }
    std::stable_sort(segs.begin(), segs.end(),
                     [](const std::pair<uint32_t, std::string> &a, const std::pair<uint32_t, std::string> &b) { return a.first < b.first; });
    std::unordered_map<uint32_t, uint32_t> dense;
    dense.reserve(segs.size() * 2);
    g.node_seq.assign(segs.size() + 1, std::string()); g.node_alive.assign(segs.size() + 1, 1);
    g.node_alive[0] = 0;
    for (size_t i = 0; i < segs.size(); i++) {
        if (i && segs[i].first == segs[i - 1].first)
            return sr_fail(SR_ERR_INVALID, "GFA: duplicate S id " + std::to_string(segs[i].first));
        dense[segs[i].first] = (uint32_t)(i + 1);
        g.node_seq[i + 1] = std::move(segs[i].second);
    }
    auto map_h = [&](uint32_t id, uint32_t rev, hnd *out) {
        auto it = dense.find(id);
        if (it == dense.end()) return false;
        *out = (it->second << 1) | rev;
        return true;
    };
    std::unordered_set<uint64_t> seen;
    for (const auto &e : edges) {
        hnd a, b;
        if (!map_h(hid(e.first), e.first & 1u, &a) || !map_h(hid(e.second), e.second & 1u, &b))
            return sr_fail(SR_ERR_INVALID, "GFA: an L line names a missing segment");
        if (seen.insert(((uint64_t)a << 32) | b).second) g.edges.push_back({a, b});
    }
    for (size_t pi = 0; pi < raw_paths.size(); pi++) {
        const auto &rp = raw_paths[pi];
        for (const auto &st : rp) {
            hnd h;
            if (!map_h(st.first, (uint32_t)st.second, &h))
                return sr_fail(SR_ERR_INVALID, "GFA: a P line names a missing segment (path '" + names[pi] + "', segment " + std::to_string(st.first) + ")");
            g.steps.push_back(h);
        }
        g.path_off.push_back(g.steps.size());
    }
    return SR_OK;
}

// ------------------------------------------------------------------ C ABI
static sr_sort_params resolve_params(const sr_sort_params *p) {
    sr_sort_params q;
    if (p) q = *p; else sr_sort_params_default(&q);
    return q;
}

extern "C" int sr_sort_gfa(const char *gfa_in, const sr_sort_params *p, char **gfa_out, uint64_t *n_nodes, uint64_t *n_edges) {
    if (!gfa_in || !gfa_out) return sr_fail(SR_ERR_INVALID, "null argument");
    SrGraph g;
    std::vector<std::string> names;
    int r = sr_graph_parse_gfa(gfa_in, g, names);
    if (r) return r;
    const sr_sort_params prm = resolve_params(p);
    if ((r = sr_graph_ygs(g, prm, nullptr))) return r;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<const char *> cn;
    for (const auto &s : names) cn.push_back(s.c_str());
    *gfa_out = sr_graph_format_gfa(g, cn.data(), n_nodes, n_edges);
    sr_sort_note_write_ms(ms_since(t0));
    return SR_OK;
}

extern "C" int sr_sgd_layout(const char *gfa_in, const sr_sort_params *p, double *pos_out, uint64_t n) {
    if (!gfa_in || !pos_out) return sr_fail(SR_ERR_INVALID, "null argument");
    SrGraph g;
    std::vector<std::string> names;
    int r = sr_graph_parse_gfa(gfa_in, g, names);
    if (r) return r;
    const sr_sort_params prm = resolve_params(p);
    SgdProblem sp;
    if ((r = sgd_prepare(g, prm, sp))) return r;
    if (n != sp.n_nodes) return sr_fail(SR_ERR_INVALID, "sr_sgd_layout: n must be the number of nodes (" + std::to_string(sp.n_nodes) + ")");
    std::vector<double> x = sp.x0;
    for (double &s : g_stats) s = 0;
    if (sp.has_terms && (r = sgd_positions(sp, prm, nullptr, x, &g_stats[0]))) return r;
    g_stats[4] = (double)sp.min_term_updates; g_stats[5] = (double)sp.iters;
    g_stats[6] = (double)((sp.min_term_updates + sp.terms_per_round - 1) / sp.terms_per_round);
    g_stats[7] = (double)sp.n_nodes; g_stats[8] = (double)g.steps.size();
    memcpy(pos_out, x.data(), n * sizeof(double));
    return SR_OK;
}

extern "C" int sr_sgd_tables(const char *gfa_in, const sr_sort_params *p, sr_sort_params *resolved, uint64_t sizes[4],
                             double *etas, double *zetas, double *prefix_theta, double *prefix_cool) {
    if (!gfa_in || !sizes) return sr_fail(SR_ERR_INVALID, "null argument");
    SrGraph g;
    std::vector<std::string> names;
    int r = sr_graph_parse_gfa(gfa_in, g, names);
    if (r) return r;
    const sr_sort_params prm = resolve_params(p);
    SgdProblem sp;
    if ((r = sgd_prepare(g, prm, sp))) return r;
    sizes[0] = sp.etas.size(); sizes[1] = sp.zetas.size(); sizes[2] = sp.prefix_theta.size(); sizes[3] = sp.n_nodes;
    if (resolved) {
        *resolved = prm;
        resolved->eta_max = sp.eta_max; resolved->min_term_updates = sp.min_term_updates; resolved->space = sp.space;
        resolved->terms_per_round = sp.terms_per_round;
    }
    if (etas) memcpy(etas, sp.etas.data(), sp.etas.size() * sizeof(double));
    if (zetas) memcpy(zetas, sp.zetas.data(), sp.zetas.size() * sizeof(double));
    if (prefix_theta) memcpy(prefix_theta, sp.prefix_theta.data(), sp.prefix_theta.size() * sizeof(double));
    if (prefix_cool) memcpy(prefix_cool, sp.prefix_cool.data(), sp.prefix_cool.size() * sizeof(double));
    return SR_OK;
}
