// sr_extract.hip -- the subgraph extraction (--extract-*; include/seqrush_amd.h "extracting a subgraph", DESIGN.md section
// 19): the nodes that regions of paths touch, their context over the L lines, the gaps between them that close, and the
// graph of those nodes with every path cut into subpaths, on the device and, in plain loops over the same rule header, on
// the host.  Every value is an integer decided by a min, a max or a sum, so the two agree exactly.  The regions are read
// and the GFA bytes are formed here on the host, once for every front end.
//
// Device: six groups of kernels on one stream, hipEvents around them: positions (step lengths, a sum scan, the offset and
// the path of every step) -> seeds (one lane per step bisects the sorted regions of its path, atomicMin of level 0) ->
// context (one launch per round, one lane per edge, atomicMin of the round) -> merge (per round: the kept flags as s + 1 or
// 0, a max scan forwards and one over the reversed array, one lane per step that is not kept, atomicMin of c + k; a word
// "added" comes back after each round) -> numbering (four sum scans) -> emission (plain stores at the scanned positions).
// The only atomics are the mins on `level`, whose result does not depend on their order.  Every dependency is a kernel
// boundary.  No captured graph.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <numeric>
#include <string>
#include <unordered_map>
#include <vector>
#include "../../include/seqrush_amd.h"
#include "sr_internal.h"
#include "sr_sort.h"
#include "sr_stage_host.h"
#include "sr_stage_dev.h"
#include "sr_bed_host.h"
#include "sr_extract_rule.h"

#define EX_BLOCK 256

typedef uint64_t u64d;

static_assert(EX_BLOCK == SR_STAGE_BLOCK, "the grids of sr_stage_grid");

// kept[s] of the rule header, read through the level of the step's node
struct ExKept {
    const uint32_t *steps, *level;
    SR_EX_HD bool operator[](uint32_t s) const { return level[(steps[s] >> 1) - 1] != SR_EXTRACT_NONE; }
};

// what the kernels read and write; every pointer is device memory
struct ExDev {
    uint32_t V, S, P, E;
    const uint32_t *len, *steps, *path_off, *efrom, *eto;      // the graph
    const u64d *reg_start, *reg_pmax;                          // the regions, sorted by (path, start); reg_off[P + 1]
    const uint32_t *reg_off;
    u64d *sinc, *pstart;                                       // [S]
    uint32_t *spath;                                           // [S] the path of a step
    uint32_t *level;                                           // [V]
    u64d *fwd, *bwd;                                           // [S] merge: the previous / the next kept step
    u64d *nnode, *nedge, *nrun, *nstep;                        // [V] [E] [S] [S] numbering
    uint32_t *o_node_old, *o_efrom, *o_eto, *o_sub_path, *o_sub_steps;
    u64d *o_sub_start, *o_sub_end, *o_sub_off;
};

// ------------------------------------------------------------------ group 0: positions
// the step lengths and their inclusive scan: sr_stage_dev.h.  (lf_pstart_kernel of sr_lift.hip with the path kept as well)
__global__ void __launch_bounds__(EX_BLOCK) ex_pstart_kernel(ExDev d) {
    const uint32_t s = blockIdx.x * EX_BLOCK + threadIdx.x;
    if (s >= d.S) return;
    const uint32_t p = sr_path_of(d.path_off, d.P, s), a0 = d.path_off[p];
    d.spath[s] = p;
    d.pstart[s] = d.sinc[s] - d.len[(d.steps[s] >> 1) - 1] - (a0 ? d.sinc[a0 - 1] : 0);
}

// ------------------------------------------------------------------ group 1: seeds
__global__ void __launch_bounds__(EX_BLOCK) ex_seed_kernel(ExDev d) {
    const uint32_t s = blockIdx.x * EX_BLOCK + threadIdx.x;
    if (s >= d.S) return;
    const uint32_t p = d.spath[s], r0 = d.reg_off[p], r1 = d.reg_off[p + 1];
    if (r0 == r1) return;
    const uint32_t v = (d.steps[s] >> 1) - 1;
    if (sr_extract_seed(d.reg_start, d.reg_pmax, r0, r1, d.pstart[s], d.len[v])) atomicMin(&d.level[v], 0u);
}

// ------------------------------------------------------------------ group 2: context, one launch per round r
// a lane tests for r - 1 only, which an earlier launch wrote: a stale read within the launch costs a redundant atomic
__global__ void __launch_bounds__(EX_BLOCK) ex_context_kernel(ExDev d, uint32_t r) {
    const uint32_t e = blockIdx.x * EX_BLOCK + threadIdx.x;
    if (e >= d.E) return;
    const uint32_t a = (d.efrom[e] >> 1) - 1, b = (d.eto[e] >> 1) - 1;
    const uint32_t la = d.level[a], lb = d.level[b];
    if (sr_extract_hands_on(la, lb, r)) atomicMin(&d.level[b], r);
    if (sr_extract_hands_on(lb, la, r)) atomicMin(&d.level[a], r);
}

// ------------------------------------------------------------------ group 3: merge, per round
// the set at the start of the round: fwd[s] = s + 1 where step s is kept, else 0, and the same over the reversed array
__global__ void __launch_bounds__(EX_BLOCK) ex_kept_kernel(ExDev d) {
    const uint32_t s = blockIdx.x * EX_BLOCK + threadIdx.x;
    if (s >= d.S) return;
    const bool k = ExKept{d.steps, d.level}[s];
    d.fwd[s] = k ? (u64d)s + 1 : 0;
    d.bwd[d.S - 1 - s] = k ? (u64d)(d.S - 1 - s) + 1 : 0;
}

// after the two max scans: fwd[s] - 1 = the last kept step at or before s, S - bwd[S - 1 - s] = the first at or behind it.
// Reads only the scans, writes only level (and the word): the round is a Jacobi round
__global__ void __launch_bounds__(EX_BLOCK) ex_gap_kernel(ExDev d, u64d D, uint32_t lvl, uint32_t *added) {
    const uint32_t s = blockIdx.x * EX_BLOCK + threadIdx.x;
    if (s >= d.S) return;
    const u64d f = d.fwd[s], b = d.bwd[d.S - 1 - s];
    if (f == (u64d)s + 1 || !f || !b) return;                  // kept, or no kept step on one side
    const uint32_t prev = (uint32_t)(f - 1), next = (uint32_t)(d.S - b), p = d.spath[s];
    if (prev < d.path_off[p] || next >= d.path_off[p + 1]) return;      // a neighbour in another path
    if (!sr_extract_gap_closes(d.pstart[prev], d.len[(d.steps[prev] >> 1) - 1], d.pstart[next], D)) return;
    atomicMin(&d.level[(d.steps[s] >> 1) - 1], lvl);
    *added = 1u;                                               // every lane stores the same word
}

// ------------------------------------------------------------------ group 4: numbering, the flags of the four sum scans
__global__ void __launch_bounds__(EX_BLOCK) ex_flag_node_kernel(ExDev d) {
    const uint32_t v = blockIdx.x * EX_BLOCK + threadIdx.x;
    if (v < d.V) d.nnode[v] = d.level[v] != SR_EXTRACT_NONE ? 1 : 0;
}

__device__ __forceinline__ bool ex_edge_kept(const ExDev &d, uint32_t e) {
    return d.level[(d.efrom[e] >> 1) - 1] != SR_EXTRACT_NONE && d.level[(d.eto[e] >> 1) - 1] != SR_EXTRACT_NONE;
}

__global__ void __launch_bounds__(EX_BLOCK) ex_flag_edge_kernel(ExDev d) {
    const uint32_t e = blockIdx.x * EX_BLOCK + threadIdx.x;
    if (e < d.E) d.nedge[e] = ex_edge_kept(d, e) ? 1 : 0;
}

__global__ void __launch_bounds__(EX_BLOCK) ex_flag_step_kernel(ExDev d) {
    const uint32_t s = blockIdx.x * EX_BLOCK + threadIdx.x;
    if (s >= d.S) return;
    const ExKept kept{d.steps, d.level};
    d.nstep[s] = kept[s] ? 1 : 0;
    d.nrun[s] = sr_extract_run_starts(kept, d.path_off[d.spath[s]], s) ? 1 : 0;
}

// ------------------------------------------------------------------ group 5: emission; no slot comes from an atomic
__global__ void __launch_bounds__(EX_BLOCK) ex_emit_node_kernel(ExDev d) {
    const uint32_t v = blockIdx.x * EX_BLOCK + threadIdx.x;
    if (v < d.V && d.level[v] != SR_EXTRACT_NONE) d.o_node_old[d.nnode[v] - 1] = v + 1;
}

__device__ __forceinline__ uint32_t ex_new_handle(const ExDev &d, uint32_t h) { return ((uint32_t)d.nnode[(h >> 1) - 1] << 1) | (h & 1u); }

__global__ void __launch_bounds__(EX_BLOCK) ex_emit_edge_kernel(ExDev d) {
    const uint32_t e = blockIdx.x * EX_BLOCK + threadIdx.x;
    if (e >= d.E || !ex_edge_kept(d, e)) return;
    const u64d k = d.nedge[e] - 1;
    d.o_efrom[k] = ex_new_handle(d, d.efrom[e]); d.o_eto[k] = ex_new_handle(d, d.eto[e]);
}

__global__ void __launch_bounds__(EX_BLOCK) ex_emit_step_kernel(ExDev d) {
    const uint32_t s = blockIdx.x * EX_BLOCK + threadIdx.x;
    if (s >= d.S) return;
    const ExKept kept{d.steps, d.level};
    if (!kept[s]) return;
    const uint32_t p = d.spath[s], h = d.steps[s];
    const u64d at = d.nstep[s] - 1, j = d.nrun[s] - 1;         // a kept step lies in the run whose start was counted last
    d.o_sub_steps[at] = ex_new_handle(d, h);
    if (sr_extract_run_starts(kept, d.path_off[p], s)) { d.o_sub_path[j] = p; d.o_sub_start[j] = d.pstart[s]; d.o_sub_off[j] = at; }
    if (sr_extract_run_ends(kept, d.path_off[p + 1], s)) d.o_sub_end[j] = d.pstart[s] + d.len[(h >> 1) - 1];
}

namespace {

// the tables both executions read.  Node v = 1..V sits at index v - 1.
struct ExTables : SrPathTables {
    uint32_t E = 0;
    std::vector<uint32_t> efrom, eto;
    std::vector<uint64_t> plen;
    uint64_t c = 0, D = 100000, R = 3;
    // the regions that count, in the order given (BED lines, then strings)
    std::vector<uint32_t> r_path;
    std::vector<uint64_t> r_start, r_end;
    uint64_t unknown = 0, out_of_range = 0;
};

struct ExOut {
    int variant = 0;
    uint64_t us = 0, kernel_us[6] = {0, 0, 0, 0, 0, 0}, rounds_run = 0;
    std::vector<uint32_t> level, node_old, edge_from, edge_to, sub_path, sub_steps;
    std::vector<uint64_t> sub_start, sub_end, sub_off;
};

// what the writer needs beyond the tables of sr_extract
struct ExPriv {
    std::vector<std::string> seq;                    // [nodes] of the result
    std::vector<std::string> names;                  // [in_paths]
};

int ex_tables(const SrGraph &g, const sr_extract_params &prm, ExTables &t) {
    const SrPathSizes z = sr_path_sizes(g);
    if (prm.context_steps > SR_EXTRACT_MAX_CONTEXT) return sr_fail(SR_ERR_UNSUPPORTED, "extract: context_steps supports at most 65535");
    if (prm.merge_rounds > SR_EXTRACT_MAX_ROUNDS) return sr_fail(SR_ERR_UNSUPPORTED, "extract: merge_rounds supports at most 64");
    if (z.nodes >= 0x3fffffffULL || z.steps >= 0x7fffffffULL || z.paths >= 0x7fffffffULL || z.edges >= 0x7fffffffULL)
        return sr_fail(SR_ERR_UNSUPPORTED, "extract supports < 2^30 nodes and < 2^31 steps, paths and edges");
    t.c = prm.context_steps; t.D = prm.merge_distance; t.R = prm.merge_rounds;
    if (const int r = sr_path_tables_fill(g, z, "extract", true, false, t)) return r;
    t.E = (uint32_t)z.edges;
    t.efrom.resize(t.E); t.eto.resize(t.E);
    for (uint32_t e = 0; e < t.E; e++) {
        t.efrom[e] = g.edges[e].first; t.eto[e] = g.edges[e].second;
        if ((t.efrom[e] >> 1) == 0 || (t.efrom[e] >> 1) > t.V || (t.eto[e] >> 1) == 0 || (t.eto[e] >> 1) > t.V)
            return sr_fail(SR_ERR_INVALID, "extract: an edge names a missing node");
    }
    t.plen.assign(t.P, 0);
    for (uint32_t p = 0; p < t.P; p++)
        for (uint32_t s = t.path_off[p]; s < t.path_off[p + 1]; s++) t.plen[p] += t.len[(t.steps[s] >> 1) - 1];
    return SR_OK;
}

// ------------------------------------------------------------------ the regions: BED lines, then strings
int ex_regions(const char *bed, const char *const *regions, uint64_t n_regions, const std::vector<std::string> &names, ExTables &t) {
    std::unordered_map<std::string, uint32_t> by_name;
    for (uint32_t p = 0; p < t.P && p < names.size(); p++) by_name.emplace(names[p], p);      // the first path of a name
    auto add = [&](uint32_t p, uint64_t start, uint64_t end) { t.r_path.push_back(p); t.r_start.push_back(start); t.r_end.push_back(end); };
    if (bed) {
        const int r = sr_bed_lines(bed, "extract", [&](const std::vector<std::string> &f, uint64_t start, uint64_t end) {
            const auto it = by_name.find(f[0]);
            if (it == by_name.end()) { t.unknown++; return SR_OK; }
            if (start >= end || end > t.plen[it->second]) { t.out_of_range++; return SR_OK; }
            add(it->second, start, end);
            return SR_OK;
        });
        if (r) return r;
    }
    for (uint64_t i = 0; i < n_regions; i++) {
        if (!regions || !regions[i]) return sr_fail(SR_ERR_INVALID, "null argument");
        const std::string s = regions[i], where = "extract: region '" + s + "': ";
        auto it = by_name.find(s);
        if (it != by_name.end()) {                                // the name wins, also where it looks like NAME:S-E
            if (!t.plen[it->second]) t.out_of_range++; else add(it->second, 0, t.plen[it->second]);
            continue;
        }
        const size_t colon = s.rfind(':');
        if (colon == std::string::npos) return sr_fail(SR_ERR_INVALID, where + "no path has this name and there is no ':START-END'");
        const std::string name = s.substr(0, colon), range = s.substr(colon + 1);
        const size_t dash = range.find('-');
        uint64_t start = 0, end = 0;
        if (dash == std::string::npos || !sr_bed_number(range.substr(0, dash), &start) || !sr_bed_number(range.substr(dash + 1), &end))
            return sr_fail(SR_ERR_INVALID, where + "'" + range + "' is not START-END");
        it = by_name.find(name);
        if (it == by_name.end()) return sr_fail(SR_ERR_INVALID, where + "no path is named '" + name + "'");
        if (start >= end) return sr_fail(SR_ERR_INVALID, where + "start must lie below end");
        if (end > t.plen[it->second]) return sr_fail(SR_ERR_INVALID, where + "end lies beyond the " + u64s(t.plen[it->second]) + " bases of the path");
        add(it->second, start, end);
    }
    if (t.r_path.size() > SR_EXTRACT_MAX_REGIONS)
        return sr_fail(SR_ERR_UNSUPPORTED, "extract: " + std::to_string(t.r_path.size()) + " regions; at most 2^24 are supported");
    return SR_OK;
}

void ex_empty(const ExTables &t, ExOut &o) { o.level.assign(t.V, SR_EXTRACT_NONE); o.sub_off.assign(1, 0); }

// ------------------------------------------------------------------ host twin: one thread, plain loops
int ex_run_host(const ExTables &t, ExOut &o) {
    const auto t_all = std::chrono::steady_clock::now();
    auto t0 = t_all;
    auto lap = [&](int k) { o.kernel_us[k] = (uint64_t)(us_since(t0) + 0.5); t0 = std::chrono::steady_clock::now(); };
    o.variant = 0;
    ex_empty(t, o);
    if (t.r_path.empty()) return SR_OK;
    std::vector<uint32_t> &level = o.level;
    auto node = [&](uint32_t s) { return (t.steps[s] >> 1) - 1; };
    std::vector<uint64_t> pstart(t.S, 0);
    for (uint32_t p = 0; p < t.P; p++) {
        uint64_t at = 0;
        for (uint32_t s = t.path_off[p]; s < t.path_off[p + 1]; s++) { pstart[s] = at; at += t.len[node(s)]; }
    }
    lap(0);
    for (size_t i = 0; i < t.r_path.size(); i++)                 // seeds: a walk per region
        for (uint32_t s = t.path_off[t.r_path[i]]; s < t.path_off[t.r_path[i] + 1] && pstart[s] < t.r_end[i]; s++)
            if (sr_extract_touches(pstart[s], t.len[node(s)], t.r_start[i], t.r_end[i])) level[node(s)] = 0;
    lap(1);
    if (t.c && t.E) {                                            // context: breadth first over an adjacency list
        std::vector<uint32_t> deg(t.V + 1, 0), adj, queue;
        for (uint32_t e = 0; e < t.E; e++) { deg[(t.efrom[e] >> 1) - 1]++; deg[(t.eto[e] >> 1) - 1]++; }
        uint32_t sum = 0;
        for (uint32_t v = 0; v <= t.V; v++) { const uint32_t n = deg[v]; deg[v] = sum; sum += n; }
        adj.resize(sum);
        std::vector<uint32_t> fill(deg.begin(), deg.end() - 1);
        for (uint32_t e = 0; e < t.E; e++) {
            const uint32_t a = (t.efrom[e] >> 1) - 1, b = (t.eto[e] >> 1) - 1;
            adj[fill[a]++] = b; adj[fill[b]++] = a;
        }
        for (uint32_t v = 0; v < t.V; v++) if (level[v] == 0) queue.push_back(v);
        for (size_t q = 0; q < queue.size(); q++) {
            const uint32_t v = queue[q], r = level[v] + 1;
            if (r > t.c) break;                                   // the queue is sorted by level
            for (uint32_t k = deg[v]; k < deg[v + 1]; k++)
                if (sr_extract_hands_on(level[v], level[adj[k]], r)) { level[adj[k]] = r; queue.push_back(adj[k]); }
        }
    }
    lap(2);
    for (uint64_t k = 1; k <= t.R; k++) {                        // merge: a walk per path, judged against the round's start
        std::vector<uint32_t> add;
        for (uint32_t p = 0; p < t.P; p++) {
            bool have = false;
            uint32_t prev = 0;
            for (uint32_t s = t.path_off[p]; s < t.path_off[p + 1]; s++) {
                if (level[node(s)] == SR_EXTRACT_NONE) continue;
                if (have && s - prev > 1 && sr_extract_gap_closes(pstart[prev], t.len[node(prev)], pstart[s], t.D))
                    for (uint32_t x = prev + 1; x < s; x++) add.push_back(node(x));
                have = true; prev = s;
            }
        }
        if (add.empty()) break;
        for (uint32_t v : add) level[v] = (uint32_t)(t.c + k);
        o.rounds_run++;
    }
    lap(3);
    std::vector<uint32_t> new_id(t.V, 0);                        // numbering by counting
    uint32_t n_nodes = 0;
    for (uint32_t v = 0; v < t.V; v++) if (level[v] != SR_EXTRACT_NONE) new_id[v] = ++n_nodes;
    lap(4);
    auto handle = [&](uint32_t h) { return (new_id[(h >> 1) - 1] << 1) | (h & 1u); };
    for (uint32_t v = 0; v < t.V; v++) if (new_id[v]) o.node_old.push_back(v + 1);
    for (uint32_t e = 0; e < t.E; e++)
        if (new_id[(t.efrom[e] >> 1) - 1] && new_id[(t.eto[e] >> 1) - 1]) { o.edge_from.push_back(handle(t.efrom[e])); o.edge_to.push_back(handle(t.eto[e])); }
    const ExKept kept{t.steps.data(), level.data()};
    o.sub_off.clear();
    for (uint32_t p = 0; p < t.P; p++)
        for (uint32_t s = t.path_off[p]; s < t.path_off[p + 1]; s++) {
            if (!kept[s]) continue;
            if (sr_extract_run_starts(kept, t.path_off[p], s)) { o.sub_path.push_back(p); o.sub_start.push_back(pstart[s]); o.sub_off.push_back(o.sub_steps.size()); }
            o.sub_steps.push_back(handle(t.steps[s]));
            if (sr_extract_run_ends(kept, t.path_off[p + 1], s)) o.sub_end.push_back(pstart[s] + t.len[node(s)]);
        }
    o.sub_off.push_back(o.sub_steps.size());
    lap(5);
    o.us = (uint64_t)(us_since(t_all) + 0.5);
    return SR_OK;
}

// ------------------------------------------------------------------ device execution
template <class K, class... A> void ex_launch(SrStage &x, K kernel, uint64_t n, A... args) {
    if (x.err || !n) return;                                     // no workgroup for no item
    hipLaunchKernelGGL(kernel, dim3(sr_stage_grid(n)), dim3(EX_BLOCK), 0, x.st, args...);
}

// consecutive tables of one device allocation, each on a 256-byte boundary
struct ExArena {
    uintptr_t base;
    uint64_t at;
    template <class T> T *take(uint64_t n) {
        T *p = (T *)(base + at);
        at += ((n ? n : 1) * sizeof(T) + 255) & ~255ULL;
        return p;
    }
};

int ex_run_device(const ExTables &t, int device, void *stream, ExOut &o) {
    const uint32_t V = t.V, S = t.S, P = t.P, E = t.E, N = (uint32_t)t.r_path.size();
    SrStage x("extract", "the extract tables");
    if (x.open(device, stream, 7)) return x.err;
    o.variant = 1;
    ex_empty(t, o);
    if (!N) return SR_OK;                                        // no region: nothing is kept (a region implies a step and a node)

    // the regions by (path, start), the largest end so far within the path
    std::vector<uint32_t> order(N), reg_off((size_t)P + 1, 0);
    std::iota(order.begin(), order.end(), 0u);
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        return t.r_path[a] != t.r_path[b] ? t.r_path[a] < t.r_path[b] : t.r_start[a] != t.r_start[b] ? t.r_start[a] < t.r_start[b] : a < b;
    });
    std::vector<uint64_t> reg_start(N), reg_pmax(N);
    for (uint32_t k = 0; k < N; k++) {
        const uint32_t i = order[k];
        reg_start[k] = t.r_start[i];
        reg_pmax[k] = k && t.r_path[order[k - 1]] == t.r_path[i] ? std::max(reg_pmax[k - 1], t.r_end[i]) : t.r_end[i];
        reg_off[t.r_path[i] + 1]++;
    }
    for (uint32_t p = 0; p < P; p++) reg_off[p + 1] += reg_off[p];

    // One allocation for every table: the stage has 32 of them, and as many hipMalloc and hipFree calls cost more than its
    // kernels run.  The tables are carved twice by the same code, first from no memory for the size, then from the arena.
    const uint64_t room = std::max(std::max(sr_scan_room(S), sr_scan_room(V)), sr_scan_room(E));
    uint32_t *d_len, *d_steps, *d_poff, *d_efrom, *d_eto, *d_roff, *d_added;
    u64d *d_rstart, *d_rpmax, *d_sums;
    ExDev d;
    d.V = V; d.S = S; d.P = P; d.E = E;
    auto carve = [&](ExArena a) {
        d.len = d_len = a.take<uint32_t>(V); d.steps = d_steps = a.take<uint32_t>(S); d.path_off = d_poff = a.take<uint32_t>((uint64_t)P + 1);
        d.efrom = d_efrom = a.take<uint32_t>(E); d.eto = d_eto = a.take<uint32_t>(E); d.reg_off = d_roff = a.take<uint32_t>((uint64_t)P + 1);
        d.reg_start = d_rstart = a.take<u64d>(N); d.reg_pmax = d_rpmax = a.take<u64d>(N); d_sums = a.take<u64d>(room);
        d_added = a.take<uint32_t>(SR_EXTRACT_MAX_ROUNDS);                // one word per round
        d.sinc = a.take<u64d>(S); d.pstart = a.take<u64d>(S); d.spath = a.take<uint32_t>(S);
        d.level = a.take<uint32_t>(V);
        d.fwd = a.take<u64d>(S); d.bwd = a.take<u64d>(S);
        d.nnode = a.take<u64d>(V); d.nedge = a.take<u64d>(E); d.nrun = a.take<u64d>(S); d.nstep = a.take<u64d>(S);
        // the outputs at their worst case
        d.o_node_old = a.take<uint32_t>(V); d.o_efrom = a.take<uint32_t>(E); d.o_eto = a.take<uint32_t>(E);
        d.o_sub_path = a.take<uint32_t>(S); d.o_sub_steps = a.take<uint32_t>(S);
        d.o_sub_start = a.take<u64d>(S); d.o_sub_end = a.take<u64d>(S); d.o_sub_off = a.take<u64d>(S);
        return a.at;
    };
    const uint64_t bytes = carve(ExArena{0, 0});
    char *arena = x.alloc<char>(bytes);
    if (x.err) return x.err;
    carve(ExArena{(uintptr_t)arena, 0});
    x.chk(hipMemsetAsync(d.level, 0xff, (size_t)V * 4, x.st));
    if (!x.err) x.chk(hipMemsetAsync(d_added, 0, SR_EXTRACT_MAX_ROUNDS * 4, x.st));
    x.put(d_len, t.len.data(), (size_t)V * 4); x.put(d_steps, t.steps.data(), (size_t)S * 4); x.put(d_poff, t.path_off.data(), ((size_t)P + 1) * 4);
    x.put(d_efrom, t.efrom.data(), (size_t)E * 4); x.put(d_eto, t.eto.data(), (size_t)E * 4); x.put(d_roff, reg_off.data(), ((size_t)P + 1) * 4);
    x.put(d_rstart, reg_start.data(), (size_t)N * 8); x.put(d_rpmax, reg_pmax.data(), (size_t)N * 8);

    x.mark(0);                                                   // ---- positions
    sr_step_len(x, d.steps, d.len, S, d.sinc);
    sr_scan<false>(x, d.sinc, S, d_sums);
    ex_launch(x, ex_pstart_kernel, S, d);
    x.mark(1);                                                   // ---- seeds
    ex_launch(x, ex_seed_kernel, S, d);
    x.mark(2);                                                   // ---- context: every round is a launch
    for (uint32_t r = 1; r <= t.c && E; r++) ex_launch(x, ex_context_kernel, E, d, r);
    x.mark(3);                                                   // ---- merge: a synchronisation per round, for the word
    for (uint64_t k = 1; k <= t.R && !x.err; k++) {
        ex_launch(x, ex_kept_kernel, S, d);
        sr_scan<true>(x, d.fwd, S, d_sums);
        sr_scan<true>(x, d.bwd, S, d_sums);
        ex_launch(x, ex_gap_kernel, S, d, (u64d)t.D, (uint32_t)(t.c + k), d_added + (k - 1));
        uint32_t added = 0;
        x.get(&added, d_added + (k - 1), 4);
        x.sync();
        if (x.err || !added) break;
        o.rounds_run++;
    }
    x.mark(4);                                                   // ---- numbering
    ex_launch(x, ex_flag_node_kernel, V, d);
    ex_launch(x, ex_flag_edge_kernel, E, d);
    ex_launch(x, ex_flag_step_kernel, S, d);
    sr_scan<false>(x, d.nnode, V, d_sums);
    sr_scan<false>(x, d.nedge, E, d_sums);
    sr_scan<false>(x, d.nrun, S, d_sums);
    sr_scan<false>(x, d.nstep, S, d_sums);
    x.mark(5);                                                   // ---- emission
    ex_launch(x, ex_emit_node_kernel, V, d);
    ex_launch(x, ex_emit_edge_kernel, E, d);
    ex_launch(x, ex_emit_step_kernel, S, d);
    x.mark(6);
    x.chk(hipGetLastError());
    uint64_t n_nodes = 0, n_edges = 0, n_sub = 0, n_steps = 0;   // the four counts, then exactly that much
    x.get(&n_nodes, d.nnode + (V - 1), 8); x.get(&n_sub, d.nrun + (S - 1), 8); x.get(&n_steps, d.nstep + (S - 1), 8);
    if (E) x.get(&n_edges, d.nedge + (E - 1), 8);
    x.sync();
    if (x.err) return x.err;
    if (n_nodes > V || n_edges > E || n_sub > S || n_steps > S) return sr_fail(SR_ERR_DEVICE_FAULT, "extract: a count exceeds its table");
    o.node_old.resize(n_nodes); o.edge_from.resize(n_edges); o.edge_to.resize(n_edges);
    o.sub_path.resize(n_sub); o.sub_start.resize(n_sub); o.sub_end.resize(n_sub); o.sub_off.assign(n_sub + 1, n_steps); o.sub_steps.resize(n_steps);
    x.get(o.level.data(), d.level, (size_t)V * 4); x.get(o.node_old.data(), d.o_node_old, (size_t)n_nodes * 4);
    x.get(o.edge_from.data(), d.o_efrom, (size_t)n_edges * 4); x.get(o.edge_to.data(), d.o_eto, (size_t)n_edges * 4);
    x.get(o.sub_path.data(), d.o_sub_path, (size_t)n_sub * 4); x.get(o.sub_start.data(), d.o_sub_start, (size_t)n_sub * 8);
    x.get(o.sub_end.data(), d.o_sub_end, (size_t)n_sub * 8); x.get(o.sub_off.data(), d.o_sub_off, (size_t)n_sub * 8);
    x.get(o.sub_steps.data(), d.o_sub_steps, (size_t)n_steps * 4);
    x.sync();                                                    // the synchronisation after the download
    if (x.err) return x.err;
    o.us = x.us(0, 6);
    for (int k = 0; k < 6; k++) o.kernel_us[k] = x.us(k, k + 1);
    return x.err;
}

void ex_free_tables(sr_extract *r) {
    free(r->level); free(r->node_old); free(r->edge_from); free(r->edge_to); free(r->sub_path); free(r->sub_start); free(r->sub_end);
    free(r->sub_off); free(r->sub_steps);
    delete (ExPriv *)r->priv;
    free(r);
}

template <class T> T *ex_copy(const std::vector<T> &v, bool *ok) {
    T *p = (T *)calloc(v.size() ? v.size() : 1, sizeof(T));
    if (!p) { *ok = false; return nullptr; }
    if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

sr_extract *ex_result(const ExTables &t, const ExOut &o, const SrGraph &g, const std::vector<std::string> &names) {
    sr_extract *r = (sr_extract *)calloc(1, sizeof(sr_extract));
    if (!r) return nullptr;
    r->regions = t.r_path.size(); r->unknown = t.unknown; r->out_of_range = t.out_of_range;
    r->in_nodes = t.V; r->in_edges = t.E; r->in_steps = t.S; r->in_paths = t.P;
    r->nodes = o.node_old.size(); r->edges = o.edge_from.size(); r->subpaths = o.sub_path.size(); r->steps = o.sub_steps.size();
    r->merge_rounds_run = o.rounds_run; r->variant = o.variant; r->extract_us = o.us;
    for (int k = 0; k < 6; k++) r->kernel_us[k] = o.kernel_us[k];
    for (uint32_t v = 0; v < t.V; v++) {
        const uint32_t l = o.level[v];
        if (l == SR_EXTRACT_NONE) continue;
        r->bases += t.len[v];
        if (l == 0) r->seeds++; else if (l <= t.c) r->by_context++; else r->by_merge++;
    }
    bool ok = true;
    r->level = ex_copy(o.level, &ok); r->node_old = ex_copy(o.node_old, &ok); r->edge_from = ex_copy(o.edge_from, &ok); r->edge_to = ex_copy(o.edge_to, &ok);
    r->sub_path = ex_copy(o.sub_path, &ok); r->sub_start = ex_copy(o.sub_start, &ok); r->sub_end = ex_copy(o.sub_end, &ok);
    r->sub_off = ex_copy(o.sub_off, &ok); r->sub_steps = ex_copy(o.sub_steps, &ok);
    ExPriv *pv = new (std::nothrow) ExPriv;
    r->priv = pv;
    if (!ok || !pv) { ex_free_tables(r); return nullptr; }
    pv->names.assign(names.begin(), names.begin() + std::min<size_t>(names.size(), t.P));
    pv->names.resize(t.P);
    pv->seq.reserve(o.node_old.size());
    for (uint32_t old : o.node_old) pv->seq.push_back(g.node_seq[old]);
    return r;
}

}   // namespace

extern "C" void sr_extract_params_default(sr_extract_params *p) {
    if (!p) return;
    p->context_steps = 0; p->merge_distance = 100000; p->merge_rounds = 3; p->reserved = 0;
}

extern "C" int sr_extract_gfa(const char *gfa_in, const char *bed_text, const char *const *regions, uint64_t n_regions,
                              const sr_extract_params *p, int device, sr_extract **out) {
    if (!gfa_in || !p || !out || (n_regions && !regions)) return sr_fail(SR_ERR_INVALID, "null argument");
    *out = nullptr;
    if (device < SR_EXTRACT_DEVICE_HOST) return sr_fail(SR_ERR_INVALID, "extract: device must be >= -1");
    try {
        SrGraph g;
        std::vector<std::string> names;
        int r = sr_graph_parse_gfa(gfa_in, g, names);
        if (r) return r;
        ExTables t;
        if ((r = ex_tables(g, *p, t))) return r;
        if ((r = ex_regions(bed_text, regions, n_regions, names, t))) return r;
        ExOut o;
        if ((r = device < 0 ? ex_run_host(t, o) : ex_run_device(t, device, nullptr, o))) return r;
        sr_extract *res = ex_result(t, o, g, names);
        if (!res) return sr_fail(SR_ERR_NOMEM, "not enough memory for the extract tables");
        *out = res;
    } catch (const std::bad_alloc &) {
        return sr_fail(SR_ERR_NOMEM, "not enough memory for the extract tables");
    }
    return SR_OK;
}

extern "C" void sr_extract_free(sr_extract *x) {
    if (x) ex_free_tables(x);
}

extern "C" int sr_extract_text(const sr_extract *x, char **gfa) {
    if (!x || !gfa || !x->priv) return sr_fail(SR_ERR_INVALID, "null argument");
    const ExPriv &pv = *(const ExPriv *)x->priv;
    const char *bad = "extract: not a result of sr_extract_gfa";
    if (pv.seq.size() != x->nodes || pv.names.size() != x->in_paths || x->sub_off[x->subpaths] != x->steps) return sr_fail(SR_ERR_INVALID, bad);
    try {
        SrGraph g;
        g.node_seq.assign(1, std::string());
        g.node_seq.insert(g.node_seq.end(), pv.seq.begin(), pv.seq.end());
        g.node_alive.assign(x->nodes + 1, 1);
        g.node_alive[0] = 0;
        for (uint64_t e = 0; e < x->edges; e++) g.edges.push_back({x->edge_from[e], x->edge_to[e]});
        g.steps.assign(x->sub_steps, x->sub_steps + x->steps);
        g.path_off.assign(x->sub_off, x->sub_off + x->subpaths + 1);
        std::vector<std::string> names(x->subpaths);
        std::vector<const char *> cn(x->subpaths ? x->subpaths : 1, nullptr);
        for (uint64_t j = 0; j < x->subpaths; j++) {
            if (x->sub_path[j] >= x->in_paths) return sr_fail(SR_ERR_INVALID, bad);
            names[j] = pv.names[x->sub_path[j]] + ":" + u64s(x->sub_start[j]) + "-" + u64s(x->sub_end[j]);
            cn[j] = names[j].c_str();
        }
        char *text = sr_graph_format_gfa(g, cn.data(), nullptr, nullptr);
        if (!text) return sr_fail(SR_ERR_NOMEM, "not enough memory for the extracted graph");
        *gfa = text;
    } catch (const std::bad_alloc &) {
        return sr_fail(SR_ERR_NOMEM, "not enough memory for the extracted graph");
    }
    return SR_OK;
}
