// sr_stats.hip -- the statistics stage (--stats; include/seqrush_amd.h "graph statistics"): exact
// integer reductions over the tables of a parsed GFA (node lengths, steps, path offsets, edges), on the device and, in
// plain loops over the same tables, on the host.  Every output is an integer, so the two agree exactly.
//
// Device: five groups of kernels on one stream, hipEvents between them, one synchronisation before the results are
// read.  steps -> depth, rev_steps and the node-major path bitset B[node][ceil(P / 64)];  nodes -> paths_on, length,
// depth_bp and the two histograms (privatised in LDS);  similarity -> B^T diag(len) B by 64 x 64 path tiles, one wave and
// one 32 KiB LDS accumulator per (tile pair, node chunk);  layout -> per-path error sums by a segmented wave reduction;
// topology -> side flags, self loops, union-find (sr_uf_dev.h), tips and roots.  No captured graph.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/seqrush_amd.h"
#include "sr_internal.h"
#include "sr_sort.h"
#include "sr_stage_host.h"
#include "sr_stage_dev.h"
#include "sr_uf_dev.h"
#include "sr_stats_rule.h"

#define ST_BLOCK 256
enum { ST_LENGTH = 0, ST_DEPTH_BP, ST_REV, ST_LOOPS, ST_TIPS, ST_ROOTS, ST_ERR, ST_NSC };
enum { LY_PAIRS = 0, LY_ABS, LY_LEN, LY_HH, LY_HL, LY_LL, LY_N };

typedef unsigned long long u64d;

// ------------------------------------------------------------------ device helpers
__device__ __forceinline__ u64d st_wave_sum(u64d v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;                                        // lane 0 holds the wave's sum
}

// ------------------------------------------------------------------ steps
__global__ void __launch_bounds__(ST_BLOCK) st_steps_kernel(const uint32_t *steps, uint32_t S, const uint32_t *path_off, uint32_t np,
                                                            uint32_t W, uint32_t *depth, u64d *bits, u64d *sc) {
    const uint32_t stride = gridDim.x * ST_BLOCK;
    u64d rev = 0;
    for (uint64_t s = (uint64_t)blockIdx.x * ST_BLOCK + threadIdx.x; s < S; s += stride) {
        const uint32_t h = steps[s], node = h >> 1;
        const uint32_t p = sr_path_of(path_off, np, (uint32_t)s);
        atomicAdd(&depth[node], 1u);
        atomicOr(&bits[(uint64_t)node * W + (p >> 6)], 1ULL << (p & 63u));
        rev += h & 1u;
    }
    rev = st_wave_sum(rev);
    if ((threadIdx.x & 63) == 0 && rev) atomicAdd(&sc[ST_REV], rev);
}

// ------------------------------------------------------------------ nodes
// dynamic LDS: (np + 1) u64 base-pair bins, then (np + 1) u32 node bins (a workgroup sees fewer than 2^32 nodes)
__global__ void __launch_bounds__(ST_BLOCK) st_nodes_kernel(const uint32_t *len, uint32_t V, uint32_t W, const u64d *bits,
                                                            const uint32_t *depth, uint32_t np, uint32_t *paths_on, u64d *hist_bp,
                                                            u64d *hist_nodes, u64d *sc) {
    extern __shared__ u64d st_lds[];
    u64d *lbp = st_lds;
    uint32_t *ln = (uint32_t *)(st_lds + np + 1);
    for (uint32_t i = threadIdx.x; i <= np; i += ST_BLOCK) { lbp[i] = 0; ln[i] = 0; }
    __syncthreads();
    const uint32_t stride = gridDim.x * ST_BLOCK;
    u64d length = 0, dbp = 0;
    for (uint64_t v = 1 + (uint64_t)blockIdx.x * ST_BLOCK + threadIdx.x; v <= V; v += stride) {
        uint32_t c = 0;
        for (uint32_t w = 0; w < W; w++) c += (uint32_t)__popcll(bits[v * W + w]);
        paths_on[v] = c;
        const u64d l = len[v];
        atomicAdd(&lbp[c], l);
        atomicAdd(&ln[c], 1u);
        length += l;
        dbp += l * depth[v];
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i <= np; i += ST_BLOCK)
        if (ln[i]) { atomicAdd(&hist_bp[i], lbp[i]); atomicAdd(&hist_nodes[i], (u64d)ln[i]); }
    length = st_wave_sum(length);
    dbp = st_wave_sum(dbp);
    if ((threadIdx.x & 63) == 0) {
        if (length) atomicAdd(&sc[ST_LENGTH], length);
        if (dbp) atomicAdd(&sc[ST_DEPTH_BP], dbp);
    }
}

// ------------------------------------------------------------------ similarity
// grid (node chunks, tile pairs ti <= tj); one wave per workgroup.  acc[a][b]: lane b owns column b, so no two lanes ever
// touch one cell and a row access is conflict-free.  64 nodes are loaded at a time, one per lane; the nodes whose two
// words are both non-zero are then visited one after the other, their words handed round by shuffles.  The row updates
// are LDS adds without a return value: the wave issues them back to back instead of waiting for a read each time (the
// read-add-write form ran at one row per LDS round trip and lost to the host twin on 64 paths).  One wave issues a row
// update every ~100 cycles, so the chunk is small: what hides that is many waves, not a long loop in one.
__global__ void __launch_bounds__(SR_STATS_TILE) st_sim_kernel(const uint32_t *len, uint32_t V, uint32_t W, const u64d *bits,
                                                               uint32_t np, uint32_t T, u64d *shared) {
    __shared__ u64d acc[SR_STATS_TILE * SR_STATS_TILE];
    const uint32_t lane = threadIdx.x;
    uint32_t tp = blockIdx.y, ti = 0;
    while (tp >= T - ti) { tp -= T - ti; ti++; }     // row ti of the upper triangle holds T - ti pairs
    const uint32_t tj = ti + tp;
#pragma unroll 8
    for (uint32_t a = 0; a < SR_STATS_TILE; a++) acc[a * SR_STATS_TILE + lane] = 0;
    const uint64_t v0 = 1 + (uint64_t)blockIdx.x * SR_STATS_CHUNK;
    const uint64_t v1 = v0 + SR_STATS_CHUNK < (uint64_t)V + 1 ? v0 + SR_STATS_CHUNK : (uint64_t)V + 1;
    u64d touched = 0;
    for (uint64_t base = v0; base < v1; base += SR_STATS_TILE) {
        const uint64_t v = base + lane;
        u64d wi = 0, wj = 0;
        uint32_t l = 0;
        if (v < v1) {
            wi = bits[v * W + ti];
            wj = ti == tj ? wi : bits[v * W + tj];
            l = len[v];
        }
        u64d live = __ballot(wi != 0 && wj != 0);
        touched |= live;
        while (live) {
            const int k = __ffsll(live) - 1;
            live &= live - 1;
            const u64d kwi = __shfl(wi, k, 64), kwj = __shfl(wj, k, 64);
            const u64d kl = __shfl(l, k, 64);
            if ((kwj >> lane) & 1ULL) {
                u64d m = kwi;                        // wave-uniform
                while (m) {
                    const int a = __ffsll(m) - 1;
                    m &= m - 1;
                    atomicAdd(&acc[a * SR_STATS_TILE + lane], kl);   // result unused: an LDS add the wave does not wait for
                }
            }
        }
    }
    if (!touched) return;                            // wave-uniform: no node of the chunk lies on both tiles
    const uint64_t j = (uint64_t)tj * SR_STATS_TILE + lane;
    for (uint32_t a = 0; a < SR_STATS_TILE; a++) {
        const u64d c = acc[a * SR_STATS_TILE + lane];
        const uint64_t i = (uint64_t)ti * SR_STATS_TILE + a;
        if (c && i < np && j < np) atomicAdd(&shared[i * np + j], c);
    }
}

// ------------------------------------------------------------------ layout
// one lane per step s; lane s owns the pair (s, s + 1) when both lie in one path.  Paths ascend with s, so a wave holds
// runs of equal paths: a segmented reduction by shuffles leaves each run's sums in its first lane, which adds them to
// the path's six sums -- at most one set of adds per path and wave.
__global__ void __launch_bounds__(ST_BLOCK) st_layout_kernel(const uint32_t *steps, uint32_t S, const uint32_t *path_off, uint32_t np,
                                                             const uint32_t *len, const uint32_t *pos, u64d *per_path) {
    const uint64_t s = (uint64_t)blockIdx.x * ST_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63;
    uint32_t p = np;                                 // past the end: sorts after every path, owns nothing
    u64d val[LY_N];
#pragma unroll
    for (int k = 0; k < LY_N; k++) val[k] = 0;
    if (s < S) {
        p = sr_path_of(path_off, np, (uint32_t)s);
        if (s + 1 < path_off[p + 1]) {
            const uint32_t a = steps[s] >> 1, b = steps[s + 1] >> 1;
            const uint64_t e = sr_stats_pair_error(pos[a], pos[b], len[a]);
            uint64_t hh, hl, ll;
            sr_stats_sq_split(e, &hh, &hl, &ll);
            val[LY_PAIRS] = 1; val[LY_ABS] = e; val[LY_LEN] = len[a]; val[LY_HH] = hh; val[LY_HL] = hl; val[LY_LL] = ll;
        }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t op = __shfl_down(p, o, 64);
        const bool take = lane + o < 64 && op == p;
#pragma unroll
        for (int k = 0; k < LY_N; k++) {
            const u64d ov = __shfl_down(val[k], o, 64);
            if (take) val[k] += ov;
        }
    }
    const uint32_t prev = __shfl_up(p, 1, 64);
    if ((lane == 0 || prev != p) && p < np && val[LY_PAIRS]) {
#pragma unroll
        for (int k = 0; k < LY_N; k++) atomicAdd(&per_path[(uint64_t)p * LY_N + k], val[k]);
    }
}

// ------------------------------------------------------------------ topology
__global__ void __launch_bounds__(ST_BLOCK) st_uf_init_kernel(u64d *uf, uint64_t n) {
    const uint64_t stride = (uint64_t)gridDim.x * ST_BLOCK;
    for (uint64_t i = (uint64_t)blockIdx.x * ST_BLOCK + threadIdx.x; i < n; i += stride) uf[i] = i;   // own parent, rank 0
}
__global__ void __launch_bounds__(ST_BLOCK) st_edges_kernel(const u64d *edges, uint32_t E, uint8_t *side, u64d *uf, u64d *sc) {
    const uint32_t stride = gridDim.x * ST_BLOCK;
    u64d loops = 0;
    int err = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * ST_BLOCK + threadIdx.x; i < E; i += stride) {
        const u64d e = edges[i];
        const uint32_t a = (uint32_t)(e >> 32), b = (uint32_t)e;
        side[sr_stats_side_from(a)] = 1;
        side[sr_stats_side_to(b)] = 1;
        if ((a >> 1) == (b >> 1)) loops++;
        else uf_unite(uf, a >> 1, b >> 1, err);
    }
    if (err) atomicOr(&sc[ST_ERR], (u64d)err);
    loops = st_wave_sum(loops);
    if ((threadIdx.x & 63) == 0 && loops) atomicAdd(&sc[ST_LOOPS], loops);
}
__global__ void __launch_bounds__(ST_BLOCK) st_count_kernel(uint32_t V, const uint8_t *side, u64d *uf, u64d *sc) {
    const uint32_t stride = gridDim.x * ST_BLOCK;
    u64d tips = 0, roots = 0;
    for (uint64_t v = 1 + (uint64_t)blockIdx.x * ST_BLOCK + threadIdx.x; v <= V; v += stride) {
        tips += (side[2 * v] ? 0u : 1u) + (side[2 * v + 1] ? 0u : 1u);
        if ((uf_load(uf, v) & UF_PARENT_MASK) == v) roots++;
    }
    tips = st_wave_sum(tips);
    roots = st_wave_sum(roots);
    if ((threadIdx.x & 63) == 0) {
        if (tips) atomicAdd(&sc[ST_TIPS], tips);
        if (roots) atomicAdd(&sc[ST_ROOTS], roots);
    }
}

namespace {

// the tables both executions read: node v = 1..V at index v, slot 0 unused (length 0)
struct StTables : SrPathTables {
    uint32_t E = 0, W = 0;
    std::vector<u64d> edges;
};

int st_tables(const SrGraph &g, StTables &t) {
    const SrPathSizes z = sr_path_sizes(g);
    const uint64_t nn = z.nodes, ne = z.edges, np = z.paths;
    if (np > SR_STATS_MAX_PATHS)
        return sr_fail(SR_ERR_UNSUPPORTED, "stats: " + std::to_string(np) + " paths; the path bitset and the similarity matrix support at most " +
                                               std::to_string(SR_STATS_MAX_PATHS));
    if (nn >= 0x3fffffffULL || z.steps >= 0x7fffffffULL || ne >= 0x7fffffffULL || z.bases >= 0x7fffffffULL)
        return sr_fail(SR_ERR_UNSUPPORTED, "stats supports < 2^30 nodes and < 2^31 steps, edges and bases");
    t.E = (uint32_t)ne; t.W = (uint32_t)((np + 63) / 64);
    if (t.W == 0) t.W = 1;
    if (const int r = sr_path_tables_fill(g, z, "stats", false, true, t)) return r;
    t.edges.resize(ne);
    for (uint64_t i = 0; i < ne; i++) {
        const uint32_t a = g.edges[i].first, b = g.edges[i].second;
        if ((a >> 1) == 0 || (a >> 1) > nn || (b >> 1) == 0 || (b >> 1) > nn) return sr_fail(SR_ERR_INVALID, "stats: an edge names a missing node");
        t.edges[i] = ((u64d)a << 32) | b;
    }
    return SR_OK;
}

template <class Tp> Tp *st_calloc(uint64_t n) { return (Tp *)calloc(n ? n : 1, sizeof(Tp)); }

sr_graph_stats *st_result(const StTables &t) {
    sr_graph_stats *r = st_calloc<sr_graph_stats>(1);
    if (!r) return nullptr;
    r->nodes = t.V; r->edges = t.E; r->paths = t.P; r->steps = t.S;
    r->depth = st_calloc<uint32_t>(t.V); r->paths_on = st_calloc<uint32_t>(t.V);
    r->bp_by_paths = st_calloc<uint64_t>((uint64_t)t.P + 1); r->nodes_by_paths = st_calloc<uint64_t>((uint64_t)t.P + 1);
    r->shared = st_calloc<uint64_t>((uint64_t)t.P * t.P);
    r->path_pairs = st_calloc<uint64_t>(t.P); r->path_abs = st_calloc<uint64_t>(t.P); r->path_len = st_calloc<uint64_t>(t.P);
    r->path_sq = st_calloc<uint64_t>((uint64_t)t.P * 3);
    if (!r->depth || !r->paths_on || !r->bp_by_paths || !r->nodes_by_paths || !r->shared || !r->path_pairs || !r->path_abs ||
        !r->path_len || !r->path_sq) { sr_graph_stats_free(r); return nullptr; }
    return r;
}

// the totals and the lower triangle follow from the per-path sums and the upper triangle on the host, for both executions
void st_finish(sr_graph_stats *r) {
    const uint64_t P = r->paths;
    for (uint64_t i = 0; i < P; i++)
        for (uint64_t j = i + 1; j < P; j++) r->shared[j * P + i] = r->shared[i * P + j];
    r->total_pairs = r->total_abs = r->total_len = 0;
    r->total_sq[0] = r->total_sq[1] = r->total_sq[2] = 0;
    for (uint64_t p = 0; p < P; p++) {
        r->total_pairs += r->path_pairs[p]; r->total_abs += r->path_abs[p]; r->total_len += r->path_len[p];
        for (int k = 0; k < 3; k++) r->total_sq[k] += r->path_sq[p * 3 + k];
    }
}

// ------------------------------------------------------------------ host twin: plain loops in table order
uint32_t host_find(std::vector<uint32_t> &par, uint32_t x) {
    while (par[x] != x) { par[x] = par[par[x]]; x = par[x]; }
    return x;
}

void st_run_host(const StTables &t, sr_graph_stats *r) {
    const uint32_t V = t.V, P = t.P, W = t.W;
    auto t0 = std::chrono::steady_clock::now();
    const auto t_all = t0;
    auto lap = [&](int k) { r->kernel_us[k] = (uint64_t)(us_since(t0) + 0.5); t0 = std::chrono::steady_clock::now(); };
    std::vector<uint64_t> bits((uint64_t)(V + 1) * W, 0);
    std::vector<uint32_t> depth(V + 1, 0);
    for (uint32_t p = 0; p < P; p++)
        for (uint32_t s = t.path_off[p]; s < t.path_off[p + 1]; s++) {
            const uint32_t h = t.steps[s];
            depth[h >> 1]++;
            bits[(uint64_t)(h >> 1) * W + (p >> 6)] |= 1ULL << (p & 63u);
            r->rev_steps += h & 1u;
        }
    lap(0);
    for (uint32_t v = 1; v <= V; v++) {
        uint32_t c = 0;
        for (uint32_t w = 0; w < W; w++) c += (uint32_t)__builtin_popcountll(bits[(uint64_t)v * W + w]);
        r->depth[v - 1] = depth[v]; r->paths_on[v - 1] = c;
        r->bp_by_paths[c] += t.len[v]; r->nodes_by_paths[c]++;
        r->length += t.len[v];
        r->depth_bp += (uint64_t)t.len[v] * depth[v];
    }
    lap(1);
    std::vector<uint32_t> on;
    for (uint32_t v = 1; v <= V; v++) {
        on.clear();
        for (uint32_t w = 0; w < W; w++)
            for (uint64_t m = bits[(uint64_t)v * W + w]; m; m &= m - 1) on.push_back(w * 64 + (uint32_t)__builtin_ctzll(m));
        const uint64_t l = t.len[v];
        for (size_t x = 0; x < on.size(); x++)
            for (size_t y = x; y < on.size(); y++) r->shared[(uint64_t)on[x] * P + on[y]] += l;
    }
    lap(2);
    std::vector<uint64_t> pos(V + 1, 0);
    for (uint32_t v = 1; v <= V; v++) pos[v] = pos[v - 1] + t.len[v - 1];
    for (uint32_t p = 0; p < P; p++)
        for (uint32_t s = t.path_off[p]; s + 1 < t.path_off[p + 1]; s++) {
            const uint32_t a = t.steps[s] >> 1, b = t.steps[s + 1] >> 1;
            const uint64_t e = sr_stats_pair_error(pos[a], pos[b], t.len[a]);
            uint64_t hh, hl, ll;
            sr_stats_sq_split(e, &hh, &hl, &ll);
            r->path_pairs[p]++; r->path_abs[p] += e; r->path_len[p] += t.len[a];
            r->path_sq[p * 3] += hh; r->path_sq[p * 3 + 1] += hl; r->path_sq[p * 3 + 2] += ll;
        }
    lap(3);
    std::vector<uint8_t> side(2 * ((uint64_t)V + 1), 0);
    std::vector<uint32_t> par(V + 1);
    for (uint32_t v = 0; v <= V; v++) par[v] = v;
    for (uint32_t i = 0; i < t.E; i++) {
        const uint32_t a = (uint32_t)(t.edges[i] >> 32), b = (uint32_t)t.edges[i];
        side[sr_stats_side_from(a)] = 1;
        side[sr_stats_side_to(b)] = 1;
        if ((a >> 1) == (b >> 1)) { r->self_loops++; continue; }
        const uint32_t x = host_find(par, a >> 1), y = host_find(par, b >> 1);
        if (x != y) par[x < y ? y : x] = x < y ? x : y;
    }
    for (uint32_t v = 1; v <= V; v++) {
        r->tips += (side[2 * (uint64_t)v] ? 0u : 1u) + (side[2 * (uint64_t)v + 1] ? 0u : 1u);
        if (par[v] == v) r->components++;
    }
    lap(4);
    r->stats_us = (uint64_t)(us_since(t_all) + 0.5);
}

// ------------------------------------------------------------------ device execution
unsigned st_grid(uint64_t n) {
    uint64_t b = (n + ST_BLOCK - 1) / ST_BLOCK;
    return (unsigned)(b > 8192 ? 8192 : (b ? b : 1));
}

int st_run_device(const StTables &t, int device, void *stream, sr_graph_stats *r) {
    const uint32_t V = t.V, S = t.S, E = t.E, P = t.P, W = t.W;
    SrStage x("stats", "the statistics stage");
    if (x.open(device, stream, 6)) return x.err;

    const uint64_t nv = (uint64_t)V + 1;
    uint32_t *d_len = x.alloc<uint32_t>(nv), *d_pos = x.alloc<uint32_t>(nv, 0), *d_steps = x.alloc<uint32_t>(S);
    uint32_t *d_poff = x.alloc<uint32_t>((uint64_t)P + 1), *d_depth = x.alloc<uint32_t>(nv, 0), *d_pon = x.alloc<uint32_t>(nv, 0);
    uint32_t *d_tile = x.alloc<uint32_t>(nv / 1024 + 2), *d_grand = x.alloc<uint32_t>(1, 0);
    u64d *d_edges = x.alloc<u64d>(E), *d_bits = x.alloc<u64d>(nv * W, 0), *d_sc = x.alloc<u64d>(ST_NSC, 0);
    u64d *d_hbp = x.alloc<u64d>((uint64_t)P + 1, 0), *d_hn = x.alloc<u64d>((uint64_t)P + 1, 0);
    u64d *d_shared = x.alloc<u64d>((uint64_t)P * P, 0), *d_pp = x.alloc<u64d>((uint64_t)P * LY_N, 0), *d_uf = x.alloc<u64d>(nv);
    uint8_t *d_side = x.alloc<uint8_t>(2 * nv, 0);
    if (x.err) return x.err;
    x.put(d_len, t.len.data(), nv * 4); x.put(d_steps, t.steps.data(), (size_t)S * 4); x.put(d_poff, t.path_off.data(), ((size_t)P + 1) * 4);
    x.put(d_edges, t.edges.data(), (size_t)E * 8);

    x.mark(0);
    if (S) hipLaunchKernelGGL(st_steps_kernel, dim3(st_grid(S)), dim3(ST_BLOCK), 0, x.st, d_steps, S, d_poff, P, W, d_depth, d_bits, d_sc);
    x.mark(1);
    if (V) hipLaunchKernelGGL(st_nodes_kernel, dim3(st_grid(V)), dim3(ST_BLOCK), ((size_t)P + 1) * 12 + 8, x.st, d_len, V, W, d_bits, d_depth, P,
                              d_pon, d_hbp, d_hn, d_sc);
    x.mark(2);
    if (V && P) {
        const uint32_t T = (P + SR_STATS_TILE - 1) / SR_STATS_TILE;
        const uint64_t chunks = ((uint64_t)V + SR_STATS_CHUNK - 1) / SR_STATS_CHUNK;
        hipLaunchKernelGGL(st_sim_kernel, dim3((unsigned)chunks, T * (T + 1) / 2), dim3(SR_STATS_TILE), 0, x.st, d_len, V, W, d_bits, P, T, d_shared);
    }
    x.mark(3);
    if (V && !x.err && srk_scan_u32(d_len, nv, d_pos, d_tile, d_grand, x.st)) x.chk(hipErrorLaunchFailure);
    if (S && P) hipLaunchKernelGGL(st_layout_kernel, dim3((unsigned)(((uint64_t)S + ST_BLOCK - 1) / ST_BLOCK)), dim3(ST_BLOCK), 0, x.st, d_steps, S,
                                   d_poff, P, d_len, d_pos, d_pp);
    x.mark(4);
    if (V) {
        hipLaunchKernelGGL(st_uf_init_kernel, dim3(st_grid(nv)), dim3(ST_BLOCK), 0, x.st, d_uf, nv);
        if (E) hipLaunchKernelGGL(st_edges_kernel, dim3(st_grid(E)), dim3(ST_BLOCK), 0, x.st, d_edges, E, d_side, d_uf, d_sc);
        hipLaunchKernelGGL(st_count_kernel, dim3(st_grid(V)), dim3(ST_BLOCK), 0, x.st, V, d_side, d_uf, d_sc);
    }
    x.mark(5);
    x.chk(hipGetLastError());

    u64d sc[ST_NSC] = {0};
    std::vector<u64d> pp((uint64_t)P * LY_N, 0);
    x.get(sc, d_sc, sizeof sc);
    if (V) { x.get(r->depth, d_depth + 1, (size_t)V * 4); x.get(r->paths_on, d_pon + 1, (size_t)V * 4); }
    x.get(r->bp_by_paths, d_hbp, ((size_t)P + 1) * 8); x.get(r->nodes_by_paths, d_hn, ((size_t)P + 1) * 8);
    x.get(r->shared, d_shared, (size_t)P * P * 8); x.get(pp.data(), d_pp, pp.size() * 8);
    x.sync();                                        // the one synchronisation
    if (x.err) return x.err;
    if (sc[ST_ERR]) return sr_fail(SR_ERR_DEVICE_FAULT, "stats: union-find retry bound hit");
    r->length = sc[ST_LENGTH]; r->depth_bp = sc[ST_DEPTH_BP]; r->rev_steps = sc[ST_REV]; r->self_loops = sc[ST_LOOPS];
    r->tips = sc[ST_TIPS]; r->components = sc[ST_ROOTS];
    for (uint32_t p = 0; p < P; p++) {
        r->path_pairs[p] = pp[(uint64_t)p * LY_N + LY_PAIRS]; r->path_abs[p] = pp[(uint64_t)p * LY_N + LY_ABS];
        r->path_len[p] = pp[(uint64_t)p * LY_N + LY_LEN];
        r->path_sq[p * 3] = pp[(uint64_t)p * LY_N + LY_HH]; r->path_sq[p * 3 + 1] = pp[(uint64_t)p * LY_N + LY_HL];
        r->path_sq[p * 3 + 2] = pp[(uint64_t)p * LY_N + LY_LL];
    }
    r->stats_us = x.us(0, 5);
    for (int k = 0; k < 5; k++) r->kernel_us[k] = x.us(k, k + 1);
    return x.err;
}

// ------------------------------------------------------------------ report
std::string u128_dec(unsigned __int128 v) {
    if (v == 0) return "0";
    std::string s;
    while (v) { s.insert(s.begin(), (char)('0' + (int)(v % 10))); v /= 10; }
    return s;
}
unsigned __int128 sq_join(const uint64_t sq[3]) {
    return ((unsigned __int128)sq[0] << 32) + ((unsigned __int128)sq[1] << 17) + (unsigned __int128)sq[2];
}
std::string ratio(double num, double den, double scale = 1.0) {
    if (!(den > 0)) return "NA";
    char buf[64];
    snprintf(buf, sizeof buf, "%.6f", num / den * scale);
    return buf;
}

}   // namespace

int sr_graph_stats_run(const SrGraph &g, int device, void *stream, sr_graph_stats **out) {
    if (!out) return sr_fail(SR_ERR_INVALID, "null argument");
    *out = nullptr;
    if (device < SR_STATS_DEVICE_HOST) return sr_fail(SR_ERR_INVALID, "stats: device must be >= -1");
    StTables t;
    int r = st_tables(g, t);
    if (r) return r;
    sr_graph_stats *res = st_result(t);
    if (!res) return sr_fail(SR_ERR_NOMEM, "not enough memory for the statistics");
    if (device < 0) st_run_host(t, res);
    else if ((r = st_run_device(t, device, stream, res))) { sr_graph_stats_free(res); return r; }
    st_finish(res);
    *out = res;
    return SR_OK;
}

extern "C" int sr_graph_stats_gfa(const char *gfa_in, int device, sr_graph_stats **out) {
    if (!gfa_in || !out) return sr_fail(SR_ERR_INVALID, "null argument");
    SrGraph g;
    std::vector<std::string> names;
    int r = sr_graph_parse_gfa(gfa_in, g, names);
    if (r) return r;
    return sr_graph_stats_run(g, device, nullptr, out);
}

extern "C" void sr_graph_stats_free(sr_graph_stats *s) {
    if (!s) return;
    free(s->depth); free(s->paths_on); free(s->bp_by_paths); free(s->nodes_by_paths); free(s->shared);
    free(s->path_pairs); free(s->path_abs); free(s->path_len); free(s->path_sq);
    free(s);
}

extern "C" int sr_stats_sq_sums_host(const uint64_t *e, uint64_t n, uint64_t out[3]) {
    if ((!e && n) || !out) return sr_fail(SR_ERR_INVALID, "null argument");
    out[0] = out[1] = out[2] = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (e[i] >> 32) return sr_fail(SR_ERR_INVALID, "sr_stats_sq_sums_host: values must be below 2^32");
        uint64_t hh, hl, ll;
        sr_stats_sq_split(e[i], &hh, &hl, &ll);
        out[0] += hh; out[1] += hl; out[2] += ll;
    }
    return SR_OK;
}

extern "C" int sr_graph_stats_report(const sr_graph_stats *s, const char *const *names, char **text) {
    if (!s || !text) return sr_fail(SR_ERR_INVALID, "null argument");
    const uint64_t P = s->paths;
    auto name = [&](uint64_t p) { return names && names[p] ? std::string(names[p]) : u64s(p); };
    std::string o = "#seqrush_amd graph statistics v1\n";
    o += "summary\tlength\t" + u64s(s->length) + "\nsummary\tnodes\t" + u64s(s->nodes) + "\nsummary\tedges\t" + u64s(s->edges) +
         "\nsummary\tpaths\t" + u64s(s->paths) + "\nsummary\tsteps\t" + u64s(s->steps) + "\n";
    o += "steps\trev_steps\t" + u64s(s->rev_steps) + "\nsteps\tdepth_bp\t" + u64s(s->depth_bp) + "\nsteps\tmean_depth\t" +
         ratio((double)s->depth_bp, (double)s->length) + "\n";
    o += "#classes\tclass\tbp\tnodes\n";
    o += "classes\tcore\t" + u64s(s->bp_by_paths[P]) + "\t" + u64s(s->nodes_by_paths[P]) + "\n";
    o += "classes\tprivate\t" + (P >= 1 ? u64s(s->bp_by_paths[1]) + "\t" + u64s(s->nodes_by_paths[1]) : std::string("0\t0")) + "\n";
    o += "classes\tunused\t" + u64s(s->bp_by_paths[0]) + "\t" + u64s(s->nodes_by_paths[0]) + "\n";
    o += "#by_paths\tpaths\tbp\tnodes\n";
    for (uint64_t c = 0; c <= P; c++)
        if (s->nodes_by_paths[c]) o += "by_paths\t" + u64s(c) + "\t" + u64s(s->bp_by_paths[c]) + "\t" + u64s(s->nodes_by_paths[c]) + "\n";
    o += "topology\tself_loops\t" + u64s(s->self_loops) + "\ntopology\ttips\t" + u64s(s->tips) + "\ntopology\tcomponents\t" +
         u64s(s->components) + "\n";
    o += "#similarity\tpath_a\tpath_b\tshared_bp\tjaccard\n";
    for (uint64_t i = 0; i < P; i++)
        for (uint64_t j = i; j < P; j++) {
            const uint64_t sij = s->shared[i * P + j], sii = s->shared[i * P + i], sjj = s->shared[j * P + j];
            if (!sij && i != j) continue;
            o += "similarity\t" + name(i) + "\t" + name(j) + "\t" + u64s(sij) + "\t" + ratio((double)sij, (double)(sii + sjj - sij)) + "\n";
        }
    o += "#layout_path\tpath\tpairs\tsum_abs\tsum_sq\tpath_length\tmse\tmae\n";
    for (uint64_t p = 0; p < P; p++) {
        if (!s->path_pairs[p]) continue;
        const unsigned __int128 sq = sq_join(s->path_sq + p * 3);
        o += "layout_path\t" + name(p) + "\t" + u64s(s->path_pairs[p]) + "\t" + u64s(s->path_abs[p]) + "\t" + u128_dec(sq) + "\t" +
             u64s(s->path_len[p]) + "\t" + ratio((double)sq, (double)s->path_pairs[p]) + "\t" +
             ratio((double)s->path_abs[p], (double)s->path_pairs[p]) + "\n";
    }
    const unsigned __int128 sq = sq_join(s->total_sq);
    const double n = (double)s->total_pairs, mse = n > 0 ? (double)sq / n : 0.0, mae = n > 0 ? (double)s->total_abs / n : 0.0;
    o += "layout\tpairs\t" + u64s(s->total_pairs) + "\nlayout\tsum_abs\t" + u64s(s->total_abs) + "\nlayout\tsum_sq\t" + u128_dec(sq) +
         "\nlayout\tpath_length\t" + u64s(s->total_len) + "\n";
    o += "layout\tmse\t" + ratio((double)sq, n) + "\n";
    {
        char buf[64];
        snprintf(buf, sizeof buf, "%.6f", __builtin_sqrt(mse));
        o += std::string("layout\trmse\t") + (n > 0 ? buf : "NA") + "\n";
    }
    o += "layout\tmae\t" + ratio((double)s->total_abs, n) + "\n";
    o += "layout\tnormalized_mse\t" + ratio((double)sq, (double)s->length) + "\n";
    o += "layout\tnormalized_mae\t" + ratio((double)s->total_abs, (double)s->length) + "\n";
    // overall_mae / (total_path_length / total_steps) * 100 (measure_layout_quality.rs:209)
    o += "layout\trelative_error_pct\t" + (n > 0 ? ratio(mae, (double)s->total_len / n, 100.0) : std::string("NA")) + "\n";
    return sr_give_text(o, text, "not enough memory for the report");
}
