// sr_growth.hip -- pangenome growth curves by permutation (--growth; include/seqrush_amd.h "pangenome growth", DESIGN.md
// section 14): for every permutation of the groups of paths, the base pairs seen by at least one (pan) and by all (core)
// of its first k groups, on the device and, in plain loops over the same bit columns and the same rule header, on the
// host.  Every quantity is an integer sum, so the two agree exactly.  Expectations, the Heaps' law fit and the report are
// formed here from the integer tables, once for every front end.
//
// Device: presence is a group-major bitset C[g][ceil(V / 64)], one bit per node, so a permutation is a prefix OR / AND
// over columns.  Four groups of kernels on one stream, hipEvents around them, one synchronisation after the download:
// presence (one lane per step) -> histogram (privatised in LDS) -> ranks (one workgroup per permutation, keys in LDS) ->
// growth (lane = node word, wave = permutation, the chunk's node lengths in LDS) and the prefix pass that forms the two
// tables.  No captured graph.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>
#include "../../include/seqrush_amd.h"
#include "sr_internal.h"
#include "sr_sort.h"
#include "sr_stage_host.h"
#include "sr_stage_dev.h"
#include "sr_growth_rule.h"

#define GR_BLOCK 256
#define GR_WAVES (GR_BLOCK / 64)
#define GR_MAX_PERMS_PER_BLOCK 64u         // a workgroup's waves share one LDS copy of the chunk's lengths over this many permutations

typedef unsigned long long u64d;

static_assert(GR_BLOCK == SR_STAGE_BLOCK, "the grids of sr_stage_grid");
static_assert(SR_GROWTH_CHUNK_WORDS == 64, "one node word per lane of a wave");
static_assert((SR_GROWTH_MAX_GROUPS + 1) * 8 <= 65536, "the histogram and the keys of one permutation fit 64 KiB of LDS");

// ------------------------------------------------------------------ presence
// steps name nodes 1..V (checked on the host); cnt[b] = groups present on node b + 1
__global__ void __launch_bounds__(GR_BLOCK) gr_presence_kernel(const uint32_t *steps, uint32_t S, const uint32_t *path_off, uint32_t np,
                                                               const uint32_t *group_of, uint64_t W, u64d *cols, uint32_t *cnt) {
    const uint64_t s = (uint64_t)blockIdx.x * GR_BLOCK + threadIdx.x;
    if (s >= S) return;
    const uint32_t b = (steps[s] >> 1) - 1;
    const uint32_t g = group_of[sr_path_of(path_off, np, (uint32_t)s)];
    const u64d bit = 1ULL << (b & 63u);
    const u64d old = atomicOr(&cols[(uint64_t)g * W + (b >> 6)], bit);
    if (!(old & bit)) atomicAdd(&cnt[b], 1u);
}

// ------------------------------------------------------------------ histogram
// dynamic LDS: (G + 1) u64 base-pair bins
__global__ void __launch_bounds__(GR_BLOCK) gr_hist_kernel(const uint32_t *len, const uint32_t *cnt, uint32_t V, uint32_t G, u64d *hist) {
    extern __shared__ u64d gr_lds[];
    for (uint32_t i = threadIdx.x; i <= G; i += GR_BLOCK) gr_lds[i] = 0;
    __syncthreads();
    const uint32_t stride = gridDim.x * GR_BLOCK;
    for (uint64_t b = (uint64_t)blockIdx.x * GR_BLOCK + threadIdx.x; b < V; b += stride) atomicAdd(&gr_lds[cnt[b]], (u64d)len[b]);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i <= G; i += GR_BLOCK)
        if (gr_lds[i]) atomicAdd(&hist[i], gr_lds[i]);
}

// ------------------------------------------------------------------ ranks
// one workgroup per sampled permutation; dynamic LDS: the G keys.  The rank of g = the groups that sort before it; every
// lane reads the same key at a time (an LDS broadcast).
__global__ void __launch_bounds__(GR_BLOCK) gr_ranks_kernel(uint64_t seed, uint32_t G, uint32_t *perm) {
    extern __shared__ u64d gr_lds[];
    const uint32_t r = blockIdx.x;
    for (uint32_t g = threadIdx.x; g < G; g += GR_BLOCK) gr_lds[g] = sr_growth_key(seed, r, g);
    __syncthreads();
    for (uint32_t g = threadIdx.x; g < G; g += GR_BLOCK) {
        const u64d kg = gr_lds[g];
        uint32_t rank = 0;
        for (uint32_t o = 0; o < G; o++) rank += sr_growth_before(gr_lds[o], o, kg, g) ? 1u : 0u;
        perm[(uint64_t)r * G + rank] = g;
    }
}

__global__ void __launch_bounds__(GR_BLOCK) gr_unrank_kernel(uint32_t R, uint32_t G, uint32_t *perm) {
    const uint64_t r = (uint64_t)blockIdx.x * GR_BLOCK + threadIdx.x;
    if (r < R) sr_growth_unrank(r, G, perm + r * G);
}

// ------------------------------------------------------------------ growth
// lane l of every wave owns word chunk * 64 + l; bit j of it is node index (chunk * 64 + l) * 64 + j, whose length sits at
// llen[l * 65 + j], bank (l + j) mod 32: the rows are padded by one dword, so lanes that walk their words in step (a
// column that is new as a whole) read 32 different banks per half wave, and the copy is stored without a conflict.
#ifndef SR_GROWTH_LEN_STRIDE
#define SR_GROWTH_LEN_STRIDE 65u           // 64u: dense rows, every lane of a half wave on one bank; the yardstick of scripts/growth_bench.py only
#endif
#define GR_LEN_STRIDE SR_GROWTH_LEN_STRIDE
static_assert(GR_LEN_STRIDE >= 64, "a row holds the 64 nodes of a word");
__device__ __forceinline__ u64d gr_weigh(u64d bits, const uint32_t *llen, uint32_t lane) {
    u64d sum = 0;
    while (bits) {
        const int j = __ffsll(bits) - 1;
        bits &= bits - 1;
        sum += llen[lane * GR_LEN_STRIDE + j];
    }
    return sum;
}

__device__ __forceinline__ u64d gr_wave_sum(u64d v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;                                        // lane 0 holds the wave's sum
}

// work item = (chunk of 64 node words, slice of ppb permutations); the waves of a workgroup take the slice's permutations
// in turn.  pan_new[r][k] and core_lost[r][k] receive one add per non-zero (r, k) and chunk; column 0 of core_lost stays
// zero (the core of one group is its pan).
__global__ void __launch_bounds__(GR_BLOCK) gr_growth_kernel(const u64d *cols, uint64_t W, uint32_t V, const uint32_t *len, const uint32_t *perm,
                                                             uint32_t R, uint32_t G, uint32_t ppb, uint32_t slices, u64d *pan_new,
                                                             u64d *core_lost) {
    __shared__ uint32_t llen[SR_GROWTH_CHUNK_WORDS * GR_LEN_STRIDE];
    const uint32_t chunk = blockIdx.x / slices, slice = blockIdx.x - chunk * slices;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t node0 = (uint64_t)chunk * SR_GROWTH_CHUNK_NODES;
    for (uint32_t i = threadIdx.x; i < SR_GROWTH_CHUNK_NODES; i += GR_BLOCK) {
        const uint64_t b = node0 + i;                // node index b = (word, bit) = (i >> 6, i & 63)
        llen[(i >> 6) * GR_LEN_STRIDE + (i & 63u)] = b < V ? len[b] : 0;
    }
    __syncthreads();
    const uint64_t word = (uint64_t)chunk * SR_GROWTH_CHUNK_WORDS + lane;
    const bool live = word < W;
    const u64d mask = live ? sr_growth_word_mask(V, word) : 0;
    const u64d *col = cols + (live ? word : 0);
    const uint32_t r1 = (uint64_t)(slice + 1) * ppb < R ? (slice + 1) * ppb : R;
    for (uint32_t r = slice * ppb + wave; r < r1; r += GR_WAVES) {     // wave-uniform
        const uint32_t *row = perm + (uint64_t)r * G;
        u64d acc_or = 0, acc_and = mask;
        for (uint32_t k = 0; k < G; k++) {
            const uint32_t g = row[k];               // the same address in every lane: one scalar-like load
            const u64d w = live ? col[(uint64_t)g * W] : 0;
            const u64d fresh = w & ~acc_or, lost = acc_and & ~w;
            acc_or |= w;
            acc_and &= w;
            if (__ballot(fresh != 0)) {              // wave-uniform: most columns bring nothing new to most chunks
                const u64d s = gr_wave_sum(gr_weigh(fresh, llen, lane));
                if (lane == 0 && s) atomicAdd(&pan_new[(uint64_t)r * G + k], s);
            }
            if (k && __ballot(lost != 0)) {
                const u64d s = gr_wave_sum(gr_weigh(lost, llen, lane));
                if (lane == 0 && s) atomicAdd(&core_lost[(uint64_t)r * G + k], s);
            }
        }
    }
}

// pan[r][k] = sum_{j <= k} pan_new[r][j];  core[r][1] = pan[r][1], core[r][k] = core[r][k - 1] - core_lost[r][k]; in place
__global__ void __launch_bounds__(GR_BLOCK) gr_prefix_kernel(uint32_t R, uint32_t G, u64d *pan, u64d *core) {
    const uint64_t r = (uint64_t)blockIdx.x * GR_BLOCK + threadIdx.x;
    if (r >= R) return;
    u64d *p = pan + r * G, *c = core + r * G;
    u64d ps = 0, cs = 0;
    for (uint32_t k = 0; k < G; k++) {
        ps += p[k];
        cs = k ? cs - c[k] : ps;
        p[k] = ps; c[k] = cs;
    }
}

namespace {

// the tables both executions read.  Node v = 1..V sits at index v - 1.
struct GrTables : SrPathTables {
    uint32_t G = 0, R = 0;
    uint64_t L = 0, W = 0, seed = 0;
    bool exhaustive = false;
    std::vector<uint32_t> group_of;
};

int gr_tables(const SrGraph &g, const uint32_t *group_of, uint32_t n_groups, const sr_growth_params &prm, GrTables &t) {
    if (prm.permutations == 0) return sr_fail(SR_ERR_INVALID, "growth: permutations must be at least 1");
    const SrPathSizes z = sr_path_sizes(g);
    const uint64_t nn = z.nodes, np = z.paths;
    if (nn >= 0x3fffffffULL || z.steps >= 0x7fffffffULL || np >= 0x7fffffffULL || z.bases >= 0x7fffffffULL)
        return sr_fail(SR_ERR_UNSUPPORTED, "growth supports < 2^30 nodes and < 2^31 steps, paths and bases");
    const uint64_t G = group_of ? n_groups : np;
    if (G > SR_GROWTH_MAX_GROUPS) return sr_fail(SR_ERR_UNSUPPORTED, "growth: " + std::to_string(G) + " groups; at most 4096 are supported");
    t.L = z.bases; t.W = sr_growth_words(nn); t.seed = prm.seed;
    t.group_of.resize(np);
    std::vector<uint8_t> used(G, 0);
    for (uint64_t p = 0; p < np; p++) {
        const uint32_t q = group_of ? group_of[p] : (uint32_t)p;
        if (q >= G) return sr_fail(SR_ERR_INVALID, "growth: path " + std::to_string(p) + " is in group " + std::to_string(q) + " of " + std::to_string(G));
        t.group_of[p] = q; used[q] = 1;
    }
    for (uint64_t q = 0; q < G; q++)
        if (!used[q]) return sr_fail(SR_ERR_INVALID, "growth: group " + std::to_string(q) + " has no path");
    if (G && prm.permutations > SR_GROWTH_MAX_CELLS / G)
        return sr_fail(SR_ERR_UNSUPPORTED, "growth: " + std::to_string(prm.permutations) + " permutations x " + std::to_string(G) + " groups; the tables support at most 2^24 cells");
    t.G = (uint32_t)G;
    t.exhaustive = G >= 1 && G <= SR_GROWTH_EXHAUSTIVE_MAX && sr_growth_factorial((uint32_t)G) <= prm.permutations;
    t.R = G == 0 ? 0 : t.exhaustive ? (uint32_t)sr_growth_factorial((uint32_t)G) : (uint32_t)prm.permutations;
    return sr_path_tables_fill(g, z, "growth", false, false, t);
}

sr_growth *gr_result(const GrTables &t) {
    sr_growth *r = (sr_growth *)calloc(1, sizeof(sr_growth));
    if (!r) return nullptr;
    r->length = t.L; r->paths = t.P; r->groups = t.G; r->permutations = t.R; r->exhaustive = t.exhaustive ? 1 : 0; r->seed = t.seed;
    const uint64_t cells = (uint64_t)t.R * t.G;
    r->pan = (uint64_t *)calloc(cells ? cells : 1, 8); r->core = (uint64_t *)calloc(cells ? cells : 1, 8);
    r->perm = (uint32_t *)calloc(cells ? cells : 1, 4); r->bp_by_groups = (uint64_t *)calloc((uint64_t)t.G + 1, 8);
    if (!r->pan || !r->core || !r->perm || !r->bp_by_groups) { sr_growth_free(r); return nullptr; }
    return r;
}

// ------------------------------------------------------------------ host twin: plain loops over the same bit columns
void gr_run_host(const GrTables &t, sr_growth *r) {
    const uint32_t V = t.V, G = t.G, R = t.R;
    const uint64_t W = t.W;
    auto t0 = std::chrono::steady_clock::now();
    const auto t_all = t0;
    r->variant = SR_GROWTH_VARIANT_HOST;
    std::vector<uint64_t> cols((uint64_t)G * W, 0);
    std::vector<uint32_t> cnt(V, 0);
    for (uint32_t p = 0; p < t.P; p++) {
        uint64_t *col = cols.data() + (uint64_t)t.group_of[p] * W;
        for (uint32_t s = t.path_off[p]; s < t.path_off[p + 1]; s++) {
            const uint32_t b = (t.steps[s] >> 1) - 1;
            const uint64_t bit = 1ULL << (b & 63u);
            if (!(col[b >> 6] & bit)) { col[b >> 6] |= bit; cnt[b]++; }
        }
    }
    r->kernel_us[0] = (uint64_t)(us_since(t0) + 0.5);
    t0 = std::chrono::steady_clock::now();
    for (uint32_t b = 0; b < V; b++) r->bp_by_groups[cnt[b]] += t.len[b];
    r->kernel_us[1] = (uint64_t)(us_since(t0) + 0.5);
    t0 = std::chrono::steady_clock::now();
    std::vector<std::pair<uint64_t, uint32_t>> keyed(G);
    for (uint32_t q = 0; q < R; q++) {
        uint32_t *row = r->perm + (uint64_t)q * G;
        if (t.exhaustive) { sr_growth_unrank(q, G, row); continue; }
        for (uint32_t g = 0; g < G; g++) keyed[g] = {sr_growth_key(t.seed, q, g), g};
        std::sort(keyed.begin(), keyed.end());       // (key, g) ascending: the order of sr_growth_before
        for (uint32_t k = 0; k < G; k++) row[k] = keyed[k].second;
    }
    r->kernel_us[2] = (uint64_t)(us_since(t0) + 0.5);
    t0 = std::chrono::steady_clock::now();
    auto weigh = [&](uint64_t bits, uint64_t word) {
        uint64_t sum = 0;
        for (; bits; bits &= bits - 1) sum += t.len[(word << 6) + (uint64_t)__builtin_ctzll(bits)];
        return sum;
    };
    std::vector<uint64_t> acc_or(W), acc_and(W);
    for (uint32_t q = 0; q < R; q++) {
        const uint32_t *row = r->perm + (uint64_t)q * G;
        uint64_t *pan = r->pan + (uint64_t)q * G, *core = r->core + (uint64_t)q * G;
        for (uint64_t w = 0; w < W; w++) { acc_or[w] = 0; acc_and[w] = sr_growth_word_mask(V, w); }
        uint64_t ps = 0, cs = 0;
        for (uint32_t k = 0; k < G; k++) {
            const uint64_t *col = cols.data() + (uint64_t)row[k] * W;
            uint64_t fresh_bp = 0, lost_bp = 0;
            for (uint64_t w = 0; w < W; w++) {
                const uint64_t c = col[w], fresh = c & ~acc_or[w], lost = acc_and[w] & ~c;
                acc_or[w] |= c; acc_and[w] &= c;
                if (fresh) fresh_bp += weigh(fresh, w);
                if (lost && k) lost_bp += weigh(lost, w);
            }
            ps += fresh_bp;
            cs = k ? cs - lost_bp : ps;
            pan[k] = ps; core[k] = cs;
        }
    }
    r->kernel_us[3] = (uint64_t)(us_since(t0) + 0.5);
    r->growth_us = (uint64_t)(us_since(t_all) + 0.5);
}

// ------------------------------------------------------------------ device execution
int gr_run_device(const GrTables &t, int device, void *stream, sr_growth *r) {
    const uint32_t V = t.V, S = t.S, P = t.P, G = t.G, R = t.R;
    const uint64_t W = t.W;
    SrStage x("growth", "the growth tables");
    if (x.open(device, stream, 6)) return x.err;
    r->variant = SR_GROWTH_VARIANT_WAVE;
    if (!G) return SR_OK;                            // no group: empty tables; bp_by_groups[0] below needs no device either
    const uint64_t cells = (uint64_t)R * G;          // <= 2^24
    const uint64_t chunks = (W + SR_GROWTH_CHUNK_WORDS - 1) / SR_GROWTH_CHUNK_WORDS;      // <= 2^18
    // permutations per workgroup: enough workgroups to fill the device on a small graph, a shared LDS copy on a large one
    uint64_t ppb = (chunks * R + 2047) / 2048;
    ppb = ppb < GR_WAVES ? GR_WAVES : ppb > GR_MAX_PERMS_PER_BLOCK ? GR_MAX_PERMS_PER_BLOCK : ppb;
    const uint64_t slices = (R + ppb - 1) / ppb;     // <= 2^22; chunks x slices < 2^31 is checked below
    if (chunks * slices > 0x7fffffffULL) return sr_fail(SR_ERR_UNSUPPORTED, "growth: too many (chunk, permutation) work items for one launch");

    uint32_t *d_len = x.alloc<uint32_t>(V), *d_cnt = x.alloc<uint32_t>(V, 0), *d_steps = x.alloc<uint32_t>(S);
    uint32_t *d_poff = x.alloc<uint32_t>((uint64_t)P + 1), *d_gof = x.alloc<uint32_t>(P);
    u64d *d_cols = x.alloc<u64d>((uint64_t)G * W, 0), *d_hist = x.alloc<u64d>((uint64_t)G + 1, 0);
    uint32_t *d_perm = x.alloc<uint32_t>(cells);
    u64d *d_pan = x.alloc<u64d>(cells, 0), *d_core = x.alloc<u64d>(cells, 0);
    if (x.err) return x.err;
    x.put(d_len, t.len.data(), (size_t)V * 4); x.put(d_steps, t.steps.data(), (size_t)S * 4);
    x.put(d_poff, t.path_off.data(), ((size_t)P + 1) * 4); x.put(d_gof, t.group_of.data(), (size_t)P * 4);

    x.mark(0);
    if (!x.err && S) hipLaunchKernelGGL(gr_presence_kernel, dim3(sr_stage_grid(S)), dim3(GR_BLOCK), 0, x.st, d_steps, S, d_poff, P, d_gof, W, d_cols, d_cnt);
    x.mark(1);
    if (!x.err && V) {
        const uint64_t blocks = sr_stage_grid(V) < 1024 ? sr_stage_grid(V) : 1024;
        hipLaunchKernelGGL(gr_hist_kernel, dim3((unsigned)blocks), dim3(GR_BLOCK), ((size_t)G + 1) * 8, x.st, d_len, d_cnt, V, G, d_hist);
    }
    x.mark(2);
    if (!x.err) {
        if (t.exhaustive) hipLaunchKernelGGL(gr_unrank_kernel, dim3(sr_stage_grid(R)), dim3(GR_BLOCK), 0, x.st, R, G, d_perm);
        else hipLaunchKernelGGL(gr_ranks_kernel, dim3(R), dim3(GR_BLOCK), (size_t)G * 8, x.st, (uint64_t)t.seed, G, d_perm);
    }
    x.mark(3);
    if (!x.err) {
        if (W) hipLaunchKernelGGL(gr_growth_kernel, dim3((unsigned)(chunks * slices)), dim3(GR_BLOCK), 0, x.st, d_cols, W, V, d_len, d_perm, R, G,
                                  (uint32_t)ppb, (uint32_t)slices, d_pan, d_core);
        hipLaunchKernelGGL(gr_prefix_kernel, dim3(sr_stage_grid(R)), dim3(GR_BLOCK), 0, x.st, R, G, d_pan, d_core);
    }
    x.mark(4);
    x.chk(hipGetLastError());
    x.get(r->pan, d_pan, (size_t)cells * 8); x.get(r->core, d_core, (size_t)cells * 8); x.get(r->perm, d_perm, (size_t)cells * 4);
    x.get(r->bp_by_groups, d_hist, ((size_t)G + 1) * 8);
    x.mark(5);
    x.sync();                                        // the one synchronisation
    if (x.err) return x.err;
    r->growth_us = x.us(0, 5);
    for (int k = 0; k < 4; k++) r->kernel_us[k] = x.us(k, k + 1);
    return x.err;
}

std::string f6(double v) { char b[64]; snprintf(b, sizeof b, "%.6f", v); return b; }

}   // namespace

int sr_graph_growth_run(const SrGraph &g, const uint32_t *group_of, uint32_t n_groups, const sr_growth_params &prm, int device, void *stream,
                        sr_growth **out) {
    if (!out) return sr_fail(SR_ERR_INVALID, "null argument");
    *out = nullptr;
    if (device < SR_GROWTH_DEVICE_HOST) return sr_fail(SR_ERR_INVALID, "growth: device must be >= -1");
    try {
        GrTables t;
        int r = gr_tables(g, group_of, n_groups, prm, t);
        if (r) return r;
        sr_growth *res = gr_result(t);
        if (!res) return sr_fail(SR_ERR_NOMEM, "not enough memory for the growth tables");
        if (device < 0) gr_run_host(t, res);
        else if ((r = gr_run_device(t, device, stream, res))) { sr_growth_free(res); return r; }
        if (!t.G) res->bp_by_groups[0] = t.L;        // no group: every node is on none
        *out = res;
    } catch (const std::bad_alloc &) {
        if (*out) { sr_growth_free(*out); *out = nullptr; }
        return sr_fail(SR_ERR_NOMEM, "not enough memory for the growth tables");
    }
    return SR_OK;
}

extern "C" void sr_growth_params_default(sr_growth_params *p) {
    if (!p) return;
    p->seed = 9399220; p->permutations = 1000;
}

extern "C" int sr_growth_gfa(const char *gfa_in, const uint32_t *group_of, uint32_t n_groups, const sr_growth_params *p, int device,
                             sr_growth **out) {
    if (!gfa_in || !p || !out) return sr_fail(SR_ERR_INVALID, "null argument");
    SrGraph g;
    std::vector<std::string> names;
    int r = sr_graph_parse_gfa(gfa_in, g, names);
    if (r) return r;
    return sr_graph_growth_run(g, group_of, n_groups, *p, device, nullptr, out);
}

extern "C" void sr_growth_free(sr_growth *g) {
    if (!g) return;
    free(g->pan); free(g->core); free(g->perm); free(g->bp_by_groups);
    free(g);
}

extern "C" int sr_growth_groups(const char *const *path_names, uint64_t n_paths, int mode, uint32_t *group_of, uint32_t *n_groups,
                                char ***group_names) {
    if ((!path_names && n_paths) || !group_of || !n_groups) return sr_fail(SR_ERR_INVALID, "null argument");
    if (mode < 0 || mode > 2) return sr_fail(SR_ERR_INVALID, "growth: the grouping mode must be 0 (path), 1 (sample) or 2 (haplotype)");
    if (n_paths >= 0x7fffffffULL) return sr_fail(SR_ERR_UNSUPPORTED, "growth supports < 2^31 paths");
    if (group_names) *group_names = nullptr;
    try {
        std::unordered_map<std::string, uint32_t> seen;
        std::vector<std::string> keys;
        for (uint64_t p = 0; p < n_paths; p++) {
            if (!path_names[p]) return sr_fail(SR_ERR_INVALID, "null argument");
            const std::string name = path_names[p];
            if (mode == 0) { group_of[p] = (uint32_t)p; keys.push_back(name); continue; }
            size_t cut = name.find('#');
            if (mode == 2 && cut != std::string::npos) cut = name.find('#', cut + 1);
            const std::string key = cut == std::string::npos ? name : name.substr(0, cut);
            auto it = seen.find(key);
            if (it == seen.end()) { it = seen.emplace(key, (uint32_t)keys.size()).first; keys.push_back(key); }
            group_of[p] = it->second;
        }
        *n_groups = (uint32_t)keys.size();
        if (group_names) {
            size_t chars = 0;
            for (const auto &k : keys) chars += k.size() + 1;
            const size_t slots = keys.size() ? keys.size() : 1;
            char **arr = (char **)malloc(sizeof(char *) * slots + chars);         // one block: the pointers, then the strings
            if (!arr) return sr_fail(SR_ERR_NOMEM, "not enough memory for the group names");
            arr[0] = nullptr;
            char *at = (char *)(arr + slots);
            for (size_t i = 0; i < keys.size(); i++) { arr[i] = at; memcpy(at, keys[i].c_str(), keys[i].size() + 1); at += keys[i].size() + 1; }
            *group_names = arr;
        }
    } catch (const std::bad_alloc &) {
        return sr_fail(SR_ERR_NOMEM, "not enough memory for the group names");
    }
    return SR_OK;
}

// E pan(k) = sum_c bp[c] (1 - prod_{i<k} (G - c - i) / (G - i)),  E core(k) = sum_c bp[c] prod_{i<k} (c - i) / (G - i):
// the products run along k for every c, a factor that reaches zero stays zero
extern "C" int sr_growth_expected(const uint64_t *bp_by_groups, uint32_t groups, double *pan_exp, double *core_exp) {
    if (!bp_by_groups || (groups && (!pan_exp || !core_exp))) return sr_fail(SR_ERR_INVALID, "null argument");
    const uint32_t G = groups;
    for (uint32_t k = 0; k < G; k++) pan_exp[k] = core_exp[k] = 0.0;
    for (uint32_t c = 1; c <= G; c++) {
        if (!bp_by_groups[c]) continue;
        const double bp = (double)bp_by_groups[c];
        double none = 1.0, all = 1.0;                // none / all of the first k groups are on a node of c groups
        for (uint32_t i = 0; i < G; i++) {           // i = k - 1
            none = i < G - c ? none * ((double)(G - c - i) / (double)(G - i)) : 0.0;
            all = i < c ? all * ((double)(c - i) / (double)(G - i)) : 0.0;
            pan_exp[i] += bp * (1.0 - none);
            core_exp[i] += bp * all;
        }
    }
    return SR_OK;
}

// least squares of y = log new(k) on x = log k, k = 2..G, new(k) = pan_exp[k - 1] - pan_exp[k - 2] > 0, about the means:
// new ~ kappa k^-alpha.  Fewer than two usable points: *points says so, alpha = kappa = 0, no error.
extern "C" int sr_growth_fit(const double *pan_exp, uint32_t groups, double *alpha, double *kappa, uint32_t *points) {
    if ((groups && !pan_exp) || !alpha || !kappa || !points) return sr_fail(SR_ERR_INVALID, "null argument");
    *alpha = *kappa = 0.0; *points = 0;
    uint32_t n = 0;
    double mx = 0.0, my = 0.0;
    for (uint32_t k = 2; k <= groups; k++) {
        const double d = pan_exp[k - 1] - pan_exp[k - 2];
        if (!(d > 0.0)) continue;
        n++; mx += log((double)k); my += log(d);
    }
    *points = n;
    if (n < 2) return SR_OK;
    mx /= n; my /= n;
    double sxx = 0.0, sxy = 0.0;
    for (uint32_t k = 2; k <= groups; k++) {
        const double d = pan_exp[k - 1] - pan_exp[k - 2];
        if (!(d > 0.0)) continue;
        const double dx = log((double)k) - mx;
        sxx += dx * dx; sxy += dx * (log(d) - my);
    }
    const double slope = sxy / sxx;                  // n >= 2 distinct k: sxx > 0
    *alpha = -slope;
    *kappa = exp(my - slope * mx);
    return SR_OK;
}

extern "C" int sr_growth_report(const sr_growth *g, char **text) {
    if (!g || !text) return sr_fail(SR_ERR_INVALID, "null argument");
    const uint64_t G = g->groups, R = g->permutations;
    if (G > SR_GROWTH_MAX_GROUPS || (G && R > SR_GROWTH_MAX_CELLS)) return sr_fail(SR_ERR_INVALID, "growth: not a result of sr_growth_gfa");
    try {
        std::vector<double> pe(G), ce(G);
        int rc = sr_growth_expected(g->bp_by_groups, (uint32_t)G, pe.data(), ce.data());
        if (rc) return rc;
        double alpha = 0, kappa = 0;
        uint32_t points = 0;
        if ((rc = sr_growth_fit(pe.data(), (uint32_t)G, &alpha, &kappa, &points))) return rc;
        const bool fit = points >= 2;
        std::string o = "#seqrush_amd growth v1\tgroups=" + u64s(G) + "\tpaths=" + u64s(g->paths) + "\tpermutations=" + u64s(R) + "\texhaustive=" +
                        u64s((uint64_t)g->exhaustive) + "\tseed=" + u64s(g->seed) + "\tlength=" + u64s(g->length) + "\n";
        o += "#classes\tunused=" + u64s(g->bp_by_groups[0]) + "\tcore=" + u64s(g->bp_by_groups[G]) + "\n";
        o += "#heaps\talpha=" + (fit ? f6(alpha) : std::string("NA")) + "\tkappa=" + (fit ? f6(kappa) : std::string("NA")) + "\tpoints=" + u64s(points) +
             "\t" + (fit ? (alpha <= 1.0 ? "open" : "closed") : "NA") + "\n";
        o += "k\tpan_exp\tcore_exp\tpan_mean\tpan_sd\tpan_min\tpan_max\tcore_mean\tcore_sd\tcore_min\tcore_max\n";
        // min, max, sum and sum of squares over the permutations in integers; the floats are formed from them here
        typedef unsigned __int128 u128;
        auto column = [&](const uint64_t *tab, uint64_t k) {
            uint64_t lo = ~0ULL, hi = 0;
            u128 s = 0, s2 = 0;
            for (uint64_t q = 0; q < R; q++) {
                const uint64_t v = tab[q * G + k];
                lo = v < lo ? v : lo; hi = v > hi ? v : hi;
                s += v; s2 += (u128)v * v;
            }
            const u128 num = (u128)R * s2 - s * s;   // R^2 x the population variance, exact
            return f6((double)s / (double)R) + "\t" + f6(sqrt((double)num / (double)(R * R))) + "\t" + u64s(lo) + "\t" + u64s(hi);
        };
        for (uint64_t k = 0; k < G; k++)
            o += u64s(k + 1) + "\t" + f6(pe[k]) + "\t" + f6(ce[k]) + "\t" + column(g->pan, k) + "\t" + column(g->core, k) + "\n";
        return sr_give_text(o, text, "not enough memory for the growth report");
    } catch (const std::bad_alloc &) {
        return sr_fail(SR_ERR_NOMEM, "not enough memory for the growth report");
    }
}
