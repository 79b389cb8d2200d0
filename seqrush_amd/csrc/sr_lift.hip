// sr_lift.hip -- the interval lift (--lift; include/seqrush_amd.h "lifting intervals"): where the BED
// intervals of one path lie in the other paths, on the device and, in plain loops over the same rule header, on the host.
// Every field is a min, a max or a sum of integers, so the two agree exactly.  The BED lines are read and the output bytes
// are formed here on the host, once for every front end.
//
// Device: five groups of kernels on one stream, hipEvents around them: positions (step lengths, an inclusive scan with a
// block-sums carry, the offset of every step in its own path) -> first visits (one lane per step of a target path,
// atomicMin into a node-major table of all ones) -> locate (one lane per query bisects twice; the queries that touch more
// than short_steps steps are compacted by a scan) -> short pairs (one lane per (query, target), targets fastest) -> long
// pairs (one wave per (long query, target), lanes stride over the steps, a shuffle reduction, lane 0 stores).  The long
// kernel reads the number of long queries from device memory and strides over the pairs, so nothing comes back before the
// download: one synchronisation.  No atomic decides a value except the min of the first-visit table.  No captured graph.
#include <hip/hip_runtime.h>
#include <algorithm>
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
#include "sr_bed_host.h"
#include "sr_lift_rule.h"

#define LF_BLOCK 256
#define LF_WAVES (LF_BLOCK / 64)
#define LF_LONG_BLOCKS 4096u                   // the long kernel's grid at most: its waves stride over the pairs

typedef uint64_t u64d;

static_assert(LF_BLOCK == SR_STAGE_BLOCK, "the grids of sr_stage_grid");

// ------------------------------------------------------------------ group 0: positions
// the step lengths and their inclusive scan: sr_stage_dev.h.  sinc = the inclusive scan over all steps -> the offset of a step in its own path
__global__ void __launch_bounds__(LF_BLOCK) lf_pstart_kernel(const uint32_t *steps, const uint32_t *len, const uint32_t *path_off, uint32_t P,
                                                             const u64d *sinc, uint32_t S, u64d *pstart) {
    const uint32_t s = blockIdx.x * LF_BLOCK + threadIdx.x;
    if (s >= S) return;
    const uint32_t a0 = path_off[sr_path_of(path_off, P, s)];
    pstart[s] = sinc[s] - len[(steps[s] >> 1) - 1] - (a0 ? sinc[a0 - 1] : 0);
}

// ------------------------------------------------------------------ group 1: first visits
// first[v * T + t]: node-major, so that lanes of the short kernel that hold consecutive targets of one node read
// consecutive words.  Steps [s0, s1); `single`: they are the steps of the one target, else target = path
__global__ void __launch_bounds__(LF_BLOCK) lf_first_kernel(const uint32_t *steps, const uint32_t *path_off, uint32_t P, uint32_t s0, uint32_t s1,
                                                            uint32_t T, int single, uint32_t *first) {
    const uint32_t s = s0 + blockIdx.x * LF_BLOCK + threadIdx.x;
    if (s >= s1) return;
    const uint32_t t = single ? 0u : sr_path_of(path_off, P, s);
    atomicMin(&first[(size_t)((steps[s] >> 1) - 1) * T + t], s);
}

// ------------------------------------------------------------------ group 2: locate
struct LfQueries { const uint32_t *path; const u64d *start, *end; uint32_t n; };

// s_lo and s_hi of every query; is_long[q] = 1 iff it touches more than short_steps steps (the input of the scan)
__global__ void __launch_bounds__(LF_BLOCK) lf_locate_kernel(LfQueries q, const uint32_t *path_off, const u64d *pstart, u64d short_steps,
                                                             uint32_t *s_lo, uint32_t *s_hi, u64d *is_long) {
    const uint32_t i = blockIdx.x * LF_BLOCK + threadIdx.x;
    if (i >= q.n) return;
    const uint32_t a0 = path_off[q.path[i]], a1 = path_off[q.path[i] + 1];
    const uint32_t lo = sr_lift_step_of(pstart, a0, a1, q.start[i]), hi = sr_lift_step_of(pstart, a0, a1, q.end[i] - 1);
    s_lo[i] = lo; s_hi[i] = hi;
    is_long[i] = (u64d)(hi - lo) + 1 > short_steps ? 1 : 0;
}

// is_long is now its inclusive scan: long query k = the scan - 1; list[k] = its index.  A query is long iff the scan rose
__global__ void __launch_bounds__(LF_BLOCK) lf_compact_kernel(const u64d *scan, uint32_t Q, uint32_t *list) {
    const uint32_t i = blockIdx.x * LF_BLOCK + threadIdx.x;
    if (i >= Q) return;
    const u64d c = scan[i];
    if (c != (i ? scan[i - 1] : 0)) list[(uint32_t)c - 1] = i;
}

// ------------------------------------------------------------------ groups 3 and 4: the pairs
struct LfOut { u64d *tstart, *tend, *covered, *rev_bp; };

__device__ __forceinline__ void lf_store(const LfOut &o, size_t pair, const SrLiftAcc &acc) {
    const SrLiftAcc r = sr_lift_finish(acc);
    o.tstart[pair] = r.lo; o.tend[pair] = r.hi; o.covered[pair] = r.covered; o.rev_bp[pair] = r.rev_bp;
}

// one lane per (query, target), targets fastest; the lanes of a long query leave it to lf_long_kernel
__global__ void __launch_bounds__(LF_BLOCK) lf_short_kernel(SrLiftTables g, LfQueries q, const uint32_t *s_lo, const uint32_t *s_hi, const u64d *scan,
                                                            const uint32_t *first, uint32_t T, LfOut out) {
    const uint32_t pair = blockIdx.x * LF_BLOCK + threadIdx.x;          // queries x targets <= 2^26
    if (pair >= q.n * T) return;
    const uint32_t i = pair / T, t = pair - i * T;
    if (scan[i] != (i ? scan[i - 1] : 0)) return;
    const u64d start = q.start[i], end = q.end[i];
    const uint32_t hi = s_hi[i];
    SrLiftAcc acc = sr_lift_empty();
    for (uint32_t s = s_lo[i]; s <= hi; s++)
        acc = sr_lift_join(acc, sr_lift_step(g, s, start, end, first[(size_t)((g.steps[s] >> 1) - 1) * T + t]));
    lf_store(out, pair, acc);
}

__device__ __forceinline__ u64d lf_shfl_down(u64d v, int o) { return __shfl_down(v, o, 64); }

// one wave per (long query, target): wave w of the grid takes the pairs w, w + waves, ... of n_long x T, where n_long is
// the last value of the scan, read here from device memory; lanes stride over the steps
__global__ void __launch_bounds__(LF_BLOCK) lf_long_kernel(SrLiftTables g, LfQueries q, const uint32_t *s_lo, const uint32_t *s_hi, const u64d *scan,
                                                           const uint32_t *list, const uint32_t *first, uint32_t T, LfOut out) {
    const uint32_t lane = threadIdx.x & 63, waves = gridDim.x * LF_WAVES;
    const u64d pairs = scan[q.n - 1] * T;
    for (u64d w = (u64d)blockIdx.x * LF_WAVES + (threadIdx.x >> 6); w < pairs; w += waves) {      // wave-uniform
        const uint32_t k = (uint32_t)(w / T), t = (uint32_t)(w - (u64d)k * T), i = list[k];
        const u64d start = q.start[i], end = q.end[i];
        const uint32_t hi = s_hi[i];
        SrLiftAcc acc = sr_lift_empty();
        for (u64d s = (u64d)s_lo[i] + lane; s <= hi; s += 64)
            acc = sr_lift_join(acc, sr_lift_step(g, (uint32_t)s, start, end, first[(size_t)((g.steps[s] >> 1) - 1) * T + t]));
#pragma unroll
        for (int o = 32; o; o >>= 1)
            acc = sr_lift_join(acc, SrLiftAcc{lf_shfl_down(acc.lo, o), lf_shfl_down(acc.hi, o), lf_shfl_down(acc.covered, o), lf_shfl_down(acc.rev_bp, o)});
        if (lane == 0) lf_store(out, (size_t)i * T + t, acc);
    }
}

namespace {

// the tables both executions read.  Node v = 1..V sits at index v - 1.
struct LfTables : SrPathTables {
    std::vector<uint64_t> plen;
    std::vector<uint32_t> target_path;
    bool to_named = false;
    uint64_t min_covered = 1, short_steps = 8;
    // the queries
    std::vector<uint32_t> q_path;
    std::vector<uint64_t> q_start, q_end;
    std::vector<std::string> label;
    uint64_t unknown = 0, out_of_range = 0;
};

struct LfOutHost {
    int variant = 0;
    uint64_t us = 0, kernel_us[5] = {0, 0, 0, 0, 0}, short_pairs = 0, long_pairs = 0;
    std::vector<uint64_t> tstart, tend, covered, rev_bp;
};

int lf_tables(const SrGraph &g, const std::vector<std::string> &names, const sr_lift_params &prm, LfTables &t) {
    const SrPathSizes z = sr_path_sizes(g);
    const uint64_t nn = z.nodes, np = z.paths;
    if (nn >= 0x3fffffffULL || z.steps >= 0x7fffffffULL || np >= 0x7fffffffULL)
        return sr_fail(SR_ERR_UNSUPPORTED, "lift supports < 2^30 nodes and < 2^31 steps and paths");
    t.min_covered = prm.min_covered; t.short_steps = prm.short_steps;
    if (prm.to_name) {
        const uint64_t p = sr_path_by_name(names, np, prm.to_name);
        if (p == np) return sr_fail(SR_ERR_INVALID, std::string("lift: no path is named '") + prm.to_name + "'");
        t.target_path.assign(1, (uint32_t)p); t.to_named = true;
    } else {
        t.target_path.resize(np);
        for (uint64_t p = 0; p < np; p++) t.target_path[p] = (uint32_t)p;
    }
    if ((uint64_t)t.target_path.size() * nn > SR_LIFT_MAX_TABLE)
        return sr_fail(SR_ERR_UNSUPPORTED, "lift: " + std::to_string(t.target_path.size()) + " targets x " + std::to_string(nn) +
                                               " nodes; the first-visit table supports at most 2^28 entries");
    if (const int r = sr_path_tables_fill(g, z, "lift", true, false, t)) return r;
    t.plen.assign(np, 0);
    for (uint64_t p = 0; p < np; p++)
        for (uint32_t s = t.path_off[p]; s < t.path_off[p + 1]; s++) t.plen[p] += t.len[(t.steps[s] >> 1) - 1];
    return SR_OK;
}

// ------------------------------------------------------------------ the BED lines
// the lines are read by sr_bed_host.h; what a name, a range and a label mean to the lift is here
int lf_queries(const char *bed, const std::vector<std::string> &names, LfTables &t) {
    std::unordered_map<std::string, uint32_t> by_name;
    for (uint32_t p = 0; p < t.P && p < names.size(); p++) by_name.emplace(names[p], p);      // the first path of a name
    const int r = sr_bed_lines(bed, "lift", [&](const std::vector<std::string> &f, uint64_t start, uint64_t end) {
        const auto it = by_name.find(f[0]);
        if (it == by_name.end()) { t.unknown++; return SR_OK; }
        if (start >= end || end > t.plen[it->second]) { t.out_of_range++; return SR_OK; }
        t.q_path.push_back(it->second); t.q_start.push_back(start); t.q_end.push_back(end);
        t.label.push_back(f.size() > 3 && !f[3].empty() ? f[3] : f[0] + ":" + f[1] + "-" + f[2]);
        return SR_OK;
    });
    if (r) return r;
    if ((uint64_t)t.q_path.size() * t.target_path.size() > SR_LIFT_MAX_PAIRS)
        return sr_fail(SR_ERR_UNSUPPORTED, "lift: " + std::to_string(t.q_path.size()) + " queries x " + std::to_string(t.target_path.size()) +
                                               " targets; the tables support at most 2^26 pairs");
    return SR_OK;
}

// ------------------------------------------------------------------ host twin: one thread, plain loops
int lf_run_host(const LfTables &t, LfOutHost &o) {
    const auto t_all = std::chrono::steady_clock::now();
    auto t0 = t_all;
    const size_t Q = t.q_path.size(), T = t.target_path.size();
    o.variant = SR_LIFT_VARIANT_HOST;
    o.tstart.assign(Q * T, 0); o.tend.assign(Q * T, 0); o.covered.assign(Q * T, 0); o.rev_bp.assign(Q * T, 0);
    if (!Q || !T) return SR_OK;
    std::vector<uint64_t> pstart(t.S, 0);
    for (uint32_t p = 0; p < t.P; p++) {
        uint64_t at = 0;
        for (uint32_t s = t.path_off[p]; s < t.path_off[p + 1]; s++) { pstart[s] = at; at += t.len[(t.steps[s] >> 1) - 1]; }
    }
    o.kernel_us[0] = (uint64_t)(us_since(t0) + 0.5);
    t0 = std::chrono::steady_clock::now();
    std::vector<std::vector<uint32_t>> first(T);
    for (size_t k = 0; k < T; k++) {
        const uint32_t b = t.target_path[k];
        first[k].assign(t.V, SR_LIFT_NONE);
        for (uint32_t s = t.path_off[b + 1]; s > t.path_off[b]; s--) first[k][(t.steps[s - 1] >> 1) - 1] = s - 1;     // the smallest index is written last
    }
    o.kernel_us[1] = (uint64_t)(us_since(t0) + 0.5);
    t0 = std::chrono::steady_clock::now();
    const SrLiftTables g{t.steps.data(), t.len.data(), pstart.data()};
    for (size_t i = 0; i < Q; i++) {
        const uint32_t a0 = t.path_off[t.q_path[i]], a1 = t.path_off[t.q_path[i] + 1];
        const uint32_t lo = sr_lift_step_of(pstart.data(), a0, a1, t.q_start[i]), hi = sr_lift_step_of(pstart.data(), a0, a1, t.q_end[i] - 1);
        for (size_t k = 0; k < T; k++) {
            SrLiftAcc acc = sr_lift_empty();
            for (uint32_t s = lo; s <= hi; s++) acc = sr_lift_join(acc, sr_lift_step(g, s, t.q_start[i], t.q_end[i], first[k][(t.steps[s] >> 1) - 1]));
            acc = sr_lift_finish(acc);
            o.tstart[i * T + k] = acc.lo; o.tend[i * T + k] = acc.hi; o.covered[i * T + k] = acc.covered; o.rev_bp[i * T + k] = acc.rev_bp;
        }
    }
    o.kernel_us[3] = (uint64_t)(us_since(t0) + 0.5);
    o.us = (uint64_t)(us_since(t_all) + 0.5);
    return SR_OK;
}

// ------------------------------------------------------------------ device execution
int lf_run_device(const LfTables &t, int device, void *stream, LfOutHost &o) {
    const uint32_t V = t.V, S = t.S, P = t.P, Q = (uint32_t)t.q_path.size(), T = (uint32_t)t.target_path.size();
    SrStage x("lift", "the lift tables");
    if (x.open(device, stream, 7)) return x.err;
    o.variant = SR_LIFT_VARIANT_DEVICE;
    const uint64_t pairs = (uint64_t)Q * T;                     // <= 2^26
    o.tstart.assign(pairs, 0); o.tend.assign(pairs, 0); o.covered.assign(pairs, 0); o.rev_bp.assign(pairs, 0);
    if (!pairs) return SR_OK;                                    // no query or no target: nothing to lift (a query implies a step)

    const uint64_t room = std::max(sr_scan_room(S), sr_scan_room(Q));
    uint32_t *d_len = x.alloc<uint32_t>(V), *d_steps = x.alloc<uint32_t>(S), *d_poff = x.alloc<uint32_t>((uint64_t)P + 1);
    u64d *d_sinc = x.alloc<u64d>(S), *d_pstart = x.alloc<u64d>(S), *d_sums = x.alloc<u64d>(room);
    uint32_t *d_first = x.alloc<uint32_t>((uint64_t)V * T, 0xff);
    uint32_t *d_qpath = x.alloc<uint32_t>(Q), *d_slo = x.alloc<uint32_t>(Q), *d_shi = x.alloc<uint32_t>(Q), *d_list = x.alloc<uint32_t>(Q);
    u64d *d_qstart = x.alloc<u64d>(Q), *d_qend = x.alloc<u64d>(Q), *d_long = x.alloc<u64d>(Q);
    LfOut out;
    out.tstart = x.alloc<u64d>(pairs); out.tend = x.alloc<u64d>(pairs); out.covered = x.alloc<u64d>(pairs); out.rev_bp = x.alloc<u64d>(pairs);
    if (x.err) return x.err;
    x.put(d_len, t.len.data(), (size_t)V * 4); x.put(d_steps, t.steps.data(), (size_t)S * 4); x.put(d_poff, t.path_off.data(), ((size_t)P + 1) * 4);
    x.put(d_qpath, t.q_path.data(), (size_t)Q * 4); x.put(d_qstart, t.q_start.data(), (size_t)Q * 8); x.put(d_qend, t.q_end.data(), (size_t)Q * 8);
    const SrLiftTables g{d_steps, d_len, d_pstart};
    const LfQueries q{d_qpath, d_qstart, d_qend, Q};
    const dim3 blk(LF_BLOCK), gs(sr_stage_grid(S)), gq(sr_stage_grid(Q));
    const bool single = t.to_named;
    const uint32_t f0 = single ? t.path_off[t.target_path[0]] : 0, f1 = single ? t.path_off[t.target_path[0] + 1] : S;

    x.mark(0);                                                   // ---- positions
    if (!x.err) {
        sr_step_len(x, d_steps, d_len, S, d_sinc);
        sr_scan<false>(x, d_sinc, S, d_sums);
        hipLaunchKernelGGL(lf_pstart_kernel, gs, blk, 0, x.st, (const uint32_t *)d_steps, (const uint32_t *)d_len, (const uint32_t *)d_poff, P,
                           (const u64d *)d_sinc, S, d_pstart);
    }
    x.mark(1);                                                   // ---- first visits
    if (!x.err && f1 > f0)
        hipLaunchKernelGGL(lf_first_kernel, dim3(sr_stage_grid(f1 - f0)), blk, 0, x.st, (const uint32_t *)d_steps, (const uint32_t *)d_poff, P, f0, f1, T,
                           single ? 1 : 0, d_first);
    x.mark(2);                                                   // ---- locate
    if (!x.err) {
        hipLaunchKernelGGL(lf_locate_kernel, gq, blk, 0, x.st, q, (const uint32_t *)d_poff, (const u64d *)d_pstart, (u64d)t.short_steps, d_slo, d_shi, d_long);
        sr_scan<false>(x, d_long, Q, d_sums);
        hipLaunchKernelGGL(lf_compact_kernel, gq, blk, 0, x.st, (const u64d *)d_long, Q, d_list);
    }
    x.mark(3);                                                   // ---- short pairs
    if (!x.err)
        hipLaunchKernelGGL(lf_short_kernel, dim3(sr_stage_grid(pairs)), blk, 0, x.st, g, q, (const uint32_t *)d_slo, (const uint32_t *)d_shi, (const u64d *)d_long,
                           (const uint32_t *)d_first, T, out);
    x.mark(4);                                                   // ---- long pairs
    if (!x.err)
        hipLaunchKernelGGL(lf_long_kernel, dim3(std::min<unsigned>(LF_LONG_BLOCKS, (unsigned)((pairs + LF_WAVES - 1) / LF_WAVES))), blk, 0, x.st, g, q,
                           (const uint32_t *)d_slo, (const uint32_t *)d_shi, (const u64d *)d_long, (const uint32_t *)d_list, (const uint32_t *)d_first, T, out);
    x.mark(5);
    x.chk(hipGetLastError());
    uint64_t n_long = 0;
    x.get(o.tstart.data(), out.tstart, (size_t)pairs * 8); x.get(o.tend.data(), out.tend, (size_t)pairs * 8);
    x.get(o.covered.data(), out.covered, (size_t)pairs * 8); x.get(o.rev_bp.data(), out.rev_bp, (size_t)pairs * 8);
    x.get(&n_long, d_long + (Q - 1), 8);
    x.mark(6);
    x.sync();                                                    // the synchronisation after the download, the only one
    if (x.err) return x.err;
    o.us = x.us(0, 6);
    for (int k = 0; k < 5; k++) o.kernel_us[k] = x.us(k, k + 1);
    o.long_pairs = n_long * T; o.short_pairs = pairs - o.long_pairs;
    return x.err;
}

sr_lift *lf_result(const LfTables &t, const LfOutHost &o) {
    sr_lift *r = (sr_lift *)calloc(1, sizeof(sr_lift));
    if (!r) return nullptr;
    const uint64_t Q = t.q_path.size(), T = t.target_path.size(), N = Q * T;
    uint64_t bytes = 0;
    for (const std::string &s : t.label) bytes += s.size();
    r->queries = Q; r->targets = T; r->paths = t.P; r->unknown = t.unknown; r->out_of_range = t.out_of_range;
    r->variant = o.variant; r->to_named = t.to_named ? 1 : 0; r->min_covered = t.min_covered;
    r->short_pairs = o.short_pairs; r->long_pairs = o.long_pairs; r->lift_us = o.us;
    for (int k = 0; k < 5; k++) r->kernel_us[k] = o.kernel_us[k];
    r->q_path = (uint32_t *)calloc(Q ? Q : 1, 4); r->q_start = (uint64_t *)calloc(Q ? Q : 1, 8); r->q_end = (uint64_t *)calloc(Q ? Q : 1, 8);
    r->label_off = (uint64_t *)calloc(Q + 1, 8); r->labels = (char *)calloc(bytes + 1, 1); r->target_path = (uint32_t *)calloc(T ? T : 1, 4);
    r->tstart = (uint64_t *)calloc(N ? N : 1, 8); r->tend = (uint64_t *)calloc(N ? N : 1, 8);
    r->covered = (uint64_t *)calloc(N ? N : 1, 8); r->rev_bp = (uint64_t *)calloc(N ? N : 1, 8);
    if (!r->q_path || !r->q_start || !r->q_end || !r->label_off || !r->labels || !r->target_path || !r->tstart || !r->tend || !r->covered || !r->rev_bp) {
        sr_lift_free(r);
        return nullptr;
    }
    uint64_t at = 0;
    for (uint64_t i = 0; i < Q; i++) {
        r->q_path[i] = t.q_path[i]; r->q_start[i] = t.q_start[i]; r->q_end[i] = t.q_end[i];
        memcpy(r->labels + at, t.label[i].data(), t.label[i].size());
        at += t.label[i].size();
        r->label_off[i + 1] = at;
    }
    for (uint64_t k = 0; k < T; k++) r->target_path[k] = t.target_path[k];
    if (N) {
        memcpy(r->tstart, o.tstart.data(), N * 8); memcpy(r->tend, o.tend.data(), N * 8);
        memcpy(r->covered, o.covered.data(), N * 8); memcpy(r->rev_bp, o.rev_bp.data(), N * 8);
    }
    for (uint64_t k = 0; k < N; k++) r->mapped += o.covered[k] != 0;
    return r;
}

}   // namespace

extern "C" void sr_lift_params_default(sr_lift_params *p) {
    if (!p) return;
    p->to_name = nullptr; p->min_covered = 1; p->short_steps = 8; p->reserved = 0;
}

extern "C" int sr_lift_gfa(const char *gfa_in, const char *bed_text, const sr_lift_params *p, int device, sr_lift **out) {
    if (!gfa_in || !bed_text || !p || !out) return sr_fail(SR_ERR_INVALID, "null argument");
    *out = nullptr;
    if (device < SR_LIFT_DEVICE_HOST) return sr_fail(SR_ERR_INVALID, "lift: device must be >= -1");
    try {
        SrGraph g;
        std::vector<std::string> names;
        int r = sr_graph_parse_gfa(gfa_in, g, names);
        if (r) return r;
        LfTables t;
        if ((r = lf_tables(g, names, *p, t))) return r;
        if ((r = lf_queries(bed_text, names, t))) return r;
        LfOutHost o;
        if ((r = device < 0 ? lf_run_host(t, o) : lf_run_device(t, device, nullptr, o))) return r;
        sr_lift *res = lf_result(t, o);
        if (!res) return sr_fail(SR_ERR_NOMEM, "not enough memory for the lift tables");
        *out = res;
    } catch (const std::bad_alloc &) {
        return sr_fail(SR_ERR_NOMEM, "not enough memory for the lift tables");
    }
    return SR_OK;
}

extern "C" void sr_lift_free(sr_lift *l) {
    if (!l) return;
    free(l->q_path); free(l->q_start); free(l->q_end); free(l->label_off); free(l->labels); free(l->target_path);
    free(l->tstart); free(l->tend); free(l->covered); free(l->rev_bp);
    free(l);
}

extern "C" int sr_lift_bed(const sr_lift *l, const char *const *names, char **text) {
    if (!l || !text || (l->paths && !names)) return sr_fail(SR_ERR_INVALID, "null argument");
    const uint64_t Q = l->queries, T = l->targets;
    if (Q * (T ? T : 1) > SR_LIFT_MAX_PAIRS) return sr_fail(SR_ERR_INVALID, "lift: not a result of sr_lift_gfa");
    try {
        std::string o;
        for (uint64_t i = 0; i < Q; i++) {
            const uint32_t a = l->q_path[i];
            for (uint64_t k = 0; k < T; k++) {
                const uint32_t b = l->target_path[k];
                const uint64_t n = i * T + k, cov = l->covered[n];
                if (a >= l->paths || b >= l->paths) return sr_fail(SR_ERR_INVALID, "lift: not a result of sr_lift_gfa");
                if (!cov || cov < l->min_covered || (a == b && !l->to_named)) continue;
                o += names[b]; o += "\t" + u64s(l->tstart[n]) + "\t" + u64s(l->tend[n]) + "\t";
                o.append(l->labels + l->label_off[i], l->label_off[i + 1] - l->label_off[i]);
                o += "\t" + u64s(cov) + "\t" + (sr_lift_reverse(cov, l->rev_bp[n]) ? "-" : "+") + "\t";
                o += names[a]; o += "\t" + u64s(l->q_start[i]) + "\t" + u64s(l->q_end[i]) + "\t" + u64s(l->rev_bp[n]) + "\n";
            }
        }
        return sr_give_text(o, text, "not enough memory for the lifted intervals");
    } catch (const std::bad_alloc &) {
        return sr_fail(SR_ERR_NOMEM, "not enough memory for the lifted intervals");
    }
    return SR_OK;
}
