// sr_extend.hip -- adding sequences to an existing GFA (--extend; include/seqrush_amd.h "extending a graph", DESIGN.md
// section 16).  The paths of the input graph are spelled back into sequences, and the partition the graph stands for is
// restored in the union-find of the merged set: per node offset, every base that visits it is united with the one the
// node's first step spells there.  After that only the pairs that touch a new sequence are aligned (sr_host.cpp
// sr_ctx_load_extend).  The kernels and the host twin share sr_extend_rule.h and nothing else.
//
// Device, two groups with hipEvents around each:
//   spell (the plan's own stream): step lengths -> inclusive u64 scan (block sums, recursing on the sums) -> one lane per
//         output base: bisection for its step in the scan, one byte loaded, complemented on a reverse step
//   seed  (the context's stream): anchor[] by atomicMin from one lane per step, then one lane per spelled base: bisection,
//         the rule, uf_unite (sr_uf_dev.h); unions attempted / joined are counted with one add per wave
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <unordered_set>
#include <vector>
#include "../../include/seqrush_amd.h"
#include "sr_internal.h"
#include "sr_sort.h"
#include "sr_stage_host.h"
#include "sr_stage_dev.h"
#include "sr_uf_dev.h"
#include "sr_extend.h"
#include "sr_extend_rule.h"

#define EX_BLOCK 256

typedef unsigned long long u64d;

static_assert(EX_BLOCK == SR_STAGE_BLOCK, "the grids of sr_stage_grid");

// ------------------------------------------------------------------ spell
// the step lengths and their inclusive scan: sr_stage_dev.h
__global__ void __launch_bounds__(EX_BLOCK) ex_spell_kernel(const uint32_t *steps, const uint32_t *len, const u64d *sinc, const uint64_t *seq_off,
                                                            const uint8_t *seq, uint32_t S, uint64_t bases, uint8_t *out) {
    const uint64_t x = (uint64_t)blockIdx.x * EX_BLOCK + threadIdx.x;
    if (x < bases) out[x] = sr_ext_spell(steps, len, (const uint64_t *)sinc, seq_off, seq, S, x);
}

// ------------------------------------------------------------------ seed
__global__ void __launch_bounds__(EX_BLOCK) ex_anchor_kernel(const uint32_t *steps, uint32_t S, uint32_t *anchor) {
    const uint32_t s = blockIdx.x * EX_BLOCK + threadIdx.x;
    if (s < S) atomicMin(&anchor[(steps[s] >> 1) - 1], s);
}

__global__ void __launch_bounds__(EX_BLOCK) ex_seed_kernel(SrExtendSeedArgs a) {
    const uint64_t x = (uint64_t)blockIdx.x * EX_BLOCK + threadIdx.x;
    uint64_t px = 0, py = 0;
    int err = 0;
    const bool tried = x < a.bases && sr_ext_seed_pair(a.steps, a.len, a.sinc, a.anchor, a.S, x, &px, &py);
    const bool joined = tried && uf_unite(a.nodes, px, py, err);
    const u64d mt = __ballot(tried), mj = __ballot(joined);
    if ((threadIdx.x & 63) == 0) {
        if (mt) atomicAdd(&a.counts[0], (u64d)__popcll(mt));
        if (mj) atomicAdd(&a.counts[1], (u64d)__popcll(mj));
    }
    if (err) atomicOr(a.error_flag, err);
}

int srk_extend_anchor(const SrExtendSeedArgs *a, void *stream) {
    if (!a->S) return 0;
    hipLaunchKernelGGL(ex_anchor_kernel, dim3(sr_stage_grid(a->S)), dim3(EX_BLOCK), 0, (hipStream_t)stream, a->steps, a->S, a->anchor);
    return (int)hipGetLastError();
}

int srk_extend_seed(const SrExtendSeedArgs *a, void *stream) {
    if (!a->bases) return 0;
    hipLaunchKernelGGL(ex_seed_kernel, dim3(sr_stage_grid(a->bases)), dim3(EX_BLOCK), 0, (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}

namespace {

// the node sequences back to back, as the spelling reads them
struct ExSeq { std::vector<uint64_t> off; std::vector<uint8_t> seq; };

// ------------------------------------------------------------------ host twin of the spell group
void ex_spell_host(sr_extend_plan &pl, const ExSeq &q) {
    const auto t0 = std::chrono::steady_clock::now();
    uint64_t at = 0;
    for (uint32_t s = 0; s < pl.S; s++) { at += pl.len[(pl.steps[s] >> 1) - 1]; pl.sinc[s] = at; }
    for (uint64_t x = 0; x < pl.old_bases; x++)
        pl.bases[x] = sr_ext_spell(pl.steps.data(), pl.len.data(), pl.sinc.data(), q.off.data(), q.seq.data(), pl.S, x);
    pl.spell_us = (uint64_t)(us_since(t0) + 0.5);
}

// ------------------------------------------------------------------ device execution of the spell group
int ex_spell_device(sr_extend_plan &pl, const ExSeq &q, int device) {
    SrStage x("extend", "the extend tables");
    if (x.open(device, nullptr, 2)) return x.err;             // the plan's own stream
    const uint32_t S = pl.S, V = pl.V;
    const uint64_t B = pl.old_bases;
    uint32_t *d_steps = x.alloc<uint32_t>(S), *d_len = x.alloc<uint32_t>(V);
    uint64_t *d_soff = x.alloc<uint64_t>((uint64_t)V + 1);
    uint8_t *d_seq = x.alloc<uint8_t>(q.seq.size()), *d_out = x.alloc<uint8_t>(B);
    u64d *d_sinc = x.alloc<u64d>(S), *d_sums = x.alloc<u64d>(sr_scan_room(S));
    if (x.err) return x.err;
    x.put(d_steps, pl.steps.data(), (size_t)S * 4); x.put(d_len, pl.len.data(), (size_t)V * 4);
    x.put(d_soff, q.off.data(), ((size_t)V + 1) * 8); x.put(d_seq, q.seq.data(), q.seq.size());
    x.mark(0);
    if (!x.err) {
        sr_step_len(x, d_steps, d_len, S, d_sinc);
        sr_scan<false>(x, d_sinc, S, d_sums);
        // B is the host's sum of the same lengths: the scan's last entry equals it
        hipLaunchKernelGGL(ex_spell_kernel, dim3(sr_stage_grid(B)), dim3(EX_BLOCK), 0, x.st, (const uint32_t *)d_steps, (const uint32_t *)d_len, (const u64d *)d_sinc,
                           (const uint64_t *)d_soff, (const uint8_t *)d_seq, S, B, d_out);
        x.chk(hipGetLastError());
    }
    x.mark(1);
    x.get(pl.bases.data(), d_out, B);                            // the one download: the front of the merged set
    x.get(pl.sinc.data(), d_sinc, (size_t)S * 8);
    x.sync();
    if (x.err) return x.err;
    pl.spell_us = x.us(0, 1);
    if (pl.sinc[S - 1] != B) return sr_fail(SR_ERR_DEVICE_FAULT, "extend: the device scan of the step lengths does not end at the number of old bases");
    return x.err;
}

// ------------------------------------------------------------------ the plan
int ex_plan(const char *gfa_in, const sr_seqset *nw, int device, sr_extend_plan &pl) {
    SrGraph g;
    std::vector<std::string> names;
    int r = sr_graph_parse_gfa(gfa_in, g, names);
    if (r) return sr_fail(r, std::string("extend: ") + sr_last_error());
    const uint64_t nn = g.node_seq.size() ? g.node_seq.size() - 1 : 0, ns = g.steps.size(), np = names.size();
    if (np == 0) return sr_fail(SR_ERR_INVALID, "extend: the GFA has no P line: there is no sequence to extend");
    const uint64_t n_new = nw ? nw->n : 0;
    if (nn >= 0x3fffffffULL || ns >= 0x7fffffffULL || np + n_new >= 0xffffffffULL)
        return sr_fail(SR_ERR_UNSUPPORTED, "extend supports < 2^30 nodes, < 2^31 steps and < 2^32 sequences");
    if (n_new && (!nw->bases || !nw->offsets || !nw->names)) return sr_fail(SR_ERR_INVALID, "extend: the new sequences need bases, offsets and names");
    std::unordered_set<std::string> seen;
    for (uint64_t p = 0; p < np; p++) {
        if (!seen.insert(names[p]).second) return sr_fail(SR_ERR_INVALID, "extend: two paths are named '" + names[p] + "'");
        if (g.path_off[p] == g.path_off[p + 1]) return sr_fail(SR_ERR_INVALID, "extend: path '" + names[p] + "' has no steps");
    }
    for (uint64_t i = 0; i < n_new; i++) {
        if (!nw->names[i]) return sr_fail(SR_ERR_INVALID, "extend: new sequence " + std::to_string(i) + " has no name");
        if (!seen.insert(nw->names[i]).second)
            return sr_fail(SR_ERR_INVALID, std::string("extend: the name '") + nw->names[i] + "' occurs twice (a path of the graph or another new sequence has it)");
    }
    pl.n_old = (uint32_t)np; pl.n_new = (uint32_t)n_new; pl.V = (uint32_t)nn; pl.S = (uint32_t)ns; pl.device = device;
    pl.steps = g.steps;
    pl.len.assign(nn, 0);
    ExSeq q;
    q.off.assign(nn + 1, 0);
    for (uint64_t v = 1; v <= nn; v++) {                          // `*` = no sequence: length 0, refused below if visited
        const std::string &sq = g.node_seq[v];
        if (sq != "*") { pl.len[v - 1] = (uint32_t)sq.size(); q.seq.insert(q.seq.end(), sq.begin(), sq.end()); }
        q.off[v] = q.seq.size();
    }
    uint64_t B = 0;
    pl.offsets.assign(1, 0);
    for (uint64_t p = 0; p < np; p++) {
        for (uint64_t s = g.path_off[p]; s < g.path_off[p + 1]; s++) {
            const uint32_t v = pl.steps[s] >> 1;
            if (v == 0 || v > nn)                                 // (the parser refuses these itself: kept as the bound of every table read)
                return sr_fail(SR_ERR_INVALID, "extend: step " + std::to_string(s - g.path_off[p]) + " of path '" + names[p] + "' names a missing node");
            if (pl.len[v - 1] == 0)
                return sr_fail(SR_ERR_INVALID, "extend: step " + std::to_string(s - g.path_off[p]) + " of path '" + names[p] + "' visits a node without a sequence (the " +
                                                   std::to_string(v) + ". S line in ascending id order)");
            B += pl.len[v - 1];
        }
        pl.offsets.push_back(B);
    }
    if (B >= SR_EXTEND_MAX_BASES) return sr_fail(SR_ERR_UNSUPPORTED, "extend supports < 2^39 bases in the paths of the input graph");
    pl.old_bases = B;
    const uint64_t NB = n_new ? nw->offsets[n_new] : 0;
    pl.bases.assign(B + NB, 0);
    pl.sinc.assign(ns, 0);
    r = device < 0 ? (ex_spell_host(pl, q), SR_OK) : ex_spell_device(pl, q, device);
    if (r) return r;
    if (NB) memcpy(pl.bases.data() + B, nw->bases, NB);
    for (uint64_t i = 0; i < n_new; i++) pl.offsets.push_back(B + nw->offsets[i + 1]);
    pl.names = names;
    for (uint64_t i = 0; i < n_new; i++) pl.names.emplace_back(nw->names[i]);
    for (const std::string &s : pl.names) pl.name_ptrs.push_back(s.c_str());
    pl.merged = sr_seqset{(uint32_t)(np + n_new), pl.bases.data(), pl.offsets.data(), pl.name_ptrs.data()};
    return SR_OK;
}

}   // namespace

extern "C" int sr_extend_plan_gfa(const char *gfa_in, const sr_seqset *new_seqs, int device, sr_extend_plan **out) {
    if (!gfa_in || !out) return sr_fail(SR_ERR_INVALID, "null argument");
    *out = nullptr;
    if (device < SR_EXTEND_DEVICE_HOST) return sr_fail(SR_ERR_INVALID, "extend: device must be >= -1");
    sr_extend_plan *pl = nullptr;
    try {
        pl = new sr_extend_plan();
        const int r = ex_plan(gfa_in, new_seqs, device, *pl);
        if (r) { delete pl; return r; }
    } catch (const std::bad_alloc &) {
        delete pl;
        return sr_fail(SR_ERR_NOMEM, "not enough memory for the extend plan");
    }
    *out = pl;
    return SR_OK;
}

extern "C" void sr_extend_plan_free(sr_extend_plan *plan) { delete plan; }
extern "C" const sr_seqset *sr_extend_plan_seqs(const sr_extend_plan *plan) { return plan ? &plan->merged : nullptr; }
extern "C" uint32_t sr_extend_plan_n_old(const sr_extend_plan *plan) { return plan ? plan->n_old : 0; }

extern "C" int sr_extend_plan_stats(const sr_extend_plan *plan, sr_extend_stats *out) {
    if (!plan || !out) return sr_fail(SR_ERR_INVALID, "null argument");
    memset(out, 0, sizeof(*out));
    out->old_paths = plan->n_old; out->old_bases = plan->old_bases; out->old_steps = plan->S; out->new_sequences = plan->n_new;
    out->spell_us = plan->spell_us;
    return SR_OK;
}

extern "C" int sr_extend_pair_list(const sr_extend_plan *plan, const uint32_t *q, const uint32_t *t, uint64_t count, uint32_t **q_out,
                                   uint32_t **t_out, uint64_t *count_out) {
    if (!plan || !q_out || !t_out || !count_out || (count && (!q || !t))) return sr_fail(SR_ERR_INVALID, "null argument");
    const uint32_t n = plan->merged.n;
    uint64_t kept = 0;
    for (uint64_t i = 0; i < count; i++) {
        if (q[i] >= n || t[i] >= n) return sr_fail(SR_ERR_INVALID, "extend: pair index out of range");
        kept += sr_ext_keep_pair(q[i], t[i], plan->n_old);
    }
    uint32_t *qo = (uint32_t *)malloc((kept ? kept : 1) * 4), *to = (uint32_t *)malloc((kept ? kept : 1) * 4);
    if (!qo || !to) { free(qo); free(to); return sr_fail(SR_ERR_NOMEM, "not enough memory for the pair list"); }
    uint64_t w = 0;
    for (uint64_t i = 0; i < count; i++)
        if (sr_ext_keep_pair(q[i], t[i], plan->n_old)) { qo[w] = q[i]; to[w] = t[i]; w++; }
    *q_out = qo; *t_out = to; *count_out = kept;
    return SR_OK;
}

// the twin of the seed group: the same rule in index order through sr_uf_unite_host
extern "C" int sr_extend_seed_host(const sr_extend_plan *plan, uint64_t *nodes, uint64_t n, uint64_t stats[2]) {
    if (!plan || !nodes) return sr_fail(SR_ERR_INVALID, "null argument");
    if (n < 2 * (uint64_t)plan->bases.size() + 2) return sr_fail(SR_ERR_INVALID, "node array shorter than 2 * total length of the merged set + 2");
    try {
        std::vector<uint32_t> anchor(plan->V, SR_EXTEND_NO_ANCHOR);
        for (uint32_t s = plan->S; s-- > 0;) anchor[(plan->steps[s] >> 1) - 1] = s;
        uint64_t tried = 0, joined = 0;
        for (uint64_t x = 0; x < plan->old_bases; x++) {
            uint64_t px, py;
            if (!sr_ext_seed_pair(plan->steps.data(), plan->len.data(), plan->sinc.data(), anchor.data(), plan->S, x, &px, &py)) continue;
            const int r = sr_uf_unite_host(nodes, n, px, py);
            if (r < 0) return r;
            tried++; joined += (uint64_t)r;
        }
        if (stats) { stats[0] = tried; stats[1] = joined; }
    } catch (const std::bad_alloc &) {
        return sr_fail(SR_ERR_NOMEM, "not enough memory for the anchor table");
    }
    return SR_OK;
}
