// sr_variants.hip -- reference-anchored variant sites and genotypes (--vcf; include/seqrush_amd.h "variant sites",
// DESIGN.md section 15): where the paths of a graph differ from one of them, and which allele every path carries, on the
// device and, in plain loops over the same rule header, on the host.  Every quantity is an integer or a byte string, so
// the two agree exactly.  The final numbering of a site's alleles by (length, bytes), the allele arena and the VCF text are
// formed here on the host, once for every front end.
//
// Device: six groups of kernels on one stream, hipEvents around them: anchors (visits of the reference, step positions) ->
// scan (previous anchor step of every step: a max scan whose segments are cut at the path offsets) -> emit (classify, count,
// scan, scatter: records leave in (path, step) order) -> hash (one lane per traversal) -> sort and classes (stable rocPRIM
// radix passes, then allele bytes against the predecessor's and against the reference) -> genotypes (runs write 0, the
// first traversal of every (site, path) writes its allele).  No atomic decides an order: the only atomics are integer
// counters.  Two 8-byte counts come back in between (the traversals size the sort, the sites size the table), then one
// synchronisation after the download.  No captured graph.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <string>
#include <vector>
#include "../../include/seqrush_amd.h"
#include "sr_internal.h"
#include "sr_sort.h"
#include "sr_stage_host.h"
#include "sr_stage_dev.h"
#include "sr_variants_rule.h"

#define VA_BLOCK 256

typedef unsigned long long u64d;

static_assert(VA_BLOCK == SR_STAGE_BLOCK, "the grids of sr_stage_grid");

// ------------------------------------------------------------------ tables on the device
struct VaDev {
    SrVarGraph g;
    const uint32_t *path_off;                  // [P + 1]
    const uint32_t *visits;                    // [V] steps of the reference on the node
    const uint32_t *ref_pr;                    // [V] ref_pos << 1 | ref_or of an anchor
    const u64d *spos;                          // [S] inclusive scan of the step lengths
    const u64d *prev;                          // [S] inclusive max scan of (anchor step ? index + 1 : 0)
    uint32_t V, S, P;
    uint64_t max_len, hash_mask;
};

__device__ __forceinline__ u64d va_spos_ex(const VaDev &d, uint32_t s) { return s ? d.spos[s - 1] : 0; }

// one add per wave and path: the lanes with `flag` are grouped by path through ballots; call from uniform control flow
__device__ __forceinline__ void va_count_by_path(bool flag, uint32_t p, u64d *table) {
    u64d m = __ballot(flag);
    while (m) {
        const int first = __ffsll(m) - 1;
        const uint32_t p0 = __shfl(p, first, 64);
        const u64d same = __ballot(flag && p == p0);
        if ((int)(threadIdx.x & 63) == first) atomicAdd(&table[p0], (u64d)__popcll(same));
        m &= ~same;
    }
}

// ------------------------------------------------------------------ group 0: anchors
// the step lengths and the scans (sum and max): sr_stage_dev.h
__global__ void __launch_bounds__(VA_BLOCK) va_visits_kernel(const uint32_t *steps, uint32_t s0, uint32_t s1, uint32_t *visits) {
    const uint32_t s = s0 + blockIdx.x * VA_BLOCK + threadIdx.x;
    if (s < s1) atomicAdd(&visits[(steps[s] >> 1) - 1], 1u);
}

__global__ void __launch_bounds__(VA_BLOCK) va_refpos_kernel(VaDev d, uint32_t s0, uint32_t s1, uint32_t *ref_pr, u64d *anchors) {
    const uint32_t s = s0 + blockIdx.x * VA_BLOCK + threadIdx.x;
    bool anchor = false;
    if (s < s1) {
        const uint32_t h = d.g.steps[s], v = (h >> 1) - 1;
        anchor = d.visits[v] == 1;
        if (anchor) ref_pr[v] = (uint32_t)(va_spos_ex(d, s) - va_spos_ex(d, s0)) << 1 | (h & 1u);
    }
    const u64d m = __ballot(anchor);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(anchors, (u64d)__popcll(m));
}

// ------------------------------------------------------------------ group 1: the previous anchor step
__global__ void __launch_bounds__(VA_BLOCK) va_mark_kernel(const uint32_t *steps, const uint32_t *visits, uint32_t S, u64d *out) {
    const uint32_t s = blockIdx.x * VA_BLOCK + threadIdx.x;
    if (s < S) out[s] = visits[(steps[s] >> 1) - 1] == 1 ? (u64d)s + 1 : 0;
}

// ------------------------------------------------------------------ group 2: emit
struct VaPair { int cls; uint32_t i, a, b, strand; uint64_t alen; };

// the pair that ends on anchor step j of path p: cls = -1 when j has no anchor step before it in its path
__device__ __forceinline__ VaPair va_pair(const VaDev &d, uint32_t j, uint32_t p) {
    VaPair r; r.cls = -1; r.i = SR_VARIANTS_NONE; r.a = r.b = 0; r.strand = 0; r.alen = 0;
    const u64d before = j ? d.prev[j - 1] : 0;                 // index + 1 of the last anchor step before j, any path
    if (before < (u64d)d.path_off[p] + 1) return r;
    const uint32_t i = (uint32_t)(before - 1);
    const uint32_t hi = d.g.steps[i], hj = d.g.steps[j], vi = (hi >> 1) - 1, vj = (hj >> 1) - 1;
    const uint32_t pri = d.ref_pr[vi], prj = d.ref_pr[vj];
    r.i = i; r.strand = (hj & 1u) ^ (prj & 1u);
    r.alen = va_spos_ex(d, j) - d.spos[i];
    r.cls = sr_var_classify((hi & 1u) ^ (pri & 1u), r.strand, pri >> 1, (pri >> 1) + d.g.len[vi], prj >> 1, (prj >> 1) + d.g.len[vj], r.alen,
                            d.max_len, &r.a, &r.b);
    return r;
}

#define VA_F_ANCHOR 1u
#define VA_F_TRAV 2u
#define VA_F_HEAD 4u
// cls[s]: anchor step, traversal ends here, head of a run; cnt[s] = traversal | run head << 32 for the scan
__global__ void __launch_bounds__(VA_BLOCK) va_classify_kernel(VaDev d, uint8_t *cls, u64d *cnt, u64d *breaks, u64d *skipped) {
    const uint32_t s = blockIdx.x * VA_BLOCK + threadIdx.x;
    const bool live = s < d.S;
    uint32_t p = 0, f = 0;
    bool brk = false, skp = false;
    if (live && d.visits[(d.g.steps[s] >> 1) - 1] == 1) {
        p = sr_path_of(d.path_off, d.P, s);
        const VaPair q = va_pair(d, s, p);
        brk = q.cls == SR_VAR_BREAK; skp = q.cls == SR_VAR_SKIPPED;
        f = VA_F_ANCHOR | (q.cls == SR_VAR_TRAVERSAL ? VA_F_TRAV : 0u) | (q.cls == SR_VAR_ADJACENT && q.i + 1 == s ? 0u : VA_F_HEAD);
    }
    if (live) { cls[s] = (uint8_t)f; cnt[s] = (u64d)((f & VA_F_TRAV) ? 1 : 0) | (u64d)((f & VA_F_HEAD) ? 1 : 0) << 32; }
    va_count_by_path(brk, p, breaks);
    va_count_by_path(skp, p, skipped);
}

struct VaRec { uint32_t *i, *j, *a, *b, *len, *path; uint8_t *strand; };
struct VaRuns { uint32_t *head, *tail, *path; };

// cnt is now the inclusive scan: traversal k = low word - 1, run = high word - 1
__global__ void __launch_bounds__(VA_BLOCK) va_scatter_kernel(VaDev d, const uint8_t *cls, const u64d *cnt, VaRec rec, VaRuns runs) {
    const uint32_t s = blockIdx.x * VA_BLOCK + threadIdx.x;
    if (s >= d.S) return;
    const uint32_t f = cls[s];
    if (!(f & VA_F_ANCHOR)) return;
    const uint32_t p = sr_path_of(d.path_off, d.P, s);
    const u64d c = cnt[s];
    if (f & VA_F_TRAV) {
        const VaPair q = va_pair(d, s, p);
        const uint32_t k = (uint32_t)c - 1;
        rec.i[k] = q.i; rec.j[k] = s; rec.a[k] = q.a; rec.b[k] = q.b; rec.len[k] = (uint32_t)q.alen; rec.path[k] = p; rec.strand[k] = (uint8_t)q.strand;
    }
    const uint32_t run = (uint32_t)(c >> 32) - 1;                // every anchor step lies in a run: its head is at or before s
    if (f & VA_F_HEAD) { runs.head[run] = s; runs.path[run] = p; }
    const bool tail = s + 1 >= d.path_off[p + 1] || !(cls[s + 1] & VA_F_ANCHOR) || (cls[s + 1] & VA_F_HEAD);
    if (tail) runs.tail[run] = s;
}

// ------------------------------------------------------------------ group 3: the allele hash
__global__ void __launch_bounds__(VA_BLOCK) va_hash_kernel(VaDev d, VaRec rec, uint32_t T, u64d *hash, uint32_t *iota) {
    const uint32_t k = blockIdx.x * VA_BLOCK + threadIdx.x;
    if (k >= T) return;
    SrVarWalk w(&d.g, rec.i[k], rec.j[k], rec.strand[k]);
    const uint32_t n = rec.len[k];
    u64d h = SR_VAR_HASH_SEED;
    for (uint32_t x = 0; x < n; x++) h = sr_var_hash_step(h, w.next());
    hash[k] = sr_var_hash_end(h, n) & d.hash_mask;
    iota[k] = k;
}

// ------------------------------------------------------------------ group 4: sort and classes
__global__ void __launch_bounds__(VA_BLOCK) va_key_len_kernel(const uint32_t *perm, const uint32_t *len, uint32_t T, uint32_t *key) {
    const uint32_t k = blockIdx.x * VA_BLOCK + threadIdx.x;
    if (k < T) key[k] = len[perm[k]];
}
__global__ void __launch_bounds__(VA_BLOCK) va_key_ab_kernel(const uint32_t *perm, const uint32_t *a, const uint32_t *b, uint32_t T, u64d *key) {
    const uint32_t k = blockIdx.x * VA_BLOCK + threadIdx.x;
    if (k < T) { const uint32_t r = perm[k]; key[k] = (u64d)a[r] << 32 | b[r]; }
}

#define VA_C_SITE 1u           // first record of its site
#define VA_C_SAME 2u           // same key and the same bytes as the predecessor
#define VA_C_CLASH 4u          // same key, other bytes: the hashes collided
#define VA_C_REF 8u            // the bytes of refseq[a:b]
#define VA_C_HEAD 16u          // first record of its allele class (set by va_class_kernel)
__global__ void __launch_bounds__(VA_BLOCK) va_compare_kernel(VaDev d, VaRec rec, const uint32_t *perm, const u64d *hash, const uint8_t *refseq,
                                                              uint32_t T, uint8_t *flags, u64d *site_in) {
    const uint32_t k = blockIdx.x * VA_BLOCK + threadIdx.x;
    if (k >= T) return;
    const uint32_t r = perm[k], n = rec.len[r], a = rec.a[r], b = rec.b[r];
    uint32_t f = 0;
    if (k == 0) f = VA_C_SITE;
    else {
        const uint32_t q = perm[k - 1];
        if (rec.a[q] != a || rec.b[q] != b) f = VA_C_SITE;
        else if (rec.len[q] == n && hash[q] == hash[r]) {
            SrVarWalk x(&d.g, rec.i[r], rec.j[r], rec.strand[r]), y(&d.g, rec.i[q], rec.j[q], rec.strand[q]);
            bool eq = true;
            for (uint32_t t = 0; t < n && eq; t++) eq = x.next() == y.next();
            f = eq ? VA_C_SAME : VA_C_CLASH;
        }
    }
    if (n == b - a && !(f & VA_C_SAME)) {
        SrVarWalk x(&d.g, rec.i[r], rec.j[r], rec.strand[r]);
        bool eq = true;
        for (uint32_t t = 0; t < n && eq; t++) eq = x.next() == refseq[a + t];
        if (eq) f |= VA_C_REF;
    }
    flags[k] = (uint8_t)f;
    site_in[k] = f & VA_C_SITE;
}

__global__ void __launch_bounds__(VA_BLOCK) va_clash_kernel(const uint8_t *flags, const u64d *site, uint32_t T, uint32_t *coll) {
    const uint32_t k = blockIdx.x * VA_BLOCK + threadIdx.x;
    if (k < T && (flags[k] & VA_C_CLASH)) coll[(uint32_t)site[k] - 1] = 1;     // every writer stores the same value
}

__global__ void __launch_bounds__(VA_BLOCK) va_class_kernel(VaDev d, VaRec rec, const uint32_t *perm, const uint8_t *refseq, uint8_t *flags,
                                                            const u64d *site, const uint32_t *coll, uint32_t T, uint32_t *keep, u64d *class_in) {
    const uint32_t k = blockIdx.x * VA_BLOCK + threadIdx.x;
    if (k >= T) return;
    uint32_t f = flags[k];
    const uint32_t sx = (uint32_t)site[k] - 1;
    const bool head = (f & VA_C_SITE) || !(f & VA_C_SAME) || coll[sx];
    if (head && (f & VA_C_SAME)) {                               // a site with a collision: every record is its own class
        const uint32_t r = perm[k], n = rec.len[r], a = rec.a[r];
        f &= ~VA_C_SAME;
        if (n == rec.b[r] - a) {
            SrVarWalk x(&d.g, rec.i[r], rec.j[r], rec.strand[r]);
            bool eq = true;
            for (uint32_t t = 0; t < n && eq; t++) eq = x.next() == refseq[a + t];
            if (eq) f |= VA_C_REF;
        }
    }
    if (head) f |= VA_C_HEAD;
    flags[k] = (uint8_t)f;
    const bool alt = head && !(f & VA_C_REF);
    if (alt) keep[sx] = 1;
    class_in[k] = (u64d)(alt ? 1 : 0) | (u64d)(head ? 1 : 0) << 32;
}

// cls is now the inclusive scan: ALT classes in the low word, classes in the high word.  Per class (at its index): is it
// the reference allele; per site (at its index): the ALT classes before it, and the scan input kept | collision << 32
__global__ void __launch_bounds__(VA_BLOCK) va_site_kernel(const uint8_t *flags, const u64d *site, const u64d *cls, const uint32_t *keep,
                                                           const uint32_t *coll, uint32_t T, uint32_t *base, uint32_t *cref, u64d *site_out_in) {
    const uint32_t k = blockIdx.x * VA_BLOCK + threadIdx.x;
    if (k >= T) return;
    if (flags[k] & VA_C_HEAD) cref[(uint32_t)(cls[k] >> 32) - 1] = (flags[k] & VA_C_REF) ? 1u : 0u;
    if (!(flags[k] & VA_C_SITE)) return;
    const uint32_t sx = (uint32_t)site[k] - 1;
    const bool alt = (flags[k] & VA_C_HEAD) && !(flags[k] & VA_C_REF);
    base[sx] = (uint32_t)cls[k] - (alt ? 1u : 0u);
    site_out_in[sx] = (u64d)(keep[sx] ? 1 : 0) | (u64d)(keep[sx] && coll[sx] ? 1 : 0) << 32;
}

// a record that does not head its class has the counts of its head: no head lies between them
__global__ void __launch_bounds__(VA_BLOCK) va_number_kernel(VaRec rec, const uint32_t *perm, const uint8_t *flags, const u64d *site, const u64d *cls,
                                                             const uint32_t *keep, const uint32_t *base, const uint32_t *cref, const u64d *site_out, uint32_t T,
                                                             uint32_t *pos_site, uint32_t *pos_allele, uint32_t *rec_site, uint32_t *rec_allele,
                                                             uint32_t *out_a, uint32_t *out_b) {
    const uint32_t k = blockIdx.x * VA_BLOCK + threadIdx.x;
    if (k >= T) return;
    const uint32_t sx = (uint32_t)site[k] - 1, r = perm[k];
    if (!keep[sx]) { pos_site[k] = SR_VARIANTS_NONE; pos_allele[k] = 0; rec_site[r] = SR_VARIANTS_NONE; rec_allele[r] = 0; return; }
    const uint32_t allele = cref[(uint32_t)(cls[k] >> 32) - 1] ? 0u : (uint32_t)cls[k] - base[sx];
    const uint32_t os = (uint32_t)site_out[sx] - 1;
    pos_site[k] = os; pos_allele[k] = allele; rec_site[r] = os; rec_allele[r] = allele;
    if (flags[k] & VA_C_SITE) { out_a[os] = rec.a[r]; out_b[os] = rec.b[r]; }
}

// ------------------------------------------------------------------ group 5: genotypes
// one lane per run: the sites with lo < a and b < hi, found by bisection on a (the sites are in (a, b) order), get 0.  A
// lane writes the first VA_RUN_OWN sites of its run itself; what is left of a long run is walked by the whole wave, run by
// run, so a path that follows the reference for thousands of sites does not hold one lane for all of them.
#define VA_RUN_OWN 4
__global__ void __launch_bounds__(VA_BLOCK) va_runs_kernel(VaDev d, VaRuns runs, uint32_t n_runs, const uint32_t *out_a, const uint32_t *out_b,
                                                           uint32_t n_sites, int32_t *gt) {
    const uint32_t run = blockIdx.x * VA_BLOCK + threadIdx.x, lane = threadIdx.x & 63;
    uint32_t x = n_sites, hi = 0, p = 0;                          // x: the next site of the run; no run: none
    if (run < n_runs) {
        const uint32_t hs = d.g.steps[runs.head[run]], ts = d.g.steps[runs.tail[run]], hv = (hs >> 1) - 1, tv = (ts >> 1) - 1;
        const uint32_t strand = (hs & 1u) ^ (d.ref_pr[hv] & 1u);
        const uint32_t first = strand ? tv : hv, last = strand ? hv : tv;
        const uint32_t lo = d.ref_pr[first] >> 1;
        hi = (d.ref_pr[last] >> 1) + d.g.len[last];
        uint32_t y = n_sites;                                     // first site with a > lo
        x = 0;
        while (x < y) {
            const uint32_t mid = (x + y) >> 1;
            if (out_a[mid] > lo) y = mid; else x = mid + 1;
        }
        p = runs.path[run];
    }
    for (int k = 0; k < VA_RUN_OWN && x < n_sites && out_a[x] < hi; k++, x++)
        if (out_b[x] < hi) gt[(uint64_t)x * d.P + p] = 0;
    u64d m = __ballot(x < n_sites && out_a[x] < hi);
    while (m) {                                                   // wave-uniform
        const int src = __ffsll(m) - 1;
        const uint32_t x0 = __shfl(x, src, 64), hi0 = __shfl(hi, src, 64), p0 = __shfl(p, src, 64);
        for (uint32_t s = x0 + lane; s < n_sites && out_a[s] < hi0; s += 64)
            if (out_b[s] < hi0) gt[(uint64_t)s * d.P + p0] = 0;
        m &= m - 1;
    }
}

// the records in (site, path, step) order: the first of every (site, path) writes
__global__ void __launch_bounds__(VA_BLOCK) va_gt_kernel(const uint32_t *site_sorted, const uint32_t *order, const uint32_t *rec_path,
                                                         const uint32_t *rec_allele, uint32_t T, uint32_t P, int32_t *gt) {
    const uint32_t m = blockIdx.x * VA_BLOCK + threadIdx.x;
    if (m >= T) return;
    const uint32_t s = site_sorted[m], r = order[m];
    if (s == SR_VARIANTS_NONE) return;
    if (m && site_sorted[m - 1] == s && rec_path[order[m - 1]] == rec_path[r]) return;
    gt[(uint64_t)s * P + rec_path[r]] = (int32_t)rec_allele[r];
}

namespace {

// the tables both executions read.  Node v = 1..V sits at index v - 1.
struct VaTables : SrPathTables {
    uint32_t R = 0;
    uint64_t max_len = 0, hash_mask = ~0ULL;
    std::vector<uint64_t> seq_off;
    std::vector<uint8_t> seq;
    std::string refseq;
    SrVarGraph view() const { return SrVarGraph{steps.data(), len.data(), seq_off.data(), seq.data()}; }
};

// what both executions hand to va_result
struct VaSite { uint32_t a = 0, b = 0; std::vector<std::string> alts; };
struct VaOut {
    uint64_t anchors = 0, traversals = 0, collisions = 0, us = 0, kernel_us[6] = {0, 0, 0, 0, 0, 0};
    int variant = 0;
    std::vector<uint64_t> breaks, skipped;
    std::vector<VaSite> sites;
    std::vector<int32_t> gt;
};

int va_tables(const SrGraph &g, const std::vector<std::string> &names, const sr_variant_params &prm, VaTables &t) {
    const SrPathSizes z = sr_path_sizes(g);
    const uint64_t nn = z.nodes, np = z.paths;
    if (nn >= 0x3fffffffULL || z.steps >= 0x7fffffffULL || np >= 0x7fffffffULL || z.bases >= 0x7fffffffULL)
        return sr_fail(SR_ERR_UNSUPPORTED, "variants support < 2^30 nodes and < 2^31 steps, paths and bases");
    t.max_len = prm.max_allele_len; t.hash_mask = prm.hash_mask;
    if (prm.ref_name) {
        const uint64_t p = sr_path_by_name(names, np, prm.ref_name);
        if (p == np) return sr_fail(SR_ERR_INVALID, std::string("variants: no path is named '") + prm.ref_name + "'");
        t.R = (uint32_t)p;
    }
    if (const int r = sr_path_tables_fill(g, z, "variants", true, false, t)) return r;
    t.seq_off.assign(nn + 1, 0); t.seq.reserve(z.bases);
    for (uint64_t v = 1; v <= nn; v++) {
        t.seq.insert(t.seq.end(), g.node_seq[v].begin(), g.node_seq[v].end());
        t.seq_off[v] = t.seq.size();
    }
    if (np) {
        uint64_t L = 0;
        for (uint32_t s = t.path_off[t.R]; s < t.path_off[t.R + 1]; s++) L += t.len[(t.steps[s] >> 1) - 1];
        if (L >= 0x7fffffffULL) return sr_fail(SR_ERR_UNSUPPORTED, "variants support a reference path of < 2^31 bases");
        t.refseq.reserve(L);
        for (uint32_t s = t.path_off[t.R]; s < t.path_off[t.R + 1]; s++) {
            const uint32_t h = t.steps[s], v = (h >> 1) - 1;
            for (uint32_t k = 0; k < t.len[v]; k++) t.refseq.push_back((char)sr_var_handle_byte(t.seq.data() + t.seq_off[v], t.len[v], h & 1u, k));
        }
    }
    return SR_OK;
}

std::string va_allele(const SrVarGraph &g, uint32_t i, uint32_t j, uint32_t strand, uint64_t n) {
    std::string s;
    s.reserve(n);
    SrVarWalk w(&g, i, j, strand);
    for (uint64_t k = 0; k < n; k++) s.push_back((char)w.next());
    return s;
}

bool va_allele_less(const std::string &x, const std::string &y) { return x.size() != y.size() ? x.size() < y.size() : x < y; }

// ------------------------------------------------------------------ host twin: plain loops, allele bytes compared directly
int va_run_host(const VaTables &t, VaOut &o) {
    const auto t_all = std::chrono::steady_clock::now();
    auto t0 = t_all;
    const SrVarGraph g = t.view();
    const uint32_t P = t.P;
    o.variant = SR_VARIANTS_VARIANT_HOST;
    o.breaks.assign(P, 0); o.skipped.assign(P, 0);
    if (!P) return SR_OK;
    std::vector<uint32_t> visits(t.V, 0), ref_pos(t.V, 0), ref_or(t.V, 0);
    uint32_t at = 0;
    for (uint32_t s = t.path_off[t.R]; s < t.path_off[t.R + 1]; s++) {
        const uint32_t v = (t.steps[s] >> 1) - 1;
        visits[v]++; ref_pos[v] = at; ref_or[v] = t.steps[s] & 1u;
        at += t.len[v];
    }
    for (uint32_t v = 0; v < t.V; v++) o.anchors += visits[v] == 1;
    o.kernel_us[0] = (uint64_t)(us_since(t0) + 0.5);
    t0 = std::chrono::steady_clock::now();
    struct Trav { uint32_t path, step; std::string allele; };
    struct Run { uint32_t path, lo, hi; };
    std::map<std::pair<uint32_t, uint32_t>, std::vector<Trav>> by_site;     // traversals arrive in (path, step) order
    std::vector<Run> runs;
    for (uint32_t p = 0; p < P; p++) {
        uint32_t i = SR_VARIANTS_NONE;
        uint64_t between = 0;                                    // bytes of the steps after i
        bool in_run = false;
        Run run{p, 0, 0};
        for (uint32_t j = t.path_off[p]; j < t.path_off[p + 1]; j++) {
            const uint32_t vj = (t.steps[j] >> 1) - 1;
            if (visits[vj] != 1) { between += t.len[vj]; if (in_run) { runs.push_back(run); in_run = false; } continue; }
            const uint32_t sj = (t.steps[j] & 1u) ^ ref_or[vj], pj = ref_pos[vj], ej = pj + t.len[vj];
            bool joins = false;
            if (i != SR_VARIANTS_NONE) {
                const uint32_t vi = (t.steps[i] >> 1) - 1;
                uint32_t a = 0, b = 0;
                const int cls = sr_var_classify((t.steps[i] & 1u) ^ ref_or[vi], sj, ref_pos[vi], ref_pos[vi] + t.len[vi], pj, ej, between, t.max_len, &a, &b);
                if (cls == SR_VAR_BREAK) o.breaks[p]++;
                else if (cls == SR_VAR_SKIPPED) o.skipped[p]++;
                else if (cls == SR_VAR_TRAVERSAL) { by_site[{a, b}].push_back(Trav{p, i, va_allele(g, i, j, sj, between)}); o.traversals++; }
                else joins = i + 1 == j;
            }
            if (joins) { run.lo = std::min(run.lo, pj); run.hi = std::max(run.hi, ej); }
            else { if (in_run) runs.push_back(run); run = Run{p, pj, ej}; in_run = true; }
            i = j; between = 0;
        }
        if (in_run) runs.push_back(run);
    }
    o.kernel_us[2] = (uint64_t)(us_since(t0) + 0.5);
    t0 = std::chrono::steady_clock::now();
    std::vector<const std::vector<Trav> *> kept;
    for (const auto &kv : by_site) {
        const uint32_t a = kv.first.first, b = kv.first.second;
        const std::string ref = t.refseq.substr(a, b - a);
        VaSite site; site.a = a; site.b = b;
        for (const Trav &tr : kv.second) if (tr.allele != ref) site.alts.push_back(tr.allele);
        std::sort(site.alts.begin(), site.alts.end(), va_allele_less);
        site.alts.erase(std::unique(site.alts.begin(), site.alts.end()), site.alts.end());
        if (site.alts.empty()) continue;
        o.sites.push_back(site); kept.push_back(&kv.second);
    }
    if ((uint64_t)o.sites.size() * P > SR_VARIANTS_MAX_CELLS)
        return sr_fail(SR_ERR_UNSUPPORTED, "variants: " + std::to_string(o.sites.size()) + " sites x " + std::to_string(P) + " paths; the table supports at most 2^26 cells");
    o.kernel_us[4] = (uint64_t)(us_since(t0) + 0.5);
    t0 = std::chrono::steady_clock::now();
    o.gt.assign(o.sites.size() * (size_t)P, -1);
    for (const Run &r : runs) {
        size_t x = std::upper_bound(o.sites.begin(), o.sites.end(), r.lo, [](uint32_t lo, const VaSite &s) { return lo < s.a; }) - o.sites.begin();
        for (; x < o.sites.size() && o.sites[x].a < r.hi; x++)
            if (o.sites[x].b < r.hi) o.gt[x * P + r.path] = 0;
    }
    for (size_t x = 0; x < o.sites.size(); x++) {
        const VaSite &site = o.sites[x];
        const std::string ref = t.refseq.substr(site.a, site.b - site.a);
        std::vector<uint8_t> seen(P, 0);
        for (const Trav &tr : *kept[x]) {
            if (seen[tr.path]) continue;                         // the smallest step index of the path came first
            seen[tr.path] = 1;
            o.gt[x * P + tr.path] = tr.allele == ref ? 0
                : (int32_t)(std::lower_bound(site.alts.begin(), site.alts.end(), tr.allele, va_allele_less) - site.alts.begin()) + 1;
        }
    }
    o.kernel_us[5] = (uint64_t)(us_since(t0) + 0.5);
    o.us = (uint64_t)(us_since(t_all) + 0.5);
    return SR_OK;
}

// ------------------------------------------------------------------ device execution
template <class K> void va_sort(SrStage &x, void *temp, size_t temp_bytes, K *kin, K *kout, uint32_t *vin, uint32_t *vout, uint32_t n, unsigned bits) {
    if (x.err || !n) return;
    size_t need = temp_bytes;
    x.chk(rocprim::radix_sort_pairs(temp, need, kin, kout, vin, vout, (size_t)n, 0, bits, x.st));
}

int va_run_device(const VaTables &t, int device, void *stream, VaOut &o) {
    const uint32_t V = t.V, S = t.S, P = t.P;
    SrStage x("variants", "the variant tables");
    if (x.open(device, stream, 8)) return x.err;
    o.variant = SR_VARIANTS_VARIANT_DEVICE;
    o.breaks.assign(P, 0); o.skipped.assign(P, 0);
    const uint32_t s0 = P ? t.path_off[t.R] : 0, s1 = P ? t.path_off[t.R + 1] : 0;
    if (!P || !S || s0 == s1) return SR_OK;                      // no path, no step or a reference without steps: nothing to find

    uint32_t *d_len = x.alloc<uint32_t>(V), *d_steps = x.alloc<uint32_t>(S), *d_poff = x.alloc<uint32_t>((uint64_t)P + 1);
    uint64_t *d_soff = x.alloc<uint64_t>((uint64_t)V + 1);
    uint8_t *d_seq = x.alloc<uint8_t>(t.seq.size()), *d_ref = x.alloc<uint8_t>(t.refseq.size());
    uint32_t *d_visits = x.alloc<uint32_t>(V, 0), *d_refpr = x.alloc<uint32_t>(V, 0);
    u64d *d_spos = x.alloc<u64d>(S), *d_prev = x.alloc<u64d>(S), *d_cnt = x.alloc<u64d>(S), *d_sums = x.alloc<u64d>(sr_scan_room(S));
    u64d *d_breaks = x.alloc<u64d>(P, 0), *d_skipped = x.alloc<u64d>(P, 0), *d_counts = x.alloc<u64d>(4, 0);
    uint8_t *d_cls = x.alloc<uint8_t>((uint64_t)S + 1, 0);
    if (x.err) return x.err;
    x.put(d_len, t.len.data(), (size_t)V * 4); x.put(d_steps, t.steps.data(), (size_t)S * 4); x.put(d_poff, t.path_off.data(), ((size_t)P + 1) * 4);
    x.put(d_soff, t.seq_off.data(), ((size_t)V + 1) * 8); x.put(d_seq, t.seq.data(), t.seq.size()); x.put(d_ref, t.refseq.data(), t.refseq.size());
    VaDev d;
    d.g = SrVarGraph{d_steps, d_len, d_soff, d_seq};
    d.path_off = d_poff; d.visits = d_visits; d.ref_pr = d_refpr; d.spos = d_spos; d.prev = d_prev;
    d.V = V; d.S = S; d.P = P; d.max_len = t.max_len; d.hash_mask = t.hash_mask;
    const dim3 blk(VA_BLOCK), gs(sr_stage_grid(S));

    x.mark(0);                                                   // ---- anchors
    if (!x.err) {
        sr_step_len(x, d_steps, d_len, S, d_spos);
        sr_scan<false>(x, d_spos, S, d_sums);
        hipLaunchKernelGGL(va_visits_kernel, dim3(sr_stage_grid(s1 - s0)), blk, 0, x.st, (const uint32_t *)d_steps, s0, s1, d_visits);
        hipLaunchKernelGGL(va_refpos_kernel, dim3(sr_stage_grid(s1 - s0)), blk, 0, x.st, d, s0, s1, d_refpr, d_counts + 0);
    }
    x.mark(1);                                                   // ---- the previous anchor step
    if (!x.err) {
        hipLaunchKernelGGL(va_mark_kernel, gs, blk, 0, x.st, (const uint32_t *)d_steps, (const uint32_t *)d_visits, S, d_prev);
        sr_scan<true>(x, d_prev, S, d_sums);
    }
    x.mark(2);                                                   // ---- emit
    if (!x.err) {
        hipLaunchKernelGGL(va_classify_kernel, gs, blk, 0, x.st, d, d_cls, d_cnt, d_breaks, d_skipped);
        sr_scan<false>(x, d_cnt, S, d_sums);
    }
    uint64_t totals = 0;
    x.get(&totals, d_cnt + (S - 1), 8);
    x.sync();                                                    // the traversals size the sort, the runs their table
    if (x.err) return x.err;
    const uint32_t T = (uint32_t)totals, NR = (uint32_t)(totals >> 32);
    VaRec rec;
    rec.i = x.alloc<uint32_t>(T); rec.j = x.alloc<uint32_t>(T); rec.a = x.alloc<uint32_t>(T); rec.b = x.alloc<uint32_t>(T);
    rec.len = x.alloc<uint32_t>(T); rec.path = x.alloc<uint32_t>(T); rec.strand = x.alloc<uint8_t>(T);
    VaRuns runs;
    runs.head = x.alloc<uint32_t>(NR); runs.tail = x.alloc<uint32_t>(NR); runs.path = x.alloc<uint32_t>(NR);
    u64d *d_hash = x.alloc<u64d>(T), *d_k64 = x.alloc<u64d>(T), *d_k64o = x.alloc<u64d>(T);
    uint32_t *d_iota = x.alloc<uint32_t>(T), *d_cref = x.alloc<uint32_t>(T, 0), *d_p0 = x.alloc<uint32_t>(T), *d_p1 = x.alloc<uint32_t>(T), *d_k32 = x.alloc<uint32_t>(T), *d_k32o = x.alloc<uint32_t>(T);
    uint8_t *d_flags = x.alloc<uint8_t>(T);
    u64d *d_site = x.alloc<u64d>(T), *d_class = x.alloc<u64d>(T), *d_sout = x.alloc<u64d>(T, 0);
    uint32_t *d_coll = x.alloc<uint32_t>(T, 0), *d_keep = x.alloc<uint32_t>(T, 0), *d_base = x.alloc<uint32_t>(T, 0);
    uint32_t *d_psite = x.alloc<uint32_t>(T), *d_palle = x.alloc<uint32_t>(T), *d_rsite = x.alloc<uint32_t>(T), *d_ralle = x.alloc<uint32_t>(T);
    uint32_t *d_oa = x.alloc<uint32_t>(T), *d_ob = x.alloc<uint32_t>(T);
    size_t tb64 = 0, tb32 = 0;
    if (T) {
        x.chk(rocprim::radix_sort_pairs(nullptr, tb64, (u64d *)nullptr, (u64d *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)T, 0, 64, x.st));
        x.chk(rocprim::radix_sort_pairs(nullptr, tb32, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)T, 0, 32, x.st));
    }
    const size_t temp_bytes = tb64 > tb32 ? tb64 : tb32;
    void *d_temp = x.alloc<uint8_t>(temp_bytes);
    if (x.err) return x.err;
    const dim3 gt_(sr_stage_grid(T));
    if (!x.err) hipLaunchKernelGGL(va_scatter_kernel, gs, blk, 0, x.st, d, (const uint8_t *)d_cls, (const u64d *)d_cnt, rec, runs);
    x.mark(3);                                                   // ---- hash
    if (!x.err && T) hipLaunchKernelGGL(va_hash_kernel, gt_, blk, 0, x.st, d, rec, T, d_hash, d_iota);
    x.mark(4);                                                   // ---- sort and classes
    uint64_t site_totals = 0;
    if (!x.err && T) {
        va_sort<u64d>(x, d_temp, temp_bytes, d_hash, d_k64o, d_iota, d_p1, T, 64);               // by hash; ties keep (path, step)
        hipLaunchKernelGGL(va_key_len_kernel, gt_, blk, 0, x.st, (const uint32_t *)d_p1, (const uint32_t *)rec.len, T, d_k32);
        va_sort<uint32_t>(x, d_temp, temp_bytes, d_k32, d_k32o, d_p1, d_p0, T, 32);             // by (length, hash)
        hipLaunchKernelGGL(va_key_ab_kernel, gt_, blk, 0, x.st, (const uint32_t *)d_p0, (const uint32_t *)rec.a, (const uint32_t *)rec.b, T, d_k64);
        va_sort<u64d>(x, d_temp, temp_bytes, d_k64, d_k64o, d_p0, d_p1, T, 64);                  // by (a, b, length, hash): d_p1
        hipLaunchKernelGGL(va_compare_kernel, gt_, blk, 0, x.st, d, rec, (const uint32_t *)d_p1, (const u64d *)d_hash, (const uint8_t *)d_ref, T, d_flags, d_site);
        sr_scan<false>(x, d_site, T, d_sums);
        hipLaunchKernelGGL(va_clash_kernel, gt_, blk, 0, x.st, (const uint8_t *)d_flags, (const u64d *)d_site, T, d_coll);
        hipLaunchKernelGGL(va_class_kernel, gt_, blk, 0, x.st, d, rec, (const uint32_t *)d_p1, (const uint8_t *)d_ref, d_flags, (const u64d *)d_site,
                           (const uint32_t *)d_coll, T, d_keep, d_class);
        sr_scan<false>(x, d_class, T, d_sums);
        hipLaunchKernelGGL(va_site_kernel, gt_, blk, 0, x.st, (const uint8_t *)d_flags, (const u64d *)d_site, (const u64d *)d_class, (const uint32_t *)d_keep,
                           (const uint32_t *)d_coll, T, d_base, d_cref, d_sout);
        sr_scan<false>(x, d_sout, T, d_sums);
        hipLaunchKernelGGL(va_number_kernel, gt_, blk, 0, x.st, rec, (const uint32_t *)d_p1, (const uint8_t *)d_flags, (const u64d *)d_site, (const u64d *)d_class,
                           (const uint32_t *)d_keep, (const uint32_t *)d_base, (const uint32_t *)d_cref, (const u64d *)d_sout, T, d_psite, d_palle, d_rsite, d_ralle, d_oa, d_ob);
        x.get(&site_totals, d_sout + (T - 1), 8);
        x.sync();                                                // the sites size the genotype table
    }
    if (x.err) return x.err;
    const uint32_t NS = (uint32_t)site_totals;
    o.collisions = site_totals >> 32;
    if ((uint64_t)NS * P > SR_VARIANTS_MAX_CELLS)
        return sr_fail(SR_ERR_UNSUPPORTED, "variants: " + std::to_string(NS) + " sites x " + std::to_string(P) + " paths; the table supports at most 2^26 cells");
    const uint64_t cells = (uint64_t)NS * P;
    int32_t *d_gt = x.alloc<int32_t>(cells, 0xff);
    if (x.err) return x.err;
    x.mark(5);                                                   // ---- genotypes
    if (!x.err && NS) {
        if (NR) hipLaunchKernelGGL(va_runs_kernel, dim3(sr_stage_grid(NR)), blk, 0, x.st, d, runs, NR, (const uint32_t *)d_oa, (const uint32_t *)d_ob, NS, d_gt);
        // the order of the records by site is a stable sort of the emission order: (site, path, step)
        va_sort<uint32_t>(x, d_temp, temp_bytes, d_rsite, d_k32o, d_iota, d_k32, T, 32);
        hipLaunchKernelGGL(va_gt_kernel, gt_, blk, 0, x.st, (const uint32_t *)d_k32o, (const uint32_t *)d_k32, (const uint32_t *)rec.path,
                           (const uint32_t *)d_ralle, T, P, d_gt);
    }
    std::vector<uint32_t> h_perm(T), h_psite(T), h_palle(T), h_i(T), h_j(T), h_oa(NS), h_ob(NS);
    std::vector<uint8_t> h_flags(T), h_strand(T);
    std::vector<uint64_t> h_count(4, 0);
    o.gt.assign(cells, -1);
    x.mark(6);
    x.chk(hipGetLastError());
    x.get(h_perm.data(), d_p1, (size_t)T * 4); x.get(h_psite.data(), d_psite, (size_t)T * 4); x.get(h_palle.data(), d_palle, (size_t)T * 4);
    x.get(h_i.data(), rec.i, (size_t)T * 4); x.get(h_j.data(), rec.j, (size_t)T * 4); x.get(h_flags.data(), d_flags, T); x.get(h_strand.data(), rec.strand, T);
    x.get(h_oa.data(), d_oa, (size_t)NS * 4); x.get(h_ob.data(), d_ob, (size_t)NS * 4);
    x.get(o.gt.data(), d_gt, (size_t)cells * 4); x.get(o.breaks.data(), d_breaks, (size_t)P * 8); x.get(o.skipped.data(), d_skipped, (size_t)P * 8);
    x.get(h_count.data(), d_counts, 32);
    x.mark(7);
    x.sync();                                                    // the synchronisation after the download
    if (x.err) return x.err;
    o.us = x.us(0, 7);
    for (int k = 0; k < 6; k++) o.kernel_us[k] = x.us(k, k + 1);
    o.anchors = h_count[0]; o.traversals = T;

    // host work over the output: the ALT classes of every kept site, numbered by (length, bytes); where that is not the
    // order of the classes on the device (by length and hash), or where bytes repeat (a site with a collision), the row of
    // the table is renumbered
    const SrVarGraph g = t.view();
    o.sites.resize(NS);
    for (uint32_t s = 0; s < NS; s++) { o.sites[s].a = h_oa[s]; o.sites[s].b = h_ob[s]; }
    std::vector<std::vector<std::pair<uint32_t, std::string>>> found(NS);
    // the length of a record is not downloaded: it is read off the graph between its two steps
    std::vector<uint64_t> spos((size_t)S + 1, 0);
    for (uint32_t s = 0; s < S; s++) spos[s + 1] = spos[s] + t.len[(t.steps[s] >> 1) - 1];
    for (uint32_t k = 0; k < T; k++) {
        if (h_psite[k] == SR_VARIANTS_NONE || !(h_flags[k] & VA_C_HEAD) || (h_flags[k] & VA_C_REF)) continue;
        const uint32_t r = h_perm[k];
        found[h_psite[k]].emplace_back(h_palle[k], va_allele(g, h_i[r], h_j[r], h_strand[r], spos[h_j[r]] - spos[h_i[r] + 1]));
    }
    for (uint32_t s = 0; s < NS; s++) {
        VaSite &site = o.sites[s];
        for (const auto &f : found[s]) site.alts.push_back(f.second);
        std::sort(site.alts.begin(), site.alts.end(), va_allele_less);
        site.alts.erase(std::unique(site.alts.begin(), site.alts.end()), site.alts.end());
        std::vector<int32_t> to(found[s].size() + 1, 0);
        bool same = true;
        for (const auto &f : found[s]) {
            to[f.first] = (int32_t)(std::lower_bound(site.alts.begin(), site.alts.end(), f.second, va_allele_less) - site.alts.begin()) + 1;
            same = same && to[f.first] == (int32_t)f.first;
        }
        if (same) continue;
        int32_t *row = o.gt.data() + (size_t)s * P;
        for (uint32_t p = 0; p < P; p++) if (row[p] > 0) row[p] = to[row[p]];
    }
    return SR_OK;
}

sr_variants *va_result(const VaTables &t, const VaOut &o) {
    sr_variants *r = (sr_variants *)calloc(1, sizeof(sr_variants));
    if (!r) return nullptr;
    const uint64_t P = t.P, NS = o.sites.size();
    uint64_t alts = 0, bytes = 0;
    for (const VaSite &s : o.sites) { alts += s.alts.size(); for (const auto &a : s.alts) bytes += a.size(); }
    r->ref_path = t.R; r->ref_len = t.refseq.size(); r->paths = P; r->anchors = o.anchors; r->traversals = o.traversals; r->sites = NS;
    r->hash_collision_sites = o.collisions; r->variant = o.variant; r->variants_us = o.us;
    for (int k = 0; k < 6; k++) r->kernel_us[k] = o.kernel_us[k];
    r->breaks = (uint64_t *)calloc(P ? P : 1, 8); r->skipped = (uint64_t *)calloc(P ? P : 1, 8);
    r->site_start = (uint64_t *)calloc(NS ? NS : 1, 8); r->site_end = (uint64_t *)calloc(NS ? NS : 1, 8);
    r->site_alleles = (uint32_t *)calloc(NS ? NS : 1, 4); r->allele_off = (uint64_t *)calloc(alts + 1, 8);
    r->alleles = (char *)calloc(bytes + 1, 1); r->gt = (int32_t *)calloc(NS * P ? NS * P : 1, 4); r->ref_seq = (char *)calloc(t.refseq.size() + 1, 1);
    if (!r->breaks || !r->skipped || !r->site_start || !r->site_end || !r->site_alleles || !r->allele_off || !r->alleles || !r->gt || !r->ref_seq) {
        sr_variants_free(r);
        return nullptr;
    }
    for (uint64_t p = 0; p < P; p++) { r->breaks[p] = o.breaks[p]; r->skipped[p] = o.skipped[p]; }
    uint64_t k = 0, at = 0;
    for (uint64_t s = 0; s < NS; s++) {
        r->site_start[s] = o.sites[s].a; r->site_end[s] = o.sites[s].b; r->site_alleles[s] = (uint32_t)o.sites[s].alts.size();
        for (const auto &a : o.sites[s].alts) { memcpy(r->alleles + at, a.data(), a.size()); at += a.size(); r->allele_off[++k] = at; }
    }
    if (NS * P) memcpy(r->gt, o.gt.data(), NS * P * 4);
    memcpy(r->ref_seq, t.refseq.data(), t.refseq.size());
    return r;
}

}   // namespace

int sr_graph_variants_run(const SrGraph &g, const std::vector<std::string> &names, const sr_variant_params &prm, int device, void *stream,
                          sr_variants **out) {
    if (!out) return sr_fail(SR_ERR_INVALID, "null argument");
    *out = nullptr;
    if (device < SR_VARIANTS_DEVICE_HOST) return sr_fail(SR_ERR_INVALID, "variants: device must be >= -1");
    try {
        VaTables t;
        int r = va_tables(g, names, prm, t);
        if (r) return r;
        VaOut o;
        if ((r = device < 0 ? va_run_host(t, o) : va_run_device(t, device, stream, o))) return r;
        sr_variants *res = va_result(t, o);
        if (!res) return sr_fail(SR_ERR_NOMEM, "not enough memory for the variant tables");
        *out = res;
    } catch (const std::bad_alloc &) {
        return sr_fail(SR_ERR_NOMEM, "not enough memory for the variant tables");
    }
    return SR_OK;
}

extern "C" void sr_variant_params_default(sr_variant_params *p) {
    if (!p) return;
    p->ref_name = nullptr; p->max_allele_len = 10000; p->hash_mask = ~0ULL; p->reserved = 0;
}

extern "C" int sr_variants_gfa(const char *gfa_in, const sr_variant_params *p, int device, sr_variants **out) {
    if (!gfa_in || !p || !out) return sr_fail(SR_ERR_INVALID, "null argument");
    SrGraph g;
    std::vector<std::string> names;
    int r = sr_graph_parse_gfa(gfa_in, g, names);
    if (r) return r;
    return sr_graph_variants_run(g, names, *p, device, nullptr, out);
}

extern "C" void sr_variants_free(sr_variants *v) {
    if (!v) return;
    free(v->breaks); free(v->skipped); free(v->site_start); free(v->site_end); free(v->site_alleles); free(v->allele_off);
    free(v->alleles); free(v->gt); free(v->ref_seq);
    free(v);
}

extern "C" int sr_variants_vcf(const sr_variants *v, const char *const *names, char **text) {
    if (!v || !text || (v->paths && !names)) return sr_fail(SR_ERR_INVALID, "null argument");
    const uint64_t P = v->paths, NS = v->sites, R = v->ref_path;
    if (NS * (P ? P : 1) > SR_VARIANTS_MAX_CELLS || (P && R >= P)) return sr_fail(SR_ERR_INVALID, "variants: not a result of sr_variants_gfa");
    try {
        uint64_t breaks = 0, skipped = 0;
        for (uint64_t p = 0; p < P; p++) { breaks += v->breaks[p]; skipped += v->skipped[p]; }
        const std::string chrom = P ? names[R] : "";
        std::string o = "##fileformat=VCFv4.2\n##source=seqrush_amd variants v1\n";
        if (P) o += "##contig=<ID=" + chrom + ",length=" + u64s(v->ref_len) + ">\n";
        o += "##seqrush_amd=<anchors=" + u64s(v->anchors) + ",traversals=" + u64s(v->traversals) + ",sites=" + u64s(NS) + ",breaks=" + u64s(breaks) +
             ",skipped=" + u64s(skipped) + ">\n";
        o += "##INFO=<ID=AC,Number=A,Type=Integer,Description=\"Samples that carry each ALT allele\">\n"
             "##INFO=<ID=AN,Number=1,Type=Integer,Description=\"Samples with a genotype\">\n"
             "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"
             "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT";
        for (uint64_t p = 0; p < P; p++) if (p != R) { o += "\t"; o += names[p]; }
        o += "\n";
        uint64_t k = 0;
        for (uint64_t s = 0; s < NS; s++) {
            const uint64_t a = v->site_start[s], b = v->site_end[s], n = v->site_alleles[s];
            bool pad = b == a;
            for (uint64_t x = 0; x < n; x++) pad = pad || v->allele_off[k + x + 1] == v->allele_off[k + x];
            if (pad && a == 0) return sr_fail(SR_ERR_INVALID, "variants: a site without a base before it");
            const uint64_t from = pad ? a - 1 : a;
            o += chrom + "\t" + u64s(from + 1) + "\t.\t" + std::string(v->ref_seq + from, b - from) + "\t";
            for (uint64_t x = 0; x < n; x++) {
                if (x) o += ",";
                if (pad) o += v->ref_seq[a - 1];
                o.append(v->alleles + v->allele_off[k + x], v->allele_off[k + x + 1] - v->allele_off[k + x]);
            }
            std::vector<uint64_t> ac(n, 0);
            uint64_t an = 0;
            const int32_t *row = v->gt + s * P;
            for (uint64_t p = 0; p < P; p++) {
                if (p == R || row[p] < 0) continue;
                an++;
                if (row[p] > 0 && (uint64_t)row[p] <= n) ac[row[p] - 1]++;
            }
            o += "\t.\t.\tAC=";
            for (uint64_t x = 0; x < n; x++) { if (x) o += ","; o += u64s(ac[x]); }
            o += ";AN=" + u64s(an) + "\tGT";
            for (uint64_t p = 0; p < P; p++) if (p != R) { o += "\t"; o += row[p] < 0 ? std::string(".") : u64s((uint64_t)row[p]); }
            o += "\n";
            k += n;
        }
        return sr_give_text(o, text, "not enough memory for the VCF text");
    } catch (const std::bad_alloc &) {
        return sr_fail(SR_ERR_NOMEM, "not enough memory for the VCF text");
    }
    return SR_OK;
}
