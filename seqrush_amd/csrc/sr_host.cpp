// sr_host.cpp -- the resident context behind the C ABI of include/seqrush_amd.h: its life, a load (index, packing, pair list,
// kernel plan, workspace), the passes that enqueue the alignment and unite kernels, the accessors, result collection and the
// iterative mode.  No CPU alignment path exists here: without a HIP device the compute entry points fail with SR_ERR_NO_DEVICE.
#include "sr_ctx.h"
#include "sr_mirror_rule.h"
#include "sr_prio_rule.h"
#include "sr_extend_rule.h"

int dev_alloc(sr_ctx *c, void **p, size_t bytes) {
    hipError_t e = hipMalloc(p, bytes ? bytes : 16);
    if (e != hipSuccess) {
        char buf[160];
        snprintf(buf, sizeof(buf), "hipMalloc of %zu bytes failed: %s", bytes, hipGetErrorString(e));
        return sr_fail(e == hipErrorOutOfMemory ? SR_ERR_NOMEM : SR_ERR_HIP, buf);
    }
    c->dev_allocs.push_back(*p);
    return SR_OK;
}
// The state of the load goes with its buffers, as one value: a load that fails half-way, or one that writes only a part of it
// (sr_ctx_load_paf has no kernel plan and no workspace report), must not show what the load before it left
void free_dev(sr_ctx *c) {
    for (void *p : c->dev_allocs) (void)hipFree(p);
    c->dev_allocs.clear();
    sr_alignments_free(c->iter_al);                // (sr_alignments_free accepts a null pointer: nothing kept, nothing freed)
    sr_alignments_free(c->inv_al);
    static_cast<SrLoadState &>(*c) = SrLoadState{};
}

// A load that failed after it had freed the load before it: nothing of either stays -- not the buffers it had allocated so far,
// not the pair list, sizes or report it had written so far (a failure before that point leaves the context as it was)
int unload_if_failed(sr_ctx *c, int r) {
    if (r && c && !c->loaded) {
        SrKeepError keep;
        (void)hipStreamSynchronize(c->stream);
        free_dev(c);
    }
    return r;
}

// event pair `idx` of kind `kind` (created on first use)
int ev_get(sr_ctx *c, int kind, int idx, hipEvent_t **a, hipEvent_t **b) {
    while ((int)c->ev[kind].size() <= idx) {
        hipEvent_t x = nullptr, y = nullptr;
        HIPCHK(hipEventCreate(&x)); HIPCHK(hipEventCreate(&y));
        c->ev[kind].push_back({x, y});
    }
    *a = &c->ev[kind][idx].first; *b = &c->ev[kind][idx].second;
    return SR_OK;
}

extern "C" int sr_ctx_create(int device, sr_ctx **out) {
    if (const int r = sr_pick_device(device)) return r;
    sr_ctx *c = new sr_ctx();
    c->device = device;
    if (hipStreamCreate(&c->stream) != hipSuccess) { delete c; return sr_fail(SR_ERR_HIP, "hipStreamCreate failed"); }
    c->own_stream = true;
    *out = c;
    return SR_OK;
}

extern "C" void sr_ctx_destroy(sr_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    free_dev(c);
    for (int k = 0; k < 5; k++)
        for (auto &e : c->ev[k]) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    for (auto &e : c->inv_ev) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    for (hipEvent_t e : c->ext_ev) if (e) (void)hipEventDestroy(e);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

// The context's own stream is drained and destroyed; a caller's stream it gives up is not waited for (the caller owns it and
// may have work of its own there): the rule is sr_ctx_sync() before sr_ctx_set_stream() on a context with work in flight
// (include/seqrush_amd.h; tests/test_resident_gpu.py changes streams on a loaded context that way)
extern "C" int sr_ctx_set_stream(sr_ctx *c, void *hip_stream) {
    if (!c) return sr_fail(SR_ERR_INVALID, "null ctx");
    if (c->own_stream && c->stream) { (void)hipStreamSynchronize(c->stream); (void)hipStreamDestroy(c->stream); }
    c->stream = (hipStream_t)hip_stream;
    c->own_stream = false;
    return SR_OK;
}

// ------------------------------------------------------------------ load
// Symbol codes of the packed buffer.  The reference compares raw bytes (seqrush.rs:1162-1176, 1268-1283), so any
// injective byte -> code map keeps every comparison: 2 bits when the inputs (and their complements) are within
// upper-case ACGT, 4 bits for <= 16 distinct bytes (N, IUPAC, soft-masked lower case), else the bytes themselves.
struct SymMap { int bits; int code[256]; };
static SymMap make_symmap(const sr_seqset *seqs) {
    bool present[256] = {false};
    const uint64_t N = seqs->offsets[seqs->n];
    for (uint64_t i = 0; i < N; i++) present[seqs->bases[i]] = true;
    for (int b = 0; b < 256; b++) if (present[b]) present[comp_base((uint8_t)b)] = true;
    SymMap m;
    for (int b = 0; b < 256; b++) m.code[b] = -1;
    bool acgt = true;
    int distinct = 0;
    for (int b = 0; b < 256; b++) if (present[b]) { distinct++; if (b != 'A' && b != 'C' && b != 'G' && b != 'T') acgt = false; }
    if (acgt) { m.bits = 2; m.code['A'] = 0; m.code['C'] = 1; m.code['G'] = 2; m.code['T'] = 3; return m; }
    if (distinct <= 16) { m.bits = 4; int k = 0; for (int b = 0; b < 256; b++) if (present[b]) m.code[b] = k++; return m; }
    m.bits = 8;
    for (int b = 0; b < 256; b++) m.code[b] = b;
    return m;
}

// A load runs these steps in order (round 3: one function each):
//   load_index        lengths, offsets, penalties, parameter checks
//   pack_sequences    byte -> symbol map, packed copies (forward / reverse complement [/ reversed / complemented])
//   upload_sequences  raw bytes + packed words + per-sequence tables to the device
//   build_pair_list   enumeration or explicit list, sparsification (tree: k-mer sketches on the device), shard
//   plan_launch       which kernel, workgroup shape, per-workgroup workspace, CIGAR arena and batches, workgroup count
//   alloc_workspace   device allocations, per-pair arrays, kernel arguments, sizing report
struct PackedSeqs {
    SymMap sm;
    int per_word = 16, ncopies = 2;
    std::vector<uint64_t> woff[4];                 // word offset of every sequence's copy k (k = 2, 3 alias 1, 0 for 2-bit buffers)
    std::vector<uint32_t> words;
};
struct SeqDev { uint32_t *words = nullptr; uint64_t *woff[4] = {nullptr, nullptr, nullptr, nullptr}; uint64_t *goff = nullptr; uint32_t *len = nullptr; };
struct Plan {
    // kernel + launch shape
    int impl = 1, kblock = 0, wg_per_cu = 4, cus = 256, lazy_id = 0, ring_u16 = 0, bbase_jobs = 16;
    int tail_threads = 0;                 // shape of the tail launch, 0 = none
    bool wave_wg = false;
    uint32_t max_words = 0;
    size_t osz = 2, rsz = 2;
    // per-workgroup workspace (cells unless stated)
    int ring_scope = 0, ring_hot = 0, hist_levels = 0, hist_w = 0, brow = 0, kdepth = 0, kdepth2 = 0;
    uint64_t bring_wg = 0, bhist_wg = 0, hist_cap = 0, hist_nul_w = 0, bseg_wg = 0, bbt_wg = 0, bcl_wg = 0, per_wg_bytes = 0;
    uint64_t brec_wg = 0, brec_bytes = 0;          // replay: bytes of a workgroup's breakpoint records; of all (0: the load keeps none)
    // memory budget
    size_t free_b = 0;
    uint64_t arena_ops = 0, left = 0, max_reserve = 4;
    uint32_t nbatch = 0, max_batch_pairs = 0;
    int nwg = 1;
    uint64_t oring_bytes = 0;
};

static int load_index(sr_ctx *c, const sr_seqset *seqs, const sr_params *p, bool explicit_pairs, SrPen *pen, SrPen *ori, uint64_t *maxlen_out) {
    c->prm = *p;
    const uint32_t n = seqs->n;
    c->n = n;
    c->len.assign(n, 0); c->goff.assign(n, 0);
    uint64_t maxlen = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t L = seqs->offsets[i + 1] - seqs->offsets[i];
        if (L == 0) {
            std::string nm = (seqs->names && seqs->names[i]) ? seqs->names[i] : std::to_string(i);
            return sr_fail(SR_ERR_EMPTY_SEQ, "Empty sequences are not allowed: sequence '" + nm + "' has length 0");
        }
        if (L > 0x7fff0000ULL) return sr_fail(SR_ERR_UNSUPPORTED, "sequence too long");
        c->len[i] = (uint32_t)L; c->goff[i] = seqs->offsets[i];
        maxlen = std::max(maxlen, L);
    }
    *maxlen_out = maxlen;
    c->total_len = seqs->offsets[n];
    c->uf_size = (c->total_len << 1) + 2;          // bidirected_union_find.rs:16-24
    int r;
    if ((r = make_pen(*p, false, pen))) return r;
    if ((r = make_pen(*p, true, ori))) return r;
    if (p->memory_mode != SR_MEM_ULTRALOW)
        return sr_fail(SR_ERR_UNSUPPORTED, "memory_mode must be SR_MEM_ULTRALOW (biWFA, what the reference selects: src/wfa.rs:57); "
                                        "the device keeps full wavefront history only for biWFA's base cases");
    if (p->sparsify_kind < SR_SPARSE_NONE || p->sparsify_kind > SR_SPARSE_TREE) return sr_fail(SR_ERR_INVALID, "bad sparsify_kind");
    if (p->sparsify_kind == SR_SPARSE_TREE && (p->tree_kmer < 1 || p->tree_kmer > 32))
        return sr_fail(SR_ERR_UNSUPPORTED, "tree sparsification: k-mer size must be in 1..32 on the device");
    if (p->shard_count == 0 || p->shard_rank >= p->shard_count) return sr_fail(SR_ERR_INVALID, "bad shard");
    if (!explicit_pairs && (uint64_t)n * n > 0xffffffffULL)
        return sr_fail(SR_ERR_UNSUPPORTED, "more than 2^32 ordered pairs: sparsify (-x) or pass an explicit pair list");
    return SR_OK;
}

// packed symbol buffer: forward, reverse complement (+ reversed, complemented when the alphabet is not plain ACGT: seqrush's
// complement maps lower case to upper case, so "equal complements <=> equal bases" fails); one pad word either side of a copy
static void pack_sequences(const sr_ctx *c, const sr_seqset *seqs, PackedSeqs &pk) {
    const uint32_t n = seqs->n;
    pk.sm = make_symmap(seqs);
    pk.per_word = 32 / pk.sm.bits;
    pk.ncopies = pk.sm.bits == 2 ? 2 : 4;
    for (int k = 0; k < 4; k++) pk.woff[k].assign(n, 0);
    uint64_t words = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t w = (c->len[i] + pk.per_word - 1) / pk.per_word;
        for (int k = 0; k < pk.ncopies; k++) { pk.woff[k][i] = words + 1; words += w + 2; }
        if (pk.ncopies == 2) { pk.woff[2][i] = pk.woff[1][i]; pk.woff[3][i] = pk.woff[0][i]; }      // aliases (see sr_align_blk.inc)
    }
    pk.words.assign(words, 0);
    const SymMap &sm = pk.sm;
    for (uint32_t i = 0; i < n; i++) {
        const uint8_t *b = seqs->bases + seqs->offsets[i];
        const uint64_t L = c->len[i];
        for (uint64_t j = 0; j < L; j++) {
            const unsigned sh = (unsigned)(j % pk.per_word) * sm.bits;
            const uint64_t wi = j / pk.per_word;
            pk.words[pk.woff[0][i] + wi] |= (uint32_t)sm.code[b[j]] << sh;                          // forward
            pk.words[pk.woff[1][i] + wi] |= (uint32_t)sm.code[comp_base(b[L - 1 - j])] << sh;      // reverse complement
            if (pk.ncopies == 4) {
                pk.words[pk.woff[2][i] + wi] |= (uint32_t)sm.code[b[L - 1 - j]] << sh;              // reversed
                pk.words[pk.woff[3][i] + wi] |= (uint32_t)sm.code[comp_base(b[j])] << sh;           // complemented
            }
        }
    }
}

static int upload_sequences(sr_ctx *c, const sr_seqset *seqs, const PackedSeqs &pk, SeqDev &sd) {
    int r;
    void *d;
    if ((r = dev_alloc(c, &d, c->total_len))) return r;                // raw bytes (sketches, graph induction)
    c->d_bases = (uint8_t *)d;
    HIPCHK(hipMemcpyAsync(c->d_bases, seqs->bases, c->total_len, hipMemcpyHostToDevice, c->stream));
    if ((r = dev_upload(c, pk.words, &sd.words))) return r;
    if ((r = dev_upload(c, pk.woff[0], &sd.woff[0]))) return r;
    if ((r = dev_upload(c, pk.woff[1], &sd.woff[1]))) return r;
    if (pk.ncopies == 4) { if ((r = dev_upload(c, pk.woff[2], &sd.woff[2])) || (r = dev_upload(c, pk.woff[3], &sd.woff[3]))) return r; }
    else { sd.woff[2] = sd.woff[1]; sd.woff[3] = sd.woff[0]; }
    if ((r = dev_upload(c, c->len, &sd.len))) return r;
    if ((r = dev_upload(c, c->goff, &sd.goff))) return r;
    HIPCHK(hipStreamSynchronize(c->stream));                           // (the host vectors may go away after this)
    return SR_OK;
}

// `tree:` sparsification: bottom-1000 sketches, pairwise similarities and the k-nearest / k-farthest selection on the device.
// ONE routine for the load path and the tests: entries (sr_sketch_device, sr_knn_select_device): padded lengths, stride,
// allocations, fills and launches are here and nowhere else.
//   h_shared / h_denom given: the matrices come from the host and the sketch / Jaccard stages do not run (len, d_* unused);
//   sel == nullptr: the selection does not run;  tap: copies of the intermediates for the tests
#define SR_SKETCH_SIZE 1000
int tree_stages(hipStream_t stream, uint32_t n, const uint32_t *len, const uint8_t *d_bases, const uint64_t *d_goff,
                const uint32_t *d_len, uint32_t kmer, const uint32_t *h_shared, const uint32_t *h_denom,
                uint32_t k_nearest, uint32_t k_farthest, std::vector<uint8_t> *sel, const TreeTap *tap) {
    const int S = SR_SKETCH_SIZE;
    const size_t nn = (size_t)n * n;
    SrScratch tmp;
    uint32_t *d_sh = (uint32_t *)tmp.alloc(nn * 4), *d_dn = (uint32_t *)tmp.alloc(nn * 4);
    if (!d_sh || !d_dn) return sr_fail(SR_ERR_NOMEM, "not enough device memory for the k-mer sketches");
    unsigned long long *d_sk = nullptr;
    uint32_t *d_skn = nullptr;
    std::vector<uint32_t> npad;                    // (read by an asynchronous copy: lives until the synchronize below)
    if (h_shared) {
        HIPCHK(hipMemcpyAsync(d_sh, h_shared, nn * 4, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(d_dn, h_denom, nn * 4, hipMemcpyHostToDevice, stream));
    } else {
        npad.resize(n);
        uint64_t stride = 2;
        for (uint32_t i = 0; i < n; i++) { uint32_t v = 2; while (v < len[i]) v <<= 1; npad[i] = v; stride = std::max<uint64_t>(stride, v); }
        unsigned long long *d_scr = (unsigned long long *)tmp.alloc((size_t)n * stride * 8);
        d_sk = (unsigned long long *)tmp.alloc((size_t)n * S * 8);
        d_skn = (uint32_t *)tmp.alloc((size_t)n * 4);
        uint32_t *d_npad = (uint32_t *)tmp.alloc((size_t)n * 4);
        if (!d_scr || !d_sk || !d_skn || !d_npad) return sr_fail(SR_ERR_NOMEM, "not enough device memory for the k-mer sketches");
        HIPCHK(hipMemcpyAsync(d_npad, npad.data(), (size_t)n * 4, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemsetAsync(d_sk, 0xFF, (size_t)n * S * 8, stream));     // (a write past a row's count shows in sr_sketch_device)
        HIPCHK(hipMemsetAsync(d_sh, 0, nn * 4, stream));
        HIPCHK(hipMemsetAsync(d_dn, 0, nn * 4, stream));
        if (srk_sketch(d_bases, d_goff, d_len, n, (int)kmer, S, d_scr, stride, d_npad, d_sk, d_skn, stream) ||
            srk_jaccard(d_sk, d_skn, n, S, d_sh, d_dn, stream))
            return sr_fail(SR_ERR_HIP, "sketch kernel launch failed");
    }
    uint8_t *d_sel = nullptr;
    if (sel) {
        if (!(d_sel = (uint8_t *)tmp.alloc(nn))) return sr_fail(SR_ERR_NOMEM, "not enough device memory for the k-mer sketches");
        HIPCHK(hipMemsetAsync(d_sel, 0, nn, stream));
        if (srk_knn_select(d_sh, d_dn, n, (int)std::min<uint32_t>(k_nearest, n), (int)std::min<uint32_t>(k_farthest, n), d_sel, stream))
            return sr_fail(SR_ERR_HIP, "sketch kernel launch failed");
        sel->resize(nn);
    }
    HIPCHK(hipStreamSynchronize(stream));
    if (sel) HIPCHK(hipMemcpy(sel->data(), d_sel, nn, hipMemcpyDeviceToHost));
    if (tap) {
        if (tap->sketch && d_sk) { tap->sketch->resize((size_t)n * S); HIPCHK(hipMemcpy(tap->sketch->data(), d_sk, (size_t)n * S * 8, hipMemcpyDeviceToHost)); }
        if (tap->sketch_n && d_skn) { tap->sketch_n->resize(n); HIPCHK(hipMemcpy(tap->sketch_n->data(), d_skn, (size_t)n * 4, hipMemcpyDeviceToHost)); }
        if (tap->shared) { tap->shared->resize(nn); HIPCHK(hipMemcpy(tap->shared->data(), d_sh, nn * 4, hipMemcpyDeviceToHost)); }
        if (tap->denom) { tap->denom->resize(nn); HIPCHK(hipMemcpy(tap->denom->data(), d_dn, nn * 4, hipMemcpyDeviceToHost)); }
    }
    return SR_OK;
}
static int tree_selection(sr_ctx *c, const sr_params *p, const SeqDev &sd, std::vector<uint8_t> &sel) {
    return tree_stages(c->stream, c->n, c->len.data(), c->d_bases, sd.goff, sd.len, p->tree_kmer, nullptr, nullptr,
                       p->tree_k_nearest, p->tree_k_farthest, &sel, nullptr);
}

// ordered pair list of this rank + what follows from it: DP cells, worst-case CIGAR reserve per pair, divergence thresholds
static int build_pair_list(sr_ctx *c, const sr_params *p, const SeqDev &sd, const uint32_t *eq, const uint32_t *et, uint64_t ecount,
                           bool explicit_pairs, std::vector<int32_t> &max_score, uint64_t *max_reserve, bool iterative = false,
                           uint32_t ext_n_old = 0) {
    const uint32_t n = c->n;
    if (iterative) {                  // --iterative: expanded tree entries, then expanded random entries (explicit list, no shard)
        std::vector<uint8_t> sel;
        if (n > 1) { const int r = tree_selection(c, p, sd, sel); if (r) return r; }
        std::vector<uint32_t> ti, tj, ri, rj;
        iterative_lists(n, sel.empty() ? nullptr : sel.data(), p->sparsify_seed, p->tree_rand_frac, ti, tj, ri, rj);
        if (4 * ((uint64_t)ti.size() + ri.size()) > 0xfffffff0ULL) return sr_fail(SR_ERR_UNSUPPORTED, "more than 2^32 pairs in one shard");
        c->pair_q.clear(); c->pair_t.clear();
        auto expand = [&](uint32_t i, uint32_t j) {
            const uint32_t q[4] = {i, i, j, j}, t[4] = {i, j, i, j};
            for (int k = 0; k < 4; k++) { c->pair_q.push_back(q[k]); c->pair_t.push_back(t[k]); }
        };
        for (size_t e = 0; e < ti.size(); e++) expand(ti[e], tj[e]);
        for (size_t e = 0; e < ri.size(); e++) expand(ri[e], rj[e]);
        c->iter_tree_pairs = 4 * (uint64_t)ti.size();
        c->iter_stats.tree_entries = ti.size(); c->iter_stats.random_entries = ri.size();
    } else if (explicit_pairs) {
        c->pair_q.assign(eq, eq + ecount); c->pair_t.assign(et, et + ecount);
        for (uint64_t i = 0; i < ecount; i++)
            if (eq[i] >= n || et[i] >= n) return sr_fail(SR_ERR_INVALID, "pair index out of range");
    } else {
        std::vector<uint8_t> sel;
        if (p->sparsify_kind == SR_SPARSE_TREE && n > 1) { const int r = tree_selection(c, p, sd, sel); if (r) return r; }
        enumerate_pairs(n, *p, sel.empty() ? nullptr : sel.data(), c->pair_q, c->pair_t);
        if (ext_n_old) {              // --extend: the pairs between two old sequences were aligned when the input graph was built
            c->ext_stats.pairs_before = c->pair_q.size();
            size_t w = 0;
            for (size_t i = 0; i < c->pair_q.size(); i++)
                if (sr_ext_keep_pair(c->pair_q[i], c->pair_t[i], ext_n_old)) { c->pair_q[w] = c->pair_q[i]; c->pair_t[w] = c->pair_t[i]; w++; }
            c->pair_q.resize(w); c->pair_t.resize(w);
            c->ext_stats.pairs_after = w;
        }
    }
    c->total_pairs_all_ranks = c->pair_q.size();
    shard_pairs(c->len, p->shard_rank, p->shard_count, c->pair_q, c->pair_t);
    if (c->pair_q.size() > 0xfffffff0ULL) return sr_fail(SR_ERR_UNSUPPORTED, "more than 2^32 pairs in one shard");
    const uint32_t np = (uint32_t)c->pair_q.size();
    c->dp_cells = 0;
    c->cigar_base.assign((size_t)np + 1, 0);
    max_score.assign(std::max<uint32_t>(np, 1), INT_MAX);
    *max_reserve = 4;
    for (uint32_t i = 0; i < np; i++) {
        const uint64_t lq = c->len[c->pair_q[i]], lt = c->len[c->pair_t[i]];
        c->dp_cells += lq * lt;
        c->cigar_base[i + 1] = c->cigar_base[i] + lq + lt + 2;
        *max_reserve = std::max(*max_reserve, lq + lt + 2);
        if (p->max_divergence >= 0.0) max_score[i] = max_score_for_divergence(*p, std::min(lq, lt), p->max_divergence);
    }
    return SR_OK;
}

// static tables of the alignment kernels (upper estimates; the blocked kernel's scan arrays of the fused unite grow with the
// workgroup: 25 296 / 28 416 / 34 656 bytes at 256 / 512 / 1024 threads with the second key table of breakpoint detection and
// the replay's per-segment state)
static size_t align_static_lds(bool wave_wg, int impl, int nthreads) {
    return (size_t)(wave_wg ? 6 : impl != 2 ? 28 : nthreads >= 1024 ? 34 : nthreads >= 512 ? 28 : 25) * 1024;
}
// Shape of the tail launch: threads per workgroup of the widest blocked instance srk_align dispatches for the plan that is
// wider than the main launch and whose LDS fits by plan_kernel's tests (static tables + four sequence copies inside the
// 128 KB window); 0 = no tail launch.  Instances (sr_align_blk.hip): 10-level blocks on int16 rows -- 1 024 threads for the
// two-piece 2-bit build, 512 for all; 32-bit searches on the uint16 ring -- 512; everything has 256.  The one-wave builds,
// the 5-level instances and 32-bit rows have nothing wider.  forced (SR_TAIL_THREADS) > 0: the widest instance <= forced,
// whatever the main launch has.  Pure, and exported for the tests.
extern "C" int sr_tail_shape(int impl, int kblock, int wave_wg, int off16, int ring_u16, int symbits, int two, int main_threads,
                             uint32_t max_words, int forced) {
    if (impl != 2 || kblock != 10 || wave_wg) return 0;
    if (!off16 && !ring_u16 && forced < 256) return 0;                     // 32-bit rows: the 256-thread build only
    static const int shapes[3] = {1024, 512, 256};
    for (int nt : shapes) {
        if (forced > 0 ? nt > forced : nt <= main_threads) continue;
        if (nt == 1024 && !(off16 && symbits == 2 && two)) continue;
        if (nt == 512 && !(off16 || ring_u16)) continue;
        if ((size_t)max_words * 16 + 16 + align_static_lds(false, 2, nt) > 128 * 1024) continue;
        return nt;
    }
    return 0;
}

// kernel choice and workgroup shape.  impl 2 = score-blocked wave-tiled kernel (when this build has an instance for the
// penalties), impl 1 = level-synchronous kernel (any penalties; rings deeper than 32 levels take its wide instance)
static int plan_kernel(sr_ctx *c, const PackedSeqs &pk, const SrPen &pen, const SrPen &ori, uint64_t maxlen, uint32_t np, Plan &pl) {
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, c->device));
    pl.cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    const int cus = pl.cus, bits = pk.sm.bits;
    c->off16 = maxlen <= 32000 ? 1 : 0;
    if (knob("SR_FORCE_INT32")) c->off16 = 0;             // (tests: the 32-bit searches and their 16-bit ring on short sequences)
    pl.osz = c->off16 ? 2 : 4;
    pl.max_words = (uint32_t)((maxlen + pk.per_word - 1) / pk.per_word + 2);
    c->lds_bytes = (size_t)pl.max_words * 3 * 4;          // query fwd / rc + target fwd
    if ((long long)c->lds_bytes > (long long)srk_align_max_lds())
        return sr_fail(SR_ERR_UNSUPPORTED, "sequences too long to stage in LDS (limit 177456 / 88728 / 44364 symbols per sequence at 2 / 4 / 8 bits per symbol)");
    pl.impl = 1;
    pl.kblock = srk_align_blk_supports(&pen, &ori);
    // SR_BLK_LEVELS=5: the generic 5-level instance instead of the exact-penalty 10-level one (A/B runs, tests)
    if (const char *e = knob("SR_BLK_LEVELS")) { if (atoi(e) == 5 && pl.kblock == 10) pl.kblock = 5; }
    // (the blocked kernel stages four sequence copies, has ~20 KB of static LDS and keeps its LDS window addresses within
    // 128 KB: static tables + copies must fit below; it has its own ring depth limit, srk_align_blk_supports)
    if (pl.kblock > 0 && (long long)pl.max_words * 16 + 28 * 1024 <= 128 * 1024) pl.impl = 2;
    if (const char *e = knob("SR_ALIGN_IMPL")) { if (atoi(e) <= 1) pl.impl = 1; }      // (tests: the level-per-pass kernel)
    int &impl = pl.impl, &kblock = pl.kblock;
    if (impl == 2) c->lds_bytes = (size_t)pl.max_words * 4 * 4 + 16;      // (+ read slack of a two-window extension step)
    pl.wg_per_cu = 4;
    if (const char *e = knob("SR_WG_PER_CU")) pl.wg_per_cu = std::max(1, atoi(e));
    c->nthreads = 256;
    // few pairs (e.g. the 1/8 shard of C2): one pair per workgroup leaves CUs short of waves, so give every
    // pair 8 waves instead of 4 (measured 31 -> 23 ms for 529 pairs of 5 kb)
    if (impl == 2 && (uint64_t)np <= 2ULL * (uint64_t)cus + (uint64_t)cus / 2) c->nthreads = 512;
    // fewer pairs than CUs (C3: 144): a pair has a CU to itself -- 16 waves (C3 90.1 -> 69.2 ms)
    if (impl == 2 && (uint64_t)np <= (uint64_t)cus) c->nthreads = 1024;
    if (const char *e = knob("SR_ALIGN_THREADS")) {
        const int v = atoi(e);
        if (v == 128 || v == 256 || v == 512 || (v == 1024 && impl == 2) || (v == 64 && impl == 2 && bits == 2)) c->nthreads = v;
    }
    if (c->nthreads == 1024 && !(impl == 2 && kblock == 10 && c->off16 && bits == 2 && pen.two)) c->nthreads = 512;   // (the one 1024-thread build)
    if (impl == 2 && c->nthreads == 128 && kblock == 10 && !(bits == 2 && c->off16)) kblock = 5;   // (no 128-thread 10-level instance there)
    pl.wave_wg = impl == 2 && (c->nthreads == 64 || (c->nthreads == 128 && kblock == 10));   // lean builds: 16 / 8 pairs per CU
    if (pl.wave_wg) pl.wg_per_cu = c->nthreads == 64 ? 16 : 8;
    auto static_lds = [&](int nthreads) -> size_t { return align_static_lds(pl.wave_wg, impl, nthreads); };
    const size_t lds_per_wg = c->lds_bytes + static_lds(c->nthreads);
    pl.wg_per_cu = (int)std::min<size_t>((size_t)pl.wg_per_cu, std::max<size_t>(1, (160 * 1024) / lds_per_wg));
    // long sequences: the four LDS copies leave room for two workgroups per CU (C5: 50 KB each) -- give each 8 waves, or
    // the SIMDs hold two waves (C5 subset 3 507 -> 2 200 ms).  512-thread builds: int16 rows; 32-bit searches with the
    // uint16 ring (exact instance below 57 k, see ring_u16)
    const char *ru = knob("SR_RING_U16");
    const bool u16_ok = kblock == 10 && maxlen <= 57000 && !(ru && atoi(ru) == 0);
    if (impl == 2 && !pl.wave_wg && pl.wg_per_cu <= 2 && !knob("SR_ALIGN_THREADS") && (c->off16 || u16_ok)) c->nthreads = 512;
    pl.wg_per_cu = (int)std::min<size_t>((size_t)pl.wg_per_cu, std::max<size_t>(1, (160 * 1024) / (c->lds_bytes + static_lds(c->nthreads))));
    // 32-bit searches below 57 k keep their ring as 16-bit cells (offset - 24576): half the row bytes (C5 is bound by them).
    // The exact 10-level instance at >= 256 threads has that build; SR_RING_U16=0 keeps 32-bit rows.
    pl.ring_u16 = (impl == 2 && !c->off16 && u16_ok && c->nthreads >= 256) ? 1 : 0;
    // 32-bit searches on 32-bit rows have one workgroup build, 256 threads (srk_align_blk launches it whatever it is asked
    // for): say so here, so that the launch and the workspace report carry the shape that runs
    if (impl == 2 && !pl.wave_wg && !c->off16 && !pl.ring_u16) c->nthreads = 256;
    pl.rsz = pl.ring_u16 ? 2 : pl.osz;                 // bytes per ring cell (the base-case history keeps osz)
    pl.bbase_jobs = pl.wave_wg ? (c->nthreads == 64 ? 4 : 8) : 16;
    if (const char *e = knob("SR_BFS_BASE_JOBS")) pl.bbase_jobs = std::max(1, std::min(16, atoi(e)));
    // the tail launch; whether a load has partners at all is alloc_workspace's business
    const char *tl = knob("SR_TAIL"), *tt = knob("SR_TAIL_THREADS");
    pl.tail_threads = (tl && !strcmp(tl, "0")) ? 0
                      : sr_tail_shape(impl, kblock, pl.wave_wg, c->off16, pl.ring_u16, bits, pen.two, c->nthreads, pl.max_words, tt ? std::max(1, atoi(tt)) : 0);
    return SR_OK;
}

// per-workgroup workspace: shared rows (every aligner of a pass owns a sub-range), base-case history, segment lists,
// reversed op buffers of the base cases, breakpoint candidate list, per-level maxima
static int plan_workspace(const sr_ctx *c, const SrPen &pen, const SrPen &ori, uint64_t maxlen, Plan &pl) {
    const int impl = pl.impl, kblock = pl.kblock;
    pl.ring_scope = std::max(pen.scope, ori.scope);
    int emax = std::max(pen.e1, ori.e1);
    if (pen.two) emax = std::max(emax, pen.e2);
    pl.ring_hot = emax + 2;
    const int gapmax = pen.two ? std::max(pen.o1, pen.o2) : pen.o1;
    auto gc = [&](int len) { int g = pen.o1 + pen.e1 * len; if (pen.two) g = std::min(g, pen.o2 + pen.e2 * len); return g; };
    // worst base case: score <= 250 (+ one gap-open: a half that ends in a gap component) or both lengths <= 100
    const int smax_base = std::max(250 + gapmax, 2 * gc(100)) + 2 * gapmax + 4;
    pl.hist_levels = smax_base + 1 + std::max(kblock, 5);   // + one block of levels (impl 2 computes whole blocks)
    int rmax = smax_base / pen.e1;
    if (pen.two) rmax = std::max(rmax, smax_base / pen.e2);
    pl.hist_w = (2 * (rmax + pen.scope + 2) + 1 + 8 + 64 + 7) & ~7;   // rows hold whole 4-diagonal groups, + halo groups either side
    pl.brow = (int)((4 * maxlen + 32 * 72 + 64 + 512 + 7) & ~7ULL);     // per-aligner margins + read slack of the last wave tile
    pl.kdepth = std::max(pen.scope + std::max(kblock, 1), ori.scope + 1) + 1;
    // lazy I/D rows (sr_align_blk.inc blk_recompute): the M rows must reach 2 * scope + 2 blocks back
    const char *lz = knob("SR_LAZY_ID");
    pl.lazy_id = (impl == 2 && !(lz && atoi(lz) == 0) && 2 * pen.scope + 2 * kblock + 2 <= SR_BLK_MAK_SLOTS) ? 1 : 0;
    pl.kdepth2 = pl.kdepth;
    if (pl.lazy_id) {
        // I / D rows are read by breakpoint detection (scope levels back from the newest block) and written by the recompute
        // pass from the block boundary before that window: scope + 2 blocks + 2 levels are live at most
        pl.kdepth2 = std::max(pl.kdepth, pen.scope + 2 * kblock + 2);
        pl.kdepth = std::max(pl.kdepth, 2 * pen.scope + 2 * kblock + 2);
    }
    if (impl == 2 && kblock == 10) {
        // exact instance: ring depths are multiples of the block, so that a block's ten levels (and five levels from a multiple
        // of five) are adjacent rows that never straddle the ring's wrap -- the tile addresses them as base + immediate
        // (sr_align_blk.inc kbase; default penalties: 74 -> 80 M levels, 48 -> 50 I / D levels)
        pl.kdepth = (pl.kdepth + 9) / 10 * 10; pl.kdepth2 = (pl.kdepth2 + 9) / 10 * 10;
    }
    // level-per-pass kernel: M ring | 4 hot I/D rings | cold I/D history | NULL row | U row, rows of brow cells
    pl.bring_wg = ((uint64_t)(pl.ring_scope + 1) + 4ULL * pl.ring_hot + 4ULL * (pl.ring_scope + 1) + 2ULL) * (uint64_t)pl.brow;
    // blocked kernel: chunk-major ring (sr_align_blk.inc KRows): 256-cell pieces of all depth + 4 * depth2 + 3 rows together
    // (NULL, U, trash), + 2 pieces of read slack; a workgroup's rows are addressed as base + 32-bit byte offset
    if (impl == 2) pl.bring_wg = ((uint64_t)pl.brow / 256 + 2ULL) * ((uint64_t)pl.kdepth + 4ULL * pl.kdepth2 + (uint64_t)SR_NULL_ROWS + 2ULL) * 256ULL + 1024;
    if (impl == 2 && pl.bring_wg * pl.rsz >= (1ULL << 32)) return sr_fail(SR_ERR_UNSUPPORTED, "sequences too long for the device row workspace (4 GB per workgroup)");
    // base-case history.  Level-per-pass kernel: bbase_jobs fixed slots of the worst-case width.  Blocked kernel: hist_cap
    // cells in which every job of a batch gets a region for the levels and width it really needs (sr_align_blk.inc); one
    // worst-case job always fits, the default holds 4 of them (C2: 11 MB instead of 40.6 -- a pair's 16 base cases of score
    // ~150 need 6.5 M cells and still run as one batch; SR_HIST_JOBS=n: n of them)
    const uint64_t hist_worst = (uint64_t)pl.hist_levels * 5 * (uint64_t)pl.hist_w;
    pl.hist_cap = hist_worst * 4;
    if (const char *e = knob("SR_HIST_JOBS")) pl.hist_cap = hist_worst * (uint64_t)std::max(1, std::min(16, atoi(e)));
    pl.hist_nul_w = impl == 2 ? (uint64_t)pl.hist_w + 256 : (uint64_t)pl.bbase_jobs * (uint64_t)pl.hist_w;
    pl.bhist_wg = impl == 2 ? ((pl.hist_cap + pl.hist_nul_w + 256 + 1024 + 7) & ~7ULL)      // data, NULL row, trash cells, slack
                            : ((uint64_t)pl.hist_levels * 5 + 1) * pl.hist_nul_w + 1024;
    // (The tail launch of the blocked kernel reuses slots 0 .. grid - 1 at another thread count: nothing above or below
    // depends on the threads of a workgroup -- bbase_jobs does only for the one-wave builds, which have no tail launch.)
    pl.bseg_wg = 2ULL * SR_BFS_MAXSEG * SR_BFS_SEGREC * 4;          // bytes
    pl.bbt_wg = (uint64_t)pl.bbase_jobs * SR_BFS_BTCAP * 4;        // bytes
    // breakpoint records of a primary (replay, sr_mirror_rule.h); allocated only by loads that have partners (load_device)
    pl.brec_wg = impl == 2 ? (uint64_t)SR_BPREC_MAX * SR_BPREC_INTS * 4 : 0;
    pl.bcl_wg = 0;                 // (round 3: breakpoint detection keeps a band per unit in LDS instead of a candidate list in global memory)
    pl.per_wg_bytes = pl.bring_wg * pl.rsz + pl.bhist_wg * pl.osz + pl.bseg_wg + pl.bbt_wg + pl.bcl_wg * 4 + (impl == 2 ? 32 * SR_BLK_MAK_SLOTS * 4 : 0) +
                      pl.brec_wg;       // (budgeted for every blocked load; a load without partners leaves it unallocated)
    (void)c;
    return SR_OK;
}

// memory budget: every buffer counted.  fixed = union-find arrays + per-pair arrays; then the CIGAR arena (worst
// case |q|+|t|+2 ops per pair; pairs run in batches that reuse it), the orientation rings and the alignment workspaces share
// what is left
static int plan_memory(sr_ctx *c, uint32_t np, Plan &pl, bool iterative = false) {
    size_t total_b = 0;
    HIPCHK(hipMemGetInfo(&pl.free_b, &total_b));
    const uint64_t fixed = 3ULL * c->uf_size * 8 + (uint64_t)np * 40 + (1ULL << 20);
    if (fixed + (64ULL << 20) > pl.free_b) return sr_fail(SR_ERR_NOMEM, "not enough device memory for the union-find arrays");
    const uint64_t avail = pl.free_b - fixed;
    pl.arena_ops = c->cigar_base[np] + 1;
    {
        uint64_t cap = std::max<uint64_t>((uint64_t)(avail * 0.25) / 4, pl.max_reserve + 1);
        if (const char *e = knob("SR_CIGAR_ARENA_OPS")) cap = std::max<uint64_t>((uint64_t)atoll(e), pl.max_reserve + 1);   // (tests: force batches)
        if (iterative)                // a phase-2 window holds at least one whole chunk
            for (uint64_t f = c->iter_tree_pairs; f < np; f += 4 * SR_ITER_CHECK_INTERVAL)
                cap = std::max<uint64_t>(cap, c->cigar_base[std::min<uint64_t>(np, f + 4 * SR_ITER_CHECK_INTERVAL)] - c->cigar_base[f] + 1);
        pl.arena_ops = std::min(pl.arena_ops, cap);
    }
    if (pl.arena_ops * 4 > avail / 2) return sr_fail(SR_ERR_NOMEM, "not enough device memory for one pair's CIGAR");
    c->batch_first.assign(1, 0);
    const uint32_t tp = iterative ? (uint32_t)c->iter_tree_pairs : np;
    for (uint32_t i = 0; i < tp; i++)
        if (c->cigar_base[i + 1] - c->cigar_base[c->batch_first.back()] + 1 > pl.arena_ops) c->batch_first.push_back(i);
    if (iterative) {
        // tree part ends on a batch boundary; then windows of whole chunks: 10 chunks first (the earliest possible stop),
        // doubling after each window, as many as the arena holds (>= 1)
        if (tp > 0 && tp < np) c->batch_first.push_back(tp);
        c->iter_tree_batches = tp == 0 ? 0 : (tp < np ? (uint32_t)c->batch_first.size() - 1 : (uint32_t)c->batch_first.size());
        const uint32_t CH = 4 * SR_ITER_CHECK_INTERVAL;
        uint64_t target = SR_ITER_STABILITY_THRESHOLD;
        c->iter_max_chunks = 0;
        for (uint32_t f = tp; f < np;) {
            uint32_t l = f, chunks = 0;
            while (l < np && (chunks == 0 || chunks < target)) {
                const uint32_t e = std::min(np, l + CH);
                if (chunks > 0 && c->cigar_base[e] - c->cigar_base[f] + 1 > pl.arena_ops) break;
                l = e; chunks++;
            }
            c->iter_max_chunks = std::max(c->iter_max_chunks, chunks);
            if (l < np) c->batch_first.push_back(l);
            f = l;
            target = std::min<uint64_t>(2 * target, 1ULL << 32);     // (doubling stops before it could wrap)
        }
    } else {
        c->iter_tree_batches = 0;
    }
    c->batch_first.push_back(np);
    pl.nbatch = (uint32_t)c->batch_first.size() - 1;
    pl.max_batch_pairs = 0;
    for (uint32_t b = 0; b < pl.nbatch; b++) pl.max_batch_pairs = std::max(pl.max_batch_pairs, c->batch_first[b + 1] - c->batch_first[b]);
    pl.left = avail - pl.arena_ops * 4;
    const uint64_t budget = (uint64_t)(pl.left * 0.7);
    int nwg = pl.cus * pl.wg_per_cu;
    if (const char *e = knob("SR_NWG")) nwg = std::max(1, std::min(nwg, atoi(e)));   // (tests: several pairs per workgroup on a small input)
    if ((uint64_t)nwg > pl.max_batch_pairs) nwg = (int)pl.max_batch_pairs;
    if (nwg < 1) nwg = 1;
    while (nwg > 1 && (uint64_t)nwg * pl.per_wg_bytes > budget) nwg--;
    if ((uint64_t)nwg * pl.per_wg_bytes > budget) return sr_fail(SR_ERR_NOMEM, "not enough device memory for one workgroup's wavefront ring");
    pl.nwg = c->nwg = nwg;
    return SR_OK;
}

// per-pair device arrays, workspaces, kernel arguments
// forced_strand (the patch pass of --patch-inversions): every query is loaded in the orientation it is to be aligned in and
// no orientation search may run: no orientation kernel and none of its buffers; the blocked kernel takes strand 0 as an
// input (pre_oriented), the level-per-pass kernel -- which always scores both copies and lets the forward one win ties -- is
// given the forward copy as its reverse-complement copy too, so the two searches are the same and forward is chosen
static int alloc_workspace(sr_ctx *c, const sr_params *p, const PackedSeqs &pk, const SeqDev &sd, const SrPen &pen, const SrPen &ori,
                           uint64_t maxlen, const std::vector<int32_t> &max_score, Plan &pl, bool forced_strand = false) {
    int r;
    void *d;
    const uint32_t np = (uint32_t)c->pair_q.size(), nbatch = pl.nbatch;
    const int impl = pl.impl, nwg = pl.nwg;
    const size_t osz = pl.osz, rsz = pl.rsz;
    SrAlignArgs &a = c->aa;
    memset(&a, 0, sizeof(a));
    uint32_t *d_pq, *d_pt;
    std::vector<uint32_t> pq = c->pair_q, pt = c->pair_t;
    if (pq.empty()) { pq.push_back(0); pt.push_back(0); }
    if ((r = dev_upload(c, pq, &d_pq))) return r;
    if ((r = dev_upload(c, pt, &d_pt))) return r;
    // per-batch relative CIGAR bases: batch b owns entries [first_b + b, first_b + b + count_b]
    std::vector<uint64_t> cb((size_t)np + nbatch, 0);
    for (uint32_t b = 0; b < nbatch; b++) {
        const uint32_t f = c->batch_first[b], l = c->batch_first[b + 1];
        for (uint32_t i = f; i <= l; i++) cb[(size_t)i + b] = c->cigar_base[i] - c->cigar_base[f];
    }
    if ((r = dev_upload(c, cb, &c->d_cbase))) return r;
    // cost-sorted dequeue order inside each batch: the longest pairs start first (self pairs last)
    std::vector<uint32_t> order(std::max<uint32_t>(np, 1), 0);
    for (uint32_t b = 0; b < nbatch; b++) {
        const uint32_t f = c->batch_first[b], l = c->batch_first[b + 1];
        std::vector<uint32_t> idx(l - f);
        for (uint32_t i = 0; i < l - f; i++) idx[i] = i;
        auto cost = [&](uint32_t i) { const uint32_t q = c->pair_q[f + i], t = c->pair_t[f + i];
                                      return q == t ? (uint64_t)c->len[q] : (uint64_t)c->len[q] * c->len[t]; };
        std::stable_sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) { return cost(x) > cost(y); });
        for (uint32_t i = 0; i < l - f; i++) order[f + i] = idx[i];
    }
    if ((r = dev_upload(c, order, &c->d_order))) return r;
    if ((r = dev_upload(c, max_score, &c->d_max_score))) return r;
    // mirror partners: blocked kernel on 2-bit buffers (elsewhere the reference's complement is no involution and the strand
    // decision loses its symmetry), pairs aligned with an orientation search
    std::vector<uint32_t> mirror;
    c->mirror_partners = 0;
    if (impl == 2 && pk.sm.bits == 2 && !forced_strand && np > 0) {
        mirror.assign(np, SR_MIRROR_NONE);
        if (!knob("SR_NO_MIRROR")) c->mirror_partners = mirror_map(c->pair_q.data(), c->pair_t.data(), c->batch_first.data(), nbatch, (uint32_t)nwg, mirror.data());
        if ((r = dev_upload(c, mirror, &c->d_mirror))) return r;
    }
    // primaries per batch: the tail launch's grid and the capacity of its list
    c->batch_partners.assign(nbatch, 0);
    uint32_t max_partners = 0;
    for (uint32_t b = 0; b < nbatch && !mirror.empty(); b++) {
        for (uint32_t i = c->batch_first[b]; i < c->batch_first[b + 1]; i++)
            if (mirror[i] != SR_MIRROR_NONE && !(mirror[i] & SR_MIRROR_SECONDARY)) c->batch_partners[b]++;
        max_partners = std::max(max_partners, c->batch_partners[b]);
    }
    HIPCHK(hipStreamSynchronize(c->stream));   // the uploads above have read their host vectors (pq, pt, cb, order, mirror)
    // queue_head, and behind it the tail launch's tail_count and tail_head: one memset per batch resets the three
    if ((r = dev_alloc(c, &d, 4 * sizeof(uint32_t)))) return r; c->d_queue = (uint32_t *)d;
    c->tail_threads = c->mirror_partners > 0 ? pl.tail_threads : 0;
    pl.tail_threads = c->tail_threads;
    if (c->tail_threads) {
        // workgroups per CU of the tail shape: 16 waves per CU (the kernel's register budget: 4 per SIMD), and its LDS
        c->tail_wg_per_cu = (int)std::max<size_t>(1, std::min<size_t>((size_t)1024 / c->tail_threads,
                                                                      (160 * 1024) / (c->lds_bytes + align_static_lds(false, 2, c->tail_threads))));
        const char *tl = knob("SR_TAIL"), *tr = knob("SR_TAIL_ROUNDS");
        c->tail_all = tl && !strcmp(tl, "all");
        c->tail_rounds = tr ? std::max(0, atoi(tr)) : SR_TAIL_ROUNDS_DEFAULT;
        c->tail_cus = pl.cus;
        if ((r = dev_alloc(c, &d, (size_t)max_partners * 4))) return r; c->d_tail_list = (uint32_t *)d;
        if ((r = dev_alloc(c, &d, sizeof(uint32_t)))) return r; c->d_tail_deferred = (uint32_t *)d;
        HIPCHK(hipMemsetAsync(c->d_tail_deferred, 0, sizeof(uint32_t), c->stream));
    }
    if (impl == 2 && knob("SR_PROFILE_TICKS") && atoi(knob("SR_PROFILE_TICKS")) != 0) {
        if ((r = dev_alloc(c, &d, (size_t)nwg * 4 * 8))) return r; c->d_timeline = (unsigned long long *)d;
        HIPCHK(hipMemsetAsync(c->d_timeline, 0, (size_t)nwg * 4 * 8, c->stream));
        if ((r = dev_alloc(c, &d, (size_t)nwg * 4 * 8))) return r; c->d_prio_timeline = (unsigned long long *)d;
        HIPCHK(hipMemsetAsync(c->d_prio_timeline, 0, (size_t)nwg * 4 * 8, c->stream));
    }
    if (impl == 2) {
        // rotating tile priority: the workgroups per CU the wave budget allows (16 waves per CU: 4 per SIMD); one per CU -- the
        // 1 024-thread shape -- has nothing to arbitrate and the rule is off, as under SR_TILE_PRIO=0
        if ((r = dev_alloc(c, &d, SR_PRIO_TABLE * sizeof(uint32_t)))) return r; c->d_cu_arrivals = (uint32_t *)d;
        HIPCHK(hipMemsetAsync(c->d_cu_arrivals, 0, SR_PRIO_TABLE * sizeof(uint32_t), c->stream));
        const char *tp = knob("SR_TILE_PRIO");
        a.prio_wg = std::max(1, std::min(pl.wg_per_cu, 1024 / std::max(64, c->nthreads)));
        a.tile_prio = (a.prio_wg > 1 && !(tp && atoi(tp) == 0)) ? 1 : 0;
        const char *trk = knob("SR_TAIL_ROUNDS");
        c->prio_rounds = trk ? std::max(0, atoi(trk)) : SR_TAIL_ROUNDS_DEFAULT;
    }
    if ((r = dev_alloc(c, &d, (uint64_t)nwg * pl.bring_wg * rsz))) return r; a.bring = d;
    if ((r = dev_alloc(c, &d, (uint64_t)nwg * pl.bhist_wg * osz))) return r; a.bhist = d;
    // (tests: the kernels must not depend on what the row workspaces held before -- poison them with plausible offsets)
    if (const char *e = knob("SR_POISON_ROWS")) {
        const int v = atoi(e);
        if (rsz == 2) HIPCHK(hipMemsetD16Async((hipDeviceptr_t)a.bring, (unsigned short)(pl.ring_u16 ? v - 24576 : v), (size_t)nwg * pl.bring_wg, c->stream));
        else HIPCHK(hipMemsetD32Async((hipDeviceptr_t)a.bring, v, (size_t)nwg * pl.bring_wg, c->stream));
        if (osz == 2) HIPCHK(hipMemsetD16Async((hipDeviceptr_t)a.bhist, (unsigned short)v, (size_t)nwg * pl.bhist_wg, c->stream));
        else HIPCHK(hipMemsetD32Async((hipDeviceptr_t)a.bhist, v, (size_t)nwg * pl.bhist_wg, c->stream));
    }
    if ((r = dev_alloc(c, &d, (uint64_t)nwg * pl.bseg_wg))) return r; a.bseg = (int *)d;
    if ((r = dev_alloc(c, &d, (uint64_t)nwg * pl.bbt_wg))) return r; a.bbt = (uint32_t *)d;
    {   // replay of tied secondaries: only where there are partners (SR_MIRROR_REPLAY=0: the kernel without it)
        const char *rpk = knob("SR_MIRROR_REPLAY");
        pl.brec_bytes = 0;
        if (impl == 2 && c->mirror_partners > 0 && pl.brec_wg && !(rpk && atoi(rpk) == 0)) {
            pl.brec_bytes = (uint64_t)nwg * pl.brec_wg;
            if ((r = dev_alloc(c, &d, pl.brec_bytes))) return r; a.brec = (int *)d;
        }
    }
    if (pl.bcl_wg) { if ((r = dev_alloc(c, &d, (uint64_t)nwg * pl.bcl_wg * 4))) return r; a.bcl = (uint32_t *)d; a.bcl_wg_stride = pl.bcl_wg; }
    if (impl == 2) { if ((r = dev_alloc(c, &d, (uint64_t)nwg * 32 * SR_BLK_MAK_SLOTS * 4))) return r; a.bmak = (int *)d; }
    // orientation as its own kernel, one pair per wave (sr_orient.hip); SR_PREORIENT=0 keeps it in the alignment kernel.
    // Worth it when there are enough pairs to fill the chip with one wave each and the three sequence copies of a
    // wave leave >= 8 waves per CU (measured: C2 / C4 faster; C3 -- 144 pairs -- 1.6x and C5 -- 50 kb, 4 waves per
    // CU by LDS -- 9 % slower than orientation inside the alignment kernel's workgroup).  SR_PREORIENT=1 / 0 forces.
    const char *po = knob("SR_PREORIENT");
    const bool pre_auto = (uint64_t)np >= 4ULL * (uint64_t)pl.cus && (size_t)pl.max_words * 12 <= 20 * 1024;
    if (!forced_strand && impl == 2 && (po ? atoi(po) != 0 : pre_auto) && (size_t)pl.max_words * 12 <= 60 * 1024) {
        const int orow = (int)((2 * ((2 * maxlen + 32) & ~3ULL) + 512 + 7) & ~7ULL);
        const uint64_t oring_wg = ((uint64_t)(ori.scope + 1) * 3 + 1) * (uint64_t)orow + 256;
        int onwg = (int)std::min<uint64_t>(pl.max_batch_pairs, (uint64_t)pl.cus * 16);
        while (onwg > 1 && (uint64_t)onwg * oring_wg * osz > (uint64_t)(pl.left * 0.2)) onwg--;
        if (onwg >= 1 && np > 0) {
            pl.oring_bytes = (uint64_t)onwg * oring_wg * osz;
            if ((r = dev_alloc(c, &d, pl.oring_bytes))) return r; a.oring = d;
            if ((r = dev_alloc(c, &d, sizeof(uint32_t)))) return r; c->d_oqueue = (uint32_t *)d;
            a.oring_wg_stride = oring_wg; a.orow = orow; a.oqueue = c->d_oqueue; a.pre_oriented = 1;
            if (!knob("SR_NO_REORDER")) {       // dequeue order from the orientation scores, per batch
                c->otemp_bytes = srk_order_temp_bytes(pl.max_batch_pairs);
                if ((r = dev_alloc(c, &d, (uint64_t)pl.max_batch_pairs * 8))) return r; c->d_okeys = (uint64_t *)d;
                if ((r = dev_alloc(c, &d, (uint64_t)pl.max_batch_pairs * 8))) return r; c->d_okeys2 = (uint64_t *)d;
                if ((r = dev_alloc(c, &d, (uint64_t)pl.max_batch_pairs * 4))) return r; c->d_ovals = (uint32_t *)d;
                if ((r = dev_alloc(c, &d, std::max<size_t>(c->otemp_bytes, 16)))) return r; c->d_otemp = d;
            }
            c->onwg = onwg; c->olds_bytes = (size_t)pl.max_words * 3 * 4;
        }
    }
    if ((r = dev_alloc(c, &d, (size_t)np + 1))) return r; a.is_reverse = (uint8_t *)d;
    if ((r = dev_alloc(c, &d, ((size_t)np + 1) * 4))) return r; a.score = (int32_t *)d;
    if ((r = dev_alloc(c, &d, ((size_t)np + 1) * 4))) return r; a.ori_fwd = (int32_t *)d;
    if ((r = dev_alloc(c, &d, ((size_t)np + 1) * 4))) return r; a.ori_rev = (int32_t *)d;
    if ((r = dev_alloc(c, &d, ((size_t)np + 1) * 4))) return r; a.cigar_cnt = (uint32_t *)d;
    if ((r = dev_alloc(c, &d, (pl.arena_ops + 1) * 4))) return r; a.cigar_ops = (uint32_t *)d;
    if ((r = dev_alloc(c, &d, SR_NCOUNTERS * sizeof(unsigned long long)))) return r; c->d_counters = (unsigned long long *)d;
    if ((r = dev_alloc(c, &d, sizeof(int)))) return r; c->d_error = (int *)d;
    if ((r = dev_alloc(c, &d, c->uf_size * 8))) return r; c->d_nodes = (unsigned long long *)d;
    if ((r = dev_alloc(c, &d, c->uf_size * 8))) return r; c->d_minarr = (unsigned long long *)d;
    if ((r = dev_alloc(c, &d, c->uf_size * 8))) return r; c->d_labels = (unsigned long long *)d;
    HIPCHK(hipMemsetAsync(c->d_counters, 0, SR_NCOUNTERS * sizeof(unsigned long long), c->stream));
    HIPCHK(hipMemsetAsync(c->d_error, 0, sizeof(int), c->stream));
    HIPCHK(hipMemsetAsync(a.cigar_cnt, 0, ((size_t)np + 1) * 4, c->stream));
    HIPCHK(hipMemsetAsync(a.score, 0xff, ((size_t)np + 1) * 4, c->stream));
    if (forced_strand) {
        HIPCHK(hipMemsetAsync(a.is_reverse, 0, (size_t)np + 1, c->stream));
        HIPCHK(hipMemsetAsync(a.ori_fwd, 0, ((size_t)np + 1) * 4, c->stream));
        HIPCHK(hipMemsetAsync(a.ori_rev, 0, ((size_t)np + 1) * 4, c->stream));
    }
    a.seqwords = sd.words; a.word_off_fwd = sd.woff[0]; a.word_off_rc = sd.woff[1]; a.word_off_rev = sd.woff[2]; a.word_off_cmp = sd.woff[3];
    if (forced_strand) { if (impl == 2) a.pre_oriented = 1; else a.word_off_rc = a.word_off_fwd; }
    a.symbits = pk.sm.bits; a.order = c->d_order; a.seqlen = sd.len;
    a.max_words = pl.max_words; a.pair_q = d_pq; a.pair_t = d_pt; a.npairs = np;
    a.queue_head = c->d_queue; a.pen = pen; a.ori = ori; a.mem_mode = p->memory_mode;
    a.ring_scope = pl.ring_scope; a.ring_hot = pl.ring_hot;
    a.hist_w = pl.hist_w; a.hist_levels = pl.hist_levels;
    { const char *pt_ = knob("SR_PROFILE_TICKS"); a.profile_ticks = (pt_ && atoi(pt_) != 0) ? 1 : 0; }
    a.impl = impl; a.kdepth = pl.kdepth; a.kdepth2 = pl.kdepth2; a.kblock = pl.kblock; a.lazy_id = pl.lazy_id; a.ring_u16 = pl.ring_u16;
    a.ori_levels = knob("SR_ORIENT_LEVELS") ? 1 : 0;
    { const char *tb = knob("SR_TEST_BASE_LEVELS"); a.test_base_levels = tb ? std::max(0, atoi(tb)) : 0; }
    a.bring_wg_stride = pl.bring_wg; a.brow = pl.brow; a.bhist_wg_stride = pl.bhist_wg; a.bbase_jobs = pl.bbase_jobs;
    a.hist_cap = pl.hist_cap; a.hist_nul_w = (uint32_t)pl.hist_nul_w; a.hist_stride = (uint32_t)((uint64_t)pl.bbase_jobs * (uint64_t)pl.hist_w);
    a.cigar_base = c->d_cbase; a.counters = c->d_counters; a.error_flag = c->d_error;
    // 8-mer sets of the sequences (8 KB each) for the orientation kernel's lower bound of the reverse orientation's score:
    // plain ACGT buffers, default orientation penalties (the blocked orientation kernel), at most 256 MB and 5 % of what
    // is left.  SR_NO_KBITS=1 switches the bound off (both orientations in lockstep from level 0, as before round 3).
    if (a.pre_oriented && pk.sm.bits == 2 && !ori.two && ori.x == 1 && ori.o1 == 1 && ori.e1 == 1 && !knob("SR_NO_KBITS") && !knob("SR_ORIENT_LEVELS")) {
        const uint64_t kb = (uint64_t)c->len.size() * 8192ull;
        if (kb > 0 && kb <= (256ull << 20) && kb <= (uint64_t)(pl.left * 0.05)) {
            if ((r = dev_alloc(c, &d, kb))) return r;
            if ((r = srk_kmer_bits(&a, (uint32_t)c->len.size(), (uint32_t *)d, c->stream))) return sr_fail(SR_ERR_DEVICE_FAULT, "k-mer set kernel failed to launch");
            a.kbits = (const uint32_t *)d;
        }
    }
    SrUniteArgs &u = c->ua;
    memset(&u, 0, sizeof(u));
    u.pair_q = d_pq; u.pair_t = d_pt; u.npairs = np; u.seqlen = sd.len; u.seq_goff = sd.goff;
    a.fuse_unite = 0; a.uf_nodes = c->d_nodes; a.seq_goff = sd.goff; a.max_score = c->d_max_score; a.min_match_len = p->min_match_len;
    a.mirror = c->d_mirror;
    // (tail_list is set per batch, enqueue_align_batch: NULL unless the batch defers)
    a.tail_count = c->d_queue + 1; a.tail_head = c->d_queue + 2; a.tail_deferred = c->d_tail_deferred; a.timeline = c->d_timeline;
    a.cu_arrivals = c->d_cu_arrivals; a.prio_timeline = c->d_prio_timeline;
    c->fuse_unite = impl == 2 && !knob("SR_NO_FUSED_UNITE");
    u.is_reverse = a.is_reverse; u.score = a.score; u.max_score = c->d_max_score;
    u.cigar_ops = a.cigar_ops; u.cigar_base = c->d_cbase; u.cigar_cnt = a.cigar_cnt;
    u.min_match_len = p->min_match_len; u.nodes = c->d_nodes; u.uf_size = c->uf_size;
    u.counters = c->d_counters; u.error_flag = c->d_error;
    return SR_OK;
}

static void write_report(sr_ctx *c, const PackedSeqs &pk, const SrPen &pen, const Plan &pl) {
    const uint32_t np = (uint32_t)c->pair_q.size();
    char buf[3072];
    // which build the launchers take (srk_align: lean wave build / wide level kernel; srk_orient: blocked or level by level)
    const SrPen &ori = c->aa.ori;
    const char *oroute = c->onwg == 0 ? "in-kernel"
                         : (!ori.two && ori.x == 1 && ori.o1 == 1 && ori.e1 == 1 && !knob("SR_ORIENT_LEVELS")) ? "orient-blk" : "orient-levels";
    snprintf(buf, sizeof(buf),
             "{\"pairs\": %u, \"batches\": %u, \"symbol_bits\": %d, \"offset_bytes\": %zu, \"ring_cell_bytes\": %zu, \"kernel_impl\": %d, "
             "\"block_levels\": %d, \"two_piece\": %d, \"lazy_id_rows\": %d, \"workgroups\": %d, "
             "\"threads_per_workgroup\": %d, \"workgroups_per_cu\": %d, \"lds_dynamic_bytes\": %zu, \"ring_bytes_per_workgroup\": %llu, "
             "\"base_history_bytes_per_workgroup\": %llu, \"workspace_bytes\": %llu, \"cigar_arena_bytes\": %llu, "
             "\"orientation_ring_bytes\": %llu, \"union_find_bytes\": %llu, \"device_free_bytes_at_load\": %zu, \"kernel_build\": \"%s\", "
             "\"ring_depth_m\": %d, \"ring_depth_id\": %d, \"fused_unite\": %d, \"wave_build\": %d, \"level_kernel_wide\": %d, "
             "\"profile_ticks\": %d, \"orientation_route\": \"%s\", \"source_digest\": \"%s\", \"mirror_partners\": %llu, \"tail_threads\": %d, \"mirror_replay\": %d, \"replay_record_bytes\": %llu, \"tile_prio\": %d, \"prio_epoch_shift\": %d, \"prio_workgroups_per_cu\": %d, \"knobs\": ",
             np, pl.nbatch, pk.sm.bits, pl.osz, pl.impl == 2 ? pl.rsz : pl.osz, pl.impl, pl.impl == 2 ? pl.kblock : 1, pen.two ? 1 : 0, pl.lazy_id,
             pl.nwg, c->nthreads, pl.wg_per_cu, c->lds_bytes,
             (unsigned long long)(pl.bring_wg * pl.rsz), (unsigned long long)(pl.bhist_wg * pl.osz),
             (unsigned long long)((uint64_t)pl.nwg * pl.per_wg_bytes), (unsigned long long)(pl.arena_ops * 4), (unsigned long long)pl.oring_bytes,
             (unsigned long long)(3ULL * c->uf_size * 8), pl.free_b, srk_align_blk_build_tag(), pl.kdepth, pl.kdepth2, c->fuse_unite ? 1 : 0,
             pl.wave_wg ? 1 : 0, (pl.impl == 1 && pl.ring_scope + 1 > 32) ? 1 : 0, c->aa.profile_ticks, oroute, srk_source_digest(),
             (unsigned long long)c->mirror_partners, c->tail_threads, pl.brec_bytes ? 1 : 0, (unsigned long long)pl.brec_bytes,
             c->aa.tile_prio, SR_PRIO_EPOCH_SHIFT, c->aa.prio_wg);
    c->workspace_report = std::string(buf) + knobs_json() + "}";
}

int load_impl(sr_ctx *c, const sr_seqset *seqs, const sr_params *p, const uint32_t *eq, const uint32_t *et,
                     uint64_t ecount, bool explicit_pairs, bool iterative, bool forced_strand, uint32_t ext_n_old) {
    if (!c || !seqs || !p) return sr_fail(SR_ERR_INVALID, "null argument");
    if (seqs->n == 0) return sr_fail(SR_ERR_INVALID, "no sequences");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    free_dev(c);
    int r;
    SrPen pen, ori;
    uint64_t maxlen = 0;
    if ((r = load_index(c, seqs, p, explicit_pairs, &pen, &ori, &maxlen))) return r;
    PackedSeqs pk;
    pack_sequences(c, seqs, pk);
    c->symbits = pk.sm.bits;
    SeqDev sd;
    if ((r = upload_sequences(c, seqs, pk, sd))) return r;
    Plan pl;
    std::vector<int32_t> max_score;
    if ((r = build_pair_list(c, p, sd, eq, et, ecount, explicit_pairs, max_score, &pl.max_reserve, iterative, ext_n_old))) return r;
    const uint32_t np = (uint32_t)c->pair_q.size();
    if ((r = plan_kernel(c, pk, pen, ori, maxlen, np, pl))) return r;
    if ((r = plan_workspace(c, pen, ori, maxlen, pl))) return r;
    if ((r = plan_memory(c, np, pl, iterative))) return r;
    if ((r = alloc_workspace(c, p, pk, sd, pen, ori, maxlen, max_score, pl, forced_strand))) return r;
    write_report(c, pk, pen, pl);
    c->t_first_kernel = std::chrono::steady_clock::now();
    if (srk_uf_init(c->d_nodes, c->total_len, c->uf_size, c->stream)) return sr_fail(SR_ERR_HIP, "uf init launch failed");
    HIPCHK(hipStreamSynchronize(c->stream));
    c->loaded = true;
    return SR_OK;
}

extern "C" int sr_ctx_load(sr_ctx *c, const sr_seqset *seqs, const sr_params *p) {
    return unload_if_failed(c, load_impl(c, seqs, p, nullptr, nullptr, 0, false));
}
extern "C" int sr_ctx_load_pairs(sr_ctx *c, const sr_seqset *seqs, const sr_params *p, const uint32_t *query_idx,
                                 const uint32_t *target_idx, uint64_t count) {
    if (count && (!query_idx || !target_idx)) return sr_fail(SR_ERR_INVALID, "null pair list");
    return unload_if_failed(c, load_impl(c, seqs, p, query_idx, target_idx, count, true));
}

extern "C" int sr_ctx_pairs(const sr_ctx *c, uint32_t **q_out, uint32_t **t_out, uint64_t *count) {
    if (!c || !c->loaded || !q_out || !t_out || !count) return sr_fail(SR_ERR_INVALID, "context not loaded");
    *count = c->pair_q.size();
    const int r = to_malloc(c->pair_q, q_out);
    return r ? r : to_malloc(c->pair_t, t_out);
}
// the orientation scores the alignment stage left per pair (forward; reverse complement, INT32_MAX where it was not better)
extern "C" int sr_ctx_orientation_scores(sr_ctx *c, int32_t *fwd, int32_t *rev) {
    if (!c || !c->loaded || c->from_paf || !c->aa.ori_fwd) return sr_fail(SR_ERR_INVALID, "context has no alignment stage");
    const size_t np = c->pair_q.size();
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (fwd && np) HIPCHK(hipMemcpy(fwd, c->aa.ori_fwd, np * 4, hipMemcpyDeviceToHost));
    if (rev && np) HIPCHK(hipMemcpy(rev, c->aa.ori_rev, np * 4, hipMemcpyDeviceToHost));
    return SR_OK;
}
extern "C" uint32_t sr_ctx_num_batches(const sr_ctx *c) { return (c && c->loaded) ? (uint32_t)c->batch_first.size() - 1 : 0; }
extern "C" const char *sr_ctx_workspace_report(const sr_ctx *c) { return c ? c->workspace_report.c_str() : ""; }

// --extend: the seed of the loaded plan on the context's stream, hipEvents around it
static int enqueue_extend_seed(sr_ctx *c) {
    for (hipEvent_t &e : c->ext_ev) if (!e) HIPCHK(hipEventCreate(&e));
    HIPCHK(hipMemsetAsync(c->ext.counts, 0, 2 * sizeof(unsigned long long), c->stream));
    HIPCHK(hipEventRecord(c->ext_ev[0], c->stream));
    const int r = srk_extend_seed(&c->ext, c->stream);
    if (r) return sr_fail(SR_ERR_HIP, std::string("extend seed launch failed: ") + hipGetErrorString((hipError_t)r));
    HIPCHK(hipEventRecord(c->ext_ev[1], c->stream));
    return SR_OK;
}

extern "C" int sr_ctx_reset_uf(sr_ctx *c) {
    if (!c || !c->loaded) return sr_fail(SR_ERR_INVALID, "context not loaded");
    HIPCHK(hipSetDevice(c->device));
    if (srk_uf_init(c->d_nodes, c->total_len, c->uf_size, c->stream)) return sr_fail(SR_ERR_HIP, "uf init launch failed");
    if (c->ext_loaded) return enqueue_extend_seed(c);      // a context of sr_ctx_load_extend starts from the input graph's partition
    return SR_OK;
}

// sr_ctx_load of the plan's merged set with the pair filter, then the seed tables and the seed (include/seqrush_amd.h)
static int load_extend(sr_ctx *c, const sr_extend_plan *plan, const sr_params *p) {
    if (!c || !plan || !p) return sr_fail(SR_ERR_INVALID, "null argument");
    if (plan->n_new == 0) return sr_fail(SR_ERR_INVALID, "extend: no new sequences: there is nothing to align");
    int r = load_impl(c, &plan->merged, p, nullptr, nullptr, 0, false, false, false, plan->n_old);
    if (r) return r;
    if (plan->old_bases > c->total_len || plan->S == 0 || plan->sinc[plan->S - 1] != plan->old_bases) {
        c->loaded = false;
        return sr_fail(SR_ERR_INVALID, "extend: the plan's tables do not match its merged set");
    }
    const uint64_t before = c->ext_stats.pairs_before, after = c->ext_stats.pairs_after;
    sr_extend_plan_stats(plan, &c->ext_stats);
    c->ext_stats.pairs_before = before; c->ext_stats.pairs_after = after;
    void *d_steps = nullptr, *d_len = nullptr, *d_sinc = nullptr, *d_anchor = nullptr, *d_counts = nullptr;
    if ((r = dev_alloc(c, &d_steps, (size_t)plan->S * 4)) || (r = dev_alloc(c, &d_len, (size_t)plan->V * 4)) ||
        (r = dev_alloc(c, &d_sinc, (size_t)plan->S * 8)) || (r = dev_alloc(c, &d_anchor, (size_t)plan->V * 4)) ||
        (r = dev_alloc(c, &d_counts, 2 * sizeof(unsigned long long)))) { c->loaded = false; return r; }
    c->loaded = false;                                       // until the tables are in place
    HIPCHK(hipMemcpyAsync(d_steps, plan->steps.data(), (size_t)plan->S * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_len, plan->len.data(), (size_t)plan->V * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_sinc, plan->sinc.data(), (size_t)plan->S * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(d_anchor, 0xff, (size_t)plan->V * 4, c->stream));
    c->ext.steps = (const uint32_t *)d_steps; c->ext.len = (const uint32_t *)d_len; c->ext.sinc = (const uint64_t *)d_sinc;
    c->ext.anchor = (uint32_t *)d_anchor; c->ext.S = plan->S; c->ext.V = plan->V; c->ext.bases = plan->old_bases;
    c->ext.nodes = c->d_nodes; c->ext.counts = (unsigned long long *)d_counts; c->ext.error_flag = c->d_error;
    if ((r = srk_extend_anchor(&c->ext, c->stream))) return sr_fail(SR_ERR_HIP, std::string("extend anchor launch failed: ") + hipGetErrorString((hipError_t)r));
    HIPCHK(hipStreamSynchronize(c->stream));                 // (the plan's vectors may go away after this)
    c->loaded = true; c->ext_loaded = true;
    return enqueue_extend_seed(c);
}
extern "C" int sr_ctx_load_extend(sr_ctx *c, const sr_extend_plan *plan, const sr_params *p) {
    return unload_if_failed(c, load_extend(c, plan, p));
}

extern "C" int sr_ctx_extend_stats(sr_ctx *c, sr_extend_stats *out) {
    if (!c || !out || !c->loaded || !c->ext_loaded) return sr_fail(SR_ERR_INVALID, "context was not loaded by sr_ctx_load_extend");
    unsigned long long cnt[2] = {0, 0};
    const int r = ctx_read(c, cnt, c->ext.counts, sizeof(cnt));
    if (r) return r;
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, c->ext_ev[0], c->ext_ev[1]));
    c->ext_stats.unions_attempted = cnt[0]; c->ext_stats.unions_joined = cnt[1];
    c->ext_stats.seed_us = (uint64_t)(ms * 1000.0 + 0.5);
    *out = c->ext_stats;
    return SR_OK;
}

// kernel arguments of batch b: the per-pair arrays shifted to the batch, its slice of d_cbase
void batch_args(const sr_ctx *c, uint32_t b, SrAlignArgs *a, SrUniteArgs *u) {
    const uint32_t f = c->batch_first[b], cnt = c->batch_first[b + 1] - f;
    if (a) {
        *a = c->aa;
        a->pair_q += f; a->pair_t += f; a->npairs = cnt; if (a->order) a->order += f;
        a->is_reverse += f; a->score += f; a->ori_fwd += f; a->ori_rev += f; a->cigar_cnt += f;
        if (a->max_score) a->max_score += f;
        if (a->mirror) a->mirror += f;
        a->cigar_base = c->d_cbase + f + b;
    }
    if (u) {
        *u = c->ua;
        u->pair_q += f; u->pair_t += f; u->npairs = cnt; u->is_reverse += f; u->score += f; u->max_score += f;
        u->cigar_cnt += f; u->cigar_base = c->d_cbase + f + b;
        if (u->q_start) { u->q_start += f; u->t_start += f; }
    }
}

int enqueue_align_batch(sr_ctx *c, uint32_t b, bool fuse_unite) {
    SrAlignArgs a;
    batch_args(c, b, &a, nullptr);
    a.fuse_unite = fuse_unite ? 1 : 0;
    // Tail launch: the batch defers when it has partners and its alignments (pairs minus secondaries) are at most
    // tail_rounds x the launch's workgroups -- beyond, one solo alignment at the end is noise (SR_TAIL=all: always)
    const int main_wg = std::min<int>(c->nwg, (int)a.npairs);
    const uint32_t partners = c->tail_threads && b < c->batch_partners.size() ? c->batch_partners[b] : 0;
    const bool defer = partners > 0 && (c->tail_all || (uint64_t)(a.npairs - partners) <= (uint64_t)c->tail_rounds * (uint64_t)main_wg);
    a.tail_list = defer ? c->d_tail_list : nullptr;
    a.tail_mode = defer && c->tail_all ? SR_TAIL_DEFER_ALL : SR_TAIL_MAIN;
    // Rotating tile priority: short lists only, by the tail launch's rule (alignments <= SR_TAIL_ROUNDS x workgroups).  What the
    // rotation evens out is the end of a round of alignments; a long list (C4: 60 rounds) keeps every CU full until its last
    // round whoever is served first, and measured 0.7 % slower with the rotation than without.
    const uint32_t secondaries = b < c->batch_partners.size() ? std::min<uint32_t>(c->batch_partners[b], a.npairs) : 0;
    if ((uint64_t)(a.npairs - secondaries) > (uint64_t)c->prio_rounds * (uint64_t)main_wg) a.tile_prio = 0;
    HIPCHK(hipMemsetAsync(c->d_queue, 0, (c->tail_threads ? 3 : 1) * sizeof(uint32_t), c->stream));
    hipEvent_t *e0, *e1;
    int r;
    if (c->onwg > 0 && a.npairs > 0) {           // which = 4: the orientation kernel
        HIPCHK(hipMemsetAsync(c->d_oqueue, 0, sizeof(uint32_t), c->stream));
        if ((r = ev_get(c, 4, c->ev_used[4], &e0, &e1))) return r;
        HIPCHK(hipEventRecord(*e0, c->stream));
        r = srk_orient(&a, std::min<int>(c->onwg, (int)a.npairs), c->olds_bytes, c->off16, c->stream);
        if (r) return sr_fail(SR_ERR_HIP, std::string("orientation kernel launch failed: ") + hipGetErrorString((hipError_t)r));
        if (c->d_okeys && a.order) {             // longest predicted alignment first (orientation score x length)
            r = srk_order(&a, c->d_okeys, c->d_okeys2, c->d_ovals, c->d_otemp, c->otemp_bytes, (uint32_t *)a.order, c->stream);
            if (r) return sr_fail(SR_ERR_HIP, std::string("dequeue-order sort failed: ") + hipGetErrorString((hipError_t)r));
        }
        HIPCHK(hipEventRecord(*e1, c->stream));
        c->ev_used[4]++;
    }
    if ((r = ev_get(c, 0, c->ev_used[0], &e0, &e1))) return r;
    HIPCHK(hipEventRecord(*e0, c->stream));
    if (a.npairs > 0) {
        if (a.cu_arrivals) HIPCHK(hipMemsetAsync(a.cu_arrivals, 0, SR_PRIO_TABLE * sizeof(uint32_t), c->stream));
        r = srk_align(&a, main_wg, c->lds_bytes, c->off16, c->nthreads, c->stream);
        if (r) return sr_fail(SR_ERR_HIP, std::string("align kernel launch failed: ") + hipGetErrorString((hipError_t)r));
        if (defer) {
            // the same kernel at the tail shape, one workgroup per CU slot, on workspace slots 0 .. grid - 1 of the main launch
            // (the kernel boundary orders the list); an empty list makes every workgroup return at once
            const int grid = (int)std::min<uint64_t>({(uint64_t)c->tail_cus * (uint64_t)c->tail_wg_per_cu, (uint64_t)c->nwg, (uint64_t)partners});
            a.tail_mode = SR_TAIL_RUN; a.timeline = nullptr;
            a.cu_arrivals = nullptr; a.prio_timeline = nullptr; a.tile_prio = 0;       // (one workgroup per CU slot: no rank, tile code at 0)
            r = srk_align(&a, grid, c->lds_bytes, c->off16, c->tail_threads, c->stream);
            if (r) return sr_fail(SR_ERR_HIP, std::string("align kernel tail launch failed: ") + hipGetErrorString((hipError_t)r));
        }
    }
    HIPCHK(hipEventRecord(*e1, c->stream));
    c->ev_used[0]++;
    return SR_OK;
}

int enqueue_unite_batch(sr_ctx *c, uint32_t b, bool fused) {
    SrUniteArgs u;
    batch_args(c, b, nullptr, &u);
    hipEvent_t *e0, *e1;
    int r;
    if ((r = ev_get(c, 1, c->ev_used[1], &e0, &e1))) return r;
    HIPCHK(hipEventRecord(*e0, c->stream));
    if (u.npairs > 0 && !fused) {                  // (fused: the alignment kernel did it; the empty event pair keeps kernel_ms(1) defined)
        int nwg = (int)std::min<uint64_t>(u.npairs, 4096);
        r = srk_unite(&u, nwg, c->stream);
        if (r) return sr_fail(SR_ERR_HIP, std::string("unite kernel launch failed: ") + hipGetErrorString((hipError_t)r));
    }
    HIPCHK(hipEventRecord(*e1, c->stream));
    c->ev_used[1]++;
    return SR_OK;
}

int begin_pass(sr_ctx *c, bool reset_counters) {
    HIPCHK(hipSetDevice(c->device));
    if (reset_counters) {
        HIPCHK(hipMemsetAsync(c->d_counters, 0, SR_NCOUNTERS * sizeof(unsigned long long), c->stream));
        if (c->d_tail_deferred) HIPCHK(hipMemsetAsync(c->d_tail_deferred, 0, sizeof(uint32_t), c->stream));
        c->ev_used[0] = c->ev_used[4] = 0;
    }
    return SR_OK;
}

extern "C" int sr_ctx_align(sr_ctx *c) {
    if (!c || !c->loaded) return sr_fail(SR_ERR_INVALID, "context not loaded");
    if (c->from_paf) return sr_fail(SR_ERR_INVALID, "context was loaded from a PAF file: there is no alignment stage");
    if (c->batch_first.size() > 2)
        return sr_fail(SR_ERR_UNSUPPORTED, "the pair list runs in several batches that share one CIGAR arena: use sr_ctx_run "
                                        "(align + unite per batch) or sr_align_all");
    int r = begin_pass(c, true);
    if (r) return r;
    if ((r = enqueue_align_batch(c, 0))) return r;
    c->aligned_batch_valid = true;
    return SR_OK;
}

extern "C" int sr_ctx_unite(sr_ctx *c) {
    if (!c || !c->loaded) return sr_fail(SR_ERR_INVALID, "context not loaded");
    if (c->batch_first.size() > 2) return sr_fail(SR_ERR_UNSUPPORTED, "several batches: use sr_ctx_run");
    HIPCHK(hipSetDevice(c->device));
    c->ev_used[1] = 0;
    return enqueue_unite_batch(c, 0);
}

// alignment + match-run extraction + unite of the whole pair list, batch after batch (no host sync, unless inversion
// patching is on: then the scan's job list is read after every batch and the patch pass follows the last one)
extern "C" int sr_ctx_run(sr_ctx *c) {
    if (!c || !c->loaded) return sr_fail(SR_ERR_INVALID, "context not loaded");
    int r = begin_pass(c, !c->from_paf);
    if (r) return r;
    c->ev_used[1] = 0;
    const uint32_t nbatch = (uint32_t)c->batch_first.size() - 1;
    const bool fuse = c->fuse_unite && !c->from_paf;
    if (c->inv_on && (r = inv_begin_run(c))) return r;
    for (uint32_t b = 0; b < nbatch; b++) {
        if (!c->from_paf && (r = enqueue_align_batch(c, b, fuse))) return r;
        if ((r = enqueue_unite_batch(c, b, fuse))) return r;
        if (c->inv_on && (r = inv_scan_batch(c, b))) return r;
    }
    c->aligned_batch_valid = nbatch == 1 && !c->from_paf;
    if (c->inv_on && (r = inv_patch_pass(c))) return r;
    return SR_OK;
}

extern "C" int sr_ctx_sync(sr_ctx *c) {
    if (!c) return sr_fail(SR_ERR_INVALID, "null ctx");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->loaded) {
        int err = 0;
        HIPCHK(hipMemcpy(&err, c->d_error, sizeof(int), hipMemcpyDeviceToHost));
        if (err) {
            static const char *names[9] = {"score bound exceeded", "base-case history overflow", "backtrace found no predecessor",
                                           "recursion stack / segment list overflow", "CIGAR buffer overflow", "union-find retry bound",
                                           "breakpoint outside its segment", "graph induction",
                                           "row / LDS address outside the workgroup's extent (bounds-checked build)"};
            std::string msg = "device reported internal fault bits";
            char buf[32];
            snprintf(buf, sizeof(buf), " 0x%x:", err);
            msg += buf;
            for (int b = 0; b < 9; b++) if (err & (1 << b)) { msg += " ["; msg += names[b]; msg += "]"; }
            if (err & SR_DEV_ERR_ADDRESS) {                  // first offender: counters[40..43] = pair + 1, what, offset, extent
                uint64_t d[4] = {0, 0, 0, 0};
                if (hipMemcpy(d, c->d_counters + 40, sizeof(d), hipMemcpyDeviceToHost) == hipSuccess && d[0]) {
                    char b2[160];
                    snprintf(b2, sizeof(b2), " first: pair #%llu, %s, offset %llu, extent %llu", (unsigned long long)(d[0] - 1),
                             d[1] == 1 ? "ring row" : d[1] == 2 ? "history row" : "LDS window", (unsigned long long)d[2], (unsigned long long)d[3]);
                    msg += b2;
                }
            }
            // which pair(s): a failed alignment leaves score -1
            if (!c->from_paf && c->aa.score) {
                const size_t np = c->pair_q.size();
                std::vector<int32_t> sc(np);
                if (np && hipMemcpy(sc.data(), c->aa.score, np * 4, hipMemcpyDeviceToHost) == hipSuccess) {
                    int shown = 0;
                    for (size_t i = 0; i < np && shown < 4; i++)
                        if (sc[i] < 0) { snprintf(buf, sizeof(buf), " pair(%u,%u)", c->pair_q[i], c->pair_t[i]); msg += buf; shown++; }
                }
            }
            return sr_fail(SR_ERR_DEVICE_FAULT, msg);
        }
    }
    return SR_OK;
}

extern "C" uint64_t sr_ctx_uf_size(const sr_ctx *c) { return c ? c->uf_size : 0; }
extern "C" uint64_t sr_ctx_num_pairs(const sr_ctx *c) { return c ? c->pair_q.size() : 0; }
extern "C" uint64_t sr_ctx_dp_cells(const sr_ctx *c) { return c ? c->dp_cells : 0; }

extern "C" const char *sr_ctx_align_kernel(const sr_ctx *c) {
    if (!c || !c->loaded || c->from_paf) return nullptr;
    return c->aa.impl == 2 ? "sr_align_blk_kernel" : "sr_align_bfs_kernel";
}

extern "C" int sr_ctx_kernel_ms(sr_ctx *c, int which, float *ms) {
    if (!c || which < 0 || which > 4 || c->ev_used[which] == 0) return sr_fail(SR_ERR_INVALID, "no timing recorded");
    float tot = 0;
    for (int i = 0; i < c->ev_used[which]; i++) {
        float t = 0;
        HIPCHK(hipEventSynchronize(c->ev[which][i].second));
        HIPCHK(hipEventElapsedTime(&t, c->ev[which][i].first, c->ev[which][i].second));
        tot += t;
    }
    *ms = tot;
    return SR_OK;
}

static int counters_read(sr_ctx *c, uint64_t *out, uint32_t n) {
    if (!c || !c->loaded) return sr_fail(SR_ERR_INVALID, "context not loaded");
    return ctx_read(c, out, c->d_counters, n * sizeof(uint64_t));
}
extern "C" int sr_ctx_counters(sr_ctx *c, uint64_t out[16]) { return counters_read(c, out, 16); }
extern "C" int sr_ctx_counters_ext(sr_ctx *c, uint64_t out[32]) { return counters_read(c, out, 32); }
// every slot the device keeps (SR_NCOUNTERS = 54: 48 since round 4, [48..51] the replay's, [52..53] the tile priority's); returns the number of slots written (<= cap) or a negative status
extern "C" int sr_ctx_counters_all(sr_ctx *c, uint64_t *out, uint32_t cap) {
    if (!c || !c->loaded || !out) return sr_fail(SR_ERR_INVALID, "context not loaded");
    const uint32_t n = std::min<uint32_t>(cap, SR_NCOUNTERS);
    const int r = ctx_read(c, out, c->d_counters, n * sizeof(uint64_t));
    return r ? r : (int)n;
}

// secondaries the alignment kernel handed to its tail launch since the counters were last reset (all batches of the pass)
extern "C" int sr_ctx_tail_deferred(sr_ctx *c, uint64_t *out) {
    if (!c || !c->loaded || !out) return sr_fail(SR_ERR_INVALID, "context not loaded");
    *out = 0;
    if (!c->d_tail_deferred) return SR_OK;
    uint32_t v = 0;
    const int r = ctx_read(c, &v, c->d_tail_deferred, sizeof(v));
    *out = v;
    return r;
}
// per-workgroup timeline of the last main launch of the instrumented instance (SR_PROFILE_TICKS=1): 4 words per workgroup
// (SrAlignArgs::timeline); returns the number of workgroups written (<= cap_wg), 0 without the instrumented instance
extern "C" int sr_ctx_tail_timeline(sr_ctx *c, uint64_t *out, uint32_t cap_wg) {
    if (!c || !c->loaded || !out) return sr_fail(SR_ERR_INVALID, "context not loaded");
    if (!c->d_timeline) return 0;
    const uint32_t n = std::min<uint32_t>(cap_wg, (uint32_t)c->nwg);
    const int r = ctx_read(c, out, c->d_timeline, (size_t)n * 4 * sizeof(uint64_t));
    return r ? r : (int)n;
}
// the instrumented instance's second record of the last main launch, 4 words per workgroup (SrAlignArgs::prio_timeline): tick of
// the end of the first alignment, rank on the CU, table index of the CU, arrival count; same return value as sr_ctx_tail_timeline
extern "C" int sr_ctx_prio_timeline(sr_ctx *c, uint64_t *out, uint32_t cap_wg) {
    if (!c || !c->loaded || !out) return sr_fail(SR_ERR_INVALID, "context not loaded");
    if (!c->d_prio_timeline) return 0;
    const uint32_t n = std::min<uint32_t>(cap_wg, (uint32_t)c->nwg);
    const int r = ctx_read(c, out, c->d_prio_timeline, (size_t)n * 4 * sizeof(uint64_t));
    return r ? r : (int)n;
}

extern "C" int sr_ctx_download_uf(sr_ctx *c, uint64_t *parent_out) {
    if (!c || !c->loaded) return sr_fail(SR_ERR_INVALID, "context not loaded");
    return ctx_read(c, parent_out, c->d_nodes, c->uf_size * 8);
}

static int labels_timed(sr_ctx *c, uint64_t *dev_labels64, uint32_t *dev_labels32) {
    hipEvent_t *e0, *e1;
    int r;
    if ((r = ev_get(c, 2, 0, &e0, &e1))) return r;
    HIPCHK(hipEventRecord(*e0, c->stream));
    if (dev_labels64) {
        if (srk_labels(c->d_nodes, c->uf_size, c->d_minarr, (unsigned long long *)dev_labels64, c->d_error, c->stream))
            return sr_fail(SR_ERR_HIP, "label kernel launch failed");
    } else {
        if (srk_labels32(c->d_nodes, c->uf_size, c->d_minarr, dev_labels32, c->d_error, c->stream))
            return sr_fail(SR_ERR_HIP, "label kernel launch failed");
    }
    HIPCHK(hipEventRecord(*e1, c->stream));
    c->ev_used[2] = 1;
    return SR_OK;
}

extern "C" int sr_ctx_labels_device(sr_ctx *c, uint64_t *dev_labels) {
    if (!c || !c->loaded) return sr_fail(SR_ERR_INVALID, "context not loaded");
    HIPCHK(hipSetDevice(c->device));
    return labels_timed(c, dev_labels, nullptr);
}
extern "C" int sr_ctx_labels_device_u32(sr_ctx *c, uint32_t *dev_labels) {
    if (!c || !c->loaded) return sr_fail(SR_ERR_INVALID, "context not loaded");
    if (c->uf_size > 0xffffffffULL) return sr_fail(SR_ERR_UNSUPPORTED, "2N+2 >= 2^32: use the 64-bit label exchange");
    HIPCHK(hipSetDevice(c->device));
    return labels_timed(c, nullptr, dev_labels);
}

extern "C" int sr_ctx_merge_labels(sr_ctx *c, const uint64_t *dev_labels, uint32_t count) {
    if (!c || !c->loaded) return sr_fail(SR_ERR_INVALID, "context not loaded");
    HIPCHK(hipSetDevice(c->device));
    if (srk_merge(c->d_nodes, c->uf_size, (const unsigned long long *)dev_labels, count, c->d_error, c->stream))
        return sr_fail(SR_ERR_HIP, "merge kernel launch failed");
    return SR_OK;
}
extern "C" int sr_ctx_merge_labels_u32(sr_ctx *c, const uint32_t *dev_labels, uint32_t count) {
    if (!c || !c->loaded) return sr_fail(SR_ERR_INVALID, "context not loaded");
    if (c->uf_size > 0xffffffffULL) return sr_fail(SR_ERR_UNSUPPORTED, "2N+2 >= 2^32: use the 64-bit label exchange");
    HIPCHK(hipSetDevice(c->device));
    if (srk_merge32(c->d_nodes, c->uf_size, dev_labels, count, c->d_error, c->stream))
        return sr_fail(SR_ERR_HIP, "merge kernel launch failed");
    return SR_OK;
}

// host-resident label arrays (e.g. read back from files written by other processes / nodes): upload + replay-unite
extern "C" int sr_ctx_merge_labels_host(sr_ctx *c, const uint64_t *labels, uint32_t count) {
    if (!c || !c->loaded || !labels) return sr_fail(SR_ERR_INVALID, "context not loaded");
    HIPCHK(hipSetDevice(c->device));
    for (uint32_t i = 0; i < count; i++) {
        HIPCHK(hipMemcpyAsync(c->d_labels, labels + (uint64_t)i * c->uf_size, c->uf_size * 8, hipMemcpyHostToDevice, c->stream));
        if (srk_merge(c->d_nodes, c->uf_size, c->d_labels, 1, c->d_error, c->stream)) return sr_fail(SR_ERR_HIP, "merge kernel launch failed");
    }
    return SR_OK;
}

extern "C" int sr_ctx_download_labels(sr_ctx *c, uint64_t *labels_out) {
    int r = sr_ctx_labels_device(c, (uint64_t *)c->d_labels);
    if (r) return r;
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(labels_out, c->d_labels, c->uf_size * 8, hipMemcpyDeviceToHost));
    return SR_OK;
}

// ------------------------------------------------------------------ results
extern "C" void sr_alignments_free(sr_alignments *a) {
    if (!a) return;
    free(a->query_idx); free(a->target_idx); free(a->is_reverse); free(a->score);
    free(a->query_start); free(a->query_end); free(a->target_start); free(a->target_end);
    free(a->cigar_off); free(a->cigar_ops);
    free(a);
}

// host copy of the alignments of batch b (its CIGARs must still be in the arena), appended to `ops`
int collect_batch(sr_ctx *c, uint32_t b, AlnAcc &acc) {
    const uint32_t f = c->batch_first[b], l = c->batch_first[b + 1], cntp = l - f;
    if (cntp == 0) return SR_OK;
    std::vector<uint32_t> cnt(cntp);
    HIPCHK(hipMemcpy(cnt.data(), c->aa.cigar_cnt + f, (size_t)cntp * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(acc.score.data() + f, c->aa.score + f, (size_t)cntp * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(acc.isrev.data() + f, c->aa.is_reverse + f, (size_t)cntp, hipMemcpyDeviceToHost));
    const uint64_t arena_used = c->cigar_base[l] - c->cigar_base[f];
    std::vector<uint32_t> raw(arena_used + 1);
    HIPCHK(hipMemcpy(raw.data(), c->aa.cigar_ops, (arena_used + 1) * 4, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < cntp; i++) {
        acc.cnt[f + i] = cnt[i];
        const uint32_t *src = raw.data() + (c->cigar_base[f + i] - c->cigar_base[f]);
        for (uint32_t j = 0; j < cnt[i]; j++) {
            const uint32_t op = src[j] & 15u, len = src[j] >> 4;
            // raw WFA2 alphabet -> reference alphabet (src/wfa.rs:25-31): M->'=', I<->D swapped
            const uint32_t o2 = op == SR_OP_M ? 0u : op == SR_OP_X ? 1u : op == SR_OP_I ? 3u : 2u;
            acc.ops.push_back((len << 4) | o2);
        }
    }
    return SR_OK;
}

sr_alignments *make_alignments_of(const std::vector<uint32_t> &pair_q, const std::vector<uint32_t> &pair_t,
                                  const std::vector<uint32_t> &len, const AlnAcc &acc, size_t count) {
    const size_t np = std::min(count, pair_q.size());
    sr_alignments *a = (sr_alignments *)calloc(1, sizeof(sr_alignments));
    a->n = np;
    const size_t m = np ? np : 1;
    a->query_idx = (uint32_t *)malloc(m * 4); a->target_idx = (uint32_t *)malloc(m * 4);
    a->is_reverse = (uint8_t *)malloc(m); a->score = (int32_t *)malloc(m * 4);
    a->query_start = (uint64_t *)malloc(m * 8); a->query_end = (uint64_t *)malloc(m * 8);
    a->target_start = (uint64_t *)malloc(m * 8); a->target_end = (uint64_t *)malloc(m * 8);
    a->cigar_off = (uint64_t *)malloc((np + 1) * 8);
    a->cigar_ops = (uint32_t *)malloc((acc.ops.size() ? acc.ops.size() : 1) * 4);
    memcpy(a->cigar_ops, acc.ops.data(), acc.ops.size() * 4);
    uint64_t w = 0;
    for (size_t i = 0; i < np; i++) {
        a->query_idx[i] = pair_q[i]; a->target_idx[i] = pair_t[i];
        a->is_reverse[i] = acc.isrev[i]; a->score[i] = acc.score[i];
        a->query_start[i] = 0; a->query_end[i] = len[pair_q[i]];     // allwave aligns full sequences (seqrush.rs:743-753)
        a->target_start[i] = 0; a->target_end[i] = len[pair_t[i]];
        a->cigar_off[i] = w;
        w += acc.cnt[i];
    }
    a->cigar_off[np] = w;
    return a;
}

extern "C" int sr_ctx_alignments(sr_ctx *c, sr_alignments **out) {
    if (!c || !c->loaded) return sr_fail(SR_ERR_INVALID, "context not loaded");
    if (c->from_paf) return sr_fail(SR_ERR_INVALID, "context was loaded from a PAF file: it holds no device alignments");
    if (c->batch_first.size() > 2 || !c->aligned_batch_valid)
        return sr_fail(SR_ERR_UNSUPPORTED, "the CIGARs of this context are not resident (several batches, or no alignment pass yet): use sr_align_all");
    int r = sr_ctx_sync(c);
    if (r) return r;
    const size_t np = c->pair_q.size();
    AlnAcc acc;
    acc.cnt.assign(np + 1, 0); acc.score.assign(np + 1, 0); acc.isrev.assign(np + 1, 0);
    if ((r = collect_batch(c, 0, acc))) return r;
    *out = make_alignments_of(c->pair_q, c->pair_t, c->len, acc);
    return SR_OK;
}

// per-pair results that stay resident for every batch: score, strand flag, CIGAR op count (arrays of num_pairs)
extern "C" int sr_ctx_pair_results(sr_ctx *c, int32_t *score, uint8_t *is_reverse, uint32_t *cigar_ops) {
    if (!c || !c->loaded || c->from_paf) return sr_fail(SR_ERR_INVALID, "context holds no device alignments");
    int r = sr_ctx_sync(c);
    if (r) return r;
    const size_t np = c->pair_q.size();
    if (!np) return SR_OK;
    if (score) HIPCHK(hipMemcpy(score, c->aa.score, np * 4, hipMemcpyDeviceToHost));
    if (is_reverse) HIPCHK(hipMemcpy(is_reverse, c->aa.is_reverse, np, hipMemcpyDeviceToHost));
    if (cigar_ops) HIPCHK(hipMemcpy(cigar_ops, c->aa.cigar_cnt, np * 4, hipMemcpyDeviceToHost));
    return SR_OK;
}

extern "C" size_t sr_alignment_cigar(const sr_alignments *a, uint64_t i, char *buf, size_t cap) {
    static const char opc[4] = {'=', 'X', 'I', 'D'};
    size_t need = 0;
    if (!a || i >= a->n) return 0;
    for (uint64_t j = a->cigar_off[i]; j < a->cigar_off[i + 1]; j++) {
        char tmp[24];
        int l = snprintf(tmp, sizeof(tmp), "%u%c", a->cigar_ops[j] >> 4, opc[a->cigar_ops[j] & 3u]);
        if (buf && need + (size_t)l < cap) memcpy(buf + need, tmp, (size_t)l);
        need += (size_t)l;
    }
    if (buf && cap) buf[std::min(need, cap - 1)] = 0;
    return need;
}

// one batch at a time: align, copy its CIGARs to the host, (optionally) unite, next batch
static int align_all_impl(sr_ctx *c, bool unite, sr_alignments **out) {
    int r = begin_pass(c, true);
    if (r) return r;
    c->ev_used[1] = 0;
    const size_t np = c->pair_q.size();
    AlnAcc acc;
    acc.cnt.assign(np + 1, 0); acc.score.assign(np + 1, 0); acc.isrev.assign(np + 1, 0);
    const uint32_t nbatch = (uint32_t)c->batch_first.size() - 1;
    const bool inv = unite && c->inv_on;
    if (inv && (r = inv_begin_run(c))) return r;
    for (uint32_t b = 0; b < nbatch; b++) {
        if ((r = enqueue_align_batch(c, b))) return r;
        if (unite && (r = enqueue_unite_batch(c, b))) return r;
        if (inv && (r = inv_scan_batch(c, b))) return r;
        if ((r = sr_ctx_sync(c))) return r;
        if ((r = collect_batch(c, b, acc))) return r;
    }
    c->aligned_batch_valid = nbatch == 1;
    if (inv && (r = inv_patch_pass(c))) return r;
    *out = make_alignments_of(c->pair_q, c->pair_t, c->len, acc);
    return SR_OK;
}

extern "C" int sr_ctx_align_all(sr_ctx *c, int unite, sr_alignments **out) {
    if (!c || !c->loaded || !out) return sr_fail(SR_ERR_INVALID, "context not loaded");
    if (c->from_paf) return sr_fail(SR_ERR_INVALID, "context was loaded from a PAF file: there is no alignment stage");
    return align_all_impl(c, unite != 0, out);
}

extern "C" int sr_align_all(const sr_seqset *seqs, const sr_params *p, sr_alignments **out) {
    if (!seqs || !p || !out) return sr_fail(SR_ERR_INVALID, "null argument");
    return sr_with_ctx(p->device, [&](sr_ctx *c) { const int r = sr_ctx_load(c, seqs, p); return r ? r : align_all_impl(c, false, out); });
}

// run the loaded list, then the forest as the parameters ask for it: canonical labels or the raw node array
int run_to_parent(sr_ctx *c, const sr_params *p, uint64_t *parent_out) {
    int r;
    if ((r = sr_ctx_run(c)) || (r = sr_ctx_sync(c))) return r;
    r = p->canonical_labels ? sr_ctx_download_labels(c, parent_out) : sr_ctx_download_uf(c, parent_out);
    return r ? r : sr_ctx_sync(c);
}
extern "C" int sr_align_and_unite(const sr_seqset *seqs, const sr_params *p, uint64_t *parent_out) {
    if (!seqs || !p || !parent_out) return sr_fail(SR_ERR_INVALID, "null argument");
    return sr_with_ctx(p->device, [&](sr_ctx *c) { const int r = sr_ctx_load(c, seqs, p); return r ? r : run_to_parent(c, p, parent_out); });
}

// ------------------------------------------------------------------ iterative mode (--iterative)
// align_and_unite_iterative (src/seqrush.rs:867-1132) on one context.  Pair list: the expanded tree entries, then the
// expanded random entries (sr_pairs.cpp "pair list"), loaded through load_impl without sharding.  Phase 1 runs the tree
// batches like sr_ctx_run (fused unite).  Phase 2 runs window after window: the alignment kernel without the fused unite, then
// per chunk of CHECK_INTERVAL random entries the guarded unite, the root count and the decision (sr_iter.hip), all on the
// stream; the host reads the decision state and the window's counts after the window and starts the next one only if the
// run has not stopped.  The union-find then holds exactly the processed alignments, whatever the schedule.
extern "C" int sr_ctx_load_iterative(sr_ctx *c, const sr_seqset *seqs, const sr_params *p, int keep_alignments) {
    if (!c || !seqs || !p) return sr_fail(SR_ERR_INVALID, "null argument");
    if (p->shard_count != 1 || p->shard_rank != 0)
        return sr_fail(SR_ERR_UNSUPPORTED, "--iterative runs one global sequential stop rule: it cannot be sharded over ranks");
    sr_params q = *p;
    const bool defaulted = q.sparsify_kind != SR_SPARSE_TREE;
    if (defaulted) {                                   // :957-967: any other strategy -> tree:3,3,0.1,16
        q.sparsify_kind = SR_SPARSE_TREE; q.tree_k_nearest = 3; q.tree_k_farthest = 3; q.tree_rand_frac = 0.1; q.tree_kmer = 16;
    }
    int r = unload_if_failed(c, load_impl(c, seqs, &q, nullptr, nullptr, 0, true, true));
    if (r) return r;
    void *d;
    if ((r = dev_alloc(c, &d, sizeof(SrIterState)))) return r;
    c->d_iter_state = (SrIterState *)d;
    if ((r = dev_alloc(c, &d, ((size_t)c->iter_max_chunks + 1) * 8))) return r;
    c->d_iter_counts = (unsigned long long *)d;
    sr_iter_stats &st = c->iter_stats;
    st.tree_defaulted = defaulted ? 1 : 0;
    st.tree_k_nearest = q.tree_k_nearest; st.tree_k_farthest = q.tree_k_farthest; st.tree_rand_frac = q.tree_rand_frac; st.tree_kmer = q.tree_kmer;
    c->iter_keep = keep_alignments != 0;
    c->iter_loaded = true;
    return SR_OK;
}

// components of the context's forest: roots among nodes [0, 2T) into d_iter_counts[slot] (host sync; error flags checked)
static int iter_count_now(sr_ctx *c, uint32_t slot, uint64_t *out) {
    HIPCHK(hipMemsetAsync(c->d_iter_counts + slot, 0, 8, c->stream));
    if (srk_count_roots(c->d_nodes, c->total_len, c->d_iter_counts + slot, nullptr, c->stream)) return sr_fail(SR_ERR_HIP, "count kernel launch failed");
    int r = sr_ctx_sync(c);
    if (r) return r;
    HIPCHK(hipMemcpy(out, c->d_iter_counts + slot, 8, hipMemcpyDeviceToHost));
    return SR_OK;
}

extern "C" int sr_ctx_run_iterative(sr_ctx *c) {
    if (!c || !c->loaded || !c->iter_loaded) return sr_fail(SR_ERR_INVALID, "context not loaded with sr_ctx_load_iterative");
    int r = begin_pass(c, true);
    if (r) return r;
    c->ev_used[1] = 0;
    if (c->iter_ran && (r = sr_ctx_reset_uf(c))) return r;     // a second run starts from SeqRush::new again
    if (c->iter_al) { sr_alignments_free(c->iter_al); c->iter_al = nullptr; }
    sr_iter_stats &st = c->iter_stats;
    st.random_processed = st.random_aligned = st.checks = st.windows = 0; st.stabilized = 0;
    c->iter_counts.clear();
    const size_t np = c->pair_q.size();
    const uint32_t nbatch = (uint32_t)c->batch_first.size() - 1;
    AlnAcc acc;
    if (c->iter_keep) { acc.cnt.assign(np + 1, 0); acc.score.assign(np + 1, 0); acc.isrev.assign(np + 1, 0); }
    // phase 1: every tree entry
    for (uint32_t b = 0; b < c->iter_tree_batches; b++) {
        if ((r = enqueue_align_batch(c, b, c->fuse_unite)) || (r = enqueue_unite_batch(c, b, c->fuse_unite))) return r;
        if (c->iter_keep && ((r = sr_ctx_sync(c)) || (r = collect_batch(c, b, acc)))) return r;
    }
    const uint32_t spare = c->iter_max_chunks;
    uint64_t post_tree = 0;
    if ((r = iter_count_now(c, spare, &post_tree))) return r;
    st.post_tree = post_tree;
    SrIterState hs{};
    hs.prev = post_tree;
    HIPCHK(hipMemcpy(c->d_iter_state, &hs, sizeof(hs), hipMemcpyHostToDevice));
    // phase 2: windows of whole chunks
    const uint32_t CH = 4 * SR_ITER_CHECK_INTERVAL;
    const uint64_t tp = c->iter_tree_pairs;
    std::vector<unsigned long long> cnt(c->iter_max_chunks + 1);
    for (uint32_t b = c->iter_tree_batches; b < nbatch; b++) {
        SrUniteArgs u;
        batch_args(c, b, nullptr, &u);
        const uint32_t f = c->batch_first[b], npb = u.npairs;
        if (npb == 0) continue;
        const uint32_t nchunks = (npb + CH - 1) / CH, check0 = (uint32_t)((f - tp) / CH);
        HIPCHK(hipMemsetAsync(c->d_iter_counts, 0, (size_t)nchunks * 8, c->stream));
        if ((r = enqueue_align_batch(c, b, false))) return r;
        for (uint32_t k = 0; k < nchunks; k++) {
            SrUniteArgs uc = u;
            const uint32_t o = k * CH, m = std::min(CH, npb - o);
            uc.pair_q += o; uc.pair_t += o; uc.npairs = m; uc.is_reverse += o; uc.score += o; uc.max_score += o;
            uc.cigar_cnt += o; uc.cigar_base += o;
            if (srk_iter_unite(&uc, (int)m, c->d_iter_state, c->stream)) return sr_fail(SR_ERR_HIP, "iterative unite kernel launch failed");
            if (m < CH) break;                             // trailing partial chunk: no check (:1088)
            if (srk_count_roots(c->d_nodes, c->total_len, c->d_iter_counts + k, c->d_iter_state, c->stream) ||
                srk_iter_decide(c->d_iter_state, c->d_iter_counts, k, check0 + k, c->stream))
                return sr_fail(SR_ERR_HIP, "iterative count / decide kernel launch failed");
        }
        st.windows++;
        st.random_aligned += npb / 4;
        if ((r = sr_ctx_sync(c))) return r;
        HIPCHK(hipMemcpy(&hs, c->d_iter_state, sizeof(hs), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(cnt.data(), c->d_iter_counts, (size_t)nchunks * 8, hipMemcpyDeviceToHost));
        const uint32_t full = npb / CH;
        const uint32_t done = hs.stopped ? hs.stop_check + 1 - check0 : full;     // checks of this window that ran
        for (uint32_t k = 0; k < done; k++) c->iter_counts.push_back(cnt[k]);
        if (c->iter_keep && (r = collect_batch(c, b, acc))) return r;
        if (hs.stopped) break;
    }
    st.checks = c->iter_counts.size();
    st.stabilized = hs.stopped ? 1 : 0;
    st.random_processed = hs.stopped ? (uint64_t)(hs.stop_check + 1) * SR_ITER_CHECK_INTERVAL : st.random_entries;
    uint64_t fin = 0;
    if ((r = iter_count_now(c, spare, &fin))) return r;
    st.final_components = fin;
    if (c->iter_keep) c->iter_al = make_alignments_of(c->pair_q, c->pair_t, c->len, acc, (size_t)(tp + 4 * st.random_processed));
    c->iter_ran = true;
    c->aligned_batch_valid = false;
    return SR_OK;
}

extern "C" int sr_ctx_iterative_stats(sr_ctx *c, sr_iter_stats *out, uint64_t *check_counts, uint64_t cap) {
    if (!c || !c->iter_loaded || !out) return sr_fail(SR_ERR_INVALID, "context not loaded with sr_ctx_load_iterative");
    *out = c->iter_stats;
    if (check_counts)
        for (uint64_t i = 0; i < std::min<uint64_t>(cap, c->iter_counts.size()); i++) check_counts[i] = c->iter_counts[i];
    return SR_OK;
}

extern "C" int sr_ctx_iterative_alignments(sr_ctx *c, sr_alignments **out) {
    if (!c || !out) return sr_fail(SR_ERR_INVALID, "null argument");
    if (!c->iter_al) return sr_fail(SR_ERR_INVALID, "no processed alignments: load with keep_alignments = 1, run, and take them once");
    *out = c->iter_al;
    c->iter_al = nullptr;
    return SR_OK;
}
