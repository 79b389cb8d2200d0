// sr_inv_host.cpp -- inversion patching (--patch-inversions, --inversion-join) on the host side: the rule's host twins, the
// scan of a batch's CIGARs and the patch pass that sr_ctx_run and sr_ctx_align_all call, its accessors, and the entry points
// that run the scan kernels over alignments given on the host (tests).  The rule itself is sr_inv_rule.h, the kernels sr_inv.hip.
#include "sr_ctx.h"

// Rule and coordinates: sr_inv_rule.h.  Chain: after every batch's alignment kernel (and its unite, fused or not) the scan
// (sr_inv.hip) counts the candidates of each CIGAR in the arena, turns the counts into offsets and emits the job records;
// the host reads the total and the records (20 bytes each) before the arena is reused.  After the last batch the patch pass
// copies the raw sequence bytes back from the device (total_len bytes, once per run: the context keeps no host copy), cuts
// the jobs' segments out of them -- the query's already reverse-complemented where the patch is on '-' -- and loads them as a
// set of their own through the same pack-and-upload path (an inner context on the same device and stream, load flag
// forced_strand: pair j = (segment 2j, segment 2j + 1), aligned as loaded, no orientation search on either kernel family),
// runs the alignment kernel over it in batches under the usual arena rule and, per batch, sr_unite_kernel over the
// patch CIGARs with the ORIGINAL sequence indices, the patches' starts and the folded score bound, into this context's forest.
extern "C" int sr_inversion_candidate(uint64_t qgap, uint64_t tgap, uint64_t min_size) {
    if (min_size == 0) return sr_fail(SR_ERR_INVALID, "inversion threshold 0: every complementary SNP would be an inversion (give -k or a minimum size)");
    return sr_inv_is_candidate(qgap, tgap, min_size);
}
extern "C" int sr_inversion_accept(int32_t patch_score, int32_t main_score) { return sr_inv_accept_score(patch_score, main_score); }

// cigar_analysis.rs:23-128 over run-length ops in the sr_alignments encoding (2 'I' = query only, 3 'D' = target only)
extern "C" int sr_inversion_sites_host(const uint32_t *ops, uint64_t n_ops, uint64_t min_size, sr_inv_site **sites, uint64_t *count) {
    if ((!ops && n_ops) || !sites || !count) return sr_fail(SR_ERR_INVALID, "null argument");
    if (min_size == 0) return sr_fail(SR_ERR_INVALID, "inversion threshold 0: every complementary SNP would be an inversion (give -k or a minimum size)");
    std::vector<sr_inv_site> out;
    uint64_t q = 0, t = 0;
    for (uint64_t i = 0; i < n_ops; i++) {
        const uint32_t op = ops[i] & 3u; const uint64_t len = ops[i] >> 4;
        if (op == 0) {
            uint64_t qg = 0, tg = 0;
            for (uint64_t j = i + 1; j < n_ops && (ops[j] & 3u) != 0; j++) {
                const uint32_t o2 = ops[j] & 3u; const uint64_t l2 = ops[j] >> 4;
                if (o2 == 1) { qg += l2; tg += l2; } else if (o2 == 2) qg += l2; else tg += l2;
            }
            const int kind = sr_inv_site_kind(qg, tg, min_size);
            if (kind != SR_INV_NONE) {
                sr_inv_site s;
                s.query_start = q + len; s.target_start = t + len;
                s.query_end = s.query_start + (kind == SR_INV_TARGET_ONLY ? 0 : qg);
                s.target_end = s.target_start + (kind == SR_INV_QUERY_ONLY ? 0 : tg);
                s.kind = kind; s.candidate = sr_inv_is_candidate(qg, tg, min_size);
                out.push_back(s);
            }
            q += len; t += len;
        } else if (op == 1) { q += len; t += len; }
        else if (op == 2) q += len;
        else t += len;
    }
    *count = out.size();
    return to_malloc(out, sites);
}

static int inv_pen_of(const sr_params *p, SrInvPen *out) {
    if (!p) return sr_fail(SR_ERR_INVALID, "null argument");
    SrPen pen;
    const int r = make_pen(*p, false, &pen);
    if (r) return r;
    *out = SrInvPen{pen.x, pen.o1, pen.e1, pen.o2, pen.e2, pen.two};
    return SR_OK;
}

extern "C" int sr_inversion_accept_site(int32_t patch_score, int32_t site_cost) { return sr_inv_accept_site(patch_score, site_cost); }

// the joined rule (sr_inv_rule.h) over run-length ops in the sr_alignments encoding; cost[i] = site cost of sites[i]
extern "C" int sr_inversion_sites_host_join(const uint32_t *ops, uint64_t n_ops, uint64_t min_size, uint32_t join_below, const sr_params *pen,
                                            sr_inv_site **sites, int32_t **cost, uint64_t *count) {
    if ((!ops && n_ops) || !sites || !cost || !count) return sr_fail(SR_ERR_INVALID, "null argument");
    if (min_size == 0) return sr_fail(SR_ERR_INVALID, "inversion threshold 0: every complementary SNP would be an inversion (give -k or a minimum size)");
    if (join_below == 0) return sr_fail(SR_ERR_INVALID, "inversion join length 0: the joined rule needs J >= 1");
    if (join_below > min_size) return sr_fail(SR_ERR_INVALID, "inversion join length above the gap threshold: an island would be a candidate by itself");
    SrInvPen ip;
    int r;
    if ((r = inv_pen_of(pen, &ip))) return r;
    std::vector<sr_inv_site> out;
    std::vector<int32_t> oc;
    uint64_t q = 0, t = 0, qa = 0, ta = 0, qg = 0, tg = 0, sc = 0;
    bool open = false;
    auto close = [&]() {
        const int kind = sr_inv_site_kind(qg, tg, min_size);
        if (kind == SR_INV_NONE) return;
        sr_inv_site s;
        s.query_start = qa; s.target_start = ta;
        s.query_end = qa + (kind == SR_INV_TARGET_ONLY ? 0 : qg);
        s.target_end = ta + (kind == SR_INV_QUERY_ONLY ? 0 : tg);
        s.kind = kind; s.candidate = sr_inv_is_candidate(qg, tg, min_size);
        out.push_back(s); oc.push_back((int32_t)(uint32_t)sc);
    };
    for (uint64_t i = 0; i < n_ops; i++) {
        const uint32_t op = ops[i] & 3u, len = ops[i] >> 4;
        if (sr_inv_is_anchor(op, len, join_below)) {
            if (open) close();
            q += len; t += len;
            open = true; qa = q; ta = t; qg = tg = sc = 0;
            continue;
        }
        if (op == 0 || op == 1) { q += len; t += len; qg += len; tg += len; }
        else if (op == 2) { q += len; qg += len; }
        else { t += len; tg += len; }
        sc += sr_inv_op_cost(op, len, ip);
    }
    if (open) close();
    *count = out.size();
    return (r = to_malloc(out, sites)) ? r : to_malloc(oc, cost);
}

extern "C" int sr_ctx_enable_inversions(sr_ctx *c, const sr_inv_params *p) {
    if (!c || !c->loaded) return sr_fail(SR_ERR_INVALID, "context not loaded");
    if (!p) { c->inv_on = false; return SR_OK; }
    if (c->from_paf) return sr_fail(SR_ERR_UNSUPPORTED, "inversion patching needs the alignment stage: it cannot be combined with PAF input");
    if (c->iter_loaded) return sr_fail(SR_ERR_UNSUPPORTED, "inversion patching cannot be combined with the iterative mode");
    const uint64_t m = p->min_size ? p->min_size : 2 * c->prm.min_match_len;
    if (m == 0) return sr_fail(SR_ERR_INVALID, "inversion threshold 0: every complementary SNP would be an inversion (give -k or a minimum size)");
    if (p->join_below > m) return sr_fail(SR_ERR_INVALID, "inversion join length above the gap threshold: an island would be a candidate by itself");
    HIPCHK(hipSetDevice(c->device));
    if (!c->d_inv_count) {
        uint32_t maxb = 1;
        for (size_t b = 0; b + 1 < c->batch_first.size(); b++) maxb = std::max(maxb, c->batch_first[b + 1] - c->batch_first[b]);
        int r;
        void *d;
        if ((r = dev_alloc(c, &d, (size_t)maxb * 4))) return r; c->d_inv_count = (uint32_t *)d;
        if ((r = dev_alloc(c, &d, ((size_t)maxb + 1) * 4))) return r; c->d_inv_off = (uint32_t *)d;
        if ((r = dev_alloc(c, &d, 4 * sizeof(unsigned long long)))) return r; c->d_inv_stats = (unsigned long long *)d;
    }
    c->inv_m = m; c->inv_keep = p->keep_alignments != 0; c->inv_on = true; c->inv_join = p->join_below;
    return SR_OK;
}

int inv_begin_run(sr_ctx *c) {
    c->inv_raw.clear(); c->inv_jobs.clear(); c->inv_stats = sr_inv_stats{}; c->inv_ev_used = 0;
    c->inv_raw_j.clear();
    for (uint64_t &v : c->inv_join_stats) v = 0;
    if (c->inv_al) { sr_alignments_free(c->inv_al); c->inv_al = nullptr; }
    HIPCHK(hipMemsetAsync(c->d_inv_stats, 0, 4 * sizeof(unsigned long long), c->stream));
    return SR_OK;
}

// count, offsets, (host reads the total,) emit, (host reads the records) for one batch whose CIGARs are in the arena
// ev: two event pairs (or NULL): [0] around count + offsets, [1] around emit -- kernels only, not the host round trips
// J: SrInvJob (plain instances) or SrInvJobJ (joined instances, s.join_below >= 1)
static void inv_set_jobs(SrInvScanArgs &s, SrInvJob *j) { s.jobs = j; }
static void inv_set_jobs(SrInvScanArgs &s, SrInvJobJ *j) { s.jobs_j = j; }
template <class J>
static int inv_scan_launch(hipStream_t stream, SrInvScanArgs &s, uint32_t *d_off, std::vector<void *> *allocs, J **d_jobs,
                           uint64_t *job_cap, std::vector<J> &out, std::pair<hipEvent_t, hipEvent_t> *ev = nullptr,
                           int *ev_used = nullptr) {
    if (s.npairs == 0) return SR_OK;
    if (ev) HIPCHK(hipEventRecord(ev[0].first, stream));
    if (srk_inv_scan(&s, 0, stream) || srk_inv_offsets(s.count, s.npairs, d_off, stream)) return sr_fail(SR_ERR_HIP, "inversion scan kernel launch failed");
    if (ev) { HIPCHK(hipEventRecord(ev[0].second, stream)); *ev_used = 1; }
    uint32_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, d_off + s.npairs, 4, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    if (total == 0) return SR_OK;
    if (total > *job_cap) {
        const uint64_t cap = std::max<uint64_t>(total, 2 * *job_cap);
        void *d = nullptr;
        if (hipMalloc(&d, cap * sizeof(J)) != hipSuccess) return sr_fail(SR_ERR_NOMEM, "not enough device memory for the inversion job list");
        if (*d_jobs) {                                     // (the stream is idle: the smaller buffer's records were copied out)
            auto it = std::find(allocs->begin(), allocs->end(), (void *)*d_jobs);
            if (it != allocs->end()) allocs->erase(it);
            (void)hipFree(*d_jobs);
        }
        allocs->push_back(d);
        *d_jobs = (J *)d; *job_cap = cap;
    }
    s.offset = d_off; inv_set_jobs(s, *d_jobs); s.job_cap = *job_cap;
    if (ev) HIPCHK(hipEventRecord(ev[1].first, stream));
    if (srk_inv_scan(&s, 1, stream)) return sr_fail(SR_ERR_HIP, "inversion scan kernel launch failed");
    if (ev) { HIPCHK(hipEventRecord(ev[1].second, stream)); *ev_used = 2; }
    const size_t at = out.size();
    out.resize(at + total);
    HIPCHK(hipMemcpyAsync(out.data() + at, *d_jobs, (size_t)total * sizeof(J), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    return SR_OK;
}

int inv_scan_batch(sr_ctx *c, uint32_t b) {
    SrUniteArgs u;
    batch_args(c, b, nullptr, &u);
    while ((int)c->inv_ev.size() < c->inv_ev_used + 2) {
        hipEvent_t x = nullptr, y = nullptr;
        HIPCHK(hipEventCreate(&x)); HIPCHK(hipEventCreate(&y));
        c->inv_ev.push_back({x, y});
    }
    SrInvScanArgs s{};
    s.cigar_ops = u.cigar_ops; s.cigar_base = u.cigar_base; s.cigar_cnt = u.cigar_cnt; s.score = u.score; s.max_score = u.max_score;
    s.npairs = u.npairs; s.pair0 = c->batch_first[b]; s.min_size = c->inv_m; s.count = c->d_inv_count; s.stats = c->d_inv_stats;
    int used = 0, r;
    if (c->inv_join) {
        s.join_below = c->inv_join;
        const SrPen &pn = c->aa.pen;
        const int32_t pv[6] = {pn.x, pn.o1, pn.e1, pn.o2, pn.e2, pn.two};
        memcpy(s.pen, pv, sizeof(pv));
        r = inv_scan_launch(c->stream, s, c->d_inv_off, &c->dev_allocs, &c->d_inv_jobs_j, &c->inv_job_cap_j, c->inv_raw_j,
                            c->inv_ev.data() + c->inv_ev_used, &used);
    } else
        r = inv_scan_launch(c->stream, s, c->d_inv_off, &c->dev_allocs, &c->d_inv_jobs, &c->inv_job_cap, c->inv_raw,
                            c->inv_ev.data() + c->inv_ev_used, &used);
    if (r) return r;
    c->inv_ev_used += used;
    return SR_OK;
}

static inline int32_t inv_job_cost(const SrInvJob &) { return 0; }            // the plain record carries no cost
static inline int32_t inv_job_cost(const SrInvJobJ &w) { return w.cost; }

// J: the record type of the run's scan instances; raw: the run's records
template <class J>
static int inv_patch_pass_of(sr_ctx *c, const std::vector<J> &raw) {
    int r;
    if ((r = sr_ctx_sync(c))) return r;
    sr_inv_stats &st = c->inv_stats;
    unsigned long long ds[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpy(ds, c->d_inv_stats, sizeof(ds), hipMemcpyDeviceToHost));
    st.scanned = ds[0]; st.sites = ds[1]; st.candidates = ds[2];
    for (int i = 0; i < c->inv_ev_used; i++) {
        float t = 0;
        HIPCHK(hipEventSynchronize(c->inv_ev[i].second));
        HIPCHK(hipEventElapsedTime(&t, c->inv_ev[i].first, c->inv_ev[i].second));
        st.scan_ms += t;
    }
    const bool join = c->inv_join != 0;
    if (join) c->inv_join_stats[0] = ds[3];
    const size_t nj = raw.size();
    if ((uint64_t)nj != st.candidates) return sr_fail(SR_ERR_DEVICE_FAULT, "inversion scan: the emitted job records do not match the counted candidates");
    if (nj == 0) return SR_OK;                             // nothing to patch: no launch, the forest is the plain run's
    if (nj > 0x7ffffff0ULL) return sr_fail(SR_ERR_UNSUPPORTED, "more than 2^31 inversion candidates");
    const size_t np = c->pair_q.size();
    std::vector<int32_t> score(np);
    std::vector<uint8_t> isrev(np), bases(c->total_len);
    HIPCHK(hipMemcpy(score.data(), c->aa.score, np * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(isrev.data(), c->aa.is_reverse, np, hipMemcpyDeviceToHost));
    // host clock (sr_ctx_inversion_join_stats[2]): from here -- the download of the bases, the segment set, the inner load's
    // index, packing, uploads, planning and allocation -- to just before the inner load's first kernel (its union-find init)
    const auto host_t0 = std::chrono::steady_clock::now();
    HIPCHK(hipMemcpy(bases.data(), c->d_bases, c->total_len, hipMemcpyDeviceToHost));
    // segment set: 2 j = the pattern (the query's forward segment, reverse-complemented for a '-' patch -- the same bytes as
    // the reverse complement of the ALIGNED query's gap), 2 j + 1 = the target's segment; patch strand = negated main strand
    std::vector<uint8_t> seg;
    std::vector<uint64_t> soff(1, 0);
    std::vector<uint32_t> eq(nj), et(nj), opq(nj), opt(nj), qs(nj), ts(nj);
    std::vector<uint8_t> strand(nj);
    std::vector<int32_t> bound(nj);
    c->inv_jobs.assign(nj, sr_inv_job{});
    {
        uint64_t seg_bytes = 0;
        for (const J &w : raw) seg_bytes += (uint64_t)w.qgap + w.tgap;
        seg.reserve(seg_bytes);
        soff.reserve(2 * nj + 1);
    }
    for (size_t j = 0; j < nj; j++) {
        const J &w = raw[j];
        const int32_t cost = inv_job_cost(w);
        if (w.pair >= np) return sr_fail(SR_ERR_DEVICE_FAULT, "inversion scan: job record with a pair index out of range");
        const uint32_t q = c->pair_q[w.pair], t = c->pair_t[w.pair];
        const uint64_t lq = c->len[q], lt = c->len[t];
        if ((uint64_t)w.qa + w.qgap > lq || (uint64_t)w.ta + w.tgap > lt || w.qgap == 0 || w.tgap == 0)
            return sr_fail(SR_ERR_DEVICE_FAULT, "inversion scan: job record outside its sequences");
        const bool main_rev = isrev[w.pair] != 0;
        const uint64_t fq = main_rev ? lq - w.qa - w.qgap : w.qa;
        if (main_rev) seg.insert(seg.end(), bases.begin() + (c->goff[q] + fq), bases.begin() + (c->goff[q] + fq + w.qgap));
        else {                                             // reverse complement, written in place
            const size_t at = seg.size();
            seg.resize(at + w.qgap);
            const uint8_t *src = bases.data() + c->goff[q] + fq + w.qgap - 1;
            uint8_t *dst = seg.data() + at;
            for (uint32_t k = 0; k < w.qgap; k++) dst[k] = comp_base(src[-(ptrdiff_t)k]);
        }
        soff.push_back(seg.size());
        seg.insert(seg.end(), bases.begin() + (c->goff[t] + w.ta), bases.begin() + (c->goff[t] + w.ta + w.tgap));
        soff.push_back(seg.size());
        eq[j] = (uint32_t)(2 * j); et[j] = (uint32_t)(2 * j + 1); opq[j] = q; opt[j] = t;
        strand[j] = main_rev ? 0 : 1;
        qs[j] = (uint32_t)(lq - w.qa - w.qgap);            // first query position in the patch's own space (sr_inv_rule.h)
        ts[j] = w.ta;
        if (join && (cost < 0 || cost > score[w.pair]))
            return sr_fail(SR_ERR_DEVICE_FAULT, "inversion scan: a site cost outside [0, main score]");
        int32_t bd = join ? sr_inv_site_bound(cost) : sr_inv_score_bound(score[w.pair]);
        if (c->prm.max_divergence >= 0.0)
            bd = std::min(bd, max_score_for_divergence(c->prm, std::min<uint64_t>(w.qgap, w.tgap), c->prm.max_divergence));
        bound[j] = bd;
        sr_inv_job &o = c->inv_jobs[j];
        o.pair = w.pair; o.query_idx = q; o.target_idx = t; o.query_start = fq; o.query_end = fq + w.qgap;
        o.target_start = w.ta; o.target_end = (uint64_t)w.ta + w.tgap; o.main_score = score[w.pair]; o.patch_score = -1;
        o.is_reverse = strand[j]; o.accepted = 0; o.site_cost = join ? cost : 0;
    }
    sr_seqset ss{(uint32_t)(2 * nj), seg.data(), soff.data(), nullptr};
    sr_params pp = c->prm;
    pp.sparsify_kind = SR_SPARSE_NONE; pp.shard_rank = 0; pp.shard_count = 1; pp.max_divergence = -1.0;
    sr_ctx *in = new sr_ctx();
    in->device = c->device; in->stream = c->stream; in->own_stream = false;
    struct Guard { sr_ctx *p; ~Guard() { SrKeepError keep; sr_ctx_destroy(p); } } guard{in};
    if ((r = load_impl(in, &ss, &pp, eq.data(), et.data(), nj, true, false, true))) return r;      // forced_strand
    c->inv_join_stats[2] = (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(in->t_first_kernel - host_t0).count();
    uint32_t *d_opq, *d_opt, *d_qs, *d_ts; int32_t *d_bound; uint8_t *d_strand;
    if ((r = dev_upload(in, opq, &d_opq)) || (r = dev_upload(in, opt, &d_opt)) || (r = dev_upload(in, qs, &d_qs)) ||     // (in->stream is c->stream)
        (r = dev_upload(in, ts, &d_ts)) || (r = dev_upload(in, bound, &d_bound)) || (r = dev_upload(in, strand, &d_strand))) return r;
    HIPCHK(hipStreamSynchronize(c->stream));
    AlnAcc acc;
    if (c->inv_keep) { acc.cnt.assign(nj + 1, 0); acc.score.assign(nj + 1, 0); acc.isrev.assign(nj + 1, 0); }
    const uint32_t nbatch = (uint32_t)in->batch_first.size() - 1;
    in->ev_used[0] = in->ev_used[4] = 0;
    for (uint32_t b = 0; b < nbatch; b++) {
        if ((r = enqueue_align_batch(in, b, false))) return r;
        SrUniteArgs u;
        batch_args(in, b, nullptr, &u);
        const uint32_t f = in->batch_first[b];
        u.pair_q = d_opq + f; u.pair_t = d_opt + f; u.seqlen = c->ua.seqlen; u.seq_goff = c->ua.seq_goff;
        u.q_start = d_qs + f; u.t_start = d_ts + f; u.max_score = d_bound + f; u.is_reverse = d_strand + f;
        u.nodes = c->d_nodes; u.uf_size = c->uf_size; u.counters = in->d_counters; u.error_flag = c->d_error;
        if (u.npairs > 0 && srk_unite(&u, (int)std::min<uint64_t>(u.npairs, 4096), c->stream))
            return sr_fail(SR_ERR_HIP, "unite kernel launch failed");
        if (c->inv_keep && ((r = sr_ctx_sync(in)) || (r = collect_batch(in, b, acc)))) return r;
    }
    if ((r = sr_ctx_sync(in)) || (r = sr_ctx_sync(c))) return r;
    std::vector<int32_t> ps(nj);
    HIPCHK(hipMemcpy(ps.data(), in->aa.score, nj * 4, hipMemcpyDeviceToHost));
    unsigned long long cnt[8];
    HIPCHK(hipMemcpy(cnt, in->d_counters, sizeof(cnt), hipMemcpyDeviceToHost));
    st.united_bases = cnt[4]; st.patch_batches = nbatch;
    { float ms = 0; if (sr_ctx_kernel_ms(in, 0, &ms) == SR_OK) st.patch_align_ms = ms; }
    for (size_t j = 0; j < nj; j++) {
        sr_inv_job &o = c->inv_jobs[j];
        o.patch_score = ps[j];
        if (join ? !sr_inv_accept_site(ps[j], o.site_cost) : !sr_inv_accept_score(ps[j], o.main_score)) {
            st.rejected_score++;
            if (join) c->inv_join_stats[1]++;
        }
        else if (ps[j] > bound[j]) st.rejected_divergence++;
        else { o.accepted = 1; st.accepted++; }
    }
    if (c->inv_keep) {                                     // the accepted patches as sr_alignments, PAF coordinates
        AlnAcc ka;
        std::vector<size_t> keep;
        size_t w = 0;
        for (size_t j = 0; j < nj; j++) {
            if (c->inv_jobs[j].accepted) {
                keep.push_back(j); ka.cnt.push_back(acc.cnt[j]); ka.score.push_back(acc.score[j]); ka.isrev.push_back(acc.isrev[j]);
                ka.ops.insert(ka.ops.end(), acc.ops.begin() + w, acc.ops.begin() + w + acc.cnt[j]);
            }
            w += acc.cnt[j];
        }
        ka.cnt.push_back(0); ka.score.push_back(0); ka.isrev.push_back(0);
        std::vector<uint32_t> kq, kt;
        for (size_t j : keep) { kq.push_back(opq[j]); kt.push_back(opt[j]); }
        sr_alignments *al = make_alignments_of(kq, kt, c->len, ka);
        for (size_t i = 0; i < keep.size(); i++) {
            const sr_inv_job &o = c->inv_jobs[keep[i]];
            al->query_start[i] = o.query_start; al->query_end[i] = o.query_end;
            al->target_start[i] = o.target_start; al->target_end[i] = o.target_end;
            al->is_reverse[i] = o.is_reverse;
        }
        c->inv_al = al;
    }
    return SR_OK;
}

int inv_patch_pass(sr_ctx *c) {
    return c->inv_join ? inv_patch_pass_of(c, c->inv_raw_j) : inv_patch_pass_of(c, c->inv_raw);
}

extern "C" int sr_ctx_inversion_stats(sr_ctx *c, sr_inv_stats *out) {
    if (!c || !c->loaded || !out) return sr_fail(SR_ERR_INVALID, "context not loaded");
    *out = c->inv_stats;
    return SR_OK;
}

extern "C" int sr_ctx_inversion_join_stats(sr_ctx *c, uint64_t out[4]) {
    if (!c || !c->loaded || !out) return sr_fail(SR_ERR_INVALID, "context not loaded");
    memcpy(out, c->inv_join_stats, sizeof(c->inv_join_stats));
    return SR_OK;
}

extern "C" int sr_ctx_inversion_jobs(sr_ctx *c, sr_inv_job **jobs, uint64_t *count) {
    if (!c || !c->loaded || !jobs || !count) return sr_fail(SR_ERR_INVALID, "context not loaded");
    *count = c->inv_jobs.size();
    return to_malloc(c->inv_jobs, jobs);
}

extern "C" int sr_ctx_inversion_alignments(sr_ctx *c, sr_alignments **out) {
    if (!c || !out) return sr_fail(SR_ERR_INVALID, "null argument");
    if (!c->inv_al) return sr_fail(SR_ERR_INVALID, "no patch alignments: enable with keep_alignments = 1, run, and take them once (none are kept when no job ran)");
    *out = c->inv_al;
    c->inv_al = nullptr;
    return SR_OK;
}

// tests: the scan kernels over alignments given on the host
template <class J>
static int inv_scan_device_impl(int device, const uint32_t *ops, const uint64_t *cigar_off, uint64_t n, uint64_t min_size,
                                uint32_t join_below, const SrInvPen *pen, const int32_t *score, const int32_t *max_score,
                                std::vector<J> &jobs, uint64_t stats_out[4]) {
    if (!cigar_off || (!ops && n && cigar_off[n])) return sr_fail(SR_ERR_INVALID, "null argument");
    if (min_size == 0) return sr_fail(SR_ERR_INVALID, "inversion threshold 0");
    if (n == 0 || n > 0x7fffffffULL) return sr_fail(SR_ERR_INVALID, "bad alignment count");
    int r;
    if ((r = sr_pick_device(device))) return r;
    const uint64_t nops = cigar_off[n];
    std::vector<uint32_t> raw(nops ? nops : 1), cnt(n);
    for (uint64_t i = 0; i < nops; i++) {                  // reference alphabet -> raw device alphabet (I <-> D)
        const uint32_t op = ops[i] & 3u;
        raw[i] = (ops[i] & ~15u) | (op == 0 ? SR_OP_M : op == 1 ? SR_OP_X : op == 2 ? SR_OP_D : SR_OP_I);
    }
    for (uint64_t i = 0; i < n; i++) {
        if (cigar_off[i + 1] < cigar_off[i] || cigar_off[i + 1] - cigar_off[i] > 0xffffffffULL) return sr_fail(SR_ERR_INVALID, "bad cigar_off");
        cnt[i] = (uint32_t)(cigar_off[i + 1] - cigar_off[i]);
    }
    SrScratch tmp;
    SrInvScanArgs s{};
    s.cigar_ops = (const uint32_t *)tmp.up(raw.data(), raw.size() * 4);
    s.cigar_base = (const uint64_t *)tmp.up(cigar_off, (n + 1) * 8);
    s.cigar_cnt = (const uint32_t *)tmp.up(cnt.data(), n * 4);
    s.count = (uint32_t *)tmp.alloc(n * 4);
    uint32_t *d_off = (uint32_t *)tmp.alloc((n + 1) * 4);
    s.stats = (unsigned long long *)tmp.alloc(32);
    if (!s.cigar_ops || !s.cigar_base || !s.cigar_cnt || !s.count || !d_off || !s.stats) return sr_fail(SR_ERR_NOMEM, "device allocation failed");
    HIPCHK(hipMemset(s.stats, 0, 32));
    s.npairs = (uint32_t)n; s.pair0 = 0; s.min_size = min_size;
    if (score && !(s.score = (const int32_t *)tmp.up(score, n * 4))) return sr_fail(SR_ERR_NOMEM, "device allocation failed");
    if (max_score && !(s.max_score = (const int32_t *)tmp.up(max_score, n * 4))) return sr_fail(SR_ERR_NOMEM, "device allocation failed");
    if (pen) {
        s.join_below = join_below;
        const int32_t pv[6] = {pen->x, pen->o1, pen->e1, pen->o2, pen->e2, pen->two};
        memcpy(s.pen, pv, sizeof(pv));
    }
    J *d_jobs = nullptr;
    uint64_t cap = 0;
    if ((r = inv_scan_launch(nullptr, s, d_off, &tmp.v, &d_jobs, &cap, jobs))) return r;
    if (stats_out) {
        unsigned long long ds[4];
        HIPCHK(hipMemcpy(ds, s.stats, sizeof(ds), hipMemcpyDeviceToHost));
        for (int i = 0; i < 4; i++) stats_out[i] = ds[i];
    }
    return SR_OK;
}

template <class J>
static int inv_sites_of_jobs(const std::vector<J> &jobs, sr_inv_site **sites, uint64_t **owner, uint64_t *count) {
    *count = jobs.size();
    *sites = (sr_inv_site *)malloc((jobs.empty() ? 1 : jobs.size()) * sizeof(sr_inv_site));
    *owner = (uint64_t *)malloc((jobs.empty() ? 1 : jobs.size()) * 8);
    if (!*sites || !*owner) return sr_fail(SR_ERR_NOMEM, "out of memory");
    for (size_t j = 0; j < jobs.size(); j++) {
        sr_inv_site &o = (*sites)[j];
        o.query_start = jobs[j].qa; o.query_end = (uint64_t)jobs[j].qa + jobs[j].qgap;
        o.target_start = jobs[j].ta; o.target_end = (uint64_t)jobs[j].ta + jobs[j].tgap;
        o.kind = SR_INV_DIVERGENT; o.candidate = 1;
        (*owner)[j] = jobs[j].pair;
    }
    return SR_OK;
}

extern "C" int sr_inversion_scan_device(int device, const uint32_t *ops, const uint64_t *cigar_off, uint64_t n, uint64_t min_size,
                                        sr_inv_site **sites, uint64_t **owner, uint64_t *count) {
    if (!sites || !owner || !count) return sr_fail(SR_ERR_INVALID, "null argument");
    std::vector<SrInvJob> jobs;
    const int r = inv_scan_device_impl(device, ops, cigar_off, n, min_size, 0, nullptr, nullptr, nullptr, jobs, nullptr);
    return r ? r : inv_sites_of_jobs(jobs, sites, owner, count);
}

extern "C" int sr_inversion_scan_device_join(int device, const uint32_t *ops, const uint64_t *cigar_off, uint64_t n, uint64_t min_size,
                                             uint32_t join_below, const sr_params *pen, const int32_t *score, const int32_t *max_score,
                                             sr_inv_site **sites, uint64_t **owner, int32_t **cost, uint64_t *count, uint64_t stats[4]) {
    if (!sites || !owner || !cost || !count) return sr_fail(SR_ERR_INVALID, "null argument");
    if (join_below == 0) return sr_fail(SR_ERR_INVALID, "inversion join length 0: the joined rule needs J >= 1");
    if (join_below > min_size) return sr_fail(SR_ERR_INVALID, "inversion join length above the gap threshold: an island would be a candidate by itself");
    SrInvPen ip;
    int r;
    if ((r = inv_pen_of(pen, &ip))) return r;
    std::vector<SrInvJobJ> jobs;
    if ((r = inv_scan_device_impl(device, ops, cigar_off, n, min_size, join_below, &ip, score, max_score, jobs, stats))) return r;
    if ((r = inv_sites_of_jobs(jobs, sites, owner, count))) return r;
    std::vector<int32_t> oc;
    for (const SrInvJobJ &w : jobs) oc.push_back(w.cost);
    return to_malloc(oc, cost);
}
