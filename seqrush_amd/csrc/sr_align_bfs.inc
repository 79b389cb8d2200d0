// sr_align_bfs.inc -- level-synchronous ("breadth-first") biWFA kernel, included
// by sr_device.hip.
//
// Same alignment rules as sr_align_kernel / oracle/wfa.c, different schedule:
// the segments of one recursion level of biWFA are independent, so all of them
// (forward and reverse aligner each) advance one score level per pass.  All
// aligners of a pass are at the same score level s, hence share the ring rows
// (each owns a sub-range of every row) and the row addressing is uniform; the
// cells of all aligners are flattened over the workgroup's threads, 4 adjacent
// diagonals per thread.  Orientation scoring runs the forward and the
// reverse-complement query as two aligners of one pass; base cases are batched
// the same way and back-traced one thread per base case.  Per pair this cuts
// the number of barrier-separated passes ~2.7x and keeps the lanes full at the
// deep recursion levels.
#define BJ_MAX (2 * SR_BFS_MAXACT)
#ifndef BFS_MAK_SLOTS
#define BFS_MAK_SLOTS 32            // ring depth supported by this kernel (scope + 1 <= 32)
#endif
#define BFS_BASE_MAX 16

struct BJob {                        // 72 bytes
    int base, shift, plen, tlen;     // idx = base + shift + k
    int p0, t0, sgn, begin;          // base index of v = 0 / h = 0 in the pair's sequences, direction
    int chk, seg, poff, active;      // end component tested at k_end (-1 none), owner, pattern copy, running
    int kend, pad0, pad1, pad2;
    unsigned hbase, hw;              // blocked kernel, base cases: the job's own history region (first cell, cells per row)
};

struct BSeg {                        // a segment under breakpoint search
    int pb, pe, tb, te, cb, ce;
    int score_f, score_r, last_fwd, f_ak, r_ak, phase, max_ad;   // phase: 1, 2, 3 = done, 4 = failed
    int bp_score, bp_score_f, bp_score_r, bp_k_f, bp_k_r, bp_comp, bp_off_f, bp_off_r;
    int list_pos;
};

struct BGeom { int brow, ring_scope, ring_hot, bbase_jobs, hist_w, hist_levels; unsigned urow; unsigned hist_stride; };   // hist_stride: cells per history row

struct BShared {
    BJob job[BJ_MAX];
#ifndef SR_BLK_TU                   // (the blocked kernel keeps its own per-level tables, see sr_align_blk.inc)
    int jglo[BJ_MAX], jgstart[BJ_MAX + 1], jklo[BJ_MAX], jkhi[BJ_MAX];
    int jak[2][BJ_MAX], jreach[2][BJ_MAX];
#endif
#ifndef SR_BLK_TU                   // (the blocked kernel keeps the per-level max antidiagonals in global memory)
    int mak[BJ_MAX][BFS_MAK_SLOTS];
#endif
    BSeg seg[SR_BFS_MAXACT];
#ifndef SR_BLK_TU
    int candk[5 * BFS_MAK_SLOTS];
    int cl_k[2048], cl_n;
#endif
    int ulevel[BJ_MAX];
    int njobs, nact, next_pos, nrunning, total_groups, offT;
    int err, pair, score_acc;
    uint32_t cig_cnt;
    int base_score[BFS_BASE_MAX], base_entry[BFS_BASE_MAX], bt_n[BFS_BASE_MAX];
    int nbase, emit_pos, list_n;
    SrPen pen[2];
    BGeom geom;
    unsigned long long cells;
};

__shared__ BShared b_sh;

__device__ __forceinline__ BGeom load_geom() {
    BGeom g;
    g.brow = RFL(b_sh.geom.brow); g.ring_scope = RFL(b_sh.geom.ring_scope); g.ring_hot = RFL(b_sh.geom.ring_hot);
    g.bbase_jobs = RFL(b_sh.geom.bbase_jobs); g.hist_w = RFL(b_sh.geom.hist_w); g.hist_levels = RFL(b_sh.geom.hist_levels);
    g.urow = RFL(b_sh.geom.urow); g.hist_stride = RFL(b_sh.geom.hist_stride);
    return g;
}
__device__ __forceinline__ SrPen load_bpen(int sel) {
    const SrPen &q = b_sh.pen[sel];
    SrPen p;
    p.x = RFL(q.x); p.o1 = RFL(q.o1); p.e1 = RFL(q.e1); p.o2 = RFL(q.o2); p.e2 = RFL(q.e2);
    p.two = RFL(q.two); p.scope = RFL(q.scope);
    return p;
}

// segment list record (global, SR_BFS_SEGREC ints)
enum { SL_PB = 0, SL_PE, SL_TB, SL_TE, SL_CB, SL_CE, SL_REM, SL_KIND, SL_BV, SL_BH, SL_BCOMP, SL_BSF, SL_BSR,
       SL_SOLVED, SL_PASSES };       // (blocked kernel, replaying pair: breakpoint taken from a record; passes its search took)
enum { SK_TRIVIAL = 0, SK_BASE = 1, SK_BP = 2 };

__device__ __forceinline__ int seg_kind(int plen, int tlen, int score_rem) {
    if (plen == 0 || tlen == 0) return SK_TRIVIAL;
    if (score_rem <= 250 || max(plen, tlen) <= 100) return SK_BASE;
    return SK_BP;
}

template <typename OT>
struct BRows {
    GP<OT> pMx, pMo1, pI1, pD1, pMo2, pI2, pD2;
    GP<OT> oM, oI1, oD1, oI2, oD2, cI1, cD1, cI2, cD2;
};

// ring rows of level s (all aligners of the pass share them)
template <typename OT, bool TWO>
__device__ __forceinline__ void brows_ring(BRows<OT> &r, GP<OT> bring, const SrAlignArgs &a, const SrPen &pen, int s,
                                           bool with_cold) {
    const size_t w = (size_t)a.brow;
    const int nsm = pen.scope + 1, ns1 = pen.e1 + 2, ns2 = pen.two ? pen.e2 + 2 : 2;
    GP<OT> m = bring;
    GP<OT> g = bring + (size_t)(a.ring_scope + 1) * w;
    GP<OT> gI1 = g, gI2 = g + (size_t)a.ring_hot * w, gD1 = g + 2 * (size_t)a.ring_hot * w, gD2 = g + 3 * (size_t)a.ring_hot * w;
    GP<OT> cold = g + 4 * (size_t)a.ring_hot * w;
    GP<OT> nul = cold + (size_t)(a.ring_scope + 1) * 4 * w;
    r.pMx = (s >= pen.x) ? m + (size_t)((s - pen.x) % nsm) * w : nul;
    r.pMo1 = (s >= pen.o1 + pen.e1) ? m + (size_t)((s - pen.o1 - pen.e1) % nsm) * w : nul;
    r.pI1 = (s >= pen.e1) ? gI1 + (size_t)((s - pen.e1) % ns1) * w : nul;
    r.pD1 = (s >= pen.e1) ? gD1 + (size_t)((s - pen.e1) % ns1) * w : nul;
    r.pMo2 = r.pI2 = r.pD2 = nul;
    if (TWO) {
        if (s >= pen.o2 + pen.e2) r.pMo2 = m + (size_t)((s - pen.o2 - pen.e2) % nsm) * w;
        if (s >= pen.e2) { r.pI2 = gI2 + (size_t)((s - pen.e2) % ns2) * w; r.pD2 = gD2 + (size_t)((s - pen.e2) % ns2) * w; }
    }
    r.oM = m + (size_t)(s % nsm) * w;
    r.oI1 = gI1 + (size_t)(s % ns1) * w; r.oD1 = gD1 + (size_t)(s % ns1) * w;
    r.oI2 = gI2 + (size_t)(s % ns2) * w; r.oD2 = gD2 + (size_t)(s % ns2) * w;
    r.cI1 = r.cD1 = r.cI2 = r.cD2 = nullptr;
    if (with_cold) {
        GP<OT> c = cold + (size_t)(s % nsm) * 4 * w;
        r.cI1 = c; r.cI2 = c + w; r.cD1 = c + 2 * w; r.cD2 = c + 3 * w;
    }
}
// arbitrary level / component of the ring (breakpoint detection); cold history for I/D
template <typename OT, typename G>
__device__ __forceinline__ GP<OT> bring_row(GP<OT> bring, const G &a, const SrPen &pen, int s, int comp) {
    const size_t w = (size_t)a.brow;
    const int nsm = pen.scope + 1;
    if (comp == SR_C_M) return bring + (size_t)(s % nsm) * w;
    GP<OT> cold = bring + ((size_t)(a.ring_scope + 1) + 4 * (size_t)a.ring_hot) * w;
    return cold + ((size_t)(s % nsm) * 4 + (comp - 1)) * w;
}
// base-case history rows: [level][comp][hist_stride] (this kernel: bbase_jobs * hist_w cells per row, NULL row after the last level;
// the blocked kernel packs the jobs of a batch side by side and sets the stride per batch)
template <typename OT, typename G>
__device__ __forceinline__ GP<OT> bhist_row(GP<OT> bhist, const G &a, int s, int comp) {
    const size_t w = (size_t)a.hist_stride;
    return bhist + ((size_t)s * 5 + comp) * w;
}
template <typename OT, bool TWO>
__device__ __forceinline__ void brows_hist(BRows<OT> &r, GP<OT> bhist, const SrAlignArgs &a, const SrPen &pen, int s) {
    GP<OT> nul = bhist_row(bhist, a, a.hist_levels, 0);
    r.pMx = (s >= pen.x) ? bhist_row(bhist, a, s - pen.x, SR_C_M) : nul;
    r.pMo1 = (s >= pen.o1 + pen.e1) ? bhist_row(bhist, a, s - pen.o1 - pen.e1, SR_C_M) : nul;
    r.pI1 = (s >= pen.e1) ? bhist_row(bhist, a, s - pen.e1, SR_C_I1) : nul;
    r.pD1 = (s >= pen.e1) ? bhist_row(bhist, a, s - pen.e1, SR_C_D1) : nul;
    r.pMo2 = r.pI2 = r.pD2 = nul;
    if (TWO) {
        if (s >= pen.o2 + pen.e2) r.pMo2 = bhist_row(bhist, a, s - pen.o2 - pen.e2, SR_C_M);
        if (s >= pen.e2) { r.pI2 = bhist_row(bhist, a, s - pen.e2, SR_C_I2); r.pD2 = bhist_row(bhist, a, s - pen.e2, SR_C_D2); }
    }
    r.oM = bhist_row(bhist, a, s, SR_C_M); r.oI1 = bhist_row(bhist, a, s, SR_C_I1); r.oD1 = bhist_row(bhist, a, s, SR_C_D1);
    r.oI2 = bhist_row(bhist, a, s, SR_C_I2); r.oD2 = bhist_row(bhist, a, s, SR_C_D2);
    r.cI1 = r.cD1 = r.cI2 = r.cD2 = nullptr;
}

// per-lane view of the aligner a group belongs to
#ifndef SR_BLK_TU
struct LaneJob { int base, shift, plen, tlen, p0, t0, sgn, begin, chk, kend, poff, jid, klo, khi; };

template <typename OT, bool TWO>
__device__ __forceinline__ void bgroup_load(const BRows<OT> &r, const LaneJob &j, int lg, int s, GroupIn<OT> &in) {
    const V4<OT> nv = {(OT)NULLV, (OT)NULLV, (OT)NULLV, (OT)NULLV};
    in.mo1 = in.i1 = in.d1 = in.mo2 = in.i2 = in.d2 = in.mx = nv;
    in.mo1L = in.mo1R = in.i1L = in.d1R = in.mo2L = in.mo2R = in.i2L = in.d2R = NULLV;
    const int k0 = (lg << 2) - j.shift;
    const unsigned idx0 = (unsigned)(j.base + (lg << 2));
    if (s > 0 && k0 + 3 >= j.klo && k0 <= j.khi) {
        in.mo1 = ld4<OT>(r.pMo1, idx0); in.i1 = ld4<OT>(r.pI1, idx0); in.d1 = ld4<OT>(r.pD1, idx0);
        in.mx = ld4<OT>(r.pMx, idx0);
        if (TWO) { in.mo2 = ld4<OT>(r.pMo2, idx0); in.i2 = ld4<OT>(r.pI2, idx0); in.d2 = ld4<OT>(r.pD2, idx0); }
        if (k0 >= j.klo) {
            in.mo1L = (int)r.pMo1[idx0 - 1]; in.i1L = (int)r.pI1[idx0 - 1];
            if (TWO) { in.mo2L = (int)r.pMo2[idx0 - 1]; in.i2L = (int)r.pI2[idx0 - 1]; }
        }
        if (k0 + 3 <= j.khi) {
            in.mo1R = (int)r.pMo1[idx0 + 4]; in.d1R = (int)r.pD1[idx0 + 4];
            if (TWO) { in.mo2R = (int)r.pMo2[idx0 + 4]; in.d2R = (int)r.pD2[idx0 + 4]; }
        }
    }
}

template <typename OT, bool TWO>
__device__ __forceinline__ void bgroup_finish(const BRows<OT> &r, const LaneJob &j, int lg, int s, const GroupIn<OT> &in,
                                              int par, LP T) {
    const int k0 = (lg << 2) - j.shift;
    const unsigned idx0 = (unsigned)(j.base + (lg << 2));
    const LP P = (LP)(lds_seq + j.poff);
    int mv[4], i1v[4], i2v[4], d1v[4], d2v[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int k = k0 + q;
        int m = NULLV, i1 = NULLV, i2 = NULLV, d1 = NULLV, d2 = NULLV;
        if (k >= j.klo && k <= j.khi) {
            if (s == 0) {
                if (k == 0) {
                    if (j.begin == SR_C_M) m = 0;
                    else if (j.begin == SR_C_I1) i1 = 0;
                    else if (j.begin == SR_C_I2) i2 = 0;
                    else if (j.begin == SR_C_D1) d1 = 0;
                    else d2 = 0;
                }
            } else {
                const unsigned lim = (unsigned)min(j.tlen, j.plen + k);
                const int a1 = (q == 0) ? in.mo1L : (int)in.mo1[q == 0 ? 0 : q - 1];
                const int b1 = (q == 0) ? in.i1L : (int)in.i1[q == 0 ? 0 : q - 1];
                const int c1 = (q == 3) ? in.mo1R : (int)in.mo1[q == 3 ? 3 : q + 1];
                const int e1 = (q == 3) ? in.d1R : (int)in.d1[q == 3 ? 3 : q + 1];
                i1 = bnd(max(a1, b1) + 1, lim);
                d1 = bnd(max(c1, e1), lim);
                if (TWO) {
                    const int a2 = (q == 0) ? in.mo2L : (int)in.mo2[q == 0 ? 0 : q - 1];
                    const int b2 = (q == 0) ? in.i2L : (int)in.i2[q == 0 ? 0 : q - 1];
                    const int c2 = (q == 3) ? in.mo2R : (int)in.mo2[q == 3 ? 3 : q + 1];
                    const int e2 = (q == 3) ? in.d2R : (int)in.d2[q == 3 ? 3 : q + 1];
                    i2 = bnd(max(a2, b2) + 1, lim);
                    d2 = bnd(max(c2, e2), lim);
                }
                m = bnd((int)in.mx[q] + 1, lim);
                m = max(m, max(max(i1, i2), max(d1, d2)));
                if (m < 0) m = NULLV;
            }
        }
        mv[q] = m; i1v[q] = i1; i2v[q] = i2; d1v[q] = d1; d2v[q] = d2;
    }
    // extension (first 16-base window of the four cells fetched together)
    uint32_t xw[4];
    int nn[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        nn[q] = 0; xw[q] = 1u;
        if (mv[q] >= 0) {
            const int v = mv[q] - (k0 + q), h = mv[q];
            nn[q] = min(j.plen - v, j.tlen - h);
            if (nn[q] > 0) {
                if (j.sgn > 0) xw[q] = win_fwd(P, j.p0 + v) ^ win_fwd(T, j.t0 + h);
                else xw[q] = win_rev(P, j.p0 - v) ^ win_rev(T, j.t0 - h);
            }
        }
    }
    int ak = 0;
    bool reached = false;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int k = k0 + q;
        if (mv[q] >= 0) {
            if (nn[q] > 0) {
                int c;
                if (j.sgn > 0) c = xw[q] ? ((__ffs((int)xw[q]) - 1) >> SR_SYM_LOG) : SR_WIN;
                else c = xw[q] ? (__clz((int)xw[q]) >> SR_SYM_LOG) : SR_WIN;
                c = min(c, nn[q]);
                if (xw[q] == 0 && nn[q] > SR_WIN) {
                    const int v = mv[q] - k + SR_WIN, h = mv[q] + SR_WIN;
                    if (j.sgn > 0) c += ext_fwd(P, T, j.p0 + v, j.t0 + h, nn[q] - SR_WIN);
                    else c += ext_rev(P, T, j.p0 - v, j.t0 - h, nn[q] - SR_WIN);
                }
                mv[q] += c;
            }
            ak = max(ak, 2 * mv[q] - k);
        }
        if (j.chk >= 0 && k == j.kend && k >= j.klo && k <= j.khi) {
            int val = mv[q];
            if (j.chk == SR_C_I1) val = i1v[q];
            else if (j.chk == SR_C_I2) val = i2v[q];
            else if (j.chk == SR_C_D1) val = d1v[q];
            else if (j.chk == SR_C_D2) val = d2v[q];
            if (val >= j.tlen) reached = true;
        }
    }
    if (ak > 0) atomicMax(&b_sh.jak[par][j.jid], ak);
    if (reached) b_sh.jreach[par][j.jid] = 1;
    V4<OT> oM, oI1, oI2, oD1, oD2;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        oM[q] = (OT)mv[q]; oI1[q] = (OT)i1v[q]; oI2[q] = (OT)i2v[q]; oD1[q] = (OT)d1v[q]; oD2[q] = (OT)d2v[q];
    }
    st4<OT>(r.oM, idx0, oM); st4<OT>(r.oI1, idx0, oI1); st4<OT>(r.oD1, idx0, oD1);
    if (TWO) { st4<OT>(r.oI2, idx0, oI2); st4<OT>(r.oD2, idx0, oD2); }
    if (r.cI1) {
        st4<OT>(r.cI1, idx0, oI1); st4<OT>(r.cD1, idx0, oD1);
        if (TWO) { st4<OT>(r.cI2, idx0, oI2); st4<OT>(r.cD2, idx0, oD2); }
    }
}

__device__ __forceinline__ void lane_job(int jid, LaneJob &lj) {
    const BJob &b = b_sh.job[jid];
    lj.base = b.base; lj.shift = b.shift; lj.plen = b.plen; lj.tlen = b.tlen;
    lj.p0 = b.p0; lj.t0 = b.t0; lj.sgn = b.sgn; lj.begin = b.begin;
    lj.chk = b.chk; lj.kend = b.kend; lj.poff = b.poff; lj.jid = jid;
    lj.klo = b_sh.jklo[jid]; lj.khi = b_sh.jkhi[jid];
}

// One pass: level s of every active aligner.  Ends with the data of the pass
// still in flight: the caller's __syncthreads() publishes rows and reductions.
template <typename OT, bool TWO, int NT>
__device__ __forceinline__ void bfs_pass(const BRows<OT> &r, int s, const SrPen &pen, int njobs, int par) {
    const int tid = threadIdx.x;
    // per-aligner ranges of this level + flat work list (wave 0: one aligner per lane, prefix by shuffles)
    if (tid < 64) {
        int n = 0, glo = 0, klo = 0, khi = -1;
        if (tid < njobs && b_sh.job[tid].active) {
            const BJob &b = b_sh.job[tid];
            const int R = reach(pen, s, b.begin);
            klo = max(-b.plen, -R); khi = min(b.tlen, R);
            const int wlo = max(-b.plen - 1, -R - pen.scope - 1), whi = min(b.tlen + 1, R + pen.scope + 1);
            glo = (wlo + b.shift) >> 2;
            n = ((whi + b.shift) >> 2) - glo + 1;
        }
        int incl = n;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(incl, o, 64); if (tid >= o) incl += v; }
        if (tid < BJ_MAX) {
            b_sh.jglo[tid] = glo; b_sh.jklo[tid] = klo; b_sh.jkhi[tid] = khi;
            b_sh.jgstart[tid + 1] = incl;
            b_sh.jak[par][tid] = 0; b_sh.jreach[par][tid] = 0;
        }
        if (tid == 0) b_sh.jgstart[0] = 0;
        if (tid == 63) b_sh.total_groups = incl;
        int cells = (khi >= klo) ? khi - klo + 1 : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cells += __shfl_xor(cells, o, 64);
        if (tid == 0) b_sh.cells += (unsigned long long)cells;
    }
    __syncthreads();
    const int total = RFL(b_sh.total_groups);
    const LP T = (LP)(lds_seq + RFL(b_sh.offT));
    for (int g0 = tid; g0 < total; g0 += 2 * NT) {
        const int g1 = g0 + NT;
        LaneJob j0, j1;
        GroupIn<OT> i0, i1;
        int lg0, lg1 = 0;
        {
            int lo = 0, hi = njobs;            // last job with jgstart <= g0
            while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (b_sh.jgstart[mid] <= g0) lo = mid; else hi = mid; }
            lane_job(lo, j0); lg0 = b_sh.jglo[lo] + (g0 - b_sh.jgstart[lo]);
        }
        bgroup_load<OT, TWO>(r, j0, lg0, s, i0);
        if (g1 < total) {
            int lo = 0, hi = njobs;
            while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (b_sh.jgstart[mid] <= g1) lo = mid; else hi = mid; }
            lane_job(lo, j1); lg1 = b_sh.jglo[lo] + (g1 - b_sh.jgstart[lo]);
            bgroup_load<OT, TWO>(r, j1, lg1, s, i1);
        }
        bgroup_finish<OT, TWO>(r, j0, lg0, s, i0, par, T);
        if (g1 < total) bgroup_finish<OT, TWO>(r, j1, lg1, s, i1, par, T);
    }
}

// Breakpoint detection for segment sa: level score_0 of aligner (2*sa + side0)
// against the last `scope` levels of the other one (oracle bialign_overlap).
//
// The oracle walks (i ascending, component in the order D2 I2 D1 I1 M), takes the
// smallest overlapping diagonal of each (i, component) and accepts it when
// score_0 + score_i - gap(component) is strictly below the running best.  The
// accepted value depends on (i, component) only, so the outcome of the whole walk
// is the candidate with the smallest value, earliest in walk order among equals,
// if that value is below the incoming best -- evaluated here as one reduction.
//
// Diagonals are pre-filtered with an upper bound: U[k] = max M offset of the
// other aligner over (a superset of) its last `scope` levels (M bounds every
// component of its level; level 0 takes all components because the begin
// component need not be M).  Only diagonals with M0[k0] + U1[kinv - k0] >= tlen
// can overlap at all; U is kept up to date incrementally, one row per aligner.
#define BFS_CL_MAX 2048
template <typename OT, bool TWO, int NT>
__device__ __noinline__ void bfs_overlap(GP<OT> bring, int a_, int side0_, int score_0_, int score_1_,
                                         int bp_forward_) {
    const BGeom a = load_geom();
    const int tid = threadIdx.x;
    const int sa = RFL(a_), side0 = RFL(side0_), score_0 = RFL(score_0_), score_1 = RFL(score_1_);
    const bool bp_forward = RFL(bp_forward_) != 0;
    const SrPen pen = load_bpen(0);
    const int j0 = 2 * sa + side0, j1 = 2 * sa + (1 - side0);
    const int plen = RFL(b_sh.job[j0].plen), tlen = RFL(b_sh.job[j0].tlen);
    const int off0 = RFL(b_sh.job[j0].base) + RFL(b_sh.job[j0].shift), off1 = RFL(b_sh.job[j1].base) + RFL(b_sh.job[j1].shift);
    const int beg0 = RFL(b_sh.job[j0].begin), beg1 = RFL(b_sh.job[j1].begin);
    const int kinv = tlen - plen;
    const int nsm = pen.scope + 1;
    const int gapmax = TWO ? max(pen.o1, pen.o2) : pen.o1;
    const int bp_in = RFL(b_sh.seg[sa].bp_score);
    // which levels i can matter at all (wave-uniform mask, computed by every wave)
    // (two 64-bit words: the wide instance has up to 128 levels in scope)
    unsigned long long imask, imask_hi;
    {
        bool ok[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int i = (tid & 63) + 64 * h;
            ok[h] = false;
            if (i < pen.scope && i < BFS_MAK_SLOTS && score_1 - i >= 0) {
                const int mak0 = b_sh.mak[j0][score_0 % nsm], mak1 = b_sh.mak[j1][(score_1 - i) % nsm];
                ok[h] = (mak0 + mak1 >= plen + tlen) && (score_0 + score_1 - i - gapmax < bp_in);
            }
        }
        imask = __ballot(ok[0]); imask_hi = __ballot(ok[1]);
    }
    if ((imask | imask_hi) == 0ull) return;
    const int ni_lo = __popcll(imask), ni = ni_lo + __popcll(imask_hi);
    for (int t = tid; t < 5 * BFS_MAK_SLOTS; t += NT) b_sh.candk[t] = INT_MAX;
    if (tid == 0) b_sh.cl_n = 0;
    // ---- bring U of the other aligner up to level score_1
    GP<OT> U1 = bring + a.urow + off1;
    {
        const int ul = RFL(b_sh.ulevel[j1]);
        const int lv_from = max(max(ul + 1, score_1 - pen.scope + 1), 0);
        if (lv_from <= score_1) {
            const int Rn = reach(pen, score_1, beg1);
            const int klo = max(-plen, -Rn), khi = min(tlen, Rn);
            int ulo = 1, uhi = 0;                              // diagonals U already covers
            if (ul >= 0) { const int Ro = reach(pen, ul, beg1); ulo = max(-plen, -Ro); uhi = min(tlen, Ro); }
            for (int k = klo + tid; k <= khi; k += NT) {
                int v = (k >= ulo && k <= uhi) ? (int)U1[k] : NULLV;
                for (int lv = lv_from; lv <= score_1; lv++) {
                    const int Rl = reach(pen, lv, beg1);
                    if (k < -Rl || k > Rl) continue;
                    v = max(v, (int)(bring_row<OT>(bring, a, pen, lv, SR_C_M) + off1)[k]);
                    if (lv == 0) {
#pragma unroll
                        for (int c = 1; c < 5; c++) {
                            if (!TWO && (c == SR_C_I2 || c == SR_C_D2)) continue;
                            v = max(v, (int)(bring_row<OT>(bring, a, pen, 0, c) + off1)[k]);
                        }
                    }
                }
                U1[k] = (OT)v;
            }
        }
    }
    __syncthreads();
    if (tid == 0) b_sh.ulevel[j1] = max(RFL(b_sh.ulevel[j1]), score_1);
    const int R0 = reach(pen, score_0, beg0);
    const int klo0 = max(-plen, -R0), khi0 = min(tlen, R0);
    const int R1 = reach(pen, score_1, beg1);
    const int klo1 = max(-plen, -R1), khi1 = min(tlen, R1);
    const int lo = max(klo0, kinv - khi1), hi = min(khi0, kinv - klo1);
    GP<OT> M0 = bring_row<OT>(bring, a, pen, score_0, SR_C_M) + off0;
    for (int c0 = lo; c0 <= hi; c0 += BFS_CL_MAX) {            // chunks the candidate list always holds
        const int c1 = min(hi, c0 + BFS_CL_MAX - 1);
        for (int k0 = c0 + tid; k0 <= c1; k0 += NT) {
            int m0 = (int)M0[k0];
            if (score_0 == 0) {
#pragma unroll
                for (int c = 1; c < 5; c++) {
                    if (!TWO && (c == SR_C_I2 || c == SR_C_D2)) continue;
                    m0 = max(m0, (int)(bring_row<OT>(bring, a, pen, 0, c) + off0)[k0]);
                }
            }
            const int u1 = (int)U1[kinv - k0];
            if (m0 >= 0 && u1 >= 0 && m0 + u1 >= tlen) b_sh.cl_k[atomicAdd(&b_sh.cl_n, 1)] = k0;
        }
        __syncthreads();
        const int n = RFL(b_sh.cl_n);
        if (n > 0) {
            for (int t = tid; t < n * ni; t += NT) {
                const int ci = t / ni, ii = t - ci * ni;
                // ii-th set bit of the level mask
                const bool hi_ = ii >= ni_lo;
                unsigned long long m = hi_ ? imask_hi : imask;
                for (int z = hi_ ? ni_lo : 0; z < ii; z++) m &= m - 1;
                const int i = __ffsll((long long)m) - 1 + (hi_ ? 64 : 0);
                const int score_i = score_1 - i;
                const int k0 = b_sh.cl_k[ci], k1 = kinv - k0;
                const int Ri = reach(pen, score_i, beg1);
                if (k1 < max(-plen, -Ri) || k1 > min(tlen, Ri)) continue;
#pragma unroll
                for (int c = 0; c < 5; c++) {
                    if (!TWO && (c == SR_C_I2 || c == SR_C_D2)) continue;
                    const int o0 = (int)(bring_row<OT>(bring, a, pen, score_0, c) + off0)[k0];
                    const int o1 = (int)(bring_row<OT>(bring, a, pen, score_i, c) + off1)[k1];
                    if (o0 >= 0 && o1 >= 0 && o0 + o1 >= tlen) atomicMin(&b_sh.candk[i * 5 + c], k0);
                }
            }
        }
        __syncthreads();
        if (tid == 0) b_sh.cl_n = 0;
        // the next chunk's appends come after its own barrier-free filter loop: order them after this reset
        __syncthreads();
    }
    // ---- the walk as one reduction (wave 0)
    if (tid < 64) {
        // 64-bit key (round 4, ADVICE r3): the value field is 32 bits wide, so no score a 32-bit search can reach is cut off
        // (a 32-bit key left 22 bits: 4.19 M, below what x = 60 on divergent 100 kb pairs reaches)
        unsigned long long best = ~0ull;
        for (int e = tid; e < 5 * pen.scope; e += 64) {
            const int i = e / 5, c = e - i * 5;
            if (b_sh.candk[e] == INT_MAX) continue;
            const int gap = (c == SR_C_M) ? 0 : ((c == SR_C_I1 || c == SR_C_D1) ? pen.o1 : pen.o2);
            const int rank = (c == SR_C_D2) ? 0 : (c == SR_C_I2) ? 1 : (c == SR_C_D1) ? 2 : (c == SR_C_I1) ? 3 : 4;
            const int val = score_0 + score_1 - i - gap;
            const unsigned long long key = ((unsigned long long)(unsigned)(val + gapmax) << 10) | (unsigned long long)(unsigned)(i * 5 + rank);      // (i * 5 + rank < 640)
            best = min(best, key);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)best, o, 64), hi = (unsigned)__shfl_xor((int)(unsigned)(best >> 32), o, 64);
            best = min(best, ((unsigned long long)hi << 32) | lo);
        }
        if (tid == 0 && best != ~0ull) {
            const int val = (int)(unsigned)(best >> 10) - gapmax;
            if (val < bp_in) {
                const int ord = (int)(best & 1023u), i = ord / 5, rank = ord - i * 5;
                const int c = (rank == 0) ? SR_C_D2 : (rank == 1) ? SR_C_I2 : (rank == 2) ? SR_C_D1 : (rank == 3) ? SR_C_I1 : SR_C_M;
                const int score_i = score_1 - i;
                const int k0 = b_sh.candk[i * 5 + c], k1 = kinv - k0;
                const int o0 = (int)(bring_row<OT>(bring, a, pen, score_0, c) + off0)[k0];
                const int o1 = (int)(bring_row<OT>(bring, a, pen, score_i, c) + off1)[k1];
                BSeg &sg = b_sh.seg[sa];
                if (bp_forward) {
                    sg.bp_score_f = score_0; sg.bp_score_r = score_i;
                    sg.bp_k_f = k0; sg.bp_k_r = k1; sg.bp_off_f = o0; sg.bp_off_r = o1;
                } else {
                    sg.bp_score_f = score_i; sg.bp_score_r = score_0;
                    sg.bp_k_f = k1; sg.bp_k_r = k0; sg.bp_off_f = o1; sg.bp_off_r = o0;
                }
                sg.bp_score = val;
                sg.bp_comp = c;
            }
        }
    }
    __syncthreads();
}

#endif  // !SR_BLK_TU
__device__ __forceinline__ void bfs_bt_push(GP<uint32_t> buf, int &n, int op, int len, int &err) {
    if (len <= 0) return;
    if (n > 0 && (int)(buf[n - 1] & 15u) == op) { buf[n - 1] += (uint32_t)len << 4; return; }
    if (n >= SR_BFS_BTCAP) { err |= SR_DEV_ERR_CIGAR_OVERFLOW; return; }
    buf[n++] = ((uint32_t)len << 4) | (uint32_t)op;
}

// one thread: backtrace of base case `bj` (oracle wfa_full); reversed run-length ops into buf.  Returns the error bits,
// | SR_MIRROR_BT_TIE when an M step had an I tag and a D tag at the maximum offset and no MISMS (sr_mirror_rule.h: the
// transposed pair would have picked the other one; the steps inside an I / D component are symmetric)
template <typename OT, bool TWO>
// hist / hstride: first cell and cells per row of the history rows [level][component] the job's columns live in
__device__ SR_BT_ATTR int bfs_backtrace(GP<OT> hist, unsigned hstride, int bj, int score, GP<uint32_t> buf, int *n_out) {
    const SrPen pen = b_sh.pen[0];
    const BJob &b = b_sh.job[bj];
    const int plen = b.plen, tlen = b.tlen, cb = b.begin, ce = b.chk;
    const int off = b.base + b.shift;
    int err = 0, n = 0, tie = 0;
    int s = score, k = tlen - plen, comp = ce, o = tlen;
    bool done = false;
#define HR(S, C) (hist + ((size_t)(S) * 5 + (size_t)(C)) * (size_t)hstride + off)
    for (int guard = 0; guard < 4 * (plen + tlen) + 64 && !done; guard++) {
        if (comp == SR_C_M) {
            if (s == 0) {
                if (cb != SR_C_M || k != 0) err |= SR_DEV_ERR_BACKTRACE;
                bfs_bt_push(buf, n, SR_OP_M, o, err);
                done = true; break;
            }
            const unsigned lim = (unsigned)min(tlen, plen + k);
            int bo = NULLV, bty = 0, bi = NULLV;                  // bi: the furthest offset an I tag reaches
            if (s >= pen.x) bt_best(bo, bty, bnd((int)HR(s - pen.x, SR_C_M)[k] + 1, lim), 9);
            if (s >= pen.o1 + pen.e1) {
                const GP<OT> r = HR(s - pen.o1 - pen.e1, SR_C_M);
                bt_best_ins(bo, bty, bi, bnd((int)r[k - 1] + 1, lim), 1);
                bt_best(bo, bty, bnd((int)r[k + 1], lim), 5);
            }
            if (s >= pen.e1) {
                bt_best_ins(bo, bty, bi, bnd((int)HR(s - pen.e1, SR_C_I1)[k - 1] + 1, lim), 2);
                bt_best(bo, bty, bnd((int)HR(s - pen.e1, SR_C_D1)[k + 1], lim), 6);
            }
            if (TWO) {
                if (s >= pen.o2 + pen.e2) {
                    const GP<OT> r = HR(s - pen.o2 - pen.e2, SR_C_M);
                    bt_best_ins(bo, bty, bi, bnd((int)r[k - 1] + 1, lim), 3);
                    bt_best(bo, bty, bnd((int)r[k + 1], lim), 7);
                }
                if (s >= pen.e2) {
                    bt_best_ins(bo, bty, bi, bnd((int)HR(s - pen.e2, SR_C_I2)[k - 1] + 1, lim), 4);
                    bt_best(bo, bty, bnd((int)HR(s - pen.e2, SR_C_D2)[k + 1], lim), 8);
                }
            }
            if (bty == 0 || bo > o) { err |= SR_DEV_ERR_BACKTRACE; break; }
            if (sr_mirror_bt_tie(bty, bo, bi)) tie = SR_MIRROR_BT_TIE;
            bfs_bt_push(buf, n, SR_OP_M, o - bo, err);
            o = bo;
            switch (bty) {
            case 9: bfs_bt_push(buf, n, SR_OP_X, 1, err); o -= 1; s -= pen.x; break;
            case 1: bfs_bt_push(buf, n, SR_OP_I, 1, err); o -= 1; k -= 1; s -= pen.o1 + pen.e1; break;
            case 2: bfs_bt_push(buf, n, SR_OP_I, 1, err); o -= 1; k -= 1; s -= pen.e1; comp = SR_C_I1; break;
            case 3: bfs_bt_push(buf, n, SR_OP_I, 1, err); o -= 1; k -= 1; s -= pen.o2 + pen.e2; break;
            case 4: bfs_bt_push(buf, n, SR_OP_I, 1, err); o -= 1; k -= 1; s -= pen.e2; comp = SR_C_I2; break;
            case 5: bfs_bt_push(buf, n, SR_OP_D, 1, err); k += 1; s -= pen.o1 + pen.e1; break;
            case 6: bfs_bt_push(buf, n, SR_OP_D, 1, err); k += 1; s -= pen.e1; comp = SR_C_D1; break;
            case 7: bfs_bt_push(buf, n, SR_OP_D, 1, err); k += 1; s -= pen.o2 + pen.e2; break;
            default: bfs_bt_push(buf, n, SR_OP_D, 1, err); k += 1; s -= pen.e2; comp = SR_C_D2; break;
            }
        } else {
            if (s == 0) {
                if (comp != cb || k != 0 || o != 0) err |= SR_DEV_ERR_BACKTRACE;
                done = true; break;
            }
            const bool is_ins = (comp == SR_C_I1 || comp == SR_C_I2);
            const bool p1 = (comp == SR_C_I1 || comp == SR_C_D1);
            const int go = p1 ? pen.o1 : pen.o2, ge = p1 ? pen.e1 : pen.e2;
            const unsigned lim = (unsigned)min(tlen, plen + k);
            int c_open = NULLV, c_ext = NULLV;
            if (is_ins) {
                if (s >= go + ge) c_open = bnd((int)HR(s - go - ge, SR_C_M)[k - 1] + 1, lim);
                if (s >= ge) c_ext = bnd((int)HR(s - ge, comp)[k - 1] + 1, lim);
            } else {
                if (s >= go + ge) c_open = bnd((int)HR(s - go - ge, SR_C_M)[k + 1], lim);
                if (s >= ge) c_ext = bnd((int)HR(s - ge, comp)[k + 1], lim);
            }
            bool take_ext;
            if (c_ext >= 0 && c_ext >= c_open) take_ext = true;
            else if (c_open >= 0) take_ext = false;
            else { err |= SR_DEV_ERR_BACKTRACE; break; }
            if ((take_ext ? c_ext : c_open) != o) { err |= SR_DEV_ERR_BACKTRACE; break; }
            if (is_ins) { bfs_bt_push(buf, n, SR_OP_I, 1, err); o -= 1; k -= 1; }
            else { bfs_bt_push(buf, n, SR_OP_D, 1, err); k += 1; }
            if (take_ext) s -= ge; else { s -= go + ge; comp = SR_C_M; }
        }
        if (s < 0) { err |= SR_DEV_ERR_BACKTRACE; break; }
    }
#undef HR
    if (!done) err |= SR_DEV_ERR_BACKTRACE;
    *n_out = n;
    return err | tie;
}

// thread 0: describe aligner jid
__device__ __forceinline__ void bjob_set(int jid, int base, int pb, int pe, int tb, int te, int rev, int begin, int chk,
                                         int seg, int poff) {
    BJob &b = b_sh.job[jid];
    const int plen = pe - pb, tlen = te - tb;
    b.base = base; b.shift = plen + 1; b.plen = plen; b.tlen = tlen;
    b.p0 = rev ? pe - 1 : pb; b.t0 = rev ? te - 1 : tb; b.sgn = rev ? -1 : 1; b.begin = begin;
    b.chk = chk; b.seg = seg; b.poff = poff; b.active = 1; b.kend = tlen - plen;
    b_sh.ulevel[jid] = -1;
}
__device__ __forceinline__ int bjob_width(int plen, int tlen) { return ((plen + tlen + 3) + 3 + 4) & ~3; }

#ifndef SR_BLK_TU
template <typename OT, int NT, bool TWO>
__global__ void __launch_bounds__(NT, (NT >= 512 ? NT / 256 : SR_MIN_WAVES)) sr_align_bfs_kernel(SrAlignArgs a) {
    const int tid = threadIdx.x;
    GP<OT> bring = (GP<OT>)(OT *)a.bring + (size_t)blockIdx.x * a.bring_wg_stride;
    GP<OT> bhist = (GP<OT>)(OT *)a.bhist + (size_t)blockIdx.x * a.bhist_wg_stride;
    GP<int> lists = (GP<int>)a.bseg + (size_t)blockIdx.x * 2 * SR_BFS_MAXSEG * SR_BFS_SEGREC;
    GP<uint32_t> btbuf = (GP<uint32_t>)a.bbt + (size_t)blockIdx.x * a.bbase_jobs * SR_BFS_BTCAP;
    unsigned long long steps = 0, nbase = 0, nbp = 0, t_ori = 0, t_bp = 0, t_base = 0, t_all = 0;
    unsigned long long tq_pass = 0, tq_bar = 0, tq_ctl = 0, tq_ph2 = 0, tq_tail = 0, npass = 0;
    {   // NULL rows
        GP<OT> nr = bring + a.bring_wg_stride - 2 * (size_t)a.brow;      // [.. NULL row][U row]
        for (int i = tid; i < a.brow; i += NT) nr[i] = (OT)NULLV;
        const int hw = a.bbase_jobs * a.hist_w;
        GP<OT> nh = bhist_row<OT>(bhist, a, a.hist_levels, 0);
        for (int i = tid; i < hw; i += NT) nh[i] = (OT)NULLV;
        if (tid == 0) {
            b_sh.pen[0] = a.pen; b_sh.pen[1] = a.ori; b_sh.cells = 0;
            if (TWO) { b_sh.pen[1].two = 1; b_sh.pen[1].o2 = 1 << 28; b_sh.pen[1].e2 = 1; }
            b_sh.geom.brow = a.brow; b_sh.geom.ring_scope = a.ring_scope; b_sh.geom.ring_hot = a.ring_hot;
            b_sh.geom.bbase_jobs = a.bbase_jobs; b_sh.geom.hist_w = a.hist_w; b_sh.geom.hist_levels = a.hist_levels;
            b_sh.geom.hist_stride = (unsigned)a.bbase_jobs * (unsigned)a.hist_w;
            b_sh.geom.urow = (unsigned)(a.bring_wg_stride - (size_t)a.brow);
        }
        __syncthreads();
    }
    const SrPen pen = a.pen;
    SrPen open_ = a.ori;
    if (TWO) { open_.two = 1; open_.o2 = 1 << 28; open_.e2 = 1; }
    const int scope = pen.scope, nsm = pen.scope + 1;
    const int gap_opening = TWO ? max(pen.o1, pen.o2) : pen.o1;
    for (;;) {
        if (tid == 0) {
            b_sh.pair = (int)atomicAdd(a.queue_head, 1u);
            b_sh.err = 0; b_sh.cig_cnt = 0; b_sh.score_acc = 0;
        }
        __syncthreads();
        int pair = RFL(b_sh.pair);
        if (pair >= (int)a.npairs) break;
        if (a.order) pair = (int)a.order[pair];
        const uint32_t q = a.pair_q[pair], t = a.pair_t[pair];
        const int plen = (int)a.seqlen[q], tlen = (int)a.seqlen[t];
        const int pw = SR_SEQ_WORDS(plen), tw = SR_SEQ_WORDS(tlen);
        uint32_t *Pf = lds_seq, *Pr = lds_seq + a.max_words, *Tt = lds_seq + 2 * (size_t)a.max_words;
        load_seq_lds<NT>(Pf, (GP<const uint32_t>)a.seqwords + a.word_off_fwd[q] - 1, pw);
        load_seq_lds<NT>(Pr, (GP<const uint32_t>)a.seqwords + a.word_off_rc[q] - 1, pw);
        load_seq_lds<NT>(Tt, (GP<const uint32_t>)a.seqwords + a.word_off_fwd[t] - 1, tw);
        GP<uint32_t> ops = (GP<uint32_t>)a.cigar_ops + a.cigar_base[pair];
        const uint32_t cap = (uint32_t)(a.cigar_base[pair + 1] - a.cigar_base[pair]);
        const unsigned long long tk0 = __builtin_amdgcn_s_memrealtime();
        // ---------------- orientation: forward and reverse-complement query as two aligners of one pass.
        // Forward wins ties; the reverse complement is chosen iff it reaches the end at a strictly lower score.
        int fwd = -1, rev = INT_MAX, is_rev = 0;
        if (tid == 0) {
            b_sh.offT = 2 * (int)a.max_words + 1;
            const int w = bjob_width(plen, tlen);
            bjob_set(0, 0, 0, plen, 0, tlen, 0, SR_C_M, SR_C_M, 0, 1);
            bjob_set(1, w, 0, plen, 0, tlen, 0, SR_C_M, SR_C_M, 0, (int)a.max_words + 1);
            b_sh.njobs = 2;
        }
        __syncthreads();
        {
            const long long smax = (long long)a.ori.o1 * 2 + (long long)a.ori.e1 * (plen + tlen) + 64;
            for (int s = 0;; s++) {
                BRows<OT> r;
                brows_ring<OT, TWO>(r, bring, a, open_, s, false);
                bfs_pass<OT, TWO, NT>(r, s, open_, 2, s & 1);
                __syncthreads();
                steps += 2;
                const bool rf = RFL(b_sh.jreach[s & 1][0]) != 0, rr = RFL(b_sh.jreach[s & 1][1]) != 0;
                if (rf) { fwd = s; break; }
                if (rr) { rev = s; is_rev = 1; break; }
                if (s > smax) { if (tid == 0) b_sh.err |= SR_DEV_ERR_SCORE_BOUND; break; }
            }
        }
        const int poff = is_rev ? (int)a.max_words + 1 : 1;
        const unsigned long long tk1 = __builtin_amdgcn_s_memrealtime();
        t_ori += tk1 - tk0;
        // ---------------- ordered segment list, breadth-first breakpoint search
        GP<int> cur = lists, nxt = lists + (size_t)SR_BFS_MAXSEG * SR_BFS_SEGREC;
        if (tid == 0) {
            cur[SL_PB] = 0; cur[SL_PE] = plen; cur[SL_TB] = 0; cur[SL_TE] = tlen; cur[SL_CB] = SR_C_M; cur[SL_CE] = SR_C_M;
            const int rem = (a.mem_mode == 3) ? INT_MAX : -1;
            cur[SL_REM] = rem; cur[SL_KIND] = seg_kind(plen, tlen, rem);
            b_sh.list_n = 1;
        }
        __syncthreads();
        for (;;) {                                           // one iteration per recursion level
            const int n_cur = RFL(b_sh.list_n);
            bool any_bp = false;
            int pos = 0;
            while (pos < n_cur && RFL(b_sh.err) == 0) {      // chunks of <= SR_BFS_MAXACT segments
                __syncthreads();
                if (tid == 0) {
                    int na = 0, p = pos, base = 0;
                    for (; p < n_cur && na < SR_BFS_MAXACT; p++) {
                        GP<int> e = cur + (size_t)p * SR_BFS_SEGREC;
                        if (e[SL_KIND] != SK_BP) continue;
                        BSeg &sg = b_sh.seg[na];
                        sg.pb = e[SL_PB]; sg.pe = e[SL_PE]; sg.tb = e[SL_TB]; sg.te = e[SL_TE]; sg.cb = e[SL_CB]; sg.ce = e[SL_CE];
                        sg.score_f = sg.score_r = 0; sg.last_fwd = 0; sg.f_ak = sg.r_ak = 0; sg.phase = 1;
                        const int sp = sg.pe - sg.pb, st = sg.te - sg.tb;
                        sg.max_ad = sp + st - 1; sg.bp_score = INT_MAX; sg.list_pos = p;
                        const int w = bjob_width(sp, st);
                        bjob_set(2 * na, base, sg.pb, sg.pe, sg.tb, sg.te, 0, sg.cb, -1, na, poff); base += w;
                        bjob_set(2 * na + 1, base, sg.pb, sg.pe, sg.tb, sg.te, 1, sg.ce, -1, na, poff); base += w;
                        na++;
                    }
                    b_sh.nact = na; b_sh.next_pos = p; b_sh.njobs = 2 * na; b_sh.nrunning = na;
                }
                __syncthreads();
                const int nact = RFL(b_sh.nact);
                pos = RFL(b_sh.next_pos);
                if (nact == 0) break;
                any_bp = true;
                nbp += (unsigned long long)nact;
                const unsigned long long tb0 = __builtin_amdgcn_s_memrealtime();
                const int njobs = 2 * nact;
                for (int s = 0; RFL(b_sh.nrunning) > 0; s++) {
                    BRows<OT> r;
                    const unsigned long long q0 = __builtin_amdgcn_s_memrealtime();
                    brows_ring<OT, TWO>(r, bring, a, pen, s, true);
                    bfs_pass<OT, TWO, NT>(r, s, pen, njobs, s & 1);
                    const unsigned long long q1 = __builtin_amdgcn_s_memrealtime();
                    __syncthreads();
                    const unsigned long long q2 = __builtin_amdgcn_s_memrealtime();
                    tq_pass += q1 - q0; tq_bar += q2 - q1;
                    steps += (unsigned long long)njobs;
                    // per-aligner max antidiagonal of this level; per-segment phase-1 control (one thread each)
                    if (tid < njobs) b_sh.mak[tid][s % nsm] = b_sh.jak[s & 1][tid];
                    if (tid < nact) {
                        BSeg &sg = b_sh.seg[tid];
                        if (sg.phase == 1) {
                            const int akf = b_sh.jak[s & 1][2 * tid], akr = b_sh.jak[s & 1][2 * tid + 1];
                            const long long smax = 2LL * ((long long)pen.o1 * 2 + (long long)pen.e1 * (sg.max_ad + 1)) + 1024;
                            if (s == 0) {
                                sg.f_ak = akf; sg.r_ak = akr;
                                if (sg.f_ak + sg.r_ak >= sg.max_ad) sg.phase = 2;
                            } else {
                                sg.score_f = s; sg.f_ak = akf; sg.last_fwd = 1;
                                if (sg.f_ak + sg.r_ak >= sg.max_ad) sg.phase = 2;
                                else {
                                    sg.score_r = s; sg.r_ak = akr; sg.last_fwd = 0;
                                    if ((long long)sg.score_f + sg.score_r > smax) sg.phase = 4;
                                    else if (sg.f_ak + sg.r_ak >= sg.max_ad) sg.phase = 2;
                                }
                            }
                        }
                    }
                    __syncthreads();
                    const unsigned long long q3 = __builtin_amdgcn_s_memrealtime();
                    tq_ctl += q3 - q2;
                    // phase 2 (overlap rounds) is cooperative: one segment after the other
                    for (int sa = 0; sa < nact; sa++) {
                        if (RFL(b_sh.seg[sa].phase) != 2) continue;
                        int score_f = RFL(b_sh.seg[sa].score_f), score_r = RFL(b_sh.seg[sa].score_r);
                        const int last_fwd = RFL(b_sh.seg[sa].last_fwd);
                        int ph = 2;
                        if (last_fwd) {
                            const int min_score_r = (score_r > scope - 1) ? score_r - (scope - 1) : 0;
                            if (score_f + min_score_r - gap_opening >= RFL(b_sh.seg[sa].bp_score)) ph = 3;
                            else {
                                bfs_overlap<OT, TWO, NT>(bring, sa, 0, score_f, score_r, 1);
                                ++score_r;
                            }
                        }
                        if (ph == 2) {
                            const int min_score_f = (score_f > scope - 1) ? score_f - (scope - 1) : 0;
                            if (min_score_f + score_r - gap_opening >= RFL(b_sh.seg[sa].bp_score)) ph = 3;
                            else {
                                bfs_overlap<OT, TWO, NT>(bring, sa, 1, score_r, score_f, 0);
                                ++score_f;
                                const long long smax = 2LL * ((long long)pen.o1 * 2 + (long long)pen.e1 * (RFL(b_sh.seg[sa].max_ad) + 1)) + 1024;
                                if ((long long)score_f + score_r > smax) ph = 4;
                            }
                        }
                        __syncthreads();
                        if (tid == 0) {
                            BSeg &sg = b_sh.seg[sa];
                            sg.score_f = score_f; sg.score_r = score_r; sg.last_fwd = 1; sg.phase = ph;
                        }
                        __syncthreads();
                    }
                    if (tid == 0) {
                        int run = 0;
                        for (int sa = 0; sa < nact; sa++) {
                            const int ph = b_sh.seg[sa].phase;
                            if (ph == 1 || ph == 2) run++;
                            else { b_sh.job[2 * sa].active = 0; b_sh.job[2 * sa + 1].active = 0; }
                        }
                        b_sh.nrunning = run;
                    }
                    const unsigned long long q4 = __builtin_amdgcn_s_memrealtime();
                    __syncthreads();
                    tq_ph2 += q4 - q3; tq_tail += __builtin_amdgcn_s_memrealtime() - q4;
                    npass++;
                }
                // results into the list records
                if (tid < nact) {
                    BSeg &sg = b_sh.seg[tid];
                    GP<int> e = cur + (size_t)sg.list_pos * SR_BFS_SEGREC;
                    const int sp = sg.pe - sg.pb, st = sg.te - sg.tb;
                    const int bh = sg.bp_off_f, bv = sg.bp_off_f - sg.bp_k_f;
                    if (sg.phase != 3 || sg.bp_score == INT_MAX) atomicOr(&b_sh.err, SR_DEV_ERR_SCORE_BOUND);
                    else if (bv < 0 || bv > sp || bh < 0 || bh > st) atomicOr(&b_sh.err, SR_DEV_ERR_BREAKPOINT);
                    else { e[SL_BV] = bv; e[SL_BH] = bh; e[SL_BCOMP] = sg.bp_comp; e[SL_BSF] = sg.bp_score_f; e[SL_BSR] = sg.bp_score_r; }
                }
                __syncthreads();
                t_bp += __builtin_amdgcn_s_memrealtime() - tb0;
            }
            __syncthreads();
            if (!any_bp || RFL(b_sh.err) != 0) break;
            // next level: every searched segment is replaced (in order) by its two halves
            if (tid == 0) {
                int m = 0;
                for (int p = 0; p < n_cur; p++) {
                    GP<int> e = cur + (size_t)p * SR_BFS_SEGREC;
                    if (e[SL_KIND] != SK_BP) {
                        if (m >= SR_BFS_MAXSEG) { b_sh.err |= SR_DEV_ERR_STACK; break; }
                        GP<int> d = nxt + (size_t)m * SR_BFS_SEGREC;
                        for (int f = 0; f < 8; f++) d[f] = e[f];
                        m++;
                    } else {
                        if (m + 2 > SR_BFS_MAXSEG) { b_sh.err |= SR_DEV_ERR_STACK; break; }
                        const int bv = e[SL_BV], bh = e[SL_BH], bc = e[SL_BCOMP];
                        GP<int> h0 = nxt + (size_t)m * SR_BFS_SEGREC, h1 = nxt + (size_t)(m + 1) * SR_BFS_SEGREC;
                        h0[SL_PB] = e[SL_PB]; h0[SL_PE] = e[SL_PB] + bv; h0[SL_TB] = e[SL_TB]; h0[SL_TE] = e[SL_TB] + bh;
                        h0[SL_CB] = e[SL_CB]; h0[SL_CE] = bc; h0[SL_REM] = e[SL_BSF];
                        h0[SL_KIND] = seg_kind(bv, bh, e[SL_BSF]);
                        h1[SL_PB] = e[SL_PB] + bv; h1[SL_PE] = e[SL_PE]; h1[SL_TB] = e[SL_TB] + bh; h1[SL_TE] = e[SL_TE];
                        h1[SL_CB] = bc; h1[SL_CE] = e[SL_CE]; h1[SL_REM] = e[SL_BSR];
                        h1[SL_KIND] = seg_kind(e[SL_PE] - e[SL_PB] - bv, e[SL_TE] - e[SL_TB] - bh, e[SL_BSR]);
                        m += 2;
                    }
                }
                b_sh.list_n = m;
            }
            __syncthreads();
            { GP<int> tmp = cur; cur = nxt; nxt = tmp; }
        }
        // ---------------- leaves in order: trivial ones are emitted directly, base cases in batches
        const unsigned long long tc0 = __builtin_amdgcn_s_memrealtime();
        {
            const int n_cur = RFL(b_sh.list_n);
            if (tid == 0) b_sh.emit_pos = 0;
            __syncthreads();
            int pos = 0;
            while (pos < n_cur && RFL(b_sh.err) == 0) {
                __syncthreads();
                if (tid == 0) {
                    int nb = 0, p = pos;
                    for (; p < n_cur && nb < a.bbase_jobs; p++) {
                        GP<int> e = cur + (size_t)p * SR_BFS_SEGREC;
                        if (e[SL_KIND] != SK_BASE) continue;
                        bjob_set(nb, nb * a.hist_w, e[SL_PB], e[SL_PE], e[SL_TB], e[SL_TE], 0, e[SL_CB], e[SL_CE], nb, poff);
                        b_sh.job[nb].shift = a.hist_w / 2;
                        b_sh.base_entry[nb] = p; b_sh.base_score[nb] = -1;
                        nb++;
                    }
                    b_sh.nbase = nb; b_sh.next_pos = p; b_sh.njobs = nb; b_sh.nrunning = nb;
                }
                __syncthreads();
                const int nb = RFL(b_sh.nbase);
                pos = RFL(b_sh.next_pos);
                if (nb > 0) {
                    nbase += (unsigned long long)nb;
                    for (int s = 0; RFL(b_sh.nrunning) > 0; s++) {
                        if (s >= a.hist_levels) { if (tid == 0) b_sh.err |= SR_DEV_ERR_BASE_OVERFLOW; break; }
                        BRows<OT> r;
                        brows_hist<OT, TWO>(r, bhist, a, pen, s);
                        bfs_pass<OT, TWO, NT>(r, s, pen, nb, s & 1);
                        __syncthreads();
                        steps += (unsigned long long)RFL(b_sh.nrunning);
                        if (tid == 0) {
                            int run = 0;
                            for (int j = 0; j < nb; j++) {
                                if (!b_sh.job[j].active) continue;
                                if (b_sh.jreach[s & 1][j]) { b_sh.base_score[j] = s; b_sh.job[j].active = 0; }
                                else run++;
                            }
                            b_sh.nrunning = run;
                        }
                        __syncthreads();
                    }
                    __syncthreads();
                    // one thread per base case: backtrace into its reversed op buffer
                    if (tid < nb && RFL(b_sh.err) == 0) {
                        int n = 0;
                        const int e = bfs_backtrace<OT, TWO>(bhist, b_sh.geom.hist_stride, tid, b_sh.base_score[tid],
                                                             btbuf + (size_t)tid * SR_BFS_BTCAP, &n);
                        b_sh.bt_n[tid] = n;
                        if (e & ~SR_MIRROR_BT_TIE) atomicOr(&b_sh.err, e & ~SR_MIRROR_BT_TIE);      // (this kernel has no use for the tie bit)
                    }
                    __syncthreads();
                }
                // emit list entries [emit_pos, pos) in order
                if (tid == 0 && b_sh.err == 0) {
                    int err = 0, bj = 0;
                    uint32_t cnt = b_sh.cig_cnt;
                    for (int p = b_sh.emit_pos; p < pos; p++) {
                        GP<int> e = cur + (size_t)p * SR_BFS_SEGREC;
                        const int sp = e[SL_PE] - e[SL_PB], st = e[SL_TE] - e[SL_TB];
                        if (e[SL_KIND] == SK_TRIVIAL) {
                            if (st == 0) cig_append(ops, cnt, cap, SR_OP_D, sp, err);
                            else cig_append(ops, cnt, cap, SR_OP_I, st, err);
                        } else if (e[SL_KIND] == SK_BASE) {
                            GP<uint32_t> b = btbuf + (size_t)bj * SR_BFS_BTCAP;
                            for (int i = b_sh.bt_n[bj] - 1; i >= 0; i--)
                                cig_append(ops, cnt, cap, (int)(b[i] & 15u), (int)(b[i] >> 4), err);
                            bj++;
                        } else err |= SR_DEV_ERR_BACKTRACE;
                    }
                    b_sh.cig_cnt = cnt; b_sh.emit_pos = pos;
                    if (err) b_sh.err |= err;
                }
                __syncthreads();
            }
        }
        t_base += __builtin_amdgcn_s_memrealtime() - tc0;
        // ---------------- score of the final CIGAR, outputs
        __syncthreads();
        const uint32_t cnt = RFL(b_sh.cig_cnt);
        int part = 0;
        for (uint32_t i = tid; i < cnt; i += NT) {
            const uint32_t op = ops[i] & 15u; const int len = (int)(ops[i] >> 4);
            if (op == SR_OP_X) part += len * pen.x;
            else if (op == SR_OP_I || op == SR_OP_D) {
                int g = pen.o1 + pen.e1 * len;
                if (TWO) g = min(g, pen.o2 + pen.e2 * len);
                part += g;
            }
        }
        if (part) atomicAdd(&b_sh.score_acc, part);
        __syncthreads();
        if (tid == 0) {
            a.is_reverse[pair] = is_rev ? 1 : 0;
            a.score[pair] = b_sh.err ? -1 : b_sh.score_acc;
            a.ori_fwd[pair] = fwd; a.ori_rev[pair] = rev;
            a.cigar_cnt[pair] = b_sh.err ? 0u : cnt;
            if (b_sh.err) atomicOr(a.error_flag, b_sh.err);
        }
        __syncthreads();
        t_all += __builtin_amdgcn_s_memrealtime() - tk0;
    }
    if (tid == 0) {
        atomicAdd(&a.counters[0], b_sh.cells);
        atomicAdd(&a.counters[1], steps);
        atomicAdd(&a.counters[2], nbase);
        atomicAdd(&a.counters[3], nbp);
        atomicAdd(&a.counters[6], t_ori);
        atomicAdd(&a.counters[7], t_bp);
        atomicAdd(&a.counters[8], t_base);
        atomicAdd(&a.counters[10], t_all);
        atomicAdd(&a.counters[9], npass);
        atomicAdd(&a.counters[11], tq_pass);
        atomicAdd(&a.counters[12], tq_bar);
        atomicAdd(&a.counters[13], tq_ctl);
        atomicAdd(&a.counters[14], tq_ph2);
        atomicAdd(&a.counters[15], tq_tail);
    }
}

#endif  // !SR_BLK_TU