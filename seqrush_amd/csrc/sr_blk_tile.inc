// sr_blk_tile.inc -- blocked kernel (sr_align_blk.inc), part 2: one wave tile of a block of levels -- the 32-bit tile
// (blk_tile), the packed 16-bit tile (blk_tile16) and the dispatch between them (blk_tile_any).
// one wave, one tile of aligner jid: levels s0 .. s0+B-1 of KGeo<B>::OWN owned groups
// IDONLY: recompute pass -- only the I/D chains of the block (M comes from the stored rows of older levels, the
// block's own M rows exist already); tix = index of the aligner's range tables (jid, or BJ_MAX + 0/1).
// X, OE1 (exact-penalty instance, X = mismatch, OE1 = o1 + e1, B == OE1 <= o2 + e2): a block is twice as deep as the
// mismatch distance, so M[s - x] of the block's later levels is the lane's own M of x levels earlier (registers), and
// the rows M[s0-x .. s0-1] that feed the first x levels are the same rows levels x.. read as M[s - o1 - e1]: 26 row
// loads + 16 row stores per 10 levels instead of 2 x (21 + 12).  The M[s - o2 - e2] rows are prefetched three
// levels ahead instead of all up front (registers).  X = 0: generic instance, B <= min(x, o1+e1, o2+e2).
template <typename OT, bool TWO, int B, int E1, int E2, bool IDONLY = false, int X = 0, int OE1 = 0, typename ST = OT>
__device__ __forceinline__ void blk_tile(const KRows<OT, ST> &R, const int s0, const int slot0, const SrPen &pen,
                                         const int jid, const int ti, const int tix, unsigned &row_ld, unsigned &row_st) {
    constexpr int N1 = E1 < B ? E1 : B, N2 = E2 < B ? E2 : B;
    constexpr bool XK = X > 0;
    static_assert(!XK || (B == OE1 && X <= B), "exact-penalty instance: block depth == o1 + e1 >= x");
    constexpr int HL = KGeo<B>::HL, OWN = KGeo<B>::OWN;
    constexpr int PF = XK ? 3 : B;                        // prefetch distance of the M[s - o2 - e2] rows
    const int lane = threadIdx.x & 63;
    const BJob &jb = b_sh.job[jid];
    const int base = RFL(jb.base), shift = RFL(jb.shift), plen = RFL(jb.plen), tlen = RFL(jb.tlen);
    const int p0 = RFL(jb.p0), t0 = RFL(jb.t0), begin = RFL(jb.begin);
    const int chk = RFL(jb.chk), kend = RFL(jb.kend), poff = RFL(jb.poff), toff = RFL(jb.pad0);
    const bool rec = IDONLY || RFL(jb.pad2) != 0;             // store every I/D row (phase 2 / base case / recompute)
    const int glo = RFL(k_sh.jglo[tix]), ghi = RFL(k_sh.jghi[tix]);
    const int g = glo + ti * OWN + lane - HL;
    const bool owned = (lane >= HL) && (lane < 64 - HL) && (g <= ghi);
    const int k0 = (g << 2) - shift;
    const unsigned idx0 = klane(R, (unsigned)(base + (g << 2)));      // lane part of the row addresses
    const LP P = (LP)(lds_seq + poff), T = (LP)(lds_seq + toff);
    // symbol index (LDS-wide: 16 / 8 / 4 symbols per word from LDS address 0) of P[p0 - k0] and T[t0]
    const int cp0 = p0 - k0 + (int)(((uint32_t)(uintptr_t)P >> 2) << SR_WIN_LOG);
    const int ct0 = t0 + (int)(((uint32_t)(uintptr_t)T >> 2) << SR_WIN_LOG);
    const KAdr A = kadr(R, jb, slot0);
#define KROW(LVL, C) krow_rel(R, A, s0, (LVL), (C))
    // ---- every source row of the block that older blocks wrote: one load per row and lane
    V4<OT> Lmx[XK ? 1 : B], Lmo1[B], Lmo2[B], Li1[N1], Ld1[N1], Li2[N2], Ld2[N2];
#pragma unroll
    for (int j = 0; j < B; j++) {
        if (!IDONLY && !XK) Lmx[XK ? 0 : j] = rld<OT>(R, KROW(s0 + j - pen.x, SR_C_M), idx0);
        // (exact instance: rows s0-x .. s0-1 double as the M[s-x] source of levels 0 .. x-1, so no last-use hint there)
        Lmo1[j] = rld<OT>(R, KROW(s0 + j - pen.o1 - E1, SR_C_M), idx0);
        if (TWO && j < PF) Lmo2[j] = rld_nt<OT>(R, KROW(s0 + j - pen.o2 - E2, SR_C_M), idx0);   // last use of that M level
    }
#pragma unroll
    for (int j = 0; j < N1; j++) {
        Li1[j] = rld_nt<OT>(R, KROW(s0 + j - E1, SR_C_I1), idx0);      // chain sources: read once
        Ld1[j] = rld_nt<OT>(R, KROW(s0 + j - E1, SR_C_D1), idx0);
    }
    if (TWO) {
#pragma unroll
        for (int j = 0; j < N2; j++) {
            Li2[j] = rld_nt<OT>(R, KROW(s0 + j - E2, SR_C_I2), idx0);
            Ld2[j] = rld_nt<OT>(R, KROW(s0 + j - E2, SR_C_D2), idx0);
        }
    }
    // U row (breakpoint detection filter): running max of the aligner's M offsets per diagonal
    // (kept only while the search stores its I/D rows, i.e. in phase 2; the recompute pass builds it from the
    // stored M rows of the scope window -- a superset bound of the window is all the filter needs)
    const bool with_u = (chk < 0) && (R.urow != 0u) && rec;
    {   // row traffic of this tile in 8-byte (int16) / 16-byte (int32) lane accesses: the kernel's algorithmic HBM bytes
        // (bench.py roofline): every lane of the wave loads, the owned lanes store
        const int nown = min(OWN, max(0, ghi - (glo + ti * OWN) + 1));
        int nld = ((!IDONLY && !XK) ? B : 0) + (IDONLY ? B : 0) + B + (TWO ? B : 0) + 2 * N1 + (TWO ? 2 * N2 : 0) + ((with_u && s0 > 0) ? 1 : 0);
        int nst = (IDONLY ? 0 : B) + (with_u ? 1 : 0);
#pragma unroll
        for (int j = 0; j < B; j++) {
            nst += (j + E1 >= B || rec) ? 2 : 0;
            if (TWO) nst += (j + E2 >= B || rec) ? 2 : 0;
        }
        row_ld += 64u * (unsigned)nld * (unsigned)(sizeof(ST) / 2); row_st += (unsigned)nown * (unsigned)nst * (unsigned)(sizeof(ST) / 2);
    }
    int uacc[4] = {NULLV, NULLV, NULLV, NULLV};
    V4<OT> Lown[IDONLY ? B : 1];                           // recompute pass: the block's own (stored) M rows
    if (IDONLY) {
#pragma unroll
        for (int j = 0; j < B; j++) Lown[IDONLY ? j : 0] = rld<OT>(R, KROW(s0 + j, SR_C_M), idx0);
    }
    if (with_u) {
        const int gplo = RFL(k_sh.jgplo[tix]), gphi = RFL(k_sh.jgphi[tix]);
        if (s0 > 0 && g >= gplo && g <= gphi) {
            const V4<OT> u = rld<OT>(R, R.urow, idx0);
#pragma unroll
            for (int q = 0; q < 4; q++) uacc[q] = (int)u[q];
        }
    }
    // Every negative offset is NULL to every reader (bounds, >= 0 tests, maxima); the cells computed here use -16, an
    // inline constant of the ISA, instead of materialising SR_NULL_OFF (-8192, the value of the NULL rows) per select.
#define KNULL (-16)
#define KBND(C, L1) (((unsigned)(C) >= (L1)) ? KNULL : (C))      // L1 = bound + 1, or 0: nothing is a cell
    int hI1[B][4], hD1[B][4], hI2[B][4], hD2[B][4];      // I/D cells of this block's levels (chain sources)
    int mvh[XK ? B : 1][4];                              // exact instance: this lane's M cells of the block's levels
#pragma unroll
    for (int j = 0; j < B; j++) {
        const int s = s0 + j;
        const int klo = RFL(k_sh.jklo[j][tix]), khi = RFL(k_sh.jkhi[j][tix]);
        if (TWO && XK && j + PF < B) Lmo2[j + PF < B ? j + PF : 0] = rld_nt<OT>(R, KROW(s0 + j + PF - pen.o2 - E2, SR_C_M), idx0);
        int mx[4], mo1[4], mo2[4], si1[4], sd1[4], si2[4], sd2[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            if (IDONLY) mx[q] = NULLV;
            else if (!XK) mx[q] = (int)Lmx[XK ? 0 : j][q];
            else if (j >= X) mx[q] = mvh[(XK && j >= X) ? j - X : 0][q];                    // own M, x levels earlier
            else mx[q] = (int)Lmo1[(XK && j + OE1 - X < B) ? j + OE1 - X : 0][q];           // row s0 + j - x
            mo1[q] = (int)Lmo1[j][q];
            if (j < N1) { si1[q] = (int)Li1[j < N1 ? j : 0][q]; sd1[q] = (int)Ld1[j < N1 ? j : 0][q]; }
            else { si1[q] = hI1[j >= E1 ? j - E1 : 0][q]; sd1[q] = hD1[j >= E1 ? j - E1 : 0][q]; }
            mo2[q] = si2[q] = sd2[q] = NULLV;
            if (TWO) {
                mo2[q] = (int)Lmo2[j][q];
                if (j < N2) { si2[q] = (int)Li2[j < N2 ? j : 0][q]; sd2[q] = (int)Ld2[j < N2 ? j : 0][q]; }
                else { si2[q] = hI2[j >= E2 ? j - E2 : 0][q]; sd2[q] = hD2[j >= E2 ? j - E2 : 0][q]; }
            }
        }
        const int mo1L = lane_left(mo1[3]), mo1R = lane_right(mo1[0]);
        const int i1L = lane_left(si1[3]), d1R = lane_right(sd1[0]);
        int mo2L = NULLV, mo2R = NULLV, i2L = NULLV, d2R = NULLV;
        if (TWO) { mo2L = lane_left(mo2[3]); mo2R = lane_right(mo2[0]); i2L = lane_left(si2[3]); d2R = lane_right(sd2[0]); }
        int mv[4], i1v[4], i2v[4], d1v[4], d2v[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int k = k0 + q;
            const bool inr = (k >= klo) && (k <= khi);
            int m, i1, i2 = KNULL, d1, d2 = KNULL;
            {
                // cells of diagonal k: 0 <= offset <= min(tlen, plen + k); outside the level's range: none
                const unsigned lim = inr ? (unsigned)(min(tlen, plen + k) + 1) : 0u;
                const int a1 = (q == 0) ? mo1L : mo1[q == 0 ? 0 : q - 1];
                const int b1 = (q == 0) ? i1L : si1[q == 0 ? 0 : q - 1];
                const int c1 = (q == 3) ? mo1R : mo1[q == 3 ? 3 : q + 1];
                const int f1 = (q == 3) ? d1R : sd1[q == 3 ? 3 : q + 1];
                i1 = KBND(max(a1, b1) + 1, lim);
                d1 = KBND(max(c1, f1), lim);
                if (TWO) {
                    const int a2 = (q == 0) ? mo2L : mo2[q == 0 ? 0 : q - 1];
                    const int b2 = (q == 0) ? i2L : si2[q == 0 ? 0 : q - 1];
                    const int c2 = (q == 3) ? mo2R : mo2[q == 3 ? 3 : q + 1];
                    const int f2 = (q == 3) ? d2R : sd2[q == 3 ? 3 : q + 1];
                    i2 = KBND(max(a2, b2) + 1, lim);
                    d2 = KBND(max(c2, f2), lim);
                }
                m = KBND(mx[q] + 1, lim);
                m = max(m, max(max(i1, i2), max(d1, d2)));
            }
            if (j == 0 && s0 == 0) {          // level 0: only the begin component's cell of diagonal 0 exists
                const int z = (inr && k == 0) ? 0 : KNULL;
                m = (begin == SR_C_M) ? z : KNULL; i1 = (begin == SR_C_I1) ? z : KNULL; i2 = (begin == SR_C_I2) ? z : KNULL;
                d1 = (begin == SR_C_D1) ? z : KNULL; d2 = (begin == SR_C_D2) ? z : KNULL;
            }
            mv[q] = m; i1v[q] = i1; i2v[q] = i2; d1v[q] = d1; d2v[q] = d2;
            hI1[j][q] = i1; hD1[j][q] = d1; hI2[j][q] = i2; hD2[j][q] = d2;
        }
        if (!IDONLY) {
        // ---- extension of the owned M cells.  Reverse aligners walk the reverse-complement copies
        // forward (equal bases <=> equal complements), so there is one code path; the first 16-base
        // window of the four cells is branch-free, longer runs continue in one predicated loop.
        // A cell at offset h of diagonal k compares P[p0 + h - k ..] with T[t0 + h ..]; at most L(k) - h symbols are left,
        // L = min(tlen, plen + k) the cell's limit.  The eight window reads of the level are in flight together; a cell
        // that does not extend (NULL, halo lane) reads wherever its coordinates point and adds nothing.
        int more = 0;
        if constexpr (sizeof(OT) == 2) {
            uint32_t pl[4], ph[4], tl[4], th[4];
            int sp[4], st[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                sp[q] = mv[q] + cp0 - q; st[q] = mv[q] + ct0;
                win_words(sp[q], pl[q], ph[q]); win_words(st[q], tl[q], th[q]);
            }
            asm volatile("; 8 windows in flight" : "+v"(pl[0]), "+v"(ph[0]), "+v"(pl[1]), "+v"(ph[1]), "+v"(pl[2]), "+v"(ph[2]), "+v"(pl[3]), "+v"(ph[3]),
                                                    "+v"(tl[0]), "+v"(th[0]), "+v"(tl[1]), "+v"(th[1]), "+v"(tl[2]), "+v"(th[2]), "+v"(tl[3]), "+v"(th[3]));
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const bool valid = owned && mv[q] >= 0;
                const int nn = valid ? min(tlen, plen + k0 + q) - mv[q] : 0;
                const uint32_t xw = __builtin_amdgcn_alignbit(ph[q], pl[q], (uint32_t)sp[q] << SR_SYM_LOG) ^
                                    __builtin_amdgcn_alignbit(th[q], tl[q], (uint32_t)st[q] << SR_SYM_LOG);
                mv[q] += (int)min3u(ffs_sym(xw), (unsigned)SR_WIN, (unsigned)nn);
                more |= (xw == 0u && nn > SR_WIN) ? (1 << q) : 0;
            }
        } else {
            // (32-bit rows: a row is four registers per lane, sixteen more for the windows of a level spill: cell by cell,
            // every coordinate of a cell that does not extend forced to the sequences' first symbols)
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const bool valid = owned && mv[q] >= 0;
                const int h = valid ? mv[q] : 0, v = valid ? mv[q] - (k0 + q) : 0;
                const int nn = valid ? min(plen - v, tlen - h) : 0;
                const uint32_t xw = win_fwd(P, p0 + v) ^ win_fwd(T, t0 + h);
                const unsigned z = (unsigned)(__ffs((int)xw) - 1) >> SR_SYM_LOG;          // 2^31-1 when the window is all equal
                mv[q] += (int)min(min(z, (unsigned)SR_WIN), (unsigned)nn);
                more |= (xw == 0u && nn > SR_WIN) ? (1 << q) : 0;
            }
        }
        // runs longer than a window: the wave iterates, skipping the cell positions q no lane needs
        unsigned long long pend[4];
#pragma unroll
        for (int q = 0; q < 4; q++) pend[q] = __ballot((more >> q) & 1);
        while ((pend[0] | pend[1] | pend[2] | pend[3]) != 0ull) {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                if (pend[q] == 0ull) continue;
                if constexpr (sizeof(OT) == 2) {
                    const int nn = lanes_or_zero(pend[q], min(tlen, plen + k0 + q) - mv[q]);      // 0 for the lanes that are done
                    const uint32_t xw = win_sym(mv[q] + cp0 - q) ^ win_sym(mv[q] + ct0);
                    mv[q] += (int)min3u(ffs_sym(xw), (unsigned)SR_WIN, (unsigned)nn);
                    pend[q] = __ballot(xw == 0u && nn > SR_WIN);
                } else {
                    const bool on = (more >> q) & 1;
                    const int h = on ? mv[q] : 0, v = on ? mv[q] - (k0 + q) : 0;
                    const int nn = on ? min(plen - v, tlen - h) : 0;
                    const uint32_t xw = win_fwd(P, p0 + v) ^ win_fwd(T, t0 + h);
                    const unsigned z = (unsigned)(__ffs((int)xw) - 1) >> SR_SYM_LOG;
                    mv[q] += (int)min(min(z, (unsigned)SR_WIN), (unsigned)nn);
                    if (!(xw == 0u && nn > SR_WIN)) more &= ~(1 << q);
                    pend[q] = __ballot((more >> q) & 1);
                }
            }
        }
        int ak = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            if (XK) mvh[XK ? j : 0][q] = mv[q];
            ak = max(ak, (owned && mv[q] >= 0) ? 2 * mv[q] - (k0 + q) : 0);
            uacc[q] = max(uacc[q], mv[q]);
            if (j == 0 && s0 == 0) uacc[q] = max(uacc[q], max(max(i1v[q], i2v[q]), max(d1v[q], d2v[q])));
        }
        if (chk >= 0) {                       // score-only / base-case aligners: has the end cell been reached?
            bool reached = false;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int k = k0 + q;
                int val = mv[q];
                if (chk == SR_C_I1) val = i1v[q];
                else if (chk == SR_C_I2) val = i2v[q];
                else if (chk == SR_C_D1) val = d1v[q];
                else if (chk == SR_C_D2) val = d2v[q];
                reached |= owned && k == kend && k >= klo && k <= khi && val >= tlen;
            }
            if (reached) k_sh.jreach[j][jid] = 1;
        }
        ak = row16_max(ak);
        if ((lane & 15) == 15 && ak > 0) atomicMax(&k_sh.jak[j][jid], ak);
        } else {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                uacc[q] = max(uacc[q], (int)Lown[IDONLY ? j : 0][q]);
                if (j == 0 && s0 == 0) uacc[q] = max(uacc[q], max(max(i1v[q], i2v[q]), max(d1v[q], d2v[q])));
            }
        }
        if (owned) {
            V4<OT> oM, oI1, oI2, oD1, oD2;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                oM[q] = (OT)mv[q]; oI1[q] = (OT)i1v[q]; oI2[q] = (OT)i2v[q]; oD1[q] = (OT)d1v[q]; oD2[q] = (OT)d2v[q];
            }
            // The I/D rows of all but the block's last e levels are read again only by breakpoint detection: a
            // search in phase 1 does not store them at all (rec == 0); when it enters phase 2 the rows of the scope
            // window are recomputed from the M rows (blk_recompute) and from then on stored (streaming).
            if (!IDONLY) rst<OT>(R, KROW(s, SR_C_M), idx0, oM);
            if (j + E1 < B) { if (rec) { rst_nt<OT>(R, KROW(s, SR_C_I1), idx0, oI1); rst_nt<OT>(R, KROW(s, SR_C_D1), idx0, oD1); } }
            else { rst<OT>(R, KROW(s, SR_C_I1), idx0, oI1); rst<OT>(R, KROW(s, SR_C_D1), idx0, oD1); }
            if (TWO) {
                if (j + E2 < B) { if (rec) { rst_nt<OT>(R, KROW(s, SR_C_I2), idx0, oI2); rst_nt<OT>(R, KROW(s, SR_C_D2), idx0, oD2); } }
                else { rst<OT>(R, KROW(s, SR_C_I2), idx0, oI2); rst<OT>(R, KROW(s, SR_C_D2), idx0, oD2); }
            }
        }
    }
    if (with_u && owned) {
        V4<OT> u;
#pragma unroll
        for (int q = 0; q < 4; q++) u[q] = (OT)uacc[q];
        rst<OT>(R, R.urow, idx0, u);
    }
#undef KROW
#undef KBND
#undef KNULL
}

// ---- packed 16-bit tile (int16 rows) --------------------------------------------------------------------------
// Same tile, same rows, same results as blk_tile<short, ...>; the I/D chains, the M maximum, the limit tests and the
// histories stay in the rows' own format -- two 16-bit cells per register (v_pk_max_i16 / v_pk_add_u16 / ...) -- so a
// level costs half the chain instructions and none of the per-cell unpack / repack of the 32-bit version.  Only the
// extension (sequence comparison) and the antidiagonal maximum work on 32-bit cells.
//  * neighbours: the k-1 / k+1 cells of a register pair are one DPP lane shift + two v_alignbit.
//  * limit test: a cell above its limit L becomes NULL16 via sat(L - v) >> 15 (three instructions per pair); cells
//    outside the level's diagonal range get L = -32768, which sends every value there.  Negative inputs pass
//    through; every cell outside the range or beyond the matrix is reset to NULL16 at every level, so a NULL can only
//    creep upwards (+1 per chain step) through the few unreachable in-range cells of the first levels.
typedef short __attribute__((ext_vector_type(2))) H2;
struct Q4 { H2 a, b; };                                   // cells 0,1 | 2,3 of a lane's group
#define NULL16 0xC000C000u                                // (-16384, -16384)
__device__ __forceinline__ H2 h2_bits(uint32_t u) { return __builtin_bit_cast(H2, u); }
__device__ __forceinline__ uint32_t h2_u(H2 h) { return __builtin_bit_cast(uint32_t, h); }
__device__ __forceinline__ H2 h2_pack(int lo, int hi) { return h2_bits(((uint32_t)lo & 0xffffu) | ((uint32_t)hi << 16)); }
__device__ __forceinline__ H2 h2_pack_perm(int lo, int hi) { return h2_bits(__builtin_amdgcn_perm((uint32_t)hi, (uint32_t)lo, 0x05040100u)); }   // one v_perm_b32
__device__ __forceinline__ Q4 q4_from(V4<short> v) {
    Q4 r; r.a = __builtin_shufflevector(v, v, 0, 1); r.b = __builtin_shufflevector(v, v, 2, 3); return r;
}
__device__ __forceinline__ V4<short> q4_vec(Q4 q) { return __builtin_shufflevector(q.a, q.b, 0, 1, 2, 3); }
__device__ __forceinline__ Q4 q4_null() { Q4 r; r.a = h2_bits(NULL16); r.b = h2_bits(NULL16); return r; }
__device__ __forceinline__ Q4 q4_max(Q4 x, Q4 y) {
    Q4 r; r.a = __builtin_elementwise_max(x.a, y.a); r.b = __builtin_elementwise_max(x.b, y.b); return r;
}
__device__ __forceinline__ Q4 q4_inc(Q4 x) { const H2 one = {1, 1}; Q4 r; r.a = x.a + one; r.b = x.b + one; return r; }
// cell of diagonal k-1 for every cell of the group: [left lane's cell 3, c0, c1, c2]; k+1: [c1, c2, c3, right lane's cell 0]
__device__ __forceinline__ Q4 q4_from_left(Q4 x) {
    // (zero fill at the wave's ends: those lanes are halo, see KGeo)
    const uint32_t L = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)h2_u(x.b), 0x138, 0xf, 0xf, true);
    Q4 r;
    r.a = h2_bits(__builtin_amdgcn_alignbit(h2_u(x.a), L, 16));
    r.b = h2_bits(__builtin_amdgcn_alignbit(h2_u(x.b), h2_u(x.a), 16));
    return r;
}
__device__ __forceinline__ Q4 q4_from_right(Q4 x) {
    const uint32_t R = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)h2_u(x.a), 0x130, 0xf, 0xf, true);
    Q4 r;
    r.a = h2_bits(__builtin_amdgcn_alignbit(h2_u(x.b), h2_u(x.a), 16));
    r.b = h2_bits(__builtin_amdgcn_alignbit(R, h2_u(x.b), 16));
    return r;
}
template <uint32_t NUL = NULL16>
__device__ __forceinline__ Q4 q4_bound(Q4 v, Q4 L) {
    // (inline assembly: written as C the compiler turns the three instructions per register back into two 16-bit
    // compares and two selects, and between separate asm statements it pads with s_nop)
    uint32_t ta, tb, ra, rb;
    const uint32_t nul = NUL;
    asm("v_pk_sub_i16 %0, %4, %6 clamp\n\t"
        "v_pk_sub_i16 %1, %5, %7 clamp\n\t"
        "v_pk_ashrrev_i16 %0, 15, %0 op_sel_hi:[0,1]\n\t"
        "v_pk_ashrrev_i16 %1, 15, %1 op_sel_hi:[0,1]\n\t"
        "v_bfi_b32 %2, %0, %8, %6\n\t"
        "v_bfi_b32 %3, %1, %8, %7"
        : "=&v"(ta), "=&v"(tb), "=&v"(ra), "=&v"(rb)
        : "v"(h2_u(L.a)), "v"(h2_u(L.b)), "v"(h2_u(v.a)), "v"(h2_u(v.b)), "s"(nul));
    Q4 r; r.a = h2_bits(ra); r.b = h2_bits(rb);
    return r;
}
// cells below offset 0 (stored value < -BIAS) become exactly NULL again.  The packed chains let negatives pass (only "above
// the limit" is tested), and a NULL creeps: +1 per chain step, up to +17 per M step once the extension has run over it (its
// windows usually lie outside the LDS allocation, read 0 on both sides and "match" 16 symbols).  On diagonals that have run
// off the matrix nothing real ever overrides it again, so after thousands of levels a NULL would cross into the valid range
// (margin 16384 for int16 rows, 8192 for the 16-bit ring of 32-bit searches: ~4 800 / ~2 400 levels at 17 per 5 levels) and
// be extended, stored and tested for overlaps like a cell (round 4: found by the bounds-checked build -- an LDS window of a
// "live" cell 2 KB in front of the sequences -- on a 50 kb pair of score > 16 000; C5's mean score is 15 000).  Tiles of
// deep levels (`deep`, uniform) therefore reset, when they are loaded, the chain sources of the four gap components and the
// M[s - x] sources of the block's first x levels: the creep through THOSE sources is bounded by one block.  The gap-open
// sources -- Lmo1[0..4] (M[s - o1 - e1]) and every Lmo2[j] (M[s - o2 - e2]), the rows prefetched inside the level loop
// included -- are not reset, so a NULL can still creep through M -> I/D -> M across blocks (ADVICE.md round 4 estimates the
// valid range near level 6 600 / 3 300 from reading the code).  tests/test_deep_gpu.py runs one-sided gaps and unrelated pairs
// past those levels on both cell widths, production and bounds-checked build, against the oracle.
template <uint32_t NUL, int BIAS>
__device__ __forceinline__ Q4 q4_renull(Q4 v) {
    uint32_t ta, tb, ra, rb;
    const uint32_t nul = NUL;
    if constexpr (BIAS == 0) {
        asm("v_pk_ashrrev_i16 %0, 15, %4 op_sel_hi:[0,1]\n\t"
            "v_pk_ashrrev_i16 %1, 15, %5 op_sel_hi:[0,1]\n\t"
            "v_bfi_b32 %2, %0, %6, %4\n\t"
            "v_bfi_b32 %3, %1, %6, %5"
            : "=&v"(ta), "=&v"(tb), "=&v"(ra), "=&v"(rb)
            : "v"(h2_u(v.a)), "v"(h2_u(v.b)), "s"(nul));
    } else {
        const uint32_t bias2 = ((uint32_t)BIAS & 0xffffu) | ((uint32_t)BIAS << 16);
        asm("v_pk_add_i16 %0, %4, %7 clamp\n\t"
            "v_pk_add_i16 %1, %5, %7 clamp\n\t"
            "v_pk_ashrrev_i16 %0, 15, %0 op_sel_hi:[0,1]\n\t"
            "v_pk_ashrrev_i16 %1, 15, %1 op_sel_hi:[0,1]\n\t"
            "v_bfi_b32 %2, %0, %6, %4\n\t"
            "v_bfi_b32 %3, %1, %6, %5"
            : "=&v"(ta), "=&v"(tb), "=&v"(ra), "=&v"(rb)
            : "v"(h2_u(v.a)), "v"(h2_u(v.b)), "s"(nul), "v"(bias2));
    }
    Q4 r; r.a = h2_bits(ra); r.b = h2_bits(rb);
    return r;
}
#define SR_DEEP_INT16 3000         // first level whose tiles reset creeping NULLs: int16 rows (creep <= 3.4 per level: 10 200 of the 16 384 margin)
#define SR_DEEP_RING16 1500        // ... the 16-bit ring of 32-bit searches (5 100 of 8 192)
__device__ __forceinline__ int q4_get(Q4 x, int q) {       // q compile-time
    return (q == 0) ? (int)x.a.x : (q == 1) ? (int)x.a.y : (q == 2) ? (int)x.b.x : (int)x.b.y;
}

// KR / BIAS: the rows' container and what a stored cell is short of its offset -- KRows<short>, 0: int16 searches;
// KRows<int, uint16_t>, SR_RING_BIAS: the 16-bit ring of a 32-bit search (cell = offset - 24576, NULL = -32768; round 4:
// C5's ring tiles ran the 32-bit tile with a conversion at every load and store).  Everything packed works on the stored
// values; what looks at an offset -- limits, window addresses, validity, the antidiagonal -- carries the bias as a constant.
template <bool TWO, int B, int E1, int E2, bool IDONLY = false, int X = 0, int OE1 = 0, bool RING = false, typename KR = KRows<short>, int BIAS = 0>
__device__ __forceinline__ void blk_tile16(const KR &R, const int s0, const int slot0, const SrPen &pen,
                                           const int jid, const int ti, const int tix, unsigned &row_ld, unsigned &row_st) {
    typedef short OT;
    typedef short ST;
    static_assert(BIAS == 0 || (RING && X > 0 && B % 10 == 0), "the biased tile exists for ring rows with immediate addressing only");
    constexpr uint32_t NUL = BIAS ? 0x80008000u : NULL16;          // two NULL cells
    constexpr int NULC = BIAS ? -32768 : -16384;                  // one NULL cell
    const Q4 nulq = {h2_bits(NUL), h2_bits(NUL)};
    constexpr int N1 = E1 < B ? E1 : B, N2 = E2 < B ? E2 : B;
    constexpr bool XK = X > 0;
    static_assert(!XK || (B == OE1 && X <= B), "exact-penalty instance: block depth == o1 + e1 >= x");
    constexpr int HL = KGeo<B>::HL, OWN = KGeo<B>::OWN;
    constexpr int PF = XK ? 3 : B;
    const int lane = threadIdx.x & 63;
    const BJob &jb = b_sh.job[jid];
    const int base = RFL(jb.base), p0 = RFL(jb.p0), t0 = RFL(jb.t0), poff = RFL(jb.poff), toff = RFL(jb.pad0);
    const int shift = RFL(jb.shift), plen = RFL(jb.plen), tlen = RFL(jb.tlen), begin = RFL(jb.begin);
    const int chk = RFL(jb.chk), kend = RFL(jb.kend);
    const bool rec = IDONLY || RFL(jb.pad2) != 0;
    const int glo = RFL(k_sh.jglo[tix]), ghi = RFL(k_sh.jghi[tix]);
    const int g = glo + ti * OWN + lane - HL;
    const bool owned = (lane >= HL) && (lane < 64 - HL) && (g <= ghi);
    const int k0 = (g << 2) - shift;
    const unsigned idx0 = klane(R, (unsigned)(base + (g << 2)));      // lane part of the row addresses
    const LP P = (LP)(lds_seq + poff), T = (LP)(lds_seq + toff);
    const KAdr A = kadr(R, jb, slot0);
#define KROW(LVL, C) krow_rel(R, A, s0, (LVL), (C))
#define LDQ(LVL, C) q4_from(rld<OT>(R, KROW((LVL), (C)), idx0))
#define LDQ_NT(LVL, C) q4_from(rld_nt<OT>(R, KROW((LVL), (C)), idx0))
    // immediate-offset addressing (see kbase): ring rows of the exact instance whose second gap piece sits a multiple of
    // five levels back (the host sends other penalties to the generic instance)
    constexpr bool IMMR = RING && XK && (B % 10 == 0);
    const unsigned lane_b = idx0 * (unsigned)sizeof(ST);
    // bases (uniform): the block below (its M rows feed levels 0..9 as M[s - o1 - e1] and 0..x-1 as M[s - x]), the two
    // five-level runs of M[s - o2 - e2], the chain-source rows of the four gap components, this block's rows
    GPB bM1 = nullptr, bM2a = nullptr, bM2b = nullptr, bI1 = nullptr, bD1 = nullptr, bI2 = nullptr, bD2 = nullptr;
    GPB sM = nullptr, sI1 = nullptr, sD1 = nullptr, sI2 = nullptr, sD2 = nullptr;
    if constexpr (IMMR) {
        const int oe2 = pen.o2 + E2;
        bM1 = kbase(R, s0 - B < 0 ? R.nuloff + KBLK_C * 256u : KROW(s0 - B + KBLK_C, SR_C_M));
        bM2a = kbase(R, KROW(s0 - oe2, SR_C_M)); bM2b = kbase(R, KROW(s0 - oe2 + 5, SR_C_M));
        bI1 = kbase(R, KROW(s0 - E1, SR_C_I1)); bD1 = kbase(R, KROW(s0 - E1, SR_C_D1));
        bI2 = kbase(R, KROW(s0 - E2, SR_C_I2)); bD2 = kbase(R, KROW(s0 - E2, SR_C_D2));
        sM = kbase(R, KROW(s0 + KBLK_C, SR_C_M));
        sI1 = kbase(R, KROW(s0 + KBLK_C, SR_C_I1)); sD1 = kbase(R, KROW(s0 + KBLK_C, SR_C_D1));
        sI2 = kbase(R, KROW(s0 + KBLK_C, SR_C_I2)); sD2 = kbase(R, KROW(s0 + KBLK_C, SR_C_D2));
    }
    // TIGHT coverage (kwindow): lanes outside the coverage of a source block would read cells nobody wrote -> they hold NULL
    // instead and -- round 4b -- do not load at all.  The source blocks: s0 - B (M[s - o1 - e1] / M[s - x] rows and the chain
    // sources) and the blocks the two five-level runs of M[s - o2 - e2] come from; blocks below level 0 are the NULL rows.
    // Coverages are nested (older = narrower): a tile whose 64 lanes lie inside the oldest one (`msk == false`, most tiles
    // of a wide search) loads every lane as before; an edge tile loads under the lanes' masks -- the last tile of an
    // aligner covers half a tile's groups on average, and its other lanes' loads were 12 % of the kernel's row bytes.
    constexpr bool TIGHT = IMMR && (BIAS ? true : (bool)KTIGHT_OF(short, short, B, X));
    bool msk = false, in10 = true, in2a = true, in2b = true;
    if constexpr (TIGHT) {
        const int oe2 = TWO ? pen.o2 + E2 : B;
        const int l2a = s0 - oe2, l2b = s0 - oe2 + 5;                                      // first levels of the two runs (multiples of 5)
        const int b2a = l2a >= 0 ? (l2a / B) * B : -1, b2b = l2b >= 0 ? (l2b / B) * B : -1;      // their blocks (-1: NULL rows)
        int lo10 = INT_MIN / 2, hi10 = INT_MAX / 2, lo2a = lo10, hi2a = hi10, lo2b = lo10, hi2b = hi10;
        if (s0 - B >= 0) kwindow<TWO, B, E1, E2, true>(pen, jb, s0 - B, lo10, hi10);
        if (TWO && b2a >= 0) kwindow<TWO, B, E1, E2, true>(pen, jb, b2a, lo2a, hi2a);
        if (TWO && b2b >= 0) kwindow<TWO, B, E1, E2, true>(pen, jb, b2b, lo2b, hi2b);
        lo10 = RFL(lo10); hi10 = RFL(hi10); lo2a = RFL(lo2a); hi2a = RFL(hi2a); lo2b = RFL(lo2b); hi2b = RFL(hi2b);
        in10 = g >= lo10 && g <= hi10; in2a = g >= lo2a && g <= hi2a; in2b = g >= lo2b && g <= hi2b;
        msk = __builtin_amdgcn_ballot_w64(!(in10 && in2a && in2b)) != 0ull;
    }
    Q4 Lmx[XK ? 1 : B], Lmo1[B], Lmo2[B], Li1[N1], Ld1[N1], Li2[N2], Ld2[N2];
    unsigned ld_lanes10 = 64u, ld_lanes2 = 64u;              // lanes that load from block s0 - B / from the first M[s - o2 - e2] rows (byte count)
    if (TIGHT && msk) {
        // edge tile: NULL everywhere, loads under the lanes' masks
#pragma unroll
        for (int j = 0; j < B; j++) { Lmo1[j] = nulq; Lmo2[j] = nulq; }
#pragma unroll
        for (int j = 0; j < N1; j++) { Li1[j] = nulq; Ld1[j] = nulq; }
#pragma unroll
        for (int j = 0; j < N2; j++) { Li2[j] = nulq; Ld2[j] = nulq; }
        if constexpr (IMMR) {
            if (in10) {
#pragma unroll
                for (int j = 0; j < B; j++) Lmo1[j] = q4_from(ild<OT, ST>(R, bM1, lane_b, j - KBLK_C));
#pragma unroll
                for (int j = 0; j < N1; j++) { Li1[j] = q4_from(ild_nt<OT, ST>(R, bI1, lane_b, j)); Ld1[j] = q4_from(ild_nt<OT, ST>(R, bD1, lane_b, j)); }
                if (TWO) {
#pragma unroll
                    for (int j = 0; j < N2; j++) { Li2[j] = q4_from(ild_nt<OT, ST>(R, bI2, lane_b, j)); Ld2[j] = q4_from(ild_nt<OT, ST>(R, bD2, lane_b, j)); }
                }
            }
            if (TWO && in2a) {                                // (PF = 3 < 5: the first rows all come from the first run)
#pragma unroll
                for (int j = 0; j < PF && j < 5; j++) Lmo2[j] = q4_from(ild_nt<OT, ST>(R, bM2a, lane_b, j));
            }
        }
        ld_lanes10 = (unsigned)__popcll(__builtin_amdgcn_ballot_w64(in10)); ld_lanes2 = (unsigned)__popcll(__builtin_amdgcn_ballot_w64(in2a));
    } else {
#pragma unroll
    for (int j = 0; j < B; j++) {
        if constexpr (!IDONLY && !XK) Lmx[XK ? 0 : j] = LDQ(s0 + j - pen.x, SR_C_M);
        if constexpr (IMMR) {
            Lmo1[j] = q4_from(ild<OT, ST>(R, bM1, lane_b, j - KBLK_C));
            if (TWO && j < PF) Lmo2[j] = q4_from(ild_nt<OT, ST>(R, j < 5 ? bM2a : bM2b, lane_b, j < 5 ? j : j - 5));
        } else {
            Lmo1[j] = LDQ(s0 + j - pen.o1 - E1, SR_C_M);
            if (TWO && j < PF) Lmo2[j] = LDQ_NT(s0 + j - pen.o2 - E2, SR_C_M);
        }
    }
#pragma unroll
    for (int j = 0; j < N1; j++) {
        if constexpr (IMMR) {
            Li1[j] = q4_from(ild_nt<OT, ST>(R, bI1, lane_b, j)); Ld1[j] = q4_from(ild_nt<OT, ST>(R, bD1, lane_b, j));
        } else {
            Li1[j] = LDQ_NT(s0 + j - E1, SR_C_I1);
            Ld1[j] = LDQ_NT(s0 + j - E1, SR_C_D1);
        }
    }
    if (TWO) {
#pragma unroll
        for (int j = 0; j < N2; j++) {
            if constexpr (IMMR) {
                Li2[j] = q4_from(ild_nt<OT, ST>(R, bI2, lane_b, j)); Ld2[j] = q4_from(ild_nt<OT, ST>(R, bD2, lane_b, j));
            } else {
                Li2[j] = LDQ_NT(s0 + j - E2, SR_C_I2);
                Ld2[j] = LDQ_NT(s0 + j - E2, SR_C_D2);
            }
        }
    }
    }
    const bool with_u = (chk < 0) && (R.urow != 0u) && rec;
    {   // row traffic of this tile (see blk_tile): lane accesses really made
        const int nown = min(OWN, max(0, ghi - (glo + ti * OWN) + 1));
        const int n10 = ((!IDONLY && !XK) ? B : 0) + B + 2 * N1 + (TWO ? 2 * N2 : 0);          // rows of block s0 - B (and M[s - x] rows of the generic instance)
        const int n2f = TWO ? (PF < B ? PF : B) : 0, n2p = TWO ? B - n2f : 0;                    // M[s - o2 - e2]: first rows, rows prefetched inside the level loop (all lanes)
        int nst = (IDONLY ? 0 : B) + (with_u ? 1 : 0);
#pragma unroll
        for (int j = 0; j < B; j++) {
            nst += (j + E1 >= B || rec) ? 2 : 0;
            if (TWO) nst += (j + E2 >= B || rec) ? 2 : 0;
        }
        row_ld += ld_lanes10 * (unsigned)n10 + ld_lanes2 * (unsigned)n2f + 64u * (unsigned)(n2p + (IDONLY ? B : 0) + ((with_u && s0 > 0) ? 1 : 0));
        row_st += (unsigned)nown * (unsigned)nst;
    }
    Q4 uacc = nulq;
    Q4 Lown[IDONLY ? B : 1];
    if (IDONLY) {
#pragma unroll
        for (int j = 0; j < B; j++) {
            if constexpr (IMMR) Lown[IDONLY ? j : 0] = q4_from(ild<OT, ST>(R, sM, lane_b, j - KBLK_C));
            else Lown[IDONLY ? j : 0] = LDQ(s0 + j, SR_C_M);
        }
    }
    if (with_u) {
        const int gplo = RFL(k_sh.jgplo[tix]), gphi = RFL(k_sh.jgphi[tix]);
        if (s0 > 0 && g >= gplo && g <= gphi) uacc = q4_from(rld_raw16(R, R.urow, idx0));
    }
    // deep levels: creeping NULLs are reset (q4_renull) where a block takes its chains up -- the M[s - x] sources of the
    // block's first levels and the gap chains' sources -- under ONE uniform branch per tile (nothing per level: the
    // level code is not duplicated).  Through these sources an M chain creeps at most two steps (34) and a gap chain ten
    // before the next reset; the gap-open sources (Lmo1[0..4], every Lmo2[j]) pass unreset (see q4_renull).
    const bool deep = s0 >= (BIAS ? SR_DEEP_RING16 : SR_DEEP_INT16);
    if (deep) {
#pragma unroll
        for (int j = 0; j < B; j++) {
            if (XK) { if (j + OE1 - X < B && j + OE1 - X >= 0 && j < X) Lmo1[(XK && j + OE1 - X < B) ? j + OE1 - X : 0] = q4_renull<NUL, BIAS>(Lmo1[(XK && j + OE1 - X < B) ? j + OE1 - X : 0]); }
            else if (!IDONLY) Lmx[XK ? 0 : j] = q4_renull<NUL, BIAS>(Lmx[XK ? 0 : j]);
        }
#pragma unroll
        for (int j = 0; j < N1; j++) { Li1[j] = q4_renull<NUL, BIAS>(Li1[j]); Ld1[j] = q4_renull<NUL, BIAS>(Ld1[j]); }
        if (TWO) {
#pragma unroll
            for (int j = 0; j < N2; j++) { Li2[j] = q4_renull<NUL, BIAS>(Li2[j]); Ld2[j] = q4_renull<NUL, BIAS>(Ld2[j]); }
        }
    }
    // limits of the lane's four diagonals: 0 <= offset <= min(tlen, plen + k), none when that is negative
    Q4 Lb;
    {
        int l[4];
#pragma unroll
        for (int q = 0; q < 4; q++) l[q] = max(min(tlen, plen + k0 + q), -1) - BIAS;
        Lb.a = h2_pack(l[0], l[1]); Lb.b = h2_pack(l[2], l[3]);
    }
    // symbol index (LDS-wide: 16 / 8 / 4 symbols per word from LDS address 0) of P[p0 - k0] and T[t0]
    // (a stored cell is offset - BIAS: the constants carry the bias)
    const int cp0 = p0 - k0 + BIAS + (int)(((uint32_t)(uintptr_t)P >> 2) << SR_WIN_LOG);
    const int ct0 = t0 + BIAS + (int)(((uint32_t)(uintptr_t)T >> 2) << SR_WIN_LOG);
    // the same as bit indices, per cell of the lane (P: cell q sits on diagonal k0 + q), and the owned lanes as a mask
    const int cpb0 = cp0 << SR_SYM_LOG, cpb1 = (cp0 - 1) << SR_SYM_LOG, cpb2 = (cp0 - 2) << SR_SYM_LOG, cpb3 = (cp0 - 3) << SR_SYM_LOG;
    const int ctb = ct0 << SR_SYM_LOG;
    const unsigned long long ownb = __builtin_amdgcn_ballot_w64(owned);
    Q4 kk;                                               // the lane's diagonals
    kk.a = h2_pack(k0, k0 + 1); kk.b = h2_pack(k0 + 2, k0 + 3);
    // the ranges of a block's levels are nested (level 0 the narrowest): a tile inside level 0's range needs no range masks.
    // (Base cases, never ring tiles: a level's range is forward range x backward cone, blk_setup -- the forward side widens
    // with the level, the cone side narrows, so the intersection of the block's ranges is that of its first and last level.)
    int klo0 = RFL(k_sh.jklo[0][tix]), khi0 = RFL(k_sh.jkhi[0][tix]);
    if constexpr (!RING) { klo0 = max(klo0, RFL(k_sh.jklo[B - 1][tix])); khi0 = min(khi0, RFL(k_sh.jkhi[B - 1][tix])); }
    const bool inside = __builtin_amdgcn_ballot_w64(!(k0 >= klo0 && k0 + 3 <= khi0)) == 0ull;
    Q4 hI1[B], hD1[B], hI2[B], hD2[B], mvh[XK ? B : 1];
#pragma unroll
    for (int j = 0; j < B; j++) {
        const int s = s0 + j;
        int klo = 0, khi = 0;                              // (only edge tiles and base-case aligners look at the level's range)
        if (!inside || chk >= 0 || (j == 0 && s0 == 0)) { klo = RFL(k_sh.jklo[j][tix]); khi = RFL(k_sh.jkhi[j][tix]); }
        if (TWO && XK && j + PF < B) {
            if constexpr (IMMR) Lmo2[j + PF < B ? j + PF : 0] = q4_from(ild_nt<OT, ST>(R, j + PF < 5 ? bM2a : bM2b, kopaque_v(lane_b), j + PF < 5 ? j + PF : j + PF - 5));
            else Lmo2[j + PF < B ? j + PF : 0] = LDQ_NT(s0 + j + PF - pen.o2 - E2, SR_C_M);
        }
        if (TIGHT && TWO && msk && j >= PF) {            // (the row prefetched PF levels ago, used by this level: same mask as the first ones)
            const bool in_ = j < 5 ? in2a : in2b;
            const Q4 nq = nulq;
            Lmo2[j].a = in_ ? Lmo2[j].a : nq.a; Lmo2[j].b = in_ ? Lmo2[j].b : nq.b;
        }
        const unsigned lane_j = IMMR ? kopaque_v(lane_b) : 0u;
        Q4 Lj = Lb;
        if (!inside) {
            int l[4];
#pragma unroll
            for (int q = 0; q < 4; q++) { const int k = k0 + q; l[q] = (k >= klo && k <= khi) ? q4_get(Lb, q) : -32768; }
            Lj.a = h2_pack(l[0], l[1]); Lj.b = h2_pack(l[2], l[3]);
        }
        Q4 mx, mo1 = Lmo1[j], si1, sd1, mo2 = nulq, si2 = nulq, sd2 = nulq;
        if (IDONLY) mx = nulq;
        else if (!XK) mx = Lmx[XK ? 0 : j];
        else if (j >= X) mx = mvh[(XK && j >= X) ? j - X : 0];
        else mx = Lmo1[(XK && j + OE1 - X < B) ? j + OE1 - X : 0];
        if (j < N1) { si1 = Li1[j < N1 ? j : 0]; sd1 = Ld1[j < N1 ? j : 0]; }
        else { si1 = hI1[j >= E1 ? j - E1 : 0]; sd1 = hD1[j >= E1 ? j - E1 : 0]; }
        if (TWO) {
            mo2 = Lmo2[j];
            if (j < N2) { si2 = Li2[j < N2 ? j : 0]; sd2 = Ld2[j < N2 ? j : 0]; }
            else { si2 = hI2[j >= E2 ? j - E2 : 0]; sd2 = hD2[j >= E2 ? j - E2 : 0]; }
        }
        Q4 i1 = q4_bound<NUL>(q4_inc(q4_from_left(q4_max(mo1, si1))), Lj);
        Q4 d1 = q4_bound<NUL>(q4_from_right(q4_max(mo1, sd1)), Lj);
        Q4 i2 = nulq, d2 = nulq;
        if (TWO) {
            i2 = q4_bound<NUL>(q4_inc(q4_from_left(q4_max(mo2, si2))), Lj);
            d2 = q4_bound<NUL>(q4_from_right(q4_max(mo2, sd2)), Lj);
        }
        Q4 m = q4_bound<NUL>(q4_inc(mx), Lj);
        m = TWO ? q4_max(m, q4_max(q4_max(i1, i2), q4_max(d1, d2))) : q4_max(m, q4_max(i1, d1));
        if (j == 0 && s0 == 0) {              // level 0: only the begin component's cell of diagonal 0 exists
            int z[4];
#pragma unroll
            for (int q = 0; q < 4; q++) { const int k = k0 + q; z[q] = (k == 0 && k >= klo && k <= khi) ? -BIAS : NULC; }
            // (selects on the 32-bit halves: a conditional on the struct would go through the stack)
            const H2 za = h2_pack(z[0], z[1]), zb = h2_pack(z[2], z[3]), nh = h2_bits(NUL);
            m.a = (begin == SR_C_M) ? za : nh; m.b = (begin == SR_C_M) ? zb : nh;
            i1.a = (begin == SR_C_I1) ? za : nh; i1.b = (begin == SR_C_I1) ? zb : nh;
            i2.a = (begin == SR_C_I2) ? za : nh; i2.b = (begin == SR_C_I2) ? zb : nh;
            d1.a = (begin == SR_C_D1) ? za : nh; d1.b = (begin == SR_C_D1) ? zb : nh;
            d2.a = (begin == SR_C_D2) ? za : nh; d2.b = (begin == SR_C_D2) ? zb : nh;
        }
        hI1[j] = i1; hD1[j] = d1; hI2[j] = i2; hD2[j] = d2;
        if (!IDONLY) {
            int mv[4];
#pragma unroll
            for (int q = 0; q < 4; q++) mv[q] = q4_get(m, q);
            // A cell at offset h of diagonal k compares P[p0 + h - k ..] with T[t0 + h ..]; at most L(k) - h symbols are
            // left, L the cell's limit.  Cells that do not extend (NULL, halo lanes) run through the same code: their
            // addresses may lie anywhere (LDS reads outside the allocation return 0), a NULL stays far below 0 when a
            // window's worth is added to it, and only the "longer than a window" flag is masked.
            // The eight window reads of a level (two per cell) are issued together and waited for once: taken cell by
            // cell the compiler serialises read - wait - use, eight exposed LDS round trips per level.
            // Round 3: a window is addressed by its LDS-wide BIT index = cell * 2^SR_SYM_LOG + constant, one v_mad_i32_i16
            // straight from the packed cell (it is the read address >> 3 and v_alignbit's shift at once); "longer than a
            // window" is ext == SR_WIN (a cell with exactly SR_WIN symbols left takes one idle turn of the loop below).
            unsigned long long pend[4];
            {
                uint32_t pl[4], ph[4], tl[4], th[4];
                int bp[4], bt[4];
                const uint32_t mwa = h2_u(m.a), mwb = h2_u(m.b);
                bp[0] = bit_index<0>(mwa, cpb0); bp[1] = bit_index<1>(mwa, cpb1); bp[2] = bit_index<0>(mwb, cpb2); bp[3] = bit_index<1>(mwb, cpb3);
                bt[0] = bit_index_u<0>(mwa, ctb); bt[1] = bit_index_u<1>(mwa, ctb); bt[2] = bit_index_u<0>(mwb, ctb); bt[3] = bit_index_u<1>(mwb, ctb);
#ifdef SR_BOUNDS
                {   // live cells (owned, offset >= 0, within their limit) must read their windows inside the staged sequences
                    const unsigned lo_ = (unsigned)(uintptr_t)lds_seq;
                    const unsigned seq_hi = lo_ + RFL(k_sh.lds_seq_bytes);
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const int mvq = q4_get(m, q);
                        if (owned && mvq >= -BIAS && mvq <= q4_get(Lb, q)) {
                            const unsigned ap = ((unsigned)bp[q] >> 3) & ~3u, at = ((unsigned)bt[q] >> 3) & ~3u;
                            if (ap < lo_ || ap + 8u > seq_hi) kbnd_fail(3u, ap, seq_hi);
                            if (at < lo_ || at + 8u > seq_hi) kbnd_fail(3u, at, seq_hi);
                        }
                    }
                }
#endif
#pragma unroll
                for (int q = 0; q < 4; q++) { win_words_bit(bp[q], pl[q], ph[q]); win_words_bit(bt[q], tl[q], th[q]); }
                asm volatile("; 8 windows in flight" : "+v"(pl[0]), "+v"(ph[0]), "+v"(pl[1]), "+v"(ph[1]), "+v"(pl[2]), "+v"(ph[2]), "+v"(pl[3]), "+v"(ph[3]),
                                                        "+v"(tl[0]), "+v"(th[0]), "+v"(tl[1]), "+v"(th[1]), "+v"(tl[2]), "+v"(th[2]), "+v"(tl[3]), "+v"(th[3]));
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int nn = q4_get(Lb, q) - mv[q];
                    const uint32_t xw = __builtin_amdgcn_alignbit(ph[q], pl[q], (uint32_t)bp[q]) ^
                                        __builtin_amdgcn_alignbit(th[q], tl[q], (uint32_t)bt[q]);
                    const int ext_ = (int)min3u(ffs_sym(xw), (unsigned)SR_WIN, (unsigned)nn);
                    mv[q] += ext_;
                    // (one ballot per compare: a ballot of `a && b` goes through a 0 / 1 register and a third compare)
                    pend[q] = __builtin_amdgcn_ballot_w64(ext_ == SR_WIN) & __builtin_amdgcn_ballot_w64(mv[q] >= -BIAS) & ownb;
                }
            }
            // runs longer than a window: the wave iterates, skipping the cell positions q no lane needs
            while ((pend[0] | pend[1] | pend[2] | pend[3]) != 0ull) {
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    if (pend[q] == 0ull) continue;
                    const int nn = lanes_or_zero(pend[q], q4_get(Lb, q) - mv[q]);      // 0 for the lanes that are done
                    const uint32_t xw = win_sym(mv[q] + cp0 - q) ^ win_sym(mv[q] + ct0);
                    mv[q] += (int)min3u(ffs_sym(xw), (unsigned)SR_WIN, (unsigned)nn);
                    pend[q] = __builtin_amdgcn_ballot_w64(xw == 0u && nn > SR_WIN);
                }
            }
            m.a = h2_pack_perm(mv[0], mv[1]); m.b = h2_pack_perm(mv[2], mv[3]);
            if (XK) mvh[XK ? j : 0] = m;
            // max antidiagonal 2h - k of the lane's valid cells (<= plen + tlen < 2^16: unsigned 16-bit lanes; the biased tile
            // serves sequences up to 57 k: 32-bit there)
            int ak;
            if constexpr (BIAS == 0) {
                typedef unsigned short __attribute__((ext_vector_type(2))) U2;
                const uint32_t va = ~h2_u(m.a >> (H2){15, 15}), vb = ~h2_u(m.b >> (H2){15, 15});
                const uint32_t aa = h2_u(m.a + m.a - kk.a) & va, ab = h2_u(m.b + m.b - kk.b) & vb;
                const uint32_t mx2 = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(U2, aa), __builtin_bit_cast(U2, ab)));
                ak = owned ? (int)max(mx2 >> 16, mx2 & 0xffffu) : 0;
            } else {
                ak = 0;
#pragma unroll
                for (int q = 0; q < 4; q++) ak = max(ak, mv[q] >= -BIAS ? 2 * (mv[q] + BIAS) - (k0 + q) : 0);
                ak = owned ? ak : 0;
            }
            uacc = q4_max(uacc, m);
            if (j == 0 && s0 == 0) uacc = TWO ? q4_max(uacc, q4_max(q4_max(i1, i2), q4_max(d1, d2))) : q4_max(uacc, q4_max(i1, d1));
            if (chk >= 0) {                   // score-only / base-case aligners: has the end cell been reached?
                const int qe = kend - k0;                                   // the end diagonal's cell of this lane, if any
                if (owned && qe >= 0 && qe < 4 && kend >= klo && kend <= khi) {
                    const uint32_t wa = (chk == SR_C_I1) ? h2_u(i1.a) : (chk == SR_C_I2) ? h2_u(i2.a) : (chk == SR_C_D1) ? h2_u(d1.a)
                                      : (chk == SR_C_D2) ? h2_u(d2.a) : h2_u(m.a);
                    const uint32_t wb = (chk == SR_C_I1) ? h2_u(i1.b) : (chk == SR_C_I2) ? h2_u(i2.b) : (chk == SR_C_D1) ? h2_u(d1.b)
                                      : (chk == SR_C_D2) ? h2_u(d2.b) : h2_u(m.b);
                    const uint32_t w = (qe & 2) ? wb : wa;
                    const int val = (int)(short)((qe & 1) ? (w >> 16) : (w & 0xffffu));
                    if (val + BIAS >= tlen) k_sh.jreach[j][jid] = 1;
                }
            }
            ak = row16_max_nn(ak);
            if ((lane & 15) == 15 && ak > 0) atomicMax(&k_sh.jak[j][jid], ak);
        } else {
            uacc = q4_max(uacc, Lown[IDONLY ? j : 0]);
            if (j == 0 && s0 == 0) uacc = TWO ? q4_max(uacc, q4_max(q4_max(i1, i2), q4_max(d1, d2))) : q4_max(uacc, q4_max(i1, d1));
        }
        if (owned) {
            if constexpr (IMMR) {
                const int im = j - KBLK_C;
                const bool l1 = j + E1 >= B, l2 = j + E2 >= B;       // the block's last e levels: chain sources of the next block
                if (!IDONLY) ist<OT, ST>(R, sM, lane_j, im, q4_vec(m));
                if (l1) { ist<OT, ST>(R, sI1, lane_j, im, q4_vec(i1)); ist<OT, ST>(R, sD1, lane_j, im, q4_vec(d1)); }
                if (TWO && l2) { ist<OT, ST>(R, sI2, lane_j, im, q4_vec(i2)); ist<OT, ST>(R, sD2, lane_j, im, q4_vec(d2)); }
                if (rec && (!l1 || (TWO && !l2))) {
                    const unsigned lane_r = kopaque_v(lane_b);           // (own block: see kopaque_v)
                    if (!l1) { ist_nt<OT, ST>(R, sI1, lane_r, im, q4_vec(i1)); ist_nt<OT, ST>(R, sD1, lane_r, im, q4_vec(d1)); }
                    if (TWO && !l2) { ist_nt<OT, ST>(R, sI2, lane_r, im, q4_vec(i2)); ist_nt<OT, ST>(R, sD2, lane_r, im, q4_vec(d2)); }
                }
            } else {
            if (!IDONLY) rst<OT>(R, KROW(s, SR_C_M), idx0, q4_vec(m));
            if (j + E1 < B) { if (rec) { rst_nt<OT>(R, KROW(s, SR_C_I1), idx0, q4_vec(i1)); rst_nt<OT>(R, KROW(s, SR_C_D1), idx0, q4_vec(d1)); } }
            else { rst<OT>(R, KROW(s, SR_C_I1), idx0, q4_vec(i1)); rst<OT>(R, KROW(s, SR_C_D1), idx0, q4_vec(d1)); }
            if (TWO) {
                if (j + E2 < B) { if (rec) { rst_nt<OT>(R, KROW(s, SR_C_I2), idx0, q4_vec(i2)); rst_nt<OT>(R, KROW(s, SR_C_D2), idx0, q4_vec(d2)); } }
                else { rst<OT>(R, KROW(s, SR_C_I2), idx0, q4_vec(i2)); rst<OT>(R, KROW(s, SR_C_D2), idx0, q4_vec(d2)); }
            }
            }
        }
    }
    if (with_u && owned) rst_raw16(R, R.urow, idx0, q4_vec(uacc));
#undef KROW
#undef LDQ
#undef LDQ_NT
}

// tile dispatch: int16 rows of the blocked instances take the packed tile
template <typename OT, bool TWO, int B, int E1, int E2, bool IDONLY, int X, int OE1, typename ST = OT, bool RING = false>
__device__ __forceinline__ void blk_tile_any(const KRows<OT, ST> &R, const int s0, const int slot0, const SrPen &pen,
                                             const int jid, const int ti, const int tix, unsigned &row_ld, unsigned &row_st) {
    // (round 2 kept the packed tile off the generic 5-level instance: built with it, a workgroup's second pair failed in most
    // builds, blamed on LDS reads outside the LDS.  Round 3: such reads return 0 and leave nothing behind
    // (profiles/r03_lds_oob.log), and neither today's source nor the round-2 source rebuilt without the address wrap
    // reproduces the failure -- 53 parity tests incl. several pairs per workgroup pass; enabled, DESIGN 4.1)
    if constexpr (sizeof(OT) == 2 && (X > 0 || B >= 5)) blk_tile16<TWO, B, E1, E2, IDONLY, X, OE1, RING>(R, s0, slot0, pen, jid, ti, tix, row_ld, row_st);
    // 32-bit search, 16-bit ring (C5): the packed tile on the rows as stored
    else if constexpr (KPK_U16_OF(OT, ST, B, X) && RING) blk_tile16<TWO, B, E1, E2, IDONLY, X, OE1, true, KRows<OT, ST>, SR_RING_BIAS>(R, s0, slot0, pen, jid, ti, tix, row_ld, row_st);
    else blk_tile<OT, TWO, B, E1, E2, IDONLY, X, OE1>(R, s0, slot0, pen, jid, ti, tix, row_ld, row_st);
}
