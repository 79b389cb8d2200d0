// sr_blk_phase2.inc -- blocked kernel (sr_align_blk.inc), part 4: batched breakpoint detection of one pass (blk_phase2).
// ---- batched breakpoint detection ("phase 2") of one pass ------------------------------------
// Reference loop (oracle bialign_find_breakpoint, WFA2 wavefront_bialign.c), per segment:
//     if (last_fwd) { done-check; overlap(F@score_f vs R <= score_r); ++score_r; }
//     done-check; overlap(R@score_r vs F <= score_f); ++score_f; last_fwd = 1
// A block makes levels <= avail of both aligners available, so a segment runs the loop while
// score_f <= avail: at most 2B overlap calls per pass.  overlap() walks (i ascending, component in the
// order D2 I2 D1 I1 M), takes the smallest overlapping diagonal of each (i, component) and accepts it
// when score_0 + score_i - gap(component) is strictly below the running best; the accepted value
// depends on (i, component) only, so a call's outcome is its candidate with the smallest value,
// earliest in walk order among equals (then the smallest diagonal), if that is below the best so far.
// What a call can find does not depend on the running best, so all calls of all segments of the pass
// are evaluated together:
//   A  one thread per segment lists its calls
//   F  filter: diagonals whose M offset plus the other aligner's U bound (blk_tile keeps U = running
//      max of M per diagonal, a superset bound of the scope window) reaches tlen -> candidate list
//   E  candidates x scope levels: exact overlap test per component, 64-bit atomicMin of the packed
//      (value, walk order, diagonal) per call -- and of the key the transposed pair would form (pc_best_t)
//   W  one thread per segment replays the reference loop with the done-checks over the calls' results; an accepted
//      result whose two keys name different (component, diagonal) marks the pair tie-sensitive (k_sh.mir_tie).
template <typename OT, bool TWO, int NT, int B, int E1, int E2, typename ST = OT, bool PROF = false>
__device__ __forceinline__ void blk_phase2(const KRows<OT, ST> &RR, GP<uint32_t> clist, GP<int> gmak,
                                           const SrPen &pen, const int s0, const int nact, const int gap_opening) {
    const int depth = RR.depth;
    const int tid = threadIdx.x;
    const int avail = s0 + B - 1, scope = pen.scope;
    const int gapmax = gap_opening;
#define KR(S, C) krow_abs(RR, (S), (C))
    // k_sh.p2mask (written by the control section of wave 0): segments in phase 2; rounds of <= K_P2 of them
    for (;;) {
        const unsigned long long pmask = ((unsigned long long)RFL(k_sh.p2mask_hi) << 32) | (unsigned)RFL(k_sh.p2mask_lo);
        if (pmask == 0ull) break;
        __syncthreads();                                   // every wave has read the mask before wave 0 replaces it
        const int n2 = min(__popcll(pmask), K_P2);
        const unsigned long long tp0 = PROF ? __builtin_amdgcn_s_memrealtime() : 0ull;
        if (tid < 64) KPRIO_HI();                          // wave 0 lists the calls and the filter units alone
        if (tid < 64) {
            const bool mine = (pmask >> tid) & 1ull;
            const int rank = __popcll(pmask & ((1ull << tid) - 1ull));
            if (mine && rank < K_P2) k_sh.p2seg[rank] = tid;
            const unsigned long long rest = __ballot(mine && rank >= K_P2);      // next round
            if (tid == 0) { k_sh.p2mask_lo = (unsigned)rest; k_sh.p2mask_hi = (unsigned)(rest >> 32); k_sh.cl_n = 0; }
        }
        // ---- A: calls of each segment; filter units (segment, side)
        if (tid < n2) {
            const BSeg &sg = b_sh.seg[k_sh.p2seg[tid]];
            int n = 0, f = sg.score_f, r = sg.score_r, lf = sg.last_fwd;
#pragma unroll
            for (int j = 0; j < B; j++) { k_sh.pc_idx[tid][0][j] = -1; k_sh.pc_idx[tid][1][j] = -1; }
            while (f <= avail) {
                if (lf) {
                    k_sh.pc_side[tid][n] = 0; k_sh.pc_s1[tid][n] = r; k_sh.pc_best[tid][n] = ~0ull; k_sh.pc_best_t[tid][n] = ~0ull;
                    k_sh.pc_idx[tid][0][f - s0] = n; n++; r++;
                }
                k_sh.pc_side[tid][n] = 1; k_sh.pc_s1[tid][n] = f; k_sh.pc_best[tid][n] = ~0ull; k_sh.pc_best_t[tid][n] = ~0ull;
                k_sh.pc_idx[tid][1][r - s0] = n; n++; f++; lf = 1;
            }
            k_sh.pc_n[tid] = n;
        }
        if (tid < 64) {
            int ng = 0, glo = 0;
            if (tid < 2 * n2) {
                const int p = tid >> 1, side = tid & 1, sa = k_sh.p2seg[p];
                const BJob &b0 = b_sh.job[2 * sa + side];
                const int j0 = 2 * sa + side, j1 = 2 * sa + 1 - side, kinv = b0.tlen - b0.plen;
                const int lo = max(k_sh.jklo[B - 1][j0], kinv - k_sh.jkhi[B - 1][j1]);
                const int hi = min(k_sh.jkhi[B - 1][j0], kinv - k_sh.jklo[B - 1][j1]);
                if (hi >= lo) { glo = (lo + b0.shift) >> 2; ng = ((hi + b0.shift) >> 2) - glo + 1; }
            }
            int incl = ng;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(incl, o, 64); if (tid >= o) incl += v; }
            if (tid < 2 * K_P2) { k_sh.pu_glo[tid] = glo; k_sh.pu_start[tid + 1] = incl; k_sh.pu_kmin[tid] = INT_MAX; k_sh.pu_kmax[tid] = INT_MIN; }
            if (tid == 0) k_sh.pu_start[0] = 0;
            KPRIO_LO();
        }
        __syncthreads();
        const unsigned long long tp1 = PROF ? __builtin_amdgcn_s_memrealtime() : 0ull;
        // ---- F: filter
        {
            const int total = RFL(k_sh.pu_start[2 * n2]);
            if (tid == 0) { k_sh.dg_f += (unsigned long long)total; k_sh.dg_r += 1ull; }
            for (int it = tid; it < total; it += NT) {
                int lo = 0, hi = 2 * n2;
                while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (k_sh.pu_start[mid] <= it) lo = mid; else hi = mid; }
                const int unit = lo, p = unit >> 1, side = unit & 1, sa = k_sh.p2seg[p];
                const int j0 = 2 * sa + side, j1 = 2 * sa + 1 - side;
                const BJob &b0 = b_sh.job[j0];
                const BJob &b1 = b_sh.job[j1];
                const int tlen = b0.tlen, kinv = b0.tlen - b0.plen;
                const int g = k_sh.pu_glo[unit] + (it - k_sh.pu_start[unit]);
                const int k0 = (g << 2) - b0.shift;
                const unsigned idx0 = klane(RR, (unsigned)(b0.base + (g << 2)));
                const int klo1 = k_sh.jklo[B - 1][j1], khi1 = k_sh.jkhi[B - 1][j1];
                const int u1off = b1.base + b1.shift;
                // every load of the unit is issued before the first one is looked at: the block's M rows of the group
                // (all stored, whether a level has a call or not) and the other aligner's U cells
                V4<OT> mrows[B];
#pragma unroll
                for (int j = 0; j < B; j++) mrows[j] = rld<OT>(RR, KR(s0 + j, SR_C_M), idx0);
                int u1[4];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int k1 = kinv - (k0 + q);
                    const int uv = rcell<OT>(RR, RR.urow, u1off + min(max(k1, klo1), khi1));
                    u1[q] = (k1 >= klo1 && k1 <= khi1) ? uv : NULLV;
                }
#pragma unroll
                for (int j = 0; j < B; j++) {
                    const int ci = k_sh.pc_idx[p][side][j];
                    if (ci < 0) continue;
                    const int lvl = s0 + j;
                    const int klo0 = k_sh.jklo[j][j0], khi0 = k_sh.jkhi[j][j0];
                    int m0[4];
#pragma unroll
                    for (int q = 0; q < 4; q++) m0[q] = (int)mrows[j][q];
                    if (lvl == 0) {                        // the begin component need not be M
#pragma unroll
                        for (int c = 1; c < 5; c++) {
                            if (!TWO && (c == SR_C_I2 || c == SR_C_D2)) continue;
                            const V4<OT> x = rld<OT>(RR, KR(0, c), idx0);
#pragma unroll
                            for (int q = 0; q < 4; q++) m0[q] = max(m0[q], (int)x[q]);
                        }
                    }
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const int k = k0 + q;
                        if (k >= klo0 && k <= khi0 && m0[q] >= 0 && u1[q] >= 0 && m0[q] + u1[q] >= tlen) {
                            atomicMin(&k_sh.pu_kmin[unit], k); atomicMax(&k_sh.pu_kmax[unit], k);
                        }
                    }
                }
            }
        }
        __syncthreads();
        const unsigned long long tp2 = PROF ? __builtin_amdgcn_s_memrealtime() : 0ull;
        // ---- E: exact overlap tests.  One wave per (segment, side, 64 diagonals of the unit's band): lanes are adjacent
        // diagonals, so the cells of a (level, component) row are one coalesced access (the other aligner's run downwards).
        // The calls of a side are consecutive levels of its own aligner and their scope windows of the other aligner overlap
        // almost entirely, so the loops run over ABSOLUTE levels: five calls' own cells (5 x 5 registers) against blocks of
        // five levels of the other aligner (5 x 5 registers), every (call, level) pair inside a call's window tested from
        // registers -- one memory round trip per 125 (call, level, component) tests.  All skips are wave-uniform.  Diagonals
        // of the band that did not pass the filter at a call's level cannot pass here either (a component never exceeds
        // its level's M, an M never the U bound).
        {
            int mch = 0;                                        // most 64-diagonal chunks of a unit
            for (int u = 0; u < 2 * n2; u++) {
                const int a0 = RFL(k_sh.pu_kmin[u]), a1 = RFL(k_sh.pu_kmax[u]);
                if (a1 >= a0) mch = max(mch, (a1 - a0 + 64) >> 6);
            }
            const int total = 2 * n2 * mch, lane = tid & 63;
            if (tid == 0) { k_sh.dg_c += (unsigned long long)total; }
            for (int it = tid >> 6; it < total; it += NT / 64) {
                const int unit = it / mch, ch = it - unit * mch, p = unit >> 1, side = unit & 1;
                const int kmin = RFL(k_sh.pu_kmin[unit]), kmax = RFL(k_sh.pu_kmax[unit]);
                if (kmax < kmin || kmin + 64 * ch > kmax) continue;
                const int sa = RFL(k_sh.p2seg[p]);
                const int bp0 = RFL(b_sh.seg[sa].bp_score);
                const int j0 = 2 * sa + side, j1 = 2 * sa + 1 - side;
                const BJob &b0 = b_sh.job[j0];
                const BJob &b1 = b_sh.job[j1];
                const int plen = RFL(b0.plen), tlen = RFL(b0.tlen), beg0 = RFL(b0.begin), beg1 = RFL(b1.begin);
                const int off0 = RFL(b0.base) + RFL(b0.shift), off1 = RFL(b1.base) + RFL(b1.shift);
                const int k0 = kmin + 64 * ch + lane, k1 = tlen - plen - k0;
                const bool onb = k0 <= kmax;
                if (lane == 0) atomicAdd(&k_sh.dg_e, 1ull);
                for (int jb = 0; jb < B; jb += 5) {             // five levels of the own aligner = up to five calls
                    int cix[5], sc1[5];                         // call index (-1: the level has no call on this side), other aligner's level
                    int lmin = INT_MAX, lmax = INT_MIN;
#pragma unroll
                    for (int jj = 0; jj < 5; jj++) {
                        cix[jj] = (jb + jj < B) ? RFL((int)k_sh.pc_idx[p][side][jb + jj < B ? jb + jj : 0]) : -1;
                        sc1[jj] = cix[jj] >= 0 ? RFL(k_sh.pc_s1[p][cix[jj] >= 0 ? cix[jj] : 0]) : 0;
                        const int score_0 = s0 + jb + jj;
                        // levels of the other aligner this call can still accept something from
                        if (cix[jj] >= 0) {
                            const int lo_l = max(0, sc1[jj] - (scope - 1)), hi_l = min(sc1[jj], bp0 == INT_MAX ? INT_MAX : bp0 + gapmax - 1 - score_0);
                            if (hi_l >= lo_l) { lmin = min(lmin, lo_l); lmax = max(lmax, hi_l); }
                            else cix[jj] = -1;
                        }
                    }
                    if (lmax < lmin) continue;
                    int c0[5][5], ak0[5];
#pragma unroll
                    for (int jj = 0; jj < 5; jj++) {
                        const int score_0 = s0 + jb + jj;
                        const int R0 = kreach<TWO, E1, E2>(pen, score_0, beg0);
                        const bool on0 = onb && cix[jj] >= 0 && k0 >= max(-plen, -R0) && k0 <= min(tlen, R0);
                        ak0[jj] = cix[jj] >= 0 ? gmak[j0 * BFS_MAK_SLOTS + score_0 % depth] : 0;
#pragma unroll
                        for (int c = 0; c < 5; c++) {
                            c0[jj][c] = NULLV;
                            if (!TWO && (c == SR_C_I2 || c == SR_C_D2)) continue;
                            if (on0) c0[jj][c] = rcell<OT>(RR, KR(score_0, c), off0 + k0);
                        }
                    }
                    // Levels of the other aligner whose furthest antidiagonal cannot meet any of these calls' own levels hold no
                    // overlap: one lane per level of the window looks its max_ak up, the ballot is the set of levels worth
                    // loading (round 3: at first contact that is the top few of the 26 + 4; their rows were all loaded before).
                    int ak0max = 0;
#pragma unroll
                    for (int jj = 0; jj < 5; jj++) ak0max = max(ak0max, RFL(ak0[jj]));
                    const int nlev = lmax - lmin + 1;                                  // <= scope + 4 <= 78 (ring depth <= 80): two words
                    const int akv = (lane < nlev) ? gmak[j1 * BFS_MAK_SLOTS + (lmin + lane) % depth] : 0;
                    const unsigned long long need = __builtin_amdgcn_ballot_w64(lane < nlev && akv + ak0max >= plen + tlen);
                    unsigned long long need_hi = 0ull;                                 // levels lmin + 64 .. (deep scopes only)
                    if (nlev > 64) {
                        const int akw = (lane + 64 < nlev) ? gmak[j1 * BFS_MAK_SLOTS + (lmin + 64 + lane) % depth] : 0;
                        need_hi = __builtin_amdgcn_ballot_w64(lane + 64 < nlev && akw + ak0max >= plen + tlen);
                    }
                    if ((need | need_hi) == 0ull) continue;
                    for (int lb = lmin; lb <= lmax; lb += 5) {   // five levels of the other aligner
                        const int off = lb - lmin;
                        unsigned long long w = off < 64 ? need >> off : need_hi >> (off - 64);
                        if (off < 64 && off > 59) w |= need_hi << (64 - off);
                        const unsigned bits = (unsigned)w & 31u;
                        if (bits == 0u) continue;
                        int c1[5][5];
#pragma unroll
                        for (int u = 0; u < 5; u++) {
                            const int L = lb + u;
                            const bool lon = (bits >> u) & 1u;
                            const int R1 = kreach<TWO, E1, E2>(pen, L, beg1);
                            const bool on1 = lon && onb && k1 >= max(-plen, -R1) && k1 <= min(tlen, R1);
#pragma unroll
                            for (int c = 0; c < 5; c++) {
                                c1[u][c] = NULLV;
                                if (!TWO && (c == SR_C_I2 || c == SR_C_D2)) continue;
                                if (on1) c1[u][c] = rcell<OT>(RR, KR(L, c), off1 + k1);
                            }
                        }
#pragma unroll
                        for (int jj = 0; jj < 5; jj++) {
                            if (cix[jj] < 0) continue;
                            const int score_0 = s0 + jb + jj;
#pragma unroll
                            for (int u = 0; u < 5; u++) {
                                const int L = lb + u, i = sc1[jj] - L;
                                if (i < 0 || i >= scope || !((bits >> u) & 1u)) continue;      // outside this call's window / level cannot meet
                                if (score_0 + L - gapmax >= bp0) continue;                     // no component could be accepted
#pragma unroll
                                for (int c = 0; c < 5; c++) {
                                    if (!TWO && (c == SR_C_I2 || c == SR_C_D2)) continue;
                                    const int gap = (c == SR_C_M) ? 0 : ((c == SR_C_I1 || c == SR_C_D1) ? pen.o1 : pen.o2);
                                    const int val = score_0 + L - gap;
                                    const int o0 = c0[jj][c], o1 = c1[u][c];
                                    if (val < bp0 && o0 >= 0 && o1 >= 0 && o0 + o1 >= tlen) {
                                        // (value, i * 5 + walk rank, diagonal): i * 5 + rank < 5 * SR_BLK_MAK_SLOTS: 10 bits.  The second key
                                        // is the transposed pair's: the other walk order, the largest diagonal (sr_mirror_rule.h)
                                        atomicMin(&k_sh.pc_best[p][cix[jj]], sr_mirror_bp_key((unsigned)(val + gapmax), i, c, k0));
                                        atomicMin(&k_sh.pc_best_t[p][cix[jj]], sr_mirror_bp_key_t((unsigned)(val + gapmax), i, c, k0));
                                    }
                                }
                            }
                        }
                    }
                }
            }
        }
        __syncthreads();
        const unsigned long long tp3 = PROF ? __builtin_amdgcn_s_memrealtime() : 0ull;
        // ---- W: replay the reference loop
        if (tid < 64) KPRIO_HI();
        if (tid < n2) {
            const int sa = k_sh.p2seg[tid];
            BSeg &sg = b_sh.seg[sa];
            int f = sg.score_f, r = sg.score_r, lf = sg.last_fwd, ph = 2, ci = 0;
            const long long smax = 2LL * ((long long)pen.o1 * 2 + (long long)pen.e1 * (sg.max_ad + 1)) + 1024;
            const BJob &bF = b_sh.job[2 * sa];
            const BJob &bR = b_sh.job[2 * sa + 1];
            const int kinv = bF.tlen - bF.plen;
            while (ph == 2 && f <= avail) {
                for (int half = lf ? 0 : 1; half < 2; half++) {
                    // half 0: F@f against R <= r (then ++r);  half 1: R@r against F <= f (then ++f)
                    const int score_0 = half ? r : f, score_1 = half ? f : r;
                    const int min_1 = (score_1 > scope - 1) ? score_1 - (scope - 1) : 0;
                    if (score_0 + min_1 - gap_opening >= sg.bp_score) { ph = 3; break; }
                    const unsigned long long key = k_sh.pc_best[tid][ci], key_t = k_sh.pc_best_t[tid][ci];
                    ci++;
                    if (key != ~0ull) {
                        const int val = (int)(key >> 42) - gapmax;
                        if (val < sg.bp_score) {
                            if (sr_mirror_bp_tie(key, key_t)) { k_sh.mir_tie = 1; k_sh.sg_tie[sa] = 1; }     // the transposed pair would have split elsewhere
                            const int ord = (int)((key >> 32) & 1023ull), i = ord / 5, rank = ord - i * 5;
                            const int c = (rank == 0) ? SR_C_D2 : (rank == 1) ? SR_C_I2 : (rank == 2) ? SR_C_D1 : (rank == 3) ? SR_C_I1 : SR_C_M;
                            const int k0 = (int)(unsigned)(key & 0xffffffffull) - (1 << 30), k1 = kinv - k0;
                            const int score_i = score_1 - i;
                            const BJob &b0 = half ? bR : bF;
                            const BJob &b1 = half ? bF : bR;
                            const int o0 = rcell<OT>(RR, KR(score_0, c), b0.base + b0.shift + k0);
                            const int o1 = rcell<OT>(RR, KR(score_i, c), b1.base + b1.shift + k1);
                            if (!half) {
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
                    if (half) ++f; else ++r;
                }
                if (ph != 2) break;
                lf = 1;
                if ((long long)f + r > smax) ph = 4;
            }
            sg.score_f = f; sg.score_r = r; sg.last_fwd = lf; sg.phase = ph;
            if (ph != 2) {                                  // levels past the last one the search needed were surplus
                const int last = min(avail, max(f, r));
                const long long sur = blk_surplus(pen, 2 * sa, last, avail) + blk_surplus(pen, 2 * sa + 1, last, avail);
                atomicAdd(&b_sh.cells, (unsigned long long)(-sur));
                k_sh.sg_sur[sa] = (int)sur; k_sh.sg_done[sa] = s0;        // (the search's own tallies: its breakpoint record)
            }
        }
        if (tid < 64) KPRIO_LO();
        __syncthreads();
        if (PROF && tid == 0) {
            const unsigned long long tp4 = __builtin_amdgcn_s_memrealtime();
            k_sh.t_p2a += tp1 - tp0; k_sh.t_p2f += tp2 - tp1; k_sh.t_p2e += tp3 - tp2; k_sh.t_p2w += tp4 - tp3;
        }
    }
#undef KR
}
