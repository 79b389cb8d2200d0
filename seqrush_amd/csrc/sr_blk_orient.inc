// sr_blk_orient.inc -- blocked kernel (sr_align_blk.inc), part 5: in-kernel orientation in register blocks (ori_pass8).
// ---- in-kernel orientation, default penalties (mismatch 1, gap-open 1, gap-extend 1, one piece): register blocks --------
// Same scheme as sr_orient_blk_kernel (sr_orient.hip): a cell of level s depends on levels s-1, s-2 at diagonals k-1..k+1
// only, so a wave tile keeps M[s-1], M[s-2], I[s-1], D[s-1] of its 4 diagonals per lane in registers and walks ORI_B levels
// without touching memory (neighbours by DPP, one diagonal of halo per level and side: 2 lanes).  One workgroup pass = one
// block of both aligners: 1/8 of the barriers and table set-ups of the level-per-pass version, rows read and written
// once per block.  Rows of a block: {M last, M last-1, I last, D last} in ring slots chosen by the block's parity.
#define ORI_B SR_ORI_B           // (one diagonal of halo per level and side: (ORI_B + 3) / 4 lanes; round 3: 8 levels.  The passes of an
                                 // orientation are pure latency -- set-up, one or two tile rounds, three barriers -- and C3 / C5 spend
                                 // 16 % / ~8 % of a pair in them: half as many passes)
template <typename OT, int NT, typename ST>
__device__ __forceinline__ void ori_pass8(const KRows<OT, ST> &R, const int s0, const SrPen &pen, unsigned &row_ld, unsigned &row_st) {
    const int tid = threadIdx.x, lane = tid & 63;
    constexpr int HL = (ORI_B + 3) / 4, OWN = 64 - 2 * HL;
    static_assert(ORI_B <= KB_LV && HL * 4 + 5 <= 24, "orientation block: level tables / the 24-cell margin of the orientation jobs hold the halo");
    if (tid < 64) {
        int nt = 0, glo = 0, ghi = -1, cells = 0;
        if (tid < 2) {
            const BJob &b = b_sh.job[tid];
            int Rw = 0;
#pragma unroll
            for (int j = 0; j < ORI_B; j++) {
                Rw = kreach<false, 1, 1>(pen, s0 + j, SR_C_M);
                const int klo = max(-b.plen, -Rw), khi = min(b.tlen, Rw);
                k_sh.jklo[j][tid] = klo; k_sh.jkhi[j][tid] = khi;
                k_sh.jreach[j][tid] = 0;
                cells += (khi >= klo) ? khi - klo + 1 : 0;
            }
            // window of the block: the last level's range + one diagonal per level of the next block's reach + neighbours
            const int wlo = max(-b.plen - 1, -Rw - ORI_B - 2), whi = min(b.tlen + 1, Rw + ORI_B + 2);
            glo = (wlo + b.shift) >> 2; ghi = (whi + b.shift) >> 2;
            nt = (ghi - glo + OWN) / OWN;
            k_sh.jglo[tid] = glo; k_sh.jghi[tid] = ghi;
        }
        const int n0 = __shfl(nt, 0, 64), n1 = __shfl(nt, 1, 64);
        if (tid == 0) { k_sh.jtstart[0] = 0; k_sh.jtstart[1] = n0; k_sh.total_tiles = n0 + n1; k_sh.next_tile = NT / 64; }
        k_sh.cells_l[tid] += (unsigned long long)cells;
    }
    __syncthreads();
    const int total = RFL(k_sh.total_tiles), n0 = RFL(k_sh.jtstart[1]);
    const int par = (s0 / ORI_B) & 1;
    // rows of the previous block (NULL row before the first one) and of this one
    const unsigned pM1 = s0 ? krow_fix(R, SR_C_M, (1 - par) * 2) : R.nuloff;
    const unsigned pM2 = s0 ? krow_fix(R, SR_C_M, (1 - par) * 2 + 1) : R.nuloff;
    const unsigned pI = s0 ? krow_fix(R, SR_C_I1, 1 - par) : R.nuloff;
    const unsigned pD = s0 ? krow_fix(R, SR_C_D1, 1 - par) : R.nuloff;
    const unsigned oM1 = krow_fix(R, SR_C_M, par * 2), oM2 = krow_fix(R, SR_C_M, par * 2 + 1);
    const unsigned oI = krow_fix(R, SR_C_I1, par), oD = krow_fix(R, SR_C_D1, par);
    for (int t = (tid >> 6); t < total;) {
        const int jid = t >= n0 ? 1 : 0, ti = t - (jid ? n0 : 0);
        const BJob &jb = b_sh.job[jid];
        const int base = RFL(jb.base), shift = RFL(jb.shift), plen = RFL(jb.plen), tlen = RFL(jb.tlen);
        const int kend = RFL(jb.kend), poff = RFL(jb.poff), toff = RFL(jb.pad0);
        const int glo = RFL(k_sh.jglo[jid]), ghi = RFL(k_sh.jghi[jid]);
        const int g = glo + ti * OWN + lane - HL;
        const bool owned = (lane >= HL) && (lane < 64 - HL) && (g <= ghi);
        const int k0 = (g << 2) - shift;
        const unsigned idx0 = klane(R, (unsigned)(base + (g << 2)));
        const LP P = (LP)(lds_seq + poff), T = (LP)(lds_seq + toff);
        const V4<OT> v1 = rld<OT>(R, pM1, idx0), v2 = rld<OT>(R, pM2, idx0), vi = rld_nt<OT>(R, pI, idx0), vd = rld_nt<OT>(R, pD, idx0);
        {
            const int nown = min(OWN, max(0, ghi - (glo + ti * OWN) + 1));
            row_ld += 64u * 4u * (unsigned)(sizeof(ST) / 2); row_st += (unsigned)nown * 4u * (unsigned)(sizeof(ST) / 2);
        }
        int m1[4], m2[4], i1[4], d1[4];
        unsigned lim[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            m1[q] = (int)v1[q]; m2[q] = (int)v2[q]; i1[q] = (int)vi[q]; d1[q] = (int)vd[q];
            lim[q] = (unsigned)min(tlen, plen + k0 + q);
        }
        // LDS-wide symbol / bit index of P[-k0] and T[0] (the orientation aligners span the whole sequences)
        const int cp0 = -k0 + (int)(((uint32_t)(uintptr_t)P >> 2) << SR_WIN_LOG), ct0 = (int)(((uint32_t)(uintptr_t)T >> 2) << SR_WIN_LOG);
        const int cpb = cp0 << SR_SYM_LOG, ctb = ct0 << SR_SYM_LOG;
#pragma unroll
        for (int j = 0; j < ORI_B; j++) {
            const int s = s0 + j;
            const int klo = RFL(k_sh.jklo[j][jid]), khi = RFL(k_sh.jkhi[j][jid]);
            int tiq[4], tdq[4];
#pragma unroll
            for (int q = 0; q < 4; q++) { tiq[q] = max(m2[q], i1[q]); tdq[q] = max(m2[q], d1[q]); }
            const int tiL = lane_left(tiq[3]), tdR = lane_right(tdq[0]);
            int mv[4], iv[4], dv[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int k = k0 + q;
                const bool inr = (k >= klo) && (k <= khi);
                int in_ = bnd(((q == 0) ? tiL : tiq[q == 0 ? 0 : q - 1]) + 1, lim[q]);
                int dn_ = bnd((q == 3) ? tdR : tdq[q == 3 ? 3 : q + 1], lim[q]);
                int m = bnd(m1[q] + 1, lim[q]);
                m = max(m, max(in_, dn_));
                if (!inr) { m = NULLV; in_ = NULLV; dn_ = NULLV; }
                if (s == 0) { m = (inr && k == 0) ? 0 : NULLV; in_ = NULLV; dn_ = NULLV; }
                mv[q] = m; iv[q] = in_; dv[q] = dn_;
            }
            // extension of every cell of the wave (halo lanes feed owned cells of later levels), as in blk_tile16: the eight
            // window reads of the level are in flight together, a window is addressed by its LDS-wide bit index, a NULL
            // cell runs through the same code (it stays negative and bnd() resets it at the next level).  Round 3; before,
            // every cell waited for its own two reads.
            unsigned long long pend[4];
            {
                uint32_t pl[4], ph[4], tl[4], th[4];
                int bp[4], bt[4];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    bp[q] = (mv[q] << SR_SYM_LOG) + cpb - (q << SR_SYM_LOG); bt[q] = (mv[q] << SR_SYM_LOG) + ctb;
                    win_words_bit(bp[q], pl[q], ph[q]); win_words_bit(bt[q], tl[q], th[q]);
                }
                asm volatile("; 8 windows in flight" : "+v"(pl[0]), "+v"(ph[0]), "+v"(pl[1]), "+v"(ph[1]), "+v"(pl[2]), "+v"(ph[2]), "+v"(pl[3]), "+v"(ph[3]),
                                                        "+v"(tl[0]), "+v"(th[0]), "+v"(tl[1]), "+v"(th[1]), "+v"(tl[2]), "+v"(th[2]), "+v"(tl[3]), "+v"(th[3]));
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int nn = (int)lim[q] - mv[q];
                    const uint32_t xw = __builtin_amdgcn_alignbit(ph[q], pl[q], (uint32_t)bp[q]) ^
                                        __builtin_amdgcn_alignbit(th[q], tl[q], (uint32_t)bt[q]);
                    const int ext_ = (int)min3u(ffs_sym(xw), (unsigned)SR_WIN, (unsigned)nn);
                    mv[q] += ext_;
                    pend[q] = __builtin_amdgcn_ballot_w64(ext_ == SR_WIN) & __builtin_amdgcn_ballot_w64(mv[q] >= 0);
                }
            }
            while ((pend[0] | pend[1] | pend[2] | pend[3]) != 0ull) {        // runs longer than a window
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    if (pend[q] == 0ull) continue;
                    const int nn = lanes_or_zero(pend[q], (int)lim[q] - mv[q]);          // 0 for the lanes that are done
                    const uint32_t xw = win_sym(mv[q] + cp0 - q) ^ win_sym(mv[q] + ct0);
                    mv[q] += (int)min3u(ffs_sym(xw), (unsigned)SR_WIN, (unsigned)nn);
                    pend[q] = __builtin_amdgcn_ballot_w64(xw == 0u && nn > SR_WIN);
                }
            }
            bool reached = false;
#pragma unroll
            for (int q = 0; q < 4; q++) reached |= owned && (k0 + q) == kend && (k0 + q) >= klo && (k0 + q) <= khi && mv[q] >= tlen;
            if (reached) k_sh.jreach[j][jid] = 1;
#pragma unroll
            for (int q = 0; q < 4; q++) { m2[q] = m1[q]; m1[q] = mv[q]; i1[q] = iv[q]; d1[q] = dv[q]; }
        }
        if (owned) {
            V4<OT> a1, a2, ai, ad;
#pragma unroll
            for (int q = 0; q < 4; q++) { a1[q] = (OT)m1[q]; a2[q] = (OT)m2[q]; ai[q] = (OT)i1[q]; ad[q] = (OT)d1[q]; }
            rst<OT>(R, oM1, idx0, a1); rst<OT>(R, oM2, idx0, a2); rst<OT>(R, oI, idx0, ai); rst<OT>(R, oD, idx0, ad);
        }
        int nx = 0;
        if (lane == 0) nx = atomicAdd(&k_sh.next_tile, 1);
        t = RFL(nx);
    }
}
