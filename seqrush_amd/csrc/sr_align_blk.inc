// sr_align_blk.inc -- score-blocked, wave-tiled biWFA kernel (included by sr_align_blk.hip
// after sr_align_bfs.inc, whose job / segment bookkeeping and backtrace it reuses).
//
// Same alignment rules as oracle/wfa.c and the two older kernels.  The schedule:
//
//  * Score blocking.  M[s] reads M[s-x], M[s-o1-e1], M[s-o2-e2] and the I/D cells
//    of its own level; I/D[s] read I/D[s-e] and the same M rows.  So the B =
//    min(x, o1+e1, o2+e2, 5) levels s0 .. s0+B-1 depend on levels < s0 except for the
//    I/D extension chains (distance e1 / e2), which are short integer recurrences
//    without sequence comparison.  One pass therefore computes B levels: a fifth
//    of the barriers, row look-ups and control of a level-per-pass schedule, and
//    every source row is read once per block instead of once per level.
//  * Wave tiles.  A wave owns 60 adjacent 4-diagonal groups (lanes 2..61; lanes
//    0,1,62,63 recompute the neighbours' chain cells as a halo), so the k-1 / k+1
//    neighbours of every row are the adjacent lanes' registers (DPP wave shifts):
//    one 8-byte load per row and lane, no neighbour loads, and all aligner
//    parameters are wave-uniform (SGPRs).
//  * Rows: [level mod depth][component] in one ring (depth = scope + B + 1), the
//    base-case history has the same shape with depth = all levels.
//  * Breakpoint detection: see blk_overlap (upper-bound row filter + reduction).
#include "sr_blk_rows.inc"      // LDS state, row storage and addressing, lane helpers
#include "sr_blk_tile.inc"      // wave tiles
#include "sr_blk_pass.inc"      // pass tables, tile queue, I/D recompute
#include "sr_blk_phase2.inc"    // batched breakpoint detection
#include "sr_blk_orient.inc"    // in-kernel orientation

// Margins of an aligner's range in the shared rows: diagonal k lives at base + |p| + K_SHIFT0 + k so that the halo
// lanes of the widest tile geometry (ceil(B / 4) groups: 7 = 28 diagonals for 25-level blocks, + the -|p| - 1 margin diagonal) stay
// inside the aligner's own range on the left, K_WIDTH0 covers the same on the right.
#define K_SHIFT0 29
#define K_WIDTH0 64
// thread 0: describe aligner jid.  Row geometry of this kernel: the halo groups lie inside the aligner's own
// range.  A reverse aligner is the forward aligner of the reverse complements: LDS holds both copies of
// the query (poff_f = chosen orientation, poff_r = the other one) and of the target.
struct KSeqs { int poff_f, poff_r, toff_f, toff_r, plen_all, tlen_all; };
__device__ __forceinline__ void kjob_set(int jid, int base, int pb, int pe, int tb, int te, int rev, int begin, int chk,
                                         int seg, const KSeqs &q) {
    bjob_set(jid, base, pb, pe, tb, te, 0, begin, chk, seg, rev ? q.poff_r : q.poff_f);
    BJob &b = b_sh.job[jid];
    b.shift = (pe - pb) + K_SHIFT0;
    b.pad0 = rev ? q.toff_r : q.toff_f;
    b.pad2 = 1;                                             // store every I/D row (breakpoint searches may clear it)
    if (rev) { b.p0 = q.plen_all - pe; b.t0 = q.tlen_all - te; }
}
__device__ __forceinline__ int kjob_width(int plen, int tlen) { return (plen + tlen + K_WIDTH0) & ~3; }

// B, E1, E2: block of the alignment penalties (host guarantees B <= min(x, o1+e1, o2+e2), e1 == E1, e2 == E2);
// the orientation penalties run level by level (B = 1) and must be one-piece with gap-extend 1.
// PROF: 100 MHz tick counters of the phases of a pair (counters[6..15]); only the instance SR_PROFILE_TICKS=1 selects
// carries the s_memrealtime reads (they cost ~10 % of the wave cycles)
// RT: storage type of the ring's cells (OT, or uint16_t = offset - SR_RING_BIAS for 32-bit searches below 57 k, see KRows)
#define SR_BLK_MIN_WAVES 4         // second __launch_bounds__ argument: the occupancy the kernel's registers are budgeted for
template <typename OT, int NT, bool TWO, int B, int E1, int E2, bool PROF = false, int X = 0, int OE1 = 0, typename RT = OT>
__global__ void __launch_bounds__(NT, SR_BLK_MIN_WAVES) sr_align_blk_kernel(SrAlignArgs a) {
    const int tid = threadIdx.x;
    // tail launch (DESIGN.md 4.3): nothing was deferred -> the workgroup leaves before it touches a row or a barrier.  (Uniform:
    // nothing in a tail launch writes tail_count; the main launch that did ended before this one began.)
    if (a.tail_mode == SR_TAIL_RUN && *a.tail_count == 0u) return;
    GP<RT> bring = (GP<RT>)(RT *)a.bring + (size_t)blockIdx.x * a.bring_wg_stride;
    GP<OT> bhist = (GP<OT>)(OT *)a.bhist + (size_t)blockIdx.x * a.bhist_wg_stride;
    GP<int> lists = (GP<int>)a.bseg + (size_t)blockIdx.x * 2 * SR_BFS_MAXSEG * SR_BFS_SEGREC;
    GP<uint32_t> btbuf = (GP<uint32_t>)a.bbt + (size_t)blockIdx.x * a.bbase_jobs * SR_BFS_BTCAP;
    GP<uint32_t> clist = (GP<uint32_t>)a.bcl + (size_t)blockIdx.x * a.bcl_wg_stride;
    GP<int> gmak = (GP<int>)a.bmak + (size_t)blockIdx.x * (BJ_MAX * BFS_MAK_SLOTS);   // [aligner][level mod depth] max antidiagonal
    unsigned long long t_ori = 0, t_bp = 0, t_base = 0, t_all = 0, tb_bt = 0, tb_emit = 0;
    unsigned long long tq_pass = 0, tq_bar = 0, tq_ctl = 0, tq_ph2 = 0, tq_tail = 0, tq_rec = 0;
    unsigned row_ld = 0, row_st = 0;                     // per pair, in lane accesses (flushed to the wave's sums in LDS per pair)
    // PROF, thread 0: the workgroup's timeline (a.timeline, 4 words per workgroup): first dequeue, start of the last alignment,
    // alignments run, whether the last one came from mir_next; and (a.prio_timeline, 4 more words) the end of its first alignment, its
    // rank on the CU, the CU's table index and its arrival count there
    unsigned long long tl_first = 0, tl_last = 0, tl_n = 0, tl_mir = 0, tl_end1 = 0;
    const int depth = a.kdepth;
    // ring: chunk-major rows (see KRows); rows = 5 components x depth levels + NULL row + U row
    const int depth2 = a.kdepth2;
    const unsigned nrows = (unsigned)depth + 4u * (unsigned)depth2 + (unsigned)SR_NULL_ROWS + 2u;      // + NULL rows, U row, trash row
    KRows<OT, RT> RR;
    KRows<OT, OT> RH;
    RR.base = bring; RR.cM = (unsigned)depth * 256u; RR.cst2 = (unsigned)depth2 * 256u; RR.sstr = 256u; RR.chs = nrows * 256u;
    RR.depth = depth; RR.depth2 = depth2; RR.perjob = false; RR.extent = (unsigned)a.bring_wg_stride;
    // (SR_NULL_ROWS = 10 adjacent NULL rows: a block of levels below 0 is read with the same immediates as a block of the ring)
    RR.nuloff = ((unsigned)depth + 4u * (unsigned)depth2) * 256u; RR.urow = RR.nuloff + (unsigned)SR_NULL_ROWS * 256u; RR.trash = RR.urow + 256u;
    const unsigned urow = RR.urow;
    // base-case history: hist_cap cells; every job of a batch has its own region [its levels][component][its width] (BJob
    // hbase / hw), the NULL row (one worst-case job wide: the jobs' columns start at 0) sits behind the data
    const unsigned hw = a.hist_nul_w;
    RH.base = bhist; RH.cM = 0; RH.cst2 = 0; RH.sstr = 0; RH.chs = 256u; RH.depth = 0x3fff; RH.depth2 = 0x3fff; RH.urow = 0; RH.perjob = true; RH.extent = (unsigned)a.bhist_wg_stride;
    RH.nuloff = (unsigned)a.hist_cap; RH.trash = RH.nuloff + hw;
    if (tid < 64) k_sh.cells_l[tid] = 0ull;
    if (tid < 64) k_sh.row_w[tid >> 4][tid & 15] = 0ull;
    {   // NULL rows
        for (int r = 0; r < SR_NULL_ROWS; r++)
            for (int i = tid; i < a.brow; i += NT) rput(RR, RR.nuloff + (unsigned)r * 256u, (unsigned)i, NULLV);
        for (int i = tid; i < (int)hw; i += NT) RH.base[RH.nuloff + (unsigned)i] = (OT)NULLV;
        if (tid == 0) {
            b_sh.pen[0] = a.pen; b_sh.pen[1] = a.ori; b_sh.cells = 0; k_sh.t_setup = 0; k_sh.t_p2a = k_sh.t_p2f = k_sh.t_p2e = k_sh.t_p2w = 0; k_sh.t_c1 = k_sh.t_c2 = 0;
            k_sh.dg_f = k_sh.dg_c = k_sh.dg_e = k_sh.dg_r = 0; k_sh.dg_redo = 0;
#ifdef SR_BOUNDS
            k_sh.bnd_flag = 0; k_sh.bnd_off = k_sh.bnd_ext = k_sh.bnd_what = 0; k_sh.lds_seq_bytes = 16u * a.max_words + 16u;
#endif
            k_sh.dg_steps = k_sh.dg_nbase = k_sh.dg_nbp = k_sh.dg_npass = 0; k_sh.base_tiles = k_sh.base_cells = 0;
            k_sh.mir_next = -1; k_sh.mir_pairs = k_sh.mir_ties = 0;
            k_sh.rp_record = k_sh.rp_on = k_sh.rp_ready = 0; k_sh.rp_nrec = 0;
            k_sh.rp_replays = k_sh.rp_cached = k_sh.rp_tie_top = k_sh.rp_tie_base = 0;
            b_sh.geom.brow = a.brow; b_sh.geom.ring_scope = a.ring_scope; b_sh.geom.ring_hot = a.ring_hot;
            b_sh.geom.bbase_jobs = a.bbase_jobs; b_sh.geom.hist_w = a.hist_w; b_sh.geom.hist_levels = a.hist_levels;
            b_sh.geom.urow = urow;
            // rank among the workgroups of this CU (sr_prio_rule.h): arrival count of the CU the hardware ids name.  Reads only:
            // HW_REG_XCC_ID (20) bits [3:0]; HW_REG_HW_ID (4) bits [15:8] = CU_ID, SH_ID, SE_ID
            unsigned p_rank = 0, p_idx = 0, p_arr = 0;
            if (a.cu_arrivals) {
                const unsigned xcc = (unsigned)__builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11));
                const unsigned cu = (unsigned)__builtin_amdgcn_s_getreg(4 | (8 << 6) | (7 << 11));
                p_idx = sr_prio_table_index(xcc, cu);
                p_arr = atomicAdd(&a.cu_arrivals[p_idx], 1u);
                p_rank = p_arr % (unsigned)max(a.prio_wg, 1);
                atomicAdd(&a.counters[52], 1ull);
                atomicMax(&a.counters[53], (unsigned long long)p_arr + 1ull);
            }
            k_sh.prio_rank = (int)p_rank; k_sh.prio_role = 0;
            k_sh.prio_wg = (a.tile_prio && a.cu_arrivals && a.prio_wg > 1) ? a.prio_wg : 0;
            if (PROF && a.prio_timeline) {
                unsigned long long *tp = a.prio_timeline + 4ull * blockIdx.x;
                tp[0] = 0ull; tp[1] = p_rank; tp[2] = p_idx; tp[3] = p_arr;
            }
        }
        __syncthreads();
    }
    const SrPen pen = a.pen;
    const SrPen ori = a.ori;
    constexpr bool KTIGHT = KTIGHT_OF(OT, RT, B, X);      // ring tiles cover a block's own range only (kwindow)
    const int scope = pen.scope;
    const int gap_opening = TWO ? max(pen.o1, pen.o2) : pen.o1;
    // Mirrored emission (DESIGN.md 4.3, sr_mirror_rule.h).  a.mirror pairs (q, t) with the (t, q) of the same batch: the
    // secondary is skipped when it is dequeued; the primary's workgroup either writes the secondary's outputs itself -- the
    // transposed CIGAR, when the primary ran on the forward strand without an error and without a tie-sensitive decision --
    // or aligns the secondary next (mir_next), as an ordinary pair, without going to the queue.
    for (;;) {
        if (tid < 64) {
            // the cells of the pairs so far leave the lanes' sums: what a pair adds to b_sh.cells is then its own
            unsigned long long cl = k_sh.cells_l[tid];
            k_sh.cells_l[tid] = 0ull;
            for (int o = 32; o > 0; o >>= 1) cl += __shfl_xor(cl, o, 64);
            if (tid == 0) b_sh.cells += cl;
        }
        if (tid == 0) {
            int pr = k_sh.mir_next;
            k_sh.mir_next = -1;
            const bool from_mir = pr >= 0;
            if (a.tail_mode == SR_TAIL_RUN) {
                // tail launch: the deferred secondaries, by batch-relative index, each an ordinary pair (no order[], no skip)
                const uint32_t i = atomicAdd(a.tail_head, 1u);
                pr = i < *a.tail_count ? (int)a.tail_list[i] : (int)a.npairs;
            } else while (pr < 0) {
                pr = (int)atomicAdd(a.queue_head, 1u);
                if (pr >= (int)a.npairs) { pr = (int)a.npairs; break; }
                if (a.order) pr = (int)a.order[pr];          // cost-sorted dequeue order (longest pairs first)
                if (a.mirror && a.mirror[pr] != SR_MIRROR_NONE && (a.mirror[pr] & SR_MIRROR_SECONDARY)) pr = -1;   // its primary's business
            }
            if (PROF) {
                const unsigned long long now = KTICK();
                if (tl_n == 0) tl_first = now;
                if (tl_n == 1 && tl_end1 == 0) tl_end1 = now;      // the first alignment ended (its own emitted secondary included)
                if (pr < (int)a.npairs) { tl_last = now; tl_n++; tl_mir = from_mir ? 1ull : 0ull; }
            }
            // replay (sr_mirror_rule.h): a secondary that follows its primary on this workgroup takes breakpoints from the primary's
            // records when the primary's end said they suit it; a primary that has a partner writes records
            k_sh.rp_on = (from_mir && k_sh.rp_ready) ? 1 : 0;
            k_sh.rp_ready = 0; k_sh.rp_record = 0;
            if (a.brec && !from_mir && a.tail_mode != SR_TAIL_RUN && a.mirror && pr < (int)a.npairs) {
                const uint32_t m = a.mirror[pr];
                if (m != SR_MIRROR_NONE && !(m & SR_MIRROR_SECONDARY)) { k_sh.rp_record = 1; k_sh.rp_nrec = 0; }
            }
            k_sh.rp_level = 0; k_sh.rp_rd = 0; k_sh.rp_top_tie = 0; k_sh.rp_seg_tie = 0;
            b_sh.pair = pr;
            b_sh.err = 0; b_sh.cig_cnt = 0; b_sh.score_acc = 0; k_sh.pend_op = -1; k_sh.pend_len = 0;
            k_sh.mir_tie = 0;
            k_sh.mir_snap[0] = b_sh.cells; k_sh.mir_snap[1] = k_sh.dg_steps; k_sh.mir_snap[2] = k_sh.dg_nbase; k_sh.mir_snap[3] = k_sh.dg_nbp;
        }
        __syncthreads();
        const int pair = RFL(b_sh.pair);
        if (pair >= (int)a.npairs) break;
        const uint32_t q = a.pair_q[pair], t = a.pair_t[pair];
        const int plen = (int)a.seqlen[q], tlen = (int)a.seqlen[t];
        const int pw = SR_SEQ_WORDS(plen), tw = SR_SEQ_WORDS(tlen);
        // LDS: query forward / reverse complement, target forward / reverse complement (each with a pad word in front)
        load_seq_lds<NT>(lds_seq, (GP<const uint32_t>)a.seqwords + a.word_off_fwd[q] - 1, pw);
        load_seq_lds<NT>(lds_seq + a.max_words, (GP<const uint32_t>)a.seqwords + a.word_off_rc[q] - 1, pw);
        load_seq_lds<NT>(lds_seq + 2 * (size_t)a.max_words, (GP<const uint32_t>)a.seqwords + a.word_off_fwd[t] - 1, tw);
        // (2-bit ACGT buffers: the reversed copies are the reverse complements -- complementing both sides keeps
        // equality; other alphabets: plain reversed copies, the reference's complement is not injective on them)
        load_seq_lds<NT>(lds_seq + 3 * (size_t)a.max_words, (GP<const uint32_t>)a.seqwords + a.word_off_rev[t] - 1, tw);
        const int oPf = 1, oPr = (int)a.max_words + 1, oTf = 2 * (int)a.max_words + 1, oTr = 3 * (int)a.max_words + 1;
        GP<uint32_t> ops = (GP<uint32_t>)a.cigar_ops + a.cigar_base[pair];
        const uint32_t cap = (uint32_t)(a.cigar_base[pair + 1] - a.cigar_base[pair]);
        const unsigned long long tk0 = KTICK();
        // ---------------- orientation: forward and reverse-complement query as two aligners of one pass.
        // Forward wins ties; the reverse complement is chosen iff it reaches the end at a strictly lower score.
        int fwd = -1, rev = INT_MAX, is_rev = 0;
        if (a.pre_oriented) {                                 // sr_orient_kernel ran before this kernel
            is_rev = a.is_reverse[pair] != 0; fwd = a.ori_fwd[pair]; rev = a.ori_rev[pair];
        } else {
        if (tid == 0) {
            const int w = kjob_width(plen, tlen);
            const KSeqs k0 = {oPf, oPr, oTf, oTr, plen, tlen}, k1 = {oPr, oPf, oTf, oTr, plen, tlen};
            kjob_set(0, 0, 0, plen, 0, tlen, 0, SR_C_M, SR_C_M, 0, k0);
            kjob_set(1, w, 0, plen, 0, tlen, 0, SR_C_M, SR_C_M, 0, k1);
            b_sh.njobs = 2;
        }
        __syncthreads();
        const long long smax = (long long)ori.o1 * 2 + (long long)ori.e1 * (plen + tlen) + 64;
        if (!ori.two && ori.x == 1 && ori.o1 == 1 && ori.e1 == 1 && !a.ori_levels) {
            // default orientation penalties: 8-level register blocks (ori_pass8); wider margins than the alignment jobs
            if (tid == 0) {
                b_sh.job[0].shift = plen + 24; b_sh.job[1].shift = plen + 24;
                b_sh.job[1].base = (plen + tlen + 64) & ~3;
            }
            __syncthreads();
            for (int s0 = 0;; s0 += ORI_B) {
                ori_pass8<OT, NT>(RR, s0, ori, row_ld, row_st);
                __syncthreads();
                int hit = -1, who = 0;                         // per level the forward aligner is looked at first
#pragma unroll
                for (int j = ORI_B - 1; j >= 0; j--) {
                    const bool rf = RFL(k_sh.jreach[j][0]) != 0, rr = RFL(k_sh.jreach[j][1]) != 0;
                    if (rf || rr) { hit = j; who = rf ? 0 : 1; }
                }
                __syncthreads();                      // the next pass resets jreach
                const int used = hit >= 0 ? hit + 1 : ORI_B;
                if (tid == 0) k_sh.dg_steps += 2ull * (unsigned long long)used;
                if (hit >= 0) {
                    if (tid == 0) {                             // cells of the block's levels past the deciding one were surplus
                        long long sur = 0;
                        for (int l = s0 + hit + 1; l < s0 + ORI_B; l++) {
                            const int Rw = reach(ori, l, SR_C_M);
                            sur += 2LL * (long long)(min(tlen, Rw) - max(-plen, -Rw) + 1);
                        }
                        b_sh.cells -= (unsigned long long)sur;
                    }
                    if (who == 0) fwd = s0 + hit; else { rev = s0 + hit; is_rev = 1; }
                    break;
                }
                if (s0 + ORI_B - 1 > smax) { if (tid == 0) b_sh.err |= SR_DEV_ERR_SCORE_BOUND; break; }
            }
        } else {
            for (int s = 0;; s++) {
                blk_pass<OT, false, NT, 1, 1, 1, PROF>(RR, s, ori, 2, row_ld, row_st);
                __syncthreads();
                if (tid == 0) k_sh.dg_steps += 2ull;
                const bool rf = RFL(k_sh.jreach[0][0]) != 0, rr = RFL(k_sh.jreach[0][1]) != 0;
                __syncthreads();                      // the next pass resets jreach
                if (rf) { fwd = s; break; }
                if (rr) { rev = s; is_rev = 1; break; }
                if (s > smax) { if (tid == 0) b_sh.err |= SR_DEV_ERR_SCORE_BOUND; break; }
            }
        }
        }
        if (a.word_off_rev != a.word_off_rc) {
            // the reverse aligners read the pattern backwards: reversed query (forward orientation) or
            // complemented query (reverse-complement orientation) replaces the copy the orientation did not choose
            __syncthreads();
            load_seq_lds<NT>(lds_seq + (is_rev ? 0 : (size_t)a.max_words),
                             (GP<const uint32_t>)a.seqwords + (is_rev ? a.word_off_cmp[q] : a.word_off_rev[q]) - 1, pw);
            __syncthreads();
        }
        const KSeqs ks = {is_rev ? oPr : oPf, is_rev ? oPf : oPr, oTf, oTr, plen, tlen};
        const unsigned long long tk1 = KTICK();
        t_ori += tk1 - tk0;
        // ---------------- ordered segment list, breadth-first breakpoint search
        GP<int> cur = lists, nxt = lists + (size_t)SR_BFS_MAXSEG * SR_BFS_SEGREC;
        if (tid == 0) {
            cur[SL_PB] = 0; cur[SL_PE] = plen; cur[SL_TB] = 0; cur[SL_TE] = tlen; cur[SL_CB] = SR_C_M; cur[SL_CE] = SR_C_M;
            const int rem = (a.mem_mode == 3) ? INT_MAX : -1;
            cur[SL_REM] = rem; cur[SL_KIND] = seg_kind(plen, tlen, rem);
            b_sh.list_n = 1;
            if (is_rev) k_sh.rp_on = 0;                      // (a reverse-strand secondary is not the transpose of anything recorded)
            if (k_sh.rp_on) k_sh.rp_replays += 1ull;
        }
        __syncthreads();
        for (;;) {                                           // one iteration per recursion level
            const int n_cur = RFL(b_sh.list_n);
            bool any_bp = false;
            int pos = 0;
            if (RFL(k_sh.rp_on) != 0 && tid == 0) {
                // Replay: the level's segments under search against the primary's records of the level, both in list order
                // (two-pointer walk, sr_mirror_rule.h).  A segment whose transposed record exists and has no tie bit gets the
                // transposed breakpoint and the search's tallies and is not searched; every other one is searched as ever.
                GP<int> recs = (GP<int>)a.brec + (size_t)blockIdx.x * (SR_BPREC_MAX * SR_BPREC_INTS);
                const int nrec = min(k_sh.rp_nrec, SR_BPREC_MAX), lvl = k_sh.rp_level;
                int rd = k_sh.rp_rd;
                unsigned long long cells = 0ull, cached = 0ull;
                while (rd < nrec && recs[rd * SR_BPREC_INTS + SR_BR_LEVEL] < lvl) rd++;
                for (int p = 0; p < n_cur; p++) {
                    GP<int> e = cur + (size_t)p * SR_BFS_SEGREC;
                    if (e[SL_KIND] != SK_BP) continue;
                    int solved = 0;
                    while (rd < nrec) {
                        GP<int> r = recs + rd * SR_BPREC_INTS;
                        if (r[SR_BR_LEVEL] != lvl) break;
                        const int c = sr_replay_cmp(r, e);
                        if (c > 0) break;
                        rd++;
                        if (c < 0) continue;
                        if (r[SR_BR_TIE] == 0 && sr_replay_same(r, e)) {
                            e[SL_BV] = sr_bprec_t(r, SR_BR_BV); e[SL_BH] = sr_bprec_t(r, SR_BR_BH); e[SL_BCOMP] = sr_bprec_t(r, SR_BR_BCOMP);
                            e[SL_BSF] = r[SR_BR_BSF]; e[SL_BSR] = r[SR_BR_BSR]; e[SL_PASSES] = r[SR_BR_PASSES];
                            cells += ((unsigned long long)(unsigned)r[SR_BR_CELLS_HI] << 32) | (unsigned long long)(unsigned)r[SR_BR_CELLS_LO];
                            cached += 1ull; solved = 1;
                        }
                        break;
                    }
                    e[SL_SOLVED] = solved;
                }
                k_sh.rp_rd = rd; b_sh.cells += cells; k_sh.rp_cached += cached;
            }
            while (pos < n_cur && RFL(b_sh.err) == 0) {      // chunks of <= SR_BFS_MAXACT segments
                __syncthreads();
                if (tid == 0) {
                    // (a replaying pair keeps the chunks it would have had: its solved segments take a place in the chunk and are
                    // not activated, so that the levels counted per pass, chunk by chunk, come out as without the replay)
                    int na = 0, p = pos, base = 0, ntot = 0, maxp = 0;
                    const bool rp_on = k_sh.rp_on != 0, rp_rec = k_sh.rp_record != 0;
                    for (; p < n_cur && ntot < SR_BFS_MAXACT; p++) {
                        GP<int> e = cur + (size_t)p * SR_BFS_SEGREC;
                        if (e[SL_KIND] != SK_BP) continue;
                        ntot++;
                        if (rp_on && e[SL_SOLVED] != 0) { maxp = max(maxp, e[SL_PASSES]); continue; }
                        k_sh.sg_tie[na] = 0; k_sh.sg_sur[na] = 0; k_sh.sg_done[na] = 0;
                        if (rp_rec) {                           // the two aligners' cell sums start at 0: what they hold when the search ends is its own
                            b_sh.cells += k_sh.cells_l[2 * na] + k_sh.cells_l[2 * na + 1];
                            k_sh.cells_l[2 * na] = 0ull; k_sh.cells_l[2 * na + 1] = 0ull;
                        }
                        BSeg &sg = b_sh.seg[na];
                        sg.pb = e[SL_PB]; sg.pe = e[SL_PE]; sg.tb = e[SL_TB]; sg.te = e[SL_TE]; sg.cb = e[SL_CB]; sg.ce = e[SL_CE];
                        sg.score_f = sg.score_r = 0; sg.last_fwd = 0; sg.f_ak = sg.r_ak = 0; sg.phase = 1;
                        const int sp = sg.pe - sg.pb, st = sg.te - sg.tb;
                        sg.max_ad = sp + st - 1; sg.bp_score = INT_MAX; sg.list_pos = p;
                        const int w = kjob_width(sp, st);
                        kjob_set(2 * na, base, sg.pb, sg.pe, sg.tb, sg.te, 0, sg.cb, -1, na, ks); base += w;
                        kjob_set(2 * na + 1, base, sg.pb, sg.pe, sg.tb, sg.te, 1, sg.ce, -1, na, ks); base += w;
                        if (a.lazy_id) { b_sh.job[2 * na].pad2 = 0; b_sh.job[2 * na + 1].pad2 = 0; }
                        na++;
                    }
                    b_sh.nact = na; b_sh.next_pos = p; b_sh.njobs = 2 * na; b_sh.nrunning = na;
                    k_sh.rp_ntot = ntot; k_sh.rp_maxp = maxp; k_sh.rp_npass0 = k_sh.dg_npass;
                }
                __syncthreads();
                const int nact = RFL(b_sh.nact);
                pos = RFL(b_sh.next_pos);
                if (RFL(k_sh.rp_ntot) == 0) break;
                any_bp = true;
                if (tid == 0) k_sh.dg_nbp += (unsigned long long)k_sh.rp_ntot;
                if (nact == 0) {
                    // every segment of the chunk has its breakpoint: no pass; the levels its searches would have counted
                    if (tid == 0) k_sh.dg_steps += 2ull * (unsigned long long)k_sh.rp_ntot * B * (unsigned long long)k_sh.rp_maxp;
                    continue;
                }
                const unsigned long long tb0 = KTICK();
                const int njobs = 2 * nact;
                for (int s0i = 0; RFL(b_sh.nrunning) > 0; s0i += B) {
                    const int s0 = kopaque_s(s0i);      // (no per-lane induction variables derived from the level across the pass)
                    const unsigned long long q0 = KTICK();
                    blk_pass<OT, TWO, NT, B, E1, E2, PROF, X, OE1, RT, true>(RR, s0, pen, njobs, row_ld, row_st, s0 == 0);
                    const unsigned long long q1 = KTICK();
                    __syncthreads();
                    const unsigned long long q2 = KTICK();
                    tq_pass += q1 - q0; tq_bar += q2 - q1;
                    if (tid == 0) k_sh.dg_steps += (unsigned long long)njobs * B;
                    const int avail = s0 + B - 1;
                    // wave 0: per-aligner max antidiagonal of the block's levels, per-segment phase-1 control (one
                    // lane each), the set of segments in phase 2 and -- when there is none -- the pass's tail
                    const int tid_o = tid;
                    if (tid < 64) {
                        // (the section's per-lane addresses -- the lane's max_ak slots, its segment record -- are formed from an opaque
                        //  copy of the thread index, here, once per pass: hoisted out of the pass loop they lived, spilled, across the tiles)
                        const int tid = (int)kopaque_v((unsigned)tid_o);
                        KPRIO_HI();
                        {   // max_ak of the block's levels: one (aligner, level) pair per lane, as the pass tables (sr_pass_rule.h);
                            // one modulo per pass (uniform; B < depth, so + level wraps once); the stores drain under the rest
                            const int sb = s0 % depth, steps = sr_pass_steps(njobs, B);
                            for (int st = 0; st < steps; st++) {
                                int al, j;
                                if (sr_pass_lane(tid, st, B, al, j) && al < njobs) {
                                    const int sl = sb + j;
                                    gmak[al * BFS_MAK_SLOTS + (sl >= depth ? sl - depth : sl)] = k_sh.jak[j][al];
                                }
                            }
                        }
                        const unsigned long long qc1 = KTICK();
                        int ph = 0, ph0 = 0;
                        if (tid < nact) {
                            BSeg &sg = b_sh.seg[tid];
                            ph = sg.phase; ph0 = ph;
                            const long long smax = 2LL * ((long long)pen.o1 * 2 + (long long)pen.e1 * (sg.max_ad + 1)) + 1024;
                            if (ph == 1) {
                                int score_f = sg.score_f, score_r = sg.score_r, last_fwd = sg.last_fwd, f_ak = sg.f_ak, r_ak = sg.r_ak;
                                const int max_ad = sg.max_ad;
                                // the segment's 2 B max antidiagonals in one batch of independent LDS reads (a pair per level):
                                // the walk over the levels then runs on registers
                                typedef int __attribute__((ext_vector_type(2), may_alias)) I2;
                                I2 ak[B];
#pragma unroll
                                for (int j = 0; j < B; j++) ak[j] = *(const I2 *)&k_sh.jak[j][2 * tid];
                                // Per level, in the order of the search: the forward aligner takes the level (score_f = s) and is
                                // tested against the reverse aligner's previous one, then the reverse aligner takes it and the sum
                                // of the scores and the antidiagonals are tested again.  Selects, not branches: a level that comes
                                // after the segment left phase 1 changes nothing (ten nested lane conditions would cost ten
                                // saved EXEC masks, which this kernel keeps in spilled registers).
#pragma unroll
                                for (int j = 0; j < B; j++) {
                                    const int s = s0 + j;                       // (uniform)
                                    const bool on = ph == 1;
                                    const int akf = ak[j].x, akr = ak[j].y;
                                    const bool both = akf + akr >= max_ad;
                                    if (s == 0) {
                                        f_ak = on ? akf : f_ak; r_ak = on ? akr : r_ak;
                                        ph = (on && both) ? 2 : ph;
                                    } else {
                                        const bool fwd_hit = akf + r_ak >= max_ad;     // forward at s, reverse still at s - 1
                                        const bool rev = on && !fwd_hit;
                                        const bool over = (long long)s + s > smax;     // score_f + score_r, both s
                                        score_f = on ? s : score_f; f_ak = on ? akf : f_ak; last_fwd = on ? (fwd_hit ? 1 : 0) : last_fwd;
                                        score_r = rev ? s : score_r; r_ak = rev ? akr : r_ak;
                                        ph = on ? (fwd_hit ? 2 : (over ? 4 : (both ? 2 : 1))) : ph;
                                    }
                                }
                                sg.score_f = score_f; sg.score_r = score_r; sg.last_fwd = last_fwd; sg.f_ak = f_ak; sg.r_ak = r_ak;
                                sg.phase = ph;
                            }
                        }
                        const unsigned long long qc2 = KTICK();
                        if (PROF && tid == 0) { k_sh.t_c1 += qc1 - q2; k_sh.t_c2 += qc2 - qc1; }
                        const unsigned long long m2 = __ballot(ph == 2);
                        const unsigned long long mnew = __ballot(ph == 2 && ph0 == 1);
                        if (tid == 0) k_sh.newmask = (unsigned)mnew;
                        if (tid == 0) { k_sh.p2mask_lo = (unsigned)m2; k_sh.p2mask_hi = (unsigned)(m2 >> 32); }
                        if (m2 == 0ull) {                           // no breakpoint detection this pass: finish it here
                            const unsigned long long run = __ballot(ph == 1);
                            if (tid < nact && ph != 1) { b_sh.job[2 * tid].active = 0; b_sh.job[2 * tid + 1].active = 0; }
                            if (tid == 0) b_sh.nrunning = __popcll(run);
                            // (the lanes' stores to job[].active above are read by other lanes below: same wave, LDS in order)
                            if (run != 0ull) blk_setup<TWO, NT, B, E1, E2, KTIGHT>(s0 + B, pen, njobs, tid);   // tables of the next pass
                        }
                        KPRIO_LO();
                    }
                    __syncthreads();
                    const unsigned long long q3 = KTICK();
                    tq_ctl += q3 - q2;
                    bool p2_or_rec = (RFL(k_sh.p2mask_lo) | RFL(k_sh.p2mask_hi)) != 0u;
                    if (a.lazy_id) {
                        if (RFL(k_sh.newmask) != 0u) p2_or_rec = true;
                        for (unsigned nm = RFL(k_sh.newmask); nm != 0u; nm &= nm - 1u) {
                            const int sa = __ffs((int)nm) - 1;
                            blk_recompute<OT, TWO, NT, B, E1, E2, X, OE1>(RR, pen, sa, RFL(b_sh.seg[sa].score_f), s0, row_ld, row_st);
                        }
                    }
                    tq_rec += KTICK() - q3;
                    if ((RFL(k_sh.p2mask_lo) | RFL(k_sh.p2mask_hi)) != 0u) {
                        blk_phase2<OT, TWO, NT, B, E1, E2, RT, PROF>(RR, clist, gmak, pen, s0, nact, gap_opening);
                        if (tid < 64) {
                            const int tid = (int)kopaque_v((unsigned)tid_o);
                            KPRIO_HI();
                            const int ph = (tid < nact) ? b_sh.seg[tid].phase : 0;
                            const unsigned long long run = __ballot(ph == 1 || ph == 2);
                            if (tid < nact && ph != 1 && ph != 2) { b_sh.job[2 * tid].active = 0; b_sh.job[2 * tid + 1].active = 0; }
                            if (tid == 0) b_sh.nrunning = __popcll(run);
                            if (run != 0ull) blk_setup<TWO, NT, B, E1, E2, KTIGHT>(s0 + B, pen, njobs, tid);   // tables of the next pass
                            KPRIO_LO();
                        }
                    }
                    const unsigned long long q4 = KTICK();
                    // (a pass without a recompute or breakpoint detection ends at the control section's barrier: its wave-0
                    // section already wrote the next pass's tables; round 4: one barrier less for most passes)
                    if (p2_or_rec) __syncthreads();
                    tq_ph2 += q4 - q3; tq_tail += KTICK() - q4;
                    if (tid == 0) k_sh.dg_npass += 1ull;
                }
                // results into the list records
                if (tid < nact) {
                    BSeg &sg = b_sh.seg[tid];
                    GP<int> e = cur + (size_t)sg.list_pos * SR_BFS_SEGREC;
                    const int sp = sg.pe - sg.pb, st = sg.te - sg.tb;
                    const int bh = sg.bp_off_f, bv = sg.bp_off_f - sg.bp_k_f;
                    if (sg.phase != 3 || sg.bp_score == INT_MAX) atomicOr(&b_sh.err, SR_DEV_ERR_SCORE_BOUND);
                    else if (bv < 0 || bv > sp || bh < 0 || bh > st) atomicOr(&b_sh.err, SR_DEV_ERR_BREAKPOINT);
                    else {
                        e[SL_BV] = bv; e[SL_BH] = bh; e[SL_BCOMP] = sg.bp_comp; e[SL_BSF] = sg.bp_score_f; e[SL_BSR] = sg.bp_score_r;
                        // a primary that has a partner keeps the search for its secondary (sr_mirror_rule.h: the breakpoint record)
                        const int ri = k_sh.rp_nrec + tid;
                        if (k_sh.rp_record != 0 && ri < SR_BPREC_MAX) {
                            GP<int> r = (GP<int>)a.brec + (size_t)blockIdx.x * (SR_BPREC_MAX * SR_BPREC_INTS) + ri * SR_BPREC_INTS;
                            const unsigned long long cs = k_sh.cells_l[2 * tid] + k_sh.cells_l[2 * tid + 1] - (unsigned long long)(long long)k_sh.sg_sur[tid];
                            r[SR_BR_LEVEL] = k_sh.rp_level;
                            r[SR_BR_PB] = sg.pb; r[SR_BR_PE] = sg.pe; r[SR_BR_TB] = sg.tb; r[SR_BR_TE] = sg.te; r[SR_BR_CB] = sg.cb; r[SR_BR_CE] = sg.ce;
                            r[SR_BR_BV] = bv; r[SR_BR_BH] = bh; r[SR_BR_BCOMP] = sg.bp_comp; r[SR_BR_BSF] = sg.bp_score_f; r[SR_BR_BSR] = sg.bp_score_r;
                            r[SR_BR_TIE] = k_sh.sg_tie[tid];
                            r[SR_BR_CELLS_LO] = (int)(unsigned)cs; r[SR_BR_CELLS_HI] = (int)(unsigned)(cs >> 32);
                            r[SR_BR_PASSES] = k_sh.sg_done[tid] / B + 1;
                        }
                    }
                    if (k_sh.sg_tie[tid] != 0) { k_sh.rp_seg_tie = 1; if (k_sh.rp_level == 0) k_sh.rp_top_tie = 1; }
                }
                __syncthreads();
                if (tid == 0) {
                    if (k_sh.rp_record != 0) k_sh.rp_nrec += nact;       // (read by the lanes above, before the barrier)
                    if (k_sh.rp_on != 0) {
                        // the chunk as it would have run: all its segments for the passes of its longest search
                        const unsigned long long ran = k_sh.dg_npass - k_sh.rp_npass0;
                        const unsigned long long all = max(ran, (unsigned long long)k_sh.rp_maxp);
                        k_sh.dg_steps += 2ull * B * ((unsigned long long)k_sh.rp_ntot * all - (unsigned long long)nact * ran);
                    }
                }
                t_bp += KTICK() - tb0;
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
                k_sh.rp_level += 1;
            }
            __syncthreads();
            { GP<int> tmp = cur; cur = nxt; nxt = tmp; }
        }
        // ---------------- leaves in order: trivial ones are emitted directly, base cases in batches
        const unsigned long long tc0 = KTICK();
        // (row traffic so far was the ring's: from here to the end of the pair the tiles run on the base-case histories)
        if ((tid & 63) == 0) { k_sh.row_w[0][(tid >> 6) & 15] += row_ld; k_sh.row_w[1][(tid >> 6) & 15] += row_st; }
        row_ld = 0; row_st = 0;
        {
            const int n_cur = RFL(b_sh.list_n);
            if (tid == 0) b_sh.emit_pos = 0;
            __syncthreads();
            int pos = 0;
            while (pos < n_cur && RFL(b_sh.err) == 0) {
                __syncthreads();
                if (tid == 0) {
                    // A base case of a split segment ends at the score its half of the breakpoint carried (SL_REM), or one
                    // gap-open above it: its levels and -- through the reach of those levels -- its width are known.  Every job
                    // of a batch gets a region of its own in the workgroup's history, [its levels][component][its width], so
                    // a batch costs the sum of what its jobs need and not jobs x the widest x the deepest (the first job always
                    // fits: the host sizes hist_cap for a worst-case one).  A job that would run past the levels it was given
                    // is stopped before the block that would leave its region, and the batch is cut in front of it: the job is
                    // searched again as the first job of the next batch with the worst-case levels and width (SL_REM = -1
                    // marks it; round 4, ADVICE r3) -- only a job that outgrows THAT raises SR_DEV_ERR_BASE_OVERFLOW.
                    int nb = 0, p = pos, lmax = 0;
                    k_sh.redo_from = BJ_MAX;
                    unsigned long long used = 0;
                    for (; p < n_cur && nb < a.bbase_jobs; p++) {
                        GP<int> e = cur + (size_t)p * SR_BFS_SEGREC;
                        if (e[SL_KIND] != SK_BASE) continue;
                        const int sp = e[SL_PE] - e[SL_PB], st = e[SL_TE] - e[SL_TB], rem = e[SL_REM], ce = e[SL_CE];
                        // (measured on the oracle: a half that ends in a gap component pays the open the breakpoint's total
                        // counted once -- rem + o1 for I1 / D1, rem + o2 for I2 / D2 --, rem or less when it ends in M)
                        const int open_e = (ce == SR_C_M) ? 0 : ((ce == SR_C_I1 || ce == SR_C_D1) ? pen.o1 : (TWO ? pen.o2 : pen.o1));
                        int lj = a.hist_levels;                                   // levels the job may compute (whole blocks)
                        if (rem >= 0 && rem < a.hist_levels - 2 * B - open_e - 2) lj = ((rem + open_e + 2) / B + 1) * B;
                        if (rem >= 0 && a.test_base_levels > 0) lj = min(lj, ((a.test_base_levels + B - 1) / B) * B);   // (tests: force the re-queue)
                        const int Rj = kreach<TWO, E1, E2>(pen, lj, e[SL_CB]);
                        const int half = min(Rj + scope + 2, max(sp, st) + 2);
                        const int wj = min((2 * half + 1 + 8 + 8 * KGeo<B>::HL + 16 + 7) & ~7, a.hist_w);      // + halo groups either side
                        const unsigned long long need = (unsigned long long)lj * 5ull * (unsigned long long)wj;
                        if (nb > 0 && used + need > a.hist_cap) break;
                        kjob_set(nb, 0, e[SL_PB], e[SL_PE], e[SL_TB], e[SL_TE], 0, e[SL_CB], ce, nb, ks);
                        b_sh.job[nb].shift = wj / 2;
                        b_sh.job[nb].pad1 = lj;
                        b_sh.job[nb].hbase = (unsigned)used; b_sh.job[nb].hw = (unsigned)wj;
                        b_sh.base_entry[nb] = p; b_sh.base_score[nb] = -1;
                        used += need; lmax = max(lmax, lj);
                        nb++;
                    }
                    b_sh.nbase = nb; b_sh.next_pos = p; b_sh.njobs = nb; b_sh.nrunning = nb;
                    b_sh.geom.hist_levels = lmax;
                }
                __syncthreads();
                int nb = RFL(b_sh.nbase);
                pos = RFL(b_sh.next_pos);
                if (nb > 0) {
                    if (tid == 0) k_sh.dg_nbase += (unsigned long long)nb;
                    const int hlevels = RFL(b_sh.geom.hist_levels);
                    for (int s0i = 0; RFL(b_sh.nrunning) > 0; s0i += B) {
                        const int s0 = kopaque_s(s0i);
                        if (s0 + B > hlevels) { if (tid == 0) b_sh.err |= SR_DEV_ERR_BASE_OVERFLOW; break; }
                        blk_pass<OT, TWO, NT, B, E1, E2, PROF, X, OE1, OT, false, true>(RH, s0, pen, nb, row_ld, row_st, s0 == 0);
                        __syncthreads();
                        if (tid == 0) k_sh.dg_steps += (unsigned long long)b_sh.nrunning * B;
                        const int tid_o = tid;
                        if (tid < 64) {                          // one lane per base case: first level of the block that reached the end
                            const int tid = (int)kopaque_v((unsigned)tid_o);       // (per pass, as in the searches' control section)
                            KPRIO_HI();
                            bool running = false;
                            if (tid < nb && b_sh.job[tid].active) {
                                int hit = -1, jr[B];                 // the job's B reach flags: one batch of independent LDS reads
#pragma unroll
                                for (int l = 0; l < B; l++) jr[l] = k_sh.jreach[l][tid];
#pragma unroll
                                for (int l = B - 1; l >= 0; l--) if (jr[l]) hit = l;
                                if (hit >= 0) {
                                    b_sh.base_score[tid] = s0 + hit; b_sh.job[tid].active = 0;
                                    atomicAdd(&b_sh.cells, (unsigned long long)(-blk_surplus(pen, tid, s0 + hit, s0 + B - 1)));
                                } else if (s0 + 2 * B > b_sh.job[tid].pad1) {       // the next block would leave the job's levels / columns
                                    GP<int> e = cur + (size_t)b_sh.base_entry[tid] * SR_BFS_SEGREC;
                                    b_sh.job[tid].active = 0;                       // stopped here: nothing is written past its region
                                    if (e[SL_REM] < 0 || b_sh.job[tid].pad1 >= a.hist_levels) atomicOr(&b_sh.err, SR_DEV_ERR_BASE_OVERFLOW);
                                    else { e[SL_REM] = -1; atomicMin(&k_sh.redo_from, tid); atomicAdd(&k_sh.dg_redo, 1ull); }
                                } else running = true;
                            }
                            const unsigned long long rm = __ballot(running);
                            if (tid == 0) b_sh.nrunning = __popcll(rm);
                            if (rm != 0ull) blk_setup<TWO, NT, B, E1, E2, false, true>(s0 + B, pen, nb, tid);   // tables of the next pass (cone-clipped)
                            KPRIO_LO();
                        }
                        __syncthreads();
                    }
                    __syncthreads();
                    // a job outgrew its levels: this batch ends in front of it, the next one starts with it (worst-case region)
                    const int redo = RFL(k_sh.redo_from);
                    if (redo < nb) {
                        if (tid == 0) k_sh.dg_nbase -= (unsigned long long)(nb - redo);       // (searched again: counted by the next batch)
                        nb = redo; pos = RFL(b_sh.base_entry[redo]);
                    }
                    // one thread per base case: backtrace into its reversed op buffer
                    const unsigned long long tbt0 = KTICK();
                    if (tid < nb && RFL(b_sh.err) == 0) {
                        KPRIO_HI();
                        int n = 0;
                        const int e = bfs_backtrace<OT, TWO>(bhist + b_sh.job[tid].hbase, b_sh.job[tid].hw, tid, b_sh.base_score[tid],
                                                             btbuf + (size_t)tid * SR_BFS_BTCAP, &n);
                        b_sh.bt_n[tid] = n;
                        if (e & SR_MIRROR_BT_TIE) k_sh.mir_tie = 1;
                        if (e & ~SR_MIRROR_BT_TIE) atomicOr(&b_sh.err, e & ~SR_MIRROR_BT_TIE);
                        KPRIO_LO();
                    }
                    __syncthreads();
                    tb_bt += KTICK() - tbt0;
                }
                const unsigned long long tem0 = KTICK();
                // emit list entries [emit_pos, pos) in order: wave 0, with everything it decides on wave-uniform.  The run being
                // built stays in (scalar) registers -- adjacent runs of one op merge, also across segments --, finished runs are
                // stored by lane 0 without reading back, and the reversed op buffers of the base cases are read 64 ops per
                // round trip (one per lane) and handed to the uniform control flow by lane index.
                if (tid < 64 && RFL(b_sh.err) == 0) {
                    KPRIO_HI();
                    const int lane = tid;
                    int err = 0, bj = 0, pop = RFL(k_sh.pend_op), plen_ = RFL(k_sh.pend_len);
                    uint32_t cnt = RFL(b_sh.cig_cnt);
#define EMIT(OP, LEN)                                                                                   \
    do {                                                                                                \
        const int op_ = (OP), len_ = (LEN);                                                             \
        if (len_ > 0) {                                                                                 \
            if (op_ == pop) plen_ += len_;                                                              \
            else {                                                                                      \
                if (pop >= 0) { if (cnt >= cap) err |= SR_DEV_ERR_CIGAR_OVERFLOW; else { if (lane == 0) ops[cnt] = ((uint32_t)plen_ << 4) | (uint32_t)pop; cnt++; } } \
                pop = op_; plen_ = len_;                                                                \
            }                                                                                           \
        }                                                                                               \
    } while (0)
                    const int p_first = RFL(b_sh.emit_pos);
                    for (int p = p_first; p < pos; p++) {
                        GP<int> e = cur + (size_t)p * SR_BFS_SEGREC;
                        const int sp = RFL(e[SL_PE] - e[SL_PB]), st = RFL(e[SL_TE] - e[SL_TB]), kind = RFL(e[SL_KIND]);
                        if (kind == SK_TRIVIAL) {
                            if (st == 0) EMIT(SR_OP_D, sp);
                            else EMIT(SR_OP_I, st);
                        } else if (kind == SK_BASE) {
                            GP<uint32_t> b = btbuf + (size_t)bj * SR_BFS_BTCAP;
                            const int nbt = RFL(b_sh.bt_n[bj]);
                            for (int i = nbt - 1; i >= 0; i -= 64) {
                                const uint32_t v = (i - lane >= 0) ? b[i - lane] : 0u;
                                const int m = min(64, i + 1);
                                for (int u = 0; u < m; u++) {
                                    const uint32_t x = (uint32_t)__builtin_amdgcn_readlane((int)v, u);
                                    EMIT((int)(x & 15u), (int)(x >> 4));
                                }
                            }
                            bj++;
                        } else err |= SR_DEV_ERR_BACKTRACE;
                    }
#undef EMIT
                    if (lane == 0) {
                        b_sh.cig_cnt = cnt; b_sh.emit_pos = pos; k_sh.pend_op = pop; k_sh.pend_len = plen_;
                        if (err) b_sh.err |= err;
                    }
                    KPRIO_LO();
                }
                __syncthreads();
                tb_emit += KTICK() - tem0;
            }
            // the last run
            if (tid == 0 && b_sh.err == 0 && k_sh.pend_op >= 0) {
                uint32_t cnt = b_sh.cig_cnt;
                if (cnt >= cap) b_sh.err |= SR_DEV_ERR_CIGAR_OVERFLOW;
                else { ops[cnt++] = ((uint32_t)k_sh.pend_len << 4) | (uint32_t)k_sh.pend_op; b_sh.cig_cnt = cnt; }
            }
            __syncthreads();
        }
        t_base += KTICK() - tc0;
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
        // (read between the two barriers: past the second one thread 0 may already be resetting them for the next pair)
        const int p_err = RFL(b_sh.err), p_score = RFL(b_sh.score_acc), p_tie = RFL(k_sh.mir_tie);
        if (tid == 0) {
            a.is_reverse[pair] = is_rev ? 1 : 0;
            a.score[pair] = b_sh.err ? -1 : b_sh.score_acc;
            a.ori_fwd[pair] = fwd; a.ori_rev[pair] = rev;
            a.cigar_cnt[pair] = b_sh.err ? 0u : cnt;
            if (b_sh.err) atomicOr(a.error_flag, b_sh.err);
#ifdef SR_BOUNDS
            if (k_sh.bnd_flag == 1) {                         // first offender of the launch: pair, what, offset, extent
                k_sh.bnd_flag = 2;
                if (atomicCAS(&a.counters[40], 0ull, (unsigned long long)pair + 1ull) == 0ull) {
                    a.counters[41] = k_sh.bnd_what; a.counters[42] = k_sh.bnd_off; a.counters[43] = k_sh.bnd_ext;
                }
            }
#endif
        }
        __syncthreads();
        // ---------------- the pair's secondary: emitted by symmetry or queued for this workgroup
        const uint32_t mir = a.mirror ? a.mirror[pair] : SR_MIRROR_NONE;
        bool mir_emit = false;
        if (mir != SR_MIRROR_NONE && !(mir & SR_MIRROR_SECONDARY)) {
            // (orientation as its own kernel: the secondary's strand and orientation scores are already there, and stay)
            mir_emit = p_err == 0 && !is_rev && p_tie == 0 && !(a.pre_oriented && a.is_reverse[mir] != 0);
            if (mir_emit) {
                // the transposed CIGAR: I <-> D (op codes 2 and 3), same runs, into the secondary's own arena region
                // (the same reserve, |q| + |t| + 2 ops); the barrier above ordered the primary's ops
                GP<uint32_t> ops2 = (GP<uint32_t>)a.cigar_ops + a.cigar_base[mir];
                for (uint32_t i = tid; i < cnt; i += NT) { const uint32_t v = ops[i]; ops2[i] = v ^ ((v & 2u) >> 1); }
                if (tid < 64) {
                    // the secondary's tallies as the oracle counts them are its primary's: cells, levels, base cases, searches
                    unsigned long long cl = k_sh.cells_l[tid];
                    k_sh.cells_l[tid] = 0ull;
                    for (int o = 32; o > 0; o >>= 1) cl += __shfl_xor(cl, o, 64);
                    if (tid == 0) {
                        b_sh.cells += cl;
                        b_sh.cells += b_sh.cells - k_sh.mir_snap[0]; k_sh.dg_steps += k_sh.dg_steps - k_sh.mir_snap[1];
                        k_sh.dg_nbase += k_sh.dg_nbase - k_sh.mir_snap[2]; k_sh.dg_nbp += k_sh.dg_nbp - k_sh.mir_snap[3];
                        k_sh.mir_pairs += 1ull;
                        a.score[mir] = p_score; a.cigar_cnt[mir] = cnt;
                        if (!a.pre_oriented) { a.is_reverse[mir] = 0; a.ori_fwd[mir] = fwd; a.ori_rev[mir] = rev; }
                    }
                }
            } else if (tid == 0) {
                // aligned after all.  By this workgroup, next -- unless the queue is dry (or SR_TAIL=all): then nothing else would
                // start on this CU any more, and the secondary goes on the list of the wide tail launch that follows
                k_sh.mir_ties += 1ull;
                if (p_tie != 0) {                                // where the tie sits: the depth-0 search / in no search at all
                    if (k_sh.rp_top_tie != 0) k_sh.rp_tie_top += 1ull;
                    else if (k_sh.rp_seg_tie == 0) k_sh.rp_tie_base += 1ull;
                }
                // Replay: the primary kept its searches, ended well on the forward strand, and its depth-0 search decided nothing
                // by a tie -- the secondary takes the breakpoints of all untied searches from the records and is short: it runs
                // here, next, dry queue or not.  (SR_TAIL=all keeps deferring every tied secondary to a full alignment.)
                const bool replay = k_sh.rp_record != 0 && p_err == 0 && !is_rev && k_sh.rp_top_tie == 0 &&
                                    !(a.pre_oriented && a.is_reverse[mir] != 0) && a.tail_mode != SR_TAIL_DEFER_ALL;
                bool defer = false;
                if (!replay && a.tail_list && a.tail_mode != SR_TAIL_RUN)
                    defer = a.tail_mode == SR_TAIL_DEFER_ALL ||
                            __hip_atomic_load(a.queue_head, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= a.npairs;
                if (defer) { a.tail_list[atomicAdd(a.tail_count, 1u)] = mir; atomicAdd(a.tail_deferred, 1u); }
                else { k_sh.mir_next = (int)mir; k_sh.rp_ready = replay ? 1 : 0; }
            }
        }
        if (a.fuse_unite) {
            // unite the bases of the match runs (what sr_unite_kernel does for a pair, sr_uf.hip); same filter: aligned, and
            // the score within the divergence bound.  The CIGAR was stored by this workgroup and the barrier above orders it.
            const int sc = p_err ? -1 : p_score;
            if (sc >= 0 && sc <= a.max_score[pair]) {
                unsigned long long united = 0, runs = 0;
                int uerr = 0;
                uf_unite_cigar<NT>((const uint32_t *)a.cigar_ops + a.cigar_base[pair], cnt, a.seq_goff[q], a.seq_goff[t],
                                   (unsigned long long)plen, is_rev != 0, 0ull, 0ull, a.min_match_len, a.uf_nodes, united, runs, uerr);
                for (int o = 32; o > 0; o >>= 1) { united += __shfl_xor(united, o, 64); runs += __shfl_xor(runs, o, 64); }
                // (a secondary emitted by symmetry would unite exactly these base pairs again: only its tallies are added)
                if ((tid & 63) == 0) {
                    if (united) atomicAdd(&a.counters[4], mir_emit ? 2ull * united : united);
                    if (runs) atomicAdd(&a.counters[5], mir_emit ? 2ull * runs : runs);
                }
                if (uerr) atomicOr(a.error_flag, uerr);
            }
        }
        t_all += KTICK() - tk0;
        // (the wave's 64-bit sums live in LDS, not in registers across the pairs)
        if ((tid & 63) == 0) {
            k_sh.row_w[0][(tid >> 6) & 15] += row_ld; k_sh.row_w[1][(tid >> 6) & 15] += row_st;
            k_sh.row_w[2][(tid >> 6) & 15] += row_ld; k_sh.row_w[3][(tid >> 6) & 15] += row_st;      // (the histories' share)
        }
        row_ld = 0; row_st = 0;
    }
    if (tid < 64 && k_sh.cells_l[tid]) atomicAdd(&a.counters[0], k_sh.cells_l[tid]);
    if ((tid & 63) == 0) {                       // row traffic of this wave's tiles, in bytes
        const unsigned long long lane_bytes = 8ull;           // (the tiles count 8-byte units: 4 cells of 2 bytes)
        const unsigned long long row_ld_acc = k_sh.row_w[0][(tid >> 6) & 15], row_st_acc = k_sh.row_w[1][(tid >> 6) & 15];
        if (row_ld_acc) atomicAdd(&a.counters[16], row_ld_acc * lane_bytes);
        if (row_st_acc) atomicAdd(&a.counters[17], row_st_acc * lane_bytes);
        // of these, the base-case histories (the ring's share is the difference), the base cases' tiles and level-diagonals as
        // executed: the experiment slots [44..47]
        const unsigned long long hist_ld_acc = k_sh.row_w[2][(tid >> 6) & 15], hist_st_acc = k_sh.row_w[3][(tid >> 6) & 15];
        if (hist_ld_acc) atomicAdd(&a.counters[44], hist_ld_acc * lane_bytes);
        if (hist_st_acc) atomicAdd(&a.counters[45], hist_st_acc * lane_bytes);
    }
    if (tid == 0) {
        atomicAdd(&a.counters[0], b_sh.cells);
        atomicAdd(&a.counters[1], k_sh.dg_steps);
        atomicAdd(&a.counters[2], k_sh.dg_nbase);
        atomicAdd(&a.counters[3], k_sh.dg_nbp);
        atomicAdd(&a.counters[9], k_sh.dg_npass);
        atomicAdd(&a.counters[19], k_sh.dg_f); atomicAdd(&a.counters[20], k_sh.dg_c);
        atomicAdd(&a.counters[21], k_sh.dg_e); atomicAdd(&a.counters[22], k_sh.dg_r);
        if (k_sh.dg_redo) atomicAdd(&a.counters[37], k_sh.dg_redo);
        if (k_sh.mir_pairs) atomicAdd(&a.counters[38], k_sh.mir_pairs);
        if (k_sh.mir_ties) atomicAdd(&a.counters[39], k_sh.mir_ties);
        if (k_sh.rp_tie_top) atomicAdd(&a.counters[48], k_sh.rp_tie_top);
        if (k_sh.rp_tie_base) atomicAdd(&a.counters[49], k_sh.rp_tie_base);
        if (k_sh.rp_replays) atomicAdd(&a.counters[50], k_sh.rp_replays);
        if (k_sh.rp_cached) atomicAdd(&a.counters[51], k_sh.rp_cached);
        atomicAdd(&a.counters[46], k_sh.base_tiles); atomicAdd(&a.counters[47], k_sh.base_cells);
        if (PROF && a.timeline) {
            unsigned long long *tl = a.timeline + 4ull * blockIdx.x;
            tl[0] = tl_first; tl[1] = tl_last; tl[2] = KTICK(); tl[3] = tl_n | (tl_mir << 32);
        }
        if (PROF && a.prio_timeline) a.prio_timeline[4ull * blockIdx.x] = tl_end1;
        if (PROF) {
            if (!a.pre_oriented) atomicAdd(&a.counters[6], t_ori);    // ([6] holds sr_orient_kernel's cells otherwise)
            atomicAdd(&a.counters[7], t_bp);
            atomicAdd(&a.counters[8], t_base);
            atomicAdd(&a.counters[10], t_all);
            atomicAdd(&a.counters[11], tq_pass);
            atomicAdd(&a.counters[12], tq_bar);
            atomicAdd(&a.counters[13], k_sh.t_setup);
            atomicAdd(&a.counters[25], tq_ctl); atomicAdd(&a.counters[26], k_sh.t_c1); atomicAdd(&a.counters[27], k_sh.t_c2);
            atomicAdd(&a.counters[28], k_sh.t_p2a); atomicAdd(&a.counters[29], k_sh.t_p2f); atomicAdd(&a.counters[30], k_sh.t_p2e); atomicAdd(&a.counters[31], k_sh.t_p2w);
            atomicAdd(&a.counters[14], tq_ph2);
            atomicAdd(&a.counters[18], tq_rec);
            atomicAdd(&a.counters[23], tb_bt); atomicAdd(&a.counters[24], tb_emit);       // (of [8]: backtraces, ordered emission)                          // (of tq_ph2: the I/D recompute passes)
            atomicAdd(&a.counters[15], tq_tail);
        }
    }
#undef KTICK
}
