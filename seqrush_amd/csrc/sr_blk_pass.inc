// sr_blk_pass.inc -- blocked kernel (sr_align_blk.inc), part 3: a pass over a block of levels -- reach and tile windows
// (kreach, kwindow), the pass tables (blk_setup), the tile queue (blk_pass), the I/D recompute pass (blk_recompute).
#include "sr_base_cone.h"       // backward cone of a base case (shared with the host twin)
#include "sr_prio_rule.h"       // rotating tile priority of co-resident workgroups (shared with the host twin)
#include "sr_pass_rule.h"       // the tables of a pass: reach, ranges, cone clip, cells, tile windows (shared with the host twin)
// reach() with compile-time gap-extends (the host guarantees pen.e1 == E1, pen.e2 == E2): no runtime division
template <bool TWO, int E1, int E2>
__device__ __forceinline__ int kreach(const SrPen &p, int s, int begin) {
    return sr_pass_reach(p.o1, E1, p.o2, E2, TWO, s, begin == SR_C_M);
}

// Groups [glo, ghi] the tiles of block s0 (levels s0 .. s0+B-1) of aligner b cover -- and store (sr_pass_window).
//  * wide (round 1-3, still used by base-case histories and the generic instances): the last level's range + scope + 1
//    diagonals either side, so that every later reader (levels up to scope + B above, one neighbour diagonal) finds NULL
//    beyond the range instead of whatever the ring slot held before: 2 (scope + 1) = 54 extra diagonals per aligner and
//    level for the default penalties -- 9 % of all tile lanes on C2, more the deeper the recursion (narrow segments).
//  * TIGHT (round 4, ring tiles of the exact instance): the last level's range + the one neighbour diagonal.  What lies
//    outside is never written and may hold anything; a tile that reads a source block (s0 - B: M[s - o1 - e1], M[s - x], the
//    chain sources; the one or two blocks M[s - o2 - e2] comes from) masks the lanes outside THAT block's coverage to NULL
//    (blk_tile16: `in10 / in2a / in2b`; a tile whose 64 lanes lie inside the narrowest source coverage skips the masks),
//    breakpoint detection tests every cell against its level's range anyway.
template <bool TWO, int B, int E1, int E2, bool TIGHT>
__device__ __forceinline__ void kwindow(const SrPen &pen, const BJob &b, int s0, int &glo, int &ghi) {
    int nt;
    sr_pass_window(kreach<TWO, E1, E2>(pen, s0 + B - 1, b.begin), TIGHT ? 1 : pen.scope + 1, b.plen, b.tlen, b.shift, false, 0, 0,
                   KGeo<B>::OWN, glo, ghi, nt);
}

// One pass: levels s0 .. s0+B-1 of every active aligner.  Ends with the data of the
// pass still in flight: the caller's __syncthreads() publishes rows and reductions.
#define KTICK() (PROF ? __builtin_amdgcn_s_memrealtime() : 0ull)
// Sections that one wave (or one lane) runs while the workgroup's other waves wait at the barrier are the pair's critical
// path, and the SIMD they run on is shared with three waves of other workgroups that are usually in their tiles: raised
// issue priority (s_setprio) lets the lone wave through first; back to 0 before the barrier.
// The tile code does not run at 0 but at the workgroup's role of the pass (sr_prio_rule.h): the waves of the workgroups of a
// CU share the SIMDs one each, issue is arbitrated by priority, then by age, and the workgroups are persistent -- at equal
// priority the workgroup dispatched last would be served last for the whole launch.  s_setprio takes an immediate and
// ignores EXEC: a switch over a wave-uniform value (scalar branches), never a lane condition.
__device__ __forceinline__ void kprio_role() {
    switch (RFL(k_sh.prio_role)) {
    case 1: __builtin_amdgcn_s_setprio(1); break;
    case 2: __builtin_amdgcn_s_setprio(2); break;
    case 3: __builtin_amdgcn_s_setprio(3); break;
    default: __builtin_amdgcn_s_setprio(0); break;
    }
}
// wave 0, once per pass (blk_setup): the role of the next pass from the workgroup's rank and the real-time counter.  The
// counter is the same on every CU, so co-resident workgroups change roles together.  Rule off: no clock read, role stays 0.
// (Issuing the read at the start of the caller's section and consuming it here was measured and did not pay: the next LDS
// wait has to wait for the scalar read as well, DESIGN.md 6.1.)
__device__ __forceinline__ void kprio_epoch() {
    const int wg = RFL(k_sh.prio_wg);
    if (wg > 1) {
        const unsigned epoch = (unsigned)(__builtin_amdgcn_s_memrealtime() >> SR_PRIO_EPOCH_SHIFT);
        if (threadIdx.x == 0) k_sh.prio_role = sr_tile_prio_role((unsigned)k_sh.prio_rank, epoch, (unsigned)wg);
    }
}
#define KPRIO_HI() __builtin_amdgcn_s_setprio(3)
#define KPRIO_LO() kprio_role()
// Tables of one pass (levels s0 .. s0+B-1 of every active aligner): wave 0.  The first pass of a batch
// of searches runs it inside blk_pass; later passes get their tables from the wave-0 section that ends the previous pass
// (control, or the section after breakpoint detection), so a pass costs one barrier and one serial hop less.
// The section is the pair's critical path and mostly serves two aligners (a depth-0 search), so nothing in it is a loop
// over the block's levels (sr_pass_rule.h): the per-level tables are written one (aligner, level) pair per lane, 64 / B
// aligners per step, the per-aligner ones one aligner per lane from the block's first and last level alone, and the tile
// prefix is a DPP scan.  tid: the caller's opaque copy of the thread index (< 64).
// BASE: the aligners are base cases.  Each knows its end diagonal (kend) and the levels it was given (pad1 = lj), so every
// level's range, and the tile window with it, is intersected with the backward cone of the end (sr_base_cone.h): cells outside
// it cannot lie on a path to the end, are not computed (NULL inside the window) and not stored.  The window keeps the wide
// margin on its forward sides: a reader in the cone reads neighbours in the (wider) cone of the source level, which lie
// within the source block's forward range + scope + 1 as before, so inside its window.  A job whose clipped range is empty
// gets no tiles (it cannot end within its levels and is re-queued or fails as before).
// The cells counted (cells_l -> counters[0], b_sh.cells, blk_surplus) stay those of the UNCLIPPED ranges, as the oracle
// counts them; tiles and row bytes are counted as executed (base_tiles / base_cells: the clipped figures).
#ifndef SR_BASE_CONE
#define SR_BASE_CONE 1             // (0: A/B build that computes the full forward triangle, as before)
#endif
// inclusive prefix sum over the first BJ_MAX lanes of a full wave (lanes past them hold 0)
__device__ __forceinline__ int kscan_jobs(int v) {
    static_assert(BJ_MAX <= 32 && BJ_MAX % 4 == 0, "kscan_jobs: at most two DPP rows of aligners");
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, true);      // row_shr:1, 2, 4, 8 (zero-filled): the scan of a row of 16
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, true);
    if (BJ_MAX > 8) v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, true);
    if (BJ_MAX > 16) v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);   // row_bcast:15 into rows 1 and 3
    return v;
}
template <bool TWO, int NT, int B, int E1, int E2, bool TIGHT = false, bool BASE = false>
__device__ __forceinline__ void blk_setup(int s0, const SrPen &pen, int njobs, const int tid) {
    constexpr bool CONE = BASE && SR_BASE_CONE;
    if (tid < BJ_MAX) {        // (cleared per aligner lane: 16-byte stores over the flat tables were measured and did not pay)
#pragma unroll
        for (int j = 0; j < B; j++) { k_sh.jak[j][tid] = 0; k_sh.jreach[j][tid] = 0; }
    }
    if (BASE) {
        // base cases: one lane per job, its levels one after the other -- a batch keeps up to 16 lanes busy, and by (job, level)
        // lanes it took three steps and an LDS add per level (measured: the base cases' section 6 % slower, profiles/pass_ctl_ab.log)
        if (tid < njobs && b_sh.job[tid].active) {
            const BJob &b = b_sh.job[tid];
            int cells = 0, ccells = 0;
#pragma unroll
            for (int j = 0; j < B; j++) {
                const int rb = CONE ? sr_cone_reach(E1, E2, TWO, b.pad1 - 1 - (s0 + j)) : 0;      // (< 0 past the job's levels: empty)
                int klo, khi, c, cc;
                sr_pass_level(kreach<TWO, E1, E2>(pen, s0 + j, b.begin), b.plen, b.tlen, CONE, CONE ? b.kend : 0, rb, klo, khi, c, cc);
                k_sh.jklo[j][tid] = klo; k_sh.jkhi[j][tid] = khi;
                cells += c; ccells += cc;
            }
            k_sh.cells_l[tid] += (unsigned long long)cells;
            if (ccells) atomicAdd(&k_sh.base_cells, (unsigned long long)ccells);
        }
    } else {
        // searches: range and cells per level -- lanes enumerate (aligner, level) pairs
        const int steps = sr_pass_steps(njobs, B);
        for (int st = 0; st < steps; st++) {
            int a, j;
            if (sr_pass_lane(tid, st, B, a, j) && a < njobs && b_sh.job[a].active) {
                const BJob &b = b_sh.job[a];
                int klo, khi, cells, ccells;
                sr_pass_level(kreach<TWO, E1, E2>(pen, s0 + j, b.begin), b.plen, b.tlen, false, 0, 0, klo, khi, cells, ccells);
                k_sh.jklo[j][a] = klo; k_sh.jkhi[j][a] = khi;
                if (cells) atomicAdd(&k_sh.cells_l[a], (unsigned long long)cells);
            }
        }
    }
    // per aligner: window, tiles
    int nt = 0, glo = 0, ghi = -1;
    const bool act = tid < njobs && b_sh.job[tid].active;
    const int pglo = (tid < BJ_MAX) ? k_sh.jglo[tid] : 0, pghi = (tid < BJ_MAX) ? k_sh.jghi[tid] : -1;
    if (act) {
        const BJob &b = b_sh.job[tid];
        const int rb0 = CONE ? sr_cone_reach(E1, E2, TWO, b.pad1 - 1 - s0) : 0;                // the block's widest cone
        sr_pass_window(kreach<TWO, E1, E2>(pen, s0 + B - 1, b.begin), TIGHT ? 1 : pen.scope + 1, b.plen, b.tlen, b.shift, CONE,
                       CONE ? b.kend : 0, rb0, KGeo<B>::OWN, glo, ghi, nt);
    }
    const int incl = kscan_jobs(nt);
    if (tid < BJ_MAX) {
        k_sh.jglo[tid] = glo; k_sh.jghi[tid] = ghi;
        k_sh.jgplo[tid] = pglo; k_sh.jgphi[tid] = pghi;
        k_sh.jtstart[tid + 1] = incl;
    }
    // (the queue's start as an opaque copy: as a plain constant it was kept in a register across the pass loop, spilled, and
    //  reloaded here, a memory round trip for a literal)
    if (tid == 0) { k_sh.jtstart[0] = 0; k_sh.next_tile = (int)kopaque_v((unsigned)(NT / 64)); }
    if (tid == BJ_MAX - 1) { k_sh.total_tiles = incl; if (BASE) k_sh.base_tiles += (unsigned long long)incl; }
    kprio_epoch();
}

template <typename OT, bool TWO, int NT, int B, int E1, int E2, bool PROF, int X = 0, int OE1 = 0, typename ST = OT, bool RING = false, bool BASE = false>
__device__ __forceinline__ void blk_pass(const KRows<OT, ST> &R, int s0, const SrPen &pen, int njobs,
                                         unsigned &row_ld, unsigned &row_st, const bool setup = true) {
    const int tid = threadIdx.x;
    if (setup) {
        const unsigned long long tsu0 = KTICK();
        if (tid < 64) blk_setup<TWO, NT, B, E1, E2, RING && KTIGHT_OF(OT, ST, B, X), BASE>(s0, pen, njobs, (int)kopaque_v((unsigned)tid));
        __syncthreads();
        if (PROF && threadIdx.x == 0) k_sh.t_setup += KTICK() - tsu0;
    }
    kprio_role();                                        // every wave: the pass's tiles at the workgroup's role
    const int total = RFL(k_sh.total_tiles);
    const int slot0 = kslots(R, s0);
    // Tiles differ in cost (extension loops, edge tiles): every wave takes its first tile by index and the following
    // ones from a queue, so that the pass ends when the work does and not when the unluckiest wave's share does.
    for (int t = (tid >> 6); t < total;) {
        int hi = njobs, lo = 0;                     // last aligner with jtstart <= t (wave-uniform)
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (RFL(k_sh.jtstart[mid]) <= t) lo = mid; else hi = mid; }
        const int ti = t - RFL(k_sh.jtstart[lo]);
        blk_tile_any<OT, TWO, B, E1, E2, false, X, OE1, ST, RING>(R, s0, slot0, pen, lo, ti, lo, row_ld, row_st);
        int nx = 0;
        if ((tid & 63) == 0) nx = atomicAdd(&k_sh.next_tile, 1);
        t = RFL(nx);
    }
}

// Segment sa has just entered phase 2: recompute and store the I/D rows of the levels breakpoint detection will
// read (the scope window below the entry level, up to the end of the current block), block by block from the last
// block boundary before the window -- its chain sources, the previous block's last e levels, are always stored.
// Needs the M rows down to (window start - scope): ring depth >= 2 * scope + 2 * B + 2.
template <typename OT, bool TWO, int NT, int B, int E1, int E2, int X = 0, int OE1 = 0, typename ST = OT>
__device__ __forceinline__ void blk_recompute(const KRows<OT, ST> &R, const SrPen &pen, int sa, int entry_level, int s0_now,
                                              unsigned &row_ld, unsigned &row_st) {
    const int tid = threadIdx.x;
    const int wlo = max(0, entry_level - pen.scope);
    for (int blk = (wlo / B) * B; blk <= s0_now; blk += B) {
        __syncthreads();
        if (tid < 2) {
            const BJob &b = b_sh.job[2 * sa + tid];
            int Rw = 0;
#pragma unroll
            for (int j = 0; j < B; j++) {
                Rw = kreach<TWO, E1, E2>(pen, blk + j, b.begin);
                k_sh.jklo[j][BJ_MAX + tid] = max(-b.plen, -Rw); k_sh.jkhi[j][BJ_MAX + tid] = min(b.tlen, Rw);
            }
            (void)Rw;
            int glo, ghi;
            kwindow<TWO, B, E1, E2, KTIGHT_OF(OT, ST, B, X)>(pen, b, blk, glo, ghi);      // (the coverage the block's own pass had)
            const bool first = blk == (wlo / B) * B;        // U starts from NULL in the first recompute block
            k_sh.jgplo[BJ_MAX + tid] = first ? 1 : k_sh.jglo[BJ_MAX + tid];
            k_sh.jgphi[BJ_MAX + tid] = first ? 0 : k_sh.jghi[BJ_MAX + tid];
            k_sh.jglo[BJ_MAX + tid] = glo; k_sh.jghi[BJ_MAX + tid] = ghi;
            const int nt = (ghi - glo + KGeo<B>::OWN) / KGeo<B>::OWN;
            const int n0 = __shfl(nt, 0, 64), n1 = __shfl(nt, 1, 64);
            if (tid == 0) { k_sh.rt_n0 = n0; k_sh.rt_total = n0 + n1; }
        }
        __syncthreads();
        const int n0 = RFL(k_sh.rt_n0), total = RFL(k_sh.rt_total);
        const int slot0 = kslots(R, blk);
        for (int t = (tid >> 6); t < total; t += NT / 64) {
            const int side = (t >= n0) ? 1 : 0;
            blk_tile_any<OT, TWO, B, E1, E2, true, X, OE1, ST, true>(R, blk, slot0, pen, 2 * sa + side, t - (side ? n0 : 0), BJ_MAX + side, row_ld, row_st);
        }
    }
    __syncthreads();
    if (tid < 2) b_sh.job[2 * sa + tid].pad2 = 1;           // from now on the search stores its I/D rows
}

// cells of levels (l0, l1] of aligner jid -- work a block computed past the aligner's last level
__device__ __forceinline__ long long blk_surplus(const SrPen &pen, int jid, int l0, int l1) {
    const BJob &b = b_sh.job[jid];
    long long c = 0;
    for (int l = l0 + 1; l <= l1; l++) {
        const int Rw = reach(pen, l, b.begin);
        const int klo = max(-b.plen, -Rw), khi = min(b.tlen, Rw);
        c += (khi >= klo) ? khi - klo + 1 : 0;
    }
    return c;
}
