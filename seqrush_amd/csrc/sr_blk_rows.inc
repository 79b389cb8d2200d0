// sr_blk_rows.inc -- blocked kernel (sr_align_blk.inc), part 1: the kernel's LDS state (KShared), row storage (KRows),
// row addressing, row loads and stores, DPP lane helpers and the tile geometry (KGeo).
#include "sr_pass_rule.h"       // tile geometry and pass tables shared with the host twin
#define SR_ORI_B 16                // levels per pass of the in-kernel orientation (default orientation penalties; round 4: 8 -> 16)
#define SR_KB_MAX 10               // deepest block any alignment instance of this build computes per pass (static LDS tables)
#define KB_LV (SR_ORI_B > SR_KB_MAX ? SR_ORI_B : SR_KB_MAX)      // levels of the per-level range / reach tables (orientation blocks may be deeper)
#define KB_MAX SR_KB_MAX
// packed tile on the 16-bit ring of a 32-bit search / tight ring cover (kwindow): exact 10-level instances with 16-bit cells
#define KPK_U16_OF(OT, ST, B, X) (sizeof(OT) == 4 && sizeof(ST) == 2 && (X) > 0 && (B) % 10 == 0)
#define KTIGHT_OF(OT, ST, B, X) ((X) > 0 && (B) % 10 == 0 && (sizeof(OT) == 2 || KPK_U16_OF(OT, ST, B, X)))

struct KShared {
    int jklo[KB_LV][BJ_MAX + 2], jkhi[KB_LV][BJ_MAX + 2];     // (+2: the aligners of an I/D recompute pass)
    alignas(8) int jak[KB_MAX][BJ_MAX];                       // (8-byte aligned: the control lanes read a segment's two aligners as a pair)
    int jreach[KB_LV][BJ_MAX];
    int jtstart[BJ_MAX + 1], jglo[BJ_MAX + 2], jghi[BJ_MAX + 2];
    unsigned newmask;                                  // segments that entered phase 2 in this pass
    int rt_n0, rt_total;                               // recompute pass: tiles of its first aligner, of both
    int jgplo[BJ_MAX + 2], jgphi[BJ_MAX + 2];                  // groups the previous block of the aligner covered (U row validity)
    int total_tiles;
    int next_tile;                                     // tile queue of a pass: the next tile nobody has taken yet
    // rotating tile priority (sr_prio_rule.h): the s_setprio level of the pass's tile code (blk_setup writes it, 0 when the
    // rule is off), the workgroup's rank on its CU, the workgroups per CU the rule runs with (0: off, nothing reads the clock)
    int prio_role, prio_rank, prio_wg;
    // batched breakpoint detection (phase 2) of one pass: up to K_P2 segments, <= 2*KB_MAX overlap calls each
    int p2n, p2seg[K_P2];
    unsigned p2mask_lo, p2mask_hi;
    int pc_n[K_P2], pc_s1[K_P2][2 * KB_MAX];            // calls of a segment; the other aligner's level of each
    unsigned char pc_side[K_P2][2 * KB_MAX];
    signed char pc_idx[K_P2][2][KB_MAX];               // call index of (side, level of the block) or -1
    unsigned long long pc_best[K_P2][2 * KB_MAX];
    unsigned long long pc_best_t[K_P2][2 * KB_MAX];    // the same call as the transposed pair would decide it (sr_mirror_rule.h)
    int pu_start[2 * K_P2 + 1], pu_glo[2 * K_P2];
    int pu_kmin[2 * K_P2], pu_kmax[2 * K_P2];          // band of diagonals of a filter unit (segment, side) that passed the filter at some level
    int cl_n;
#ifdef SR_BOUNDS
    unsigned lds_seq_bytes;                                // dynamic LDS of the workgroup: four sequence copies + read slack
    int bnd_flag; unsigned bnd_off, bnd_ext, bnd_what;     // first offending access of the workgroup (offset, extent, what: 1 ring / 2 history row, 3 LDS window)
#endif
    // mirrored emission (sr_align_blk.inc): the pair in hand had a tie-sensitive decision; the secondary this workgroup aligns
    // next (-1: none, take a pair from the queue); the pair's counters [0..3] as they stood when it began
    int mir_tie, mir_next;
    unsigned long long mir_snap[4];
    unsigned long long mir_pairs, mir_ties;    // secondaries emitted by symmetry / aligned after all -> counters[38], [39]
    // replay of a tied secondary (sr_mirror_rule.h, DESIGN.md 4.3).  Per segment of the chunk: a tie-sensitive accepted call,
    // the surplus cells stage W took off, the first level of the block in which its search ended
    int sg_tie[SR_BFS_MAXACT], sg_sur[SR_BFS_MAXACT], sg_done[SR_BFS_MAXACT];
    int rp_record, rp_on, rp_ready;    // the pair in hand: writes records / takes breakpoints from them; the records suit mir_next
    int rp_level, rp_nrec, rp_rd;      // recursion level, records written, the walk's position in them
    int rp_top_tie, rp_seg_tie;        // the pair's depth-0 search / any of its searches was tie-sensitive
    int rp_ntot, rp_maxp;              // chunk of a replaying pair: its segments solved ones included, most passes a solved one took
    unsigned long long rp_npass0;      // dg_npass when the chunk began
    unsigned long long rp_replays, rp_cached, rp_tie_top, rp_tie_base;   // -> counters[50], [51], [48], [49]
    int redo_from;                     // base cases: first job of the batch that outgrew the levels it was given (BJ_MAX: none)
    int pend_op, pend_len;             // CIGAR emission: the run being built (not yet stored)
    unsigned long long row_w[4][16];   // per wave, lane accesses of its tiles' row loads / stores (summed when the kernel ends); [2..3]: the base-case histories' share
    unsigned long long base_tiles, base_cells;   // base cases: tiles really run, level-diagonals really computed (cone-clipped; cells_l counts the unclipped ranges)
    unsigned long long cells_l[64];    // wavefront cells per lane of wave 0 (= aligner), summed when the kernel ends
    unsigned long long t_c1, t_c2;                           // PROF: control section: max_ak stores, per-segment control
    unsigned long long t_setup, t_p2a, t_p2f, t_p2e, t_p2w;     // PROF: ticks of the set-up sections, of breakpoint detection's stages
    unsigned long long dg_steps, dg_nbase, dg_nbp, dg_npass;   // levels x aligners advanced, base cases, breakpoint searches, passes (lane 0 of wave 0 adds)
    unsigned long long dg_f, dg_c, dg_e, dg_r;         // breakpoint detection: filter units, candidates, exact-test units, rounds
    unsigned long long dg_redo;                        // base cases searched again with the worst-case region (outgrew their levels)
};
__shared__ KShared k_sh;

// Row storage of a workgroup.  A row (one component of one level) is addressed by a row offset (uniform) plus a
// lane part that depends on the diagonal only:  element = rowoff(level, component) + klane(idx),
//     rowoff = component * cstr + slot(level) * sstr,   klane(idx) = (idx >> 8) * chs + (idx & 255).
//  * ring (breakpoint searches): chunk-major -- the 256-cell pieces (64 groups, one wave access) of all rows that
//    cover the same diagonals are stored together, a component's levels next to each other (cstr = depth * 256,
//    sstr = 256, chs = rows * 256).  The 10 M rows a tile loads as M[s-10] are then ten adjacent 512-byte pieces, the
//    10 it stores likewise: runs of adjacent rows sustain 5.0-5.2 TB/s where rows 10+ KB apart reach 3.7
//    (scripts/calib/chunk.hip, profiles/r02_chunk_locality.json).
//  * base-case history: plain rows [level][component][diagonal] (cstr = w, sstr = 5 w, chs = 256: klane(idx) = idx),
//    the layout the backtrace of sr_align_bfs.inc reads.
// One uniform 64-bit base per workspace + 32-bit offsets: the accesses take the "saddr" form, a row costs one SGPR
// (a 64-bit address per row would cost a pair each: 42 rows per 10-level tile, i.e. a tile living on spilled SGPRs).
// The host keeps a workspace below 4 GB.
// ST = storage type of the cells.  ST == OT, or (ring of 32-bit searches whose longest sequence is < 57 k) uint16_t
// holding offset - SR_RING_BIAS as a signed 16-bit value (see below): the rows are half the bytes (C5 is bound by them).
template <typename OT, typename ST = OT>
struct KRows {
    GP<ST> base;
    unsigned cM, cst2, sstr, chs;      // component c's rows start at (c ? cM + (c - 1) * cst2 : 0); slot stride; chunk stride of klane()
    unsigned urow, nuloff, trash;      // row offsets of the U row (0 = none), the NULL row, 256 cells nobody reads
    int depth, depth2;                 // ring depth of the M rows / of the I and D rows (round 3: the latter only span
                                       // breakpoint detection's window, scope + 2 B + 2 levels: 269 rows instead of 373)
    bool perjob;                       // base-case history: every job has its own region and row width (BJob hbase / hw)
    unsigned extent;                   // cells of the workgroup's region (bounds-checked build: every access is tested against it)
};
// ---- bounds-checked debug build (-DSR_BOUNDS: libseqrush_amd_bounds.so, csrc/Makefile; VERDICT r3 item 3) ---------------
// Every row access (ring and base-case history, 4 cells from `cell`) is tested against the workgroup's extent and every LDS
// window address of a live cell against the sequence region; an offender sets SR_DEV_ERR_ADDRESS, is recorded (first one per
// workgroup -> counters[40..43]: pair, what << 28 | level, offset, extent) and does NOT touch memory: loads return NULL
// cells, stores are dropped.  Costs ~15 % of kernel time; production builds carry none of it.
#ifdef SR_BOUNDS
__device__ __forceinline__ void kbnd_fail(unsigned what, unsigned off, unsigned ext) {
    atomicOr(&b_sh.err, SR_DEV_ERR_ADDRESS);
    if (atomicCAS(&k_sh.bnd_flag, 0, 1) == 0) { k_sh.bnd_off = off; k_sh.bnd_ext = ext; k_sh.bnd_what = what; }
}
#define SR_BND_OK(R, CELL, WHAT) (((CELL) + 3u < (R).extent) ? true : (kbnd_fail((WHAT), (CELL), (R).extent), false))
#else
#define SR_BND_OK(R, CELL, WHAT) true
#endif
// per-tile addressing context (all wave-uniform)
struct KAdr { unsigned hb, cM, cst2, sst; int slotM, slotD, depth, depth2; };
template <typename OT, typename ST>
__device__ __forceinline__ KAdr kadr(const KRows<OT, ST> &R, const BJob &jb, int slots) {
    KAdr A;
    if (R.perjob) { const unsigned hw = RFL(jb.hw); A.hb = RFL(jb.hbase); A.cM = hw; A.cst2 = hw; A.sst = 5u * hw; }
    else { A.hb = 0u; A.cM = R.cM; A.cst2 = R.cst2; A.sst = R.sstr; }
    A.slotM = slots & 0xffff; A.slotD = (int)((unsigned)slots >> 16); A.depth = R.depth; A.depth2 = R.depth2;
    return A;
}
// the two ring slots of level s packed into one int (M rows: low half, I / D rows: high half)
template <typename OT, typename ST>
__device__ __forceinline__ int kslots(const KRows<OT, ST> &R, int s) { return (s % R.depth) | ((s % R.depth2) << 16); }
// 16-bit ring of a 32-bit search (longest sequence < 57 k): a cell holds offset - SR_RING_BIAS as a SIGNED 16-bit value
// (round 3 stored offset + 8192 unsigned -- the same bits with the top one flipped).  NULL (-8192) is -32768, the smallest
// value, offsets up to 57343 fit, and -- the point of the signed form -- the packed 16-bit tile runs on the rows as they are
// (signed packed max / saturating subtract for the limit test; blk_tile16<.., BIAS = SR_RING_BIAS>): no conversion at a
// load or store, half the VALU of the 32-bit tile.  32-bit readers (breakpoint detection, control) add the bias back.
#define SR_RING_BIAS 24576
typedef short __attribute__((ext_vector_type(4))) S4;
template <typename OT, typename ST> __device__ __forceinline__ V4<OT> kcvt_in(V4<ST> v) {
    if constexpr (sizeof(ST) == sizeof(OT)) return v;
    else { const V4<OT> b = {SR_RING_BIAS, SR_RING_BIAS, SR_RING_BIAS, SR_RING_BIAS}; return __builtin_convertvector((S4)v, V4<OT>) + b; }
}
template <typename OT, typename ST> __device__ __forceinline__ V4<ST> kcvt_out(V4<OT> v) {
    if constexpr (sizeof(ST) == sizeof(OT)) return v;
    else { const V4<OT> b = {SR_RING_BIAS, SR_RING_BIAS, SR_RING_BIAS, SR_RING_BIAS}; return (V4<ST>)__builtin_convertvector(v - b, S4); }
}

// ring slot of level s0 + d, given slot0 = s0 mod depth and |d| < depth
__device__ __forceinline__ unsigned kslot(int slot0, int d, int depth) {
    int t = slot0 + d;
    t += (t < 0) ? depth : 0;
    t -= (t >= depth) ? depth : 0;
    return (unsigned)t;
}
template <typename OT, typename ST>
__device__ __forceinline__ unsigned klane(const KRows<OT, ST> &R, unsigned idx) { return (idx >> 8) * R.chs + (idx & 255u); }
template <typename OT, typename ST>
__device__ __forceinline__ unsigned krow_rel(const KRows<OT, ST> &R, const KAdr &A, int s0, int lvl, int c) {
    if (lvl < 0) return R.nuloff;
    if (c == SR_C_M) return A.hb + kslot(A.slotM, lvl - s0, A.depth) * A.sst;
    return A.hb + A.cM + (unsigned)(c - 1) * A.cst2 + kslot(A.slotD, lvl - s0, A.depth2) * A.sst;
}
// absolute level of the ring (breakpoint detection, walk)
template <typename OT, typename ST>
__device__ __forceinline__ unsigned krow_abs(const KRows<OT, ST> &R, int lvl, int c) {
    if (c == SR_C_M) return (unsigned)(lvl % R.depth) * R.sstr;
    return R.cM + (unsigned)(c - 1) * R.cst2 + (unsigned)(lvl % R.depth2) * R.sstr;
}
// row `slot` of component c of the ring (in-kernel orientation: fixed slots)
template <typename OT, typename ST>
__device__ __forceinline__ unsigned krow_fix(const KRows<OT, ST> &R, int c, int slot) {
    return (c == SR_C_M ? 0u : R.cM + (unsigned)(c - 1) * R.cst2) + (unsigned)slot * R.sstr;
}
// li = klane(idx) of the lane's first cell (4 cells of a group never straddle a 256-cell piece)
#define SR_ROWPTR(R, OFF, LI) ((V4<ST> __attribute__((address_space(1))) *)((char __attribute__((address_space(1))) *)(R).base + (((OFF) + (LI)) * (unsigned)sizeof(ST))))
#define SR_BND_WHAT(R) ((R).perjob ? 2u : 1u)
template <typename OT> __device__ __forceinline__ V4<OT> knull4() { const V4<OT> n = {(OT)NULLV, (OT)NULLV, (OT)NULLV, (OT)NULLV}; return n; }
template <typename OT, typename ST> __device__ __forceinline__ V4<OT> rld(const KRows<OT, ST> &R, unsigned off, unsigned li) {
    if (!SR_BND_OK(R, off + li, SR_BND_WHAT(R))) return knull4<OT>();
    return kcvt_in<OT, ST>(*SR_ROWPTR(R, off, li));
}
template <typename OT, typename ST> __device__ __forceinline__ V4<OT> rld_nt(const KRows<OT, ST> &R, unsigned off, unsigned li) {
    if (!SR_BND_OK(R, off + li, SR_BND_WHAT(R))) return knull4<OT>();
    return kcvt_in<OT, ST>(__builtin_nontemporal_load(SR_ROWPTR(R, off, li)));
}
template <typename OT, typename ST> __device__ __forceinline__ void rst(const KRows<OT, ST> &R, unsigned off, unsigned li, V4<OT> v) {
    if (!SR_BND_OK(R, off + li, SR_BND_WHAT(R))) return;
    *SR_ROWPTR(R, off, li) = kcvt_out<OT, ST>(v);
}
template <typename OT, typename ST> __device__ __forceinline__ void rst_nt(const KRows<OT, ST> &R, unsigned off, unsigned li, V4<OT> v) {
    if (!SR_BND_OK(R, off + li, SR_BND_WHAT(R))) return;
    __builtin_nontemporal_store(kcvt_out<OT, ST>(v), SR_ROWPTR(R, off, li));
}
// one cell
template <typename OT, typename ST> __device__ __forceinline__ int rcell(const KRows<OT, ST> &R, unsigned off, int idx) {
    if (!SR_BND_OK(R, off + klane(R, (unsigned)idx), SR_BND_WHAT(R))) return NULLV;
    const int v = (int)R.base[off + klane(R, (unsigned)idx)];
    return sizeof(ST) == sizeof(OT) ? v : (int)(short)v + SR_RING_BIAS;
}
template <typename OT, typename ST> __device__ __forceinline__ void rput(const KRows<OT, ST> &R, unsigned off, unsigned idx, int val) {
    if (!SR_BND_OK(R, off + klane(R, idx), SR_BND_WHAT(R))) return;
    R.base[off + klane(R, idx)] = (ST)(sizeof(ST) == sizeof(OT) ? val : val - SR_RING_BIAS);
}

// ---- immediate-offset row addressing (round 4; exact 10-level instance on the ring) -------------------------------------
// The ring is chunk-major with a component's levels adjacent, and the host keeps both ring depths multiples of the block
// (80 / 50 levels for the default penalties), so a block's ten levels -- and any five consecutive levels that start at a
// multiple of five -- are ten (five) ADJACENT 512-byte pieces that never straddle the ring's wrap.  A tile therefore
// addresses its 42 rows as 13 uniform bases (SGPR pairs) + one lane offset (a VGPR for the whole tile) + the row's
// distance as the instruction's immediate: no address VALU, no row offset per row in an SGPR (round 3: 42 offsets hoisted
// out of the tile loop and spilled into VGPR lanes -- v_readlane + hazard s_nop + v_add per row).  Levels below 0 read a
// NULL block of ten rows.  KBLK_C: a block base points at the block's fifth row, so that the immediates of its ten rows
// (-4 .. +5 rows = -2048 .. +2560 bytes) fit the instruction's 13-bit signed field.
typedef char __attribute__((address_space(1))) *GPB;
#define KBLK_C 4
template <typename OT, typename ST>
__device__ __forceinline__ GPB kbase(const KRows<OT, ST> &R, unsigned off_cells) { return (GPB)R.base + (size_t)off_cells * sizeof(ST); }
// lane_b = byte offset of the lane's group inside a row (klane(idx) * sizeof(ST)), IMM = distance in rows (compile time)
#define SR_IMMPTR(B, LANE_B, IMM) ((V4<ST> __attribute__((address_space(1))) *)((B) + (LANE_B) + (IMM) * (256 * (int)sizeof(ST))))
// (imm: a constant once the level loops are unrolled -- it folds into the instruction's offset field.  Instruction selection
// works block by block and only sees the saddr form -- uniform 64-bit base + zero-extended 32-bit lane offset -- when the
// zero extension happens in the block of the access: a level of the tile takes its own opaque copy of the lane offset
// (kopaque_v, one v_mov); without it the compiler forms base + lane once per base as a 64-bit VGPR pair ahead of the loop)
__device__ __forceinline__ unsigned kopaque_v(unsigned l) { asm volatile("" : "+v"(l)); return l; }
__device__ __forceinline__ int kopaque_s(int x) { asm volatile("" : "+s"(x)); return x; }       // a uniform value the optimiser may not look through
#define SR_IMMCELL(R, B, LANE_B, IMM) ((unsigned)(((B) - (GPB)(R).base) / (long)sizeof(ST)) + (LANE_B) / (unsigned)sizeof(ST) + (unsigned)((IMM) * 256))
template <typename OT, typename ST, typename KR> __device__ __forceinline__ V4<OT> ild(const KR &R, GPB b, unsigned lane_b, int imm) {
    if (!SR_BND_OK(R, SR_IMMCELL(R, b, lane_b, imm), 1u)) return knull4<OT>();
    return kcvt_in<OT, ST>(*SR_IMMPTR(b, lane_b, imm));
}
template <typename OT, typename ST, typename KR> __device__ __forceinline__ V4<OT> ild_nt(const KR &R, GPB b, unsigned lane_b, int imm) {
    if (!SR_BND_OK(R, SR_IMMCELL(R, b, lane_b, imm), 1u)) return knull4<OT>();
    return kcvt_in<OT, ST>(__builtin_nontemporal_load(SR_IMMPTR(b, lane_b, imm)));
}
template <typename OT, typename ST, typename KR> __device__ __forceinline__ void ist(const KR &R, GPB b, unsigned lane_b, int imm, V4<OT> v) {
    if (!SR_BND_OK(R, SR_IMMCELL(R, b, lane_b, imm), 1u)) return;
    *SR_IMMPTR(b, lane_b, imm) = kcvt_out<OT, ST>(v);
}
template <typename OT, typename ST, typename KR> __device__ __forceinline__ void ist_nt(const KR &R, GPB b, unsigned lane_b, int imm, V4<OT> v) {
    if (!SR_BND_OK(R, SR_IMMCELL(R, b, lane_b, imm), 1u)) return;
    __builtin_nontemporal_store(kcvt_out<OT, ST>(v), SR_IMMPTR(b, lane_b, imm));
}

// 4 cells of a 16-bit row as they are stored (packed tiles: the U row)
template <typename KR> __device__ __forceinline__ S4 rld_raw16(const KR &R, unsigned off, unsigned li) {
    if (!SR_BND_OK(R, off + li, 1u)) { const S4 n = {(short)-32768, (short)-32768, (short)-32768, (short)-32768}; return n; }
    return *(S4 __attribute__((address_space(1))) *)((char __attribute__((address_space(1))) *)R.base + (size_t)(off + li) * 2u);
}
template <typename KR> __device__ __forceinline__ void rst_raw16(const KR &R, unsigned off, unsigned li, S4 v) {
    if (!SR_BND_OK(R, off + li, 1u)) return;
    *(S4 __attribute__((address_space(1))) *)((char __attribute__((address_space(1))) *)R.base + (size_t)(off + li) * 2u) = v;
}

// value held by the previous / next lane (NULL at the wave's ends)
__device__ __forceinline__ int lane_left(int x) { return __builtin_amdgcn_update_dpp(NULLV, x, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ int lane_right(int x) { return __builtin_amdgcn_update_dpp(NULLV, x, 0x130, 0xf, 0xf, false); }
// max over each row of 16 lanes, result in the row's last lane
__device__ __forceinline__ int row16_max(int v) {
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x111, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x112, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x114, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x118, 0xf, 0xf, false));
    return v;
}

// same for values >= 0: zero-filled shifts fold into v_max_i32_dpp (no copy of the operand first)
__device__ __forceinline__ int row16_max_nn(int v) {
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, true));
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, true));
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, true));
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, true));
    return v;
}

// lanes of halo on either side of a wave tile: the I2 / D2 chains (gap-extend 1) consume one diagonal per level
template <int B> struct KGeo {
    static constexpr int HL = B <= 5 ? 2 : (B + 3) / 4;
    static constexpr int OWN = 64 - 2 * HL;              // owned 4-diagonal groups per tile
    static_assert(OWN == sr_pass_own(B), "sr_pass_rule.h: the host twin of the pass tables counts tiles with the same geometry");
};

// (window reads, ffs_sym, min3u, lanes_or_zero: sr_dev_common.h)
