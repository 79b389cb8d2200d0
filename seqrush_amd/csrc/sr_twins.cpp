// sr_twins.cpp -- entry points that exist for the tests and for hosts without a device: the host twins of the rules the
// kernels share with them (mirror picks, replay, tile priority, pass tables, base cone, the iterative stop rule), the host
// union-find, and the stages of `tree:` selection run alone on a device.  No load path calls anything here.
#include "sr_ctx.h"
#include "sr_base_cone.h"
#include "sr_mirror_rule.h"
#include "sr_prio_rule.h"
#include "sr_pass_rule.h"

// the rules of sr_mirror_rule.h for the tests.  off[1..9]: candidate offsets of the nine tags (< 0: none); transposed: rank
// the tags as the transposed pair does -> the tag picked (0: none)
extern "C" int sr_mirror_bt_pick(const int *off, int transposed) {
    int bo = -1, bty = 0;
    for (int tag = 1; tag <= 9; tag++) {
        if (off[tag] < 0) continue;
        const int r = transposed ? sr_mirror_bt_rank_t(tag) : tag, rb = transposed ? sr_mirror_bt_rank_t(bty) : bty;
        if (off[tag] > bo || (off[tag] == bo && r > rb)) { bo = off[tag]; bty = tag; }
    }
    return bty;
}
extern "C" int sr_mirror_bt_rank_transposed(int tag) { return sr_mirror_bt_rank_t(tag); }
// what the kernel's backtrace computes for the same candidates: 1 = tie-sensitive
extern "C" int sr_mirror_bt_tie_host(const int *off) {
    int bo = -1, bty = 0, bi = -1;
    for (int tag = 1; tag <= 9; tag++) {
        if (off[tag] < 0) continue;
        if (tag <= SR_BT_I2_EXT && off[tag] > bi) bi = off[tag];
        if (off[tag] > bo || (off[tag] == bo && tag > bty)) { bo = off[tag]; bty = tag; }
    }
    return bty != 0 && sr_mirror_bt_tie(bty, bo, bi) ? 1 : 0;
}
// breakpoint call: n candidates (value, distance i, component, diagonal) -> the candidate each walk accepts (index) and
// whether the packed keys call the choice tie-sensitive; value_bias makes the values non-negative (the kernel adds gap-open)
extern "C" int sr_mirror_bp_pick_host(const int *val, const int *dist, const int *comp, const int *diag, int n, int value_bias,
                                      int *pick_out, int *pick_t_out) {
    unsigned long long best = ~0ull, best_t = ~0ull;
    *pick_out = *pick_t_out = -1;
    for (int j = 0; j < n; j++) {
        const unsigned long long k = sr_mirror_bp_key((unsigned)(val[j] + value_bias), dist[j], comp[j], diag[j]);
        const unsigned long long kt = sr_mirror_bp_key_t((unsigned)(val[j] + value_bias), dist[j], comp[j], diag[j]);
        if (k < best) { best = k; *pick_out = j; }
        if (kt < best_t) { best_t = kt; *pick_t_out = j; }
    }
    return n > 0 && sr_mirror_bp_tie(best, best_t) ? 1 : 0;
}
// replay (sr_mirror_rule.h): the transposed record; the kernel's walk of one level -- nrec records of SR_BPREC_INTS ints in
// list order (any levels; those of `level` are used), nseg segments under search of six ints (pb pe tb te cb ce) in list
// order -> match_out[i] = index of the record whose breakpoint segment i takes, -1 = it is searched; returns the matches
extern "C" int sr_replay_record_ints(void) { return SR_BPREC_INTS; }
extern "C" void sr_replay_transpose_host(const int *rec, int *out) {
    for (int f = 0; f < SR_BPREC_INTS; f++) out[f] = sr_bprec_t(rec, f);
}
extern "C" int sr_replay_match_host(const int *recs, int nrec, const int *segs, int nseg, int level, int *match_out) {
    int rd = 0, n = 0;
    while (rd < nrec && recs[rd * SR_BPREC_INTS + SR_BR_LEVEL] < level) rd++;
    for (int p = 0; p < nseg; p++) {
        const int *e = segs + 6 * p;
        match_out[p] = -1;
        while (rd < nrec) {
            const int *r = recs + rd * SR_BPREC_INTS;
            if (r[SR_BR_LEVEL] != level) break;
            const int c = sr_replay_cmp(r, e);
            if (c > 0) break;
            rd++;
            if (c < 0) continue;
            if (r[SR_BR_TIE] == 0 && sr_replay_same(r, e)) { match_out[p] = rd - 1; n++; }
            break;
        }
    }
    return n;
}

// host twin of the device rule (sr_prio_rule.h): s_setprio level of a workgroup's tile code
extern "C" int sr_tile_prio_role_host(uint32_t rank, uint32_t epoch, uint32_t wg_per_cu) { return sr_tile_prio_role(rank, epoch, wg_per_cu); }
extern "C" int sr_tile_prio_epoch_shift(void) { return SR_PRIO_EPOCH_SHIFT; }

// tests: the stages of `tree:` selection (tree_stages, the routine the load path runs)

extern "C" int sr_sketch_device(int device, const sr_seqset *seqs, uint32_t kmer, uint64_t **sketch, uint32_t **sketch_n,
                                uint32_t **shared, uint32_t **denom) {
    if (!seqs || !seqs->bases || !seqs->offsets || !sketch || !sketch_n || !shared || !denom) return sr_fail(SR_ERR_INVALID, "null argument");
    if (seqs->n == 0 || (uint64_t)seqs->n * seqs->n > 0xffffffffULL) return sr_fail(SR_ERR_INVALID, "bad sequence count");
    if (kmer < 1 || kmer > 32) return sr_fail(SR_ERR_UNSUPPORTED, "tree sparsification: k-mer size must be in 1..32 on the device");
    const uint32_t n = seqs->n;
    std::vector<uint32_t> len(n);
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t L = seqs->offsets[i + 1] - seqs->offsets[i];
        if (L == 0 || seqs->offsets[i + 1] < seqs->offsets[i]) return sr_fail(SR_ERR_EMPTY_SEQ, "Empty sequences are not allowed");
        if (L > 0x7fff0000ULL) return sr_fail(SR_ERR_UNSUPPORTED, "sequence too long");
        len[i] = (uint32_t)L;
    }
    int r;
    if ((r = sr_pick_device(device))) return r;
    SrScratch tmp;
    const uint8_t *d_bases = (const uint8_t *)tmp.up(seqs->bases + seqs->offsets[0], seqs->offsets[n] - seqs->offsets[0]);
    std::vector<uint64_t> goff(n);
    for (uint32_t i = 0; i < n; i++) goff[i] = seqs->offsets[i] - seqs->offsets[0];
    const uint64_t *d_goff = (const uint64_t *)tmp.up(goff.data(), (size_t)n * 8);
    const uint32_t *d_len = (const uint32_t *)tmp.up(len.data(), (size_t)n * 4);
    if (!d_bases || !d_goff || !d_len) return sr_fail(SR_ERR_NOMEM, "device allocation failed");
    std::vector<unsigned long long> sk;
    std::vector<uint32_t> skn, sh, dn;
    TreeTap tap;
    tap.sketch = &sk; tap.sketch_n = &skn; tap.shared = &sh; tap.denom = &dn;
    if ((r = tree_stages(nullptr, n, len.data(), d_bases, d_goff, d_len, kmer, nullptr, nullptr, 0, 0, nullptr, &tap))) return r;
    unsigned long long *skp = nullptr;
    if ((r = to_malloc(sk, &skp)) || (r = to_malloc(skn, sketch_n)) || (r = to_malloc(sh, shared)) || (r = to_malloc(dn, denom))) return r;
    *sketch = (uint64_t *)skp;
    return SR_OK;
}

extern "C" int sr_knn_select_device(int device, const uint32_t *shared, const uint32_t *denom, uint32_t n, uint32_t k_nearest,
                                    uint32_t k_farthest, uint8_t **sel) {
    if (!shared || !denom || !sel) return sr_fail(SR_ERR_INVALID, "null argument");
    if (n == 0 || (uint64_t)n * n > 0xffffffffULL) return sr_fail(SR_ERR_INVALID, "bad sequence count");
    int r;
    if ((r = sr_pick_device(device))) return r;
    std::vector<uint8_t> s;
    if ((r = tree_stages(nullptr, n, nullptr, nullptr, nullptr, nullptr, 0, shared, denom, k_nearest, k_farthest, &s, nullptr))) return r;
    return to_malloc(s, sel);
}

// UFRush::find (read-only walk) / same, uf_rush lib.rs:112-133, 72-84
extern "C" uint64_t sr_uf_find(const uint64_t *nodes, uint64_t n, uint64_t x) {
    const uint64_t mask = 0x03FFFFFFFFFFFFFFULL;
    if (x >= n) return UINT64_MAX;
    uint64_t guard = 0;
    while ((nodes[x] & mask) != x && guard++ < n) x = nodes[x] & mask;
    return x;
}
extern "C" int sr_uf_same(const uint64_t *nodes, uint64_t n, uint64_t x, uint64_t y) {
    return sr_uf_find(nodes, n, x) == sr_uf_find(nodes, n, y);
}

// Host-side uf_rush over a node array (same packing parent | rank << 58, path halving, union by rank, tie rule "larger
// index wins" as uf_rush lib.rs:112-208; one thread, so the CAS loops collapse to plain stores).  For hosts that merge
// per-GPU forests or replay unites themselves without a device: SURVEY 8(e)'s merge and 8(b)'s Seam 2 consumers.
static const uint64_t UFH_MASK = 0x03FFFFFFFFFFFFFFULL;
static inline uint64_t ufh_find(uint64_t *nodes, uint64_t x) {          // UFRush::find, lib.rs:112-133
    uint64_t xn = nodes[x];
    while (x != (xn & UFH_MASK)) {
        const uint64_t par = xn & UFH_MASK, pp = nodes[par] & UFH_MASK;
        nodes[x] = pp | (xn & ~UFH_MASK);                                // path halving: parent := grandparent, rank bits kept
        x = pp; xn = nodes[x];
    }
    return x;
}
static inline bool ufh_unite(uint64_t *nodes, uint64_t x, uint64_t y) { // UFRush::unite, lib.rs:159-208
    uint64_t xr = ufh_find(nodes, x), yr = ufh_find(nodes, y);
    if (xr == yr) return false;
    uint64_t xk = nodes[xr] >> 58, yk = nodes[yr] >> 58;
    if (xk > yk || (xk == yk && xr > yr)) { std::swap(xr, yr); std::swap(xk, yk); }
    nodes[xr] = yr | (xk << 58);
    if (xk == yk) nodes[yr] = yr | ((yk + 1) << 58);
    return true;
}
// SeqRush::new (src/seqrush.rs:308-336): 2N+2 nodes, unite(fwd(i), rev(i)) for every offset i, in order
extern "C" int sr_uf_init_host(uint64_t *nodes, uint64_t n, uint64_t total_len) {
    if (!nodes || n < 2 * total_len + 2) return sr_fail(SR_ERR_INVALID, "node array shorter than 2 * total_len + 2");
    for (uint64_t i = 0; i < n; i++) nodes[i] = i;
    for (uint64_t i = 0; i < total_len; i++) ufh_unite(nodes, 2 * i, 2 * i + 1);
    return SR_OK;
}
extern "C" int sr_uf_unite_host(uint64_t *nodes, uint64_t n, uint64_t x, uint64_t y) {
    if (!nodes || x >= n || y >= n) return sr_fail(SR_ERR_INVALID, "union-find index out of range");   // uf_rush panics (lib.rs:113)
    return ufh_unite(nodes, x, y) ? 1 : 0;
}
// SURVEY 8(e) merge on the host: replay unite(i, labels_g[i]) for `count` label arrays of n entries laid out back to back
extern "C" int sr_uf_merge_labels_host(uint64_t *nodes, uint64_t n, const uint64_t *labels, uint32_t count) {
    if (!nodes || !labels) return sr_fail(SR_ERR_INVALID, "null argument");
    for (uint32_t g = 0; g < count; g++) {
        const uint64_t *lab = labels + (uint64_t)g * n;
        for (uint64_t i = 0; i < n; i++) {
            if (lab[i] >= n) return sr_fail(SR_ERR_INVALID, "label out of range");
            if (lab[i] != i) ufh_unite(nodes, i, lab[i]);
        }
    }
    return SR_OK;
}
// count_components (src/seqrush.rs:341-353) of a SeqRush forest: roots among nodes [0, 2 total_len) -- every component with a
// base holds both strands of it (SeqRush::new) and nodes >= 2T are never united (sr_iter.hip does the same on the device)
extern "C" int sr_uf_count_components_host(const uint64_t *nodes, uint64_t n, uint64_t total_len, uint64_t *count) {
    if (!nodes || !count || 2 * total_len > n) return sr_fail(SR_ERR_INVALID, "bad node array");
    uint64_t c = 0;
    for (uint64_t x = 0; x < 2 * total_len; x++) c += (nodes[x] & UFH_MASK) == x;
    *count = c;
    return SR_OK;
}

// the stop rule over given per-check counts (sr_iter_rule.h, the decide kernel's rule): *stop_check = number of checks
// consumed when it fired (the run stops after 10 * *stop_check random entries), 0 = never within nchecks
extern "C" int sr_iterative_stop_host(const uint64_t *counts, uint64_t nchecks, uint64_t post_tree, uint64_t *stop_check) {
    if ((!counts && nchecks) || !stop_check) return sr_fail(SR_ERR_INVALID, "null argument");
    SrIterState s{};
    s.prev = post_tree;
    *stop_check = 0;
    for (uint64_t k = 0; k < nchecks && !s.stopped; k++) sr_iter_step(&s, counts[k], (uint32_t)k);
    if (s.stopped) *stop_check = (uint64_t)s.stop_check + 1;
    return SR_OK;
}

// the blocked kernel's backward cone of a base case (sr_base_cone.h, what blk_setup clips every level's range with):
// diagonals either side of the end diagonal that a level with `levels_left` levels to go keeps; < 0: none
extern "C" int sr_base_cone_reach(int e1, int e2, int two, int levels_left) {
    return sr_cone_reach(e1, e2, two != 0, levels_left);
}

// host twin of the blocked kernel's pass tables (sr_pass_rule.h, blk_setup of sr_blk_pass.inc), organised as the kernel is: the
// per-level tables by (aligner, level) lanes in steps of SR_PASS_LANES / B aligners, the per-aligner ones from the block's
// first and last level, then the tile prefix.  pen6 = x, o1, e1, o2, e2, two; jobs = njobs records of SR_PASS_JOB_INTS ints
// (active, begin component, plen, tlen, shift, kend, lj); base: the aligners are base cases (ranges and window cut to the cone
// of lj).  klo / khi: [B][njobs], written for active aligners only, like the kernel's; cells / ccells: per-aligner sums of the
// unclipped / clipped ranges (added to what the arrays hold); glo / ghi / nt per aligner; tstart[njobs + 1]: the prefix.
// Returns the steps the lanes took, < 0 for arguments no instance has.
#define SR_PASS_JOB_INTS 7
extern "C" int sr_pass_tile_own(int B) { return sr_pass_own(B); }
extern "C" int sr_pass_tables_host(const int *pen6, int scope, int B, int tight, int base, int s0, int njobs, const int *jobs,
                                   int *klo, int *khi, long long *cells, long long *ccells, int *glo, int *ghi, int *nt, int *tstart) {
    if (!pen6 || !jobs || B < 1 || B > SR_PASS_LANES || njobs < 0 || pen6[2] < 1 || (pen6[5] && pen6[4] < 1)) return -1;
    const int o1 = pen6[1], e1 = pen6[2], o2 = pen6[3], e2 = pen6[4];
    const bool two = pen6[5] != 0, cone = base != 0;
    const int steps = sr_pass_steps(njobs, B);
    for (int st = 0; st < steps; st++)
        for (int lane = 0; lane < SR_PASS_LANES; lane++) {
            int a, j;
            if (!sr_pass_lane(lane, st, B, a, j) || a >= njobs) continue;
            const int *b = jobs + (size_t)a * SR_PASS_JOB_INTS;
            if (!b[0]) continue;
            const int rb = cone ? sr_cone_reach(e1, e2, two, b[6] - 1 - (s0 + j)) : 0;
            int lo, hi, c, cc;
            sr_pass_level(sr_pass_reach(o1, e1, o2, e2, two, s0 + j, b[1] == SR_C_M), b[2], b[3], cone, cone ? b[5] : 0, rb, lo, hi, c, cc);
            klo[(size_t)j * njobs + a] = lo; khi[(size_t)j * njobs + a] = hi;
            cells[a] += c; ccells[a] += cc;
        }
    tstart[0] = 0;
    for (int a = 0; a < njobs; a++) {
        const int *b = jobs + (size_t)a * SR_PASS_JOB_INTS;
        glo[a] = 0; ghi[a] = -1; nt[a] = 0;
        if (b[0]) {
            const int rb0 = cone ? sr_cone_reach(e1, e2, two, b[6] - 1 - s0) : 0;
            sr_pass_window(sr_pass_reach(o1, e1, o2, e2, two, s0 + B - 1, b[1] == SR_C_M), tight ? 1 : scope + 1, b[2], b[3], b[4], cone,
                           cone ? b[5] : 0, rb0, sr_pass_own(B), glo[a], ghi[a], nt[a]);
        }
        tstart[a + 1] = tstart[a] + nt[a];
    }
    return steps;
}

// canonical labels of a node array: the minimum element of each set (what sr_ctx_download_labels returns)
extern "C" int sr_uf_canonical_labels_host(const uint64_t *nodes, uint64_t n, uint64_t *labels_out) {
    if (!nodes || !labels_out) return sr_fail(SR_ERR_INVALID, "null argument");
    std::vector<uint64_t> root(n), mn(n, UINT64_MAX);
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t r = sr_uf_find(nodes, n, i);
        if (r >= n) return sr_fail(SR_ERR_INVALID, "node array is not a uf_rush forest");
        root[i] = r;
        if (mn[r] == UINT64_MAX) mn[r] = i;                              // ascending i: the first one seen is the minimum
    }
    for (uint64_t i = 0; i < n; i++) labels_out[i] = mn[root[i]];
    return SR_OK;
}
