// sr_pairs.cpp -- which ordered pairs a load aligns, as pure host rules over indices and lengths: the enumeration with its
// sparsification strategies, the two entry lists of --iterative, the cost-balanced shard, and the mirror map of a list that
// runs in batches.  No device call and no context: a load applies them, and the exported twins let the tests do the same.
#include <cmath>
#include <functional>
#include <queue>
#include <unordered_map>
#include "sr_ctx.h"
#include "sr_mirror_rule.h"

static inline double unit53(uint64_t h) { return (double)(h >> 11) * (1.0 / 9007199254740992.0); }

// ------------------------------------------------------------------ pair list (A2)
// Ordered pair list before sharding: row-major n*n incl. self pairs ("all-vs-all including self",
// seqrush.rs:718-734), optional exclude_self, then the sparsification strategy (grammar seqrush.rs:356-431).
// allwave's selection rules are not in the reference tree; the definitions below are this project's own
// (restated in oracle/seqrush.c, PARITY UNPINNED):
//   random:F        ordered pair (q,t), q != t, kept iff unit(splitmix64(seed ^ (q*n+t))) < F
//   connectivity:P  unordered pair {i<j} kept iff unit(splitmix64(seed ^ (i*n+j))) < f,
//                   f = min(1, (ln n + c) / n), c = -ln(-ln P): the Erdos-Renyi threshold at which G(n,f) is
//                   connected with probability P (P = 1 or n <= 2: f = 1); both directions of a kept pair are aligned
//   auto            n < 10: none; else connectivity:0.99
//   tree:kn,kf,rf,k unordered pair kept iff it is one of the kn nearest or kf farthest neighbours of either end by
//                   k-mer sketch similarity (sr_sketch.hip), or unit(splitmix64(seed ^ (i*n+j))) < rf
// Self pairs are always kept unless exclude_self.
// --iterative (align_and_unite_iterative, src/seqrush.rs:867-1132) splits the unordered pairs of tree:kn,kf,rf,k into
//   tree entries    {i<j} selected for either end by the k-NN selection, row-major
//   random entries  the other {i<j} with unit(h) < rf, h = splitmix64(seed ^ (i*n+j)), ordered by h ascending, ties by (i, j):
//                   a seeded shuffle, so the early checks do not all see pairs of sequence 0
// (together exactly the unordered pairs of the tree: list above); each entry expands to the ordered alignments (i,i) (i,j)
// (j,i) (j,j), AllPairIterator over the two-sequence slice with exclude_self = false (:984-991), row-major like `none`.
static double connectivity_fraction(uint32_t n, double P) {
    if (n <= 2 || P >= 1.0) return 1.0;
    const double c = -std::log(-std::log(P));
    const double f = (std::log((double)n) + c) / (double)n;
    return f >= 1.0 ? 1.0 : (f <= 0.0 ? 0.0 : f);
}

// sel: n*n bytes from the device k-NN selection (tree), or NULL
void enumerate_pairs(uint32_t n, const sr_params &p, const uint8_t *sel, std::vector<uint32_t> &pq, std::vector<uint32_t> &pt) {
    pq.clear(); pt.clear();
    int kind = p.sparsify_kind;
    double frac = p.sparsify_factor;
    if (kind == SR_SPARSE_AUTO) { if (n < 10) kind = SR_SPARSE_NONE; else { kind = SR_SPARSE_CONNECTIVITY; frac = 0.99; } }
    const double conn_f = (kind == SR_SPARSE_CONNECTIVITY) ? connectivity_fraction(n, frac) : 1.0;
    for (uint32_t q = 0; q < n; q++)
        for (uint32_t t = 0; t < n; t++) {
            if (q == t) { if (p.exclude_self) continue; pq.push_back(q); pt.push_back(t); continue; }
            const uint32_t i = std::min(q, t), j = std::max(q, t);
            bool keep = true;
            if (kind == SR_SPARSE_RANDOM)
                keep = unit53(splitmix64(p.sparsify_seed ^ ((uint64_t)q * n + t))) < frac;
            else if (kind == SR_SPARSE_CONNECTIVITY)
                keep = unit53(splitmix64(p.sparsify_seed ^ ((uint64_t)i * n + j))) < conn_f;
            else if (kind == SR_SPARSE_TREE)
                keep = (sel && (sel[(uint64_t)i * n + j] || sel[(uint64_t)j * n + i])) ||
                       unit53(splitmix64(p.sparsify_seed ^ ((uint64_t)i * n + j))) < p.tree_rand_frac;
            if (keep) { pq.push_back(q); pt.push_back(t); }
        }
}

// the two entry lists of --iterative (definition above); sel: n*n bytes of the k-NN selection or NULL (n <= 1)
void iterative_lists(uint32_t n, const uint8_t *sel, uint64_t seed, double rf, SrU32s &ti, SrU32s &tj, SrU32s &ri, SrU32s &rj) {
    ti.clear(); tj.clear(); ri.clear(); rj.clear();
    struct R { uint64_t h; uint32_t i, j; };
    std::vector<R> rnd;
    for (uint32_t i = 0; i < n; i++)
        for (uint32_t j = i + 1; j < n; j++) {
            if (sel && (sel[(uint64_t)i * n + j] || sel[(uint64_t)j * n + i])) { ti.push_back(i); tj.push_back(j); continue; }
            const uint64_t h = splitmix64(seed ^ ((uint64_t)i * n + j));
            if (unit53(h) < rf) rnd.push_back({h, i, j});
        }
    std::sort(rnd.begin(), rnd.end(), [](const R &a, const R &b) {
        return a.h != b.h ? a.h < b.h : (a.i != b.i ? a.i < b.i : a.j < b.j); });
    for (const R &e : rnd) { ri.push_back(e.i); rj.push_back(e.j); }
}

extern "C" int sr_iterative_pair_lists(uint32_t n, const uint8_t *sel, const sr_params *p, uint32_t **tree_i, uint32_t **tree_j,
                                       uint64_t *tree_count, uint32_t **rand_i, uint32_t **rand_j, uint64_t *rand_count) {
    if (!p || !tree_i || !tree_j || !tree_count || !rand_i || !rand_j || !rand_count) return sr_fail(SR_ERR_INVALID, "null argument");
    std::vector<uint32_t> ti, tj, ri, rj;
    iterative_lists(n, sel, p->sparsify_seed, p->tree_rand_frac, ti, tj, ri, rj);
    *tree_count = ti.size(); *rand_count = ri.size();
    int r;
    if ((r = to_malloc(ti, tree_i)) || (r = to_malloc(tj, tree_j)) || (r = to_malloc(ri, rand_i))) return r;
    return to_malloc(rj, rand_j);
}

// Cost-balanced shard: pairs sorted by cost (|q|*|t|; self pairs cost |q|: they end in one
// extension), longest first, each handed to the least loaded rank (lowest rank on ties); a rank keeps its pairs
// in enumeration order.  Every rank computes the same assignment.  Equal costs degenerate to round-robin.
void shard_pairs(const std::vector<uint32_t> &len, uint32_t rank, uint32_t count, std::vector<uint32_t> &pq, std::vector<uint32_t> &pt) {
    if (count <= 1) return;
    const size_t m = pq.size();
    std::vector<uint64_t> cost(m);
    for (size_t i = 0; i < m; i++)
        cost[i] = pq[i] == pt[i] ? (uint64_t)len[pq[i]] : (uint64_t)len[pq[i]] * (uint64_t)len[pt[i]];
    std::vector<uint32_t> idx(m);
    for (size_t i = 0; i < m; i++) idx[i] = (uint32_t)i;
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return cost[a] > cost[b]; });
    typedef std::pair<uint64_t, uint32_t> LR;           // (load, rank): min-heap
    std::priority_queue<LR, std::vector<LR>, std::greater<LR>> heap;
    for (uint32_t r = 0; r < count; r++) heap.push({0, r});
    std::vector<uint8_t> mine(m, 0);
    for (uint32_t i : idx) {
        LR top = heap.top(); heap.pop();
        if (top.second == rank) mine[i] = 1;
        top.first += cost[i] ? cost[i] : 1;
        heap.push(top);
    }
    size_t w = 0;
    for (size_t i = 0; i < m; i++) if (mine[i]) { pq[w] = pq[i]; pt[w] = pt[i]; w++; }
    pq.resize(w); pt.resize(w);
}

extern "C" int sr_pair_list(uint32_t n, const sr_params *p, uint32_t **q_out, uint32_t **t_out, uint64_t *count) {
    if (!p || !q_out || !t_out || !count) return sr_fail(SR_ERR_INVALID, "null argument");
    if (p->shard_count == 0 || p->shard_rank >= p->shard_count) return sr_fail(SR_ERR_INVALID, "bad shard");
    if (p->sparsify_kind == SR_SPARSE_TREE)
        return sr_fail(SR_ERR_UNSUPPORTED, "tree sparsification needs the sequences (k-mer sketches): load a context and call sr_ctx_pairs");
    if ((uint64_t)n * n > 0xffffffffULL) return sr_fail(SR_ERR_UNSUPPORTED, "more than 2^32 ordered pairs");
    std::vector<uint32_t> pq, pt;
    enumerate_pairs(n, *p, nullptr, pq, pt);
    // sharding by cost needs lengths; this host-only helper assumes equal lengths (= round-robin over the
    // off-diagonal pairs, then over the cheaper self pairs)
    std::vector<uint32_t> len(n, 2);
    shard_pairs(len, p->shard_rank, p->shard_count, pq, pt);
    *count = pq.size();
    const int r = to_malloc(pq, q_out);
    return r ? r : to_malloc(pt, t_out);
}

// The mirror map of a pair list that runs in the given batches (sr_mirror_rule.h; batch b = pairs [batch_first[b],
// batch_first[b + 1])): the first (q, t) with q < t of a batch is the primary of the first (t, q) of the same batch, its
// secondary.  Self pairs, further copies of either and pairs whose partner sits in another batch have none.  A batch with
// no more pairs than the launch has workgroups gets no partners at all: every pair has a workgroup of its own there, the
// launch lasts as long as its longest pair, and a primary that aligns its secondary after itself (a tie, the reverse
// strand) could only lengthen it while the secondary's workgroup stood idle.  Returns the number of primaries.
uint64_t mirror_map(const uint32_t *q, const uint32_t *t, const uint32_t *batch_first, uint32_t nbatch, uint32_t workgroups, uint32_t *out) {
    uint64_t partners = 0;
    for (uint32_t b = 0; b < nbatch; b++) {
        const uint32_t f = batch_first[b], l = batch_first[b + 1];
        for (uint32_t i = f; i < l; i++) out[i] = SR_MIRROR_NONE;
        if ((uint64_t)l - f >= (uint64_t)SR_MIRROR_SECONDARY) continue;          // (the top bit of an entry is the mark)
        if (l - f <= workgroups) continue;                                       // a workgroup per pair: nothing to gain
        std::unordered_map<uint64_t, uint32_t> first;                            // ordered (q, t) -> its first index in the batch
        for (uint32_t i = f; i < l; i++)
            if (q[i] != t[i]) first.emplace(((uint64_t)q[i] << 32) | t[i], i);
        for (uint32_t i = f; i < l; i++) {
            if (q[i] >= t[i]) continue;
            if (first.find(((uint64_t)q[i] << 32) | t[i])->second != i) continue;                // a further copy
            const auto other = first.find(((uint64_t)t[i] << 32) | q[i]);
            if (other == first.end()) continue;
            out[i] = other->second - f;
            out[other->second] = (i - f) | SR_MIRROR_SECONDARY;
            partners++;
        }
    }
    return partners;
}
// the same without a context (tests): batch_first = NULL: one batch; workgroups = what the launch would have (0: pair
// every batch)
extern "C" int sr_mirror_map(const uint32_t *query_idx, const uint32_t *target_idx, uint64_t count, const uint32_t *batch_first,
                             uint32_t nbatch, uint32_t workgroups, uint32_t *mirror_out, uint64_t *partners_out) {
    if ((count && (!query_idx || !target_idx || !mirror_out)) || count > 0xfffffff0ULL) return sr_fail(SR_ERR_INVALID, "bad pair list");
    const uint32_t one[2] = {0, (uint32_t)count};
    if (!batch_first) { batch_first = one; nbatch = 1; }
    if (nbatch == 0 || batch_first[0] != 0 || batch_first[nbatch] != count) return sr_fail(SR_ERR_INVALID, "batches do not cover the pair list");
    for (uint32_t b = 0; b < nbatch; b++)
        if (batch_first[b] > batch_first[b + 1]) return sr_fail(SR_ERR_INVALID, "batches do not cover the pair list");
    const uint64_t n = mirror_map(query_idx, target_idx, batch_first, nbatch, workgroups, mirror_out);
    if (partners_out) *partners_out = n;
    return SR_OK;
}
