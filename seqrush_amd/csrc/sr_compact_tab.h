// sr_compact_tab.h -- one round of compact() (sr_compact.cpp compact_round) as a function of per-handle tables, stated
// once for the host (device = -2 of sr_compact_gfa: every functor runs in index order) and for the device
// (sr_compact.hip: one grid-stride kernel per functor).  DESIGN.md section 4.8.
//
//   degrees   fcnt / bcnt / fonly over the edge set, each stored edge also as its implied reverse;
//   successor succ[h] = successor of any occurrence of h, bad[h] = two occurrences disagree or one ends a path;
//   links     h -> fonly[h] when fcnt[h] == 1, bcnt[fonly[h]] == 1 and perfect(h, fonly[h]).  At most one link out and
//             one in per handle, and a -> b iff b^1 -> a^1: links form disjoint simple lists, each with its mirror list;
//   ranking   pointer jumping towards the list head carries (head, members, bases, smallest handle, smallest handle
//             that may start a chain) of the prefix that ends at every handle;
//   chains    the greedy search visits handles in ascending order and walks forward until it meets a visited handle, so
//             a chain starts where a handle with fcnt == 1 is smaller than everything before it in its list and runs to
//             just before the next such handle: chain start of h = smallest such handle of the prefix ending at h.  Of a
//             list and its mirror only one keeps its chains: with M the smallest handle of the list, the list that holds
//             the forward handle of M's node wins when that handle has a link out (its chain has >= 2 members and is
//             found first; every chain of the mirror overlaps it or a later one), else the mirror wins (as one chain:
//             its head is the minimum);
//   validate  a chain of distinct nodes is refused exactly when some occurrence of a member other than the entry is
//             not preceded, in its path, by the member before it (forward or mirrored);
//   rewrite   flags + exclusive scan + emit for steps, edges (open addressing, smallest original index wins), node
//             text (bytes keep their total; reversed members are reverse-complemented) and new ids NN, NN+1, ... in
//             ascending order of the chain's start handle.
// A list that meets its own mirror (it visits a node in both orientations) or has no head (a cycle) is irregular: the
// round that holds one is run by compact_round itself and counted.
#pragma once
#include <stdint.h>
#include <stddef.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CT_HD __host__ __device__ __forceinline__
#else
#define CT_HD inline
#endif

#define CT_NONE 0xffffffffu
#define CT_DROP 0xfffffffeu
#define CT_MAX_JUMPS 40

// slots of CtView::ctl
enum { CT_IRREGULAR = 0, CT_NVALID = 1, CT_LONGEST = 2, CT_HASH_FULL = 3, CT_SIZE = 4 /* [4..5], [6..7]: step / edge counts, double-buffered */, CT_JFLAG = 8, CT_NCTL = CT_JFLAG + CT_MAX_JUMPS + 2 };

CT_HD uint8_t ct_rc_base(uint8_t b) {                // rc_node_base of sr_compact.cpp (src/bidirected_graph.rs:73-85)
    switch (b) {
    case 'A': case 'a': return 'T'; case 'T': case 't': return 'A';
    case 'C': case 'c': return 'G'; case 'G': case 'g': return 'C';
    case 'N': case 'n': return 'N';
    default: return b;
    }
}

CT_HD void ct_add(uint32_t *p) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(p, 1u);
#else
    (*p)++;
#endif
}
CT_HD void ct_min(uint32_t *p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMin(p, v);
#else
    if (v < *p) *p = v;
#endif
}
CT_HD void ct_max(uint32_t *p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMax(p, v);
#else
    if (v > *p) *p = v;
#endif
}
CT_HD unsigned long long ct_cas(unsigned long long *p, unsigned long long expect, unsigned long long v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicCAS(p, expect, v);
#else
    const unsigned long long old = *p;
    if (old == expect) *p = v;
    return old;
#endif
}
CT_HD unsigned long long ct_mix(unsigned long long x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdULL; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL; x ^= x >> 33;
    return x;
}

// One round's arrays.  Handles are node << 1 | reverse; NN counts node slots (slot 0 and merged nodes are dead).
// size[0] = steps, size[1] = edges: device-resident, because the host learns them one round late (the round's only
// readback happens before the rewrite); every step / edge functor tests its index against them.
struct CtView {
    uint32_t NN, NH, NP, T;
    const uint32_t *size;                            // [2] steps, edges of this round
    uint32_t *size_out;                              // [2] after the rewrite
    uint64_t hmask;
    // graph
    const uint32_t *steps; const unsigned long long *edges; const uint32_t *path_off;
    const uint32_t *node_len, *node_off, *alive; const uint8_t *text;
    uint32_t *o_steps; unsigned long long *o_edges; uint32_t *o_path_off;
    uint32_t *o_len, *o_off, *o_alive; uint8_t *o_text;
    // tables per handle
    uint32_t *fcnt, *bcnt, *fonly, *succ, *next, *pred, *listmin, *cstart, *clast, *refused, *vflag, *rank, *pm, *cid;
    uint8_t *visits, *bad;
    const uint32_t *jp, *jmin, *jall, *jhead, *jcnt, *jlen;          // ranking: buffer read
    uint32_t *kp, *kmin, *kall, *khead, *kcnt, *klen;                // ranking: buffer written
    // per node
    uint32_t *mdst, *moff, *mrev;
    // per step / edge
    uint8_t *pfirst;
    uint32_t *sflag, *spos;                          // flags and their exclusive scan (steps, then edges)
    unsigned long long *hkeys, *ekey; uint32_t *hvals, *eslot;
    uint32_t *ctl;                                   // CT_NCTL
    uint32_t jump;                                   // index of the ranking launch (its flag: ctl[CT_JFLAG + jump])
};

CT_HD bool ct_last_step(const CtView &v, uint64_t i) { return i + 1 >= v.size[0] || v.pfirst[i + 1]; }
CT_HD bool ct_perfect(const CtView &v, uint32_t from, uint32_t to) {
    if (v.visits[from] && (v.bad[from] || v.succ[from] != to)) return false;
    const uint32_t tr = to ^ 1u, fr = from ^ 1u;
    if (v.visits[tr] && (v.bad[tr] || v.succ[tr] != fr)) return false;
    return true;
}

// ---- tables
struct CtDegree { CtView v; CT_HD void operator()(uint64_t i) const {
    if (i >= v.size[1]) return;
    const uint32_t a = (uint32_t)(v.edges[i] >> 32), b = (uint32_t)v.edges[i];
    ct_add(&v.fcnt[a]); v.fonly[a] = b; ct_add(&v.bcnt[b]);
    ct_add(&v.fcnt[b ^ 1u]); v.fonly[b ^ 1u] = a ^ 1u; ct_add(&v.bcnt[a ^ 1u]);
} };
struct CtPathFirst { CtView v; CT_HD void operator()(uint64_t p) const {
    if (v.path_off[p] < v.path_off[p + 1]) v.pfirst[v.path_off[p]] = 1;
} };
struct CtSuccAny { CtView v; CT_HD void operator()(uint64_t i) const {
    if (i >= v.size[0]) return;
    const uint32_t h = v.steps[i];
    v.visits[h] = 1;
    if (ct_last_step(v, i)) v.bad[h] = 1; else v.succ[h] = v.steps[i + 1];
} };
struct CtSuccBad { CtView v; CT_HD void operator()(uint64_t i) const {
    if (i >= v.size[0] || ct_last_step(v, i)) return;
    const uint32_t h = v.steps[i];
    if (v.succ[h] != v.steps[i + 1]) v.bad[h] = 1;
} };
struct CtLink { CtView v; CT_HD void operator()(uint64_t i) const {
    const uint32_t h = (uint32_t)i;
    if (v.fcnt[h] != 1) return;
    const uint32_t t = v.fonly[h];
    if (t >= v.NH || v.bcnt[t] != 1 || !ct_perfect(v, h, t)) return;
    v.next[h] = t; v.pred[t] = h;
} };

// ---- list ranking: every handle holds the summary of the members (jp[h], h] of its list
struct CtJumpInit { CtView v; CT_HD void operator()(uint64_t i) const {
    const uint32_t h = (uint32_t)i, p = v.pred[h];
    v.kp[h] = p; v.kmin[h] = v.fcnt[h] == 1 ? h : CT_NONE; v.kall[h] = h; v.khead[h] = h; v.kcnt[h] = 1;
    v.klen[h] = v.node_len[h >> 1];
    if (p != CT_NONE) v.ctl[CT_JFLAG + v.jump] = 1;
} };
struct CtJump { CtView v; CT_HD void operator()(uint64_t i) const {
    const uint32_t h = (uint32_t)i, p = v.jp[h];
    if (p == CT_NONE) {
        v.kp[h] = p; v.kmin[h] = v.jmin[h]; v.kall[h] = v.jall[h]; v.khead[h] = v.jhead[h]; v.kcnt[h] = v.jcnt[h]; v.klen[h] = v.jlen[h];
        return;
    }
    const uint32_t a = v.jmin[h], b = v.jmin[p], c = v.jall[h], d = v.jall[p], q = v.jp[p];
    v.kp[h] = q; v.kmin[h] = a < b ? a : b; v.kall[h] = c < d ? c : d; v.khead[h] = v.jhead[p];
    v.kcnt[h] = v.jcnt[h] + v.jcnt[p]; v.klen[h] = v.jlen[h] + v.jlen[p];
    if (q != CT_NONE) v.ctl[CT_JFLAG + v.jump] = 1;
} };

// ---- chains (reads the ranking through j*)
struct CtTail { CtView v; CT_HD void operator()(uint64_t i) const {
    const uint32_t h = (uint32_t)i;
    if (v.next[h] != CT_NONE || v.jp[h] != CT_NONE) return;
    v.listmin[v.jhead[h]] = v.jall[h];
    ct_max(&v.ctl[CT_LONGEST], v.jcnt[h]);
} };
struct CtChain { CtView v; CT_HD void operator()(uint64_t i) const {
    const uint32_t h = (uint32_t)i, hd = v.jhead[h];
    v.cstart[h] = CT_NONE; v.clast[h] = 0;
    const uint32_t M = v.jp[h] == CT_NONE ? v.listmin[hd] : CT_NONE;
    if (M == CT_NONE || hd == v.jhead[h ^ 1u]) { v.ctl[CT_IRREGULAR] = 1; return; }   // no head / no tail, or meets its mirror
    const bool win = (M & 1u) ? v.next[M ^ 1u] == CT_NONE : v.next[M] != CT_NONE;
    const uint32_t cs = v.jmin[h];
    if (!win || cs == CT_NONE) return;
    const uint32_t n1 = v.next[cs];
    if (n1 == CT_NONE || v.jmin[n1] != cs) return;                // a chain of one member records nothing
    v.cstart[h] = cs;
    const uint32_t nx = v.next[h];
    v.clast[h] = (nx == CT_NONE || v.jmin[nx] != cs) ? 1u : 0u;
} };
struct CtValidate { CtView v; CT_HD void operator()(uint64_t i) const {
    if (i >= v.size[0]) return;
    const uint32_t h = v.steps[i], prev = (v.pfirst[i] || i == 0) ? CT_NONE : v.steps[i - 1];
    const uint32_t cs = v.cstart[h];
    if (cs != CT_NONE && h != cs && prev != v.pred[h]) v.refused[cs] = 1;
    const uint32_t g = h ^ 1u, cr = v.cstart[g];
    if (cr != CT_NONE && !v.clast[g] && prev != (v.next[g] ^ 1u)) v.refused[cr] = 1;
} };
struct CtValidFlag { CtView v; CT_HD void operator()(uint64_t i) const {
    const uint32_t h = (uint32_t)i;
    v.vflag[h] = (v.cstart[h] == h && !v.refused[h]) ? 1u : 0u;
} };

// ---- rewrite.  pm[h]: what a path step h becomes (CT_DROP: a member behind the entry); an edge's `to` maps by pm[to],
// its `from` by pm[from ^ 1] ^ 1; cid[h]: new node of h's chain
struct CtMap { CtView v; CT_HD void operator()(uint64_t i) const {
    const uint32_t h = (uint32_t)i, n = h >> 1;
    uint32_t cs = v.cstart[h];
    if (cs != CT_NONE && !v.refused[cs]) {
        const uint32_t id = v.NN + v.rank[cs], before = v.jlen[cs] - v.node_len[cs >> 1];
        v.cid[h] = id; v.pm[h] = h == cs ? id << 1 : CT_DROP;
        v.mdst[n] = id; v.moff[n] = v.jlen[h] - v.node_len[n] - before; v.mrev[n] = h & 1u;
        v.o_len[n] = 0; v.o_alive[n] = 0;
        if (v.clast[h]) { v.o_len[id] = v.jlen[h] - before; v.o_alive[id] = 1; }
        return;
    }
    cs = v.cstart[h ^ 1u];
    if (cs != CT_NONE && !v.refused[cs]) {
        const uint32_t id = v.NN + v.rank[cs];
        v.cid[h] = id; v.pm[h] = v.clast[h ^ 1u] ? (id << 1) | 1u : CT_DROP;
        return;
    }
    v.cid[h] = CT_NONE; v.pm[h] = h;
    if (!(h & 1u)) { v.mdst[n] = CT_NONE; v.o_len[n] = v.node_len[n]; v.o_alive[n] = v.alive[n]; }
} };
struct CtStepFlag { CtView v; CT_HD void operator()(uint64_t i) const {
    v.sflag[i] = (i < v.size[0] && v.pm[v.steps[i]] != CT_DROP) ? 1u : 0u;
} };
struct CtStepEmit { CtView v; CT_HD void operator()(uint64_t i) const {
    if (i < v.size[0] && v.sflag[i]) v.o_steps[v.spos[i]] = v.pm[v.steps[i]];
} };
struct CtPathOff { CtView v; CT_HD void operator()(uint64_t p) const {
    const uint32_t o = v.path_off[p];
    v.o_path_off[p] = o < v.size[0] ? v.spos[o] : v.size_out[0];
} };
struct CtEdgeInsert { CtView v; CT_HD void operator()(uint64_t i) const {
    v.eslot[i] = CT_NONE;
    if (i >= v.size[1]) return;
    const uint32_t a = (uint32_t)(v.edges[i] >> 32), b = (uint32_t)v.edges[i];
    if (v.cid[a] != CT_NONE && v.cid[a] == v.cid[b]) return;     // inside one chain
    const uint32_t f = v.pm[a ^ 1u], t = v.pm[b];
    if (f == CT_DROP || t == CT_DROP) return;
    const unsigned long long key = ((unsigned long long)(f ^ 1u) << 32) | t;
    v.ekey[i] = key;
    uint64_t s = ct_mix(key) & v.hmask;
    for (uint64_t probe = 0; probe <= v.hmask; probe++) {
        const unsigned long long prev = ct_cas(&v.hkeys[s], ~0ull, key);
        if (prev == ~0ull || prev == key) { ct_min(&v.hvals[s], (uint32_t)i); v.eslot[i] = (uint32_t)s; return; }
        s = (s + 1) & v.hmask;
    }
    v.ctl[CT_HASH_FULL] = 1;
} };
struct CtEdgeFlag { CtView v; CT_HD void operator()(uint64_t i) const {
    const uint32_t s = v.eslot[i];
    v.sflag[i] = (s != CT_NONE && v.hvals[s] == (uint32_t)i) ? 1u : 0u;
} };
struct CtEdgeEmit { CtView v; CT_HD void operator()(uint64_t i) const {
    if (v.sflag[i]) v.o_edges[v.spos[i]] = v.ekey[i];
} };
// one thread per base of the old text
struct CtTextCopy { CtView v; CT_HD void operator()(uint64_t i) const {
    const uint32_t b = (uint32_t)i;
    uint32_t lo = 0, hi = v.NN;                     // last node with node_off <= b: the one that holds b
    while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (v.node_off[mid] <= b) lo = mid; else hi = mid; }
    const uint32_t n = lo, k = b - v.node_off[n], len = v.node_len[n], d = v.mdst[n];
    if (k >= len) return;
    if (d == CT_NONE) { v.o_text[v.o_off[n] + k] = v.text[b]; return; }
    const uint32_t base = v.o_off[d] + v.moff[n];
    if (v.mrev[n]) v.o_text[base + (len - 1 - k)] = ct_rc_base(v.text[b]); else v.o_text[base + k] = v.text[b];
} };
// ---- renumbering (rank = exclusive scan of alive): ids 1.. in ascending order of the old ids
struct CtRenumberSteps { CtView v; CT_HD void operator()(uint64_t i) const {
    if (i >= v.size[0]) return;
    const uint32_t h = v.steps[i];
    v.o_steps[i] = ((v.rank[h >> 1] + 1u) << 1) | (h & 1u);
} };
struct CtRenumberEdges { CtView v; CT_HD void operator()(uint64_t i) const {
    if (i >= v.size[1]) return;
    const uint32_t a = (uint32_t)(v.edges[i] >> 32), b = (uint32_t)v.edges[i];
    v.o_edges[i] = ((unsigned long long)(((v.rank[a >> 1] + 1u) << 1) | (a & 1u)) << 32) | (((v.rank[b >> 1] + 1u) << 1) | (b & 1u));
} };
