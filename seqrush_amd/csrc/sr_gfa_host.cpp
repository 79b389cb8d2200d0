// sr_gfa_host.cpp -- from a union-find to GFA text: graph induction on the host from labels or a node array, on the device
// from a context's forest (sr_graph.hip), then compaction, the Ygs order and the writer, which live in sr_compact.cpp,
// sr_sort.cpp and sr_graph.h.  Nothing here aligns or unites.
#include <cctype>
#include <unordered_set>
#include "sr_ctx.h"
#include "sr_compact.h"

// ------------------------------------------------------------------ GFA (A9)
// O(N) formulation of build_bidirected_graph_with_options
// (bidirected_builder.rs:17-289) for a quiescent UF given as canonical labels:
// node ids in first-encounter order over sequences / positions (:29-41,
// :154-157), node base = base at offset(label) (:176-182), step reversed iff
// node base and sequence base are complementary (:190-203), edges deduplicated
// against themselves and their complement, first orientation kept
// (bidirected_ops.rs:813-825); optional compact() + renumber (sr_compact.cpp); write_gfa layout
// bidirected_ops.rs:880-925.
struct PairHash {
    size_t operator()(const std::pair<uint64_t, uint64_t> &p) const {
        return (size_t)splitmix64(p.first * 0x9e3779b97f4a7c15ULL ^ p.second);
    }
};

// compact: 0 = none, 1 = sr_compact.cpp on the host, 2 = already compacted on the device (ctx_induce_graph)
static char *finish_gfa(SrGraph &g, const sr_seqset *seqs, int compact, uint64_t *n_nodes, uint64_t *n_edges) {
    if (compact && compact != 2) { sr_graph_compact(g); sr_graph_renumber(g); }     // src/bidirected_gfa_writer.rs:39-51
    return sr_graph_format_gfa(g, seqs->names, n_nodes, n_edges);
}

extern "C" int sr_build_gfa_opts(const sr_seqset *seqs, const uint64_t *labels, int compact, char **gfa,
                                 uint64_t *n_nodes, uint64_t *n_edges) {
    if (!seqs || !labels || !gfa || !seqs->names) return sr_fail(SR_ERR_INVALID, "null argument");
    const uint64_t N = seqs->offsets[seqs->n];
    if (N >= 0x7fffffffULL) return sr_fail(SR_ERR_UNSUPPORTED, "graph induction supports < 2^31 bases");
    if (compact == 2) return sr_fail(SR_ERR_INVALID, "compact == 2 (on the device) needs a context: sr_ctx_build_gfa_opts");
    const uint64_t ufn = 2 * N + 2;
    std::vector<uint32_t> node_of(ufn, 0);
    SrGraph g;
    g.node_seq.assign(1, std::string()); g.node_alive.assign(1, 0);
    g.steps.resize(N); g.path_off.assign(1, 0);
    uint32_t next_id = 1;
    for (uint32_t s = 0; s < seqs->n; s++) {
        for (uint64_t p = seqs->offsets[s]; p < seqs->offsets[s + 1]; p++) {
            const uint64_t lf = labels[p << 1], lr = labels[(p << 1) | 1];
            if (lf >= ufn || lr >= ufn) return sr_fail(SR_ERR_INVALID, "label out of range");
            const uint64_t rep = node_of[lf] ? lf : (node_of[lr] ? lr : lf);
            uint32_t id = node_of[rep];
            if (!id) {
                id = next_id++;
                node_of[rep] = id;
                const uint64_t off = rep >> 1;
                g.node_seq.push_back(std::string(1, (char)(off < N ? seqs->bases[off] : seqs->bases[p])));
                g.node_alive.push_back(1);
            }
            const uint8_t nb = (uint8_t)toupper((unsigned char)g.node_seq[id][0]), eb = (uint8_t)toupper(seqs->bases[p]);
            const bool rev = (nb == 'A' && eb == 'T') || (nb == 'T' && eb == 'A') ||
                             (nb == 'C' && eb == 'G') || (nb == 'G' && eb == 'C');
            g.steps[p] = (id << 1) | (rev ? 1u : 0u);
        }
        g.path_off.push_back(seqs->offsets[s + 1]);
    }
    std::unordered_set<std::pair<uint64_t, uint64_t>, PairHash> eset;
    eset.reserve(N);
    for (uint32_t s = 0; s < seqs->n; s++)
        for (uint64_t p = seqs->offsets[s]; p + 1 < seqs->offsets[s + 1]; p++) {
            const uint32_t from = g.steps[p], to = g.steps[p + 1];
            if (eset.count({from, to}) || eset.count({to ^ 1u, from ^ 1u})) continue;
            eset.insert({from, to});
            g.edges.push_back({from, to});
        }
    *gfa = finish_gfa(g, seqs, compact, n_nodes, n_edges);
    return SR_OK;
}
extern "C" int sr_build_gfa(const sr_seqset *seqs, const uint64_t *labels, char **gfa, uint64_t *n_nodes, uint64_t *n_edges) {
    return sr_build_gfa_opts(seqs, labels, 0, gfa, n_nodes, n_edges);
}
// The reference's own root rule (src/bidirected_builder.rs:46-48, 176-182): a node takes the base at the offset of its
// component's union-find ROOT (union_find.find(pos)), whichever element the unite order made the root -- not the minimum
// Pos the canonical entry points above use.  Given the raw uf_rush node array (sr_align_and_unite with canonical_labels
// = 0, sr_ctx_download_uf, or an array a host built by replaying unites in its own fixed order through uf_rush /
// sr_uf_unite_host), the representative of every element is its root and the induction is otherwise the same: GFA
// byte equality with a reference run whose unites happened in that order, node orientation included.
extern "C" int sr_build_gfa_from_nodes(const sr_seqset *seqs, const uint64_t *nodes, int compact, char **gfa,
                                       uint64_t *n_nodes, uint64_t *n_edges) {
    if (!seqs || !nodes || !gfa || !seqs->names) return sr_fail(SR_ERR_INVALID, "null argument");
    const uint64_t N = seqs->offsets[seqs->n], ufn = 2 * N + 2;
    std::vector<uint64_t> root(ufn);
    for (uint64_t i = 0; i < ufn; i++) {
        root[i] = sr_uf_find(nodes, ufn, i);
        if (root[i] >= ufn) return sr_fail(SR_ERR_INVALID, "node array is not a uf_rush forest");
    }
    return sr_build_gfa_opts(seqs, root.data(), compact, gfa, n_nodes, n_edges);
}

// graph induction on the device from the context's union-find (sr_graph.hip); same
// text as sr_build_gfa() on the downloaded canonical labels.  which = 3 of sr_ctx_kernel_ms times it.
// compact == 2: the induced arrays go straight into compaction on the same device and stream (sr_compact.hip); g is
// then the compacted, renumbered graph and the induced one never reaches the host
static int ctx_induce_graph(sr_ctx *c, const sr_seqset *seqs, SrGraph &g, int compact = 0) {
    if (!c || !c->loaded) return sr_fail(SR_ERR_INVALID, "context not loaded");
    if (!seqs || !seqs->names) return sr_fail(SR_ERR_INVALID, "null argument");
    const uint64_t N = seqs->offsets[seqs->n];
    if (seqs->n != c->n || N != c->total_len) return sr_fail(SR_ERR_INVALID, "sequence set differs from the loaded one");
    if (N >= 0x7fffffffULL) return sr_fail(SR_ERR_UNSUPPORTED, "graph induction on device supports < 2^31 bases");
    HIPCHK(hipSetDevice(c->device));
    int r = sr_ctx_labels_device(c, (uint64_t *)c->d_labels);
    if (r) return r;
    std::vector<uint8_t> islast(N, 0);
    for (uint32_t s = 0; s < seqs->n; s++) islast[seqs->offsets[s + 1] - 1] = 1;
    uint64_t hcap = 64;
    while (hcap < 2 * N + 16) hcap <<= 1;
    const uint64_t ntiles = (N + 1023) / 1024 + 1;
    SrScratch tmp;
    uint8_t *d_bases = c->d_bases, *d_islast = (uint8_t *)tmp.alloc(N), *d_nbase = (uint8_t *)tmp.alloc(N);
    bool own_bases = false;
    if (!d_bases) { d_bases = (uint8_t *)tmp.alloc(N); own_bases = true; }        // (PAF contexts keep no byte copy)
    uint32_t *d_flag = (uint32_t *)tmp.alloc(N * 4), *d_nid = (uint32_t *)tmp.alloc(N * 4), *d_steps = (uint32_t *)tmp.alloc((N + 1) * 4);
    uint32_t *d_eslot = (uint32_t *)tmp.alloc(N * 4), *d_hvals = (uint32_t *)tmp.alloc(hcap * 4), *d_tiles = (uint32_t *)tmp.alloc(ntiles * 4);
    uint32_t *d_counts = (uint32_t *)tmp.alloc(8);
    unsigned long long *d_hkeys = (unsigned long long *)tmp.alloc(hcap * 8), *d_edges = (unsigned long long *)tmp.alloc(N * 8);
    if (!d_bases || !d_islast || !d_nbase || !d_flag || !d_nid || !d_steps || !d_eslot || !d_hvals || !d_tiles || !d_counts ||
        !d_hkeys || !d_edges) return sr_fail(SR_ERR_NOMEM, "not enough device memory for graph induction");
    if (own_bases) HIPCHK(hipMemcpyAsync(d_bases, seqs->bases, N, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_islast, islast.data(), N, hipMemcpyHostToDevice, c->stream));
    hipEvent_t *ge0, *ge1;
    if ((r = ev_get(c, 3, 0, &ge0, &ge1))) return r;
    HIPCHK(hipEventRecord(*ge0, c->stream));
    // d_minarr (uf_size entries) is free again once the labels exist: first-position table
    if (srk_graph_induce(c->d_labels, d_bases, d_islast, N, c->uf_size, c->d_minarr, d_flag, d_nid, d_steps, d_nbase, d_hkeys,
                         d_hvals, hcap, d_eslot, d_edges, d_tiles, d_counts, c->d_error, c->stream))
        return sr_fail(SR_ERR_HIP, "graph induction launch failed");
    HIPCHK(hipEventRecord(*ge1, c->stream));
    c->ev_used[3] = 1;
    if ((r = sr_ctx_sync(c))) return r;
    uint32_t counts[2] = {0, 0};
    HIPCHK(hipMemcpy(counts, d_counts, 8, hipMemcpyDeviceToHost));
    if (compact == 2) {
        std::vector<uint64_t> poff(seqs->offsets, seqs->offsets + seqs->n + 1);
        return srk_compact_induced(c->device, (void *)c->stream, d_steps, N, d_edges, counts[1], d_nbase, counts[0], poff.data(), seqs->n,
                                   g, nullptr);
    }
    std::vector<uint8_t> nbase(counts[0] ? counts[0] : 1);
    std::vector<unsigned long long> edges(counts[1] ? counts[1] : 1);
    g = SrGraph();
    g.steps.resize(N);
    HIPCHK(hipMemcpy(nbase.data(), d_nbase, counts[0], hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(g.steps.data(), d_steps, N * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(edges.data(), d_edges, (size_t)counts[1] * 8, hipMemcpyDeviceToHost));
    g.node_seq.assign((size_t)counts[0] + 1, std::string()); g.node_alive.assign((size_t)counts[0] + 1, 1);
    g.node_alive[0] = 0;
    for (uint32_t i = 0; i < counts[0]; i++) g.node_seq[i + 1].assign(1, (char)nbase[i]);
    g.path_off.assign(1, 0);
    for (uint32_t s = 0; s < seqs->n; s++) g.path_off.push_back(seqs->offsets[s + 1]);
    g.edges.resize(counts[1]);
    for (uint32_t i = 0; i < counts[1]; i++) g.edges[i] = {(uint32_t)(edges[i] >> 32), (uint32_t)(edges[i] & 0xffffffffULL)};
    return SR_OK;
}
extern "C" int sr_ctx_build_gfa_opts(sr_ctx *c, const sr_seqset *seqs, int compact, char **gfa, uint64_t *n_nodes, uint64_t *n_edges) {
    if (!gfa) return sr_fail(SR_ERR_INVALID, "null argument");
    SrGraph g;
    int r = ctx_induce_graph(c, seqs, g, compact);
    if (r) return r;
    *gfa = finish_gfa(g, seqs, compact, n_nodes, n_edges);
    return SR_OK;
}
// the same graph, compacted + renumbered unless compact == 0, then the Ygs layout (sr_sort.cpp) before the writer
// (src/bidirected_gfa_writer.rs:39-117); the device SGD runs on this context's device and stream
extern "C" int sr_ctx_build_gfa_sorted(sr_ctx *c, const sr_seqset *seqs, int compact, const sr_sort_params *p, char **gfa,
                                       uint64_t *n_nodes, uint64_t *n_edges) {
    if (!p || !gfa) return sr_fail(SR_ERR_INVALID, "null argument");
    SrGraph g;
    int r = ctx_induce_graph(c, seqs, g, compact);
    if (r) return r;
    if (compact && compact != 2) { sr_graph_compact(g); sr_graph_renumber(g); }
    sr_sort_params prm = *p;
    if (prm.device >= 0) prm.device = c->device;
    if ((r = sr_graph_ygs(g, prm, prm.device >= 0 ? (void *)c->stream : nullptr))) return r;
    const auto t0 = std::chrono::steady_clock::now();
    *gfa = sr_graph_format_gfa(g, seqs->names, n_nodes, n_edges);
    sr_sort_note_write_ms(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    return SR_OK;
}
extern "C" int sr_ctx_build_gfa(sr_ctx *c, const sr_seqset *seqs, char **gfa, uint64_t *n_nodes, uint64_t *n_edges) {
    return sr_ctx_build_gfa_opts(c, seqs, 0, gfa, n_nodes, n_edges);
}
