// sr_stage_host.h -- the host side every graph stage shares (DESIGN.md "What a graph stage gets for free"): the tables
// {V, S, P, len, steps, path_off} of a parsed GFA with their checks, the lookup of a path by name, and the small helpers of
// the twins and the writers.  Header only: a stage's .hip file is also compiled alone (the *-asan programs, the yardstick
// builds of the Makefile) and links against the default library without further inputs.  Not part of the public interface.
#pragma once
#include <chrono>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/seqrush_amd.h"
#include "sr_sort.h"

inline double us_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
}

inline std::string u64s(uint64_t v) { return std::to_string((unsigned long long)v); }

// *text = a malloc copy of s for the caller of the C interface to sr_free(); `nomem` is the caller's message
inline int sr_give_text(const std::string &s, char **text, const char *nomem) {
    char *res = (char *)malloc(s.size() + 1);
    if (!res) return sr_fail(SR_ERR_NOMEM, nomem);
    memcpy(res, s.c_str(), s.size() + 1);
    *text = res;
    return SR_OK;
}

// the first path named `name`, np when there is none (the caller has its own "no path is named" message)
inline uint64_t sr_path_by_name(const std::vector<std::string> &names, uint64_t np, const char *name) {
    uint64_t p = 0;
    while (p < np && (p >= names.size() || names[p] != name)) p++;
    return p;
}

// The tables the host twin and the device execution of a stage both read.  A stage's own tables sit beside them.
struct SrPathTables {
    uint32_t V = 0, S = 0, P = 0;
    uint64_t bases = 0;                              // the sum of the node lengths
    std::vector<uint32_t> len, steps, path_off;      // len: node v = 1..V at v - 1, or at v with slot 0 unused (sr_path_tables_fill)
};

// Step 1, the sizes before anything is narrowed to 32 bits.  The caller holds them against its own limits, in its own
// sentence (the stages differ in what they count), makes the checks that come before its node loop, and then fills.
struct SrPathSizes { uint64_t nodes, steps, paths, edges, bases; };

inline SrPathSizes sr_path_sizes(const SrGraph &g) {
    SrPathSizes z{g.node_seq.size() ? g.node_seq.size() - 1 : 0, g.steps.size(), g.path_off.size() ? g.path_off.size() - 1 : 0, g.edges.size(), 0};
    for (uint64_t v = 1; v <= z.nodes; v++) z.bases += g.node_seq[v].size();
    return z;
}

// Step 2, fill and validate, in this order: every node is alive (and, with refuse_empty, has a sequence), every step names
// a node, the offsets are narrowed.  z.nodes < 2^30, z.steps < 2^31 and z.paths < 2^31 are the caller's limits at the least.
// slot0: len[v] holds node v and len[0] = 0 (the kernels of stats and bins index by the node id), else len[v - 1] does.
inline int sr_path_tables_fill(const SrGraph &g, const SrPathSizes &z, const char *prefix, bool refuse_empty, bool slot0, SrPathTables &t) {
    const std::string pre = std::string(prefix) + ": ";
    t.V = (uint32_t)z.nodes; t.S = (uint32_t)z.steps; t.P = (uint32_t)z.paths; t.bases = z.bases;
    t.len.assign(z.nodes + (slot0 ? 1 : 0), 0);
    for (uint64_t v = 1; v <= z.nodes; v++) {
        if (!g.node_alive[v]) return sr_fail(SR_ERR_INVALID, pre + "node ids must be dense");
        if (refuse_empty && g.node_seq[v].empty()) return sr_fail(SR_ERR_INVALID, pre + "a node has no sequence");
        t.len[slot0 ? v : v - 1] = (uint32_t)g.node_seq[v].size();
    }
    t.steps = g.steps;
    for (uint32_t h : t.steps)
        if ((h >> 1) == 0 || (h >> 1) > z.nodes) return sr_fail(SR_ERR_INVALID, pre + "a path step names a missing node");
    t.path_off.resize(z.paths + 1, 0);
    for (uint64_t p = 0; p <= z.paths && p < g.path_off.size(); p++) t.path_off[p] = (uint32_t)g.path_off[p];
    return SR_OK;
}
