// sr_sort.h -- the Ygs layout of an SrGraph (src/ygs_sort.rs:96-162): deterministic path-guided SGD (Y, sr_sgd_term.h;
// device: sr_sort.hip, host twin and sequential yardstick: sr_sort.cpp), BFS grooming (g) and the head-seeded topological
// sort (s).  Host side only; not part of the public interface.
#pragma once
#include <cstdint>
#include <string>
#include <vector>
#include "../../include/seqrush_amd.h"
#include "sr_graph.h"
#include "sr_sgd_term.h"

// everything one SGD run reads: path index, tables and schedule (built once on the host by sgd_prepare)
struct SgdProblem {
    uint64_t n_nodes = 0;                            // dense node indices 0..n-1 = alive nodes in ascending id order
    std::vector<uint32_t> node_id;                   // [n_nodes] graph id of each dense index
    std::vector<double> x0;                          // initial positions: cumulative node lengths in id order
    std::vector<uint32_t> step_node, step_path, step_rank;
    std::vector<uint64_t> step_pos, path_first;
    std::vector<uint32_t> path_nsteps;
    std::vector<double> zetas, prefix_theta, prefix_cool, etas;
    uint64_t iters = 0;                              // iterations k = 0 .. iter_max (the reference's checker runs iter_max + 1)
    uint64_t first_cooling = 0;                      // cooling for k > first_cooling
    uint64_t terms_per_round = 0;
    bool has_terms = false;                          // some path has more than one step (src/path_sgd.rs:224-236)
    SgdView view;                                    // host pointers into the vectors above
    // resolved parameters
    uint64_t seed = 0, min_term_updates = 0, space = 0, space_max = 0, space_quant = 0, iter_max = 0;
    double theta = 0, eps = 0, eta_max = 0, cooling_start = 0;
};

// fills p from g and the user parameters (0 = derive, YgsParams::from_graph src/ygs_sort.rs:50-95); negative sr_status
int sgd_prepare(const SrGraph &g, const sr_sort_params &prm, SgdProblem &p);
// the three executions of the same schedule; x gets n_nodes positions
void sgd_run_host_twin(const SgdProblem &p, std::vector<double> &x);
void sgd_run_sequential(const SgdProblem &p, std::vector<double> &x);
int srk_sgd_device(const SgdProblem &p, int device, void *stream, std::vector<double> &x, float *ms);   // sr_sort.hip

// Ygs on g in place (node ids dense 1..N in the final order, edges sorted); fills the sr_sort_stats() slots.
// stream: the device's stream (null: a stream of its own)
int sr_graph_ygs(SrGraph &g, const sr_sort_params &prm, void *stream);
// GFA text with S / L / P lines -> SrGraph + path names (numeric node ids)
int sr_graph_parse_gfa(const char *text, SrGraph &g, std::vector<std::string> &names);
// the statistics stage on a parsed graph (sr_stats.hip): device >= 0 on that HIP device and `stream` (null: a stream of its
// own), -1 the host twin; *out as sr_graph_stats_gfa returns it
int sr_graph_stats_run(const SrGraph &g, int device, void *stream, sr_graph_stats **out);
// the path-by-bin tables of a parsed graph (sr_bin.hip), with the same meaning of device and stream; *out as
// sr_path_bins_gfa returns it
int sr_graph_bins_run(const SrGraph &g, const sr_bin_params &prm, int device, void *stream, sr_path_bins **out);
// the growth curves of a parsed graph (sr_growth.hip), with the same meaning of device and stream; *out as sr_growth_gfa
// returns it
int sr_graph_growth_run(const SrGraph &g, const uint32_t *group_of, uint32_t n_groups, const sr_growth_params &prm, int device, void *stream,
                        sr_growth **out);
// the variant sites of a parsed graph against one of its paths (sr_variants.hip), with the same meaning of device and
// stream; names = the path names the parser returned (the reference is chosen by name); *out as sr_variants_gfa returns it
int sr_graph_variants_run(const SrGraph &g, const std::vector<std::string> &names, const sr_variant_params &prm, int device, void *stream,
                          sr_variants **out);
int sr_fail(int code, const std::string &msg);     // sr_params.cpp: sets sr_last_error()
void sr_sort_note_write_ms(double ms);              // slot [3] of sr_sort_stats(), also added to the stage's wall time [9]
