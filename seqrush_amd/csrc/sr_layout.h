// sr_layout.h -- the 2-D path-guided SGD layout of an SrGraph (`--layout`): schedule, tables and
// initial state (sr_layout.cpp, on top of sgd_prepare), the three executions of one schedule (device: sr_layout.hip, host
// twin and sequential yardstick: sr_layout.cpp; per-term math: sr_layout_term.h).  Host side only; not part of the public
// interface.
#pragma once
#include <cstdint>
#include <vector>
#include "sr_sort.h"
#include "sr_layout_term.h"

struct LayoutProblem {
    SgdProblem sgd;                                  // path index, zeta and prefix tables, eta schedule, resolved parameters
    std::vector<uint8_t> step_rev;
    std::vector<uint32_t> node_len;
    std::vector<sr_xy> xy0;                          // [2 * n_nodes] initial end points
    LayoutView view;                                 // host pointers into the vectors above
};

// fills p from g and the user parameters (0 = derive); negative sr_status
int layout_prepare(const SrGraph &g, const sr_layout_params &prm, LayoutProblem &p);
// the three executions of the same schedule; xy gets 2 * n_nodes end points
void layout_run_host_twin(const LayoutProblem &p, std::vector<sr_xy> &xy);
void layout_run_sequential(const LayoutProblem &p, std::vector<sr_xy> &xy);
int srk_layout_device(const LayoutProblem &p, int device, void *stream, std::vector<sr_xy> &xy, float *ms);   // sr_layout.hip
