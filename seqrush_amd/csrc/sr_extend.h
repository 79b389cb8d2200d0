// sr_extend.h -- what sr_host.cpp needs of sr_extend.hip (--extend): the plan an input GFA and the
// new sequences resolve to, and the launcher of the seed stage.  Host side only; not part of the public interface.
#pragma once
#include <cstdint>
#include <string>
#include <vector>
#include "../../include/seqrush_amd.h"

struct sr_extend_plan {
    uint32_t n_old = 0, n_new = 0, V = 0, S = 0;
    uint64_t old_bases = 0, spell_us = 0;
    int device = SR_EXTEND_DEVICE_HOST;
    std::vector<uint32_t> steps, len;              // sr_extend_rule.h
    std::vector<uint64_t> sinc;                    // [S]
    // the merged set: old sequences (what the paths spell), then the new records
    std::vector<uint8_t> bases;
    std::vector<uint64_t> offsets;
    std::vector<std::string> names;
    std::vector<const char *> name_ptrs;
    sr_seqset merged{};
};

// device tables of a context's seed stage
struct SrExtendSeedArgs {
    const uint32_t *steps, *len;
    const uint64_t *sinc;
    uint32_t *anchor;                              // [V]
    uint32_t S, V;
    uint64_t bases;                                // old bases = sinc[S - 1]
    unsigned long long *nodes;                     // uf_rush node array of the merged set
    unsigned long long *counts;                    // [0] unions attempted, [1] unions that joined two sets
    int *error_flag;
};
// anchor[] by atomicMin, one lane per step (anchor must hold SR_EXTEND_NO_ANCHOR everywhere)
int srk_extend_anchor(const SrExtendSeedArgs *a, void *stream);
// one lane per spelled base: uf_unite with the base its node's anchor step spells
int srk_extend_seed(const SrExtendSeedArgs *a, void *stream);
