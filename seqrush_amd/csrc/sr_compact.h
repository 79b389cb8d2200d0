// sr_compact.h -- compaction + renumbering from per-handle tables (sr_compact_tab.h, sr_compact.hip); host side only.
#pragma once
#include <cstdint>
#include "sr_graph.h"

// compact() + renumber_nodes_sequentially on g in place: device >= 0 on that HIP device (stream: its stream, null: a
// stream of its own), device < 0 the same functors on the host in index order.  stats: sr_compact_gfa's.
int sr_graph_compact_tables(SrGraph &g, int device, void *stream, uint64_t stats[8]);
// the same from the arrays srk_graph_induce left on the device (steps, packed edges, one base per node 1..nn): the induced
// graph never visits the host; g receives the compacted, renumbered graph
int srk_compact_induced(int device, void *stream, const uint32_t *d_steps, uint64_t ns, const unsigned long long *d_edges, uint64_t ne,
                        const uint8_t *d_node_base, uint64_t nn, const uint64_t *path_off, uint64_t np, SrGraph &g, uint64_t stats[8]);
void sr_compact_last_stats(uint64_t out[8]);        // of the calling thread's last run by tables
