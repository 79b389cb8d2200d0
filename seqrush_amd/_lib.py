"""ctypes loader for libseqrush_amd.so (the C ABI of include/seqrush_amd.h).

The library is built in-tree by ``__graft_entry__.build()`` /
``make -C seqrush_amd/csrc``.  There is no fallback: if the shared object is
missing the import of any compute entry point raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SEQRUSH_AMD_LIB: another build of the same library (kernel A/B experiments)
LIB_PATH = os.environ.get("SEQRUSH_AMD_LIB") or os.path.join(_HERE, "libseqrush_amd.so")

# every symbol include/seqrush_amd.h declares
EXPORTS = [
    "sr_default_params", "sr_parse_scores", "sr_parse_orientation_scores",
    "sr_parse_sparsification", "sr_align_all", "sr_alignments_free", "sr_alignment_cigar",
    "sr_align_and_unite", "sr_uf_find", "sr_uf_same", "sr_write_paf", "sr_ctx_create",
    "sr_ctx_destroy", "sr_ctx_set_stream", "sr_ctx_load", "sr_ctx_reset_uf", "sr_ctx_align",
    "sr_ctx_unite", "sr_ctx_sync", "sr_ctx_alignments", "sr_ctx_download_uf", "sr_ctx_uf_size",
    "sr_ctx_num_pairs", "sr_ctx_dp_cells", "sr_ctx_labels_device", "sr_ctx_merge_labels",
    "sr_ctx_download_labels", "sr_ctx_kernel_ms", "sr_ctx_counters", "sr_build_gfa", "sr_free",
    "sr_last_error", "sr_abi_version", "sr_device_count", "sr_pair_list", "sr_ctx_align_kernel",
    "sr_ctx_load_paf", "sr_unite_paf", "sr_ctx_build_gfa", "sr_ctx_load_pairs", "sr_ctx_pairs",
    "sr_ctx_num_batches", "sr_ctx_workspace_report", "sr_ctx_run", "sr_ctx_align_all", "sr_ctx_pair_results",
    "sr_ctx_labels_device_u32", "sr_ctx_merge_labels_u32", "sr_ctx_counters_ext",
    "sr_build_gfa_opts", "sr_ctx_build_gfa_opts", "sr_ctx_merge_labels_host",
    "sr_uf_init_host", "sr_uf_unite_host", "sr_uf_merge_labels_host", "sr_uf_canonical_labels_host",
    "sr_build_gfa_from_nodes", "sr_ctx_counters_all", "sr_knobs_doc",
    "sr_sort_params_default", "sr_ctx_build_gfa_sorted", "sr_sort_gfa", "sr_sgd_layout", "sr_sgd_tables", "sr_sort_stats",
    "sr_ctx_load_iterative", "sr_ctx_run_iterative", "sr_ctx_iterative_stats", "sr_ctx_iterative_alignments",
    "sr_uf_count_components_host", "sr_iterative_stop_host", "sr_iterative_pair_lists", "sr_base_cone_reach",
    "sr_ctx_enable_inversions", "sr_ctx_inversion_stats", "sr_ctx_inversion_jobs", "sr_ctx_inversion_alignments",
    "sr_append_paf_tagged", "sr_inversion_sites_host", "sr_inversion_candidate", "sr_inversion_accept",
    "sr_inversion_scan_device",
    "sr_ctx_inversion_join_stats", "sr_inversion_sites_host_join", "sr_inversion_accept_site", "sr_inversion_scan_device_join",
    "sr_compact_gfa", "sr_compact_stats",
    "sr_sketch_device", "sr_knn_select_device",
    "sr_graph_stats_gfa", "sr_graph_stats_free", "sr_graph_stats_report", "sr_stats_sq_sums_host",
    "sr_mirror_map", "sr_mirror_bt_pick", "sr_mirror_bt_rank_transposed", "sr_mirror_bt_tie_host", "sr_mirror_bp_pick_host",
    "sr_ctx_orientation_scores",
    "sr_layout_params_default", "sr_layout_gfa", "sr_layout_tsv", "sr_layout_svg", "sr_layout_quality", "sr_layout_stats",
    "sr_layout_resolve", "sr_layout_select_host",
    "sr_path_bins_gfa", "sr_path_bins_free", "sr_path_bins_tsv", "sr_viz_params_default", "sr_path_bins_rgb", "sr_path_bins_png",
    "sr_growth_params_default", "sr_growth_gfa", "sr_growth_free", "sr_growth_groups", "sr_growth_expected", "sr_growth_fit",
    "sr_growth_report",
    "sr_variant_params_default", "sr_variants_gfa", "sr_variants_free", "sr_variants_vcf",
    "sr_ctx_tail_deferred", "sr_ctx_tail_timeline", "sr_tail_shape",
    "sr_replay_record_ints", "sr_replay_transpose_host", "sr_replay_match_host",
    "sr_ctx_prio_timeline", "sr_tile_prio_role_host", "sr_tile_prio_epoch_shift",
    "sr_pass_tables_host", "sr_pass_tile_own",
    "sr_extend_plan_gfa", "sr_extend_plan_free", "sr_extend_plan_seqs", "sr_extend_plan_n_old", "sr_extend_pair_list",
    "sr_ctx_load_extend", "sr_extend_seed_host", "sr_extend_plan_stats", "sr_ctx_extend_stats",
    "sr_lift_params_default", "sr_lift_gfa", "sr_lift_free", "sr_lift_bed",
    "sr_extract_params_default", "sr_extract_gfa", "sr_extract_free", "sr_extract_text",
]


class SeqSetC(C.Structure):
    _fields_ = [("n", C.c_uint32), ("bases", C.c_char_p), ("offsets", C.POINTER(C.c_uint64)),
                ("names", C.POINTER(C.c_char_p))]


class ParamsC(C.Structure):
    _fields_ = [
        ("match_score", C.c_int32), ("mismatch_penalty", C.c_int32),
        ("gap_open1", C.c_int32), ("gap_ext1", C.c_int32),
        ("gap_open2", C.c_int32), ("gap_ext2", C.c_int32),
        ("ori_match", C.c_int32), ("ori_mismatch", C.c_int32),
        ("ori_gap_open", C.c_int32), ("ori_gap_ext", C.c_int32),
        ("min_match_len", C.c_uint64), ("max_divergence", C.c_double),
        ("exclude_self", C.c_int32), ("memory_mode", C.c_int32),
        ("sparsify_kind", C.c_int32), ("sparsify_factor", C.c_double),
        ("sparsify_seed", C.c_uint64), ("canonical_labels", C.c_int32), ("device", C.c_int32),
        ("shard_rank", C.c_uint32), ("shard_count", C.c_uint32),
        ("tree_k_nearest", C.c_uint32), ("tree_k_farthest", C.c_uint32), ("tree_rand_frac", C.c_double),
        ("tree_kmer", C.c_uint32),
    ]


class SortParamsC(C.Structure):
    """sr_sort_params (include/seqrush_amd.h, Ygs layout)"""
    _fields_ = [
        ("seed", C.c_uint64), ("iter_max", C.c_uint64), ("theta", C.c_double), ("eps", C.c_double),
        ("eta_max", C.c_double), ("cooling_start", C.c_double), ("space", C.c_uint64), ("space_max", C.c_uint64),
        ("space_quant", C.c_uint64), ("min_term_updates", C.c_uint64), ("terms_per_round", C.c_uint64),
        ("skip_sgd", C.c_int32), ("skip_groom", C.c_int32), ("skip_topo", C.c_int32), ("device", C.c_int32),
    ]


class LayoutParamsC(C.Structure):
    """sr_layout_params (include/seqrush_amd.h, 2-D layout)"""
    _fields_ = [
        ("seed", C.c_uint64), ("iter_max", C.c_uint64), ("theta", C.c_double), ("eps", C.c_double),
        ("eta_max", C.c_double), ("cooling_start", C.c_double), ("space", C.c_uint64), ("space_max", C.c_uint64),
        ("space_quant", C.c_uint64), ("min_term_updates", C.c_uint64), ("terms_per_round", C.c_uint64),
        ("device", C.c_int32), ("reserved", C.c_int32),
    ]


class IterStatsC(C.Structure):
    """sr_iter_stats (include/seqrush_amd.h, iterative mode)"""
    _fields_ = [
        ("tree_entries", C.c_uint64), ("random_entries", C.c_uint64), ("random_processed", C.c_uint64),
        ("random_aligned", C.c_uint64), ("checks", C.c_uint64), ("windows", C.c_uint64), ("post_tree", C.c_uint64),
        ("final_components", C.c_uint64), ("stabilized", C.c_int32), ("tree_defaulted", C.c_int32),
        ("tree_k_nearest", C.c_uint32), ("tree_k_farthest", C.c_uint32), ("tree_rand_frac", C.c_double),
        ("tree_kmer", C.c_uint32), ("reserved", C.c_uint32),
    ]


class InvParamsC(C.Structure):
    """sr_inv_params (include/seqrush_amd.h, inversion patching)"""
    _fields_ = [("min_size", C.c_uint64), ("keep_alignments", C.c_int32), ("join_below", C.c_uint32)]


class InvStatsC(C.Structure):
    _fields_ = [("scanned", C.c_uint64), ("sites", C.c_uint64), ("candidates", C.c_uint64), ("accepted", C.c_uint64),
                ("rejected_score", C.c_uint64), ("rejected_divergence", C.c_uint64), ("united_bases", C.c_uint64),
                ("patch_batches", C.c_uint64), ("scan_ms", C.c_double), ("patch_align_ms", C.c_double)]


class InvJobC(C.Structure):
    _fields_ = [("pair", C.c_uint64), ("query_idx", C.c_uint32), ("target_idx", C.c_uint32),
                ("query_start", C.c_uint64), ("query_end", C.c_uint64), ("target_start", C.c_uint64),
                ("target_end", C.c_uint64), ("main_score", C.c_int32), ("patch_score", C.c_int32),
                ("is_reverse", C.c_uint8), ("accepted", C.c_uint8), ("reserved", C.c_uint8 * 2), ("site_cost", C.c_int32)]


class InvSiteC(C.Structure):
    _fields_ = [("query_start", C.c_uint64), ("query_end", C.c_uint64), ("target_start", C.c_uint64),
                ("target_end", C.c_uint64), ("kind", C.c_int32), ("candidate", C.c_int32)]


class GraphStatsC(C.Structure):
    """sr_graph_stats (include/seqrush_amd.h, graph statistics)"""
    _fields_ = [("length", C.c_uint64), ("nodes", C.c_uint64), ("edges", C.c_uint64), ("paths", C.c_uint64), ("steps", C.c_uint64),
                ("rev_steps", C.c_uint64), ("depth_bp", C.c_uint64),
                ("self_loops", C.c_uint64), ("tips", C.c_uint64), ("components", C.c_uint64),
                ("depth", C.POINTER(C.c_uint32)), ("paths_on", C.POINTER(C.c_uint32)),
                ("bp_by_paths", C.POINTER(C.c_uint64)), ("nodes_by_paths", C.POINTER(C.c_uint64)),
                ("shared", C.POINTER(C.c_uint64)),
                ("path_pairs", C.POINTER(C.c_uint64)), ("path_abs", C.POINTER(C.c_uint64)), ("path_len", C.POINTER(C.c_uint64)),
                ("path_sq", C.POINTER(C.c_uint64)),
                ("total_pairs", C.c_uint64), ("total_abs", C.c_uint64), ("total_len", C.c_uint64), ("total_sq", C.c_uint64 * 3),
                ("stats_us", C.c_uint64), ("kernel_us", C.c_uint64 * 5)]


class BinParamsC(C.Structure):
    """sr_bin_params (include/seqrush_amd.h, path-by-bin coverage)"""
    _fields_ = [("bin_width", C.c_uint64), ("bins", C.c_uint64)]


class PathBinsC(C.Structure):
    """sr_path_bins"""
    _fields_ = [("length", C.c_uint64), ("paths", C.c_uint64), ("bins", C.c_uint64), ("bin_width", C.c_uint64),
                ("cov", C.POINTER(C.c_uint64)), ("inv", C.POINTER(C.c_uint64)),
                ("bin_us", C.c_uint64), ("kernel_us", C.c_uint64 * 3)]


class VizParamsC(C.Structure):
    """sr_viz_params"""
    _fields_ = [("mode", C.c_int), ("path_height", C.c_uint32), ("path_gap", C.c_uint32), ("depth_max", C.c_uint32)]


class GrowthParamsC(C.Structure):
    """sr_growth_params (include/seqrush_amd.h, pangenome growth)"""
    _fields_ = [("seed", C.c_uint64), ("permutations", C.c_uint64)]


class GrowthC(C.Structure):
    """sr_growth"""
    _fields_ = [("length", C.c_uint64), ("paths", C.c_uint64), ("groups", C.c_uint64), ("permutations", C.c_uint64),
                ("exhaustive", C.c_int32), ("variant", C.c_int32),
                ("pan", C.POINTER(C.c_uint64)), ("core", C.POINTER(C.c_uint64)), ("perm", C.POINTER(C.c_uint32)),
                ("bp_by_groups", C.POINTER(C.c_uint64)), ("growth_us", C.c_uint64), ("kernel_us", C.c_uint64 * 4),
                ("seed", C.c_uint64)]


class VariantParamsC(C.Structure):
    """sr_variant_params (include/seqrush_amd.h, variant sites)"""
    _fields_ = [("ref_name", C.c_char_p), ("max_allele_len", C.c_uint64), ("hash_mask", C.c_uint64), ("reserved", C.c_uint64)]


class VariantsC(C.Structure):
    """sr_variants"""
    _fields_ = [("ref_path", C.c_uint64), ("ref_len", C.c_uint64), ("paths", C.c_uint64), ("anchors", C.c_uint64),
                ("traversals", C.c_uint64), ("sites", C.c_uint64), ("hash_collision_sites", C.c_uint64),
                ("breaks", C.POINTER(C.c_uint64)), ("skipped", C.POINTER(C.c_uint64)),
                ("site_start", C.POINTER(C.c_uint64)), ("site_end", C.POINTER(C.c_uint64)), ("site_alleles", C.POINTER(C.c_uint32)),
                ("allele_off", C.POINTER(C.c_uint64)), ("alleles", C.POINTER(C.c_char)), ("gt", C.POINTER(C.c_int32)),
                ("ref_seq", C.POINTER(C.c_char)), ("variant", C.c_int32), ("reserved", C.c_int32),
                ("variants_us", C.c_uint64), ("kernel_us", C.c_uint64 * 6)]


class ExtendStatsC(C.Structure):
    """sr_extend_stats (include/seqrush_amd.h, extending a graph)"""
    _fields_ = [(f, C.c_uint64) for f in ("old_paths", "old_bases", "old_steps", "new_sequences", "pairs_before", "pairs_after",
                                          "unions_attempted", "unions_joined", "spell_us", "seed_us")]


class LiftParamsC(C.Structure):
    """sr_lift_params (include/seqrush_amd.h, lifting intervals)"""
    _fields_ = [("to_name", C.c_char_p), ("min_covered", C.c_uint64), ("short_steps", C.c_uint64), ("reserved", C.c_uint64)]


class LiftC(C.Structure):
    """sr_lift"""
    _fields_ = [("queries", C.c_uint64), ("targets", C.c_uint64), ("paths", C.c_uint64), ("unknown", C.c_uint64),
                ("out_of_range", C.c_uint64), ("mapped", C.c_uint64),
                ("q_path", C.POINTER(C.c_uint32)), ("q_start", C.POINTER(C.c_uint64)), ("q_end", C.POINTER(C.c_uint64)),
                ("label_off", C.POINTER(C.c_uint64)), ("labels", C.POINTER(C.c_char)), ("target_path", C.POINTER(C.c_uint32)),
                ("tstart", C.POINTER(C.c_uint64)), ("tend", C.POINTER(C.c_uint64)), ("covered", C.POINTER(C.c_uint64)),
                ("rev_bp", C.POINTER(C.c_uint64)), ("variant", C.c_int32), ("to_named", C.c_int32), ("min_covered", C.c_uint64),
                ("short_pairs", C.c_uint64), ("long_pairs", C.c_uint64), ("lift_us", C.c_uint64), ("kernel_us", C.c_uint64 * 5)]


class ExtractParamsC(C.Structure):
    """sr_extract_params (include/seqrush_amd.h, extracting a subgraph)"""
    _fields_ = [("context_steps", C.c_uint64), ("merge_distance", C.c_uint64), ("merge_rounds", C.c_uint64), ("reserved", C.c_uint64)]


class ExtractC(C.Structure):
    """sr_extract"""
    _fields_ = [(f, C.c_uint64) for f in ("regions", "unknown", "out_of_range", "in_nodes", "in_edges", "in_steps", "in_paths", "nodes",
                                          "edges", "subpaths", "steps", "bases", "seeds", "by_context", "by_merge", "merge_rounds_run")] + \
               [("level", C.POINTER(C.c_uint32)), ("node_old", C.POINTER(C.c_uint32)), ("edge_from", C.POINTER(C.c_uint32)),
                ("edge_to", C.POINTER(C.c_uint32)), ("sub_path", C.POINTER(C.c_uint32)), ("sub_start", C.POINTER(C.c_uint64)),
                ("sub_end", C.POINTER(C.c_uint64)), ("sub_off", C.POINTER(C.c_uint64)), ("sub_steps", C.POINTER(C.c_uint32)),
                ("variant", C.c_int32), ("extract_us", C.c_uint64), ("kernel_us", C.c_uint64 * 6), ("priv", C.c_void_p)]


class AlignmentsC(C.Structure):
    _fields_ = [
        ("n", C.c_uint64), ("query_idx", C.POINTER(C.c_uint32)), ("target_idx", C.POINTER(C.c_uint32)),
        ("is_reverse", C.POINTER(C.c_uint8)), ("score", C.POINTER(C.c_int32)),
        ("query_start", C.POINTER(C.c_uint64)), ("query_end", C.POINTER(C.c_uint64)),
        ("target_start", C.POINTER(C.c_uint64)), ("target_end", C.POINTER(C.c_uint64)),
        ("cigar_off", C.POINTER(C.c_uint64)), ("cigar_ops", C.POINTER(C.c_uint32)),
    ]


class SeqRushError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"seqrush_amd error {code}: {msg}")
        self.code = code


_lib = None


def load():
    """Load the shared library and declare signatures.  Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(seqrush_amd has no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    vp, u64, i32 = C.c_void_p, C.c_uint64, C.c_int
    PP, PS = C.POINTER(ParamsC), C.POINTER(SeqSetC)
    L.sr_default_params.argtypes = [PP]; L.sr_default_params.restype = None
    L.sr_parse_scores.argtypes = [C.c_char_p, PP]
    L.sr_parse_orientation_scores.argtypes = [C.c_char_p, PP]
    L.sr_parse_sparsification.argtypes = [C.c_char_p, PP]
    L.sr_align_all.argtypes = [PS, PP, C.POINTER(C.POINTER(AlignmentsC))]
    L.sr_alignments_free.argtypes = [C.POINTER(AlignmentsC)]; L.sr_alignments_free.restype = None
    L.sr_alignment_cigar.argtypes = [C.POINTER(AlignmentsC), u64, C.c_char_p, C.c_size_t]
    L.sr_alignment_cigar.restype = C.c_size_t
    L.sr_align_and_unite.argtypes = [PS, PP, C.POINTER(u64)]
    L.sr_uf_find.argtypes = [C.POINTER(u64), u64, u64]; L.sr_uf_find.restype = u64
    L.sr_uf_same.argtypes = [C.POINTER(u64), u64, u64, u64]
    L.sr_write_paf.argtypes = [C.POINTER(AlignmentsC), PS, C.c_char_p]
    L.sr_ctx_create.argtypes = [i32, C.POINTER(vp)]
    L.sr_ctx_destroy.argtypes = [vp]; L.sr_ctx_destroy.restype = None
    L.sr_ctx_set_stream.argtypes = [vp, vp]
    L.sr_ctx_load.argtypes = [vp, PS, PP]
    for f in ("sr_ctx_reset_uf", "sr_ctx_align", "sr_ctx_unite", "sr_ctx_sync"):
        getattr(L, f).argtypes = [vp]
    L.sr_ctx_alignments.argtypes = [vp, C.POINTER(C.POINTER(AlignmentsC))]
    L.sr_ctx_download_uf.argtypes = [vp, C.POINTER(u64)]
    for f in ("sr_ctx_uf_size", "sr_ctx_num_pairs", "sr_ctx_dp_cells"):
        getattr(L, f).argtypes = [vp]; getattr(L, f).restype = u64
    L.sr_ctx_labels_device.argtypes = [vp, vp]
    L.sr_ctx_merge_labels.argtypes = [vp, vp, C.c_uint32]
    L.sr_ctx_download_labels.argtypes = [vp, C.POINTER(u64)]
    L.sr_ctx_merge_labels_host.argtypes = [vp, C.POINTER(u64), C.c_uint32]
    L.sr_ctx_kernel_ms.argtypes = [vp, i32, C.POINTER(C.c_float)]
    L.sr_ctx_align_kernel.argtypes = [vp]; L.sr_ctx_align_kernel.restype = C.c_char_p
    L.sr_ctx_load_paf.argtypes = [vp, PS, PP, C.c_char_p]
    L.sr_unite_paf.argtypes = [PS, PP, C.c_char_p, C.POINTER(u64)]
    L.sr_ctx_build_gfa.argtypes = [vp, PS, C.POINTER(vp), C.POINTER(u64), C.POINTER(u64)]
    L.sr_ctx_counters.argtypes = [vp, C.POINTER(u64)]
    L.sr_ctx_counters_ext.argtypes = [vp, C.POINTER(u64)]
    L.sr_ctx_counters_all.argtypes = [vp, C.POINTER(u64), C.c_uint32]
    L.sr_knobs_doc.restype = C.c_char_p
    L.sr_ctx_tail_deferred.argtypes = [vp, C.POINTER(u64)]
    L.sr_ctx_tail_timeline.argtypes = [vp, C.POINTER(u64), C.c_uint32]
    L.sr_ctx_prio_timeline.argtypes = [vp, C.POINTER(u64), C.c_uint32]
    L.sr_tile_prio_role_host.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
    L.sr_tile_prio_epoch_shift.argtypes = []
    L.sr_tail_shape.argtypes = [i32] * 8 + [C.c_uint32, i32]
    L.sr_ctx_load_pairs.argtypes = [vp, PS, PP, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), u64]
    L.sr_ctx_pairs.argtypes = [vp, C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(u64)]
    L.sr_ctx_num_batches.argtypes = [vp]; L.sr_ctx_num_batches.restype = C.c_uint32
    L.sr_ctx_workspace_report.argtypes = [vp]; L.sr_ctx_workspace_report.restype = C.c_char_p
    L.sr_ctx_run.argtypes = [vp]
    L.sr_ctx_align_all.argtypes = [vp, i32, C.POINTER(C.POINTER(AlignmentsC))]
    L.sr_ctx_pair_results.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)]
    L.sr_ctx_labels_device_u32.argtypes = [vp, vp]
    L.sr_ctx_merge_labels_u32.argtypes = [vp, vp, C.c_uint32]
    L.sr_build_gfa.argtypes = [PS, C.POINTER(u64), C.POINTER(vp), C.POINTER(u64), C.POINTER(u64)]
    L.sr_build_gfa_opts.argtypes = [PS, C.POINTER(u64), i32, C.POINTER(vp), C.POINTER(u64), C.POINTER(u64)]
    L.sr_ctx_build_gfa_opts.argtypes = [vp, PS, i32, C.POINTER(vp), C.POINTER(u64), C.POINTER(u64)]
    L.sr_uf_init_host.argtypes = [C.POINTER(u64), u64, u64]
    L.sr_uf_unite_host.argtypes = [C.POINTER(u64), u64, u64, u64]
    L.sr_uf_merge_labels_host.argtypes = [C.POINTER(u64), u64, C.POINTER(u64), C.c_uint32]
    L.sr_uf_canonical_labels_host.argtypes = [C.POINTER(u64), u64, C.POINTER(u64)]
    L.sr_build_gfa_from_nodes.argtypes = [PS, C.POINTER(u64), i32, C.POINTER(vp), C.POINTER(u64), C.POINTER(u64)]
    SP, PD = C.POINTER(SortParamsC), C.POINTER(C.c_double)
    L.sr_sort_params_default.argtypes = [SP]; L.sr_sort_params_default.restype = None
    L.sr_ctx_build_gfa_sorted.argtypes = [vp, PS, i32, SP, C.POINTER(vp), C.POINTER(u64), C.POINTER(u64)]
    L.sr_sort_gfa.argtypes = [C.c_char_p, SP, C.POINTER(vp), C.POINTER(u64), C.POINTER(u64)]
    L.sr_sgd_layout.argtypes = [C.c_char_p, SP, PD, u64]
    L.sr_sgd_tables.argtypes = [C.c_char_p, SP, SP, C.POINTER(u64), PD, PD, PD, PD]
    L.sr_sort_stats.argtypes = [PD, C.c_uint32]
    L.sr_pair_list.argtypes = [C.c_uint32, PP, C.POINTER(C.POINTER(C.c_uint32)),
                               C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(u64)]
    L.sr_ctx_load_iterative.argtypes = [vp, PS, PP, i32]
    L.sr_ctx_run_iterative.argtypes = [vp]
    L.sr_ctx_iterative_stats.argtypes = [vp, C.POINTER(IterStatsC), C.POINTER(u64), u64]
    L.sr_ctx_iterative_alignments.argtypes = [vp, C.POINTER(C.POINTER(AlignmentsC))]
    L.sr_uf_count_components_host.argtypes = [C.POINTER(u64), u64, u64, C.POINTER(u64)]
    L.sr_iterative_stop_host.argtypes = [C.POINTER(u64), u64, u64, C.POINTER(u64)]
    L.sr_base_cone_reach.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    IP, LP = C.POINTER(C.c_int), C.POINTER(C.c_longlong)
    L.sr_pass_tables_host.argtypes = [IP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, IP, IP, IP, LP, LP, IP, IP, IP, IP]
    L.sr_pass_tile_own.argtypes = [C.c_int]
    PU32 = C.POINTER(C.POINTER(C.c_uint32))
    L.sr_iterative_pair_lists.argtypes = [C.c_uint32, C.POINTER(C.c_uint8), PP, PU32, PU32, C.POINTER(u64), PU32, PU32,
                                          C.POINTER(u64)]
    L.sr_ctx_enable_inversions.argtypes = [vp, C.POINTER(InvParamsC)]
    L.sr_ctx_inversion_stats.argtypes = [vp, C.POINTER(InvStatsC)]
    L.sr_ctx_inversion_jobs.argtypes = [vp, C.POINTER(C.POINTER(InvJobC)), C.POINTER(u64)]
    L.sr_ctx_inversion_alignments.argtypes = [vp, C.POINTER(C.POINTER(AlignmentsC))]
    L.sr_append_paf_tagged.argtypes = [C.POINTER(AlignmentsC), PS, C.c_char_p, C.c_char_p]
    L.sr_inversion_sites_host.argtypes = [C.POINTER(C.c_uint32), u64, u64, C.POINTER(C.POINTER(InvSiteC)), C.POINTER(u64)]
    L.sr_inversion_candidate.argtypes = [u64, u64, u64]
    L.sr_inversion_accept.argtypes = [C.c_int32, C.c_int32]
    L.sr_inversion_scan_device.argtypes = [i32, C.POINTER(C.c_uint32), C.POINTER(u64), u64, u64,
                                           C.POINTER(C.POINTER(InvSiteC)), C.POINTER(C.POINTER(u64)), C.POINTER(u64)]
    PI32 = C.POINTER(C.c_int32)
    L.sr_ctx_inversion_join_stats.argtypes = [vp, C.POINTER(u64)]
    L.sr_inversion_sites_host_join.argtypes = [C.POINTER(C.c_uint32), u64, u64, C.c_uint32, PP, C.POINTER(C.POINTER(InvSiteC)),
                                               C.POINTER(PI32), C.POINTER(u64)]
    L.sr_inversion_accept_site.argtypes = [C.c_int32, C.c_int32]
    L.sr_inversion_scan_device_join.argtypes = [i32, C.POINTER(C.c_uint32), C.POINTER(u64), u64, u64, C.c_uint32, PP, PI32, PI32,
                                                C.POINTER(C.POINTER(InvSiteC)), C.POINTER(C.POINTER(u64)), C.POINTER(PI32),
                                                C.POINTER(u64), C.POINTER(u64)]
    PU32P = C.POINTER(C.POINTER(C.c_uint32))
    L.sr_sketch_device.argtypes = [i32, PS, C.c_uint32, C.POINTER(C.POINTER(u64)), PU32P, PU32P, PU32P]
    L.sr_knn_select_device.argtypes = [i32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.c_uint32,
                                       C.POINTER(C.POINTER(C.c_uint8))]
    L.sr_compact_gfa.argtypes = [C.c_char_p, i32, C.POINTER(vp), C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    L.sr_compact_stats.argtypes = [C.POINTER(u64)]
    PGS = C.POINTER(GraphStatsC)
    L.sr_graph_stats_gfa.argtypes = [C.c_char_p, i32, C.POINTER(PGS)]
    L.sr_graph_stats_free.argtypes = [PGS]; L.sr_graph_stats_free.restype = None
    L.sr_graph_stats_report.argtypes = [PGS, C.POINTER(C.c_char_p), C.POINTER(vp)]
    L.sr_stats_sq_sums_host.argtypes = [C.POINTER(u64), u64, C.POINTER(u64)]
    LP = C.POINTER(LayoutParamsC)
    L.sr_layout_params_default.argtypes = [LP]; L.sr_layout_params_default.restype = None
    L.sr_layout_gfa.argtypes = [C.c_char_p, LP, PD, u64]
    L.sr_layout_tsv.argtypes = [PD, u64, C.POINTER(vp)]
    L.sr_layout_svg.argtypes = [C.c_char_p, PD, u64, C.POINTER(vp)]
    L.sr_layout_quality.argtypes = [C.c_char_p, PD, u64, u64, u64, PD]
    L.sr_layout_stats.argtypes = [PD, C.c_uint32]
    L.sr_layout_resolve.argtypes = [C.c_char_p, LP, LP]
    L.sr_layout_select_host.argtypes = [C.c_char_p, LP, u64, u64, u64, i32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), PD]
    PPB, PVP = C.POINTER(PathBinsC), C.POINTER(VizParamsC)
    L.sr_path_bins_gfa.argtypes = [C.c_char_p, C.POINTER(BinParamsC), i32, C.POINTER(PPB)]
    L.sr_path_bins_free.argtypes = [PPB]; L.sr_path_bins_free.restype = None
    L.sr_path_bins_tsv.argtypes = [PPB, C.POINTER(C.c_char_p), C.POINTER(vp)]
    L.sr_viz_params_default.argtypes = [PVP]; L.sr_viz_params_default.restype = None
    L.sr_path_bins_rgb.argtypes = [PPB, C.POINTER(C.c_char_p), PVP, C.POINTER(vp), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.sr_path_bins_png.argtypes = [PPB, C.POINTER(C.c_char_p), PVP, C.POINTER(vp), C.POINTER(u64)]
    PG, PU32 = C.POINTER(GrowthC), C.POINTER(C.c_uint32)
    L.sr_growth_params_default.argtypes = [C.POINTER(GrowthParamsC)]; L.sr_growth_params_default.restype = None
    L.sr_growth_gfa.argtypes = [C.c_char_p, PU32, C.c_uint32, C.POINTER(GrowthParamsC), i32, C.POINTER(PG)]
    L.sr_growth_free.argtypes = [PG]; L.sr_growth_free.restype = None
    L.sr_growth_groups.argtypes = [C.POINTER(C.c_char_p), u64, i32, PU32, PU32, C.POINTER(C.POINTER(C.c_char_p))]
    L.sr_growth_expected.argtypes = [C.POINTER(u64), C.c_uint32, PD, PD]
    L.sr_growth_fit.argtypes = [PD, C.c_uint32, PD, PD, PU32]
    L.sr_growth_report.argtypes = [PG, C.POINTER(vp)]
    PV = C.POINTER(VariantsC)
    L.sr_variant_params_default.argtypes = [C.POINTER(VariantParamsC)]; L.sr_variant_params_default.restype = None
    L.sr_variants_gfa.argtypes = [C.c_char_p, C.POINTER(VariantParamsC), i32, C.POINTER(PV)]
    L.sr_variants_free.argtypes = [PV]; L.sr_variants_free.restype = None
    L.sr_variants_vcf.argtypes = [PV, C.POINTER(C.c_char_p), C.POINTER(vp)]
    PI = C.POINTER(C.c_int)
    L.sr_mirror_map.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), u64, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32,
                                C.POINTER(C.c_uint32), C.POINTER(u64)]
    L.sr_ctx_orientation_scores.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.sr_mirror_bt_pick.argtypes = [PI, i32]
    L.sr_mirror_bt_rank_transposed.argtypes = [i32]
    L.sr_mirror_bt_tie_host.argtypes = [PI]
    L.sr_mirror_bp_pick_host.argtypes = [PI, PI, PI, PI, i32, i32, PI, PI]
    L.sr_replay_record_ints.argtypes = []
    L.sr_replay_transpose_host.argtypes = [PI, PI]; L.sr_replay_transpose_host.restype = None
    L.sr_replay_match_host.argtypes = [PI, i32, PI, i32, i32, PI]
    PES = C.POINTER(ExtendStatsC)
    L.sr_extend_plan_gfa.argtypes = [C.c_char_p, PS, i32, C.POINTER(vp)]
    L.sr_extend_plan_free.argtypes = [vp]; L.sr_extend_plan_free.restype = None
    L.sr_extend_plan_seqs.argtypes = [vp]; L.sr_extend_plan_seqs.restype = PS
    L.sr_extend_plan_n_old.argtypes = [vp]; L.sr_extend_plan_n_old.restype = C.c_uint32
    L.sr_extend_pair_list.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), u64, PU32P, PU32P, C.POINTER(u64)]
    L.sr_ctx_load_extend.argtypes = [vp, vp, PP]
    L.sr_extend_seed_host.argtypes = [vp, C.POINTER(u64), u64, C.POINTER(u64)]
    L.sr_extend_plan_stats.argtypes = [vp, PES]
    L.sr_ctx_extend_stats.argtypes = [vp, PES]
    PLF = C.POINTER(LiftC)
    L.sr_lift_params_default.argtypes = [C.POINTER(LiftParamsC)]; L.sr_lift_params_default.restype = None
    L.sr_lift_gfa.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(LiftParamsC), i32, C.POINTER(PLF)]
    L.sr_lift_free.argtypes = [PLF]; L.sr_lift_free.restype = None
    L.sr_lift_bed.argtypes = [PLF, C.POINTER(C.c_char_p), C.POINTER(vp)]
    PEX = C.POINTER(ExtractC)
    L.sr_extract_params_default.argtypes = [C.POINTER(ExtractParamsC)]; L.sr_extract_params_default.restype = None
    L.sr_extract_gfa.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), u64, C.POINTER(ExtractParamsC), i32, C.POINTER(PEX)]
    L.sr_extract_free.argtypes = [PEX]; L.sr_extract_free.restype = None
    L.sr_extract_text.argtypes = [PEX, C.POINTER(vp)]
    L.sr_free.argtypes = [vp]; L.sr_free.restype = None
    L.sr_last_error.restype = C.c_char_p
    L.sr_abi_version.restype = i32
    L.sr_device_count.restype = i32
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise SeqRushError(rc, load().sr_last_error().decode(errors="replace"))
