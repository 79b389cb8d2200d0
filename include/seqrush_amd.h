/*
 * seqrush_amd.h -- C ABI of the MI355X-native seqrush hot path
 * (all-vs-all WFA2/biWFA alignment -> match-run extraction -> lock-free
 * bidirected union-find).  Plain pointers and sizes only; no torch types.
 *
 * Each entry point names the reference interface it replaces (paths relative
 * to the pangenome/seqrush checkout).  INTEGRATION.md shows the Rust
 * `extern "C"` binding a seqrush maintainer would add.
 *
 * Error model: every int-returning function returns 0 on success or a
 * negative sr_status; sr_last_error() gives a thread-local message.  Nothing
 * here falls back to a CPU path: without a HIP device every compute entry
 * point fails with SR_ERR_NO_DEVICE.
 */
#ifndef SEQRUSH_AMD_H
#define SEQRUSH_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SR_ABI_VERSION 2

typedef enum {
    SR_OK = 0,
    SR_ERR_INVALID = -1,      /* bad argument / parse error */
    SR_ERR_NO_DEVICE = -2,    /* no HIP device or HIP runtime failure at init */
    SR_ERR_HIP = -3,          /* a HIP call failed */
    SR_ERR_ALPHABET = -4,     /* (unused since ABI 2: every byte value is accepted, like the reference's raw-byte compare) */
    SR_ERR_EMPTY_SEQ = -5,    /* "Empty sequences are not allowed" seqrush.rs:310-317 */
    SR_ERR_UNSUPPORTED = -6,  /* parameter combination not implemented on device */
    SR_ERR_DEVICE_FAULT = -7, /* kernel reported an internal bound violation */
    SR_ERR_IO = -8,
    SR_ERR_NOMEM = -9
} sr_status;

/* -------- inputs --------------------------------------------------------
 * sr_seqset mirrors `&[AlignmentSequence]` (src/aligner.rs:5-9) /
 * `Vec<Sequence{id,data,offset}>` (src/seqrush.rs:272-277): concatenated
 * bases + offsets[n+1] (offset = running sum, seqrush.rs:1818) + names. */
typedef struct {
    uint32_t n;
    const uint8_t *bases;         /* offsets[n] bytes */
    const uint64_t *offsets;      /* n+1 entries, offsets[0] = 0 */
    const char *const *names;     /* n C strings (may be NULL for unite-only use) */
} sr_seqset;

/* lib_wfa2 MemoryMode as used by src/wfa.rs:57,65.  The reference always selects Ultralow (= biWFA); the device
 * keeps full wavefront history only for biWFA's base cases, so SR_MEM_HIGH is refused with SR_ERR_UNSUPPORTED. */
#define SR_MEM_HIGH 0
#define SR_MEM_ULTRALOW 3

/* SparsificationStrategy (grammar src/seqrush.rs:356-431) */
#define SR_SPARSE_NONE 0
#define SR_SPARSE_AUTO 1
#define SR_SPARSE_RANDOM 2
#define SR_SPARSE_CONNECTIVITY 3
#define SR_SPARSE_TREE 4

/* sr_params mirrors allwave::AlignmentParams (src/seqrush.rs:648-666) plus
 * the Args fields the hot path reads (-k, -d, -x; src/seqrush.rs:24-151). */
typedef struct {
    int32_t match_score;        /* must be 0: seqrush.rs:45; the trait impl's own 2,4,4,2,24,1 (allwave_impl.rs:15-23)
                                   is refused, allwave's conversion of a positive match score is not in the reference tree */
    int32_t mismatch_penalty;   /* -S default 0,5,8,2,24,1 (seqrush.rs:45) */
    int32_t gap_open1, gap_ext1;
    int32_t gap_open2, gap_ext2;        /* < 0 : single-piece affine */
    int32_t ori_match, ori_mismatch, ori_gap_open, ori_gap_ext; /* 0,1,1,1 (:49) */
    uint64_t min_match_len;     /* -k (:33), run united iff len >= k (:1311) */
    double max_divergence;      /* -d, < 0 = None */
    int32_t exclude_self;       /* reference passes false (:731) */
    int32_t memory_mode;        /* SR_MEM_ULTRALOW = reference (wfa.rs:57) */
    int32_t sparsify_kind;      /* SR_SPARSE_* (grammar seqrush.rs:356-431).  allwave's selection rules are absent from the
                                   reference tree: the definitions (sr_pairs.cpp "pair list", sr_sketch.hip) are this
                                   project's own and unpinned, random:F included */
    double sparsify_factor;     /* random:F / connectivity:P */
    uint64_t sparsify_seed;
    int32_t canonical_labels;   /* sr_align_and_unite: 1 = return min-Pos labels */
    int32_t device;             /* HIP device ordinal */
    /* pair shard for multi-GPU: this call handles shard `shard_rank` of `shard_count` of the (sparsified) row-major
     * ordered pair list.  The shards are cost-balanced: pairs sorted by |q|*|t| (self pairs: |q|), longest first, each
     * dealt to the rank with the least work so far (longest-processing-time-first; every rank computes the same
     * assignment; equal lengths degenerate to index mod shard_count -- sr_pairs.cpp shard_pairs) */
    uint32_t shard_rank, shard_count;
    /* tree:neighbor[,stranger[,random[,k-mer]]] (seqrush.rs:378-418; extract_tree_pairs_separated call :941-947) */
    uint32_t tree_k_nearest, tree_k_farthest;
    double tree_rand_frac;
    uint32_t tree_kmer;         /* default 16; 1..32 on the device */
} sr_params;

void sr_default_params(sr_params *p);
/* AlignmentScores::parse seqrush.rs:165-217 / parse_orientation :219-250 */
int sr_parse_scores(const char *s, sr_params *p);
int sr_parse_orientation_scores(const char *s, sr_params *p);
/* parse_sparsification seqrush.rs:356-431 */
int sr_parse_sparsification(const char *s, sr_params *p);

/* This rank's ordered pair list (host only, no device needed): what
 * AllPairIterator::with_options(.., exclude_self, .., sparsification) enumerates
 * (src/seqrush.rs:728-735), sharded for multi-GPU (equal sequence lengths assumed: sr_ctx_pairs gives the
 * cost-balanced shard of a loaded context).  tree: needs the sequences -> SR_ERR_UNSUPPORTED here.
 * Free both arrays with sr_free. */
int sr_pair_list(uint32_t n, const sr_params *p, uint32_t **q_out, uint32_t **t_out,
                 uint64_t *count);

/* -------- Seam 1: trait Aligner (src/aligner.rs:27-33) -----------------
 * sr_align_all == AllwaveAligner::align_sequences
 * (src/aligner/allwave_impl.rs:95-149): one call, all sequences, returns one
 * record per ordered pair (self pairs included unless exclude_self). */
typedef struct {
    uint64_t n;                 /* number of alignments */
    uint32_t *query_idx, *target_idx;
    uint8_t *is_reverse;        /* strand '-' <=> 1 (aligner.rs:18) */
    int32_t *score;
    uint64_t *query_start, *query_end, *target_start, *target_end;
    uint64_t *cigar_off;        /* n+1 offsets into cigar_ops */
    uint32_t *cigar_ops;        /* (len << 4) | op ; op: 0 '=' 1 'X' 2 'I' 3 'D'
                                   in the reference's converted alphabet
                                   (src/wfa.rs:25-31: I = query-only, D = target-only) */
} sr_alignments;

int sr_align_all(const sr_seqset *seqs, const sr_params *p, sr_alignments **out);
void sr_alignments_free(sr_alignments *a);
/* CIGAR string of alignment i ("159=1X75=..."), == cigar_bytes_to_string
 * (src/wfa.rs:9-38).  Returns needed length (excl. NUL); writes up to cap. */
size_t sr_alignment_cigar(const sr_alignments *a, uint64_t i, char *buf, size_t cap);

/* -------- Seam 2: fused production path ---------------------------------
 * == SeqRush::new (seqrush.rs:308-336) + align_and_unite_with_allwave
 * (seqrush.rs:611-757): alignment + process_alignment (:1134-1481) +
 * BidirectedUnionFind::unite_matching_region (bidirected_union_find.rs:60-98)
 * entirely on device.  parent_out has 2*N+2 entries: the uf_rush node array
 * (parent | rank << 58, uf_rush lib.rs:228-240) or, with canonical_labels,
 * the minimum Pos of each element's component. */
int sr_align_and_unite(const sr_seqset *seqs, const sr_params *p, uint64_t *parent_out);

/* uf_rush find/same over a returned node array (host side, read-only, no
 * path compression): UFRush::find lib.rs:112-133, same :72-84 */
uint64_t sr_uf_find(const uint64_t *nodes, uint64_t n, uint64_t x);
int sr_uf_same(const uint64_t *nodes, uint64_t n, uint64_t x, uint64_t y);
/* The same forest operations for hosts that build or merge node arrays WITHOUT a device (one thread, plain stores
 * instead of CAS; identical packing, path halving, union by rank and tie rule -- larger index wins -- as
 * uf_rush-0.2.1/src/lib.rs:112-208):
 *   sr_uf_init_host             SeqRush::new state (src/seqrush.rs:308-336) for total_len bases, n >= 2*total_len+2
 *   sr_uf_unite_host            UFRush::unite (lib.rs:159-208); returns 1 if two sets were joined, 0 if already one,
 *                               negative on an index out of range (the reference panics, lib.rs:113)
 *   sr_uf_merge_labels_host     SURVEY 8(e) merge: replay unite(i, labels_g[i]) for `count` gathered canonical label
 *                               arrays (n entries each, back to back) into `nodes` -- the host twin of
 *                               sr_ctx_merge_labels, for a Rust host that gathers per-GPU labels itself
 *   sr_uf_canonical_labels_host minimum element of every set (== sr_ctx_download_labels of that forest) */
int sr_uf_init_host(uint64_t *nodes, uint64_t n, uint64_t total_len);
int sr_uf_unite_host(uint64_t *nodes, uint64_t n, uint64_t x, uint64_t y);
int sr_uf_merge_labels_host(uint64_t *nodes, uint64_t n, const uint64_t *labels, uint32_t count);
int sr_uf_canonical_labels_host(const uint64_t *nodes, uint64_t n, uint64_t *labels_out);

/* -------- Seam 3: PAF interchange (seqrush.rs:510-609, 678-716) -------- */
int sr_write_paf(const sr_alignments *a, const sr_seqset *seqs, const char *path);

/* -------- resident-context API (what bench.py times) --------------------
 * Same path split so inputs can stay in HBM across calls. */
typedef struct sr_ctx sr_ctx;
int sr_ctx_create(int device, sr_ctx **out);
void sr_ctx_destroy(sr_ctx *c);
/* optional: launch on an externally owned hipStream_t (NULL: the null stream).  The context's own stream is synchronized
 * and destroyed here; a caller's stream that the context gives up is NOT waited for: change streams only after
 * sr_ctx_sync(), or the work still queued on the old stream and the first call on the new one are unordered.  The stream
 * may be blocking or non-blocking: every call that copies to or from the host waits for the context's stream itself. */
int sr_ctx_set_stream(sr_ctx *c, void *hip_stream);
/* pack (2 / 4 / 8 bits per symbol by alphabet; forward + reverse complement) and upload; pair list (sparsified:
 * k-mer sketches on the device), cost-balanced shard, SeqRush::new UF init */
int sr_ctx_load(sr_ctx *c, const sr_seqset *seqs, const sr_params *p);
/* the same with an explicit ordered pair list instead of the enumeration: the per-pair call pattern of the
 * reference's iterative mode (AllPairIterator over a 2-sequence slice, src/seqrush.rs:984-1012) and of
 * seqrush_clean (src/seqrush_clean.rs:289-292) without re-uploading the sequences; sharded like sr_ctx_load */
int sr_ctx_load_pairs(sr_ctx *c, const sr_seqset *seqs, const sr_params *p, const uint32_t *query_idx,
                      const uint32_t *target_idx, uint64_t count);
/* this rank's pair list of the loaded context (after sparsification and sharding); free with sr_free */
int sr_ctx_pairs(const sr_ctx *c, uint32_t **q_out, uint32_t **t_out, uint64_t *count);
/* The CIGAR arena holds |q|+|t|+2 ops per pair; when the shard's pairs do not fit device memory at once they run in
 * batches that reuse it (1 for every BASELINE config up to C4; C5 on one GPU: several) */
uint32_t sr_ctx_num_batches(const sr_ctx *c);
/* JSON object describing the sizing of the last load (workgroups, ring / history / arena bytes ...) */
const char *sr_ctx_workspace_report(const sr_ctx *c);
/* reset the UF to the SeqRush::new state (seqrush.rs:324-328) */
int sr_ctx_reset_uf(sr_ctx *c);
/* enqueue alignment kernel(s) for this rank's pair shard (no host sync); single-batch contexts only */
int sr_ctx_align(sr_ctx *c);
/* enqueue match-run extraction + unite kernel (no host sync); single-batch contexts only */
int sr_ctx_unite(sr_ctx *c);
/* align + unite of the whole shard, batch after batch (no host sync): == sr_ctx_align + sr_ctx_unite when there
 * is one batch; for a PAF context: unite only */
int sr_ctx_run(sr_ctx *c);
/* Seam 1 on a loaded context: every alignment of the shard on the host (batches are copied out one after the
 * other); unite != 0 also unites each batch (--output-alignments without the reference's second pass) */
int sr_ctx_align_all(sr_ctx *c, int unite, sr_alignments **out);
/* per-pair results that stay resident across batches (arrays of sr_ctx_num_pairs; NULL = skip): score (-1 = failed),
 * strand flag, number of run-length CIGAR ops */
int sr_ctx_pair_results(sr_ctx *c, int32_t *score, uint8_t *is_reverse, uint32_t *cigar_ops);
int sr_ctx_sync(sr_ctx *c);     /* stream sync + device error flags */
/* results */
int sr_ctx_alignments(sr_ctx *c, sr_alignments **out);       /* after sync */
int sr_ctx_download_uf(sr_ctx *c, uint64_t *parent_out);     /* raw nodes */
uint64_t sr_ctx_uf_size(const sr_ctx *c);                    /* 2N+2 */
uint64_t sr_ctx_num_pairs(const sr_ctx *c);                  /* this shard */
uint64_t sr_ctx_dp_cells(const sr_ctx *c);   /* sum |q|*|t| over this shard */
/* multi-GPU merge: canonical min-Pos labels of the local forest
 * written to a DEVICE buffer of uf_size u64 (e.g. a torch tensor's data_ptr);
 * sr_ctx_merge_labels replays unite(i, labels[i]) for `count` gathered arrays
 * laid out back to back in DEVICE memory. */
int sr_ctx_labels_device(sr_ctx *c, uint64_t *dev_labels);
int sr_ctx_merge_labels(sr_ctx *c, const uint64_t *dev_labels, uint32_t count);
/* the same exchange with 32-bit labels (valid while 2N+2 < 2^32: half the all-gather bytes) */
int sr_ctx_labels_device_u32(sr_ctx *c, uint32_t *dev_labels);
int sr_ctx_merge_labels_u32(sr_ctx *c, const uint32_t *dev_labels, uint32_t count);
int sr_ctx_download_labels(sr_ctx *c, uint64_t *labels_out);
/* the merge with `count` label arrays resident on the HOST (uf_size entries each): hosts without a collective
 * library exchange the arrays through files (seqrush_mi355x --shard R/N --labels-out / --labels-in) */
int sr_ctx_merge_labels_host(sr_ctx *c, const uint64_t *labels, uint32_t count);
/* Seam 3, input side (`seqrush -p file.paf`, src/seqrush.rs:510-609): replaces sr_ctx_load + sr_ctx_align.
 * Every record of the PAF file whose names are known and that carries a cg:Z: tag is replayed through
 * process_alignment's rules (src/seqrush.rs:1134-1481: bases of M/= ops are compared, runs >= min_match_len
 * are united, query_start/target_start honoured, strand '-' = reverse-complemented query); follow with
 * sr_ctx_unite.  Records are sharded over ranks like the pair list.  sr_unite_paf is the fused form of
 * load + unite + download (raw uf_rush nodes, or canonical labels with p->canonical_labels). */
int sr_ctx_load_paf(sr_ctx *c, const sr_seqset *seqs, const sr_params *p, const char *paf_path);
int sr_unite_paf(const sr_seqset *seqs, const sr_params *p, const char *paf_path, uint64_t *parent_out);
/* graph induction on the device from the context's union-find (node ids in first-
 * encounter order, node bases, path steps, deduplicated edges; src/bidirected_builder.rs:17-289,
 * src/bidirected_ops.rs:813-825) + GFA text formatted on the host.  Byte-identical to sr_build_gfa() on the
 * canonical labels of the same context; *gfa is malloc'ed (sr_free). */
int sr_ctx_build_gfa(sr_ctx *c, const sr_seqset *seqs, char **gfa, uint64_t *n_nodes, uint64_t *n_edges);
/* timing of the last enqueued kernels, measured with hipEvents on the
 * context's stream: which = 0 align (the alignment kernel proper), 1 unite, 2 labels/merge, 3 graph induction,
 * 4 the orientation kernel (when orientation runs as its own kernel before the alignment kernel) */
int sr_ctx_kernel_ms(sr_ctx *c, int which, float *ms);
/* name of the alignment kernel the loaded context launches ("sr_align_blk_kernel",
 * "sr_align_bfs_kernel" or "sr_align_kernel"), NULL before sr_ctx_load */
const char *sr_ctx_align_kernel(const sr_ctx *c);
/* device counters accumulated by the last align: [0] wavefront cells,
 * [1] wavefront steps, [2] base-case segments, [3] breakpoint searches,
 * [4] united bases (after unite), [5] match runs, [6] orientation: wavefront cells of the orientation kernel (or,
 * when orientation runs inside the alignment kernel, its 100 MHz ticks), [7..8] 100 MHz ticks summed
 * over workgroups: breakpoint search, base cases; [9] breakpoint-
 * search passes; [10] ticks of whole pairs; [11..15] ticks inside the breakpoint
 * search: wavefront pass, barrier wait, phase-1 control, breakpoint detection, tail */
int sr_ctx_counters(sr_ctx *c, uint64_t out[16]);
/* the same plus [16] bytes of wavefront rows loaded, [17] stored by the alignment kernel's tiles (every lane access of
 * every tile counted on the device: the kernel's algorithmic HBM bytes, bench.py roofline); [18..31] reserved.
 * The tick counters [6..15] are filled only by the instrumented kernel instance (environment SR_PROFILE_TICKS=1). */
int sr_ctx_counters_ext(sr_ctx *c, uint64_t out[32]);
/* every slot (48 since ABI 2 / round 4): [32..35] tile stamps of the diagnostic build (cycles waiting for a tile's first
 * rows, cycles in its levels, tiles, extension-loop iterations), [36] bytes of wavefront rows that stayed in LDS
 * (LDS-resident histories of small base cases), [37] base cases searched again with the worst-case history region,
 * [40..43] first offending access of the bounds-checked build (pair, level, row offset, extent), [48..51] replay of tied
 * secondaries (52 slots): tied primaries with a tie-sensitive depth-0 search, ties in base cases only, secondaries replayed,
 * searches they took from records; [52..53] rotating tile priority (54 slots): workgroups of the main launches that took a
 * rank on their CU, the largest arrival count of a CU; rest reserved.
 * Returns the number of slots written (<= cap) or a negative sr_status. */
int sr_ctx_counters_all(sr_ctx *c, uint64_t *out, uint32_t cap);
/* "NAME<TAB>meaning when unset<TAB>what it does" lines of every environment variable the load path reads; the ones that
 * are set are listed under "knobs" in sr_ctx_workspace_report() */
const char *sr_knobs_doc(void);
/* Tail launch of the blocked alignment kernel.  sr_ctx_tail_deferred: secondaries the main launches handed
 * to their wide tail launch since the counters were last reset (summed over the batches of the pass; <= counter mirror_ties).
 * The workspace report's "tail_threads" is the tail launch's shape, 0 = the load has none. */
int sr_ctx_tail_deferred(sr_ctx *c, uint64_t *out);
/* Per-workgroup timeline of the last main launch of the instrumented instance (SR_PROFILE_TICKS=1), 4 words per workgroup:
 * 100 MHz ticks of its first dequeue, of the start of its last alignment and of its exit, and alignments run | (1 << 32 when
 * the last one was a secondary taken over from its own primary).  Returns the workgroups written (<= cap_wg), 0 when the load
 * does not run the instrumented instance, or a negative sr_status. */
int sr_ctx_tail_timeline(sr_ctx *c, uint64_t *out, uint32_t cap_wg);
/* Rotating tile priority of the blocked alignment kernel.  sr_ctx_prio_timeline: the instrumented instance's
 * second record of the same launch, 4 words per workgroup: tick of the end of its first alignment, its rank among the
 * workgroups of its CU, the CU's index in the arrival table, its arrival count there; returns as sr_ctx_tail_timeline.
 * sr_tile_prio_role_host: the rule the kernel runs (s_setprio level 0..3 of a workgroup's tile code from its rank, the epoch =
 * 100 MHz real-time counter >> sr_tile_prio_epoch_shift(), and the workgroups per CU; 1 per CU: always 0).  Pure (host only).
 * The workspace report carries "tile_prio" (0 under SR_TILE_PRIO=0 or with one workgroup per CU) and "prio_epoch_shift". */
int sr_ctx_prio_timeline(sr_ctx *c, uint64_t *out, uint32_t cap_wg);
int sr_tile_prio_role_host(uint32_t rank, uint32_t epoch, uint32_t wg_per_cu);
int sr_tile_prio_epoch_shift(void);
/* The tail launch's threads per workgroup for a plan: the widest instance of the blocked kernel wider than main_threads whose
 * LDS (static tables + four copies of max_words words) fits the 128 KB window, 0 = none.  forced > 0 (SR_TAIL_THREADS): the
 * widest instance <= forced instead.  Pure (host only). */
int sr_tail_shape(int impl, int block_levels, int wave_build, int off16, int ring_u16, int symbol_bits, int two_piece,
                  int main_threads, uint32_t max_words, int forced);

/* -------- iterative mode (`seqrush --iterative`, align_and_unite_iterative src/seqrush.rs:867-1132) ---------------
 * Tree entries ({i<j} picked by the k-NN selection of -x tree:, row-major) are aligned and united first; then the random
 * entries (the other pairs of the tree: list, in a seeded shuffle, sr_pairs.cpp "pair list") in chunks of 10, with a
 * component count after every full chunk; the run stops once 10 checks in a row saw no change (:1034-1122).  Each entry
 * aligns (i,i) (i,j) (j,i) (j,j).  A -x other than tree: is replaced by tree:3,3,0.1,16 (tree_defaulted).  One context,
 * no shards.  The union-find holds exactly the processed alignments; the stop point does not depend on the schedule. */
typedef struct {
    uint64_t tree_entries;      /* unordered tree pairs (4 alignments each) */
    uint64_t random_entries;    /* unordered random pairs */
    uint64_t random_processed;  /* random entries united: 10 per check up to the stop, or all */
    uint64_t random_aligned;    /* random entries aligned (the last window may hold entries after the stop) */
    uint64_t checks;            /* component counts taken in phase 2 */
    uint64_t windows;           /* phase-2 alignment windows */
    uint64_t post_tree;         /* components after phase 1 */
    uint64_t final_components;  /* components at the end */
    int32_t stabilized;         /* 1 = the stop rule fired */
    int32_t tree_defaulted;     /* 1 = -x was not tree:, tree:3,3,0.1,16 was used */
    uint32_t tree_k_nearest, tree_k_farthest;   /* the tree spec used */
    double tree_rand_frac;
    uint32_t tree_kmer;
    uint32_t reserved;
} sr_iter_stats;
/* sequences + the two lists (k-NN selection on the device); keep_alignments != 0: sr_ctx_iterative_alignments afterwards */
int sr_ctx_load_iterative(sr_ctx *c, const sr_seqset *seqs, const sr_params *p, int keep_alignments);
/* both phases to the end (host syncs once per window; a second run starts again from SeqRush::new) */
int sr_ctx_run_iterative(sr_ctx *c);
/* stats of the last run + its per-check component counts (up to cap entries; NULL = skip) */
int sr_ctx_iterative_stats(sr_ctx *c, sr_iter_stats *out, uint64_t *check_counts, uint64_t cap);
/* the processed alignments of the last run in processing order (--output-alignments); ownership passes to the caller
 * (sr_alignments_free), so a second call fails until the next run */
int sr_ctx_iterative_alignments(sr_ctx *c, sr_alignments **out);
/* host twins (no device): count_components (:341-353) of a SeqRush node array = roots among nodes [0, 2 total_len);
 * the stop rule over per-check counts (*stop_check = checks consumed when it fired, 0 = never); the two entry lists for a
 * given n*n k-NN selection (sel[i*n+j] = j picked by i; NULL = none) -- free the four arrays with sr_free */
int sr_uf_count_components_host(const uint64_t *nodes, uint64_t n, uint64_t total_len, uint64_t *count);
int sr_iterative_stop_host(const uint64_t *counts, uint64_t nchecks, uint64_t post_tree, uint64_t *stop_check);
int sr_iterative_pair_lists(uint32_t n, const uint8_t *sel, const sr_params *p, uint32_t **tree_i, uint32_t **tree_j,
                            uint64_t *tree_count, uint32_t **rand_i, uint32_t **rand_j, uint64_t *rand_count);
/* host twin of the blocked alignment kernel's base-case cone: a level with `levels_left` levels to its job's last one
 * computes the diagonals within this many of the end diagonal tlen - plen (< 0: none) */
int sr_base_cone_reach(int e1, int e2, int two, int levels_left);
/* host twin of the blocked alignment kernel's pass tables (csrc/sr_pass_rule.h), organised as the kernel is: per-level ranges
 * and cells by (aligner, level) lanes, 64 / B aligners per step, then window, tile count and tile prefix per aligner.
 * pen6 = x, o1, e1, o2, e2, two; jobs = njobs records of 7 ints (active, begin component, plen, tlen, shift, kend, levels
 * given); base: base cases (ranges and window cut to the backward cone).  klo / khi: [B][njobs], written for active aligners
 * only; cells / ccells: the aligners' unclipped / clipped cells, ADDED to the arrays; tstart: njobs + 1 entries.  Returns the
 * lane steps taken, < 0 for arguments no instance has.  sr_pass_tile_own: 4-diagonal groups a tile of a B-level block owns. */
int sr_pass_tables_host(const int *pen6, int scope, int B, int tight, int base, int s0, int njobs, const int *jobs, int *klo,
                        int *khi, long long *cells, long long *ccells, int *glo, int *ghi, int *nt, int *tstart);
int sr_pass_tile_own(int B);
/* Mirror partners of the blocked alignment kernel: when a batch holds (q, t) and (t, q), the first (q, t) with
 * q < t is the primary and the first (t, q) its secondary; the kernel aligns the primary and writes the secondary's result as
 * the transposed CIGAR unless a tie-break decided something (then it aligns the secondary too).  mirror_out[i] = the
 * partner's index inside i's batch, top bit set on the secondary, 0xffffffff = no partner.  batch_first: nbatch + 1 pair
 * indices (NULL = one batch).  A batch with no more pairs than `workgroups` (what its launch has; 0 = pair every batch) gets
 * no partners: every pair has a workgroup there and mirroring could only lengthen the launch.  *partners_out = number of
 * primaries (the workspace report's "mirror_partners"). */
int sr_mirror_map(const uint32_t *query_idx, const uint32_t *target_idx, uint64_t count, const uint32_t *batch_first,
                  uint32_t nbatch, uint32_t workgroups, uint32_t *mirror_out, uint64_t *partners_out);
/* per pair of the loaded list: what the orientation search of the last alignment stage found (orientation penalties; F, R =
 * the forward and the reverse-complement score).  Only the winner's score is exact:
 *   reverse strand chosen (R < F): rev = R, fwd = -1 (the forward orientation was not searched to the end)
 *   forward strand chosen:         fwd = F, rev = INT32_MAX (the reverse orientation was not searched to the end)
 * except that a pair the orientation kernel decides by its bounds alone (2-bit symbols, penalties 0,1,1,1: the alignment
 * along diagonal 0 closed by one end gap costs less than the 8-mer lower bound of R) reports that diagonal-0 upper bound
 * of F in fwd, not F itself; the values order the alignment queue.  Either pointer may be NULL */
int sr_ctx_orientation_scores(sr_ctx *c, int32_t *fwd, int32_t *rev);
/* host twins of the kernel's tie rules (csrc/sr_mirror_rule.h).  Backtrace, M step: off[1..9] = candidate offsets of the tags
 * I1o I1e I2o I2e D1o D1e D2o D2e MISMS (< 0: none; off[0] unused) -> the tag picked by this pair's order (transposed = 0)
 * or the transposed pair's (1), 0 = none; the transposed pair's priority of a tag; 1 = the kernel flags the step.  Breakpoint
 * call: n candidates (value, distance, component 0..4 = M I1 I2 D1 D2, diagonal) -> the index either walk accepts, returns
 * 1 = the kernel flags the call. */
int sr_mirror_bt_pick(const int *off, int transposed);
int sr_mirror_bt_rank_transposed(int tag);
int sr_mirror_bt_tie_host(const int *off);
int sr_mirror_bp_pick_host(const int *val, const int *dist, const int *comp, const int *diag, int n, int value_bias,
                           int *pick_out, int *pick_t_out);
/* Replay of a tied secondary from its primary's breakpoints (csrc/sr_mirror_rule.h; SR_MIRROR_REPLAY=0 switches
 * it off, the workspace report has "mirror_replay").  Host twins: ints per breakpoint record (level, pb pe tb te cb ce, bv bh
 * bcomp bsf bsr, tie bit, cells lo/hi, passes); the transposed record; the kernel's walk of one recursion level -- nrec records
 * in list order, nseg segments under search of six ints (pb pe tb te cb ce) in list order -> match_out[i] = index of the
 * untied record of `level` that is segment i's transpose, -1 = the segment is searched; returns the number matched. */
int sr_replay_record_ints(void);
void sr_replay_transpose_host(const int *rec, int *out);
int sr_replay_match_host(const int *recs, int nrec, const int *segs, int nseg, int level, int *match_out);

/* -------- inversion patching (`--patch-inversions`; src/inversion_aware_seqrush.rs:118-255, src/cigar_analysis.rs:23-147) ----
 * After each batch's alignment kernel the device scans every CIGAR for two-sided gaps between match ops (qgap / tgap =
 * query- / target-only + mismatch columns, both >= m and 2 max <= 3 min; m = min_size or 2 * min_match_len).  Each such gap
 * becomes a job: the reverse complement of the aligned query's gap segment against the target's, same penalties, orientation
 * forced (the reference flips the target segment; this library flips the query, where its strand flag lives).  A patch is
 * accepted when 0 <= patch score < main score / 2 and, with max_divergence, patch score <= max_score_for_divergence(min(qgap,
 * tgap)); accepted patches are united like any alignment, strand = negated main strand.  Patches are not rescanned.
 * sr_ctx_enable_inversions: after a load, before a run; NULL = off.  Honoured by sr_ctx_run and sr_ctx_align_all(unite = 1)
 * (which then sync once per batch to read the job list).  Refused on PAF and iterative contexts (SR_ERR_UNSUPPORTED) and
 * with a resolved m of 0 (SR_ERR_INVALID).  The patch pass runs on whichever kernel family the penalties select.
 * Joined mode (`--inversion-join J`, join_below = J >= 1; 0 = off, everything above as it is): only match ops of at least J
 * columns (anchors) open and close gaps; the columns of shorter ones (islands) count towards qgap and tgap like mismatches, so
 * an inversion whose gap the main alignment split around a few chance matches is one gap again.  Each job carries its site
 * cost: what the main alignment paid for the gap's ops under the run's penalties (X: len x; an I or D run: min(o1 + len e1,
 * o2 + len e2); island: 0).  A patch is then accepted when 0 <= patch score < site cost / 2 (in place of main score / 2,
 * which joined SNP clusters pass), and under the -d bound as above.  J > m is SR_ERR_INVALID; J <= min_match_len is the
 * sensible range. */
typedef struct {
    uint64_t min_size;          /* 0 = 2 * min_match_len */
    int32_t keep_alignments;    /* != 0: sr_ctx_inversion_alignments afterwards */
    uint32_t join_below;        /* J of the joined mode; 0 = off */
} sr_inv_params;
typedef struct {
    uint64_t scanned;           /* alignments scanned (failed ones and those dropped by -d are not) */
    uint64_t sites;             /* gaps of any kind (divergent, query-only, target-only) */
    uint64_t candidates;        /* = jobs */
    uint64_t accepted;
    uint64_t rejected_score;    /* patch score >= main score / 2 (joined mode: >= site cost / 2) */
    uint64_t rejected_divergence;   /* passed the score rule, above the -d bound */
    uint64_t united_bases;      /* bases united from accepted patches */
    uint64_t patch_batches;     /* alignment kernel launches of the patch pass (0 without candidates) */
    double scan_ms, patch_align_ms;     /* hipEvents on the context's stream: the scan's kernels (count, offsets, emit) of
                                           every batch, without the host's reads between them; the patch alignment kernels */
} sr_inv_stats;
typedef struct {
    uint64_t pair;              /* index in sr_ctx_pairs */
    uint32_t query_idx, target_idx;
    uint64_t query_start, query_end;    /* forward-strand query range */
    uint64_t target_start, target_end;
    int32_t main_score, patch_score;
    uint8_t is_reverse;         /* the patch's strand: '-' <=> 1 */
    uint8_t accepted;
    uint8_t reserved[2];
    int32_t site_cost;          /* joined mode: what the main alignment paid for this gap; 0 when off */
} sr_inv_job;
int sr_ctx_enable_inversions(sr_ctx *c, const sr_inv_params *p);
int sr_ctx_inversion_stats(sr_ctx *c, sr_inv_stats *out);
/* joined mode, last run: [0] islands inside the candidate gaps, [1] jobs rejected by the site-cost rule, [2] host
 * microseconds of the patch pass on a host clock, from the download of the bases through the segment set and the load of
 * the segment set (index, packing, uploads, planning, allocation) to just before that load's first kernel; the uploads of
 * the jobs' starts and bounds after it are outside (any run with jobs, joined or not), [3] reserved */
int sr_ctx_inversion_join_stats(sr_ctx *c, uint64_t out[4]);
/* the jobs of the last run in pair order, then CIGAR order; *jobs is malloc'ed (sr_free) */
int sr_ctx_inversion_jobs(sr_ctx *c, sr_inv_job **jobs, uint64_t *count);
/* the accepted patches of the last run in job order, start / end filled (forward-strand query coordinates, as PAF wants
 * them); ownership passes to the caller, so a second call fails until the next run */
int sr_ctx_inversion_alignments(sr_ctx *c, sr_alignments **out);
/* sr_write_paf that appends to `path` and adds one more tag column (e.g. "sr:Z:inv") to every record; tag NULL = none */
int sr_append_paf_tagged(const sr_alignments *a, const sr_seqset *seqs, const char *path, const char *tag);
/* host twins (no device).  ops: one alignment in the sr_alignments encoding.  Sites come back in CIGAR order with the
 * coordinates of cigar_analysis.rs:80-105 (a one-sided site has an empty range on the other side); free with sr_free */
#define SR_INV_SITE_DIVERGENT 1
#define SR_INV_SITE_QUERY_ONLY 2
#define SR_INV_SITE_TARGET_ONLY 3
typedef struct {
    uint64_t query_start, query_end, target_start, target_end;
    int32_t kind;               /* SR_INV_SITE_* */
    int32_t candidate;          /* sr_inversion_candidate of its gaps */
} sr_inv_site;
int sr_inversion_sites_host(const uint32_t *ops, uint64_t n_ops, uint64_t min_size, sr_inv_site **sites, uint64_t *count);
int sr_inversion_candidate(uint64_t qgap, uint64_t tgap, uint64_t min_size);    /* 1 / 0; min_size 0: SR_ERR_INVALID */
int sr_inversion_accept(int32_t patch_score, int32_t main_score);               /* 1 / 0 */
/* the joined rule: sites with join_below = J (1 <= J <= min_size, else SR_ERR_INVALID) and, in *cost, each site's cost under
 * the penalties of `pen` (only its score fields are read); both sr_free */
int sr_inversion_sites_host_join(const uint32_t *ops, uint64_t n_ops, uint64_t min_size, uint32_t join_below, const sr_params *pen,
                                 sr_inv_site **sites, int32_t **cost, uint64_t *count);
int sr_inversion_accept_site(int32_t patch_score, int32_t site_cost);           /* 1 / 0 */
/* tests: the device scan over `n` alignments given like sr_alignments (cigar_off[n + 1], ops in its encoding): the jobs
 * as sites with kind SR_INV_SITE_DIVERGENT, and their alignment index in *owner (both sr_free) */
int sr_inversion_scan_device(int device, const uint32_t *ops, const uint64_t *cigar_off, uint64_t n, uint64_t min_size,
                             sr_inv_site **sites, uint64_t **owner, uint64_t *count);
/* tests: the joined instances of the device scan.  score / max_score: per alignment or NULL (an alignment with score < 0 or
 * score > max_score is not scanned); *cost: the jobs' site costs (sr_free); stats (or NULL): alignments scanned, sites,
 * candidates, islands inside candidates */
int sr_inversion_scan_device_join(int device, const uint32_t *ops, const uint64_t *cigar_off, uint64_t n, uint64_t min_size,
                                  uint32_t join_below, const sr_params *pen, const int32_t *score, const int32_t *max_score,
                                  sr_inv_site **sites, uint64_t **owner, int32_t **cost, uint64_t *count, uint64_t stats[4]);
/* tests: the stages of the tree: selection on `device` for `seqs` and k-mer size `kmer` (1..32): sketch = n rows of 1000
 * u64, the first sketch_n[i] of row i ascending, the rest of the row still the fill value 2^64-1; shared / denom = n*n u32
 * (diagonal 0).  All four sr_free. */
int sr_sketch_device(int device, const sr_seqset *seqs, uint32_t kmer, uint64_t **sketch, uint32_t **sketch_n,
                     uint32_t **shared, uint32_t **denom);
/* tests: sr_knn_select_kernel on given n*n shared / denom matrices: sel[i*n+j] bit 0 = j among i's k_nearest, bit 1 = among
 * its k_farthest (both clamped to n like the load path does).  sr_free. */
int sr_knn_select_device(int device, const uint32_t *shared, const uint32_t *denom, uint32_t n, uint32_t k_nearest,
                         uint32_t k_farthest, uint8_t **sel);

/* -------- consumer (A9): graph induction + GFA, host C++ -----------------
 * build_bidirected_graph_with_options (bidirected_builder.rs:17-289) +
 * write_gfa (bidirected_ops.rs:880-925) for --no-sort --no-compact, from
 * canonical labels.  Returns malloc'd text in *gfa (free with sr_free). */
int sr_build_gfa(const sr_seqset *seqs, const uint64_t *labels, char **gfa,
                 uint64_t *n_nodes, uint64_t *n_edges);
/* the same with the reference's post-induction step for `--no-sort` without `--no-compact`
 * (src/bidirected_gfa_writer.rs:39-51): compact() merges linear chains of perfect neighbours round after round
 * (src/bidirected_ops.rs:91-490), renumber_nodes_sequentially() (:75-89); compact == 0 is sr_build_gfa */
int sr_build_gfa_opts(const sr_seqset *seqs, const uint64_t *labels, int compact, char **gfa,
                      uint64_t *n_nodes, uint64_t *n_edges);
/* Induction from a RAW uf_rush node array with the reference's root rule (src/bidirected_builder.rs:46-48, 176-182: a
 * node's base is the base at the offset of union_find.find(pos), i.e. of the component's ROOT): the entry point for a
 * host that wants byte equality with a reference run -- node orientation on reverse-complement components included --
 * by replaying the unites in a fixed order (its own uf_rush, or sr_uf_unite_host).  The canonical entry points above
 * relabel every component to its minimum Pos first (schedule-independent). */
int sr_build_gfa_from_nodes(const sr_seqset *seqs, const uint64_t *nodes, int compact, char **gfa,
                            uint64_t *n_nodes, uint64_t *n_edges);
int sr_ctx_build_gfa_opts(sr_ctx *c, const sr_seqset *seqs, int compact, char **gfa, uint64_t *n_nodes, uint64_t *n_edges);

/* -------- Ygs layout (`seqrush` without --no-sort; src/bidirected_gfa_writer.rs:53-117, src/ygs_sort.rs:96-162) ----
 * Y: path-guided SGD, deterministic (counter-based draws, Zipf by table, sub-rounds with order-free int64 accumulation;
 *    DESIGN.md section 8): the device result is bit-identical to the host twin's;
 * g: BFS grooming from the head nodes (flipped nodes store their reverse complement);
 * s: topological sort seeded by the head nodes.  Node ids come out dense 1..N in the final order, edges sorted.
 * Every path must still spell what it spelled before the sort, else SR_ERR_DEVICE_FAULT and no GFA.
 * Zero fields are derived from the graph like YgsParams::from_graph (src/ygs_sort.rs:50-95). */
#define SR_SORT_DEVICE_HOST_TWIN (-1)     /* the batched SGD on one host thread (bit-identical to the device) */
#define SR_SORT_DEVICE_SEQUENTIAL (-2)    /* every term applied at once, like the reference with one thread (yardstick) */
typedef struct {
    uint64_t seed;              /* counter-based draws: splitmix64(seed, iteration, term, draw) */
    uint64_t iter_max;          /* 100: iterations 0..iter_max, as the reference's checker runs them */
    double theta;               /* 0.99; cooling iterations use 0.001 */
    double eps;                 /* 0.01 */
    double eta_max;             /* 0 = (longest path's step count)^2 */
    double cooling_start;       /* 0.5: cooling for iterations > floor(cooling_start * iter_max) */
    uint64_t space;             /* 0 = longest path length in bp */
    uint64_t space_max;         /* 100 */
    uint64_t space_quant;       /* 100 */
    uint64_t min_term_updates;  /* 0 = total path steps: terms per iteration */
    uint64_t terms_per_round;   /* terms per sub-round (0 = default) */
    int32_t skip_sgd, skip_groom, skip_topo;   /* the reference's hidden --skip-* flags (src/seqrush.rs:90-99) */
    int32_t device;             /* >= 0: HIP device, SR_SORT_DEVICE_HOST_TWIN, SR_SORT_DEVICE_SEQUENTIAL */
} sr_sort_params;
void sr_sort_params_default(sr_sort_params *p);
/* induction on the device, optional compaction + renumbering, Ygs, GFA text (device >= 0 runs the SGD on the context's
 * device and stream) */
int sr_ctx_build_gfa_sorted(sr_ctx *c, const sr_seqset *seqs, int compact, const sr_sort_params *p, char **gfa,
                            uint64_t *n_nodes, uint64_t *n_edges);
/* Ygs of any GFA with S / L / P lines and numeric node ids (the reference's sort_gfa binary) */
int sr_sort_gfa(const char *gfa_in, const sr_sort_params *p, char **gfa_out, uint64_t *n_nodes, uint64_t *n_edges);
/* the SGD positions alone, one per node in ascending id order of gfa_in (n = its number of nodes) */
int sr_sgd_layout(const char *gfa_in, const sr_sort_params *p, double *pos_out, uint64_t n);
/* the resolved parameters and tables of gfa_in: sizes[0..3] = entries of etas (iter_max + 1), zetas, each prefix table
 * (space + 1), number of nodes; arrays may be NULL (call once for the sizes) */
int sr_sgd_tables(const char *gfa_in, const sr_sort_params *p, sr_sort_params *resolved, uint64_t sizes[4], double *etas,
                  double *zetas, double *prefix_theta, double *prefix_cool);
/* timings and counts of the calling thread's last sort: [0] SGD ms (device: hipEvents), [1] groom ms, [2] topological
 * sort ms, [3] GFA writing ms, [4] terms per iteration, [5] iterations, [6] sub-rounds per iteration, [7] nodes,
 * [8] path steps, [9] wall time of the whole sort stage on a host clock (parameters and tables, device buffers and
 * copies, SGD, ordering, groom, topological sort, path verification, GFA writing).  Returns the number of slots written. */
int sr_sort_stats(double *out, uint32_t cap);

/* -------- compaction by per-handle tables ----------------------------------------------
 * compact() + renumber_nodes_sequentially() of any GFA with S / L / P lines and numeric node ids.  All three
 * executions return the same bytes.  In sr_ctx_build_gfa_opts / sr_ctx_build_gfa_sorted, compact == 2 compacts on the
 * context's device, straight from the arrays graph induction left there (0 and 1 as before).
 * stats (or NULL): [0] rounds, [1] rounds run by the host procedure because they held an irregular list (one that
 * meets its own mirror, or a cycle), [2] chains merged, [3] longest list of links, [4] pointer-jumping launches,
 * [5] compaction + renumbering in microseconds (hipEvents on a device, host clock for -1 and -2), [6] upload +
 * download in microseconds (host clock; 0 for -1 and -2), [7] 0. */
#define SR_COMPACT_DEVICE_HOST (-1)          /* sr_compact.cpp's greedy procedure */
#define SR_COMPACT_DEVICE_TABLES_HOST (-2)   /* the table formulation on the host, in index order */
int sr_compact_gfa(const char *gfa_in, int device, char **gfa_out, uint64_t *n_nodes, uint64_t *n_edges, uint64_t stats[8]);
/* stats of the calling thread's last compaction by tables (sr_compact_gfa, or a context build with compact == 2) */
int sr_compact_stats(uint64_t stats[8]);

/* -------- graph statistics (`--stats FILE`) ------------------------------------------------
 * Exact integer statistics of any GFA with S / L / P lines and numeric node ids, as the parser of sr_sort_gfa reads it:
 * nodes are 1..V in ascending id order, identical L lines count once.  The columns of `odgi stats -S`, per-node depth and
 * path count, base pairs and nodes by path count, pairwise shared base pairs of paths (`odgi similarity`), the layout error
 * of src/bin/measure_layout_quality.rs:100-210 per path, self loops, tips and weakly connected components.
 * device >= 0: HIP kernels on that device (sr_stats.hip); SR_STATS_DEVICE_HOST: the same tables in plain loops on the host.
 * Both give the same integers.  More than 4096 paths, 2^30 nodes or 2^31 steps, edges or bases: SR_ERR_UNSUPPORTED.
 * An empty graph gives zeros.  Arrays of the result (index v - 1 for node v, c for c paths, i * paths + j for a pair):
 * the sum of squared errors is kept split as e = a 2^16 + b -> sums of a^2, a b, b^2, and is
 * sq[0] 2^32 + sq[1] 2^17 + sq[2] in 128 bits. */
#define SR_STATS_DEVICE_HOST (-1)
typedef struct {
    uint64_t length, nodes, edges, paths, steps;        /* odgi stats -S */
    uint64_t rev_steps, depth_bp;                       /* steps on the reverse strand; sum of depth * length */
    uint64_t self_loops, tips, components;
    uint32_t *depth, *paths_on;                         /* [nodes] */
    uint64_t *bp_by_paths, *nodes_by_paths;             /* [paths + 1] */
    uint64_t *shared;                                   /* [paths * paths], symmetric */
    uint64_t *path_pairs, *path_abs, *path_len;         /* [paths]: step pairs, sum e, sum of the first node's length */
    uint64_t *path_sq;                                  /* [paths * 3]: the three parts of sum e^2 */
    uint64_t total_pairs, total_abs, total_len, total_sq[3];   /* over every path with at least 2 steps */
    uint64_t stats_us;                                  /* the stage: hipEvents on a device, host clock for the twin */
    uint64_t kernel_us[5];                              /* steps, nodes, similarity, layout, topology */
} sr_graph_stats;
int sr_graph_stats_gfa(const char *gfa_in, int device, sr_graph_stats **out);
void sr_graph_stats_free(sr_graph_stats *s);
/* TSV report of a result (names: one per path, NULL = path indices); the only place where a float is formed, so every
 * front end writes the same bytes.  *text is malloc'ed (sr_free). */
int sr_graph_stats_report(const sr_graph_stats *s, const char *const *names, char **text);
/* tests: the split sum of squares over n values below 2^32 on the host */
int sr_stats_sq_sums_host(const uint64_t *e, uint64_t n, uint64_t out[3]);

/* -------- 2-D layout (`--layout FILE`, `--layout-svg FILE`) -----------------------------------
 * Path-guided SGD in the plane of any GFA with S / L / P lines and numeric node ids, as the parser of sr_sort_gfa reads it
 * (what `odgi layout` + `odgi draw` give, reproducibly): two end points per node, pulled to their distance along the
 * paths.  Deterministic like the Ygs SGD (counter-based draws, Zipf by table, sub-rounds with order-free int64
 * accumulation): the device result is bit-identical to the host twin's.  A layout is defined only up to an isometry of
 * the plane.  More than 2^30 nodes or 2^31 steps: SR_ERR_UNSUPPORTED.  A graph without a path of two steps or more keeps
 * its initial state: x = cumulative node length in id order, y = a seeded value within half a node length of 0.
 * A zero field is derived (the value in brackets); the seed is taken as it is. */
#define SR_LAYOUT_DEVICE_HOST_TWIN (-1)   /* the batched SGD on one host thread (bit-identical to the device) */
#define SR_LAYOUT_DEVICE_SEQUENTIAL (-2)  /* every term applied at once (yardstick for the quality only) */
typedef struct {
    uint64_t seed;              /* counter-based draws: splitmix64(seed, iteration, term, draw); default 9399220 */
    uint64_t iter_max;          /* [30]: iterations 0..iter_max run; at least 2 */
    double theta;               /* [0.99]; cooling iterations use 0.001 */
    double eps;                 /* [0.01] */
    double eta_max;             /* [(longest path in bp)^2] */
    double cooling_start;       /* [0.5]: cooling for iterations > floor(cooling_start * iter_max) */
    uint64_t space;             /* [longest path in bp] */
    uint64_t space_max;         /* [100] */
    uint64_t space_quant;       /* [100] */
    uint64_t min_term_updates;  /* [10 * total path steps]: terms per iteration */
    uint64_t terms_per_round;   /* terms per sub-round [DESIGN.md section 12] */
    int32_t device;             /* >= 0: HIP device, SR_LAYOUT_DEVICE_HOST_TWIN, SR_LAYOUT_DEVICE_SEQUENTIAL */
    int32_t reserved;
} sr_layout_params;
void sr_layout_params_default(sr_layout_params *p);
/* the layout of gfa_in (p NULL = defaults): 4 doubles per node in ascending id order, x0 y0 x1 y1 (end point 0 = the
 * node's start on its forward strand); n_nodes must be its number of nodes */
int sr_layout_gfa(const char *gfa_in, const sr_layout_params *p, double *xy_out, uint64_t n_nodes);
/* the outputs, formed here so that every front end writes the same bytes; *text is malloc'ed (sr_free).
 * TSV (the columns of `odgi layout --tsv`): "idx\tX\tY", rows 2v and 2v + 1 for the v-th node, %.4f.
 * SVG: one <line> per node, one thin <line> per L line from the out-end of its from-handle to the in-end of its
 * to-handle, viewBox = bounding box + 2 %. */
int sr_layout_tsv(const double *xy, uint64_t n, char **text);
int sr_layout_svg(const char *gfa_in, const double *xy, uint64_t n, char **text);
/* quality of a layout on the host in double: out[0] sampled path stress = mean of ((|p_i - p_j| - d) / d)^2 over the pairs
 * that `samples` term draws select (cooling off, a stream of its own from `seed`), out[1] mean | |end1 - end0| - len | over
 * the nodes in bp, out[2] pairs used, out[3] 0 */
int sr_layout_quality(const char *gfa_in, const double *xy, uint64_t n, uint64_t seed, uint64_t samples, double out[4]);
/* the calling thread's last sr_layout_gfa: [0] SGD ms (device: hipEvents), [1] terms per iteration, [2] iterations,
 * [3] sub-rounds per iteration, [4] nodes, [5] path steps, [6] wall time of the stage in ms on a host clock.  Returns the
 * number of slots written. */
int sr_layout_stats(double *out, uint32_t cap);
/* tests: the parameters sr_layout_gfa resolves for gfa_in, and the selection of terms t0 .. t0 + count - 1 of iteration k
 * (cooling: 0 / 1): end points i, j (2 * node index + end; 0xffffffff = skipped draw) and their path distance d */
int sr_layout_resolve(const char *gfa_in, const sr_layout_params *p, sr_layout_params *resolved);
int sr_layout_select_host(const char *gfa_in, const sr_layout_params *p, uint64_t k, uint64_t t0, uint64_t count, int cooling,
                          uint32_t *i_out, uint32_t *j_out, double *d_out);

/* -------- path-by-bin coverage (`--bin FILE`, `--viz FILE.png`) ---------------------------------
 * What `odgi bin` writes and `odgi viz` draws, of any GFA with S / L / P lines and numeric node ids as the parser of
 * sr_sort_gfa reads it: nodes 1..V in ascending id order laid end to end give the pangenome sequence of `length` bp, cut
 * into bins of bin_width bp (the last one may be shorter).  cov[p * bins + b] = base pairs of bin b that the steps of path p
 * cover (a path that revisits a node counts every visit), inv = those of them covered by reverse steps.
 * device >= 0: HIP kernels on that device (sr_bin.hip); SR_BIN_DEVICE_HOST: plain loops on the host.  Both give the same
 * integers.  Limits of the graph as for the statistics (2^30 nodes, 2^31 steps and bases); paths * bins above 2^26:
 * SR_ERR_UNSUPPORTED.  An empty graph gives bins = 0 and empty tables. */
#define SR_BIN_DEVICE_HOST (-1)
typedef struct {
    uint64_t bin_width, bins;   /* exactly one non-zero, else SR_ERR_INVALID; bins = n: bin_width = ceil(length / n) */
} sr_bin_params;
typedef struct {
    uint64_t length, paths, bins, bin_width;            /* bins = ceil(length / bin_width): may be below the count asked for */
    uint64_t *cov, *inv;                                /* [paths * bins] */
    uint64_t bin_us;                                    /* the stage: hipEvents on a device, host clock for the twin */
    uint64_t kernel_us[3];                              /* position scan, steps, download of the tables */
} sr_path_bins;
int sr_path_bins_gfa(const char *gfa_in, const sr_bin_params *p, int device, sr_path_bins **out);
void sr_path_bins_free(sr_path_bins *b);
/* The outputs, formed here so that every front end writes the same bytes; names: one per path, NULL = path indices;
 * *text, *rgb and *png are malloc'ed (sr_free).
 * TSV: a `#` line with bin_width, bins, length and paths, the header "path bin cov_bp inv_bp mean_cov mean_inv", then one row
 * per cell with cov_bp > 0 by path in file order, then by bin (1-based, as in `odgi bin`); mean_cov = cov / length of the
 * bin, mean_inv = inv / cov, both %.6f: the only floats. */
int sr_path_bins_tsv(const sr_path_bins *b, const char *const *names, char **text);
/* Image: `bins` pixels wide, paths * path_height + (paths - 1) * path_gap high, path p a band in file order from the top,
 * gap rows and empty cells white; 3 bytes per pixel, rows from the top.  More than 2^30 bytes: SR_ERR_UNSUPPORTED.
 * path: the path's colour (a hash of its name) blended towards white by min(cov, bin length) / bin length;
 * strand: red where more than half of the covered base pairs are reverse, else black;
 * depth: grey, black at a mean coverage of depth_max.  All in integer arithmetic (sr_bin_rule.h). */
#define SR_VIZ_MODE_PATH 0
#define SR_VIZ_MODE_STRAND 1
#define SR_VIZ_MODE_DEPTH 2
typedef struct {
    int mode;                   /* SR_VIZ_MODE_*; default path */
    uint32_t path_height;       /* 10: rows per path, >= 1 */
    uint32_t path_gap;          /* 1: white rows between paths */
    uint32_t depth_max;         /* 4: depth mode, >= 1 */
} sr_viz_params;
void sr_viz_params_default(sr_viz_params *p);
int sr_path_bins_rgb(const sr_path_bins *b, const char *const *names, const sr_viz_params *p, uint8_t **rgb, uint32_t *width,
                     uint32_t *height);
/* the same image as a PNG: 8-bit RGB, not interlaced, filter 0 on every row, a zlib stream of stored blocks (no
 * compression, no dependency).  An image without a pixel (no path or no bin): SR_ERR_INVALID. */
int sr_path_bins_png(const sr_path_bins *b, const char *const *names, const sr_viz_params *p, uint8_t **png, uint64_t *size);

/* -------- pangenome growth (`--growth FILE`) ------------------------------------------------------
 * How the pangenome and the core grow as genomes are added (`odgi heaps`, `panacus histgrowth`), of any GFA with S / L / P
 * lines and numeric node ids as the parser of sr_sort_gfa reads it.  Every path belongs to one of `groups` groups
 * (group_of[paths]; NULL: every path its own group and n_groups is ignored); a group is present on a node iff a step of
 * one of its paths lies on it.  For permutation r of the groups and k = 1..groups, pan[r * groups + k - 1] = base pairs of the
 * nodes on which at least one of its first k groups is present, core[...] = those on which all of them are.
 * bp_by_groups[c] = base pairs of the nodes on which exactly c groups are present.
 * Permutation r orders the groups by (splitmix64 hash of (seed, r, group), group) ascending (sr_growth_rule.h); if
 * groups <= 8 and groups! <= the permutations asked for, all groups! permutations run instead, in lexicographic order
 * (exhaustive = 1).  perm[r * groups + k - 1] = the group at rank k.
 * device >= 0: HIP kernels on that device (sr_growth.hip); SR_GROWTH_DEVICE_HOST: plain loops on the host.  Both give the
 * same integers.  Limits of the graph as for the statistics; more than 4096 groups, or permutations asked for x groups
 * above 2^24: SR_ERR_UNSUPPORTED.  permutations = 0, a group_of entry >= n_groups or a group without a path:
 * SR_ERR_INVALID.  An empty graph or one without a path gives groups = 0, empty tables and no error. */
#define SR_GROWTH_DEVICE_HOST (-1)
typedef struct {
    uint64_t seed;              /* default 9399220 */
    uint64_t permutations;      /* default 1000 */
} sr_growth_params;
void sr_growth_params_default(sr_growth_params *p);
typedef struct {
    uint64_t length, paths, groups, permutations;       /* permutations actually run (groups! when exhaustive) */
    int32_t exhaustive, variant;                        /* variant: 0 the host loops, 1 the device kernels (lane = node word, wave = permutation) */
    uint64_t *pan, *core;                               /* [permutations * groups], row r = permutation r, column k - 1 */
    uint32_t *perm;                                     /* [permutations * groups], group at rank k */
    uint64_t *bp_by_groups;                             /* [groups + 1] */
    uint64_t growth_us, kernel_us[4];                   /* the stage; presence, histogram, ranks, growth */
    uint64_t seed;                                      /* as given: the report names it */
} sr_growth;
int sr_growth_gfa(const char *gfa_in, const uint32_t *group_of, uint32_t n_groups, const sr_growth_params *p, int device,
                  sr_growth **out);
void sr_growth_free(sr_growth *g);
/* groups from path names: mode 0 = every path its own group; 1 = PanSN sample (text before the first '#'); 2 = PanSN
 * haplotype (text before the second '#'); a name without that many '#' is its own key.  Groups are numbered by first
 * appearance in file order.  group_names (may be NULL) is malloc'ed as one block (sr_free), one string per group. */
int sr_growth_groups(const char *const *path_names, uint64_t n_paths, int mode, uint32_t *group_of, uint32_t *n_groups,
                     char ***group_names);
/* closed-form expectations over all orders of the groups, in double, [groups] each:
 * E pan(k) = sum_c bp[c] (1 - prod_{i<k} (G - c - i) / (G - i)),  E core(k) = sum_c bp[c] prod_{i<k} (c - i) / (G - i) */
int sr_growth_expected(const uint64_t *bp_by_groups, uint32_t groups, double *pan_exp, double *core_exp);
/* Heaps' law: least squares of log new(k) on log k, k = 2..groups, new(k) = pan_exp[k - 1] - pan_exp[k - 2], points with
 * new(k) <= 0 skipped; new ~ kappa k^-alpha.  *points < 2: no fit, alpha = kappa = 0, SR_OK. */
int sr_growth_fit(const double *pan_exp, uint32_t groups, double *alpha, double *kappa, uint32_t *points);
/* The report, the only place its floats are formed; *text is malloc'ed (sr_free).  TSV: three `#` lines (groups, paths,
 * permutations, exhaustive, seed, length; unused = bp_by_groups[0], core = bp_by_groups[groups]; alpha, kappa, points and
 * open iff alpha <= 1, NA without a fit), the header "k pan_exp core_exp pan_mean pan_sd pan_min pan_max core_mean core_sd
 * core_min core_max", one row per k.  Integers as integers, floats %.6f, sd = the population standard deviation over the
 * permutations run, from sums kept in 128-bit integers. */
int sr_growth_report(const sr_growth *g, char **text);

/* -------- variant sites (`--vcf FILE`) -------------------------------------------------------------
 * Where the paths of a graph differ from one of them, the reference R (`vg deconstruct`), of any GFA with S / L / P lines and
 * numeric node ids as the parser of sr_sort_gfa reads it.  refseq = the oriented sequence of R (a reverse handle reads its
 * node reversed and complemented by the project's rule).  A node R visits exactly once is an anchor, with its interval
 * [ref_pos, ref_end) of refseq and its orientation on R; a step of any path on an anchor is an anchor step, of strand
 * orientation xor ref_or.  Two anchor steps i < j of a path with none between them are colinear iff the strands are equal
 * and the intervals follow each other on that strand; then [a, b) is the reference between them and the allele is what the
 * path has between them, read on the reference's strand.  A pair that is not colinear is a break (breaks[path]); a
 * colinear pair with a == b and an empty allele yields nothing; one with b - a or the allele above max_allele_len (0: no
 * limit) is counted in skipped[path]; every other is a traversal.  Traversals with the same (a, b) form a site: allele 0 is
 * refseq[a:b], the other distinct alleles are numbered from 1 by (length, bytes); a site without one is not reported.
 * gt[site * paths + path] = the allele of the path's first traversal of the site, else 0 if a run of reference-adjacent
 * anchor steps of the path covers [a - 1, b + 1), else -1.  The column of R is included.
 * device >= 0: HIP kernels on that device (sr_variants.hip); SR_VARIANTS_DEVICE_HOST: plain loops on the host that compare
 * allele bytes directly.  Both give the same integers and bytes; the device groups alleles by a 64-bit hash ANDed with
 * hash_mask and then compares bytes, and no result depends on hashes not colliding (hash_collision_sites counts the
 * reported sites where they did; always 0 on the host).  Limits of the graph as for the statistics, a reference of < 2^31
 * bases; sites x paths above 2^26: SR_ERR_UNSUPPORTED.  An unknown ref_name or a node without a sequence: SR_ERR_INVALID.  An empty graph, one without
 * a path or a reference without steps gives no site and no error. */
#define SR_VARIANTS_DEVICE_HOST (-1)
typedef struct {
    const char *ref_name;       /* the reference path; NULL (default): the first path */
    uint64_t max_allele_len;    /* default 10000; 0: no limit */
    uint64_t hash_mask;         /* default all ones; fewer bits force collisions (tests) */
    uint64_t reserved;          /* 0 */
} sr_variant_params;
void sr_variant_params_default(sr_variant_params *p);
typedef struct {
    uint64_t ref_path, ref_len, paths, anchors, traversals, sites, hash_collision_sites;
    uint64_t *breaks, *skipped;                         /* [paths] */
    uint64_t *site_start, *site_end;                    /* [sites] a and b, ascending by (a, b) */
    uint32_t *site_alleles;                             /* [sites] ALT alleles of the site (>= 1) */
    uint64_t *allele_off;                               /* [sum of site_alleles + 1] into alleles: the ALT alleles of site 0 in order, then site 1 ... */
    char *alleles;
    int32_t *gt;                                        /* [sites * paths] */
    char *ref_seq;                                      /* [ref_len] refseq */
    int32_t variant, reserved;                          /* variant: 0 the host loops, 1 the device kernels */
    uint64_t variants_us, kernel_us[6];                 /* the stage; anchors, scan, emit, hash, sort and classes, genotypes */
} sr_variants;
int sr_variants_gfa(const char *gfa_in, const sr_variant_params *p, int device, sr_variants **out);
void sr_variants_free(sr_variants *v);
/* The VCF text, the only place its bytes are formed; names = the names of the paths in file order; *text is malloc'ed
 * (sr_free).  VCFv4.2: fileformat, source, contig (ID = the name of R, its length; left out without a path), one
 * ##seqrush_amd=<anchors,traversals,sites,breaks,skipped> line (breaks and skipped summed over the paths), INFO AC and AN,
 * FORMAT GT, and every path except R in file order as a haploid sample.  One record per site: POS = a + 1 and REF =
 * refseq[a:b] if b > a and no ALT allele is empty, else padded with the base before the site (POS = a, REF =
 * refseq[a-1:b], every ALT with refseq[a-1] in front).  ID, QUAL, FILTER are `.`; AC counts the samples per ALT allele, AN
 * those whose GT is not `.`. */
int sr_variants_vcf(const sr_variants *v, const char *const *names, char **text);

/* -------- extending a graph (`--extend FILE.gfa`) -------------------------------------------------
 * Adds sequences to an existing GFA without realigning the pairs it was built from.  A component of this library's
 * union-find is a set of bases and a node offset of an induced graph is exactly one component, so a GFA whose paths spell
 * their sequences IS the partition that produced it: uniting, per node offset, all bases that visit it restores the
 * partition, and only the pairs that touch a new sequence are left to align.  Any GFA with S / L / P lines and numeric
 * node ids, as the parser of sr_sort_gfa reads it, can be extended, whoever built it.
 * Old sequences = the oriented sequences of the P lines in file order, named by their paths (a reverse handle reads its
 * node reversed and complemented by the project's rule).  Merged set = the old sequences, then the records of new_seqs
 * (NULL or n = 0: none).  SR_ERR_INVALID, naming the offender: a name that occurs twice (path / path or path / record), a
 * path without steps, a step on a missing node, a visited node without a sequence (`*`), a GFA without a P line.  A node
 * no path visits is ignored, and so are the L lines: induction re-derives the edges.
 * Seed: with all steps of all paths back to back, every base a step spells is united with the base that the node's first
 * step (smallest index) spells at the same node offset (csrc/sr_extend_rule.h).  -k does not apply to it.
 * With -x none and fixed -k, -S, -d, extending the graph of the first m sequences by the other n - m gives the labels and
 * the GFA bytes of building all n at once; in general, those of sr_ctx_load_pairs over the merged set with the old pair
 * list followed by the new one.  The equality needs paths that spell their sequences (known limit).
 * device >= 0: the old sequences are spelled by HIP kernels on that device (sr_extend.hip); SR_EXTEND_DEVICE_HOST: plain
 * loops.  Both give the same bytes.  The plan owns the merged sr_seqset (sr_extend_plan_seqs: valid until the plan is
 * freed) and the step / offset / node-length tables of the seed.  Every limit of a normal load applies to the merged set;
 * 2^30 nodes, 2^31 steps or 2^39 old bases: SR_ERR_UNSUPPORTED. */
#define SR_EXTEND_DEVICE_HOST (-1)
typedef struct sr_extend_plan sr_extend_plan;
typedef struct {
    uint64_t old_paths, old_bases, old_steps, new_sequences;
    uint64_t pairs_before, pairs_after;         /* the enumeration over the merged set; what the filter kept (before sharding) */
    uint64_t unions_attempted, unions_joined;   /* of the last seed: bases not spelled by their node's first step; set joins */
    uint64_t spell_us, seed_us;                 /* hipEvents (spell_us on the host twin: a host clock) */
} sr_extend_stats;
int sr_extend_plan_gfa(const char *gfa_in, const sr_seqset *new_seqs, int device, sr_extend_plan **out);
void sr_extend_plan_free(sr_extend_plan *plan);
const sr_seqset *sr_extend_plan_seqs(const sr_extend_plan *plan);
uint32_t sr_extend_plan_n_old(const sr_extend_plan *plan);
/* the pair filter (pure host code): drops every (q, t) with q < n_old and t < n_old, keeps the order of the rest; an index
 * outside the merged set is SR_ERR_INVALID.  Both arrays sr_free. */
int sr_extend_pair_list(const sr_extend_plan *plan, const uint32_t *q, const uint32_t *t, uint64_t count, uint32_t **q_out,
                        uint32_t **t_out, uint64_t *count_out);
/* sr_ctx_load of the plan's merged set with the filter applied to what the enumeration (or the tree: selection on the
 * device) gives under p, then the seed tables are uploaded and the seed is enqueued on the context's stream (no run).  The
 * plan may be freed afterwards; build the GFA with sr_extend_plan_seqs or an equal sr_seqset.  On such a context
 * sr_ctx_reset_uf means init + seed; every other context behaves as before.  A plan without new sequences is
 * SR_ERR_INVALID: there is nothing to align. */
int sr_ctx_load_extend(sr_ctx *c, const sr_extend_plan *plan, const sr_params *p);
/* the host twin of the seed (no device) on a node array of n >= 2 * total length of the merged set + 2 entries in the
 * SeqRush::new state (sr_uf_init_host), through sr_uf_unite_host; stats (or NULL): [0] unions attempted, [1] joined */
int sr_extend_seed_host(const sr_extend_plan *plan, uint64_t *nodes, uint64_t n, uint64_t stats[2]);
/* the plan's counts alone (pairs, unions and seed_us 0) */
int sr_extend_plan_stats(const sr_extend_plan *plan, sr_extend_stats *out);
/* the same with the pair counts of the load and the counters and time of the last seed; syncs the context's stream */
int sr_ctx_extend_stats(sr_ctx *c, sr_extend_stats *out);

/* -------- lifting intervals (`--lift IN.bed --lift-out FILE`) -------------------------------------
 * Where an interval of one path lies in the other paths (`odgi position`, a liftover), of any GFA with S / L / P lines and
 * numeric node ids as the parser of sr_sort_gfa reads it.  pstart[s] = the offset of step s in the oriented sequence of
 * its own path, plen[p] = the length of path p.
 * Queries: the lines of bed_text, `name start end [label [rest...]]`, 0-based and half-open; fields are separated by tabs
 * or, on a line without a tab, by runs of blanks; a trailing CR is dropped.  A line that is blank or starts with `#`,
 * `track` or `browser` is ignored.  Fewer than three fields, or a start or end that is not a decimal number below 2^64:
 * SR_ERR_INVALID, naming the line.  A name that is no path (the first path of that name counts): skipped, counted in
 * `unknown`.  start >= end or end > plen: skipped, counted in `out_of_range`.  Every other line is a query; label defaults to
 * `name:start-end`; queries keep file order and may repeat.
 * first[B][v] = the smallest step index of path B on node v.  A step s of the query path A on handle (v, r) whose interval
 * [pstart[s], pstart[s] + len[v]) overlaps the query in the handle offsets [o0, o1) contributes to target B, if B visits
 * v, with t = first[B][v] on handle (v, r'): the strand r xor r', the image [pstart[t] + o0, pstart[t] + o1) when the
 * strands agree and [pstart[t] + len - o1, pstart[t] + len - o0) when not, and bp = o1 - o0.  The lift of (query, B):
 * tstart = the smallest image start, tend = the largest image end, covered = the sum of bp, rev_bp = the sum of bp on the
 * reverse strand; strand `-` iff 2 * rev_bp > covered.  covered = 0: unmapped, and all four are 0.  This is a hull over
 * first visits: a target that visits the nodes in another order or a node more than once widens it, so covered stands
 * beside tend - tstart for the user to filter on.  Nothing is chained.
 * Targets: every path in file order, or the one named to_name (unknown: SR_ERR_INVALID, whatever the graph holds).  The
 * tables are dense, [queries x targets], and include the query's own path (which lifts to itself when it visits no node
 * twice).  queries x targets above 2^26 or targets x nodes above 2^28: SR_ERR_UNSUPPORTED.  Limits of the graph as for the
 * statistics.  An empty graph, one without a path, or a BED without a query gives empty tables and no error.
 * device >= 0: HIP kernels on that device (sr_lift.hip); SR_LIFT_DEVICE_HOST: plain loops on the host.  Both give the same
 * integers and bytes.  short_steps: a query that touches at most this many steps is lifted by one lane per (query, target),
 * a longer one by one wave per (query, target); 0 and UINT64_MAX send every query one way (tests), and no result depends
 * on it. */
#define SR_LIFT_DEVICE_HOST (-1)
typedef struct {
    const char *to_name;        /* the one target path; NULL (default): every path */
    uint64_t min_covered;       /* default 1: sr_lift_bed leaves out pairs with covered below this */
    uint64_t short_steps;       /* default 8 */
    uint64_t reserved;          /* 0 */
} sr_lift_params;
void sr_lift_params_default(sr_lift_params *p);
typedef struct {
    uint64_t queries, targets, paths, unknown, out_of_range, mapped;      /* mapped: pairs of the tables with covered > 0 */
    uint32_t *q_path;                                   /* [queries] */
    uint64_t *q_start, *q_end;                          /* [queries] */
    uint64_t *label_off;                                /* [queries + 1] into labels */
    char *labels;
    uint32_t *target_path;                              /* [targets] */
    uint64_t *tstart, *tend, *covered, *rev_bp;         /* [queries * targets] */
    int32_t variant, to_named;                          /* variant: 0 the host loops, 1 the device kernels; to_named: to_name was given */
    uint64_t min_covered;                               /* as given: the writer filters by it */
    uint64_t short_pairs, long_pairs;                   /* pairs through the lane-per-pair and the wave-per-pair kernel (host: 0, 0) */
    uint64_t lift_us, kernel_us[5];                     /* the stage; positions, first visits, locate, short pairs, long pairs */
} sr_lift;
int sr_lift_gfa(const char *gfa_in, const char *bed_text, const sr_lift_params *p, int device, sr_lift **out);
void sr_lift_free(sr_lift *l);
/* The BED text, the only place its bytes are formed; names = the names of the paths in file order; *text is malloc'ed
 * (sr_free).  One tab-separated line per kept pair in (query, target) order:
 * `tname tstart tend label covered strand qname qstart qend rev_bp`.  Left out: unmapped pairs, pairs with covered <
 * min_covered, and pairs whose target is the query's own path unless to_name chose it. */
int sr_lift_bed(const sr_lift *l, const char *const *names, char **text);

/* -------- extracting a subgraph (`--extract-region R --extract-out FILE`) ---------------------------
 * The graph of a locus alone, with every path's allele through it (`odgi extract`), of any GFA with S / L / P lines and
 * numeric node ids as the parser of sr_sort_gfa reads it.  pstart and plen as for the lift; the E edges are the distinct L
 * lines in file order.  A node without a sequence: SR_ERR_INVALID.  Limits of the graph as for the statistics.
 * Regions: the lines of bed_text (may be NULL), read by the rules of the lift (the label is ignored; unknown names and
 * ranges outside their path are skipped and counted), and the n_regions strings `NAME` or `NAME:START-END`.  A string that
 * equals a path name (the first path of that name) is the whole path [0, plen); else it is split at its last `:` and the
 * rest at its first `-`, both decimal numbers below 2^64.  A string is explicit, so a missing `:`, a bad number, an
 * unknown path, start >= end and end > plen are SR_ERR_INVALID, naming the string; only the whole of a path of length 0 is
 * counted in out_of_range instead.  Regions may overlap, nest and repeat in any order; more than 2^24: SR_ERR_UNSUPPORTED.
 * level[v], all ones = not kept:  (1) seeds, level 0: some step s on v of a region's path has [pstart[s], pstart[s] +
 * len[v]) meet [start, end).  (2) context, context_steps = c <= 65535 (else SR_ERR_UNSUPPORTED): for r = 1..c a node
 * without a level gets level r if an L line joins it, by either end in any orientation, to a node of level r - 1; a
 * self-loop gives nothing, and a GFA without L lines has no context.  (3) merge, merge_distance = D bases and merge_rounds
 * = R <= 64 (else SR_ERR_UNSUPPORTED): in round k = 1..R, within one path, every maximal run of steps on nodes without a
 * level that has a kept step directly before and directly after it and whose lengths sum to <= D gets level c + k on all
 * its nodes; every run of a round is judged against the set at the start of the round, and a round that adds nothing
 * ends the merge.  merge_rounds_run = the rounds that added a node.
 * Result: kept nodes in their order, the new id = the rank from 1; every L line between two kept nodes, in file order
 * with its orientation; per path in file order every maximal run of steps on kept nodes as a subpath named
 * `NAME:start-end` (start = pstart of its first step, end = pstart + len of its last; always written).  Nothing kept: empty
 * tables, the text `H\tVN:Z:1.0\n` and no error.
 * device >= 0: HIP kernels on that device (sr_extract.hip); SR_EXTRACT_DEVICE_HOST: plain loops on the host.  Both give
 * the same integers and bytes. */
#define SR_EXTRACT_DEVICE_HOST (-1)
typedef struct {
    uint64_t context_steps;     /* default 0 */
    uint64_t merge_distance;    /* default 100000: a decision of the rule, not a measurement */
    uint64_t merge_rounds;      /* default 3: likewise */
    uint64_t reserved;          /* 0 */
} sr_extract_params;
void sr_extract_params_default(sr_extract_params *p);
typedef struct {
    uint64_t regions, unknown, out_of_range;               /* regions: those that count */
    uint64_t in_nodes, in_edges, in_steps, in_paths;
    uint64_t nodes, edges, subpaths, steps, bases;         /* of the result */
    uint64_t seeds, by_context, by_merge, merge_rounds_run;
    uint32_t *level;                                       /* [in_nodes], all ones: not kept */
    uint32_t *node_old;                                    /* [nodes]: the input id (1-based rank of the S line) of result node k + 1 */
    uint32_t *edge_from, *edge_to;                         /* [edges]: result handles, id << 1 | reverse */
    uint32_t *sub_path;                                    /* [subpaths]: the input path */
    uint64_t *sub_start, *sub_end, *sub_off;               /* [subpaths]; sub_off [subpaths + 1] into sub_steps */
    uint32_t *sub_steps;                                   /* [steps]: result handles */
    int32_t variant;                                       /* 0 the host loops, 1 the device kernels */
    uint64_t extract_us, kernel_us[6];                     /* the stage; positions, seeds, context, merge, numbering, emission */
    void *priv;                                            /* node sequences and path names for the writer */
} sr_extract;
int sr_extract_gfa(const char *gfa_in, const char *bed_text, const char *const *regions, uint64_t n_regions,
                   const sr_extract_params *p, int device, sr_extract **out);
/* The GFA text of the result, the only place its bytes are formed (those of the GFA writer: H, S, L with 0M, P with *);
 * *gfa is malloc'ed (sr_free). */
int sr_extract_text(const sr_extract *x, char **gfa);
void sr_extract_free(sr_extract *x);

void sr_free(void *p);

const char *sr_last_error(void);
int sr_abi_version(void);
int sr_device_count(void);

#ifdef __cplusplus
}
#endif
#endif
