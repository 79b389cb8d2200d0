// sr_ctx.h -- what the units of the host runtime share (DESIGN.md "Host runtime"): the context, split into what lives as
// long as it does and the state of one load; one of each small helper; the few functions that cross units.
// Host side only, included by no .hip file; not part of the public interface.
#pragma once
#include <hip/hip_runtime_api.h>
#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/seqrush_amd.h"
#include "sr_internal.h"
#include "sr_sort.h"
#include "sr_iter_rule.h"
#include "sr_inv_rule.h"
#include "sr_extend.h"

// ------------------------------------------------------------------ helpers
// sr_fail (sr_params.cpp, declared in sr_sort.h) sets sr_last_error() and returns the code
#define HIPCHK(expr)                                                                     \
    do {                                                                                 \
        hipError_t _e = (expr);                                                          \
        if (_e != hipSuccess)                                                            \
            return sr_fail(SR_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

// what sr_last_error() says now is what it says again at the end of the scope (a clean-up in between may fail and say more)
struct SrKeepError {
    std::string msg = sr_last_error();
    ~SrKeepError() { sr_fail(0, msg); }
};

// device memory of one call, freed when the call returns.  nullptr: the allocation (up: or the copy) failed
struct SrScratch {
    std::vector<void *> v;
    ~SrScratch() { for (void *q : v) (void)hipFree(q); }
    void *alloc(size_t bytes) {
        void *q = nullptr;
        if (hipMalloc(&q, bytes ? bytes : 16) != hipSuccess) return nullptr;
        v.push_back(q);
        return q;
    }
    void *up(const void *src, size_t bytes) {
        void *q = alloc(bytes);
        if (q && hipMemcpy(q, src, bytes, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
        return q;
    }
};

// an entry point that is given a device ordinal: there is a device, the ordinal names one, and it is the current one
static inline int sr_pick_device(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return sr_fail(SR_ERR_NO_DEVICE, "no HIP device available (seqrush_amd has no CPU fallback)");
    if (device < 0 || device >= n) return sr_fail(SR_ERR_INVALID, "device ordinal out of range");
    HIPCHK(hipSetDevice(device));
    return SR_OK;
}

// a host vector as memory the caller of the C interface owns (sr_free)
template <class T>
static int to_malloc(const std::vector<T> &v, T **out) {
    *out = (T *)malloc((v.empty() ? 1 : v.size()) * sizeof(T));
    if (!*out) return sr_fail(SR_ERR_NOMEM, "out of memory");
    if (!v.empty()) memcpy(*out, v.data(), v.size() * sizeof(T));
    return SR_OK;
}

static inline uint8_t comp_base(uint8_t b) {      // Sequence::reverse_complement seqrush.rs:281-295
    switch (b) {
    case 'A': case 'a': return 'T'; case 'T': case 't': return 'A';
    case 'C': case 'c': return 'G'; case 'G': case 'g': return 'C';
    default: return b;
    }
}

static inline uint64_t splitmix64(uint64_t x) {
    x += 0x9e3779b97f4a7c15ULL;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ULL;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebULL;
    return x ^ (x >> 31);
}

// ------------------------------------------------------------------ context
// A tied secondary is deferred to the tail launch only in batches of at most this many rounds of alignments per workgroup:
// beyond, the solo alignment at the end is a few per cent of the launch at most (SR_TAIL_ROUNDS)
#define SR_TAIL_ROUNDS_DEFAULT 8

// What describes one load.  free_dev() resets it as one value, so a field added here cannot outlive its load; every field
// carries its default.  iter_al and inv_al own their alignments: free_dev() frees them before the reset.
struct SrLoadState {
    sr_params prm{};
    uint32_t n = 0;
    std::vector<uint32_t> len;
    std::vector<uint64_t> goff;
    uint64_t total_len = 0, uf_size = 0;
    std::vector<uint32_t> pair_q, pair_t;          // this rank's pairs, in enumeration order
    std::vector<uint64_t> cigar_base;              // [np + 1] prefix sums of the per-pair CIGAR reserve (ops)
    std::vector<uint32_t> batch_first;             // [nbatch + 1]: pair ranges that share the CIGAR arena one after the other
    uint64_t total_pairs_all_ranks = 0;            // size of the (sparsified) list before sharding
    uint64_t dp_cells = 0;
    int off16 = 1, nwg = 0, nthreads = 256, symbits = 2;
    size_t lds_bytes = 0;
    SrAlignArgs aa{};
    SrUniteArgs ua{};
    unsigned long long *d_nodes = nullptr, *d_minarr = nullptr, *d_labels = nullptr;
    unsigned long long *d_counters = nullptr;
    int *d_error = nullptr;
    uint32_t *d_queue = nullptr, *d_oqueue = nullptr, *d_order = nullptr;
    uint64_t *d_okeys = nullptr, *d_okeys2 = nullptr;   // cost-ordered dequeue after the orientation kernel (sr_order.hip)
    uint32_t *d_ovals = nullptr; void *d_otemp = nullptr; size_t otemp_bytes = 0;
    uint64_t *d_cbase = nullptr;                   // [np + nbatch]: batch b starts at batch_first[b] + b, values relative to its arena
    uint8_t *d_bases = nullptr;                    // raw bytes of all sequences (sketching, graph induction)
    int onwg = 0;                      // workgroups (= waves) of the orientation kernel, 0 = orientation inside the alignment kernel
    size_t olds_bytes = 0;
    int32_t *d_max_score = nullptr;
    uint32_t *d_mirror = nullptr;                  // [np] SrAlignArgs::mirror (blocked kernel, 2-bit symbols), nullptr = none
    uint64_t mirror_partners = 0;                  // primaries of the rank's list
    // tail launch of the blocked kernel: shape (0 = none), its workgroups per CU, SR_TAIL=all, the rounds rule
    int tail_threads = 0, tail_wg_per_cu = 1, tail_rounds = SR_TAIL_ROUNDS_DEFAULT, tail_cus = 0;
    bool tail_all = false;
    std::vector<uint32_t> batch_partners;          // [nbatch] primaries per batch
    uint32_t *d_tail_list = nullptr, *d_tail_deferred = nullptr;
    unsigned long long *d_timeline = nullptr;      // instrumented instance: [nwg][4] (sr_ctx_tail_timeline)
    // rotating tile priority (sr_prio_rule.h): arrival counts per CU (reset before every main launch of the blocked kernel), the
    // instrumented instance's second record [nwg][4] (sr_ctx_prio_timeline)
    int prio_rounds = SR_TAIL_ROUNDS_DEFAULT;      // a batch rotates only when its alignments are at most this many times its workgroups
    uint32_t *d_cu_arrivals = nullptr;
    unsigned long long *d_prio_timeline = nullptr;
    int ev_used[5] = {0, 0, 0, 0, 0};              // event pairs of sr_ctx::ev this load's passes have recorded, per kind
    bool loaded = false;
    bool fuse_unite = false;           // sr_ctx_run: the blocked alignment kernel unites each pair after its CIGAR (no unite kernel)
    bool from_paf = false;             // loaded by sr_ctx_load_paf: no alignment stage, no sr_alignments
    bool aligned_batch_valid = false;  // the arena holds the CIGARs of the last batch sr_ctx_align ran
    std::string workspace_report;      // sizing of the last load (sr_ctx_workspace_report)
    // iterative mode (sr_ctx_load_iterative): pairs [0, iter_tree_pairs) are the expanded tree entries, batches
    // [0, iter_tree_batches) cover them; every later batch is a phase-2 window of whole chunks (4 * CHECK_INTERVAL pairs)
    bool iter_loaded = false, iter_keep = false, iter_ran = false;
    uint64_t iter_tree_pairs = 0;
    uint32_t iter_tree_batches = 0, iter_max_chunks = 0;
    sr_iter_stats iter_stats{};
    std::vector<uint64_t> iter_counts;                 // per-check component counts of the last run
    SrIterState *d_iter_state = nullptr;
    unsigned long long *d_iter_counts = nullptr;       // [iter_max_chunks] counts of the window's checks, [iter_max_chunks] spare slot
    sr_alignments *iter_al = nullptr;                  // processed alignments of the last run (keep_alignments)
    // inversion patching (sr_ctx_enable_inversions): the scan's buffers, the jobs and results of the last run
    bool inv_on = false, inv_keep = false;
    uint64_t inv_m = 0;                                // resolved threshold
    uint32_t *d_inv_count = nullptr, *d_inv_off = nullptr;      // [largest batch], [largest batch + 1]
    unsigned long long *d_inv_stats = nullptr;         // [4]
    SrInvJob *d_inv_jobs = nullptr;
    uint64_t inv_job_cap = 0;
    std::vector<SrInvJob> inv_raw;                     // job records of the run so far, pair order then CIGAR order
    std::vector<sr_inv_job> inv_jobs;
    sr_inv_stats inv_stats{};
    sr_alignments *inv_al = nullptr;
    // joined mode (--inversion-join): J, its 24-byte records and sr_ctx_inversion_join_stats
    uint32_t inv_join = 0;
    SrInvJobJ *d_inv_jobs_j = nullptr;
    uint64_t inv_job_cap_j = 0;
    std::vector<SrInvJobJ> inv_raw_j;
    uint64_t inv_join_stats[4] = {0, 0, 0, 0};
    std::chrono::steady_clock::time_point t_first_kernel{};    // host clock just before a load's first kernel (inv_patch_pass)
    int inv_ev_used = 0;                               // event pairs of sr_ctx::inv_ev the run has recorded
    // --extend (sr_ctx_load_extend): the seed's tables on the device, its counters; sr_ctx_reset_uf re-seeds
    bool ext_loaded = false;
    SrExtendSeedArgs ext{};
    sr_extend_stats ext_stats{};
};

// What lives as long as the context: the device, the stream, the allocations of the load (free_dev() frees them) and the
// event pools, which later loads reuse.
struct sr_ctx : SrLoadState {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::vector<void *> dev_allocs;
    // kernel timing: [kind] -> one event pair per batch (kinds: 0 align, 1 unite, 4 orientation) or a single pair (2, 3)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[5];
    std::vector<std::pair<hipEvent_t, hipEvent_t>> inv_ev;      // one event pair per scanned batch
    hipEvent_t ext_ev[2] = {nullptr, nullptr};                  // around the seed of --extend
};

// ------------------------------------------------------------------ what crosses units (none of it leaves the library)
#pragma GCC visibility push(hidden)
// sr_params.cpp
const char *knob(const char *name);
std::string knobs_json();
int32_t max_score_for_divergence(const sr_params &p, uint64_t seq_len, double d);
int make_pen(const sr_params &p, bool ori, SrPen *out);
// sr_pairs.cpp
void enumerate_pairs(uint32_t n, const sr_params &p, const uint8_t *sel, std::vector<uint32_t> &pq, std::vector<uint32_t> &pt);
typedef std::vector<uint32_t> SrU32s;
void iterative_lists(uint32_t n, const uint8_t *sel, uint64_t seed, double rf, SrU32s &ti, SrU32s &tj, SrU32s &ri, SrU32s &rj);
void shard_pairs(const std::vector<uint32_t> &len, uint32_t rank, uint32_t count, std::vector<uint32_t> &pq, std::vector<uint32_t> &pt);
uint64_t mirror_map(const uint32_t *q, const uint32_t *t, const uint32_t *batch_first, uint32_t nbatch, uint32_t workgroups, uint32_t *out);
// sr_host.cpp: the context, a load, a pass
int dev_alloc(sr_ctx *c, void **p, size_t bytes);
void free_dev(sr_ctx *c);
int unload_if_failed(sr_ctx *c, int r);
int ev_get(sr_ctx *c, int kind, int idx, hipEvent_t **a, hipEvent_t **b);
int load_impl(sr_ctx *c, const sr_seqset *seqs, const sr_params *p, const uint32_t *eq, const uint32_t *et, uint64_t ecount,
              bool explicit_pairs, bool iterative = false, bool forced_strand = false, uint32_t ext_n_old = 0);
void batch_args(const sr_ctx *c, uint32_t b, SrAlignArgs *a, SrUniteArgs *u);
int enqueue_align_batch(sr_ctx *c, uint32_t b, bool fuse_unite = false);
int enqueue_unite_batch(sr_ctx *c, uint32_t b, bool fused = false);
int begin_pass(sr_ctx *c, bool reset_counters);
int run_to_parent(sr_ctx *c, const sr_params *p, uint64_t *parent_out);
// sr_host.cpp: results.  AlnAcc: host copy of the alignments of the batches collected so far
struct AlnAcc { std::vector<uint32_t> cnt, ops; std::vector<int32_t> score; std::vector<uint8_t> isrev; };
int collect_batch(sr_ctx *c, uint32_t b, AlnAcc &acc);
sr_alignments *make_alignments_of(const std::vector<uint32_t> &pair_q, const std::vector<uint32_t> &pair_t,
                                  const std::vector<uint32_t> &len, const AlnAcc &acc, size_t count = SIZE_MAX);
// sr_host.cpp: the stages of `tree:` selection;  tap: copies of the intermediates for the tests
struct TreeTap { std::vector<unsigned long long> *sketch = nullptr; std::vector<uint32_t> *sketch_n = nullptr, *shared = nullptr, *denom = nullptr; };
int tree_stages(hipStream_t stream, uint32_t n, const uint32_t *len, const uint8_t *d_bases, const uint64_t *d_goff,
                const uint32_t *d_len, uint32_t kmer, const uint32_t *h_shared, const uint32_t *h_denom,
                uint32_t k_nearest, uint32_t k_farthest, std::vector<uint8_t> *sel, const TreeTap *tap);
// sr_inv_host.cpp: the three steps of inversion patching inside a run
int inv_begin_run(sr_ctx *c);
int inv_scan_batch(sr_ctx *c, uint32_t b);
int inv_patch_pass(sr_ctx *c);
#pragma GCC visibility pop

// ------------------------------------------------------------------ helpers over a context
// a host vector into a new buffer of the load, copied on the context's stream: the vector lives until the next synchronise
template <class T>
static int dev_upload(sr_ctx *c, const std::vector<T> &v, T **out) {
    void *d = nullptr;
    const int r = dev_alloc(c, &d, v.size() * sizeof(T));
    if (r) return r;
    HIPCHK(hipMemcpyAsync(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, c->stream));
    *out = (T *)d;
    return SR_OK;
}

// a buffer of a loaded context, read once everything on its stream is done
static inline int ctx_read(sr_ctx *c, void *dst, const void *src, size_t bytes) {
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return SR_OK;
}

// a context of one call on `device`: destroyed whatever `use` returns, and what `use` said stays the last error
template <class F>
static int sr_with_ctx(int device, F use) {
    sr_ctx *c = nullptr;
    int r = sr_ctx_create(device, &c);
    if (r) return r;
    r = use(c);
    SrKeepError keep;
    sr_ctx_destroy(c);
    return r;
}
