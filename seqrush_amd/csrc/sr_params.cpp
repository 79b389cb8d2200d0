// sr_params.cpp -- what the host runtime is told before it touches a device: the error slot behind sr_last_error(), the
// table of environment knobs, and sr_params -- its defaults, the three parsers of the command line's grammars and what
// follows from the penalties alone (the device penalties, the score bound of a divergence).  Nothing here needs a context.
#include <cmath>
#include "sr_ctx.h"

static thread_local std::string g_err;
int sr_fail(int code, const std::string &msg) { g_err = msg; return code; }      // every unit, the stages and sr_sort.cpp
extern "C" const char *sr_last_error(void) { return g_err.c_str(); }

// ------------------------------------------------------------------ environment knobs
// Every environment variable the load path reads, in ONE table: name, what unset means, what it does.  knob() is the only
// place that calls getenv for them and refuses a name that is not listed; sr_ctx_workspace_report() dumps every knob that is
// set ("knobs": {...}), so a measurement carries every non-default setting it ran with.
struct SrKnob { const char *name, *unset, *doc; };
static const SrKnob SR_KNOBS[] = {
    {"SR_ALIGN_IMPL", "2 when the penalties have a blocked instance", "1 = level-per-pass kernel (sr_align_bfs_kernel), 2 = score-blocked kernel"},
    {"SR_BLK_LEVELS", "10 for x=5, o1+e1=10", "5 = generic 5-level blocked instance instead of the exact 10-level one"},
    {"SR_ALIGN_THREADS", "by pairs per CU", "threads per workgroup: 64 | 128 | 256 | 512 | 1024"},
    {"SR_WG_PER_CU", "4", "workgroups per CU the launch is sized for"},
    {"SR_NWG", "CUs x workgroups per CU", "cap on workgroups (several pairs per workgroup on small inputs)"},
    {"SR_RING_U16", "1 below 57 k", "0 = 32-bit searches keep 32-bit ring rows"},
    {"SR_LAZY_ID", "1", "0 = searches store their I/D rows from the first level (no recompute pass)"},
    {"SR_HIST_JOBS", "4", "worst-case base cases the per-workgroup history holds (1..16)"},
    {"SR_BFS_BASE_JOBS", "16 (lean builds 4 / 8)", "base cases per batch"},
    {"SR_CIGAR_ARENA_OPS", "25 % of free memory", "CIGAR arena in ops (tests: force batches)"},
    {"SR_POISON_ROWS", "off", "fill the row workspaces with this offset before the run (stale-row tests)"},
    {"SR_PREORIENT", "by pairs per CU and LDS", "1 / 0 = orientation as its own kernel / inside the alignment kernel"},
    {"SR_NO_REORDER", "off", "keep list order instead of the cost-sorted dequeue order"},
    {"SR_ORIENT_LEVELS", "off", "orientation level by level even for the default penalties"},
    {"SR_NO_KBITS", "off", "no q-gram bound in the orientation kernel"},
    {"SR_NO_MIRROR", "off", "1 = no pair has a mirror partner: (q, t) and (t, q) are both aligned (A/B runs, tests)"},
    {"SR_MIRROR_REPLAY", "on", "0 = a tied secondary is aligned in full: its primary keeps no breakpoint records and none is matched (A/B runs, tests)"},
    {"SR_NO_FUSED_UNITE", "off", "sr_ctx_run launches sr_unite_kernel per batch instead of uniting inside the blocked alignment kernel"},
    {"SR_PROFILE_TICKS", "0", "1 = launch the instrumented instance (100 MHz tick counters, per-workgroup timeline)"},
    {"SR_TAIL", "on", "0 = no tail launch: a tied secondary is always aligned by its primary's workgroup (A/B runs); all = every such secondary is deferred to the tail launch (tests)"},
    {"SR_TAIL_THREADS", "widest instance wider than the main launch", "threads per workgroup of the tail launch among the existing instances: 256 | 512 | 1024 (tests)"},
    {"SR_TILE_PRIO", "1", "0 = no rotating tile priority among the workgroups of a CU: all tile code at priority 0, no clock read (A/B runs, tests)"},
    {"SR_TAIL_ROUNDS", "8", "a batch defers only when its alignments are at most this many times the launch's workgroups"},
    {"SR_FORCE_INT32", "off", "tests: 32-bit offsets (and the 16-bit ring of 32-bit searches) whatever the sequence length"},
    {"SR_TEST_BASE_LEVELS", "off", "tests: cap on the levels a base case is given at first (forces the re-queue path)"},
    {"SR_BOUNDS_DETAIL", "off", "1 = (bounds-checked build) keep the first offending access in counters[40..43]"},
};
const char *knob(const char *name) {
    for (const SrKnob &k : SR_KNOBS)
        if (!strcmp(k.name, name)) return getenv(name);
    fprintf(stderr, "seqrush_amd: internal error: environment knob %s is not in SR_KNOBS\n", name);
    abort();
}
std::string knobs_json() {
    std::string out = "{";
    for (const SrKnob &k : SR_KNOBS)
        if (const char *v = getenv(k.name)) {
            if (out.size() > 1) out += ", ";
            out += std::string("\"") + k.name + "\": \"";
            for (const char *q = v; *q; q++) if (*q != '"' && *q != '\\' && (unsigned char)*q >= 32) out += *q;
            out += "\"";
        }
    return out + "}";
}
// (name, unset, doc) lines of the table: `seqrush_mi355x --knobs`, scripts
extern "C" const char *sr_knobs_doc(void) {
    static std::string doc;
    if (doc.empty())
        for (const SrKnob &k : SR_KNOBS) doc += std::string(k.name) + "\t" + k.unset + "\t" + k.doc + "\n";
    return doc.c_str();
}
extern "C" int sr_abi_version(void) { return SR_ABI_VERSION; }
extern "C" void sr_free(void *p) { free(p); }
extern "C" int sr_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ------------------------------------------------------------------ params
extern "C" void sr_default_params(sr_params *p) {
    memset(p, 0, sizeof(*p));
    p->match_score = 0; p->mismatch_penalty = 5; p->gap_open1 = 8; p->gap_ext1 = 2;
    p->gap_open2 = 24; p->gap_ext2 = 1;                         // seqrush.rs:45
    p->ori_match = 0; p->ori_mismatch = 1; p->ori_gap_open = 1; p->ori_gap_ext = 1;  // :49
    p->min_match_len = 0; p->max_divergence = -1.0; p->exclude_self = 0;
    p->memory_mode = SR_MEM_ULTRALOW; p->sparsify_kind = SR_SPARSE_NONE; p->sparsify_factor = 1.0;
    p->sparsify_seed = 42; p->canonical_labels = 0; p->device = 0;
    p->shard_rank = 0; p->shard_count = 1;
    p->tree_k_nearest = 0; p->tree_k_farthest = 0; p->tree_rand_frac = 0.0; p->tree_kmer = 16;
}

static bool parse_i32(const std::string &s, int32_t *out) {     // Rust str::parse::<i32>
    if (s.empty() || s.size() > 15) return false;
    size_t i = (s[0] == '+' || s[0] == '-') ? 1 : 0;
    if (i == s.size()) return false;
    for (size_t j = i; j < s.size(); j++) if (s[j] < '0' || s[j] > '9') return false;
    long long v = atoll(s.c_str());
    if (v > INT32_MAX || v < INT32_MIN) return false;
    *out = (int32_t)v;
    return true;
}
static std::vector<std::string> split(const std::string &s, char c) {
    std::vector<std::string> out;
    size_t st = 0;
    for (;;) {
        size_t p = s.find(c, st);
        if (p == std::string::npos) { out.push_back(s.substr(st)); break; }
        out.push_back(s.substr(st, p - st));
        st = p + 1;
    }
    return out;
}

extern "C" int sr_parse_scores(const char *s, sr_params *p) {   // seqrush.rs:165-217
    auto parts = split(s, ',');
    if (parts.size() < 4)
        return sr_fail(SR_ERR_INVALID, "Scores must have at least 4 values: match,mismatch,gap1_open,gap1_extend");
    if (parts.size() > 6) return sr_fail(SR_ERR_INVALID, "Too many score values provided (max 6)");
    int32_t v[6] = {0, 0, 0, 0, -1, -1};
    static const char *nm[6] = {"match score", "mismatch penalty", "gap1_open penalty",
                                "gap1_extend penalty", "gap2_open penalty", "gap2_extend penalty"};
    for (int i = 0; i < 4; i++)
        if (!parse_i32(parts[i], &v[i])) return sr_fail(SR_ERR_INVALID, std::string("Invalid ") + nm[i] + ": " + parts[i]);
    if (parts.size() >= 6)
        for (int i = 4; i < 6; i++)
            if (!parse_i32(parts[i], &v[i])) return sr_fail(SR_ERR_INVALID, std::string("Invalid ") + nm[i] + ": " + parts[i]);
    p->match_score = v[0]; p->mismatch_penalty = v[1]; p->gap_open1 = v[2]; p->gap_ext1 = v[3];
    p->gap_open2 = v[4]; p->gap_ext2 = v[5];
    return SR_OK;
}

extern "C" int sr_parse_orientation_scores(const char *s, sr_params *p) {   // :219-250
    auto parts = split(s, ',');
    if (parts.size() != 4)
        return sr_fail(SR_ERR_INVALID, "Orientation scores must have exactly 4 values: match,mismatch,gap_open,gap_extend");
    int32_t v[4];
    for (int i = 0; i < 4; i++)
        if (!parse_i32(parts[i], &v[i])) return sr_fail(SR_ERR_INVALID, "Invalid orientation score: " + parts[i]);
    p->ori_match = v[0]; p->ori_mismatch = v[1]; p->ori_gap_open = v[2]; p->ori_gap_ext = v[3];
    return SR_OK;
}

static bool parse_f64(const std::string &s, double *out) {
    if (s.empty() || isspace((unsigned char)s[0])) return false;
    for (char ch : s) if (ch == 'x' || ch == 'X') return false;     // strtod takes hex floats, Rust's f64::from_str does not
    char *end;
    double v = strtod(s.c_str(), &end);
    if (*end != 0) return false;
    *out = v;
    return true;
}

extern "C" int sr_parse_sparsification(const char *cs, sr_params *p) {      // :356-431
    std::string s(cs);
    if (s == "none" || s == "1.0") { p->sparsify_kind = SR_SPARSE_NONE; return SR_OK; }
    if (s == "auto") { p->sparsify_kind = SR_SPARSE_AUTO; return SR_OK; }
    double f;
    if (s.rfind("random:", 0) == 0) {
        if (!parse_f64(s.substr(7), &f)) return sr_fail(SR_ERR_INVALID, "Invalid random factor: " + s);
        if (f > 0.0 && f <= 1.0) { p->sparsify_kind = SR_SPARSE_RANDOM; p->sparsify_factor = f; return SR_OK; }
        return sr_fail(SR_ERR_INVALID, "Random factor must be in (0.0, 1.0]");
    }
    if (s.rfind("connectivity:", 0) == 0) {
        if (!parse_f64(s.substr(13), &f)) return sr_fail(SR_ERR_INVALID, "Invalid connectivity probability: " + s);
        if (f > 0.0 && f <= 1.0) { p->sparsify_kind = SR_SPARSE_CONNECTIVITY; p->sparsify_factor = f; return SR_OK; }
        return sr_fail(SR_ERR_INVALID, "Connectivity probability must be in (0.0, 1.0]");
    }
    if (s.rfind("tree:", 0) == 0) {                              // tree:neighbor[,stranger[,random[,k-mer]]] (:378-418)
        auto parts = split(s.substr(5), ',');
        if (parts.empty() || parts.size() > 4)
            return sr_fail(SR_ERR_INVALID, "Tree sampling requires 1-4 values: tree:neighbor[,stranger[,random[,k-mer]]], got " + s);
        auto parse_usize = [](const std::string &t, uint64_t *v) {      // Rust str::parse::<usize>
            size_t i = (!t.empty() && t[0] == '+') ? 1 : 0;
            if (i >= t.size()) return false;
            *v = 0;
            for (; i < t.size(); i++) {
                if (t[i] < '0' || t[i] > '9') return false;
                const uint64_t dgt = (uint64_t)(t[i] - '0');
                if (*v > (0xffffffffffffffffULL - dgt) / 10) return false;      // overflow of a 64-bit usize: Err like Rust
                *v = *v * 10 + dgt;
            }
            return true;
        };
        uint64_t kn = 0, kf = 0, km = 16;
        double rf = 0.0;
        if (!parse_usize(parts[0], &kn)) return sr_fail(SR_ERR_INVALID, "Invalid neighbor count: " + parts[0]);
        if (parts.size() >= 2 && !parse_usize(parts[1], &kf)) return sr_fail(SR_ERR_INVALID, "Invalid stranger count: " + parts[1]);
        if (parts.size() >= 3) {
            if (!parse_f64(parts[2], &rf)) return sr_fail(SR_ERR_INVALID, "Invalid random fraction: " + parts[2]);
            if (rf < 0.0 || rf > 1.0) return sr_fail(SR_ERR_INVALID, "Random fraction must be in [0.0, 1.0], got " + parts[2]);
        }
        if (parts.size() >= 4) {
            if (!parse_usize(parts[3], &km)) return sr_fail(SR_ERR_INVALID, "Invalid k-mer size: " + parts[3]);
            if (km == 0) return sr_fail(SR_ERR_INVALID, "K-mer size must be > 0");
        }
        p->sparsify_kind = SR_SPARSE_TREE;
        p->tree_k_nearest = (uint32_t)std::min<uint64_t>(kn, 0xffffffffULL);
        p->tree_k_farthest = (uint32_t)std::min<uint64_t>(kf, 0xffffffffULL);
        p->tree_rand_frac = rf; p->tree_kmer = (uint32_t)std::min<uint64_t>(km, 0xffffffffULL);
        return SR_OK;
    }
    if (parse_f64(s, &f) && f > 0.0 && f <= 1.0) { p->sparsify_kind = SR_SPARSE_RANDOM; p->sparsify_factor = f; return SR_OK; }
    return sr_fail(SR_ERR_INVALID, "Invalid sparsification: '" + s + "'");
}

// max_score_for_divergence seqrush.rs:253-269
int32_t max_score_for_divergence(const sr_params &p, uint64_t seq_len, double d) {
    int32_t max_mismatches = (int32_t)std::ceil((double)seq_len * d);
    int32_t max_gaps = (int32_t)std::ceil((double)seq_len * d * 0.5);
    int32_t mismatch_score = max_mismatches * p.mismatch_penalty;
    int32_t gap_score = max_gaps > 0 ? p.gap_open1 + (max_gaps - 1) * p.gap_ext1 : 0;
    return std::max(mismatch_score + gap_score, p.mismatch_penalty * 2);
}

int make_pen(const sr_params &p, bool ori, SrPen *out) {
    if (ori) {
        if (p.ori_match != 0) return sr_fail(SR_ERR_UNSUPPORTED, "orientation match score must be 0");
        out->x = p.ori_mismatch; out->o1 = p.ori_gap_open; out->e1 = p.ori_gap_ext;
        out->o2 = 0; out->e2 = 0; out->two = 0;
    } else {
        if (p.match_score != 0)
            return sr_fail(SR_ERR_UNSUPPORTED, "match score must be 0 (WFA2 penalties, seqrush.rs:45); the Aligner-trait defaults "
                                            "2,4,4,2,24,1 (src/aligner/allwave_impl.rs:15-23) need allwave's score conversion, "
                                            "which is not in the reference tree -- see INTEGRATION.md section 8");
        out->x = p.mismatch_penalty; out->o1 = p.gap_open1; out->e1 = p.gap_ext1;
        out->two = p.gap_open2 >= 0;
        out->o2 = out->two ? p.gap_open2 : 0; out->e2 = out->two ? p.gap_ext2 : 0;
        if (out->two && out->e2 <= 0) return sr_fail(SR_ERR_INVALID, "gap2_extend must be > 0");
    }
    if (out->x <= 0 || out->o1 < 0 || out->e1 <= 0) return sr_fail(SR_ERR_INVALID, "penalties must satisfy x>0, o>=0, e>0");
    out->scope = std::max(out->x, out->o1 + out->e1);
    if (out->two) out->scope = std::max(out->scope, out->o2 + out->e2);
    out->scope += 1;
    if (out->scope > SR_MAX_SCOPE) return sr_fail(SR_ERR_UNSUPPORTED, "penalties too large for the device ring (scope > 127)");
    return SR_OK;
}
