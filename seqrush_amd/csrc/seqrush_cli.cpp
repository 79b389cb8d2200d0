// seqrush_cli.cpp -- C++ host side above the C ABI: the reference's CLI surface for the hot path
// (src/main.rs:4-7, Args src/seqrush.rs:17-152, run_seqrush :1839-1853, load_sequences :1801-1837).
// Everything that computes goes through include/seqrush_amd.h; output is the --no-sort graph or, with --sort, the Ygs
// layout (sr_ctx_build_gfa_sorted), compacted unless --no-compact.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
#include "../../include/seqrush_amd.h"

struct Seq { std::string id; std::string data; };

static bool is_ws(unsigned char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == 0x0b || c == 0x0c; }

// load_sequences, src/seqrush.rs:1801-1837
static bool load_sequences(const std::string &path, std::vector<Seq> &out) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    std::string line, cur_id, cur;
    while (std::getline(f, line)) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (!line.empty() && line[0] == '>') {
            if (!cur_id.empty()) { out.push_back({cur_id, cur}); cur.clear(); }   // data kept when the id was empty (:1812-1820)
            size_t a = 1;
            while (a < line.size() && is_ws((unsigned char)line[a])) a++;
            size_t b = a;
            while (b < line.size() && !is_ws((unsigned char)line[b])) b++;
            cur_id = line.substr(a, b - a);
        } else {
            size_t a = 0, b = line.size();
            while (a < b && is_ws((unsigned char)line[a])) a++;
            while (b > a && is_ws((unsigned char)line[b - 1])) b--;
            cur.append(line, a, b - a);
        }
    }
    if (!cur_id.empty()) out.push_back({cur_id, cur});
    return true;
}

// label part file of a shard run: header + uf_size canonical labels (u64).  The header lets the merge run refuse parts of
// another input, another shard count, a duplicated part or an incomplete set.
struct PartHeader { char magic[8]; uint64_t uf_size, shard_rank, shard_count, input_hash, flags; };
static const char PART_MAGIC[8] = {'S', 'R', 'L', 'A', 'B', 'E', 'L', '1'};
static uint64_t fnv1a(const void *data, size_t n, uint64_t h = 0xcbf29ce484222325ULL) {
    const unsigned char *b = (const unsigned char *)data;
    for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 0x100000001b3ULL; }
    return h;
}

// an f64 the way Rust's Display prints it (the reference's messages): shortest round-trip digits, positional, "50" for 50.0
static std::string rust_f64(double x) {
    if (std::isnan(x)) return "NaN";
    if (std::isinf(x)) return x < 0 ? "-inf" : "inf";
    char buf[64];
    for (int prec = 1; prec <= 17; prec++) {
        snprintf(buf, sizeof(buf), "%.*e", prec - 1, x);
        if (strtod(buf, nullptr) == x) break;
    }
    std::string s(buf);
    const bool neg = s[0] == '-';
    if (neg) s = s.substr(1);
    const size_t e = s.find('e');
    const int point = atoi(s.c_str() + e + 1) + 1;           // digits before the decimal point
    std::string digits, out;
    for (size_t i = 0; i < e; i++) if (s[i] != '.') digits += s[i];
    if (point <= 0) out = "0." + std::string((size_t)-point, '0') + digits;
    else if ((size_t)point >= digits.size()) out = digits + std::string((size_t)point - digits.size(), '0');
    else out = digits.substr(0, (size_t)point) + "." + digits.substr((size_t)point);
    if (out.find('.') != std::string::npos) { while (out.back() == '0') out.pop_back(); if (out.back() == '.') out.pop_back(); }
    return (neg ? "-" : "") + out;
}

static void usage() {
    fprintf(stderr, "usage: seqrush_mi355x -s in.fa [-o output.gfa] [-k 0] [-S 0,5,8,2,24,1] [--orientation-scores 0,1,1,1]\n"
                    "       [-d max_divergence] [-x none|auto|random:F|connectivity:P|tree:kn[,kf[,rf[,k]]]] [-p in.paf] [--output-alignments out.paf] --no-sort|--sort [--no-compact] [--compact-on host|device] [--device N]\n"
                    "       [--sort-seed N] [--sgd-iter-max N] [--skip-sgd] [--skip-groom] [--skip-topo] [--iterative] [-v]\n"
                    "       [--patch-inversions [--inversion-min-size N] [--inversion-join N]] [--stats report.tsv]\n"
                    "       [--layout graph.lay.tsv] [--layout-svg graph.svg] [--layout-seed N] [--layout-iter-max N]\n"
                    "       [--bin bins.tsv [--bin-width W | --bin-count N]] [--viz graph.png [--viz-width N] [--viz-path-height H]\n"
                    "       [--viz-path-gap G] [--viz-mode path|strand|depth] [--viz-depth-max D]]\n"
                    "       [--growth growth.tsv [--growth-permutations N] [--growth-seed N] [--growth-group-by path|sample|haplotype]]\n"
                    "       [--vcf graph.vcf [--vcf-ref NAME] [--vcf-max-allele-len N]] [--extend graph.gfa]\n"
                    "       [--lift in.bed --lift-out lifted.bed [--lift-to NAME] [--lift-min-covered N]]\n"
                    "       [--extract-region REGION ... | --extract-bed in.bed] --extract-out sub.gfa [--extract-context-steps N]\n"
                    "       [--extract-merge-distance N] [--extract-merge-rounds N]\n"
                    "       [--shard R/N --labels-out part.bin]  |  [--labels-in part0.bin --labels-in part1.bin ...]\n");
}

int main(int argc, char **argv) {
    std::string sequences, output = "output.gfa", scores = "0,5,8,2,24,1", ori = "0,1,1,1", sparsify = "none", paf_out, paf_in,
                aligner = "allwave", extend_in, stats_out, layout_out, layout_svg_out, bin_out, viz_out, bin_opt, viz_opt, growth_out, growth_opt, vcf_out, vcf_opt, vcf_ref,
                lift_in, lift_out, lift_opt, lift_to;
    sr_lift_params lfp;
    sr_lift_params_default(&lfp);
    std::vector<std::string> extract_regions;
    std::string extract_bed, extract_out, extract_opt;
    sr_extract_params exp_;
    sr_extract_params_default(&exp_);
    sr_variant_params vcp;
    sr_variant_params_default(&vcp);
    sr_growth_params gp;
    sr_growth_params_default(&gp);
    int growth_mode = 0;
    unsigned long long bin_width = 0, bin_count = 0, viz_width = 1500;
    sr_viz_params vp;
    sr_viz_params_default(&vp);
    long long k = 0;
    double max_div = -1.0;
    int device = 0;
    bool compact_dev = false;
    bool no_sort = false, no_compact = false, sort = false, iterative = false, verbose = false, patch_inv = false;
    unsigned long long inv_min = 0, inv_join = 0;
    bool inv_join_given = false;
    sr_sort_params sp;
    sr_sort_params_default(&sp);
    sr_layout_params lp;
    sr_layout_params_default(&lp);
    // multi-GPU without a collective library in this host: every process aligns one shard (--shard R/N) and writes its
    // canonical labels (--labels-out); a last run merges the files (--labels-in, repeatable) and writes the graph.
    // (With RCCL at hand the exchange is one all-gather: python -m seqrush_amd --gpus N, bench.py.)
    unsigned shard_rank = 0, shard_count = 1;
    std::string labels_out;
    std::vector<std::string> labels_in;
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        auto val = [&](const char *name) -> const char * {
            if (i + 1 >= argc) { fprintf(stderr, "error: %s needs a value\n", name); exit(2); }
            return argv[++i];
        };
        if (a == "-s" || a == "--sequences") sequences = val("-s");
        else if (a == "-o" || a == "--output") output = val("-o");
        else if (a == "-k" || a == "--min-match-length") k = atoll(val("-k"));
        else if (a == "-t" || a == "--threads") (void)val("-t");               // host threads: unused by the device path
        else if (a == "-S" || a == "--scores") scores = val("-S");
        else if (a == "--orientation-scores") ori = val("--orientation-scores");
        else if (a == "-d" || a == "--max-divergence") max_div = atof(val("-d"));
        else if (a == "-x" || a == "--sparsify") sparsify = val("-x");
        else if (a == "-p" || a == "--paf") paf_in = val("-p");
        else if (a == "--output-alignments") paf_out = val("--output-alignments");
        else if (a == "--aligner") aligner = val("--aligner");
        else if (a == "--no-sort") no_sort = true;
        else if (a == "--no-compact") no_compact = true;
        else if (a == "--compact-on") {
            const std::string w = val("--compact-on");
            if (w != "host" && w != "device") { fprintf(stderr, "Error: --compact-on takes host or device\n"); return 1; }
            compact_dev = w == "device";
        }
        else if (a == "--sort") sort = true;
        else if (a == "--sort-seed") sp.seed = strtoull(val("--sort-seed"), nullptr, 10);
        else if (a == "--sgd-iter-max") sp.iter_max = strtoull(val("--sgd-iter-max"), nullptr, 10);
        else if (a == "--skip-sgd") sp.skip_sgd = 1;
        else if (a == "--skip-groom") sp.skip_groom = 1;
        else if (a == "--skip-topo") sp.skip_topo = 1;
        else if (a == "--device") device = atoi(val("--device"));
        else if (a == "--shard") { if (sscanf(val("--shard"), "%u/%u", &shard_rank, &shard_count) != 2 || shard_count == 0 || shard_rank >= shard_count) { fprintf(stderr, "error: --shard R/N\n"); return 2; } }
        else if (a == "--labels-out") labels_out = val("--labels-out");
        else if (a == "--labels-in") labels_in.push_back(val("--labels-in"));
        else if (a == "-v" || a == "--verbose") verbose = true;
        else if (a == "--iterative") iterative = true;
        else if (a == "--stats") stats_out = val("--stats");
        else if (a == "--layout") layout_out = val("--layout");
        else if (a == "--layout-svg") layout_svg_out = val("--layout-svg");
        else if (a == "--layout-seed") lp.seed = strtoull(val("--layout-seed"), nullptr, 10);
        else if (a == "--layout-iter-max") lp.iter_max = strtoull(val("--layout-iter-max"), nullptr, 10);
        else if (a == "--bin") bin_out = val("--bin");
        else if (a == "--viz") viz_out = val("--viz");
        else if (a == "--bin-width" || a == "--bin-count" || a == "--viz-width" || a == "--viz-path-height" || a == "--viz-path-gap" ||
                 a == "--viz-depth-max") {
            const char *v = val(a.c_str());
            char *end = nullptr;
            const unsigned long long n = strtoull(v, &end, 10);
            (a.compare(0, 5, "--bin") == 0 ? bin_opt : viz_opt) = a;
            const bool zero_ok = a == "--viz-path-gap";
            if (*v < '0' || *v > '9' || *end != 0 || (n == 0 && !zero_ok) || (a.compare(0, 5, "--viz") == 0 && n > 0xffffffffULL)) {
                fprintf(stderr, "Error: %s needs a %s integer, got '%s'\n", a.c_str(), zero_ok ? "non-negative" : "positive", v);
                return 1;
            }
            if (a == "--bin-width") bin_width = n;
            else if (a == "--bin-count") bin_count = n;
            else if (a == "--viz-width") viz_width = n;
            else if (a == "--viz-path-height") vp.path_height = (uint32_t)n;
            else if (a == "--viz-path-gap") vp.path_gap = (uint32_t)n;
            else vp.depth_max = (uint32_t)n;
        }
        else if (a == "--viz-mode") {
            const std::string m = val("--viz-mode");
            viz_opt = a;
            if (m != "path" && m != "strand" && m != "depth") { fprintf(stderr, "Error: --viz-mode takes path, strand or depth\n"); return 1; }
            vp.mode = m == "path" ? SR_VIZ_MODE_PATH : m == "strand" ? SR_VIZ_MODE_STRAND : SR_VIZ_MODE_DEPTH;
        }
        else if (a == "--growth") growth_out = val("--growth");
        else if (a == "--growth-permutations" || a == "--growth-seed") {
            const char *v = val(a.c_str());
            char *end = nullptr;
            const unsigned long long n = strtoull(v, &end, 10);
            growth_opt = a;
            const bool zero_ok = a == "--growth-seed";
            if (*v < '0' || *v > '9' || *end != 0 || (n == 0 && !zero_ok)) {
                fprintf(stderr, "Error: %s needs a %s integer, got '%s'\n", a.c_str(), zero_ok ? "non-negative" : "positive", v);
                return 1;
            }
            (zero_ok ? gp.seed : gp.permutations) = n;
        }
        else if (a == "--growth-group-by") {
            const std::string m = val("--growth-group-by");
            growth_opt = a;
            if (m != "path" && m != "sample" && m != "haplotype") { fprintf(stderr, "Error: --growth-group-by takes path, sample or haplotype\n"); return 1; }
            growth_mode = m == "path" ? 0 : m == "sample" ? 1 : 2;
        }
        else if (a == "--vcf") vcf_out = val("--vcf");
        else if (a == "--vcf-ref") { vcf_ref = val("--vcf-ref"); vcf_opt = a; }
        else if (a == "--vcf-max-allele-len") {
            const char *v = val("--vcf-max-allele-len");
            char *end = nullptr;
            const unsigned long long n = strtoull(v, &end, 10);
            vcf_opt = a;
            if (*v < '0' || *v > '9' || *end != 0) { fprintf(stderr, "Error: %s needs a non-negative integer, got '%s'\n", a.c_str(), v); return 1; }
            vcp.max_allele_len = n;
        }
        else if (a == "--extract-region") extract_regions.push_back(val("--extract-region"));
        else if (a == "--extract-bed") extract_bed = val("--extract-bed");
        else if (a == "--extract-out") extract_out = val("--extract-out");
        else if (a == "--extract-context-steps" || a == "--extract-merge-distance" || a == "--extract-merge-rounds") {
            const char *v = val(a.c_str());
            char *end = nullptr;
            const unsigned long long n = strtoull(v, &end, 10);
            extract_opt = a;
            if (*v < '0' || *v > '9' || *end != 0) { fprintf(stderr, "Error: %s needs a non-negative integer, got '%s'\n", a.c_str(), v); return 1; }
            (a == "--extract-context-steps" ? exp_.context_steps : a == "--extract-merge-distance" ? exp_.merge_distance : exp_.merge_rounds) = n;
        }
        else if (a == "--lift") lift_in = val("--lift");
        else if (a == "--lift-out") { lift_out = val("--lift-out"); lift_opt = a; }
        else if (a == "--lift-to") { lift_to = val("--lift-to"); lift_opt = a; }
        else if (a == "--lift-min-covered") {
            const char *v = val("--lift-min-covered");
            char *end = nullptr;
            const unsigned long long n = strtoull(v, &end, 10);
            lift_opt = a;
            if (*v < '0' || *v > '9' || *end != 0) { fprintf(stderr, "Error: %s needs a non-negative integer, got '%s'\n", a.c_str(), v); return 1; }
            lfp.min_covered = n;
        }
        else if (a == "--extend") extend_in = val("--extend");
        else if (a == "--patch-inversions") patch_inv = true;
        else if (a == "--inversion-min-size") {
            const char *v = val("--inversion-min-size");
            char *end = nullptr;
            inv_min = strtoull(v, &end, 10);
            if (*v < '0' || *v > '9' || *end != 0) { fprintf(stderr, "Error: --inversion-min-size needs a non-negative integer, got '%s'\n", v); return 1; }
        }
        else if (a == "--inversion-join") {
            const char *v = val("--inversion-join");
            char *end = nullptr;
            inv_join = strtoull(v, &end, 10);
            if (*v < '0' || *v > '9' || *end != 0 || inv_join > 0xffffffffULL) { fprintf(stderr, "Error: --inversion-join needs a non-negative integer, got '%s'\n", v); return 1; }
            inv_join_given = inv_join != 0;
        }
        else { usage(); return 2; }
    }
    if (sequences.empty()) { usage(); return 2; }
    // the stop rule of --iterative is global and sequential: no shards, no merge of shard labels, no PAF replay
    if (iterative && (!paf_in.empty() || shard_count > 1 || !labels_out.empty() || !labels_in.empty())) {
        fprintf(stderr, "Error: --iterative cannot be combined with %s\n",
                !paf_in.empty() ? "-p" : !labels_in.empty() ? "--labels-in" : "--shard / --labels-out");
        return 1;
    }
    // --patch-inversions scans the alignments this run makes: nothing to scan with -p, --iterative or a merge run
    if (patch_inv && (iterative || !paf_in.empty() || !labels_in.empty())) {
        fprintf(stderr, "Error: --patch-inversions cannot be combined with %s\n", iterative ? "--iterative" : !paf_in.empty() ? "-p" : "--labels-in");
        return 1;
    }
    if (patch_inv && (inv_min ? inv_min : 2ULL * (unsigned long long)(k > 0 ? k : 0)) == 0) {
        fprintf(stderr, "Error: --patch-inversions needs -k or --inversion-min-size (a threshold of 0 would call every complementary SNP an inversion)\n");
        return 1;
    }
    if (inv_join_given && !patch_inv) {
        fprintf(stderr, "Error: --inversion-join is an option of --patch-inversions: give both\n");
        return 1;
    }
    if (inv_join_given && inv_join > (inv_min ? inv_min : 2ULL * (unsigned long long)(k > 0 ? k : 0))) {
        fprintf(stderr, "Error: --inversion-join %llu is above the gap threshold of --patch-inversions (%llu): an island would be a candidate by itself\n",
                inv_join, inv_min ? inv_min : 2ULL * (unsigned long long)(k > 0 ? k : 0));
        return 1;
    }
    // --extend: each of these would compose in principle, none is verified (one process, one GPU: the --gpus N of this front
    // end is --shard / --labels-out / --labels-in)
    if (!extend_in.empty() && (iterative || !paf_in.empty() || patch_inv || shard_count > 1 || !labels_out.empty() || !labels_in.empty())) {
        fprintf(stderr, "Error: --extend cannot be combined with %s\n",
                iterative ? "--iterative" : !paf_in.empty() ? "-p" : patch_inv ? "--patch-inversions" : "--gpus N > 1");
        return 1;
    }
    if (shard_count > 1 && labels_out.empty()) {
        fprintf(stderr, "Error: --shard %u/%u aligns a part of the pair list only: give --labels-out and merge the parts with --labels-in "
                        "(a graph of one shard would be silently incomplete)\n", shard_rank, shard_count);
        return 1;
    }
    if (!labels_in.empty() && (shard_count > 1 || !labels_out.empty())) { fprintf(stderr, "Error: --labels-in is the merge run: no --shard / --labels-out\n"); return 1; }
    if (aligner != "allwave" && aligner != "AllWave") { fprintf(stderr, "Error: aligner '%s' is out of scope; only 'allwave'\n", aligner.c_str()); return 1; }
    if ((!bin_opt.empty() && bin_out.empty()) || (!viz_opt.empty() && viz_out.empty())) {
        const bool b = !bin_opt.empty() && bin_out.empty();
        fprintf(stderr, "Error: %s is an option of %s: give both\n", (b ? bin_opt : viz_opt).c_str(), b ? "--bin" : "--viz");
        return 1;
    }
    if (!growth_opt.empty() && growth_out.empty()) { fprintf(stderr, "Error: %s is an option of --growth: give both\n", growth_opt.c_str()); return 1; }
    if (!vcf_opt.empty() && vcf_out.empty()) { fprintf(stderr, "Error: %s is an option of --vcf: give both\n", vcf_opt.c_str()); return 1; }
    if (!lift_in.empty() && lift_out.empty()) { fprintf(stderr, "Error: --lift needs --lift-out FILE: the lifted intervals have nowhere to go\n"); return 1; }
    if (!lift_opt.empty() && lift_in.empty()) { fprintf(stderr, "Error: %s is an option of --lift: give both\n", lift_opt.c_str()); return 1; }
    const bool extract_asked = !extract_regions.empty() || !extract_bed.empty();
    if (extract_asked && extract_out.empty()) { fprintf(stderr, "Error: --extract-region / --extract-bed need --extract-out FILE: the extracted graph has nowhere to go\n"); return 1; }
    if (!extract_out.empty() && !extract_asked) { fprintf(stderr, "Error: --extract-out needs --extract-region REGION or --extract-bed FILE: there is nothing to extract\n"); return 1; }
    if (!extract_opt.empty() && !extract_asked) { fprintf(stderr, "Error: %s is an option of --extract-region / --extract-bed: give both\n", extract_opt.c_str()); return 1; }
    if (bin_width && bin_count) { fprintf(stderr, "Error: --bin-width and --bin-count exclude each other\n"); return 1; }
    if (sort && no_sort) { fprintf(stderr, "Error: --sort and --no-sort exclude each other\n"); return 1; }
    if (compact_dev && no_compact) { fprintf(stderr, "Error: --compact-on device and --no-compact exclude each other\n"); return 1; }
    if (!no_sort && !sort) { fprintf(stderr, "Error: only --no-sort output is implemented by default; pass --sort for the Ygs layout; compaction runs unless --no-compact\n"); return 1; }
    std::vector<Seq> seqs;
    if (!load_sequences(sequences, seqs)) { fprintf(stderr, "Error: cannot read %s\n", sequences.c_str()); return 1; }
    printf("Loaded %zu sequences\n", seqs.size());
    std::string bases;
    std::vector<uint64_t> offsets(1, 0);
    std::vector<const char *> names;
    for (auto &s : seqs) { bases += s.data; offsets.push_back(bases.size()); names.push_back(s.id.c_str()); }
    sr_seqset set{(uint32_t)seqs.size(), (const uint8_t *)bases.data(), offsets.data(), names.data()};
    // --extend: the paths of the graph are spelled back into sequences (on the device) and -s holds only the new ones; from
    // here on `set` is the merged set, which the plan owns
    sr_extend_plan *plan = nullptr;
    size_t n_seqs = seqs.size(), n_bases = bases.size();
    if (!extend_in.empty()) {
        std::ifstream gf(extend_in, std::ios::binary);
        if (!gf) { fprintf(stderr, "Error: cannot read %s\n", extend_in.c_str()); return 1; }
        std::stringstream ss;
        ss << gf.rdbuf();
        if (sr_extend_plan_gfa(ss.str().c_str(), &set, device, &plan)) { fprintf(stderr, "Error: %s\n", sr_last_error()); return 1; }
        set = *sr_extend_plan_seqs(plan);
        printf("Extending %s: %u paths\n", extend_in.c_str(), sr_extend_plan_n_old(plan));
        n_seqs = set.n; n_bases = (size_t)set.offsets[set.n];
    }
    sr_params p;
    sr_default_params(&p);
    if (sr_parse_scores(scores.c_str(), &p) || sr_parse_orientation_scores(ori.c_str(), &p) ||
        sr_parse_sparsification(sparsify.c_str(), &p)) {
        fprintf(stderr, "Error: %s\n", sr_last_error());
        return 1;
    }
    p.min_match_len = (uint64_t)k; p.max_divergence = max_div; p.device = device; p.canonical_labels = 1;
    p.shard_rank = shard_rank; p.shard_count = shard_count;
    // what a part file must agree on: the sequences (bytes and boundaries) and everything that decides pairs and unions
    uint64_t input_hash = fnv1a(bases.data(), bases.size());      // (shard runs only: never with --extend)
    input_hash = fnv1a(offsets.data(), offsets.size() * 8, input_hash);
    {
        const std::string cfg = scores + "|" + ori + "|" + sparsify + "|" + std::to_string(k) + "|" + std::to_string(max_div);
        input_hash = fnv1a(cfg.data(), cfg.size(), input_hash);
    }
    printf("Building graph with %zu sequences (total length: %zu)\n", n_seqs, n_bases);
    if (!iterative) printf("Total sequence pairs: %zu (sparsification: %s)\n", n_seqs * n_seqs, sparsify.c_str());
    // one resident context: load (or PAF replay) -> align -> unite -> graph induction, all on the device
    sr_ctx *ctx = nullptr;
    auto die = [&]() { fprintf(stderr, "Error: %s\n", sr_last_error()); if (ctx) sr_ctx_destroy(ctx); sr_extend_plan_free(plan); return 1; };
    if (sr_ctx_create(device, &ctx)) return die();
    if (!labels_in.empty()) {                                // merge run: no pairs of its own, the forests come from files
        if (sr_ctx_load_pairs(ctx, &set, &p, nullptr, nullptr, 0)) return die();
        const uint64_t ufn = sr_ctx_uf_size(ctx);
        std::vector<uint64_t> lab(ufn);
        std::vector<char> seen;
        uint64_t parts_of = 0;
        for (const std::string &path : labels_in) {
            FILE *f = fopen(path.c_str(), "rb");
            PartHeader h;
            auto bad = [&](const char *why) { fprintf(stderr, "Error: label part %s: %s\n", path.c_str(), why); if (f) fclose(f); sr_ctx_destroy(ctx); return 1; };
            if (!f || fread(&h, sizeof(h), 1, f) != 1 || memcmp(h.magic, PART_MAGIC, 8) != 0) return bad("not a label part file (no header)");
            if (h.uf_size != ufn || h.input_hash != input_hash) return bad("written for other sequences or other options (-S / --orientation-scores / -x / -k / -d)");
            if (h.shard_count == 0 || h.shard_rank >= h.shard_count) return bad("bad shard in header");
            if (parts_of == 0) { parts_of = h.shard_count; seen.assign(parts_of, 0); }
            if (h.shard_count != parts_of) return bad("belongs to a run with another shard count");
            if (seen[h.shard_rank]) return bad("shard given twice");
            seen[h.shard_rank] = 1;
            if (fread(lab.data(), 8, ufn, f) != ufn || fgetc(f) != EOF) return bad("truncated or oversized");
            fclose(f); f = nullptr;
            if (sr_ctx_merge_labels_host(ctx, lab.data(), 1)) return die();
        }
        for (uint64_t r = 0; r < parts_of; r++)
            if (!seen[r]) { fprintf(stderr, "Error: shard %llu/%llu is missing from the --labels-in set\n", (unsigned long long)r, (unsigned long long)parts_of); sr_ctx_destroy(ctx); return 1; }
    } else if (!paf_in.empty()) {                            // align_and_unite_from_paf (src/seqrush.rs:510-609)
        printf("Reading alignments from PAF file: %s\n", paf_in.c_str());
        if (sr_ctx_load_paf(ctx, &set, &p, paf_in.c_str())) return die();
    } else if (iterative) {                                  // align_and_unite_iterative (src/seqrush.rs:867-1132)
        printf("Using iterative alignment with stabilization detection\n");
        if (p.sparsify_kind != SR_SPARSE_TREE)
            fprintf(stderr, "Note: Iterative mode works best with tree sampling. Using default tree:3,3,0.1,16\n");
        if (sr_ctx_load_iterative(ctx, &set, &p, paf_out.empty() ? 0 : 1)) return die();
        sr_iter_stats st;
        if (sr_ctx_iterative_stats(ctx, &st, nullptr, 0)) return die();
        printf("Processing %llu tree pairs (k=%u, k_far=%u) + %llu random pairs (frac=%s)\n", (unsigned long long)st.tree_entries,
               st.tree_k_nearest, st.tree_k_farthest, (unsigned long long)st.random_entries, rust_f64(st.tree_rand_frac).c_str());
        if (!paf_out.empty()) printf("Writing alignments to %s\n", paf_out.c_str());
        printf("\nPhase 1: Processing tree pairs (k-nearest + k-farthest)...\n");
        if (sr_ctx_run_iterative(ctx) || sr_ctx_sync(ctx) || sr_ctx_iterative_stats(ctx, &st, nullptr, 0)) return die();
        std::vector<uint64_t> cc(st.checks + 1);
        if (sr_ctx_iterative_stats(ctx, &st, cc.data(), st.checks)) return die();
        printf("Phase 1 complete: %llu components after tree pairs\n", (unsigned long long)st.post_tree);
        printf("\nPhase 2: Processing random pairs with early stopping...\n");
        uint64_t prev = st.post_tree;
        for (uint64_t k = 0; k < st.checks; k++) {
            if (verbose) printf("  After %llu random pairs: %llu components (prev: %llu)\n", (unsigned long long)(k + 1) * 10,
                                (unsigned long long)cc[k], (unsigned long long)prev);
            if (st.stabilized && k + 1 == st.checks) {
                const uint64_t m = (k + 1) * 10, r = st.random_entries;
                printf("Graph stabilized after %llu random pairs (%llu components)\n", (unsigned long long)m, (unsigned long long)cc[k]);
                printf("Skipped %llu random pairs (%s%% reduction)\n", (unsigned long long)(r - m), rust_f64((double)(r - m) / (double)r * 100.0).c_str());
            }
            prev = cc[k];
        }
        printf("\nFinal component count: %llu\n", (unsigned long long)st.final_components);
        if (!paf_out.empty()) {
            sr_alignments *al = nullptr;
            if (sr_ctx_iterative_alignments(ctx, &al)) return die();
            if (sr_write_paf(al, &set, paf_out.c_str())) { sr_alignments_free(al); return die(); }
            sr_alignments_free(al);
        }
    } else if (plan) {                                       // --extend: only the pairs that touch a new sequence, seeded union-find
        if (sr_ctx_load_extend(ctx, plan, &p)) return die();
        printf("Extending %u paths by %u sequences: %llu pairs to align\n", sr_extend_plan_n_old(plan), set.n - sr_extend_plan_n_old(plan),
               (unsigned long long)sr_ctx_num_pairs(ctx));
    } else {
        if (sr_ctx_load(ctx, &set, &p)) return die();
        if (patch_inv) {
            sr_inv_params ip{inv_min, paf_out.empty() ? 0 : 1, (uint32_t)inv_join};
            if (sr_ctx_enable_inversions(ctx, &ip)) return die();
        }
    }
    if (!labels_in.empty() || iterative) {
    } else if (!paf_in.empty() || paf_out.empty()) {
        if (sr_ctx_run(ctx)) return die();                   // align + unite, batch after batch (PAF input: unite only)
    } else {                                                 // --output-alignments (src/seqrush.rs:678-716)
        sr_alignments *al = nullptr;
        if (sr_ctx_align_all(ctx, 1, &al)) return die();
        printf("Writing alignments to %s\n", paf_out.c_str());
        if (sr_write_paf(al, &set, paf_out.c_str())) { sr_alignments_free(al); return die(); }
        sr_alignments_free(al);
        sr_inv_stats ist;
        if (patch_inv && !sr_ctx_inversion_stats(ctx, &ist) && ist.candidates > 0) {     // accepted patches after the main records
            if (sr_ctx_inversion_alignments(ctx, &al)) return die();
            if (sr_append_paf_tagged(al, &set, paf_out.c_str(), "sr:Z:inv")) { sr_alignments_free(al); return die(); }
            sr_alignments_free(al);
        }
    }
    if (sr_ctx_sync(ctx)) return die();
    if (plan && verbose) {
        sr_extend_stats es;
        if (sr_ctx_extend_stats(ctx, &es)) return die();
        printf("Extend: %llu paths %llu bases %llu steps + %llu sequences, pairs %llu of %llu, unions %llu of %llu, spell_us=%llu seed_us=%llu\n",
               (unsigned long long)es.old_paths, (unsigned long long)es.old_bases, (unsigned long long)es.old_steps,
               (unsigned long long)es.new_sequences, (unsigned long long)es.pairs_after, (unsigned long long)es.pairs_before,
               (unsigned long long)es.unions_joined, (unsigned long long)es.unions_attempted, (unsigned long long)es.spell_us,
               (unsigned long long)es.seed_us);
    }
    if (patch_inv) {
        sr_inv_stats ist;
        if (sr_ctx_inversion_stats(ctx, &ist)) return die();
        printf("Patched inversions: %llu of %llu candidate gaps\n", (unsigned long long)ist.accepted, (unsigned long long)ist.candidates);
        if (verbose && inv_join) {
            uint64_t js[4];
            if (sr_ctx_inversion_join_stats(ctx, js)) return die();
            printf("Inversion join: %llu match islands absorbed into candidate gaps, %llu jobs rejected by site cost\n",
                   (unsigned long long)js[0], (unsigned long long)js[1]);
        }
    }
    if (!labels_out.empty()) {                               // shard run: the forest's canonical labels, no graph
        const uint64_t ufn = sr_ctx_uf_size(ctx);
        std::vector<uint64_t> lab(ufn);
        if (sr_ctx_download_labels(ctx, lab.data())) return die();
        FILE *f = fopen(labels_out.c_str(), "wb");
        PartHeader h;
        memcpy(h.magic, PART_MAGIC, 8); h.uf_size = ufn; h.shard_rank = shard_rank; h.shard_count = shard_count; h.input_hash = input_hash; h.flags = 0;
        if (!f || fwrite(&h, sizeof(h), 1, f) != 1 || fwrite(lab.data(), 8, ufn, f) != ufn) { fprintf(stderr, "Error: cannot write %s\n", labels_out.c_str()); if (f) fclose(f); sr_ctx_destroy(ctx); return 1; }
        fclose(f);
        printf("Labels of shard %u/%u written to %s\n", shard_rank, shard_count, labels_out.c_str());
        sr_ctx_destroy(ctx);
        return 0;
    }
    char *gfa = nullptr;
    uint64_t nn = 0, ne = 0;
    sp.device = device;
    const int compact = no_compact ? 0 : (compact_dev ? 2 : 1);          // compact + renumber unless --no-compact
    if (sort ? sr_ctx_build_gfa_sorted(ctx, &set, compact, &sp, &gfa, &nn, &ne)
             : sr_ctx_build_gfa_opts(ctx, &set, compact, &gfa, &nn, &ne)) return die();
    if (verbose && compact_dev) {
        uint64_t cs[8] = {0};
        sr_compact_stats(cs);
        printf("Compaction on device: rounds=%llu host_rounds=%llu chains=%llu longest_list=%llu jumps=%llu compact_us=%llu copy_us=%llu\n",
               (unsigned long long)cs[0], (unsigned long long)cs[1], (unsigned long long)cs[2], (unsigned long long)cs[3],
               (unsigned long long)cs[4], (unsigned long long)cs[5], (unsigned long long)cs[6]);
    }
    sr_ctx_destroy(ctx);
    sr_extend_plan_free(plan);                               // (`set` is not read below)
    std::ofstream o(output, std::ios::binary);
    o << gfa;
    std::vector<std::string> pnames;                         // names of the P lines, as the library's parser reads them
    std::vector<const char *> pn;
    if (!stats_out.empty() || !bin_out.empty() || !viz_out.empty() || !growth_out.empty() || !vcf_out.empty() || !lift_in.empty()) {
        for (const char *q = gfa; *q;) {
            const char *eol = strchr(q, '\n');
            if (!eol) eol = q + strlen(q);
            if (*q == 'P' && q + 2 < eol && q[1] == '\t') {
                const char *b = q + 2, *e = (const char *)memchr(b, '\t', (size_t)(eol - b));
                if (e) pnames.emplace_back(b, e);
            }
            q = *eol ? eol + 1 : eol;
        }
        for (const auto &n : pnames) pn.push_back(n.c_str());
    }
    if (!stats_out.empty()) {                                // the report of the text just written
        sr_graph_stats *gs = nullptr;
        char *report = nullptr;
        if (sr_graph_stats_gfa(gfa, device, &gs)) { fprintf(stderr, "Error: %s\n", sr_last_error()); sr_free(gfa); return 1; }
        if (pn.size() != gs->paths || sr_graph_stats_report(gs, pn.data(), &report)) {
            fprintf(stderr, "Error: %s\n", pn.size() != gs->paths ? "statistics: path names do not match the paths" : sr_last_error());
            sr_graph_stats_free(gs); sr_free(gfa);
            return 1;
        }
        std::ofstream so(stats_out, std::ios::binary);
        so << report;
        sr_free(report);
        printf("Statistics written to %s\n", stats_out.c_str());
        if (verbose) printf("Statistics stage: %llu us on device %d\n", (unsigned long long)gs->stats_us, device);
        sr_graph_stats_free(gs);
    }
    if (!layout_out.empty() || !layout_svg_out.empty()) {    // the 2-D layout of the text just written
        uint64_t n_seg = 0;
        for (const char *q = gfa; *q;) {
            if (q[0] == 'S' && q[1] == '\t') n_seg++;
            const char *eol = strchr(q, '\n');
            q = eol ? eol + 1 : q + strlen(q);
        }
        lp.device = device;
        std::vector<double> xy(4 * n_seg + 1);
        char *tsv = nullptr, *svg = nullptr;
        if (sr_layout_gfa(gfa, &lp, xy.data(), n_seg) || (!layout_out.empty() && sr_layout_tsv(xy.data(), n_seg, &tsv)) ||
            (!layout_svg_out.empty() && sr_layout_svg(gfa, xy.data(), n_seg, &svg))) {
            fprintf(stderr, "Error: %s\n", sr_last_error());
            sr_free(tsv); sr_free(gfa);
            return 1;
        }
        if (tsv) { std::ofstream lo(layout_out, std::ios::binary); lo << tsv; }
        if (svg) { std::ofstream lo(layout_svg_out, std::ios::binary); lo << svg; }
        sr_free(tsv); sr_free(svg);
        printf("Layout written to %s\n", (!layout_out.empty() ? layout_out : layout_svg_out).c_str());
        if (verbose) {
            double st[7] = {0};
            sr_layout_stats(st, 7);
            printf("Layout stage: SGD %.3f ms, stage %.3f ms on device %d\n", st[0], st[6], device);
        }
    }
    for (int pass = 0; pass < 2; pass++) {                   // the path-by-bin tables of the text just written
        const std::string &dst = pass == 0 ? bin_out : viz_out;
        if (dst.empty()) continue;
        sr_bin_params bp = {0, 0};
        if (pass == 0) { bp.bin_width = bin_width; bp.bins = bin_width ? 0 : (bin_count ? bin_count : 1500); }
        else bp.bins = viz_width;
        sr_path_bins *pb = nullptr;
        char *tsv = nullptr;
        uint8_t *png = nullptr;
        uint64_t png_size = 0;
        if (sr_path_bins_gfa(gfa, &bp, device, &pb)) { fprintf(stderr, "Error: %s\n", sr_last_error()); sr_free(gfa); return 1; }
        if (pn.size() != pb->paths || (pass == 0 ? sr_path_bins_tsv(pb, pn.data(), &tsv) : sr_path_bins_png(pb, pn.data(), &vp, &png, &png_size))) {
            fprintf(stderr, "Error: %s\n", pn.size() != pb->paths ? "bins: path names do not match the paths" : sr_last_error());
            sr_path_bins_free(pb); sr_free(gfa);
            return 1;
        }
        std::ofstream bo(dst, std::ios::binary);
        if (pass == 0) bo << tsv; else bo.write((const char *)png, (std::streamsize)png_size);
        sr_free(tsv); sr_free(png);
        printf("%s written to %s\n", pass == 0 ? "Bins" : "Visualization", dst.c_str());
        if (verbose) printf("Bin stage: %llu us on device %d\n", (unsigned long long)pb->bin_us, device);
        sr_path_bins_free(pb);
    }
    if (!growth_out.empty()) {                               // the growth curves of the text just written
        std::vector<uint32_t> group_of(pn.size() ? pn.size() : 1);
        uint32_t n_groups = 0;
        sr_growth *gr = nullptr;
        char *report = nullptr;
        if (sr_growth_groups(pn.data(), pn.size(), growth_mode, group_of.data(), &n_groups, nullptr) ||
            sr_growth_gfa(gfa, group_of.data(), n_groups, &gp, device, &gr)) { fprintf(stderr, "Error: %s\n", sr_last_error()); sr_free(gfa); return 1; }
        if (sr_growth_report(gr, &report)) { fprintf(stderr, "Error: %s\n", sr_last_error()); sr_growth_free(gr); sr_free(gfa); return 1; }
        std::ofstream go(growth_out, std::ios::binary);
        go << report;
        sr_free(report);
        printf("Growth written to %s\n", growth_out.c_str());
        if (verbose) printf("Growth stage: %llu us on device %d\n", (unsigned long long)gr->growth_us, device);
        sr_growth_free(gr);
    }
    if (!vcf_out.empty()) {                                  // the variant sites of the text just written
        sr_variants *va = nullptr;
        char *vcf = nullptr;
        if (!vcf_ref.empty()) vcp.ref_name = vcf_ref.c_str();
        if (sr_variants_gfa(gfa, &vcp, device, &va)) { fprintf(stderr, "Error: %s\n", sr_last_error()); sr_free(gfa); return 1; }
        if (sr_variants_vcf(va, pn.data(), &vcf)) { fprintf(stderr, "Error: %s\n", sr_last_error()); sr_variants_free(va); sr_free(gfa); return 1; }
        std::ofstream vo(vcf_out, std::ios::binary);
        vo << vcf;
        sr_free(vcf);
        printf("VCF written to %s\n", vcf_out.c_str());
        if (verbose) printf("Variants stage: %llu us on device %d\n", (unsigned long long)va->variants_us, device);
        sr_variants_free(va);
    }
    if (!lift_in.empty()) {                                  // the BED intervals lifted over the text just written
        std::ifstream bi(lift_in, std::ios::binary);
        if (!bi) { fprintf(stderr, "Error: cannot read %s\n", lift_in.c_str()); sr_free(gfa); return 1; }
        const std::string bed((std::istreambuf_iterator<char>(bi)), std::istreambuf_iterator<char>());
        sr_lift *lf = nullptr;
        char *lifted = nullptr;
        if (!lift_to.empty()) lfp.to_name = lift_to.c_str();
        if (sr_lift_gfa(gfa, bed.c_str(), &lfp, device, &lf)) { fprintf(stderr, "Error: %s\n", sr_last_error()); sr_free(gfa); return 1; }
        if (pn.size() != lf->paths || sr_lift_bed(lf, pn.data(), &lifted)) {
            fprintf(stderr, "Error: %s\n", pn.size() != lf->paths ? "lift: path names do not match the paths" : sr_last_error());
            sr_lift_free(lf); sr_free(gfa);
            return 1;
        }
        std::ofstream lo(lift_out, std::ios::binary);
        lo << lifted;
        sr_free(lifted);
        printf("Lifted intervals written to %s\n", lift_out.c_str());
        if (verbose)
            printf("Lift stage: %llu us on device %d, %llu queries x %llu targets, %llu mapped, %llu unknown, %llu out of range\n",
                   (unsigned long long)lf->lift_us, device, (unsigned long long)lf->queries, (unsigned long long)lf->targets,
                   (unsigned long long)lf->mapped, (unsigned long long)lf->unknown, (unsigned long long)lf->out_of_range);
        sr_lift_free(lf);
    }
    if (extract_asked) {                                     // the subgraph of the regions, cut out of the text just written
        std::string bed;
        if (!extract_bed.empty()) {
            std::ifstream bi(extract_bed, std::ios::binary);
            if (!bi) { fprintf(stderr, "Error: cannot read %s\n", extract_bed.c_str()); sr_free(gfa); return 1; }
            bed.assign((std::istreambuf_iterator<char>(bi)), std::istreambuf_iterator<char>());
        }
        std::vector<const char *> regs;
        for (const std::string &r : extract_regions) regs.push_back(r.c_str());
        sr_extract *ex = nullptr;
        char *sub = nullptr;
        if (sr_extract_gfa(gfa, extract_bed.empty() ? nullptr : bed.c_str(), regs.data(), regs.size(), &exp_, device, &ex) || sr_extract_text(ex, &sub)) {
            fprintf(stderr, "Error: %s\n", sr_last_error());
            sr_extract_free(ex); sr_free(gfa);
            return 1;
        }
        std::ofstream eo(extract_out, std::ios::binary);
        eo << sub;
        sr_free(sub);
        printf("Extracted graph written to %s\n", extract_out.c_str());
        if (verbose)
            printf("Extract stage: %llu us on device %d, %llu regions, %llu unknown, %llu out of range, %llu seeds + %llu by context + %llu by merge in "
                   "%llu rounds = %llu of %llu nodes, %llu edges, %llu subpaths, %llu steps, %llu bases\n",
                   (unsigned long long)ex->extract_us, device, (unsigned long long)ex->regions, (unsigned long long)ex->unknown,
                   (unsigned long long)ex->out_of_range, (unsigned long long)ex->seeds, (unsigned long long)ex->by_context,
                   (unsigned long long)ex->by_merge, (unsigned long long)ex->merge_rounds_run, (unsigned long long)ex->nodes,
                   (unsigned long long)ex->in_nodes, (unsigned long long)ex->edges, (unsigned long long)ex->subpaths,
                   (unsigned long long)ex->steps, (unsigned long long)ex->bases);
        sr_extract_free(ex);
    }
    sr_free(gfa);
    printf("Graph written to %s\n", output.c_str());
    return 0;
}
