// extract_asan.cpp -- the host side of the subgraph extraction under AddressSanitizer and UBSan: the
// host twin, the region and BED reader with every refusal and skip, and sr_extract_text on the known-answer graph of
// tests/golden/extract_known_answers.json (its text is repeated here: this program reads no file).  A CPU program: it opens
// no device.  Built by `make -C seqrush_amd/csrc extract-asan`, run as seqrush_amd/extract_asan; exit status 0 and
// "extract_asan: ok" mean that every answer matched and the sanitizers reported nothing.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../include/seqrush_amd.h"

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "extract_asan: line %d: %s\n", __LINE__, #c); fails++; } } while (0)

// a = 1+ 2+ 3+ 4+ 5+ (13 bases), b = 5- 4- 3- 1- (reversed), c visits node 3 twice, e has no step, z shares nothing; node 8
// is on no path and hangs on node 2; node 7 has a self-loop
static const char *GFA = "H\tVN:Z:1.0\nS\t1\tACG\nS\t2\tT\nS\t3\tGGA\nS\t4\tCC\nS\t5\tTTTT\nS\t6\tAG\nS\t7\tCA\nS\t8\tG\n"
                         "L\t1\t+\t2\t+\t0M\nL\t2\t+\t3\t+\t0M\nL\t3\t+\t4\t+\t0M\nL\t4\t+\t5\t+\t0M\nL\t1\t+\t3\t+\t0M\nL\t3\t+\t6\t+\t0M\nL\t6\t+\t3\t+\t0M\n"
                         "L\t2\t+\t8\t+\t0M\nL\t7\t+\t7\t+\t0M\n"
                         "P\ta\t1+,2+,3+,4+,5+\t*\nP\tb\t5-,4-,3-,1-\t*\nP\tc\t1+,3+,6+,3+,5+\t*\nP\te\t\t*\nP\tz\t7+\t*\n";
static const char *BED = "# loci of haplotype a\r\ntrack name=loci\r\n\r\na\t3\t4\tsnp\r\nc 6 8 second\r\nchrUn\t0\t5\r\na\t5\t5\r\nb\t0\t13\r\ne\t0\t1\r\n";
static const uint32_t NONE = 0xffffffffu;

static sr_extract *run(const char *gfa, const char *bed, std::vector<const char *> regions, uint64_t c, uint64_t D, uint64_t R, int want, char **text) {
    sr_extract_params p;
    sr_extract_params_default(&p);
    EXPECT(p.context_steps == 0 && p.merge_distance == 100000 && p.merge_rounds == 3 && p.reserved == 0);
    p.context_steps = c; p.merge_distance = D; p.merge_rounds = R;
    sr_extract *x = nullptr;
    const int rc = sr_extract_gfa(gfa, bed, regions.data(), regions.size(), &p, SR_EXTRACT_DEVICE_HOST, &x);
    EXPECT(rc == want);
    if (rc) { EXPECT(x == nullptr && strlen(sr_last_error()) > 0); return nullptr; }
    EXPECT(x->variant == 0 && x->sub_off[x->subpaths] == x->steps && x->seeds + x->by_context + x->by_merge == x->nodes);
    if (text) EXPECT(sr_extract_text(x, text) == SR_OK && *text);
    return x;
}

static void refused(std::vector<const char *> regions, const char *bed, const char *what) {
    run(GFA, bed, regions, 0, 0, 3, SR_ERR_INVALID, nullptr);
    EXPECT(strstr(sr_last_error(), what) != nullptr);
}

int main() {
    char *text = nullptr;
    sr_extract *x;
    if ((x = run(GFA, nullptr, {"a:3-4"}, 0, 0, 3, SR_OK, &text))) {
        EXPECT(x->regions == 1 && x->in_nodes == 8 && x->in_edges == 9 && x->in_steps == 15 && x->in_paths == 5 && x->nodes == 1 && x->bases == 1);
        EXPECT(x->level[1] == 0 && x->level[0] == NONE && x->node_old[0] == 2 && x->sub_path[0] == 0 && x->sub_start[0] == 3 && x->sub_end[0] == 4);
        if (text) EXPECT(!strcmp(text, "H\tVN:Z:1.0\nS\t1\tT\nP\ta:3-4\t1+\t*\n"));
        sr_free(text); text = nullptr;
        sr_extract_free(x);
    }
    if ((x = run(GFA, nullptr, {"c:6-8"}, 1, 0, 3, SR_OK, &text))) {
        EXPECT(x->nodes == 2 && x->edges == 2 && x->subpaths == 3 && x->steps == 5 && x->seeds == 1 && x->by_context == 1);
        EXPECT(x->edge_from[0] == 2 && x->edge_to[0] == 4 && x->edge_from[1] == 4 && x->edge_to[1] == 2 && x->sub_steps[1] == 3);
        if (text) EXPECT(!strcmp(text, "H\tVN:Z:1.0\nS\t1\tGGA\nS\t2\tAG\nL\t1\t+\t2\t+\t0M\nL\t2\t+\t1\t+\t0M\nP\ta:4-7\t1+\t*\nP\tb:6-9\t1-\t*\nP\tc:3-11\t1+,2+,1+\t*\n"));
        sr_free(text); text = nullptr;
        sr_extract_free(x);
    }
    if ((x = run(GFA, nullptr, {"a:0-1", "a:12-13"}, 0, 6, 1, SR_OK, &text))) {
        EXPECT(x->nodes == 5 && x->subpaths == 4 && x->by_merge == 3 && x->merge_rounds_run == 1 && x->level[5] == NONE);
        if (text) EXPECT(strstr(text, "P\tc:0-6\t1+,3+\t*\nP\tc:8-15\t3+,5+\t*\n") != nullptr);
        sr_free(text); text = nullptr;
        sr_extract_free(x);
    }
    if ((x = run(GFA, nullptr, {"a:0-1", "a:12-13"}, 0, 6, 64, SR_OK, &text))) {
        EXPECT(x->nodes == 6 && x->subpaths == 3 && x->by_merge == 4 && x->merge_rounds_run == 2 && x->level[5] == 2 && x->level[2] == 1);
        sr_free(text); text = nullptr;
        sr_extract_free(x);
    }
    if ((x = run(GFA, nullptr, {"z"}, 0, 100000, 3, SR_OK, &text))) {
        if (text) EXPECT(!strcmp(text, "H\tVN:Z:1.0\nS\t1\tCA\nL\t1\t+\t1\t+\t0M\nP\tz:0-2\t1+\t*\n"));
        sr_free(text); text = nullptr;
        sr_extract_free(x);
    }
    if ((x = run(GFA, BED, {"b:11-12", "e"}, 2, 1, 3, SR_OK, &text))) {
        EXPECT(x->regions == 3 && x->unknown == 1 && x->out_of_range == 4 && x->nodes == 6 && x->level[7] == 1 && x->level[4] == NONE);
        sr_free(text); text = nullptr;
        sr_extract_free(x);
    }
    if ((x = run(GFA, nullptr, {"a", "b", "c", "e", "z"}, 65535, ~0ULL, 64, SR_OK, &text))) {
        EXPECT(x->nodes == 8 && x->edges == 9 && x->steps == 15 && x->subpaths == 4 && x->out_of_range == 1 && x->by_context == 1);
        sr_free(text); text = nullptr;
        sr_extract_free(x);
    }
    // nothing to do is no error
    for (const char *gfa : {"", "H\tVN:Z:1.0\n", "S\t1\tACGT\n", GFA})
        if ((x = run(gfa, "chrUn\t0\t1\n", {}, 2, 5, 3, SR_OK, &text))) {
            EXPECT(x->nodes == 0 && x->subpaths == 0 && x->unknown == 1 && text && !strcmp(text, "H\tVN:Z:1.0\n"));
            sr_free(text); text = nullptr;
            sr_extract_free(x);
        }
    if ((x = run(GFA, "\n\n# x\ntrack\nbrowser\n   \n\t\n", {"e"}, 0, 0, 0, SR_OK, nullptr))) { EXPECT(x->regions == 0 && x->out_of_range == 1); sr_extract_free(x); }
    if ((x = run(GFA, "a 0 13 all rest of the line", {}, 0, 0, 0, SR_OK, nullptr))) { EXPECT(x->regions == 1 && x->nodes == 5); sr_extract_free(x); }
    if ((x = run(GFA, "a\t1\t18446744073709551615\n", {}, 0, 0, 0, SR_OK, nullptr))) { EXPECT(x->out_of_range == 1 && x->regions == 0); sr_extract_free(x); }
    // every refusal of the BED reader names its line, every refusal of a region names the string
    refused({}, "a\t1\n", "extract: BED line 1: fewer than three fields");
    refused({}, "#x\n\na\t1\t2\na\tx\t2\n", "extract: BED line 4: start 'x' is not a number");
    refused({}, "a\t1\t-2\n", "BED line 1: end '-2' is not a number");
    refused({}, "a\t1\t18446744073709551616\n", "is not a number");
    refused({"nobody"}, nullptr, "region 'nobody': no path has this name");
    refused({"a:5"}, nullptr, "region 'a:5': '5' is not START-END");
    refused({"a:x-5"}, nullptr, "'x-5' is not START-END");
    refused({"a:1-"}, nullptr, "'1-' is not START-END");
    refused({"a:1-18446744073709551616"}, nullptr, "is not START-END");
    refused({"q:0-1"}, nullptr, "no path is named 'q'");
    refused({"a:3-3"}, nullptr, "start must lie below end");
    refused({"a:0-14"}, nullptr, "end lies beyond the 13 bases of the path");
    refused({"e:0-1"}, nullptr, "end lies beyond the 0 bases of the path");
    refused({""}, nullptr, "region ''");
    run(GFA, nullptr, {"a"}, 65536, 0, 3, SR_ERR_UNSUPPORTED, nullptr);
    run(GFA, nullptr, {"a"}, 0, 0, 65, SR_ERR_UNSUPPORTED, nullptr);
    run("S\tx\tACGT\n", nullptr, {}, 0, 0, 3, SR_ERR_INVALID, nullptr);
    run("S\t1\t\nP\ta\t1+\t*\n", nullptr, {"a"}, 0, 0, 3, SR_ERR_INVALID, nullptr);
    sr_extract_params p;
    sr_extract_params_default(&p);
    x = nullptr;
    const char *one[1] = {"a"};
    EXPECT(sr_extract_gfa(GFA, nullptr, one, 1, &p, -2, &x) == SR_ERR_INVALID && x == nullptr);
    EXPECT(sr_extract_gfa(nullptr, nullptr, one, 1, &p, SR_EXTRACT_DEVICE_HOST, &x) == SR_ERR_INVALID);
    EXPECT(sr_extract_gfa(GFA, nullptr, nullptr, 1, &p, SR_EXTRACT_DEVICE_HOST, &x) == SR_ERR_INVALID);
    EXPECT(sr_extract_text(nullptr, &text) == SR_ERR_INVALID);
    sr_extract_free(nullptr);
    sr_extract_params_default(nullptr);
    // a chain of 3000 one-base nodes with a gap of 2000 steps that closes, and the same with 300 regions
    std::string chain = "H\tVN:Z:1.0\n", path = "P\tw\t", bed;
    for (int v = 1; v <= 3000; v++) { chain += "S\t" + std::to_string(v) + "\tA\n"; path += std::to_string(v) + (v < 3000 ? "+," : "+"); }
    for (int v = 1; v < 3000; v++) chain += "L\t" + std::to_string(v) + "\t+\t" + std::to_string(v + 1) + "\t+\t0M\n";
    chain += path + "\t*\n";
    for (int k = 0; k < 300; k++) bed += "w\t" + std::to_string(10 * k) + "\t" + std::to_string(10 * k + 3) + "\n";
    if ((x = run(chain.c_str(), nullptr, {"w:100-101", "w:2101-2102"}, 0, 2000, 3, SR_OK, nullptr))) { EXPECT(x->nodes == 2002 && x->edges == 2001 && x->subpaths == 1); sr_extract_free(x); }
    if ((x = run(chain.c_str(), bed.c_str(), {}, 1, 0, 3, SR_OK, &text))) { EXPECT(x->regions == 300 && x->seeds == 900 && x->by_context == 599 && x->subpaths == 300); sr_free(text); text = nullptr; sr_extract_free(x); }

    if (fails) { fprintf(stderr, "extract_asan: %d check(s) failed\n", fails); return 1; }
    printf("extract_asan: ok\n");
    return 0;
}
