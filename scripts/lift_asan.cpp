// lift_asan.cpp -- the host side of the interval lift under AddressSanitizer and UBSan: the host
// twin, the BED reader with every refusal and skip, and sr_lift_bed on the known-answer graph of
// tests/golden/lift_known_answers.json (its text is repeated here: this program reads no file).  A CPU program: it opens no
// device.  Built by `make -C seqrush_amd/csrc lift-asan`, run as seqrush_amd/lift_asan; exit status 0 and "lift_asan: ok"
// mean that every answer matched and the sanitizers reported nothing.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include "../include/seqrush_amd.h"

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "lift_asan: line %d: %s\n", __LINE__, #c); fails++; } } while (0)

// a = 1+ 2+ 3+ 4+ 5+ (13 bases), b = 5- 4- 3- 1- (reversed), c visits node 3 twice, e has no step, z shares nothing
static const char *GFA = "H\tVN:Z:1.0\nS\t1\tACG\nS\t2\tT\nS\t3\tGGA\nS\t4\tCC\nS\t5\tTTTT\nS\t6\tAG\nS\t7\tCA\n"
                         "P\ta\t1+,2+,3+,4+,5+\t*\nP\tb\t5-,4-,3-,1-\t*\nP\tc\t1+,3+,6+,3+,5+\t*\nP\te\t\t*\nP\tz\t7+\t*\n";
static const char *BED = "# genes of haplotype a\r\ntrack name=genes\r\nbrowser position a:1-10\r\n\r\na\t2\t5\tgeneA\r\na\t0\t13\r\n"
                         "a\t3\t4\tsnp\t0\t+\textra\r\nb\t0\t12\twhole_b\r\nc\t5\t11\ttwice\r\nc 8 9 second_visit\r\nz\t0\t2\talone\r\n"
                         "chrUn\t0\t5\tnot_in_graph\r\na\t5\t5\tempty\r\na\t4\t14\tbeyond\r\ne\t0\t1\tno_bases\r\nb\t11\t12\r\na\t2\t5\tgeneA\r\n";
static const char *NAMES[5] = {"a", "b", "c", "e", "z"};

static sr_lift *run(const char *gfa, const char *bed, const char *to, uint64_t min_covered, int want, char **text) {
    sr_lift_params p;
    sr_lift_params_default(&p);
    EXPECT(p.to_name == nullptr && p.min_covered == 1 && p.short_steps == 8 && p.reserved == 0);
    p.to_name = to; p.min_covered = min_covered;
    sr_lift *l = nullptr;
    const int rc = sr_lift_gfa(gfa, bed, &p, SR_LIFT_DEVICE_HOST, &l);
    EXPECT(rc == want);
    if (rc) { EXPECT(l == nullptr && strlen(sr_last_error()) > 0); return nullptr; }
    EXPECT(l->variant == 0 && l->short_pairs == 0 && l->long_pairs == 0 && l->min_covered == min_covered && l->to_named == (to ? 1 : 0));
    if (text) EXPECT(sr_lift_bed(l, NAMES, text) == SR_OK && *text);
    return l;
}

static void refused(const char *bed, const char *what) {
    run(GFA, bed, nullptr, 1, SR_ERR_INVALID, nullptr);
    EXPECT(strstr(sr_last_error(), what) != nullptr);
}

int main() {
    char *text = nullptr;
    sr_lift *l;
    if ((l = run(GFA, BED, nullptr, 1, SR_OK, &text))) {
        EXPECT(l->queries == 9 && l->targets == 5 && l->paths == 5 && l->unknown == 1 && l->out_of_range == 3 && l->mapped == 23);
        EXPECT(l->q_path[0] == 0 && l->q_start[0] == 2 && l->q_end[0] == 5 && !memcmp(l->labels + l->label_off[0], "geneA", 5));
        EXPECT(l->label_off[2] - l->label_off[1] == 6 && !memcmp(l->labels + l->label_off[1], "a:0-13", 6));
        // geneA against b: the last base of node 1 and the first of node 3, both on the reverse strand
        EXPECT(l->tstart[1] == 8 && l->tend[1] == 10 && l->covered[1] == 2 && l->rev_bp[1] == 2);
        EXPECT(l->tstart[2] == 2 && l->tend[2] == 4 && l->covered[2] == 2 && l->rev_bp[2] == 0);
        EXPECT(l->covered[3] == 0 && l->tstart[3] == 0 && l->tend[3] == 0 && l->covered[4] == 0);          // e and z
        EXPECT(l->tstart[0] == 2 && l->tend[0] == 5 && l->covered[0] == 3);                              // its own path
        if (text) {
            EXPECT(strstr(text, "b\t8\t10\tgeneA\t2\t-\ta\t2\t5\t2\nc\t2\t4\tgeneA\t2\t+\ta\t2\t5\t0\n") == text);
            EXPECT(strstr(text, "c\t0\t15\ta:0-13\t10\t+\ta\t0\t13\t0\n") && strstr(text, "a\t4\t7\ttwice\t4\t+\tc\t5\t11\t0\n"));
            EXPECT(strstr(text, "b\t8\t9\tsecond_visit\t1\t-\tc\t8\t9\t1\n") && strstr(text, "a\t0\t1\tb:11-12\t1\t-\tb\t11\t12\t1\n"));
            EXPECT(!strstr(text, "alone") && !strstr(text, "snp") && !strstr(text, "whole_b\t12\t+"));
        }
        sr_free(text); text = nullptr;
        sr_lift_free(l);
    }
    if ((l = run(GFA, BED, "b", 1, SR_OK, &text))) {
        EXPECT(l->targets == 1 && l->target_path[0] == 1 && l->queries == 9);
        if (text) EXPECT(strstr(text, "b\t0\t12\twhole_b\t12\t+\tb\t0\t12\t0\n") != nullptr);
        sr_free(text); text = nullptr;
        sr_lift_free(l);
    }
    if ((l = run(GFA, BED, nullptr, 3, SR_OK, &text))) {
        if (text) EXPECT(!strstr(text, "geneA") && strstr(text, "twice\t4\t"));
        sr_free(text); text = nullptr;
        sr_lift_free(l);
    }
    if ((l = run(GFA, BED, "e", 1, SR_OK, &text))) { EXPECT(l->mapped == 0 && text && !*text); sr_free(text); text = nullptr; sr_lift_free(l); }
    // nothing to do is no error
    if ((l = run("H\tVN:Z:1.0\n", BED, nullptr, 1, SR_OK, &text))) { EXPECT(l->paths == 0 && l->queries == 0 && l->unknown == 13 && text && !*text); sr_free(text); text = nullptr; sr_lift_free(l); }
    if ((l = run(GFA, "", nullptr, 1, SR_OK, &text))) { EXPECT(l->queries == 0 && l->targets == 5 && text && !*text); sr_free(text); text = nullptr; sr_lift_free(l); }
    if ((l = run(GFA, "\n\n# x\ntrack\nbrowser\n   \n\t\n", nullptr, 1, SR_OK, nullptr))) { EXPECT(l->queries == 0); sr_lift_free(l); }
    if ((l = run(GFA, "a 0 13 all rest of the line", nullptr, 1, SR_OK, nullptr))) {        // no newline at the end, blanks
        EXPECT(l->queries == 1 && l->label_off[1] == 3 && !memcmp(l->labels, "all", 3) && l->covered[1] == 12);
        sr_lift_free(l);
    }
    // every refusal of the reader names its line
    refused("a\t1\n", "BED line 1: fewer than three fields");
    refused("a\n", "BED line 1: fewer than three fields");
    refused("#x\n\na\t1\t2\na\tx\t2\n", "BED line 4: start 'x' is not a number");
    refused("a\t1\t-2\n", "BED line 1: end '-2' is not a number");
    refused("a\t\t2\n", "BED line 1: start '' is not a number");
    refused("a\t1\t18446744073709551616\n", "is not a number");
    refused("chrUn\t1.5\t2\n", "BED line 1: start '1.5' is not a number");
    if ((l = run(GFA, "a\t1\t18446744073709551615\n", nullptr, 1, SR_OK, nullptr))) { EXPECT(l->out_of_range == 1 && l->queries == 0); sr_lift_free(l); }
    run(GFA, BED, "nobody", 1, SR_ERR_INVALID, nullptr);
    run("H\tVN:Z:1.0\n", "", "a", 1, SR_ERR_INVALID, nullptr);
    run("S\tx\tACGT\n", BED, nullptr, 1, SR_ERR_INVALID, nullptr);
    sr_lift_params p;
    sr_lift_params_default(&p);
    l = nullptr;
    EXPECT(sr_lift_gfa(GFA, BED, &p, -2, &l) == SR_ERR_INVALID && l == nullptr);
    EXPECT(sr_lift_gfa(nullptr, BED, &p, SR_LIFT_DEVICE_HOST, &l) == SR_ERR_INVALID);
    EXPECT(sr_lift_gfa(GFA, nullptr, &p, SR_LIFT_DEVICE_HOST, &l) == SR_ERR_INVALID);
    EXPECT(sr_lift_bed(nullptr, NAMES, &text) == SR_ERR_INVALID);
    sr_lift_free(nullptr);
    // queries x targets above 2^26 and targets x nodes above 2^28: 8193 targets of which all but one have no step
    std::string paths, bed, nodes;
    for (int k = 0; k < 8192; k++) { paths += "P\te" + std::to_string(k) + "\t\t*\n"; bed += "q\t0\t1\n"; }
    for (int v = 2; v <= 32769; v++) nodes += "S\t" + std::to_string(v) + "\tA\n";
    run(("S\t1\tA\nP\tq\t1+\t*\n" + paths).c_str(), bed.c_str(), nullptr, 1, SR_ERR_UNSUPPORTED, nullptr);
    run(("S\t1\tA\n" + nodes + "P\tq\t1+\t*\n" + paths).c_str(), "q\t0\t1\n", nullptr, 1, SR_ERR_UNSUPPORTED, nullptr);
    if ((l = run(("S\t1\tA\n" + nodes + "P\tq\t1+\t*\n" + paths).c_str(), "q\t0\t1\n", "q", 1, SR_OK, nullptr))) { EXPECT(l->covered[0] == 1); sr_lift_free(l); }

    if (fails) { fprintf(stderr, "lift_asan: %d check(s) failed\n", fails); return 1; }
    printf("lift_asan: ok\n");
    return 0;
}
