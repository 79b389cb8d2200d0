// variants_asan.cpp -- the host side of the variant sites under AddressSanitizer and UBSan: the host
// twin, sr_variants_vcf and the refusals on the known-answer graphs of tests/golden/variants_known_answers.json (their text
// is repeated here: this program reads no file).  A CPU program: it opens no device.  Built by
// `make -C seqrush_amd/csrc variants-asan`, run as seqrush_amd/variants_asan; exit status 0 and "variants_asan: ok" mean
// that every answer matched and the sanitizers reported nothing.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include "../include/seqrush_amd.h"

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "variants_asan: line %d: %s\n", __LINE__, #c); fails++; } } while (0)

#define NODES "H\tVN:Z:1.0\nS\t1\tACG\nS\t2\tT\nS\t3\tG\nS\t4\tTTA\n"
static const char *SNP = NODES "P\tref\t1+,2+,4+\t*\nP\ta\t1+,3+,4+\t*\n";
static const char *INS = NODES "P\tref\t1+,4+\t*\nP\ta\t1+,2+,4+\t*\n";
static const char *DEL = NODES "P\tref\t1+,2+,4+\t*\nP\ta\t1+,4+\t*\n";
static const char *TRI = NODES "S\t5\tC\nP\tref\t1+,2+,4+\t*\nP\ta\t1+,3+,4+\t*\nP\tb\t1+,5+,4+\t*\nP\tc\t1+,2+,4+\t*\n";
static const char *REVISIT = NODES "P\tref\t1+,2+,3+,2+,4+\t*\nP\ta\t1+,2+,3+,2+,4+\t*\n";
static const char *BREAKS = NODES "P\tref\t1+,2+,4+\t*\nP\ta\t1+,2+,4-\t*\nP\tb\t2+,4+,1+\t*\n";
static const char *TWICE = NODES "S\t5\tC\nP\tref\t1+,2+,4+\t*\nP\ta\t1+,3+,4+,1+,5+,4+\t*\nP\tb\t1+,5+,4+,1+,3+,4+\t*\n";
static const char *REVSAMPLE = NODES "P\tref\t1+,2+,4+\t*\nP\ta\t4-,3-,1-\t*\n";
static const char *REVREF = NODES "P\ta\t1+,3+,4+\t*\nP\tref\t4-,2-,1-\t*\n";
static const char *EMPTY = "H\tVN:Z:1.0\n";
static const char *NOSTEPS = NODES "P\tref\t\t*\nP\ta\t1+,3+,4+\t*\n";

static sr_variants *run(const char *gfa, const char *ref, uint64_t max_len, int want, const char *const *names, const char *record) {
    sr_variant_params p;
    sr_variant_params_default(&p);
    EXPECT(p.ref_name == nullptr && p.max_allele_len == 10000 && p.hash_mask == ~0ULL && p.reserved == 0);
    p.ref_name = ref; p.max_allele_len = max_len;
    sr_variants *v = nullptr;
    const int rc = sr_variants_gfa(gfa, &p, SR_VARIANTS_DEVICE_HOST, &v);
    EXPECT(rc == want);
    if (rc) { EXPECT(v == nullptr && strlen(sr_last_error()) > 0); return nullptr; }
    EXPECT(v->variant == 0 && v->hash_collision_sites == 0);
    char *text = nullptr;
    EXPECT(sr_variants_vcf(v, names, &text) == SR_OK && text && strstr(text, "##fileformat=VCFv4.2\n##source=seqrush_amd variants v1\n") == text);
    if (text && record) EXPECT(strstr(text, record) != nullptr);
    sr_free(text);
    return v;
}

int main() {
    const char *ra[2] = {"ref", "a"}, *rabc[4] = {"ref", "a", "b", "c"}, *ar[2] = {"a", "ref"};
    sr_variants *v;
    if ((v = run(SNP, nullptr, 10000, SR_OK, ra, "\nref\t4\t.\tT\tG\t.\t.\tAC=1;AN=1\tGT\t1\n"))) {
        EXPECT(v->sites == 1 && v->anchors == 3 && v->traversals == 1 && v->ref_len == 7 && !memcmp(v->ref_seq, "ACGTTTA", 7));
        EXPECT(v->site_start[0] == 3 && v->site_end[0] == 4 && v->site_alleles[0] == 1 && v->alleles[0] == 'G' && v->gt[0] == 0 && v->gt[1] == 1);
        sr_variants_free(v);
    }
    sr_variants_free(run(INS, nullptr, 10000, SR_OK, ra, "\nref\t3\t.\tG\tGT\t.\t.\tAC=1;AN=1\tGT\t1\n"));
    sr_variants_free(run(DEL, nullptr, 10000, SR_OK, ra, "\nref\t3\t.\tGT\tG\t.\t.\tAC=1;AN=1\tGT\t1\n"));
    if ((v = run(TRI, "ref", 0, SR_OK, rabc, "\nref\t4\t.\tT\tC,G\t.\t.\tAC=1,1;AN=3\tGT\t2\t1\t0\n"))) {
        EXPECT(v->sites == 1 && v->site_alleles[0] == 2 && v->allele_off[2] == 2 && !memcmp(v->alleles, "CG", 2));
        sr_variants_free(v);
    }
    if ((v = run(REVISIT, nullptr, 10000, SR_OK, ra, nullptr))) { EXPECT(v->sites == 0 && v->traversals == 4 && v->anchors == 3); sr_variants_free(v); }
    if ((v = run(BREAKS, nullptr, 10000, SR_OK, rabc, nullptr))) {
        EXPECT(v->sites == 0 && v->breaks[0] == 0 && v->breaks[1] == 1 && v->breaks[2] == 1);
        sr_variants_free(v);
    }
    if ((v = run(TWICE, nullptr, 10000, SR_OK, rabc, "\tGT\t2\t1\n"))) { EXPECT(v->gt[1] == 2 && v->gt[2] == 1 && v->breaks[1] == 1); sr_variants_free(v); }
    sr_variants_free(run(REVSAMPLE, nullptr, 10000, SR_OK, ra, "\nref\t4\t.\tT\tG\t"));
    if ((v = run(REVREF, "ref", 10000, SR_OK, ar, "\nref\t4\t.\tA\tC\t.\t.\tAC=1;AN=1\tGT\t1\n"))) {
        EXPECT(v->ref_path == 1 && !memcmp(v->ref_seq, "TAAACGT", 7));
        sr_variants_free(v);
    }
    if ((v = run(EMPTY, nullptr, 10000, SR_OK, nullptr, "\tFORMAT\n"))) { EXPECT(v->paths == 0 && v->sites == 0 && v->ref_len == 0); sr_variants_free(v); }
    if ((v = run(NOSTEPS, nullptr, 10000, SR_OK, ra, "\tFORMAT\ta\n"))) { EXPECT(v->paths == 2 && v->sites == 0 && v->anchors == 0); sr_variants_free(v); }
    if ((v = run(DEL, nullptr, 1, SR_OK, ra, nullptr))) { EXPECT(v->sites == 1 && v->skipped[1] == 0); sr_variants_free(v); }
    if ((v = run(TRI, nullptr, 0, SR_OK, rabc, nullptr))) sr_variants_free(v);
    // a two-base allele under a limit of one base is skipped
    static const char *MNP = "H\tVN:Z:1.0\nS\t1\tACG\nS\t2\tTC\nS\t3\tGA\nS\t4\tTTA\nP\tref\t1+,2+,4+\t*\nP\ta\t1+,3+,4+\t*\n";
    if ((v = run(MNP, nullptr, 1, SR_OK, ra, nullptr))) { EXPECT(v->sites == 0 && v->skipped[1] == 1 && v->traversals == 0); sr_variants_free(v); }

    run(SNP, "nobody", 10000, SR_ERR_INVALID, ra, nullptr);
    run("S\tx\tACGT\n", nullptr, 10000, SR_ERR_INVALID, ra, nullptr);
    sr_variant_params p;
    sr_variant_params_default(&p);
    v = nullptr;
    EXPECT(sr_variants_gfa(SNP, &p, -2, &v) == SR_ERR_INVALID && v == nullptr);
    EXPECT(sr_variants_gfa(nullptr, &p, SR_VARIANTS_DEVICE_HOST, &v) == SR_ERR_INVALID);
    char *text = nullptr;
    EXPECT(sr_variants_vcf(nullptr, ra, &text) == SR_ERR_INVALID);
    sr_variants_free(nullptr);
    // sites x paths above 2^26: 2048 sites, 32771 paths of which all but two have no step
    std::string big = "H\tVN:Z:1.0\nS\t1\tA\n", ref = "P\tref\t1+", alt = "P\talt\t1+";
    for (int k = 0; k < 2048; k++) {
        const std::string r = std::to_string(3 * k + 2), a = std::to_string(3 * k + 3), s = std::to_string(3 * k + 4);
        big += "S\t" + r + "\tC\nS\t" + a + "\tG\nS\t" + s + "\tT\n";
        ref += "," + r + "+," + s + "+"; alt += "," + a + "+," + s + "+";
    }
    big += ref + "\t*\n" + alt + "\t*\n";
    for (int k = 0; k < 32769; k++) big += "P\te" + std::to_string(k) + "\t\t*\n";
    run(big.c_str(), nullptr, 10000, SR_ERR_UNSUPPORTED, nullptr, nullptr);

    if (fails) { fprintf(stderr, "variants_asan: %d check(s) failed\n", fails); return 1; }
    printf("variants_asan: ok\n");
    return 0;
}
