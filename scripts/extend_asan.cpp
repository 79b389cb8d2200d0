// extend_asan.cpp -- the host side of --extend under AddressSanitizer and UBSan: the checks of the
// plan, the host twin of the spell and seed groups, the pair filter and the refusals, on small graphs with known answers
// (their text is here: this program reads no file).  A CPU program: it opens no device.  Built by
// `make -C seqrush_amd/csrc extend-asan`, run as seqrush_amd/extend_asan; exit status 0 and "extend_asan: ok" mean that
// every answer matched and the sanitizers reported nothing.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../include/seqrush_amd.h"

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "extend_asan: line %d: %s\n", __LINE__, #c); fails++; } } while (0)

static const char *HAIRPIN = "H\tVN:Z:1.0\nS\t1\tACGGT\nS\t2\tCATTG\nS\t3\tGA\nS\t9\t*\nL\t1\t+\t3\t+\t0M\n"
                             "P\ttwice\t1+,3+,1+\t*\nP\thairpin\t2+,3+,2-\t*\nP\tother\t1-,2+\t*\n";
static const char *LOWER = "S\t1\tacgN\nS\t2\tRY\nP\ta\t1+,2+\t*\nP\tb\t2-,1-\t*\n";

static sr_extend_plan *plan_of(const char *gfa, const sr_seqset *nw, int want, const char *word) {
    sr_extend_plan *pl = nullptr;
    const int rc = sr_extend_plan_gfa(gfa, nw, SR_EXTEND_DEVICE_HOST, &pl);
    EXPECT(rc == want);
    if (rc) {
        EXPECT(pl == nullptr);
        if (word && !strstr(sr_last_error(), word)) { fprintf(stderr, "extend_asan: '%s' not in '%s'\n", word, sr_last_error()); fails++; }
    }
    return pl;
}

// the components of the seeded forest among the 2 * total base elements
static uint64_t components(const sr_extend_plan *pl, uint64_t stats[2]) {
    const sr_seqset *m = sr_extend_plan_seqs(pl);
    const uint64_t total = m->offsets[m->n], n = 2 * total + 2;
    std::vector<uint64_t> nodes(n), lab(n);
    EXPECT(sr_uf_init_host(nodes.data(), n, total) == SR_OK);
    EXPECT(sr_extend_seed_host(pl, nodes.data(), n - 1, stats) == SR_ERR_INVALID);
    EXPECT(sr_extend_seed_host(pl, nodes.data(), n, stats) == SR_OK);
    EXPECT(sr_uf_canonical_labels_host(nodes.data(), n, lab.data()) == SR_OK);
    uint64_t c = 0;
    for (uint64_t i = 0; i < 2 * total; i++) c += lab[i] == i;
    return c;
}

int main() {
    const uint8_t nb[] = "ACGTTGCA";
    const uint64_t noff[3] = {0, 5, 8};
    const char *nn[2] = {"new1", "new2"}, *dup[2] = {"new1", "other"};
    const sr_seqset nw{2, nb, noff, nn}, nw_dup{2, nb, noff, dup};
    sr_extend_plan *pl;
    if ((pl = plan_of(HAIRPIN, &nw, SR_OK, nullptr))) {
        const sr_seqset *m = sr_extend_plan_seqs(pl);
        EXPECT(m->n == 5 && sr_extend_plan_n_old(pl) == 3 && m->offsets[3] == 34 && m->offsets[5] == 42);
        EXPECT(!memcmp(m->bases, "ACGGTGAACGGT" "CATTGGACAATG" "ACCGTCATTG" "ACGTTGCA", 42));
        EXPECT(!strcmp(m->names[0], "twice") && !strcmp(m->names[2], "other") && !strcmp(m->names[4], "new2"));
        uint64_t st[2] = {0, 0};
        // 12 distinct node offsets hold the 34 old bases; the 8 new bases stand alone
        EXPECT(components(pl, st) == 12 + 8 && st[0] == 34 - 12 && st[1] == 34 - 12);
        sr_extend_stats es;
        EXPECT(sr_extend_plan_stats(pl, &es) == SR_OK && es.old_paths == 3 && es.old_bases == 34 && es.old_steps == 8 && es.new_sequences == 2);
        const uint32_t q[6] = {0, 0, 3, 4, 2, 2}, t[6] = {0, 3, 1, 4, 2, 4}, bad[1] = {5};
        uint32_t *qo = nullptr, *to = nullptr;
        uint64_t cnt = 0;
        EXPECT(sr_extend_pair_list(pl, q, t, 6, &qo, &to, &cnt) == SR_OK && cnt == 4 && qo[0] == 0 && to[0] == 3 && qo[3] == 2 && to[3] == 4);
        sr_free(qo); sr_free(to);
        EXPECT(sr_extend_pair_list(pl, q, t, 0, &qo, &to, &cnt) == SR_OK && cnt == 0);
        sr_free(qo); sr_free(to);
        EXPECT(sr_extend_pair_list(pl, bad, t, 1, &qo, &to, &cnt) == SR_ERR_INVALID);
        sr_extend_plan_free(pl);
    }
    if ((pl = plan_of(LOWER, nullptr, SR_OK, nullptr))) {                // lower case comes back upper case on a reverse step
        const sr_seqset *m = sr_extend_plan_seqs(pl);
        EXPECT(m->n == 2 && !memcmp(m->bases, "acgNRY" "YRNCGT", 12));
        uint64_t st[2];
        EXPECT(components(pl, st) == 6 && st[0] == 6);
        sr_extend_plan_free(pl);
    }
    plan_of("S\t1\tACGT\nS\t2\tGG\nP\ta\t1+\t*\nP\ta\t2+\t*\n", &nw, SR_ERR_INVALID, "'a'");
    plan_of("S\t1\tACGT\nP\tnew2\t1+\t*\n", &nw, SR_ERR_INVALID, "'new2'");
    if ((pl = plan_of("S\t1\tACGT\nP\ta\t1+\t*\n", &nw_dup, SR_OK, nullptr))) sr_extend_plan_free(pl);
    plan_of("S\t1\tACGT\nP\tother\t1+\t*\n", &nw_dup, SR_ERR_INVALID, "'other'");
    plan_of("S\t1\tACGT\nP\ta\t1+\t*\nP\tempty\t\t*\n", &nw, SR_ERR_INVALID, "'empty'");
    plan_of("S\t1\tACGT\nP\ta\t1+,5-\t*\n", &nw, SR_ERR_INVALID, "segment 5");
    plan_of("S\t1\tACGT\nS\t2\t*\nP\ta\t1+\t*\nP\tb\t1+,2-\t*\n", &nw, SR_ERR_INVALID, "'b'");
    plan_of("S\t1\tACGT\nL\t1\t+\t1\t+\t0M\n", &nw, SR_ERR_INVALID, "no P line");
    plan_of("S\tx\tACGT\nP\ta\tx+\t*\n", &nw, SR_ERR_INVALID, "GFA line 1");
    pl = nullptr;
    EXPECT(sr_extend_plan_gfa(nullptr, &nw, SR_EXTEND_DEVICE_HOST, &pl) == SR_ERR_INVALID);
    EXPECT(sr_extend_plan_gfa(HAIRPIN, &nw, -2, &pl) == SR_ERR_INVALID && pl == nullptr);
    EXPECT(sr_extend_seed_host(nullptr, nullptr, 0, nullptr) == SR_ERR_INVALID);
    EXPECT(sr_extend_plan_seqs(nullptr) == nullptr && sr_extend_plan_n_old(nullptr) == 0);
    sr_extend_plan_free(nullptr);

    if (fails) { fprintf(stderr, "extend_asan: %d check(s) failed\n", fails); return 1; }
    printf("extend_asan: ok\n");
    return 0;
}
