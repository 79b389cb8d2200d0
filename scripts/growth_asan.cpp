// growth_asan.cpp -- the host side of the growth curves under AddressSanitizer and UBSan: the host
// twin, sr_growth_groups, sr_growth_expected, sr_growth_fit and sr_growth_report on the known-answer graphs of
// tests/golden/stats_known_answers.json (their text is repeated here: this program reads no file) and on the refusals.
// A CPU program: it opens no device.  Built by `make -C seqrush_amd/csrc growth-asan`, run as seqrush_amd/growth_asan;
// exit status 0 and "growth_asan: ok" mean that every answer matched and the sanitizers reported nothing.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../include/seqrush_amd.h"

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "growth_asan: line %d: %s\n", __LINE__, #c); fails++; } } while (0)

static const char *CHAIN = "H\tVN:Z:1.0\nS\t1\tACG\nS\t2\tT\nS\t3\tGG\nL\t1\t+\t2\t+\t0M\nL\t2\t+\t3\t-\t0M\nP\ta\t1+,2+,3-\t*\nP\tb\t1+,3+\t*\n";
static const char *THREE = "H\tVN:Z:1.0\nS\t1\tAAAA\nS\t2\tCC\nS\t3\tG\nS\t4\tTTT\nL\t1\t+\t2\t+\t0M\nL\t2\t+\t3\t+\t0M\nL\t3\t+\t4\t+\t0M\nL\t1\t+\t3\t+\t0M\n"
                           "L\t4\t+\t1\t+\t0M\nL\t1\t+\t2\t-\t0M\nP\tx\t1+,2+,3+,4+\t*\nP\ty\t1+,3+,4+\t*\nP\tz\t4+,1+,2-\t*\n";
static const char *LOOPS = "H\tVN:Z:1.0\nS\t1\tA\nS\t2\tCC\nS\t3\tGGG\nS\t4\tT\nS\t5\tAC\nS\t6\tG\nL\t1\t+\t1\t+\t0M\nL\t1\t+\t2\t+\t0M\nL\t3\t+\t3\t-\t0M\n"
                           "L\t1\t+\t2\t+\t0M\nL\t4\t-\t5\t+\t0M\nP\tp\t1+,1+,2+\t*\nP\tq\t3+,3-\t*\nP\tr\t4-,5+\t*\nP\ts\t2-\t*\n";
static const char *EMPTY = "H\tVN:Z:1.0\n";

static sr_growth *run(const char *gfa, const uint32_t *group_of, uint32_t G, uint64_t perms, int want) {
    sr_growth_params p;
    sr_growth_params_default(&p);
    EXPECT(p.seed == 9399220 && p.permutations == 1000);
    p.permutations = perms;
    sr_growth *g = nullptr;
    const int rc = sr_growth_gfa(gfa, group_of, G, &p, SR_GROWTH_DEVICE_HOST, &g);
    EXPECT(rc == want);
    if (rc) { EXPECT(g == nullptr && strlen(sr_last_error()) > 0); return nullptr; }
    char *text = nullptr;
    EXPECT(sr_growth_report(g, &text) == SR_OK && text && strstr(text, "#seqrush_amd growth v1\t") == text);
    sr_free(text);
    std::vector<double> pe(g->groups + 1), ce(g->groups + 1);
    EXPECT(sr_growth_expected(g->bp_by_groups, (uint32_t)g->groups, pe.data(), ce.data()) == SR_OK);
    double alpha = 0, kappa = 0;
    uint32_t points = 0;
    EXPECT(sr_growth_fit(pe.data(), (uint32_t)g->groups, &alpha, &kappa, &points) == SR_OK);
    return g;
}

int main() {
    sr_growth *g = run(CHAIN, nullptr, 0, 1000, SR_OK);
    if (g) {
        EXPECT(g->groups == 2 && g->permutations == 2 && g->exhaustive == 1 && g->variant == 0);
        const uint64_t pan[4] = {6, 6, 5, 6}, core[4] = {6, 5, 5, 5};
        EXPECT(!memcmp(g->pan, pan, sizeof pan) && !memcmp(g->core, core, sizeof core));
        sr_growth_free(g);
    }
    if ((g = run(THREE, nullptr, 0, 1000, SR_OK))) {
        EXPECT(g->groups == 3 && g->permutations == 6 && g->length == 10);
        const uint64_t pan0[3] = {10, 10, 10}, core0[3] = {10, 8, 7}, bp[4] = {0, 0, 3, 7};
        EXPECT(!memcmp(g->pan, pan0, sizeof pan0) && !memcmp(g->core, core0, sizeof core0) && !memcmp(g->bp_by_groups, bp, sizeof bp));
        sr_growth_free(g);
    }
    if ((g = run(THREE, nullptr, 0, 5, SR_OK))) {                // 3! > 5: sampled
        EXPECT(g->exhaustive == 0 && g->permutations == 5);
        sr_growth_free(g);
    }
    const uint32_t two[3] = {0, 0, 1}, bad[3] = {0, 3, 1}, hole[3] = {0, 2, 2};
    if ((g = run(THREE, two, 2, 1000, SR_OK))) {
        const uint64_t pan[4] = {10, 10, 9, 10}, core[4] = {10, 9, 9, 9};
        EXPECT(g->groups == 2 && !memcmp(g->pan, pan, sizeof pan) && !memcmp(g->core, core, sizeof core));
        sr_growth_free(g);
    }
    if ((g = run(LOOPS, nullptr, 0, 1000, SR_OK))) {
        const uint64_t bp[5] = {1, 7, 2, 0, 0}, pan0[4] = {3, 6, 9, 9}, core0[4] = {3, 0, 0, 0};
        EXPECT(g->groups == 4 && g->permutations == 24 && !memcmp(g->bp_by_groups, bp, sizeof bp));
        EXPECT(!memcmp(g->pan, pan0, sizeof pan0) && !memcmp(g->core, core0, sizeof core0));
        sr_growth_free(g);
    }
    if ((g = run(EMPTY, nullptr, 0, 1000, SR_OK))) {
        EXPECT(g->groups == 0 && g->permutations == 0 && g->bp_by_groups[0] == 0);
        sr_growth_free(g);
    }
    run(THREE, bad, 3, 10, SR_ERR_INVALID);
    run(THREE, hole, 3, 10, SR_ERR_INVALID);
    run(THREE, nullptr, 0, 0, SR_ERR_INVALID);
    run(THREE, nullptr, 0, (1ULL << 24) / 3 + 1, SR_ERR_UNSUPPORTED);

    const char *names[6] = {"a#1#c1", "a#2#c1", "b#1#x", "plain", "a#1#c2", "plain#"};
    const uint32_t want[3][6] = {{0, 1, 2, 3, 4, 5}, {0, 0, 1, 2, 0, 2}, {0, 1, 2, 3, 0, 4}};
    const uint32_t count[3] = {6, 3, 5};
    for (int mode = 0; mode < 3; mode++) {
        uint32_t group_of[6], n = 0;
        char **gn = nullptr;
        EXPECT(sr_growth_groups(names, 6, mode, group_of, &n, &gn) == SR_OK && n == count[mode] && !memcmp(group_of, want[mode], sizeof group_of));
        if (gn) EXPECT(!strcmp(gn[0], mode == 0 ? "a#1#c1" : mode == 1 ? "a" : "a#1") && !strcmp(gn[n - 1], mode == 0 ? "plain#" : mode == 1 ? "plain" : "plain#"));
        sr_free(gn);
        EXPECT(sr_growth_groups(names, 6, mode, group_of, &n, nullptr) == SR_OK);
    }
    uint32_t n = 7;
    char **gn = nullptr;
    uint32_t none[1];
    EXPECT(sr_growth_groups(nullptr, 0, 1, none, &n, &gn) == SR_OK && n == 0);
    sr_free(gn);
    EXPECT(sr_growth_groups(names, 6, 3, none, &n, nullptr) == SR_ERR_INVALID);

    std::vector<double> law(60);                                 // new(k) = 1000 k^-0.5
    double acc = 0;
    for (int k = 1; k <= 60; k++) { double r = 1.0; for (int i = 0; i < 30; i++) r = 0.5 * (r + k / r); acc += 1000.0 / r; law[k - 1] = acc; }
    double alpha = 0, kappa = 0;
    uint32_t points = 0;
    EXPECT(sr_growth_fit(law.data(), 60, &alpha, &kappa, &points) == SR_OK && points == 59 && alpha > 0.5 - 1e-9 && alpha < 0.5 + 1e-9);
    EXPECT(sr_growth_fit(law.data(), 1, &alpha, &kappa, &points) == SR_OK && points == 0);
    EXPECT(sr_growth_fit(nullptr, 0, &alpha, &kappa, &points) == SR_OK && points == 0);

    if (fails) { fprintf(stderr, "growth_asan: %d check(s) failed\n", fails); return 1; }
    printf("growth_asan: ok\n");
    return 0;
}
