// sr_variants_rule.h -- the rules of the reference-anchored variant sites (--vcf), shared by the
// kernels and the host twin of sr_variants.hip: the limits, the oriented byte of a handle, how a pair of anchor steps is
// classified, the order of the bytes of an allele and the allele hash.  Everything here is integer arithmetic, so the two
// executions agree exactly.
#pragma once
#include <cstdint>
#include "../../include/seqrush_amd.h"
#include "sr_sgd_term.h"

#define SR_VARIANTS_MAX_CELLS (1ULL << 26)     // sites x paths above this: SR_ERR_UNSUPPORTED
#define SR_VARIANTS_HARD_ALLELE 0x7fffffffULL  // an allele or a reference span beyond this is skipped whatever max_allele_len says
#define SR_VARIANTS_VARIANT_HOST 0             // sr_variants.variant: plain loops on the host
#define SR_VARIANTS_VARIANT_DEVICE 1
#define SR_VARIANTS_NONE 0xffffffffu           // no previous anchor step

// classes of a pair of neighbouring anchor steps
#define SR_VAR_BREAK 0
#define SR_VAR_ADJACENT 1
#define SR_VAR_SKIPPED 2
#define SR_VAR_TRAVERSAL 3

// the project's complement (comp_base of sr_ctx.h): lower case maps to upper case, every other byte to itself
SR_HD static inline uint8_t sr_var_comp(uint8_t b) {
    switch (b) {
    case 'A': case 'a': return 'T'; case 'T': case 't': return 'A';
    case 'C': case 'c': return 'G'; case 'G': case 'g': return 'C';
    default: return b;
    }
}

// byte k of the oriented sequence of a handle on a node of `len` bytes at `seq`
SR_HD static inline uint8_t sr_var_handle_byte(const uint8_t *seq, uint32_t len, uint32_t rev, uint32_t k) {
    return rev ? sr_var_comp(seq[len - 1 - k]) : seq[k];
}

// the pair (i, j) of anchor steps: strands si, sj; reference intervals [pi, ei) and [pj, ej) of their nodes; alen = bytes
// of the steps between them.  -> class; *a, *b set for every colinear pair
SR_HD static inline int sr_var_classify(uint32_t si, uint32_t sj, uint32_t pi, uint32_t ei, uint32_t pj, uint32_t ej, uint64_t alen,
                                        uint64_t max_allele_len, uint32_t *a, uint32_t *b) {
    if (si != sj) return SR_VAR_BREAK;
    if (si == 0) { if (pj < ei) return SR_VAR_BREAK; *a = ei; *b = pj; }
    else { if (ej > pi) return SR_VAR_BREAK; *a = ej; *b = pi; }
    if (*a == *b && alen == 0) return SR_VAR_ADJACENT;
    const uint64_t span = (uint64_t)*b - *a;
    if (span > SR_VARIANTS_HARD_ALLELE || alen > SR_VARIANTS_HARD_ALLELE) return SR_VAR_SKIPPED;
    if (max_allele_len && (span > max_allele_len || alen > max_allele_len)) return SR_VAR_SKIPPED;
    return SR_VAR_TRAVERSAL;
}

// the graph tables an allele is read from; node v = 1..V sits at index v - 1
struct SrVarGraph {
    const uint32_t *steps;                     // [S] handle = node << 1 | reverse
    const uint32_t *len;                       // [V]
    const uint64_t *seq_off;                   // [V + 1] into seq
    const uint8_t *seq;                        // the node sequences back to back
};

// the bytes of the allele of the colinear pair (i, j) of strand s, in allele order: forward strand = the oriented
// sequences of steps i + 1 .. j - 1; reverse strand = those of the flipped handles of steps j - 1 .. i + 1.  next() gives
// one byte; there are alen of them.
struct SrVarWalk {
    const SrVarGraph *g;
    uint32_t step, last, strand, k, n, rev;
    const uint8_t *seq;
    SR_HD void load() {
        const uint32_t h = g->steps[step], v = (h >> 1) - 1;
        n = g->len[v]; seq = g->seq + g->seq_off[v]; rev = (h & 1u) ^ strand; k = 0;
    }
    SR_HD SrVarWalk(const SrVarGraph *gr, uint32_t i, uint32_t j, uint32_t s) : g(gr), strand(s), k(0), n(0), rev(0), seq(nullptr) {
        step = s ? j - 1 : i + 1; last = s ? i + 1 : j - 1;
        if (j - i > 1) load();
    }
    SR_HD uint8_t next() {
        while (k == n) { step = strand ? step - 1 : step + 1; load(); }      // node lengths are >= 1; kept safe for 0
        return sr_var_handle_byte(seq, n, rev, k++);
    }
};

// 64-bit hash of an allele (FNV-1a over its bytes, then the finaliser of the SGD hash), ANDed with hash_mask by the caller
SR_HD static inline uint64_t sr_var_hash_step(uint64_t h, uint8_t b) { return (h ^ b) * 0x100000001b3ULL; }
#define SR_VAR_HASH_SEED 0xcbf29ce484222325ULL
SR_HD static inline uint64_t sr_var_hash_end(uint64_t h, uint64_t alen) { return sgd_mix(h, alen); }
