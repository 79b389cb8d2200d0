// sr_bin_rule.h -- the rules of the path-by-bin tables and of the image drawn from them (--bin / --viz; DESIGN.md
// section 13), shared by the kernels and the host twin of sr_bin.hip.  Everything here is integer arithmetic, so the
// two executions agree bit for bit.
#pragma once
#include <cstdint>
#include "../../include/seqrush_amd.h"
#include "sr_sgd_term.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SR_BIN_HD __host__ __device__
#else
#define SR_BIN_HD
#endif

#define SR_BIN_MAX_CELLS (1ULL << 26)      // P x B: two u64 tables of 512 MiB each
#define SR_BIN_MAX_PIXEL_BYTES (1ULL << 30)
#define SR_BIN_LDS_MAX_BINS 4096u          // B <= this: a workgroup keeps one path's two rows in LDS (2 x 8 B x B <= 64 KiB);
                                           // above it: global atomics after the same wave reduction
#define SR_BIN_CHUNK 4096u                 // steps of one path per workgroup in the LDS variant
#define SR_BIN_LANE_SPAN 4u                // a step over more bins than this is walked by the whole wave, lanes over bins

// the bin width of a request for n bins, and the number of bins of a width
SR_BIN_HD inline uint64_t sr_bin_width_of(uint64_t L, uint64_t n) { return L == 0 || n >= L ? 1 : (L + n - 1) / n; }
SR_BIN_HD inline uint64_t sr_bin_count_of(uint64_t L, uint64_t w) { return (L + w - 1) / w; }
SR_BIN_HD inline uint64_t sr_bin_len(uint64_t b, uint64_t w, uint64_t L) { return ((b + 1) * w < L ? (b + 1) * w : L) - b * w; }
// positions are below 2^31 (the parser's limit), so a width of 2^31 stands for every wider one: one bin either way
SR_BIN_HD inline uint32_t sr_bin_width32(uint64_t w) { return w > 0x80000000ULL ? 0x80000000u : (uint32_t)w; }
// base pairs of [pos, pos + len) inside bin b; the caller passes only bins the step touches ((b + 1) w <= pos + w < 2^32)
SR_BIN_HD inline uint32_t sr_bin_overlap(uint32_t pos, uint32_t len, uint32_t b, uint32_t w) {
    const uint32_t lo = b * w > pos ? b * w : pos, e = pos + len, hi = (b + 1) * w < e ? (b + 1) * w : e;
    return hi - lo;
}

// ------------------------------------------------------------------ image
inline uint64_t sr_bin_name_hash(const char *s) {    // 64-bit FNV-1a, finalised by the splitmix64 of sr_sgd_term.h
    uint64_t h = 0xcbf29ce484222325ULL;
    for (; *s; s++) { h ^= (uint8_t)*s; h *= 0x100000001b3ULL; }
    return sgd_mix(h, 0);
}
inline void sr_bin_base_colour(uint64_t z, uint8_t base[3]) {
    for (int i = 0; i < 3; i++) base[i] = (uint8_t)(32 + ((((z >> (8 * i)) & 0xff) * 3) >> 2));     // 32 .. 223
}
inline void sr_bin_pixel(int mode, uint64_t cov, uint64_t inv, uint64_t bin_len, uint64_t depth_max, const uint8_t base[3],
                         uint8_t out[3]) {
    if (cov == 0) { out[0] = out[1] = out[2] = 255; return; }
    if (mode == SR_VIZ_MODE_STRAND) {
        const bool red = 2 * inv > cov;
        out[0] = red ? 255 : 0; out[1] = out[2] = 0;
    } else if (mode == SR_VIZ_MODE_DEPTH) {
        const uint64_t d = cov * 255 / (bin_len * depth_max);
        out[0] = out[1] = out[2] = (uint8_t)(255 - (d < 255 ? d : 255));
    } else {
        const uint64_t a = cov < bin_len ? cov : bin_len;
        for (int i = 0; i < 3; i++) out[i] = (uint8_t)(255 - (255 - (uint64_t)base[i]) * a / bin_len);
    }
}
