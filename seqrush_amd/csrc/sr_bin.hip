// sr_bin.hip -- path-by-bin coverage (--bin / --viz; include/seqrush_amd.h "path-by-bin coverage"):
// cov[p][b] and inv[p][b], the base pairs of bin b of the pangenome sequence that the steps (the reverse steps) of path p
// cover, on the device and, in plain loops over the same tables and the same rule header, on the host.  Every quantity is an
// integer sum, so the two agree exactly.  The TSV, the image and the PNG are formed here from the tables, once for every
// front end.
//
// Device: positions by the exclusive scan of sr_graph.hip, then one pass over the steps on one stream, hipEvents around
// the stage, one synchronisation after the download.  In a sorted graph consecutive steps of a path fall into the same or
// neighbouring bins, so a plain atomic per step would serialise the lanes of a wave on one address: runs of equal
// (path, bin) keys along the lanes are summed by shuffles first and only the first lane of a run adds.  A step over more
// than SR_BIN_LANE_SPAN bins is taken out by a ballot and walked by the whole wave, lanes strided over its bins.
// B <= SR_BIN_LDS_MAX_BINS: a workgroup works inside one path and keeps its two rows in LDS; larger B: global atomics.
// No captured graph.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/seqrush_amd.h"
#include "sr_internal.h"
#include "sr_sort.h"
#include "sr_stage_host.h"
#include "sr_stage_dev.h"
#include "sr_bin_rule.h"

#define BN_BLOCK 256
#ifndef SR_BIN_RUN_REDUCE
#define SR_BIN_RUN_REDUCE 1                // 0: one add per lane and bin, the yardstick of scripts/bin_bench.py only
#endif
#define BN_NO_KEY 0xffffffffu

typedef unsigned long long u64d;

static_assert(SR_BIN_CHUNK % BN_BLOCK == 0, "a chunk is a whole number of workgroup sweeps");
static_assert(2ull * 8 * SR_BIN_LDS_MAX_BINS <= 65536, "two u64 rows of the LDS variant fit 64 KiB");

// ------------------------------------------------------------------ device helpers
// One wave, one step per lane (valid == false: no step).  `row` is the lane's path's row offset into cov / inv: p * B
// for the global tables, 0 for the LDS rows of the one path a workgroup works in.  The key of a contribution is
// row + bin, below 2^26, so a run of equal keys never joins two paths.
__device__ __forceinline__ void bn_wave_steps(bool valid, uint32_t row, uint32_t pos, uint32_t len, bool rev, uint32_t w, u64d *cov,
                                              u64d *inv) {
    const int lane = threadIdx.x & 63;
    valid = valid && len > 0;
    const uint32_t b0 = valid ? pos / w : 0, b1 = valid ? (pos + len - 1) / w : 0, nb = b1 - b0 + 1;
    // steps over many bins: the whole wave walks each of them, lanes strided over its bins (distinct addresses)
    u64d wide = __ballot(valid && nb > SR_BIN_LANE_SPAN);
    while (wide) {
        const int k = __ffsll(wide) - 1;
        wide &= wide - 1;
        const uint32_t kpos = __shfl(pos, k, 64), klen = __shfl(len, k, 64), krow = __shfl(row, k, 64);
        const uint32_t kb0 = __shfl(b0, k, 64), kb1 = __shfl(b1, k, 64);
        const bool krev = __shfl((int)rev, k, 64) != 0;
        for (uint64_t b = (uint64_t)kb0 + lane; b <= kb1; b += 64) {
            const u64d ov = sr_bin_overlap(kpos, klen, (uint32_t)b, w);
            atomicAdd(&cov[krow + b], ov);
            if (krev) atomicAdd(&inv[krow + b], ov);
        }
    }
    // the others: pass j takes the j-th bin of every lane's step; most waves need one pass
    const bool narrow = valid && nb <= SR_BIN_LANE_SPAN;
    uint32_t passes = narrow ? nb : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const uint32_t other = __shfl_xor(passes, o, 64); passes = other > passes ? other : passes; }
    passes = __builtin_amdgcn_readfirstlane(passes);                 // the wave's maximum, in every lane: a uniform trip count
    for (uint32_t j = 0; j < passes; j++) {
        const bool on = narrow && j < nb;
        const uint32_t key = on ? row + b0 + j : BN_NO_KEY;
        u64d c = on ? sr_bin_overlap(pos, len, b0 + j, w) : 0, r = rev ? c : 0;
        bool head = true;
#if SR_BIN_RUN_REDUCE
        // a run = a maximal stretch of lanes with one key; n = lanes from this one to the end of its run.  After the
        // round with offset o a lane holds the sum of the first min(2 o, n) lanes of the rest of its run.
        const uint32_t prev = __shfl_up(key, 1, 64);
        head = lane == 0 || prev != key;
        const u64d heads = __ballot(head);                           // every lane votes: not inside a conditional
        const u64d rest = (heads >> 1) >> lane;                      // the heads after this lane
        const int n = rest ? __ffsll(rest) : 64 - lane;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const u64d oc = __shfl_down(c, o, 64), orv = __shfl_down(r, o, 64);
            if (o < n) { c += oc; r += orv; }
        }
#endif
        if (head && key != BN_NO_KEY) {
            atomicAdd(&cov[key], c);
            if (r) atomicAdd(&inv[key], r);
        }
    }
}

// ------------------------------------------------------------------ B <= SR_BIN_LDS_MAX_BINS
// work item i = SR_BIN_CHUNK consecutive steps of path item_path[i] from step item_first[i].  Dynamic LDS: the path's cov
// row, then its inv row, B u64 each (u64: a bin of a chunk can receive SR_BIN_CHUNK x bin_width base pairs, which passes
// 2^32 from a width of 2^20).  The non-zero bins are flushed with one global add each.
__global__ void __launch_bounds__(BN_BLOCK) bn_steps_lds_kernel(const uint32_t *steps, const uint32_t *path_off, const uint32_t *item_path,
                                                                const uint32_t *item_first, const uint32_t *len, const uint32_t *pos,
                                                                uint32_t w, uint32_t B, u64d *cov, u64d *inv) {
    extern __shared__ u64d bn_lds[];
    u64d *lcov = bn_lds, *linv = bn_lds + B;
    for (uint32_t i = threadIdx.x; i < 2 * B; i += BN_BLOCK) bn_lds[i] = 0;
    __syncthreads();
    const uint32_t p = item_path[blockIdx.x], s0 = item_first[blockIdx.x];
    const uint32_t pend = path_off[p + 1], s1 = pend - s0 > SR_BIN_CHUNK ? s0 + SR_BIN_CHUNK : pend;
    for (uint32_t base = s0; base < s1; base += BN_BLOCK) {          // block-uniform: every wave makes every sweep
        const uint32_t s = base + threadIdx.x;
        const bool valid = s < s1;
        const uint32_t h = valid ? steps[s] : 0, node = h >> 1;
        bn_wave_steps(valid, 0, valid ? pos[node] : 0, valid ? len[node] : 0, h & 1u, w, lcov, linv);
    }
    __syncthreads();
    const uint64_t row = (uint64_t)p * B;
    for (uint32_t b = threadIdx.x; b < B; b += BN_BLOCK) {
        const u64d c = lcov[b], r = linv[b];
        if (c) atomicAdd(&cov[row + b], c);
        if (r) atomicAdd(&inv[row + b], r);
    }
}

// ------------------------------------------------------------------ larger B
__global__ void __launch_bounds__(BN_BLOCK) bn_steps_global_kernel(const uint32_t *steps, uint32_t S, const uint32_t *path_off, uint32_t np,
                                                                   const uint32_t *len, const uint32_t *pos, uint32_t w, uint32_t B,
                                                                   u64d *cov, u64d *inv) {
    const uint64_t s = (uint64_t)blockIdx.x * BN_BLOCK + threadIdx.x;
    const bool valid = s < S;
    uint32_t h = 0, row = 0;
    if (valid) { h = steps[s]; row = sr_path_of(path_off, np, (uint32_t)s) * B; }
    const uint32_t node = h >> 1;
    bn_wave_steps(valid, row, valid ? pos[node] : 0, valid ? len[node] : 0, h & 1u, w, cov, inv);
}

namespace {

// the tables both executions read: node v = 1..V at index v, slot 0 unused (length 0)
struct BnTables : SrPathTables {
    uint32_t w32 = 1;
    uint64_t L = 0, w = 1, B = 0;
};

int bn_tables(const SrGraph &g, const sr_bin_params &prm, BnTables &t) {
    if ((prm.bin_width != 0) == (prm.bins != 0)) return sr_fail(SR_ERR_INVALID, "bins: give exactly one of bin_width and bins");
    const SrPathSizes z = sr_path_sizes(g);
    const uint64_t np = z.paths, bases = z.bases;
    if (z.nodes >= 0x3fffffffULL || z.steps >= 0x7fffffffULL || np >= 0x7fffffffULL || bases >= 0x7fffffffULL)
        return sr_fail(SR_ERR_UNSUPPORTED, "bins supports < 2^30 nodes and < 2^31 steps, paths and bases");
    t.L = bases;
    t.w = prm.bin_width ? prm.bin_width : sr_bin_width_of(bases, prm.bins);
    t.w32 = sr_bin_width32(t.w);
    t.B = t.w >= bases ? (bases ? 1 : 0) : sr_bin_count_of(bases, t.w);
    if (np * t.B > SR_BIN_MAX_CELLS)
        return sr_fail(SR_ERR_UNSUPPORTED, "bins: " + std::to_string(np) + " paths x " + std::to_string(t.B) + " bins; the tables support at most 2^26 cells");
    return sr_path_tables_fill(g, z, "bins", false, true, t);
}

sr_path_bins *bn_result(const BnTables &t) {
    sr_path_bins *r = (sr_path_bins *)calloc(1, sizeof(sr_path_bins));
    if (!r) return nullptr;
    r->length = t.L; r->paths = t.P; r->bins = t.B; r->bin_width = t.w;
    const uint64_t cells = (uint64_t)t.P * t.B;
    r->cov = (uint64_t *)calloc(cells ? cells : 1, 8); r->inv = (uint64_t *)calloc(cells ? cells : 1, 8);
    if (!r->cov || !r->inv) { sr_path_bins_free(r); return nullptr; }
    return r;
}

// ------------------------------------------------------------------ host twin: plain loops in table order
void bn_run_host(const BnTables &t, sr_path_bins *r) {
    auto t0 = std::chrono::steady_clock::now();
    const auto t_all = t0;
    std::vector<uint32_t> pos((uint64_t)t.V + 1, 0);
    for (uint32_t v = 1; v <= t.V; v++) pos[v] = pos[v - 1] + t.len[v - 1];
    r->kernel_us[0] = (uint64_t)(us_since(t0) + 0.5);
    t0 = std::chrono::steady_clock::now();
    const uint32_t w = t.w32;
    for (uint32_t p = 0; p < t.P; p++) {
        uint64_t *cov = r->cov + (uint64_t)p * t.B, *inv = r->inv + (uint64_t)p * t.B;
        for (uint32_t s = t.path_off[p]; s < t.path_off[p + 1]; s++) {
            const uint32_t h = t.steps[s], a = pos[h >> 1], l = t.len[h >> 1];
            if (!l) continue;
            for (uint32_t b = a / w; b <= (a + l - 1) / w; b++) {
                const uint32_t ov = sr_bin_overlap(a, l, b, w);
                cov[b] += ov;
                if (h & 1u) inv[b] += ov;
            }
        }
    }
    r->kernel_us[1] = (uint64_t)(us_since(t0) + 0.5);
    r->bin_us = (uint64_t)(us_since(t_all) + 0.5);
}

// ------------------------------------------------------------------ device execution
int bn_run_device(const BnTables &t, int device, void *stream, sr_path_bins *r) {
    const uint32_t V = t.V, S = t.S, P = t.P, B = (uint32_t)t.B;   // P x B <= 2^26 and P >= 1 where it matters: B fits
    SrStage x("bins", "the bin tables");
    if (x.open(device, stream, 4)) return x.err;
    const uint64_t cells = (uint64_t)P * B;
    if (!cells || !S) return SR_OK;                                  // no path, no bin or no step: the tables stay zero
    // the work items of the LDS variant: every path cut into chunks of SR_BIN_CHUNK steps
    const bool lds = B <= SR_BIN_LDS_MAX_BINS;
    std::vector<uint32_t> item_path, item_first;
    if (lds)
        for (uint32_t p = 0; p < P; p++)
            for (uint64_t s = t.path_off[p]; s < t.path_off[p + 1]; s += SR_BIN_CHUNK) { item_path.push_back(p); item_first.push_back((uint32_t)s); }

    const uint64_t nv = (uint64_t)V + 1;
    uint32_t *d_len = x.alloc<uint32_t>(nv), *d_pos = x.alloc<uint32_t>(nv, 0), *d_steps = x.alloc<uint32_t>(S);
    uint32_t *d_poff = x.alloc<uint32_t>((uint64_t)P + 1);
    uint32_t *d_tile = x.alloc<uint32_t>(nv / 1024 + 2), *d_grand = x.alloc<uint32_t>(1, 0);
    uint32_t *d_ipath = x.alloc<uint32_t>(item_path.size()), *d_ifirst = x.alloc<uint32_t>(item_first.size());
    u64d *d_cov = x.alloc<u64d>(cells, 0), *d_inv = x.alloc<u64d>(cells, 0);
    if (x.err) return x.err;
    x.put(d_len, t.len.data(), nv * 4); x.put(d_steps, t.steps.data(), (size_t)S * 4); x.put(d_poff, t.path_off.data(), ((size_t)P + 1) * 4);
    x.put(d_ipath, item_path.data(), item_path.size() * 4); x.put(d_ifirst, item_first.data(), item_first.size() * 4);

    x.mark(0);
    if (!x.err && srk_scan_u32(d_len, nv, d_pos, d_tile, d_grand, x.st)) x.chk(hipErrorLaunchFailure);
    x.mark(1);
    if (!x.err) {
        if (lds)
            hipLaunchKernelGGL(bn_steps_lds_kernel, dim3((unsigned)item_path.size()), dim3(BN_BLOCK), (size_t)B * 16, x.st, d_steps, d_poff, d_ipath,
                               d_ifirst, d_len, d_pos, t.w32, B, d_cov, d_inv);
        else
            hipLaunchKernelGGL(bn_steps_global_kernel, dim3((unsigned)(((uint64_t)S + BN_BLOCK - 1) / BN_BLOCK)), dim3(BN_BLOCK), 0, x.st, d_steps, S,
                               d_poff, P, d_len, d_pos, t.w32, B, d_cov, d_inv);
    }
    x.mark(2);
    x.chk(hipGetLastError());
    x.get(r->cov, d_cov, (size_t)cells * 8); x.get(r->inv, d_inv, (size_t)cells * 8);
    x.mark(3);
    x.sync();                                        // the one synchronisation
    if (x.err) return x.err;
    r->bin_us = x.us(0, 3);
    for (int k = 0; k < 3; k++) r->kernel_us[k] = x.us(k, k + 1);
    return x.err;
}

// ------------------------------------------------------------------ outputs
std::string name_of(const char *const *names, uint64_t p) { return names && names[p] ? std::string(names[p]) : u64s(p); }

int viz_check(const sr_path_bins *b, const sr_viz_params &v, uint64_t *width, uint64_t *height) {
    if (v.mode != SR_VIZ_MODE_PATH && v.mode != SR_VIZ_MODE_STRAND && v.mode != SR_VIZ_MODE_DEPTH) return sr_fail(SR_ERR_INVALID, "viz: mode must be path, strand or depth");
    if (v.path_height == 0) return sr_fail(SR_ERR_INVALID, "viz: path_height must be at least 1");
    if (v.mode == SR_VIZ_MODE_DEPTH && v.depth_max == 0) return sr_fail(SR_ERR_INVALID, "viz: depth_max must be at least 1");
    *width = b->bins;
    *height = b->paths ? b->paths * v.path_height + (b->paths - 1) * v.path_gap : 0;
    if (*width > 0xffffffffULL || *height > 0xffffffffULL || (*width && *height > SR_BIN_MAX_PIXEL_BYTES / 3 / *width))
        return sr_fail(SR_ERR_UNSUPPORTED, "viz: an image of " + u64s(*width) + " x " + u64s(*height) + " pixels is above 2^30 bytes");
    return SR_OK;
}

uint32_t crc32_of(const uint8_t *d, size_t n, uint32_t crc = 0) {
    struct Tab {
        uint32_t t[256];
        Tab() {
            for (uint32_t i = 0; i < 256; i++) {
                uint32_t c = i;
                for (int k = 0; k < 8; k++) c = c & 1 ? 0xedb88320u ^ (c >> 1) : c >> 1;
                t[i] = c;
            }
        }
    };
    static const Tab tab;
    crc = ~crc;
    for (size_t i = 0; i < n; i++) crc = tab.t[(crc ^ d[i]) & 0xff] ^ (crc >> 8);
    return ~crc;
}
void be32(std::vector<uint8_t> &o, uint32_t v) { for (int s = 24; s >= 0; s -= 8) o.push_back((uint8_t)(v >> s)); }
void png_chunk(std::vector<uint8_t> &o, const char *type, const std::vector<uint8_t> &data) {
    be32(o, (uint32_t)data.size());
    const size_t at = o.size();
    o.insert(o.end(), type, type + 4);
    o.insert(o.end(), data.begin(), data.end());
    be32(o, crc32_of(o.data() + at, o.size() - at));
}

}   // namespace

int sr_graph_bins_run(const SrGraph &g, const sr_bin_params &prm, int device, void *stream, sr_path_bins **out) {
    if (!out) return sr_fail(SR_ERR_INVALID, "null argument");
    *out = nullptr;
    if (device < SR_BIN_DEVICE_HOST) return sr_fail(SR_ERR_INVALID, "bins: device must be >= -1");
    BnTables t;
    int r = bn_tables(g, prm, t);
    if (r) return r;
    sr_path_bins *res = bn_result(t);
    if (!res) return sr_fail(SR_ERR_NOMEM, "not enough memory for the bin tables");
    if (device < 0) bn_run_host(t, res);
    else if ((r = bn_run_device(t, device, stream, res))) { sr_path_bins_free(res); return r; }
    *out = res;
    return SR_OK;
}

extern "C" int sr_path_bins_gfa(const char *gfa_in, const sr_bin_params *p, int device, sr_path_bins **out) {
    if (!gfa_in || !p || !out) return sr_fail(SR_ERR_INVALID, "null argument");
    SrGraph g;
    std::vector<std::string> names;
    int r = sr_graph_parse_gfa(gfa_in, g, names);
    if (r) return r;
    return sr_graph_bins_run(g, *p, device, nullptr, out);
}

extern "C" void sr_path_bins_free(sr_path_bins *b) {
    if (!b) return;
    free(b->cov); free(b->inv);
    free(b);
}

extern "C" int sr_path_bins_tsv(const sr_path_bins *b, const char *const *names, char **text) {
    if (!b || !text) return sr_fail(SR_ERR_INVALID, "null argument");
    std::string o = "#seqrush_amd path bins v1\tbin_width=" + u64s(b->bin_width) + "\tbins=" + u64s(b->bins) + "\tlength=" + u64s(b->length) +
                    "\tpaths=" + u64s(b->paths) + "\n";
    o += "path\tbin\tcov_bp\tinv_bp\tmean_cov\tmean_inv\n";
    char buf[96];
    for (uint64_t p = 0; p < b->paths; p++) {
        const std::string name = name_of(names, p);
        for (uint64_t k = 0; k < b->bins; k++) {
            const uint64_t c = b->cov[p * b->bins + k], v = b->inv[p * b->bins + k];
            if (!c) continue;
            snprintf(buf, sizeof buf, "\t%llu\t%llu\t%llu\t%.6f\t%.6f\n", (unsigned long long)(k + 1), (unsigned long long)c, (unsigned long long)v,
                     (double)c / (double)sr_bin_len(k, b->bin_width, b->length), (double)v / (double)c);
            o += name;
            o += buf;
        }
    }
    return sr_give_text(o, text, "not enough memory for the bin table text");
}

extern "C" void sr_viz_params_default(sr_viz_params *p) {
    if (!p) return;
    p->mode = SR_VIZ_MODE_PATH; p->path_height = 10; p->path_gap = 1; p->depth_max = 4;
}

extern "C" int sr_path_bins_rgb(const sr_path_bins *b, const char *const *names, const sr_viz_params *p, uint8_t **rgb, uint32_t *width,
                                uint32_t *height) {
    if (!b || !rgb || !width || !height) return sr_fail(SR_ERR_INVALID, "null argument");
    sr_viz_params v;
    sr_viz_params_default(&v);
    if (p) v = *p;
    uint64_t W = 0, H = 0;
    int r = viz_check(b, v, &W, &H);
    if (r) return r;
    const size_t bytes = (size_t)(W * H * 3);
    uint8_t *img = (uint8_t *)malloc(bytes ? bytes : 1);
    if (!img) return sr_fail(SR_ERR_NOMEM, "not enough memory for the image");
    memset(img, 255, bytes);
    for (uint64_t pth = 0; pth < b->paths && W; pth++) {
        uint8_t base[3];
        sr_bin_base_colour(sr_bin_name_hash(name_of(names, pth).c_str()), base);
        uint8_t *row0 = img + pth * ((uint64_t)v.path_height + v.path_gap) * W * 3;
        for (uint64_t k = 0; k < W; k++)
            sr_bin_pixel(v.mode, b->cov[pth * W + k], b->inv[pth * W + k], sr_bin_len(k, b->bin_width, b->length), v.depth_max, base, row0 + k * 3);
        for (uint32_t y = 1; y < v.path_height; y++) memcpy(row0 + (uint64_t)y * W * 3, row0, (size_t)W * 3);
    }
    *rgb = img; *width = (uint32_t)W; *height = (uint32_t)H;
    return SR_OK;
}

extern "C" int sr_path_bins_png(const sr_path_bins *b, const char *const *names, const sr_viz_params *p, uint8_t **png, uint64_t *size) {
    if (!b || !png || !size) return sr_fail(SR_ERR_INVALID, "null argument");
    uint8_t *rgb = nullptr;
    uint32_t W = 0, H = 0;
    int r = sr_path_bins_rgb(b, names, p, &rgb, &W, &H);
    if (r) return r;
    if (!W || !H) { free(rgb); return sr_fail(SR_ERR_INVALID, "viz: nothing to draw (no path or no bin)"); }
    // the raw stream: a filter byte 0 before every row; zlib: header, stored blocks of at most 65535 bytes, Adler-32
    const size_t stride = (size_t)W * 3, raw = (stride + 1) * H;
    std::vector<uint8_t> z;
    z.reserve(raw + raw / 65535 * 5 + 16);
    z.push_back(0x78); z.push_back(0x01);
    uint32_t a1 = 1, a2 = 0;
    size_t in_block = 0, left = raw;
    auto emit = [&](const uint8_t *d, size_t n) {
        while (n) {
            if (!in_block) {
                in_block = left < 65535 ? left : 65535;
                z.push_back(in_block == left ? 1 : 0);
                z.push_back((uint8_t)in_block); z.push_back((uint8_t)(in_block >> 8));
                z.push_back((uint8_t)~in_block); z.push_back((uint8_t)(~in_block >> 8));
            }
            const size_t m = n < in_block ? n : in_block;
            z.insert(z.end(), d, d + m);
            for (size_t i = 0; i < m; i++) { a1 += d[i]; if (a1 >= 65521) a1 -= 65521; a2 += a1; if (a2 >= 65521) a2 -= 65521; }
            d += m; n -= m; in_block -= m; left -= m;
        }
    };
    const uint8_t zero = 0;
    for (uint32_t y = 0; y < H; y++) { emit(&zero, 1); emit(rgb + (size_t)y * stride, stride); }
    free(rgb);
    be32(z, (a2 << 16) | a1);
    std::vector<uint8_t> o = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'}, hdr;
    be32(hdr, W); be32(hdr, H);
    hdr.push_back(8); hdr.push_back(2); hdr.push_back(0); hdr.push_back(0); hdr.push_back(0);   // 8 bits, RGB, deflate, filter method 0, no interlace
    png_chunk(o, "IHDR", hdr);
    png_chunk(o, "IDAT", z);
    png_chunk(o, "IEND", {});
    uint8_t *res = (uint8_t *)malloc(o.size());
    if (!res) return sr_fail(SR_ERR_NOMEM, "not enough memory for the PNG");
    memcpy(res, o.data(), o.size());
    *png = res; *size = o.size();
    return SR_OK;
}
