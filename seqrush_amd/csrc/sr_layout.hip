// sr_layout.hip -- device execution of the deterministic 2-D path-guided SGD layout (`--layout`).
// Every iteration is split into sub-rounds of terms_per_round terms.  sr_layout_terms_kernel: one lane per term (wave64,
// 256-thread workgroups); each term reads its two end points (one 16-byte load each) as the sub-round found them
// (sr_layout_term.h) and adds its four contributions as int64 fixed point plus one per end point to the 64-byte records of
// the two nodes, with no-return 64- and 32-bit integer atomics (6 per live term).  sr_layout_apply_kernel: one lane per end
// point, x += acc * 2^-20 / cnt, likewise y, then its part of the record is zeroed.  Integer sums do not depend on the
// order of the atomics, so the end points are bit-identical to the host twin's (sr_layout.cpp layout_run_host_twin).  All
// launches go to one stream with the iteration's eta and cooling flag as kernel arguments: no host synchronisation
// between iterations, no captured graph.
#include <hip/hip_runtime.h>
#include <vector>
#include "../../include/seqrush_amd.h"
#include "sr_internal.h"
#include "sr_layout.h"

static_assert(sizeof(LayoutAcc) == 64 && alignof(LayoutAcc) == 64, "one accumulator record per cache line");
static_assert(sizeof(sr_xy) == 16, "one end point per 16-byte load");

__global__ void __launch_bounds__(SR_WG) sr_layout_terms_kernel(LayoutView v, uint64_t k, uint64_t t0, uint64_t nt, double eta,
                                                                int cooling, const sr_xy *__restrict__ xy,
                                                                LayoutAcc *__restrict__ acc) {
    const uint64_t l = (uint64_t)blockIdx.x * SR_WG + threadIdx.x;
    if (l >= nt) return;
    uint32_t i, j;
    double rx, ry;
    if (!layout_term(v, k, t0 + l, eta, cooling, xy, &i, &j, &rx, &ry)) return;
    LayoutAcc *ai = &acc[i >> 1], *aj = &acc[j >> 1];
    const uint32_t ei = i & 1u, ej = j & 1u;
    atomicAdd(&ai->a[2 * ei], (unsigned long long)sgd_fix(-rx));
    atomicAdd(&ai->a[2 * ei + 1], (unsigned long long)sgd_fix(-ry));
    atomicAdd(&ai->c[ei], 1u);
    atomicAdd(&aj->a[2 * ej], (unsigned long long)sgd_fix(rx));
    atomicAdd(&aj->a[2 * ej + 1], (unsigned long long)sgd_fix(ry));
    atomicAdd(&aj->c[ej], 1u);
}

__global__ void __launch_bounds__(SR_WG) sr_layout_apply_kernel(uint64_t n_ends, sr_xy *__restrict__ xy, LayoutAcc *__restrict__ acc) {
    const uint64_t e = (uint64_t)blockIdx.x * SR_WG + threadIdx.x;
    if (e >= n_ends) return;
    LayoutAcc *a = &acc[e >> 1];
    const uint32_t end = (uint32_t)(e & 1u);
    const unsigned c = a->c[end];
    if (!c) return;
    sr_xy p = xy[e];
    p.x = sgd_apply(p.x, (int64_t)a->a[2 * end], c);
    p.y = sgd_apply(p.y, (int64_t)a->a[2 * end + 1], c);
    xy[e] = p;
    a->a[2 * end] = 0;
    a->a[2 * end + 1] = 0;
    a->c[end] = 0;
}

#define LAYCHK(expr)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) return sr_fail(SR_ERR_HIP, std::string("layout: ") + #expr + ": " + hipGetErrorString(e_)); \
    } while (0)

int srk_layout_device(const LayoutProblem &p, int device, void *stream_in, std::vector<sr_xy> &xy, float *ms) {
    xy = p.xy0;
    *ms = 0;
    if (!p.sgd.has_terms) return SR_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return sr_fail(SR_ERR_NO_DEVICE, "layout: no HIP device");
    if (device >= ndev) return sr_fail(SR_ERR_INVALID, "layout: no HIP device " + std::to_string(device));
    struct Res {                                     // released on every exit; the caller's current device comes back last
        int prev_device = -1;
        std::vector<void *> bufs;
        hipStream_t own = nullptr;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Res() {
            for (void *b : bufs) (void)hipFree(b);
            if (e0) (void)hipEventDestroy(e0);
            if (e1) (void)hipEventDestroy(e1);
            if (own) (void)hipStreamDestroy(own);
            if (prev_device >= 0) (void)hipSetDevice(prev_device);
        }
    } res;
    LAYCHK(hipGetDevice(&res.prev_device));
    LAYCHK(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream_in;
    if (!st) { LAYCHK(hipStreamCreateWithFlags(&res.own, hipStreamNonBlocking)); st = res.own; }
    LAYCHK(hipEventCreate(&res.e0));
    LAYCHK(hipEventCreate(&res.e1));
    auto up = [&](const void *src, size_t bytes, void **dst) -> int {
        void *d = nullptr;
        LAYCHK(hipMalloc(&d, bytes ? bytes : 16));
        res.bufs.push_back(d);
        if (bytes) LAYCHK(hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, st));
        *dst = d;
        return SR_OK;
    };
    const SgdProblem &s = p.sgd;
    const uint64_t N = s.n_nodes;
    LayoutView v = p.view;
    void *d;
    int r;
#define LAYUP(field, vec) \
    if ((r = up(vec.data(), vec.size() * sizeof(vec[0]), &d))) return r; \
    v.field = (decltype(v.field))d;
    LAYUP(s.step_node, s.step_node) LAYUP(s.step_path, s.step_path) LAYUP(s.step_rank, s.step_rank) LAYUP(s.step_pos, s.step_pos)
    LAYUP(s.path_first, s.path_first) LAYUP(s.path_nsteps, s.path_nsteps) LAYUP(s.zetas, s.zetas)
    LAYUP(s.prefix[0], s.prefix_theta) LAYUP(s.prefix[1], s.prefix_cool)
    LAYUP(step_rev, p.step_rev) LAYUP(node_len, p.node_len)
#undef LAYUP
    sr_xy *d_xy;
    if ((r = up(p.xy0.data(), 2 * N * sizeof(sr_xy), &d))) return r;
    d_xy = (sr_xy *)d;
    LayoutAcc *d_acc;
    LAYCHK(hipMalloc(&d, N * sizeof(LayoutAcc))); res.bufs.push_back(d); d_acc = (LayoutAcc *)d;    // hipMalloc aligns to 256 bytes
    LAYCHK(hipMemsetAsync(d_acc, 0, N * sizeof(LayoutAcc), st));
    const uint64_t M = s.min_term_updates, R = s.terms_per_round;
    const unsigned apply_blocks = (unsigned)((2 * N + SR_WG - 1) / SR_WG);
    LAYCHK(hipEventRecord(res.e0, st));
    for (uint64_t k = 0; k < s.iters; k++) {
        const double eta = s.etas[k];
        const int cooling = k > s.first_cooling;
        for (uint64_t t0 = 0; t0 < M; t0 += R) {
            const uint64_t nt = M - t0 < R ? M - t0 : R;
            hipLaunchKernelGGL(sr_layout_terms_kernel, dim3((unsigned)((nt + SR_WG - 1) / SR_WG)), dim3(SR_WG), 0, st, v, k, t0, nt, eta,
                               cooling, (const sr_xy *)d_xy, d_acc);
            hipLaunchKernelGGL(sr_layout_apply_kernel, dim3(apply_blocks), dim3(SR_WG), 0, st, 2 * N, d_xy, d_acc);
        }
    }
    LAYCHK(hipGetLastError());
    LAYCHK(hipEventRecord(res.e1, st));
    LAYCHK(hipMemcpyAsync(xy.data(), d_xy, 2 * N * sizeof(sr_xy), hipMemcpyDeviceToHost, st));
    LAYCHK(hipStreamSynchronize(st));
    LAYCHK(hipEventElapsedTime(ms, res.e0, res.e1));
    return SR_OK;
}
