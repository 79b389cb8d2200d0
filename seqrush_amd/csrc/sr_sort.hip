// sr_sort.hip -- device execution of the deterministic path-guided SGD (the Y of the Ygs layout).
// Every iteration is split into sub-rounds of terms_per_round terms.  sr_sgd_terms_kernel: one lane per term (wave64,
// 256-thread workgroups); each term reads the positions as the sub-round found them (sr_sgd_term.h) and adds its two
// contributions as int64 fixed point plus one to a per-node count, with no-return 64- and 32-bit integer atomics.
// sr_sgd_apply_kernel: x += acc * 2^-20 / cnt, then both arrays are zeroed.  Integer sums do not depend on the order
// of the atomics, so the positions are bit-identical to the host twin's (sr_sort.cpp sgd_run_host_twin).  All launches
// go to one stream with the iteration's eta and cooling flag as kernel arguments: no host synchronisation between
// iterations, no captured graph.
#include <hip/hip_runtime.h>
#include <vector>
#include "../../include/seqrush_amd.h"
#include "sr_internal.h"
#include "sr_sort.h"

__global__ void __launch_bounds__(SR_WG) sr_sgd_terms_kernel(SgdView v, uint64_t k, uint64_t t0, uint64_t nt, double eta,
                                                             int cooling, const double *__restrict__ x,
                                                             unsigned long long *__restrict__ acc, unsigned *__restrict__ cnt) {
    const uint64_t l = (uint64_t)blockIdx.x * SR_WG + threadIdx.x;
    if (l >= nt) return;
    uint32_t i, j;
    double rx;
    if (!sgd_term(v, k, t0 + l, eta, cooling, x, &i, &j, &rx)) return;
    atomicAdd(&acc[i], (unsigned long long)sgd_fix(-rx));
    atomicAdd(&acc[j], (unsigned long long)sgd_fix(rx));
    atomicAdd(&cnt[i], 1u);
    atomicAdd(&cnt[j], 1u);
}

__global__ void __launch_bounds__(SR_WG) sr_sgd_apply_kernel(uint64_t n, double *__restrict__ x, unsigned long long *__restrict__ acc,
                                                             unsigned *__restrict__ cnt) {
    const uint64_t i = (uint64_t)blockIdx.x * SR_WG + threadIdx.x;
    if (i >= n) return;
    const unsigned c = cnt[i];
    if (!c) return;
    x[i] = sgd_apply(x[i], (int64_t)acc[i], c);
    acc[i] = 0;
    cnt[i] = 0;
}

#define SGDCHK(expr)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) return sr_fail(SR_ERR_HIP, std::string("sgd: ") + #expr + ": " + hipGetErrorString(e_)); \
    } while (0)

int srk_sgd_device(const SgdProblem &p, int device, void *stream_in, std::vector<double> &x, float *ms) {
    x = p.x0;
    if (!p.has_terms) return SR_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return sr_fail(SR_ERR_NO_DEVICE, "sort: no HIP device");
    if (device >= ndev) return sr_fail(SR_ERR_INVALID, "sort: no HIP device " + std::to_string(device));
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
    SGDCHK(hipGetDevice(&res.prev_device));
    SGDCHK(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream_in;
    if (!st) { SGDCHK(hipStreamCreateWithFlags(&res.own, hipStreamNonBlocking)); st = res.own; }
    SGDCHK(hipEventCreate(&res.e0));
    SGDCHK(hipEventCreate(&res.e1));
    auto up = [&](const void *src, size_t bytes, void **dst) -> int {
        void *d = nullptr;
        SGDCHK(hipMalloc(&d, bytes ? bytes : 16));
        res.bufs.push_back(d);
        if (bytes) SGDCHK(hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, st));
        *dst = d;
        return SR_OK;
    };
    const uint64_t N = p.n_nodes;
    SgdView v = p.view;
    void *d;
    int r;
#define SGDUP(field, vec) \
    if ((r = up(p.vec.data(), p.vec.size() * sizeof(p.vec[0]), &d))) return r; \
    v.field = (decltype(v.field))d;
    SGDUP(step_node, step_node) SGDUP(step_path, step_path) SGDUP(step_rank, step_rank) SGDUP(step_pos, step_pos)
    SGDUP(path_first, path_first) SGDUP(path_nsteps, path_nsteps) SGDUP(zetas, zetas)
    SGDUP(prefix[0], prefix_theta) SGDUP(prefix[1], prefix_cool)
#undef SGDUP
    double *d_x;
    if ((r = up(p.x0.data(), N * sizeof(double), &d))) return r;
    d_x = (double *)d;
    unsigned long long *d_acc;
    unsigned *d_cnt;
    SGDCHK(hipMalloc(&d, N * sizeof(unsigned long long))); res.bufs.push_back(d); d_acc = (unsigned long long *)d;
    SGDCHK(hipMalloc(&d, N * sizeof(unsigned))); res.bufs.push_back(d); d_cnt = (unsigned *)d;
    SGDCHK(hipMemsetAsync(d_acc, 0, N * sizeof(unsigned long long), st));
    SGDCHK(hipMemsetAsync(d_cnt, 0, N * sizeof(unsigned), st));
    const uint64_t M = p.min_term_updates, R = p.terms_per_round;
    const unsigned apply_blocks = (unsigned)((N + SR_WG - 1) / SR_WG);
    SGDCHK(hipEventRecord(res.e0, st));
    for (uint64_t k = 0; k < p.iters; k++) {
        const double eta = p.etas[k];
        const int cooling = k > p.first_cooling;
        for (uint64_t t0 = 0; t0 < M; t0 += R) {
            const uint64_t nt = M - t0 < R ? M - t0 : R;
            hipLaunchKernelGGL(sr_sgd_terms_kernel, dim3((unsigned)((nt + SR_WG - 1) / SR_WG)), dim3(SR_WG), 0, st, v, k, t0, nt, eta,
                               cooling, (const double *)d_x, d_acc, d_cnt);
            hipLaunchKernelGGL(sr_sgd_apply_kernel, dim3(apply_blocks), dim3(SR_WG), 0, st, N, d_x, d_acc, d_cnt);
        }
    }
    SGDCHK(hipGetLastError());
    SGDCHK(hipEventRecord(res.e1, st));
    SGDCHK(hipMemcpyAsync(x.data(), d_x, N * sizeof(double), hipMemcpyDeviceToHost, st));
    SGDCHK(hipStreamSynchronize(st));
    SGDCHK(hipEventElapsedTime(ms, res.e0, res.e1));
    return SR_OK;
}
