// sr_stage_dev.h -- the device side every graph stage shares (DESIGN.md "What a graph stage gets for free"), for .hip
// files only: the stream and arena of a stage's device execution, the path of a step, the step lengths and the inclusive
// u64 scan.  Header only, and every __global__ function is a template: the stages are separate translation units of one
// shared object, and a stage's .hip file is also compiled alone (the *-asan programs, the yardstick builds of the Makefile).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include <vector>
#include "../../include/seqrush_amd.h"
#include "sr_sort.h"

#define SR_STAGE_BLOCK 256
#define SR_STAGE_WAVES (SR_STAGE_BLOCK / 64)
#define SR_STAGE_MAX_EVENTS 8

// ------------------------------------------------------------------ the stream and the arena
// One per device execution of a stage.  Every call after the first failure is skipped and `err` keeps the first status;
// sr_last_error() then reads "<prefix>: <what HIP said>".  The destructor waits for the stream, frees every buffer, destroys
// the events and a stream of its own, and puts the caller's device back.
struct SrStage {
    const char *prefix, *noun;                       // "lift", "the lift tables" (of the out-of-memory message)
    hipStream_t st = nullptr;
    bool own_stream = false;
    int prev_device = -1;
    std::vector<void *> bufs;
    hipEvent_t ev[SR_STAGE_MAX_EVENTS] = {};
    int err = 0;
    SrStage(const char *prefix_, const char *noun_) : prefix(prefix_), noun(noun_) {}
    SrStage(const SrStage &) = delete;
    SrStage &operator=(const SrStage &) = delete;
    void chk(hipError_t e) { if (e != hipSuccess && !err) { err = SR_ERR_HIP; sr_fail(SR_ERR_HIP, std::string(prefix) + ": " + hipGetErrorString(e)); } }
    // the device is there, becomes the current one, `stream` is adopted (null: a stream of the stage's own) and exactly
    // n_events <= SR_STAGE_MAX_EVENTS events exist for mark(); -> err
    int open(int device, void *stream, int n_events) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
            return err = sr_fail(SR_ERR_NO_DEVICE, std::string(prefix) + ": no HIP device (device -1 selects the host twin)");
        if (device >= ndev) return err = sr_fail(SR_ERR_INVALID, std::string(prefix) + ": no HIP device " + std::to_string(device));
        chk(hipGetDevice(&prev_device));
        chk(hipSetDevice(device));
        st = (hipStream_t)stream;
        if (!st && !err) { chk(hipStreamCreateWithFlags(&st, hipStreamNonBlocking)); own_stream = !err; }
        for (int i = 0; i < n_events && i < SR_STAGE_MAX_EVENTS; i++) if (!err) chk(hipEventCreate(&ev[i]));
        return err;
    }
    ~SrStage() {
        if (st) (void)hipStreamSynchronize(st);
        for (void *b : bufs) (void)hipFree(b);
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        if (own_stream && st) (void)hipStreamDestroy(st);
        if (prev_device >= 0) (void)hipSetDevice(prev_device);
    }
    template <class Tp> Tp *alloc(uint64_t n, int fill = -1) {             // fill: -1 none, else the byte
        void *p = nullptr;
        const size_t bytes = (n ? n : 1) * sizeof(Tp);
        if (err) return nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) { err = SR_ERR_NOMEM; sr_fail(SR_ERR_NOMEM, std::string("not enough device memory for ") + noun); return nullptr; }
        bufs.push_back(p);
        if (fill >= 0) chk(hipMemsetAsync(p, fill, bytes, st));
        return (Tp *)p;
    }
    void put(void *dst, const void *src, size_t bytes) { if (!err && bytes) chk(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st)); }
    void get(void *dst, const void *src, size_t bytes) { if (!err && bytes) chk(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st)); }
    void mark(int i) { if (!err) chk(hipEventRecord(ev[i], st)); }
    void sync() { if (!err) chk(hipStreamSynchronize(st)); }
    // from mark(a) to mark(b), rounded; after sync()
    uint64_t us(int a, int b) {
        float ms = 0.f;
        chk(hipEventElapsedTime(&ms, ev[a], ev[b]));
        return (uint64_t)(ms * 1000.0 + 0.5);
    }
};

// workgroups of SR_STAGE_BLOCK lanes for n items, one item per lane
inline unsigned sr_stage_grid(uint64_t n) { return (unsigned)((n + SR_STAGE_BLOCK - 1) / SR_STAGE_BLOCK); }

// ------------------------------------------------------------------ the path of a step
// the largest p with path_off[p] <= s (empty paths share an offset with their successor)
__device__ __forceinline__ uint32_t sr_path_of(const uint32_t *path_off, uint32_t np, uint32_t s) {
    uint32_t lo = 0, hi = np;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (path_off[mid] <= s) lo = mid; else hi = mid;
    }
    return lo;
}

// ------------------------------------------------------------------ step lengths
// out[s] = the length of the node of step s (len: node v at v - 1), the input of the scan.  T: a 64-bit unsigned type
template <class T> __global__ void __launch_bounds__(SR_STAGE_BLOCK) sr_step_len_kernel(const uint32_t *steps, const uint32_t *len, uint32_t S, T *out) {
    const uint32_t s = blockIdx.x * SR_STAGE_BLOCK + threadIdx.x;
    if (s < S) out[s] = len[(steps[s] >> 1) - 1];
}

template <class T> void sr_step_len(SrStage &x, const uint32_t *steps, const uint32_t *len, uint32_t S, T *out) {
    if (x.err) return;
    hipLaunchKernelGGL(sr_step_len_kernel<T>, dim3(sr_stage_grid(S)), dim3(SR_STAGE_BLOCK), 0, x.st, steps, len, S, out);
}

// ------------------------------------------------------------------ scan
// inclusive scan of n 64-bit unsigned values in place, sum or max (identity 0 for both): wave shuffles, an LDS combine across
// the workgroup, and a block-sums pass as the carry across workgroups (sr_scan recurses on the sums)
template <bool MAX, class T> __device__ __forceinline__ T sr_scan_op(T a, T b) { return MAX ? (a > b ? a : b) : a + b; }

template <bool MAX, class T> __global__ void __launch_bounds__(SR_STAGE_BLOCK) sr_scan_block_kernel(T *data, uint32_t n, T *sums) {
    static_assert(sizeof(T) == 8 && (T)-1 > 0, "a 64-bit unsigned type");
    __shared__ T wsum[SR_STAGE_WAVES];
    const uint32_t i = blockIdx.x * SR_STAGE_BLOCK + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T v = i < n ? data[i] : 0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T t = __shfl_up(v, o, 64);
        if ((int)lane >= o) v = sr_scan_op<MAX>(v, t);
    }
    if (lane == 63) wsum[wave] = v;
    __syncthreads();
    T carry = 0;
#pragma unroll
    for (int w = 0; w < SR_STAGE_WAVES; w++) if (w < (int)wave) carry = sr_scan_op<MAX>(carry, wsum[w]);
    v = sr_scan_op<MAX>(v, carry);
    if (i < n) data[i] = v;
    if (threadIdx.x == SR_STAGE_BLOCK - 1) sums[blockIdx.x] = v;     // lanes beyond n carry the last value on
}

template <bool MAX, class T> __global__ void __launch_bounds__(SR_STAGE_BLOCK) sr_scan_carry_kernel(T *data, uint32_t n, const T *sums) {
    const uint32_t i = blockIdx.x * SR_STAGE_BLOCK + threadIdx.x;
    if (blockIdx.x == 0 || i >= n) return;
    data[i] = sr_scan_op<MAX>(data[i], sums[blockIdx.x - 1]);
}

// the elements `sums` of sr_scan needs for n values: the block sums of every level
inline uint64_t sr_scan_room(uint64_t n) {
    uint64_t room = 0;
    while (n > 1) { n = (n + SR_STAGE_BLOCK - 1) / SR_STAGE_BLOCK; room += n; }
    return room + 1;
}

template <bool MAX, class T> void sr_scan(SrStage &x, T *data, uint32_t n, T *sums) {
    if (x.err || !n) return;
    const unsigned blocks = sr_stage_grid(n);
    hipLaunchKernelGGL((sr_scan_block_kernel<MAX, T>), dim3(blocks), dim3(SR_STAGE_BLOCK), 0, x.st, data, n, sums);
    if (blocks == 1) return;
    sr_scan<MAX>(x, sums, blocks, sums + blocks);
    hipLaunchKernelGGL((sr_scan_carry_kernel<MAX, T>), dim3(blocks), dim3(SR_STAGE_BLOCK), 0, x.st, data, n, (const T *)sums);
}
