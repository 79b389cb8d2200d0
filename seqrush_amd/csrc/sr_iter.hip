// sr_iter.hip -- phase 2 of the iterative mode (--iterative, align_and_unite_iterative src/seqrush.rs:1034-1122) on the
// device.  After the alignment kernel of a window (unfused: the CIGARs stay in the arena) the host enqueues, per chunk of
// CHECK_INTERVAL random entries and on the same stream: unite the chunk's alignments, count the components, decide.  The
// decision state lives in device memory, so the host does not wait inside a window; once the rule has fired every later
// kernel of the run returns at once and the union-find holds exactly the processed alignments.
// Component count (count_components :341-353): SeqRush::new unites 2i with 2i+1 for every base and nodes >= 2T are never
// touched, so the number of distinct find(2i) equals the number of roots among nodes [0, 2T) -- no find needed.
#include <hip/hip_runtime.h>
#include "sr_internal.h"
#include "sr_uf_dev.h"
#include "sr_iter_rule.h"
#define WG SR_WG

// sr_unite_kernel's loop (one pair per workgroup) behind the run's stop flag, read once per workgroup
__global__ void __launch_bounds__(WG) sr_iter_unite_kernel(SrUniteArgs a, const SrIterState *st) {
    if (st->stopped) return;                                // uniform: the whole chunk is skipped after the stop
    const int lane = threadIdx.x & 63;
    unsigned long long united = 0, runs = 0;
    int err = 0;
    for (uint32_t pair = blockIdx.x; pair < a.npairs; pair += gridDim.x) {
        if (a.score[pair] < 0 || a.score[pair] > a.max_score[pair]) continue;   // failed / dropped by -d (still processed)
        const uint32_t q = a.pair_q[pair], t = a.pair_t[pair];
        uf_unite_cigar<WG>(a.cigar_ops + a.cigar_base[pair], a.cigar_cnt[pair], a.seq_goff[q], a.seq_goff[t], a.seqlen[q],
                           a.is_reverse[pair] != 0, 0, 0, a.min_match_len, a.nodes, united, runs, err);
    }
    for (int o = 32; o > 0; o >>= 1) {
        united += __shfl_xor(united, o, 64);
        runs += __shfl_xor(runs, o, 64);
    }
    if (lane == 0) {
        if (united) atomicAdd(&a.counters[4], united);
        if (runs) atomicAdd(&a.counters[5], runs);
    }
    if (err) atomicOr(a.error_flag, err);
}

// roots among nodes [0, 2T): lane reads the node words (2i, 2i+1) of base i as one 16-byte load (plain loads: the unite
// kernel before it on the stream has finished); wave sums by shuffles, workgroup sum through LDS, one 64-bit atomic per
// workgroup into *count (zeroed by the host before the window's chain).  st == NULL: count unconditionally.
__global__ void __launch_bounds__(WG) sr_count_roots_kernel(const unsigned long long *nodes, unsigned long long nbases,
                                                            unsigned long long *count, const SrIterState *st) {
    if (st && st->stopped) return;
    __shared__ unsigned long long wsum[WG / 64];
    const ulonglong2 *w = reinterpret_cast<const ulonglong2 *>(nodes);
    unsigned long long c = 0;
    const unsigned long long stride = (unsigned long long)gridDim.x * WG;
    for (unsigned long long i = (unsigned long long)blockIdx.x * WG + threadIdx.x; i < nbases; i += stride) {
        const ulonglong2 v = w[i];
        c += ((v.x & UF_PARENT_MASK) == 2 * i) ? 1 : 0;
        c += ((v.y & UF_PARENT_MASK) == 2 * i + 1) ? 1 : 0;
    }
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
        for (int k = 0; k < WG / 64; k++) s += wsum[k];
        if (s) __hip_atomic_fetch_add(count, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// one lane: the stop rule (sr_iter_rule.h) on counts[k], the count of check number `check` of the run
__global__ void sr_iter_decide_kernel(SrIterState *st, const unsigned long long *counts, uint32_t k, uint32_t check) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    SrIterState s = *st;
    if (s.stopped) return;
    sr_iter_step(&s, counts[k], check);
    *st = s;
}

extern "C" int srk_iter_unite(const SrUniteArgs *a, int nwg, const SrIterState *st, void *stream) {
    hipLaunchKernelGGL(sr_iter_unite_kernel, dim3(nwg > 0 ? nwg : 1), dim3(WG), 0, (hipStream_t)stream, *a, st);
    return (int)hipGetLastError();
}

extern "C" int srk_count_roots(const unsigned long long *nodes, uint64_t nbases, unsigned long long *count, const SrIterState *st,
                               void *stream) {
    const uint64_t nb = (nbases + WG - 1) / WG;
    hipLaunchKernelGGL(sr_count_roots_kernel, dim3(nb == 0 ? 1 : (nb > 2048 ? 2048 : (unsigned)nb)), dim3(WG), 0, (hipStream_t)stream,
                       nodes, (unsigned long long)nbases, count, st);
    return (int)hipGetLastError();
}

extern "C" int srk_iter_decide(SrIterState *st, const unsigned long long *counts, uint32_t k, uint32_t check, void *stream) {
    hipLaunchKernelGGL(sr_iter_decide_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, st, counts, k, check);
    return (int)hipGetLastError();
}
