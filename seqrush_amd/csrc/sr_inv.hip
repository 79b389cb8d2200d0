// sr_inv.hip -- the CIGAR scan of --patch-inversions (rule: sr_inv_rule.h; reference src/cigar_analysis.rs:23-147 as called
// by src/inversion_aware_seqrush.rs:163-170).  It runs on the context's stream after a batch's alignment kernel, while the
// batch's CIGARs are still in the arena.
// One wave per alignment; lanes take the run-length ops in chunks of 64.  Inclusive wave scans give four running sums per
// op: query and target coordinates, and the query / target columns of non-match ops.  A match op closes the site the match
// op before it opened (found with a ballot; the one before the chunk comes from the carry), and the site's gaps are the
// differences of the non-match sums between the two: a segmented reduction without a second scan.  The carry (four sums and
// the open site) crosses chunks, so a gap of any number of ops is handled.  The end of the CIGAR closes the last site.
// Pass 0 counts the candidates of every alignment, sr_inv_offsets_kernel turns the counts into exclusive offsets, pass 1
// walks again and writes the job records at offset + rank: pair order, then CIGAR order, no atomic append.
// JOIN = 1 is the joined instance (--inversion-join J): only match ops of at least J columns are anchors, so the columns of
// shorter ones (islands) enter both gap sums; a fifth scan carries what the main alignment paid per op (sr_inv_op_cost),
// and the 24-byte record carries the site's share of it.  Pass 0 also counts the islands inside candidates (a sixth scan,
// stats[3]).  The JOIN = 0 instances are the plain rule and write the 20-byte record.
#include <hip/hip_runtime.h>
#include "sr_internal.h"
#include "sr_inv_rule.h"
#define WG SR_WG

__device__ __forceinline__ unsigned wave_incl_scan(unsigned v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned n = __shfl_up(v, o, 64);
        if (lane >= o) v += n;
    }
    return v;
}

template <int EMIT, int JOIN>
__global__ void __launch_bounds__(WG) sr_inv_scan_kernel(SrInvScanArgs a) {
    const int lane = threadIdx.x & 63;
    const uint32_t wave = blockIdx.x * (WG / 64) + (threadIdx.x >> 6), nwaves = gridDim.x * (WG / 64);
    unsigned long long n_scanned = 0, n_sites = 0, n_cand = 0, n_isl = 0;
    const SrInvPen pen = {a.pen[0], a.pen[1], a.pen[2], a.pen[3], a.pen[4], a.pen[5]};
    for (uint32_t pair = wave; pair < a.npairs; pair += nwaves) {                  // wave-uniform
        const int32_t sc = a.score ? a.score[pair] : 0;
        if (sc < 0 || (a.max_score && sc > a.max_score[pair])) {                   // failed, or dropped by -d: not scanned
            if (!EMIT && lane == 0) a.count[pair] = 0;
            continue;
        }
        n_scanned++;
        const uint32_t *ops = a.cigar_ops + a.cigar_base[pair];
        const uint32_t cnt = a.cigar_cnt[pair];
        // carry: sums before the chunk; the site opened by the last match op before the chunk
        unsigned cq = 0, ct = 0, cgq = 0, cgt = 0;
        unsigned open_q = 0, open_t = 0, open_gq = 0, open_gt = 0;
        unsigned cc = 0, open_c = 0, ci = 0, open_i = 0;                           // JOIN: cost sum, island count
        bool open = false;
        uint32_t emitted = 0;                                                      // candidates of this alignment so far
        const uint32_t out0 = EMIT ? a.offset[pair] : 0;
        for (uint32_t base = 0; base < cnt; base += 64) {
            const uint32_t i = base + lane;
            unsigned dq = 0, dt = 0, dc = 0, di = 0;
            bool is_m = false;
            if (i < cnt) {
                const uint32_t op = ops[i] & 15u; const unsigned len = ops[i] >> 4;
                if constexpr (JOIN) {
                    dc = sr_inv_op_cost(op, len, pen);
                    di = op == SR_OP_M && len < a.join_below ? 1u : 0u;
                }
                if (op == SR_OP_M) { dq = len; dt = len; is_m = JOIN ? len >= a.join_below : true; }
                else if (op == SR_OP_X) { dq = len; dt = len; }
                else if (op == SR_OP_I) dt = len;                                  // raw 'I' consumes text (target)
                else dq = len;                                                     // raw 'D' consumes pattern (query)
            }
            const unsigned q = cq + wave_incl_scan(dq, lane), t = ct + wave_incl_scan(dt, lane);
            const unsigned gq = cgq + wave_incl_scan(is_m ? 0u : dq, lane), gt = cgt + wave_incl_scan(is_m ? 0u : dt, lane);
            unsigned c = 0, ni = 0;
            if constexpr (JOIN) c = cc + wave_incl_scan(dc, lane);
            if constexpr (JOIN && !EMIT) ni = ci + wave_incl_scan(di, lane);
            const unsigned long long mmask = __ballot(is_m);
            const unsigned long long below = mmask & ((1ULL << lane) - 1ULL);
            const int prev = below ? 63 - __clzll((long long)below) : -1;          // match op before this lane, in the chunk
            const int src = prev < 0 ? 0 : prev;
            const unsigned pq = __shfl(q, src, 64), pt = __shfl(t, src, 64), pgq = __shfl(gq, src, 64), pgt = __shfl(gt, src, 64);
            unsigned pc = 0, pni = 0;
            if constexpr (JOIN) pc = __shfl(c, src, 64);
            if constexpr (JOIN && !EMIT) pni = __shfl(ni, src, 64);
            bool cand = false;
            unsigned sqa = 0, sta = 0, sqg = 0, stg = 0;
            if (is_m && (prev >= 0 || open)) {                                     // this match op closes a site
                sqa = prev >= 0 ? pq : open_q; sta = prev >= 0 ? pt : open_t;
                sqg = gq - (prev >= 0 ? pgq : open_gq); stg = gt - (prev >= 0 ? pgt : open_gt);
                const int kind = sr_inv_site_kind(sqg, stg, a.min_size);
                if (!EMIT && kind != SR_INV_NONE) n_sites++;
                cand = sr_inv_is_candidate(sqg, stg, a.min_size) != 0;
                if constexpr (JOIN && !EMIT) { if (cand) n_isl += ni - (prev >= 0 ? pni : open_i); }
            }
            const unsigned long long cmask = __ballot(cand);
            if (cand) {
                if (EMIT) {
                    const uint64_t at = (uint64_t)out0 + emitted + (uint64_t)__popcll(cmask & ((1ULL << lane) - 1ULL));
                    if constexpr (JOIN) {                                          // (an anchor costs 0: c is the sum up to it)
                        if (at < a.job_cap) { SrInvJobJ j = {a.pair0 + pair, sqa, sqg, sta, stg, (int32_t)(c - (prev >= 0 ? pc : open_c))}; a.jobs_j[at] = j; }
                    } else
                    if (at < a.job_cap) { SrInvJob j = {a.pair0 + pair, sqa, sqg, sta, stg}; a.jobs[at] = j; }
                }
            }
            emitted += (uint32_t)__popcll(cmask);
            // carry to the next chunk
            cq = __shfl(q, 63, 64); ct = __shfl(t, 63, 64); cgq = __shfl(gq, 63, 64); cgt = __shfl(gt, 63, 64);
            if constexpr (JOIN) cc = __shfl(c, 63, 64);
            if constexpr (JOIN && !EMIT) ci = __shfl(ni, 63, 64);
            if (mmask) {
                const int last = 63 - __clzll((long long)mmask);
                open = true;
                open_q = __shfl(q, last, 64); open_t = __shfl(t, last, 64); open_gq = __shfl(gq, last, 64); open_gt = __shfl(gt, last, 64);
                if constexpr (JOIN) open_c = __shfl(c, last, 64);
                if constexpr (JOIN && !EMIT) open_i = __shfl(ni, last, 64);
            }
        }
        if (open && lane == 0) {                                                   // the end of the CIGAR closes the last site
            const unsigned sqg = cgq - open_gq, stg = cgt - open_gt;
            if (!EMIT && sr_inv_site_kind(sqg, stg, a.min_size) != SR_INV_NONE) n_sites++;
            if (sr_inv_is_candidate(sqg, stg, a.min_size)) {
                if (EMIT) {
                    const uint64_t at = (uint64_t)out0 + emitted;
                    if constexpr (JOIN) {
                        if (at < a.job_cap) { SrInvJobJ j = {a.pair0 + pair, open_q, sqg, open_t, stg, (int32_t)(cc - open_c)}; a.jobs_j[at] = j; }
                    } else
                    if (at < a.job_cap) { SrInvJob j = {a.pair0 + pair, open_q, sqg, open_t, stg}; a.jobs[at] = j; }
                }
                if constexpr (JOIN && !EMIT) n_isl += ci - open_i;
                emitted++;                                                         // (lane 0 only: it writes the count)
            }
        }
        if (!EMIT && lane == 0) a.count[pair] = emitted;
        if (!EMIT) n_cand += lane == 0 ? emitted : 0;
    }
    if (!EMIT) {
        // candidates found inside chunks were counted by every lane's `emitted`; lane 0 holds the alignment's total
        for (int o = 32; o > 0; o >>= 1) n_sites += __shfl_xor(n_sites, o, 64);
        if constexpr (JOIN) for (int o = 32; o > 0; o >>= 1) n_isl += __shfl_xor(n_isl, o, 64);
        if (lane == 0) {
            if (n_scanned) atomicAdd(&a.stats[0], n_scanned);
            if (n_sites) atomicAdd(&a.stats[1], n_sites);
            if (n_cand) atomicAdd(&a.stats[2], n_cand);
            if (JOIN && n_isl) atomicAdd(&a.stats[3], n_isl);
        }
    }
}

// exclusive offsets of the per-alignment counts: one workgroup, chunks of WG with a carry; off[n] = total
__global__ void __launch_bounds__(WG) sr_inv_offsets_kernel(const uint32_t *count, uint32_t n, uint32_t *off) {
    __shared__ unsigned wsum[WG / 64];
    __shared__ unsigned carry;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < n; base += WG) {
        const uint32_t i = base + tid;
        const unsigned v = i < n ? count[i] : 0;
        unsigned s = wave_incl_scan(v, lane);
        if (lane == 63) wsum[wv] = s;
        __syncthreads();
        unsigned add = carry;
        for (int w = 0; w < wv; w++) add += wsum[w];
        s += add;
        if (i < n) off[i] = s - v;
        __syncthreads();
        if (tid == WG - 1) carry = s;
        __syncthreads();
    }
    if (tid == 0) off[n] = carry;
}

extern "C" int srk_inv_scan(const SrInvScanArgs *a, int emit, void *stream) {
    const uint32_t per = WG / 64;
    const uint64_t nb = ((uint64_t)a->npairs + per - 1) / per;
    const dim3 grid(nb == 0 ? 1 : (nb > 4096 ? 4096 : (unsigned)nb));
    if (a->join_below) {                                                           // the joined instances
        if (emit) hipLaunchKernelGGL((sr_inv_scan_kernel<1, 1>), grid, dim3(WG), 0, (hipStream_t)stream, *a);
        else hipLaunchKernelGGL((sr_inv_scan_kernel<0, 1>), grid, dim3(WG), 0, (hipStream_t)stream, *a);
    } else if (emit) hipLaunchKernelGGL((sr_inv_scan_kernel<1, 0>), grid, dim3(WG), 0, (hipStream_t)stream, *a);
    else hipLaunchKernelGGL((sr_inv_scan_kernel<0, 0>), grid, dim3(WG), 0, (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}

extern "C" int srk_inv_offsets(const uint32_t *count, uint32_t n, uint32_t *off, void *stream) {
    hipLaunchKernelGGL(sr_inv_offsets_kernel, dim3(1), dim3(WG), 0, (hipStream_t)stream, count, n, off);
    return (int)hipGetLastError();
}
