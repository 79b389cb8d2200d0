// sr_compact.hip -- compaction + renumbering of the induced graph from per-handle tables (sr_compact_tab.h), on the
// device and, with the same functors in index order, on the host.
//
// One driver, two executors.  CtDevExec launches every functor as a grid-stride kernel of 256 threads on one stream,
// scans with sr_graph.hip's exclusive scan and clears tables with hipMemsetAsync; CtHostExec runs the functor for
// i = 0 .. n-1.  A round is: tables -> links -> list ranking by pointer jumping (one launch and one flag readback per
// jump, at most ceil(log2(handles)) + 1) -> chains -> validation -> ONE readback (irregular?, chains validated, exact
// step / edge counts) -> rewrite of steps, edges, node text.  A round that holds an irregular list is downloaded, run
// by sr_compact.cpp's compact_round and uploaded again.  No captured graph, no recursion, no loop without a bound.
#include <hip/hip_runtime.h>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/seqrush_amd.h"
#include "sr_internal.h"
#include "sr_sort.h"
#include "sr_compact.h"
#include "sr_compact_tab.h"

#define CT_BLOCK 256

template <class F>
__global__ void __launch_bounds__(CT_BLOCK) ct_kernel(uint64_t n, F f) {
    const uint64_t stride = (uint64_t)gridDim.x * CT_BLOCK;
    for (uint64_t i = (uint64_t)blockIdx.x * CT_BLOCK + threadIdx.x; i < n; i += stride) f(i);
}

namespace {

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

struct CtHostExec {
    std::vector<void *> bufs;
    int err = 0;
    ~CtHostExec() { for (void *b : bufs) free(b); }
    void *alloc(size_t bytes) { void *p = malloc(bytes ? bytes : 16); if (!p) err = SR_ERR_NOMEM; else bufs.push_back(p); return p; }
    void fill(void *p, int byte, size_t bytes) { memset(p, byte, bytes); }
    template <class F> void run(uint64_t n, const F &f) { for (uint64_t i = 0; i < n; i++) f(i); }
    void scan(const uint32_t *in, uint64_t n, uint32_t *out, uint32_t *total) {
        uint32_t s = 0;
        for (uint64_t i = 0; i < n; i++) { const uint32_t x = in[i]; out[i] = s; s += x; }
        *total = s;
    }
    void get(void *dst, const void *src, size_t bytes) { memcpy(dst, src, bytes); }       // synchronous
    void put(void *dst, const void *src, size_t bytes) { memcpy(dst, src, bytes); }
    void copy(void *dst, const void *src, size_t bytes) { memcpy(dst, src, bytes); }
    void mark(int) {}
    float device_ms() { return 0.f; }
};

struct CtDevExec {
    hipStream_t st = nullptr;
    bool own_stream = false;
    int prev_device = -1;
    std::vector<void *> bufs;
    uint32_t *tile_sum = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    int err = 0;
    void chk(hipError_t e) { if (e != hipSuccess && !err) { err = SR_ERR_HIP; sr_fail(SR_ERR_HIP, std::string("compact: ") + hipGetErrorString(e)); } }
    ~CtDevExec() {
        if (st) (void)hipStreamSynchronize(st);
        for (void *b : bufs) (void)hipFree(b);
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        if (own_stream && st) (void)hipStreamDestroy(st);
        if (prev_device >= 0) (void)hipSetDevice(prev_device);
    }
    void *alloc(size_t bytes) {
        void *p = nullptr;
        if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) { if (!err) { err = SR_ERR_NOMEM; sr_fail(SR_ERR_NOMEM, "not enough device memory for compaction"); } return nullptr; }
        bufs.push_back(p);
        return p;
    }
    void fill(void *p, int byte, size_t bytes) { if (!err && bytes) chk(hipMemsetAsync(p, byte, bytes, st)); }
    template <class F> void run(uint64_t n, const F &f) {
        if (err || !n) return;
        uint64_t b = (n + CT_BLOCK - 1) / CT_BLOCK;
        if (b > 8192) b = 8192;
        hipLaunchKernelGGL(ct_kernel<F>, dim3((unsigned)b), dim3(CT_BLOCK), 0, st, n, f);
    }
    void scan(const uint32_t *in, uint64_t n, uint32_t *out, uint32_t *total) {
        if (!err && srk_scan_u32(in, n, out, tile_sum, total, st)) chk(hipErrorLaunchFailure);
    }
    void get(void *dst, const void *src, size_t bytes) {
        if (err) return;
        if (bytes) chk(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
        chk(hipStreamSynchronize(st));
        chk(hipGetLastError());
    }
    void put(void *dst, const void *src, size_t bytes) { if (!err && bytes) chk(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st)); }
    void copy(void *dst, const void *src, size_t bytes) { if (!err && bytes) chk(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st)); }
    void mark(int i) { if (!err) chk(hipEventRecord(ev[i], st)); }
    float device_ms() {
        float ms = 0.f;
        if (!err) { chk(hipEventSynchronize(ev[1])); chk(hipEventElapsedTime(&ms, ev[0], ev[1])); }
        return ms;
    }
};

// the graph and every table of a round, in buffers sized once for the whole run
template <class X>
struct CtRun {
    X &x;
    uint64_t capN = 0, capH = 0, capS = 0, capE = 0, hcap = 0;
    uint32_t NN = 0, NP = 0, T = 0, NS = 0, NE = 0;  // NS / NE: exact after a round's readback, upper bounds before it
    int cur = 0;                                     // which of the double buffers holds the graph
    uint32_t *steps[2], *path_off[2], *len[2], *off[2], *alive[2];
    unsigned long long *edges[2];
    uint8_t *text[2];
    uint32_t *zero_blk, *ones_blk;                   // tables cleared to 0 / to all ones once per round
    uint8_t *visits, *bad, *pfirst;
    uint32_t *jbuf[2][6];
    uint32_t *cstart, *clast, *vflag, *rank, *pm, *cid, *mdst, *moff, *mrev, *sflag, *spos, *eslot, *ctl;
    unsigned long long *hkeys, *ekey;
    size_t zero_bytes = 0, ones_bytes = 0;
    explicit CtRun(X &x_) : x(x_) {}

    template <class Tp> Tp *al(size_t n) { return (Tp *)x.alloc(n * sizeof(Tp)); }
    int reserve(uint64_t nn, uint64_t ns, uint64_t ne, uint64_t np, uint64_t t) {
        if (nn >= 0x3fffffffULL || ns >= 0x7fffffffULL || ne >= 0x7fffffffULL || t >= 0x7fffffffULL)
            return sr_fail(SR_ERR_UNSUPPORTED, "compaction by tables supports < 2^30 nodes and < 2^31 steps, edges and bases");
        capN = 2 * nn + 2; capH = 2 * capN; capS = ns + 1; capE = ne + 1; NP = (uint32_t)np; T = (uint32_t)t;
        hcap = 64;
        while (hcap < 2 * ne + 16) hcap <<= 1;
        for (int b = 0; b < 2; b++) {
            steps[b] = al<uint32_t>(capS); edges[b] = al<unsigned long long>(capE); path_off[b] = al<uint32_t>(np + 1);
            len[b] = al<uint32_t>(capN); off[b] = al<uint32_t>(capN); alive[b] = al<uint32_t>(capN); text[b] = al<uint8_t>(t + 1);
            for (int k = 0; k < 6; k++) jbuf[b][k] = al<uint32_t>(capH);
        }
        // zero block: fcnt, bcnt, refused | visits, bad | pfirst;  ones block: fonly, succ, next, pred, listmin | hvals, hkeys
        zero_bytes = 3 * capH * 4 + 2 * capH + capS + 1;
        zero_blk = (uint32_t *)x.alloc(zero_bytes);
        ones_bytes = 5 * capH * 4;
        ones_blk = (uint32_t *)x.alloc(ones_bytes);
        hkeys = al<unsigned long long>(hcap + hcap / 2 + 1);     // hvals behind the keys: one fill
        cstart = al<uint32_t>(capH); clast = al<uint32_t>(capH); vflag = al<uint32_t>(capH); rank = al<uint32_t>(capH);
        pm = al<uint32_t>(capH); cid = al<uint32_t>(capH);
        mdst = al<uint32_t>(capN); moff = al<uint32_t>(capN); mrev = al<uint32_t>(capN);
        uint64_t m = capS > capE ? capS : capE;
        if (capH > m) m = capH;
        sflag = al<uint32_t>(m); spos = al<uint32_t>(m); eslot = al<uint32_t>(capE); ekey = al<unsigned long long>(capE);
        ctl = al<uint32_t>(CT_NCTL);
        if (x.err) return x.err;
        visits = (uint8_t *)(zero_blk + 3 * capH); bad = visits + capH; pfirst = bad + capH;
        x.fill(ctl, 0, CT_NCTL * 4);
        return SR_OK;
    }
    uint32_t *size_ptr(int b) { return ctl + CT_SIZE + 2 * b; }

    CtView view(int jread) {
        CtView v;
        memset(&v, 0, sizeof v);
        v.NN = NN; v.NH = 2 * NN; v.NP = NP; v.T = T; v.size = size_ptr(cur); v.size_out = size_ptr(cur ^ 1); v.hmask = hcap - 1;
        v.steps = steps[cur]; v.edges = edges[cur]; v.path_off = path_off[cur]; v.node_len = len[cur]; v.node_off = off[cur];
        v.alive = alive[cur]; v.text = text[cur];
        const int o = cur ^ 1;
        v.o_steps = steps[o]; v.o_edges = edges[o]; v.o_path_off = path_off[o]; v.o_len = len[o]; v.o_off = off[o]; v.o_alive = alive[o];
        v.o_text = text[o];
        v.fcnt = zero_blk; v.bcnt = zero_blk + capH; v.refused = zero_blk + 2 * capH; v.visits = visits; v.bad = bad; v.pfirst = pfirst;
        v.fonly = ones_blk; v.succ = ones_blk + capH; v.next = ones_blk + 2 * capH; v.pred = ones_blk + 3 * capH; v.listmin = ones_blk + 4 * capH;
        v.cstart = cstart; v.clast = clast; v.vflag = vflag; v.rank = rank; v.pm = pm; v.cid = cid;
        v.mdst = mdst; v.moff = moff; v.mrev = mrev; v.sflag = sflag; v.spos = spos; v.eslot = eslot; v.ekey = ekey;
        v.hkeys = hkeys; v.hvals = (uint32_t *)(hkeys + hcap); v.ctl = ctl;
        uint32_t **r = jbuf[jread], **w = jbuf[jread ^ 1];
        v.jp = r[0]; v.jmin = r[1]; v.jall = r[2]; v.jhead = r[3]; v.jcnt = r[4]; v.jlen = r[5];
        v.kp = w[0]; v.kmin = w[1]; v.kall = w[2]; v.khead = w[3]; v.kcnt = w[4]; v.klen = w[5];
        return v;
    }

    // ---- graph in
    int upload(const SrGraph &g) {
        std::vector<uint32_t> l(g.node_seq.size()), a(g.node_seq.size()), po(g.path_off.size());
        std::vector<unsigned long long> e(g.edges.size());
        std::string t;
        for (size_t i = 0; i < l.size(); i++) { l[i] = g.node_alive[i] ? (uint32_t)g.node_seq[i].size() : 0u; a[i] = g.node_alive[i] ? 1u : 0u; if (a[i]) t += g.node_seq[i]; }
        for (size_t i = 0; i < po.size(); i++) po[i] = (uint32_t)g.path_off[i];
        for (size_t i = 0; i < e.size(); i++) e[i] = ((unsigned long long)g.edges[i].first << 32) | g.edges[i].second;
        if (l.size() > capN || g.steps.size() > capS || e.size() > capE || t.size() > T || po.size() != (size_t)NP + 1)
            return sr_fail(SR_ERR_DEVICE_FAULT, "compact: graph outgrew its buffers");
        NN = (uint32_t)l.size(); NS = (uint32_t)g.steps.size(); NE = (uint32_t)e.size();
        const uint32_t sz[2] = {NS, NE};
        x.put(steps[cur], g.steps.data(), (size_t)NS * 4); x.put(edges[cur], e.data(), (size_t)NE * 8);
        x.put(path_off[cur], po.data(), po.size() * 4); x.put(len[cur], l.data(), (size_t)NN * 4); x.put(alive[cur], a.data(), (size_t)NN * 4);
        x.put(text[cur], t.data(), t.size()); x.put(size_ptr(cur), sz, 8);
        x.scan(len[cur], NN, off[cur], ctl + CT_NVALID);
        uint32_t dummy;
        x.get(&dummy, ctl + CT_NVALID, 4);           // the host vectors above leave scope
        return x.err;
    }
    // the arrays srk_graph_induce left on the device: nodes 1..nn of one base each
    int adopt(const uint32_t *d_steps, uint64_t ns, const unsigned long long *d_edges, uint64_t ne, const uint8_t *d_nbase, uint64_t nn,
              const uint64_t *path_off_host) {
        std::vector<uint32_t> l(nn + 1, 1u), po((size_t)NP + 1);
        l[0] = 0;
        for (size_t i = 0; i < po.size(); i++) po[i] = (uint32_t)path_off_host[i];
        NN = (uint32_t)nn + 1; NS = (uint32_t)ns; NE = (uint32_t)ne;
        const uint32_t sz[2] = {NS, NE};
        x.copy(steps[cur], d_steps, ns * 4); x.copy(edges[cur], d_edges, ne * 8); x.copy(text[cur], d_nbase, nn);
        x.put(path_off[cur], po.data(), po.size() * 4); x.put(len[cur], l.data(), (size_t)NN * 4); x.put(alive[cur], l.data(), (size_t)NN * 4);
        x.put(size_ptr(cur), sz, 8);
        x.scan(len[cur], NN, off[cur], ctl + CT_NVALID);
        uint32_t dummy;
        x.get(&dummy, ctl + CT_NVALID, 4);
        return x.err;
    }
    // ---- graph out (buffer b; node ids as they are)
    int download(int b, SrGraph &g) {
        std::vector<uint32_t> l(NN), o(NN), a(NN), po((size_t)NP + 1);
        std::vector<unsigned long long> e(NE);
        std::vector<uint8_t> t((size_t)T + 1);
        g = SrGraph();
        g.steps.resize(NS);
        x.get(g.steps.data(), steps[b], (size_t)NS * 4); x.get(e.data(), edges[b], (size_t)NE * 8);
        x.get(po.data(), path_off[cur], po.size() * 4); x.get(l.data(), len[cur], (size_t)NN * 4); x.get(o.data(), off[cur], (size_t)NN * 4);
        x.get(a.data(), alive[cur], (size_t)NN * 4); x.get(t.data(), text[cur], T);
        if (x.err) return x.err;
        g.node_seq.assign(NN, std::string()); g.node_alive.assign(NN, 0);
        for (uint32_t i = 0; i < NN; i++) if (a[i]) { g.node_alive[i] = 1; g.node_seq[i].assign((const char *)t.data() + o[i], l[i]); }
        g.path_off.assign(po.begin(), po.end());
        g.edges.resize(NE);
        for (uint32_t i = 0; i < NE; i++) g.edges[i] = {(uint32_t)(e[i] >> 32), (uint32_t)e[i]};
        return SR_OK;
    }

    // ---- compact() + renumber; g receives the result
    int compact(SrGraph &g, uint64_t stats[8], double *copy_ms) {
        uint64_t rounds = 0, fell_back = 0, merged = 0, longest = 0, jumps = 0;
        x.mark(0);
        for (;;) {
            rounds++;
            const uint32_t NH = 2 * NN;
            x.fill(zero_blk, 0, zero_bytes); x.fill(ones_blk, 0xff, ones_bytes); x.fill(ctl, 0, 12); x.fill(ctl + CT_JFLAG, 0, (CT_NCTL - CT_JFLAG) * 4);
            int jr = 0;
            CtView v = view(jr);
            x.run(NE, CtDegree{v}); x.run(NP, CtPathFirst{v}); x.run(NS, CtSuccAny{v}); x.run(NS, CtSuccBad{v}); x.run(NH, CtLink{v});
            // list ranking: jump i reads buffer jr, writes the other
            x.run(NH, CtJumpInit{v});
            jr ^= 1;
            uint32_t more = 0, max_jumps = 1;
            while ((1ull << (max_jumps - 1)) < NH) max_jumps++;          // ceil(log2(NH)) + 1
            if (max_jumps > CT_MAX_JUMPS) max_jumps = CT_MAX_JUMPS;
            x.get(&more, ctl + CT_JFLAG, 4);
            for (uint32_t it = 1; more && it <= max_jumps; it++) {
                v = view(jr); v.jump = it;
                x.run(NH, CtJump{v});
                jr ^= 1; jumps++;
                x.get(&more, ctl + CT_JFLAG + it, 4);
            }
            v = view(jr);                            // a list without a head is still unresolved here: CtChain reports it
            x.run(NH, CtTail{v}); x.run(NH, CtChain{v}); x.run(NS, CtValidate{v}); x.run(NH, CtValidFlag{v});
            x.scan(vflag, NH, rank, ctl + CT_NVALID);
            uint32_t rb[8];
            x.get(rb, ctl, sizeof rb);               // the round's readback
            if (x.err) return x.err;
            if (rb[CT_HASH_FULL]) return sr_fail(SR_ERR_DEVICE_FAULT, "compact: edge table full");
            NS = rb[CT_SIZE + 2 * cur]; NE = rb[CT_SIZE + 2 * cur + 1];
            if (rb[CT_LONGEST] > longest) longest = rb[CT_LONGEST];
            if (rb[CT_IRREGULAR]) {
                const auto t0 = std::chrono::steady_clock::now();
                SrGraph h;
                int r = download(cur, h);
                if (r) return r;
                const size_t before = h.node_seq.size();
                const bool any = sr_graph_compact_round(h);
                fell_back++;
                if (!any) { *copy_ms += ms_since(t0); break; }
                merged += h.node_seq.size() - before;
                if ((r = upload(h))) return r;
                *copy_ms += ms_since(t0);
                continue;
            }
            const uint32_t nvalid = rb[CT_NVALID];
            if (!nvalid) break;
            if ((uint64_t)NN + nvalid > capN) return sr_fail(SR_ERR_DEVICE_FAULT, "compact: node table full");
            merged += nvalid;
            x.fill(hkeys, 0xff, hcap * 12);
            x.run(NH, CtMap{v}); x.run(NS, CtStepFlag{v});
            x.scan(sflag, NS, spos, v.size_out);
            x.run(NS, CtStepEmit{v}); x.run((uint64_t)NP + 1, CtPathOff{v});
            x.run(NE, CtEdgeInsert{v}); x.run(NE, CtEdgeFlag{v});
            x.scan(sflag, NE, spos, v.size_out + 1);
            x.run(NE, CtEdgeEmit{v});
            x.scan(len[cur ^ 1], (uint64_t)NN + nvalid, off[cur ^ 1], ctl + CT_NVALID);
            x.run(T, CtTextCopy{v});
            cur ^= 1; NN += nvalid;
        }
        // renumber_nodes_sequentially: steps and edges into the other buffer, node text gathered by the host
        CtView v = view(0);
        x.scan(alive[cur], NN, rank, ctl + CT_NVALID);
        x.run(NS, CtRenumberSteps{v}); x.run(NE, CtRenumberEdges{v});
        x.mark(1);
        const auto t0 = std::chrono::steady_clock::now();
        SrGraph raw;
        int r = download(cur ^ 1, raw);
        if (r) return r;
        uint32_t hf = 0;
        x.get(&hf, ctl + CT_HASH_FULL, 4);
        if (hf) return sr_fail(SR_ERR_DEVICE_FAULT, "compact: edge table full");
        g = SrGraph();
        g.steps.swap(raw.steps); g.edges.swap(raw.edges); g.path_off.swap(raw.path_off);
        g.node_seq.assign(1, std::string()); g.node_alive.assign(1, 0);
        for (size_t i = 0; i < raw.node_seq.size(); i++)
            if (raw.node_alive[i]) { g.node_seq.push_back(std::move(raw.node_seq[i])); g.node_alive.push_back(1); }
        *copy_ms += ms_since(t0);
        if (stats) {
            stats[0] = rounds; stats[1] = fell_back; stats[2] = merged; stats[3] = longest; stats[4] = jumps;
            stats[5] = (uint64_t)(x.device_ms() * 1000.0 + 0.5); stats[6] = (uint64_t)(*copy_ms * 1000.0 + 0.5); stats[7] = 0;
        }
        return x.err;
    }
};

uint64_t graph_bases(const SrGraph &g) {
    uint64_t t = 0;
    for (size_t i = 0; i < g.node_seq.size(); i++) if (g.node_alive[i]) t += g.node_seq[i].size();
    return t;
}

int dev_open(CtDevExec &x, int device, void *stream, uint64_t scan_n) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return sr_fail(SR_ERR_NO_DEVICE, "compact: no HIP device");
    if (device >= ndev) return sr_fail(SR_ERR_INVALID, "compact: no HIP device " + std::to_string(device));
    x.chk(hipGetDevice(&x.prev_device));
    x.chk(hipSetDevice(device));
    x.st = (hipStream_t)stream;
    if (!x.st && !x.err) { x.chk(hipStreamCreateWithFlags(&x.st, hipStreamNonBlocking)); x.own_stream = !x.err; }
    if (!x.err) x.chk(hipEventCreate(&x.ev[0]));
    if (!x.err) x.chk(hipEventCreate(&x.ev[1]));
    x.tile_sum = (uint32_t *)x.alloc((scan_n / 1024 + 2) * 4);
    return x.err;
}

thread_local uint64_t g_last_stats[8];

}   // namespace

int sr_graph_compact_tables(SrGraph &g, int device, void *stream, uint64_t stats[8]) {
    uint64_t local[8] = {0};
    if (!stats) stats = local;
    const uint64_t nn = g.node_seq.size(), ns = g.steps.size(), ne = g.edges.size(), np = g.path_off.size() - 1, t = graph_bases(g);
    double copy_ms = 0;
    int r;
    if (device < 0) {
        CtHostExec x;
        CtRun<CtHostExec> run(x);
        if ((r = run.reserve(nn, ns, ne, np, t)) || (r = run.upload(g))) return r;
        const auto t0 = std::chrono::steady_clock::now();
        r = run.compact(g, stats, &copy_ms);
        stats[5] = (uint64_t)(ms_since(t0) * 1000.0 + 0.5); stats[6] = 0;
    } else {
        CtDevExec x;
        CtRun<CtDevExec> run(x);
        if ((r = dev_open(x, device, stream, 4 * nn + 8 + ns + ne)) || (r = run.reserve(nn, ns, ne, np, t))) return r;
        const auto t0 = std::chrono::steady_clock::now();
        if ((r = run.upload(g))) return r;
        copy_ms = ms_since(t0);
        r = run.compact(g, stats, &copy_ms);
    }
    memcpy(g_last_stats, stats, sizeof g_last_stats);
    return r;
}

int srk_compact_induced(int device, void *stream, const uint32_t *d_steps, uint64_t ns, const unsigned long long *d_edges, uint64_t ne,
                        const uint8_t *d_node_base, uint64_t nn, const uint64_t *path_off, uint64_t np, SrGraph &g, uint64_t stats[8]) {
    uint64_t local[8] = {0};
    if (!stats) stats = local;
    CtDevExec x;
    CtRun<CtDevExec> run(x);
    int r;
    if ((r = dev_open(x, device, stream, 4 * nn + 16 + ns + ne)) || (r = run.reserve(nn + 1, ns, ne, np, nn))) return r;
    double copy_ms = 0;
    if ((r = run.adopt(d_steps, ns, d_edges, ne, d_node_base, nn, path_off))) return r;
    r = run.compact(g, stats, &copy_ms);
    memcpy(g_last_stats, stats, sizeof g_last_stats);
    return r;
}

void sr_compact_last_stats(uint64_t out[8]) { memcpy(out, g_last_stats, sizeof g_last_stats); }

extern "C" int sr_compact_gfa(const char *gfa_in, int device, char **gfa_out, uint64_t *n_nodes, uint64_t *n_edges, uint64_t stats[8]) {
    if (!gfa_in || !gfa_out) return sr_fail(SR_ERR_INVALID, "null argument");
    if (device < SR_COMPACT_DEVICE_TABLES_HOST) return sr_fail(SR_ERR_INVALID, "sr_compact_gfa: device must be >= -2");
    SrGraph g;
    std::vector<std::string> names;
    int r = sr_graph_parse_gfa(gfa_in, g, names);
    if (r) return r;
    uint64_t local[8] = {0};
    if (!stats) stats = local;
    if (device == SR_COMPACT_DEVICE_HOST) {
        memset(stats, 0, 8 * sizeof(uint64_t));
        const size_t before = g.node_seq.size();
        const auto t0 = std::chrono::steady_clock::now();
        do stats[0]++; while (sr_graph_compact_round(g));
        stats[2] = g.node_seq.size() - before;
        sr_graph_renumber(g);
        stats[5] = (uint64_t)(ms_since(t0) * 1000.0 + 0.5);
    } else if ((r = sr_graph_compact_tables(g, device, nullptr, stats))) return r;
    std::vector<const char *> cn;
    for (const auto &s : names) cn.push_back(s.c_str());
    *gfa_out = sr_graph_format_gfa(g, cn.data(), n_nodes, n_edges);
    return SR_OK;
}

extern "C" int sr_compact_stats(uint64_t stats[8]) {
    if (!stats) return sr_fail(SR_ERR_INVALID, "null argument");
    sr_compact_last_stats(stats);
    return SR_OK;
}
