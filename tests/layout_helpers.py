"""Independent Python restatement of the 2-D path-guided SGD layout (csrc/sr_layout_term.h,
sr_layout.cpp) for test_layout_host.py and test_layout_gpu.py: parameters, tables, initial state, term selection, the
update and the batched execution in Python floats with math.sqrt, plus the hand graphs both test files run."""
import math

import numpy as np

from sort_helpers import Gfa, mix

Y_SALT = 0x6c61796f7574
SCALE = 1048576.0


def unit(r):
    return float(r >> 11) * (1.0 / 9007199254740992.0)


class Layout:
    """everything the schedule reads, derived from a Gfa like layout_prepare does"""

    def __init__(self, g, seed=9399220, iter_max=30, theta=0.99, eps=0.01, cooling_start=0.5, space_max=100, space_quant=100,
                 min_term_updates=0, terms_per_round=65536):
        ids = sorted(g.seq)
        dense = {i: k for k, i in enumerate(ids)}
        self.seed, self.iter_max, self.space_max, self.space_quant, self.tpr = seed, iter_max, space_max, space_quant, terms_per_round
        self.node_len = [len(g.seq[i]) for i in ids]
        self.xy, acc = [], 0
        for v, i in enumerate(ids):
            ln = self.node_len[v]
            for e in (0, 1):
                self.xy.append([float(acc) + (float(ln) if e else 0.0), (unit(mix(seed ^ Y_SALT, 2 * v + e)) - 0.5) * float(ln)])
            acc += ln
        self.step_node, self.step_path, self.step_rank, self.step_pos, self.step_rev, self.first, self.nsteps = [], [], [], [], [], [], []
        max_len = 0
        for p, (_, st) in enumerate(g.paths):
            self.first.append(len(self.step_node)); self.nsteps.append(len(st))
            pos = 0
            for r, h in enumerate(st):
                self.step_node.append(dense[h >> 1]); self.step_path.append(p); self.step_rank.append(r)
                self.step_pos.append(pos); self.step_rev.append(h & 1)
                pos += len(g.seq[h >> 1])
            max_len = max(max_len, pos)
        self.S = len(self.step_node)
        self.has_terms = any(n > 1 for n in self.nsteps)
        self.mtu = min_term_updates or 10 * self.S
        self.eta_max = float(max_len) * float(max_len)
        self.space = space = max(max_len, 1)
        if self.has_terms:
            emax = 1.0 / (1.0 / self.eta_max)          # the schedule function goes through w_min = 1 / eta_max
            lam = math.log(emax / eps) / (float(iter_max) - 1.0)
            self.etas = [emax * math.exp(-lam * float(t)) for t in range(iter_max + 1)]
        self.first_cool = math.floor(cooling_start * float(iter_max))
        self.zs = zs = (space if space <= space_max else space_max + (space - space_max) // space_quant + 1) + 1
        self.zetas, self.pre = [0.0] * zs, [[0.0] * (space + 1), [0.0] * (space + 1)]
        z = zc = 0.0
        for i in range(1, space + 1):
            z += math.pow(1.0 / float(i), theta)
            zc += math.pow(1.0 / float(i), 0.001)
            self.pre[0][i], self.pre[1][i] = z, zc
            if i <= space_max:
                self.zetas[i] = z
            if i >= space_max and (i - space_max) % space_quant == 0:
                idx = space_max + 1 + (i - space_max) // space_quant
                if idx < zs:
                    self.zetas[idx] = z

    def _space_idx(self, js):
        i = self.space_max + (js - self.space_max) // self.space_quant + 1 if js > self.space_max else js
        return min(i, self.zs - 1)

    @staticmethod
    def _zipf(prefix, js, target):
        if prefix[js] < target:
            return js
        lo, hi = 1, js
        while lo < hi:
            mid = lo + (hi - lo) // 2
            if prefix[mid] >= target:
                hi = mid
            else:
                lo = mid + 1
        return lo

    def select(self, k, t, cooling):
        """(end point i, end point j, d) of term t of iteration k, or None for a skipped draw"""
        base = (k * self.mtu + t) * 6
        r0, r1, r2, r3, r4, r5 = (mix(self.seed, base + d) for d in range(6))
        step = r0 % self.S
        p = self.step_path[step]
        n = self.nsteps[p]
        if n == 1:
            return None
        ra = self.step_rank[step]
        rb = ra
        if cooling or (r1 & 1):
            prefix = self.pre[1 if cooling else 0]
            if ra > 0 and ((r2 & 1) or ra == n - 1):
                js = min(self.space, ra)
                zz = self._zipf(prefix, js, unit(r3) * self.zetas[self._space_idx(js)])
                rb = ra - zz if zz < ra else 0
            elif ra < n - 1:
                js = min(self.space, n - ra - 1)
                zz = self._zipf(prefix, js, unit(r3) * self.zetas[self._space_idx(js)])
                rb = min(ra + zz, n - 1)
        else:
            rb = r3 % n
        ea, eb = r4 & 1, r5 & 1
        if ra == rb and ea == eb:
            return None
        sa, sb = self.first[p] + ra, self.first[p] + rb
        na, nb = self.step_node[sa], self.step_node[sb]
        pos_a = float(self.step_pos[sa] + (self.node_len[na] if ea else 0))
        pos_b = float(self.step_pos[sb] + (self.node_len[nb] if eb else 0))
        d = abs(pos_a - pos_b)
        if d == 0.0:
            return None
        return 2 * na + ((1 - ea) if self.step_rev[sa] else ea), 2 * nb + ((1 - eb) if self.step_rev[sb] else eb), d

    @staticmethod
    def update(eta, d, pi, pj):
        mu = min(eta / d, 1.0)
        dx = pi[0] - pj[0]
        if dx == 0.0:
            dx = 1e-9
        dy = pi[1] - pj[1]
        mag = math.sqrt(dx * dx + dy * dy)
        r = mu * (mag - d) / 2.0 / mag
        return r * dx, r * dy

    def run_batched(self):
        """the end points [[x, y]] of the batched SGD: sub-rounds read the state as they found it, contributions summed as
        int64 in units of 2^-20 bp per end point and coordinate, x += acc * 2^-20 / cnt"""
        xy = [list(p) for p in self.xy]
        if not self.has_terms:
            return np.array(xy).reshape(-1, 4)
        E = len(xy)
        for k in range(self.iter_max + 1):
            eta, cooling = self.etas[k], k > self.first_cool
            for t0 in range(0, self.mtu, self.tpr):
                ax, ay, cnt = [0] * E, [0] * E, [0] * E
                for t in range(t0, min(self.mtu, t0 + self.tpr)):
                    sel = self.select(k, t, cooling)
                    if sel is None:
                        continue
                    i, j, d = sel
                    rx, ry = self.update(eta, d, xy[i], xy[j])
                    ax[i] += round(-rx * SCALE); ay[i] += round(-ry * SCALE); cnt[i] += 1
                    ax[j] += round(rx * SCALE); ay[j] += round(ry * SCALE); cnt[j] += 1
                for e in range(E):
                    if cnt[e]:
                        xy[e][0] = xy[e][0] + (float(ax[e]) / SCALE) / float(cnt[e])
                        xy[e][1] = xy[e][1] + (float(ay[e]) / SCALE) / float(cnt[e])
        return np.array(xy).reshape(-1, 4)


def words(xy):
    """the raw 8-byte words of a layout"""
    return np.ascontiguousarray(xy, dtype=np.float64).view(np.uint64).reshape(-1).tolist()


def initial_state(g, seed=9399220):
    return np.array(Layout(g, seed=seed, iter_max=2).xy).reshape(-1, 4)


# ---------------------------------------------------------------- hand graphs (handle = id << 1 | reverse)
def two_nodes():
    """the smallest live term: 2 nodes, 1 path"""
    return Gfa({1: "ACGTA", 2: "GG"}, [(2, 4)], [("p", [2, 4])])


def reverse_steps():
    """reverse steps, and node 2 visited in both orientations"""
    return Gfa({1: "ACG", 2: "TTTT", 3: "C", 4: "GATTA"}, [(2, 4), (4, 7), (7, 5), (5, 8), (2, 5)],
               [("a", [2, 4, 7, 5, 8]), ("b", [9, 4, 3]), ("c", [2, 5, 6])])


def repeats_and_loop():
    """node 2 repeated inside one path (same orientation: both end points of a term can be one end point) and a self-loop L line"""
    return Gfa({1: "AC", 2: "GGT", 3: "A"}, [(2, 4), (4, 4), (4, 6), (6, 4)], [("p", [2, 4, 4, 6, 4]), ("q", [4, 6])])


def hub(paths=64, shared=60):
    """`paths` paths over the same `shared` nodes plus one private node each: contended accumulators"""
    seq = {i + 1: "ACGTTGCA"[: 1 + i % 7] for i in range(shared)}
    ps, edges = [], [((i + 1) << 1, (i + 2) << 1) for i in range(shared - 1)]
    for p in range(paths):
        own = shared + 1 + p
        seq[own] = "AC"
        at = 1 + p % (shared - 1)
        st = [(i + 1) << 1 for i in range(at)] + [own << 1] + [(i + 1) << 1 for i in range(at, shared)]
        edges += [(at << 1, own << 1), (own << 1, (at + 1) << 1)]
        ps.append((f"p{p}", st))
    return Gfa(seq, edges, ps)


def chain(n=300):
    """n nodes in one path and a second path over every other node: 2 n end points, more than one workgroup of the apply pass"""
    seq = {i: "ACGT"[: 1 + i % 4] for i in range(1, n + 1)}
    a = [i << 1 for i in range(1, n + 1)]
    b = [i << 1 for i in range(1, n + 1, 2)]
    edges = [(x, y) for x, y in zip(a, a[1:])] + [(x, y) for x, y in zip(b, b[1:])]
    return Gfa(seq, edges, [("a", a), ("b", b)])


def single_steps():
    return Gfa({1: "ACG", 2: "T", 5: "GGCC"}, [(2, 4)], [("a", [2]), ("b", [5]), ("c", [10])])
