"""Independent Python restatements for the Ygs-layout tests (test_sort_host.py, test_sort_gpu.py): GFA parsing, the
reference's layout quality metric (src/bin/measure_layout_quality.rs:100-200), the BFS groom, the head-seeded
topological sort, apply_ordering, the batched deterministic SGD and the checks that a sorted graph is the same graph."""
import math

import numpy as np

COMP = {**{c: c for c in map(chr, range(256))}, "A": "T", "a": "T", "T": "A", "t": "A", "C": "G", "c": "G",
        "G": "C", "g": "C", "N": "N", "n": "N"}


def rc(s):
    return "".join(COMP[c] for c in reversed(s))


class Gfa:
    """S / L / P lines: seq {id: str}, edges [(from_handle, to_handle)], paths [(name, [handle])]; handle = id << 1 | rev"""

    def __init__(self, seq, edges, paths):
        self.seq, self.edges, self.paths = dict(seq), list(edges), [(n, list(s)) for n, s in paths]

    @staticmethod
    def parse(text):
        seq, edges, paths = {}, [], []
        for line in text.strip().split("\n"):
            f = line.split("\t")
            if f[0] == "S":
                seq[int(f[1])] = f[2]
            elif f[0] == "L":
                edges.append(((int(f[1]) << 1) | (f[2] == "-"), (int(f[3]) << 1) | (f[4] == "-")))
            elif f[0] == "P":
                paths.append((f[1], [(int(s[:-1]) << 1) | (s[-1] == "-") for s in f[2].split(",")]))
        return Gfa(seq, edges, paths)

    def text(self):
        out = ["H\tVN:Z:1.0"] + [f"S\t{i}\t{self.seq[i]}" for i in sorted(self.seq)]
        out += [f"L\t{a >> 1}\t{'-' if a & 1 else '+'}\t{b >> 1}\t{'-' if b & 1 else '+'}\t0M" for a, b in self.edges]
        out += [f"P\t{n}\t" + ",".join(f"{h >> 1}{'-' if h & 1 else '+'}" for h in st) + "\t*" for n, st in self.paths]
        return "\n".join(out) + "\n"

    def spell(self, steps):
        return "".join(rc(self.seq[h >> 1]) if h & 1 else self.seq[h >> 1] for h in steps)

    def relabel(self, m):
        """m: old id -> new id"""
        f = lambda h: (m[h >> 1] << 1) | (h & 1)   # noqa: E731
        return Gfa({m[i]: s for i, s in self.seq.items()}, [(f(a), f(b)) for a, b in self.edges],
                   [(n, [f(h) for h in st]) for n, st in self.paths])

    def permuted(self, seed):
        ids = sorted(self.seq)
        perm = np.random.default_rng(seed).permutation(len(ids))
        m = {ids[i]: int(perm[i]) + 1 for i in range(len(ids))}
        return self.relabel(m), m


def acyclic_forward(g):
    """every edge and step forward and no directed cycle"""
    if any((a | b) & 1 for a, b in g.edges) or any(h & 1 for _, st in g.paths for h in st):
        return False
    out, indeg = {}, {i: 0 for i in g.seq}
    for a, b in set(g.edges):
        out.setdefault(a >> 1, []).append(b >> 1)
        indeg[b >> 1] += 1
    ready, seen = [i for i, d in indeg.items() if d == 0], 0
    while ready:
        u = ready.pop()
        seen += 1
        for v in out.get(u, []):
            indeg[v] -= 1
            if indeg[v] == 0:
                ready.append(v)
    return seen == len(g.seq)


def quality(g):
    """mean over consecutive step pairs of | |pos_b - pos_a| - len(node_a) |, nodes laid out by cumulative length in id order"""
    pos, acc = {}, 0
    for i in sorted(g.seq):
        pos[i] = acc
        acc += len(g.seq[i])
    tot, n = 0.0, 0
    for _, st in g.paths:
        for a, b in zip(st, st[1:]):
            tot += abs(abs(pos[b >> 1] - pos[a >> 1]) - len(g.seq[a >> 1]))
            n += 1
    return tot / max(n, 1)


def spearman(a, b):
    ra = np.argsort(np.argsort(np.asarray(a), kind="stable"), kind="stable")
    rb = np.argsort(np.argsort(np.asarray(b), kind="stable"), kind="stable")
    return float(np.corrcoef(ra, rb)[0, 1])


# ---------------------------------------------------------------- groom, topological sort, apply_ordering
def find_heads(g):
    """src/bidirected_ops.rs:1317-1345"""
    has_in = {b >> 1 for _, b in g.edges}
    first = {}
    for _, st in g.paths:
        for r, h in enumerate(st):
            first[h >> 1] = min(first.get(h >> 1, r), r)
    heads = [i for i in sorted(g.seq) if i not in has_in]
    heads.sort(key=lambda i: (first.get(i, float("inf")), i))
    return [i << 1 for i in heads]


def groom(g):
    """BFS groom (src/groom.rs:49-200, 253-300) + apply_grooming_with_reorder(false) (:613-...) -> new Gfa"""
    out = {}
    for a, b in g.edges:
        out.setdefault(a, []).append(b)
    visited, flipped = set(), set()
    seeds = find_heads(g) or ([min(g.seq) << 1] if g.seq else [])
    while True:
        if not seeds:
            rest = [i for i in sorted(g.seq) if i not in visited]
            if not rest:
                break
            seeds = [rest[0] << 1]
        queue = []
        for s in seeds:
            if (s >> 1) not in visited:
                visited.add(s >> 1)
                if s & 1:
                    flipped.add(s >> 1)
                queue.append(s)
        qi = 0
        while qi < len(queue):
            cur = queue[qi]
            qi += 1
            for nxt in sorted(out.get(cur, [])):
                if (nxt >> 1) not in visited:
                    visited.add(nxt >> 1)
                    if nxt & 1:
                        flipped.add(nxt >> 1)
                    queue.append(nxt)
        seeds = []
    f = lambda h: h ^ 1 if (h >> 1) in flipped else h   # noqa: E731
    return Gfa({i: rc(s) if i in flipped else s for i, s in g.seq.items()}, [(f(a), f(b)) for a, b in g.edges],
               [(n, [f(h) for h in st]) for n, st in g.paths])


def topo_order(g):
    """exact_odgi_topological_order(use_heads=True, use_tails=False), src/bidirected_ops.rs:1390-1599, literally
    (edges scanned in sorted order, sets as sorted containers)"""
    edges = sorted(set(g.edges))
    unvisited = set()
    for i in g.seq:
        unvisited.add(i << 1)
        unvisited.add((i << 1) | 1)
    S, seeds, masked, visited_nodes, out = set(), [], set(), set(), []
    for h in find_heads(g):
        S.add(h)
        unvisited.discard(h)
        unvisited.discard(h ^ 1)
    while unvisited or S:
        if not S:
            found = False
            if seeds:
                seeds.sort()
                h = seeds.pop(0)
                if h in unvisited:
                    S.add(h); unvisited.discard(h); unvisited.discard(h ^ 1); found = True
            if not found and unvisited:
                h = min(unvisited)
                S.add(h); unvisited.discard(h); unvisited.discard(h ^ 1)
        while S:
            h = min(S)
            S.discard(h)
            if (h >> 1) not in visited_nodes:
                visited_nodes.add(h >> 1)
                out.append(h >> 1)
            for e in edges:
                if e[1] == h and e not in masked:
                    masked.add(e)
            for e in edges:
                if e[0] == h and e not in masked:
                    masked.add(e)
                    nxt = e[1]
                    if nxt in unvisited:
                        if not any(o[1] == nxt and o not in masked for o in edges):
                            S.add(nxt); unvisited.discard(nxt); unvisited.discard(nxt ^ 1)
                        elif nxt not in seeds:
                            seeds.append(nxt)
    return out


def apply_ordering(g, order):
    return g.relabel({old: r + 1 for r, old in enumerate(order)})


def groom_topo(g):
    """g + s of the Ygs layout (no SGD), as the library writes it: edges sorted"""
    t = groom(g)
    t = apply_ordering(t, topo_order(t))
    t.edges.sort()
    return t


# ---------------------------------------------------------------- the batched deterministic SGD (sr_sgd_term.h)
M64 = (1 << 64) - 1


def mix(seed, idx):
    z = (seed + (idx + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def sgd_batched(g, seed, iter_max, terms_per_round, theta=0.99, eps=0.01, cooling_start=0.5, space_max=100, space_quant=100):
    """positions (ascending id order) of the batched SGD: sub-rounds read the positions as they found them, contributions
    summed as int64 in units of 2^-20 bp, x += acc * 2^-20 / cnt"""
    ids = sorted(g.seq)
    dense = {i: k for k, i in enumerate(ids)}
    x, acc = [], 0
    for i in ids:
        x.append(float(acc))
        acc += len(g.seq[i])
    step_node, step_path, step_rank, step_pos, first, nsteps = [], [], [], [], [], []
    max_steps = max_len = 0
    for p, (_, st) in enumerate(g.paths):
        first.append(len(step_node)); nsteps.append(len(st))
        pos = 0
        for r, h in enumerate(st):
            step_node.append(dense[h >> 1]); step_path.append(p); step_rank.append(r); step_pos.append(pos)
            pos += len(g.seq[h >> 1])
        max_steps, max_len = max(max_steps, len(st)), max(max_len, pos)
    S = len(step_node)
    mtu, eta_max, space = S, float(max_steps * max_steps), max_len
    w_min = 1.0 / eta_max
    emax, emin = 1.0 / w_min, eps / 1.0
    lam = math.log(emax / emin) / (float(iter_max) - 1.0)
    etas = [emax * math.exp(-lam * float(t)) for t in range(iter_max + 1)]
    first_cool = math.floor(cooling_start * float(iter_max))
    zs = (space if space <= space_max else space_max + (space - space_max) // space_quant + 1) + 1
    zetas, pre = [0.0] * zs, [[0.0] * (space + 1), [0.0] * (space + 1)]
    z = zc = 0.0
    for i in range(1, space + 1):
        z += math.pow(1.0 / float(i), theta)
        zc += math.pow(1.0 / float(i), 0.001)
        pre[0][i], pre[1][i] = z, zc
        if i <= space_max:
            zetas[i] = z
        if i >= space_max and (i - space_max) % space_quant == 0:
            idx = space_max + 1 + (i - space_max) // space_quant
            if idx < zs:
                zetas[idx] = z

    def space_idx(js):
        i = space_max + (js - space_max) // space_quant + 1 if js > space_max else js
        return min(i, zs - 1)

    def zipf(prefix, js, target):
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

    def unit(r):
        return float(r >> 11) * (1.0 / 9007199254740992.0)

    N = len(ids)
    for k in range(iter_max + 1):
        eta, cooling = etas[k], k > first_cool
        for t0 in range(0, mtu, terms_per_round):
            accs, cnt = [0] * N, [0] * N
            for t in range(t0, min(mtu, t0 + terms_per_round)):
                base = (k * mtu + t) * 4
                r0, r1, r2, r3 = (mix(seed, base + d) for d in range(4))
                step = r0 % S
                p = step_path[step]
                n = nsteps[p]
                if n == 1:
                    continue
                ra = step_rank[step]
                rb = ra
                if cooling or (r1 & 1):
                    prefix = pre[1 if cooling else 0]
                    if ra > 0 and ((r2 & 1) or ra == n - 1):
                        js = min(space, ra)
                        zz = zipf(prefix, js, unit(r3) * zetas[space_idx(js)])
                        rb = ra - zz if zz < ra else 0
                    elif ra < n - 1:
                        js = min(space, n - ra - 1)
                        zz = zipf(prefix, js, unit(r3) * zetas[space_idx(js)])
                        rb = min(ra + zz, n - 1)
                else:
                    rb = r3 % n
                if ra == rb:
                    continue
                sa, sb = first[p] + ra, first[p] + rb
                d = abs(float(step_pos[sa]) - float(step_pos[sb]))
                if d == 0.0:
                    continue
                mu = min(eta * (1.0 / d), 1.0)
                i, j = step_node[sa], step_node[sb]
                dx = x[i] - x[j]
                if dx == 0.0:
                    dx = 1e-9
                mag = abs(dx)
                rx = (mu * (mag - d) / 2.0) / mag * dx
                accs[i] += round(-rx * 1048576.0); cnt[i] += 1
                accs[j] += round(rx * 1048576.0); cnt[j] += 1
            for q in range(N):
                if cnt[q]:
                    x[q] = x[q] + (float(accs[q]) / 1048576.0) / float(cnt[q])
    return np.array(x)


# ---------------------------------------------------------------- same-graph checks
def check_same_graph(before, after, want_spellings=None):
    """after is a relabelling (node ids dense 1..N) of before with some nodes flipped: every path spells what it spelled,
    node sequences match as a multiset up to reverse complement, edges map one to one"""
    assert sorted(after.seq) == list(range(1, len(after.seq) + 1)), "node ids are not dense 1..N"
    assert len(after.seq) == len(before.seq) and len(after.paths) == len(before.paths)
    for (nb, sb), (na, sa) in zip(before.paths, after.paths):
        assert nb == na and len(sb) == len(sa)
        assert after.spell(sa) == (want_spellings[nb] if want_spellings else before.spell(sb)), f"path {na} spells otherwise"

    def canon(s):
        return min(s, rc(s))
    assert sorted(canon(s) for s in before.seq.values()) == sorted(canon(s) for s in after.seq.values())
    # relabelling and flips read off the paths: every node of `before` is visited by some path in these inputs
    m, flip = {}, {}
    for (_, sb), (_, sa) in zip(before.paths, after.paths):
        for hb, ha in zip(sb, sa):
            o, fl = hb >> 1, (hb ^ ha) & 1
            assert m.setdefault(o, ha >> 1) == ha >> 1 and flip.setdefault(o, fl) == fl, "inconsistent relabelling"
    for o, n_ in m.items():
        assert after.seq[n_] == (rc(before.seq[o]) if flip[o] else before.seq[o])

    def mapped(h):
        return (m[h >> 1] << 1) | ((h & 1) ^ flip[h >> 1])
    eb = sorted((mapped(a), mapped(b)) for a, b in before.edges)
    assert eb == sorted(after.edges), "edges do not map one to one"
