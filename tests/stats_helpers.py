"""A third statement of the statistics of DESIGN.md section 11 that shares nothing with the library: dicts, sets and Python
ints over sort_helpers.Gfa.parse.  Plus a seeded generator of random GFA text and the comparison the tests use."""
import numpy as np

import sort_helpers as sh


def parse(text):
    """sort_helpers.Gfa.parse, with the paths of zero steps (which it cannot read) put back in their places"""
    lines = text.split("\n")
    empty, kept, k = [], [], 0
    for line in lines:
        f = line.split("\t")
        if f[0] == "P":
            if len(f) > 2 and f[2] == "":
                empty.append((k, f[1]))
                k += 1
                continue
            k += 1
        kept.append(line)
    g = sh.Gfa.parse("\n".join(kept))
    for k, name in empty:
        g.paths.insert(k, (name, []))
    return g


def stats(g):
    """every quantity of the definitions -> dict of Python ints and lists (nodes in ascending id order)"""
    ids = sorted(g.seq)
    ln = {i: len(g.seq[i]) for i in ids}
    edges = set(g.edges)
    P = len(g.paths)
    d = dict(length=sum(ln.values()), nodes=len(ids), edges=len(edges), paths=P, steps=sum(len(st) for _, st in g.paths))
    depth = {i: 0 for i in ids}
    on = {i: set() for i in ids}
    rev = 0
    for p, (_, st) in enumerate(g.paths):
        for h in st:
            depth[h >> 1] += 1
            on[h >> 1].add(p)
            rev += h & 1
    d["rev_steps"] = rev
    d["depth_bp"] = sum(depth[i] * ln[i] for i in ids)
    d["depth"] = [depth[i] for i in ids]
    d["paths_on"] = [len(on[i]) for i in ids]
    d["bp_by_paths"] = [sum(ln[i] for i in ids if len(on[i]) == c) for c in range(P + 1)]
    d["nodes_by_paths"] = [sum(1 for i in ids if len(on[i]) == c) for c in range(P + 1)]
    visited = [{h >> 1 for h in st} for _, st in g.paths]
    d["shared"] = [[sum(ln[v] for v in visited[i] & visited[j]) for j in range(P)] for i in range(P)]
    pos, acc = {}, 0
    for i in ids:
        pos[i] = acc
        acc += ln[i]
    pairs, sabs, ssq, plen = [], [], [], []
    for _, st in g.paths:
        es = [abs(abs(pos[b >> 1] - pos[a >> 1]) - ln[a >> 1]) for a, b in zip(st, st[1:])]
        pairs.append(len(es))
        sabs.append(sum(es))
        ssq.append(sum(e * e for e in es))
        plen.append(sum(ln[a >> 1] for a in st[:-1]))
    d.update(path_pairs=pairs, path_abs=sabs, path_sq=ssq, path_len=plen, total_pairs=sum(pairs), total_abs=sum(sabs),
             total_sq=sum(ssq), total_len=sum(plen))
    d["self_loops"] = sum(1 for a, b in edges if a >> 1 == b >> 1)
    touched = set()
    for a, b in edges:
        touched.add((a >> 1, "L" if a & 1 else "R"))
        touched.add((b >> 1, "R" if b & 1 else "L"))
    d["tips"] = sum(1 for i in ids for side in "LR" if (i, side) not in touched)
    comp = {i: {i} for i in ids}
    for a, b in edges:
        ca, cb = comp[a >> 1], comp[b >> 1]
        if ca is not cb:
            ca |= cb
            for v in cb:
                comp[v] = ca
    d["components"] = len({id(c) for c in comp.values()})
    return d


INT_KEYS = ("length", "nodes", "edges", "paths", "steps", "rev_steps", "depth_bp", "self_loops", "tips", "components",
            "total_pairs", "total_abs", "total_sq", "total_len")
LIST_KEYS = ("depth", "paths_on", "bp_by_paths", "nodes_by_paths", "path_pairs", "path_abs", "path_sq", "path_len")


def as_plain(d):
    """a result of seqrush.graph_stats or of stats() -> the comparable part, Python ints only"""
    out = {k: int(d[k]) for k in INT_KEYS}
    for k in LIST_KEYS:
        out[k] = [int(x) for x in d[k]]
    out["shared"] = [[int(x) for x in row] for row in d["shared"]]
    return out


def assert_equal(got, want, what=""):
    got, want = as_plain(got), as_plain(want)
    for k in want:
        assert got[k] == want[k], f"{what}: {k} differs"


def random_gfa(seed, n_nodes, n_paths, steps_per_path=None, extra_edges=5, sparse_ids=False):
    """seeded random GFA text: node lengths 1..40, paths as random walks in both orientations, edges from consecutive
    steps plus a few extra ones (some repeated as duplicate L lines)"""
    rng = np.random.default_rng(seed)
    ids = list(range(1, n_nodes + 1))
    if sparse_ids:
        ids = sorted(int(x) for x in rng.choice(np.arange(1, 50 * n_nodes + 50), size=n_nodes, replace=False))
    lens = rng.integers(1, 41, size=n_nodes)
    seq = {i: "ACGT"[k % 4] * int(lens[k]) for k, i in enumerate(ids)}
    paths, edges = [], []
    for p in range(n_paths):
        m = int(steps_per_path if steps_per_path is not None else rng.integers(1, max(3, 2 * n_nodes // max(1, n_paths) + 3)))
        k = int(rng.integers(0, n_nodes))
        st = []
        for _ in range(m):
            st.append((ids[k] << 1) | int(rng.integers(0, 2)))
            k = int(rng.integers(0, n_nodes)) if rng.random() < 0.1 else (k + int(rng.integers(-2, 4))) % n_nodes
        paths.append((f"p{p}", st))
        edges += list(zip(st, st[1:]))
    for _ in range(extra_edges):
        a, b = (int(x) for x in rng.integers(0, n_nodes, size=2))
        edges.append(((ids[a] << 1) | int(rng.integers(0, 2)), (ids[b] << 1) | int(rng.integers(0, 2))))
    return sh.Gfa(seq, edges, paths).text()


# (seed, nodes, paths, steps per path): P at the bitset word and tile boundaries; V from 1 to ~3000, the largest spanning
# many similarity node chunks (64 nodes each) with a remainder
RANDOM_CASES = [(1, 1, 1, 3), (2, 7, 2, None), (3, 40, 63, None), (4, 130, 64, None), (5, 300, 65, None), (6, 500, 129, 40),
                (7, 2999, 129, 300), (8, 2050, 2, 3000), (9, 1025, 65, 100)]


def hand_cases():
    """name -> GFA text of the hand-made cases"""
    G = sh.Gfa
    big = "A" * 70000
    cases = {
        "revisit_both_orientations": G({1: "AC", 2: "GGG", 3: "T"}, [(2, 4), (4, 7), (7, 5), (5, 2)], [("p", [2, 4, 7, 5, 2, 4])]).text(),
        "nodes_on_no_path": G({1: "AC", 2: "GGG", 3: "T", 4: "CCCC"}, [(2, 4), (6, 8)], [("p", [2, 4]), ("q", [4])]).text(),
        "sparse_ids": G({5: "ACG", 9: "T", 1000000: "GGGGG"}, [(10, 18), (18, 2000001)], [("a", [10, 18, 2000001]), ("b", [2000000, 10])]).text(),
        "duplicate_l_lines": G({1: "A", 2: "CC", 3: "G"}, [(2, 4), (2, 4), (4, 6), (2, 4), (4, 6)], [("p", [2, 4, 6])]).text(),
        "self_loops": G({1: "AAA", 2: "C"}, [(2, 2), (2, 3), (5, 4), (2, 4)], [("p", [2, 2, 4]), ("q", [2, 3])]).text(),
        "isolated_node": G({1: "A", 2: "CC", 3: "GGG"}, [(2, 4)], [("p", [2, 4])]).text(),
        "three_components": G({1: "A", 2: "CC", 3: "G", 4: "TT", 5: "ACGT", 6: "C", 7: "G"}, [(2, 4), (6, 9), (8, 6), (10, 13), (12, 14)],
                              [("a", [2, 4]), ("b", [6, 9]), ("c", [10, 13, 14])]).text(),
        "node_of_70000_bp": G({1: "AC", 2: big, 3: "T", 4: "GG"}, [(2, 6), (6, 4), (4, 8), (8, 2)],
                              [("a", [2, 6, 4, 8, 2]), ("b", [8, 2, 6]), ("c", [4, 8])]).text(),
    }
    cases["empty_and_one_step_paths"] = ("H\tVN:Z:1.0\nS\t1\tACG\nS\t2\tTT\nL\t1\t+\t2\t+\t0M\nP\te0\t\t*\nP\ta\t1+,2+\t*\nP\tone\t2-\t*\n"
                                         "P\te1\t\t*\n")
    return cases
