"""Inputs and restatements for the tests of the growth curves.

restate(): the curves of a *given* permutation table by Python sets over the GFA text (set union for pan, intersection for
core), bp_by_groups by counting; it shares nothing with the library and takes the permutations from the result under test,
so it checks the curves independently of how permutations are drawn.  identity_sums(): the exact sums over all G!
permutations in Python big ints.  report_of(): the bytes sr_growth_report must write for a result.  seam_cases(): graphs
built for the seams of the kernels (a node word = 64 nodes, a chunk = 4096, the histogram and rank tables, R against the
wave and the workgroup)."""
import math
from fractions import Fraction

import numpy as np

import sort_helpers as sh
import stats_helpers as st

CHUNK_NODES = 4096      # SR_GROWTH_CHUNK_NODES
MODES = ("path", "sample", "haplotype")


def groups_of(names, mode):
    """-> (group_of, group names): the PanSN rule of sr_growth_groups, restated"""
    keys, group_of = {}, []
    for p, name in enumerate(names):
        if mode == "path":
            key = (p, name)
        else:
            parts = name.split("#")
            need = 1 if mode == "sample" else 2
            key = "#".join(parts[:need]) if len(parts) > need else name
        group_of.append(keys.setdefault(key, len(keys)))
    return group_of, [k[1] if mode == "path" else k for k in keys]


def presence(text, group_of=None):
    """-> (lengths of the nodes in ascending id order, per group the set of node indices it is present on, G)"""
    g = st.parse(text)
    ids = sorted(g.seq)
    index = {i: k for k, i in enumerate(ids)}
    if group_of is None:
        group_of = list(range(len(g.paths)))
    G = max(group_of) + 1 if len(group_of) else 0
    on = [set() for _ in range(G)]
    for p, (_, steps) in enumerate(g.paths):
        on[group_of[p]].update(index[h >> 1] for h in steps)
    return [len(g.seq[i]) for i in ids], on, G


def bp_by_groups(lens, on, G):
    count = [0] * len(lens)
    for s in on:
        for v in s:
            count[v] += 1
    out = [0] * (G + 1)
    for v, c in enumerate(count):
        out[c] += lens[v]
    return out


def curves(lens, on, row):
    """pan and core along one order of the groups, by set union and intersection"""
    seen, common, pan, core = set(), None, [], []
    total = 0
    for g in row:
        fresh = on[g] - seen
        total += sum(lens[v] for v in fresh)
        seen |= fresh
        common = set(on[g]) if common is None else common & on[g]
        pan.append(total)
        core.append(sum(lens[v] for v in common))
    return pan, core


def restate(text, perm, group_of=None, rows=None):
    """-> dict(groups, length, bp_by_groups, rows: {r: (pan, core)}) for the rows asked for (default: all) of perm"""
    lens, on, G = presence(text, group_of)
    rows = range(len(perm)) if rows is None else rows
    return dict(groups=G, length=sum(lens), bp_by_groups=bp_by_groups(lens, on, G),
                rows={r: curves(lens, on, [int(g) for g in perm[r]]) for r in rows})


def assert_restated(d, text, what, group_of=None, rows=None):
    want = restate(text, d["perm"], group_of, rows)
    assert d["groups"] == want["groups"] and d["length"] == want["length"], what
    assert d["bp_by_groups"].tolist() == want["bp_by_groups"], f"{what}: bp_by_groups"
    for r, (pan, core) in want["rows"].items():
        assert d["pan"][r].tolist() == pan, f"{what}: pan of permutation {r} = {d['perm'][r].tolist()}"
        assert d["core"][r].tolist() == core, f"{what}: core of permutation {r} = {d['perm'][r].tolist()}"


def assert_same(got, want, what=""):
    """two results of growth(): every integer"""
    for k in ("length", "paths", "groups", "permutations", "exhaustive", "seed"):
        assert int(got[k]) == int(want[k]), f"{what}: {k} {got[k]} != {want[k]}"
    for k in ("pan", "core", "perm", "bp_by_groups"):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, f"{what}: shape of {k}"
        bad = np.argwhere(got[k] != want[k])
        assert len(bad) == 0, f"{what}: {k} differs in {len(bad)} cells, first at {tuple(bad[0])}: " \
                              f"{got[k][tuple(bad[0])]} != {want[k][tuple(bad[0])]}"


def assert_invariants(d, what=""):
    R, G = d["permutations"], d["groups"]
    assert d["pan"].shape == d["core"].shape == d["perm"].shape == (R, G) and d["bp_by_groups"].shape == (G + 1,), what
    assert int(d["bp_by_groups"].sum()) == d["length"], what
    if G == 0:
        return
    pan, core = d["pan"].astype(np.int64), d["core"].astype(np.int64)
    assert (np.diff(pan, axis=1) >= 0).all() and (np.diff(core, axis=1) <= 0).all(), f"{what}: monotony"
    assert (pan[:, 0] == core[:, 0]).all() and (core <= pan).all(), what
    assert (pan[:, -1] == d["length"] - int(d["bp_by_groups"][0])).all(), f"{what}: pan(G)"
    assert (core[:, -1] == int(d["bp_by_groups"][G])).all(), f"{what}: core(G)"
    assert (np.sort(d["perm"], axis=1) == np.arange(G, dtype=np.uint32)[None, :]).all(), f"{what}: a row of perm is no permutation"


def identity_sums(bp, k):
    """sum over all G! orders of pan(k) and of core(k), exact, from the histogram"""
    G = len(bp) - 1
    f = math.factorial
    pan = sum(int(bp[c]) * (f(G) - math.comb(G - c, k) * f(k) * f(G - k)) for c in range(G + 1))
    core = sum(int(bp[c]) * math.comb(c, k) * f(k) * f(G - k) for c in range(G + 1))
    return pan, core


def assert_exhaustive(d, what=""):
    """all G! rows in lexicographic order, and the integer identity for every k"""
    import itertools
    G = d["groups"]
    assert d["exhaustive"] == 1 and d["permutations"] == math.factorial(G), what
    if G <= 6:
        assert d["perm"].tolist() == [list(p) for p in itertools.permutations(range(G))], f"{what}: order of the rows"
    else:
        rows = [tuple(r) for r in d["perm"].tolist()]
        assert rows == sorted(rows) and len(set(rows)) == len(rows), f"{what}: order of the rows"
    for k in range(1, G + 1):
        pan, core = identity_sums(d["bp_by_groups"], k)
        assert sum(int(x) for x in d["pan"][:, k - 1]) == pan, f"{what}: sum of pan({k})"
        assert sum(int(x) for x in d["core"][:, k - 1]) == core, f"{what}: sum of core({k})"


def expected_exact(bp, k):
    """E pan(k), E core(k) as Fractions"""
    G = len(bp) - 1
    pan = sum(int(bp[c]) * (1 - Fraction(math.comb(G - c, k), math.comb(G, k))) for c in range(G + 1))
    core = sum(int(bp[c]) * Fraction(math.comb(c, k), math.comb(G, k)) for c in range(G + 1))
    return pan, core


def report_of(d, pan_exp, core_exp, fit):
    """the bytes sr_growth_report must write for the integers of d; the expectations and the fit are given (they have
    tests of their own), mean and sd are restated: sums in Python ints, one division and one square root in double"""
    R, G = d["permutations"], d["groups"]
    alpha, kappa, points = fit
    ok = points >= 2
    out = [f"#seqrush_amd growth v1\tgroups={G}\tpaths={d['paths']}\tpermutations={R}\texhaustive={d['exhaustive']}\tseed={d['seed']}"
           f"\tlength={d['length']}\n",
           f"#classes\tunused={int(d['bp_by_groups'][0])}\tcore={int(d['bp_by_groups'][G])}\n",
           "#heaps\talpha=" + ("%.6f" % alpha if ok else "NA") + "\tkappa=" + ("%.6f" % kappa if ok else "NA") + f"\tpoints={points}\t" +
           (("open" if alpha <= 1.0 else "closed") if ok else "NA") + "\n",
           "k\tpan_exp\tcore_exp\tpan_mean\tpan_sd\tpan_min\tpan_max\tcore_mean\tcore_sd\tcore_min\tcore_max\n"]

    def column(tab, k):
        v = [int(x) for x in tab[:, k]]
        s, s2 = sum(v), sum(x * x for x in v)
        return "%.6f\t%.6f\t%d\t%d" % (float(s) / float(R), math.sqrt(float(R * s2 - s * s) / float(R * R)), min(v), max(v))
    for k in range(G):
        out.append("%d\t%.6f\t%.6f\t%s\t%s\n" % (k + 1, pan_exp[k], core_exp[k], column(d["pan"], k), column(d["core"], k)))
    return "".join(out)


# ------------------------------------------------------------------ inputs
def rename_paths(text, names):
    """the same graph with its P lines named `names` in order"""
    out, k = [], 0
    for line in text.split("\n"):
        f = line.split("\t")
        if f[0] == "P":
            f[1] = names[k]
            k += 1
            line = "\t".join(f)
        out.append(line)
    assert k == len(names)
    return "\n".join(out)


PANSN = ["a#1#c1", "a#2#c1", "b#1#x", "plain", "a#1#c2", "b#1#y", "c#2#z", "plain#", "b#2#x", "c#2#w", "d", "a#2#c3"]


def host_inputs():
    """every input of the statistics tests: (name, GFA text)"""
    from test_stats_host import GOLDEN
    out = [("golden:" + c["name"], c["gfa"]) for c in GOLDEN]
    out += [("random:%d" % c[0], st.random_gfa(c[0], c[1], c[2], c[3], sparse_ids=c[0] % 2 == 0)) for c in st.RANDOM_CASES]
    out += [("hand:" + n, t) for n, t in sorted(st.hand_cases().items())]
    return out


def small_random(G, seed):
    """a random graph of G paths on 30 nodes: reverse steps, revisits, nodes on no path"""
    return st.random_gfa(1000 + 10 * seed + G, 30, G, 12)


def _gfa(lens, paths):
    return sh.Gfa({i + 1: "ACGT"[i % 4] * n for i, n in enumerate(lens)}, [], paths).text()


def shaped(V, G, seed, steps=40, backbone=3):
    """V nodes, G one-path groups: every path a random walk of `steps` steps in both orientations plus the `backbone`
    nodes spread over the graph (first, middle, last ...), which are therefore core; most of a large graph is on no path"""
    rng = np.random.default_rng(seed)
    lens = [int(x) for x in rng.integers(1, 41, size=V)]
    spine = sorted({int(x) for x in np.linspace(1, V, num=min(backbone, V))})
    paths = []
    for g in range(G):
        k = int(rng.integers(0, V))
        walk = []
        for _ in range(min(steps, 2 * V)):
            walk.append(((k + 1) << 1) | int(rng.integers(0, 2)))
            k = int(rng.integers(0, V)) if rng.random() < 0.2 else (k + int(rng.integers(0, 3))) % V
        paths.append((f"g{g}", walk + [v << 1 for v in spine]))
    return _gfa(lens, paths)


def all_private(V, G):
    """node v is on the path of group v mod G alone: every column brings something new, nothing is ever lost after k = 2"""
    rng = np.random.default_rng(V * 131 + G)
    lens = [int(x) for x in rng.integers(1, 41, size=V)]
    return _gfa(lens, [(f"g{g}", [v << 1 for v in range(1, V + 1) if v % G == g]) for g in range(G)])


def all_core(V, G):
    """every path visits every node: everything is new at k = 1 and nothing is ever lost"""
    rng = np.random.default_rng(V * 137 + G)
    lens = [int(x) for x in rng.integers(1, 41, size=V)]
    return _gfa(lens, [(f"g{g}", [(v << 1) | ((v + g) & 1) for v in range(1, V + 1)]) for g in range(G)])


def seam_cases():
    """name -> (GFA text, permutations asked for): V over the word and chunk edges, G over the histogram and rank-table
    edges, R over sizes that are no multiple of the wave or the workgroup"""
    cases = {}
    for V in (1, 63, 64, 65, 4095, 4097):
        cases[f"V{V}_G9_R70"] = (shaped(V, 9, V), 70)
    for G in (1, 2, 63, 64, 65, 130):
        cases[f"V4097_G{G}_R70"] = (shaped(4097, G, 50 + G), 70)
    for R in (1, 70, 257):
        cases[f"V65_G64_R{R}"] = (shaped(65, 64, 7), R)
    cases["V4097_G130_R257"] = (shaped(4097, 130, 11, steps=120), 257)
    cases["V9000_G12_R257"] = (shaped(9000, 12, 12, steps=3000, backbone=40), 257)      # three chunks, dense columns
    return cases
