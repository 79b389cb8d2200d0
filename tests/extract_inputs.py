"""Inputs and restatements for the tests of the subgraph extraction.

restate(): the rule in Python dicts, sets and lists over stats_helpers.parse: seeds base by base (a dict from each base of a
region to its node), context by set operations over the distinct L lines, merge with lists per path, the output by
counting.  It reads the BED lines and the region strings itself and shares nothing with the library.  report_of(): the GFA
bytes sr_extract_text must write for a result.  with_edges(): a graph with the L lines its paths walk.  random_regions():
seeded regions on a graph.  seam_cases(): graphs and regions built for the seams of the kernels."""
import numpy as np

import sort_helpers as sh
import stats_helpers as st
import variants_inputs as vi

BLOCK = 256             # EX_BLOCK: steps, nodes and edges per workgroup
NONE = 0xffffffff       # level: not kept
COUNTERS = ("regions", "unknown", "out_of_range", "in_nodes", "in_edges", "in_steps", "in_paths", "nodes", "edges", "subpaths", "steps", "bases",
            "seeds", "by_context", "by_merge", "merge_rounds_run")
TABLES = ("level", "node_old", "edge_from", "edge_to", "sub_path", "sub_start", "sub_end", "sub_off", "sub_steps")


class Invalid(Exception):
    """what the library answers with SR_ERR_INVALID"""


def read_bed(bed, names, plen):
    """-> (regions [(path, start, end)], unknown, out_of_range); Invalid names the line"""
    regions, unknown, out_of_range = [], 0, 0
    for no, line in enumerate(bed.split("\n"), 1):
        if line.endswith("\r"):
            line = line[:-1]
        if not line.strip(" \t") or line.startswith(("#", "track", "browser")):
            continue
        f = line.split("\t") if "\t" in line else line.split()
        if len(f) < 3:
            raise Invalid(f"BED line {no}: fewer than three fields")
        for what, x in (("start", f[1]), ("end", f[2])):
            if not (x.isascii() and x.isdigit()) or int(x) >= 2 ** 64:
                raise Invalid(f"BED line {no}: {what} '{x}' is not a number")
        start, end = int(f[1]), int(f[2])
        if f[0] not in names:
            unknown += 1
        elif start >= end or end > plen[names.index(f[0])]:
            out_of_range += 1
        else:
            regions.append((names.index(f[0]), start, end))
    return regions, unknown, out_of_range


def _number(x):
    return x.isascii() and x.isdigit() and int(x) < 2 ** 64


def read_strings(strings, names, plen):
    """-> (regions, out_of_range); Invalid names the string"""
    regions, out_of_range = [], 0
    for s in strings:
        if s in names:
            p = names.index(s)
            if plen[p]:
                regions.append((p, 0, plen[p]))
            else:
                out_of_range += 1
            continue
        name, colon, rng = s.rpartition(":")
        if not colon:
            raise Invalid(f"region '{s}': no path has this name")
        a, dash, b = rng.partition("-")
        if not dash or not _number(a) or not _number(b):
            raise Invalid(f"region '{s}': '{rng}' is not START-END")
        if name not in names:
            raise Invalid(f"region '{s}': no path is named '{name}'")
        p, a, b = names.index(name), int(a), int(b)
        if a >= b:
            raise Invalid(f"region '{s}': start must lie below end")
        if b > plen[p]:
            raise Invalid(f"region '{s}': end lies beyond the {plen[p]} bases of the path")
        regions.append((p, a, b))
    return regions, out_of_range


def restate(text, regions=(), bed=None, c=0, D=100000, R=3):
    """-> dict with the fields of seqrush_amd.extract() that the rule fixes, as Python ints and lists"""
    g = st.parse(text)
    ids = sorted(g.seq)
    rank = {v: k + 1 for k, v in enumerate(ids)}
    ln = {v: len(g.seq[v]) for v in ids}
    names = [n for n, _ in g.paths]
    plen = [sum(ln[h >> 1] for h in s) for _, s in g.paths]
    edges = list(dict.fromkeys(g.edges))                       # the distinct L lines, first seen first
    regs, unknown, out_of_range = read_bed(bed, names, plen) if bed is not None else ([], 0, 0)
    more, oor = read_strings([regions] if isinstance(regions, str) else list(regions), names, plen)
    regs, out_of_range = regs + more, out_of_range + oor
    # seeds, base by base
    node_at, level = {}, {}
    for p, start, end in regs:
        if p not in node_at:
            node_at[p] = [h >> 1 for h in g.paths[p][1] for _ in range(ln[h >> 1])]
        where = {b: node_at[p][b] for b in range(start, end)}
        for v in where.values():
            level[v] = 0
    # context, by sets
    for r in range(1, c + 1):
        front, have = {v for v, x in level.items() if x == r - 1}, set(level)
        new = {b >> 1 for a, b in edges if a >> 1 in front and a >> 1 != b >> 1} | {a >> 1 for a, b in edges if b >> 1 in front and a >> 1 != b >> 1}
        new -= have
        if not new:
            break
        for v in new:
            level[v] = r
    # merge, with lists
    rounds = 0
    for k in range(1, R + 1):
        kept, add = set(level), []
        for _, steps in g.paths:
            at = [i for i, h in enumerate(steps) if h >> 1 in kept]
            for i, j in zip(at, at[1:]):
                run = [h >> 1 for h in steps[i + 1:j]]
                if run and sum(ln[v] for v in run) <= D:
                    add += run
        if not add:
            break
        for v in add:
            level[v] = c + k
        rounds += 1
    # the result, by counting
    kept = sorted(level)
    new_id = {v: k + 1 for k, v in enumerate(kept)}

    def handle(h):
        return (new_id[h >> 1] << 1) | (h & 1)
    out_edges = [(handle(a), handle(b)) for a, b in edges if a >> 1 in new_id and b >> 1 in new_id]
    sub_path, sub_start, sub_end, sub_off, sub_steps = [], [], [], [0], []
    for p, (_, steps) in enumerate(g.paths):
        pos, open_ = 0, False
        for h in steps:
            if h >> 1 in new_id:
                if not open_:
                    sub_path.append(p)
                    sub_start.append(pos)
                    sub_end.append(pos)
                    sub_off.append(sub_off[-1])
                    open_ = True
                sub_steps.append(handle(h))
                sub_off[-1] += 1
                sub_end[-1] = pos + ln[h >> 1]
            else:
                open_ = False
            pos += ln[h >> 1]
    return dict(regions=len(regs), unknown=unknown, out_of_range=out_of_range, in_nodes=len(ids), in_edges=len(edges),
                in_steps=sum(len(s) for _, s in g.paths), in_paths=len(names), nodes=len(kept), edges=len(out_edges), subpaths=len(sub_path),
                steps=len(sub_steps), bases=sum(ln[v] for v in kept), seeds=sum(1 for x in level.values() if x == 0),
                by_context=sum(1 for x in level.values() if 0 < x <= c), by_merge=sum(1 for x in level.values() if x > c), merge_rounds_run=rounds,
                level=[level.get(v, NONE) for v in ids], node_old=[rank[v] for v in kept], edge_from=[a for a, _ in out_edges],
                edge_to=[b for _, b in out_edges], sub_path=sub_path, sub_start=sub_start, sub_end=sub_end, sub_off=sub_off, sub_steps=sub_steps,
                sub_names=[f"{names[p]}:{a}-{b}" for p, a, b in zip(sub_path, sub_start, sub_end)])


def plain(d):
    """a result of seqrush_amd.extract() in the shape of restate()"""
    if isinstance(d["level"], list):
        return d
    out = {k: int(d[k]) for k in COUNTERS}
    for k in TABLES:
        out[k] = [int(x) for x in d[k]]
    out["sub_names"] = list(d["sub_names"])
    return out


def assert_same(got, want, what=""):
    """two results, each from extract() or restate(): every counter and every table"""
    got, want = plain(got), plain(want)
    for k in COUNTERS + TABLES + ("sub_names",):
        assert got[k] == want[k], f"{what}: {k}: {str(got[k])[:300]} != {str(want[k])[:300]}"


def report_of(d, text):
    """the bytes sr_extract_text must write for the result d of the graph `text`"""
    d, g = plain(d), st.parse(text)
    ids = sorted(g.seq)

    def hs(h):
        return f"{h >> 1}\t{'-' if h & 1 else '+'}"
    out = ["H\tVN:Z:1.0\n"] + [f"S\t{k + 1}\t{g.seq[ids[old - 1]]}\n" for k, old in enumerate(d["node_old"])]
    out += [f"L\t{hs(a)}\t{hs(b)}\t0M\n" for a, b in zip(d["edge_from"], d["edge_to"])]
    for j, name in enumerate(d["sub_names"]):
        steps = d["sub_steps"][d["sub_off"][j]:d["sub_off"][j + 1]]
        out.append(f"P\t{name}\t" + ",".join(f"{h >> 1}{'-' if h & 1 else '+'}" for h in steps) + "\t*\n")
    return "".join(out)


def names_of(text):
    return [n for n, _ in st.parse(text).paths]


def path_lengths(text):
    g = st.parse(text)
    return [sum(len(g.seq[h >> 1]) for h in s) for _, s in g.paths]


def step_starts(text, name):
    """the offsets of the steps of path `name` in its own sequence, and its length at the end"""
    g = st.parse(text)
    at = [0]
    for h in dict(g.paths)[name]:
        at.append(at[-1] + len(g.seq[h >> 1]))
    return at


def with_edges(text):
    """the same graph with an L line for every two consecutive steps of a path that has none yet (variants_inputs.bubbles
    writes no L line, and context has nothing to follow without)"""
    g = st.parse(text)
    edges = list(g.edges)
    have = set(edges)
    for _, steps in g.paths:
        for e in zip(steps, steps[1:]):
            if e not in have:
                have.add(e)
                edges.append(e)
    return sh.Gfa(g.seq, edges, g.paths).text()


def usable_names(text):
    """the paths a region string or a BED line can name without ambiguity: a base, the first of their name, a plain name"""
    names, plen = names_of(text), path_lengths(text)
    return [p for p, n in enumerate(names) if plen[p] and names.index(n) == p and n and not n.startswith(("#", "track", "browser"))
            and "\t" not in n and " " not in n and ":" not in n]


def random_regions(text, seed, n=6):
    """-> (region strings, BED text): n seeded regions over the usable paths, half as strings and half as BED lines between
    lines that are ignored, one BED line on a name the graph does not have and one that ends beyond its path"""
    rng = np.random.default_rng(seed)
    names, plen, live = names_of(text), path_lengths(text), usable_names(text)
    strings, lines = [], ["# seeded regions", "track name=seeded", ""]
    for k in range(n if live else 0):
        p = live[int(rng.integers(0, len(live)))]
        start = int(rng.integers(0, plen[p]))
        end = start + 1 if k % 3 == 0 else int(rng.integers(start + 1, min(plen[p], start + 1 + max(1, plen[p] // 8)) + 1))
        if k % 2:
            strings.append(f"{names[p]}:{start}-{end}")
        else:
            lines.append(f"{names[p]}\t{start}\t{end}" + ("\tlabel" if k % 4 else ""))
    lines.append("no_such_contig\t0\t10\tgene")
    if live:
        lines.append(f"{names[live[0]]}\t0\t{plen[live[0]] + 1}\tbeyond")
    return tuple(strings), "\n".join(lines) + "\n"


OPTION_SETS = (dict(), dict(context_steps=1, merge_distance=0), dict(context_steps=2, merge_distance=7, merge_rounds=1),
               dict(merge_distance=3, merge_rounds=64))


def rule_kw(kw):
    """the keyword arguments of extract() as those of restate()"""
    return dict(c=kw.get("context_steps", 0), D=kw.get("merge_distance", 100000), R=kw.get("merge_rounds", 3))


# ------------------------------------------------------------------ the graph of the known answers
# a = 1+ 2+ 3+ 4+ 5+ (13 bases), b = 5- 4- 3- 1- (reversed), c visits node 3 twice, e has no step, z shares nothing;
# node 8 is on no path and hangs on node 2; node 7 has a self-loop
KNOWN_GFA = ("H\tVN:Z:1.0\nS\t1\tACG\nS\t2\tT\nS\t3\tGGA\nS\t4\tCC\nS\t5\tTTTT\nS\t6\tAG\nS\t7\tCA\nS\t8\tG\n"
             "L\t1\t+\t2\t+\t0M\nL\t2\t+\t3\t+\t0M\nL\t3\t+\t4\t+\t0M\nL\t4\t+\t5\t+\t0M\nL\t1\t+\t3\t+\t0M\nL\t3\t+\t6\t+\t0M\nL\t6\t+\t3\t+\t0M\n"
             "L\t2\t+\t8\t+\t0M\nL\t7\t+\t7\t+\t0M\n"
             "P\ta\t1+,2+,3+,4+,5+\t*\nP\tb\t5-,4-,3-,1-\t*\nP\tc\t1+,3+,6+,3+,5+\t*\nP\te\t\t*\nP\tz\t7+\t*\n")
KNOWN_BED = "# loci of haplotype a\r\ntrack name=loci\r\n\r\na\t3\t4\tsnp\r\nc 6 8 second\r\nchrUn\t0\t5\r\na\t5\t5\r\nb\t0\t13\r\ne\t0\t1\r\n"


def known_cases():
    """name -> (regions, BED text or None, keyword arguments of extract())"""
    return {
        "node_2_alone": (("a:3-4",), None, dict(merge_distance=0)),
        "node_6_alone": (("c:6-8",), None, dict(merge_distance=0)),
        "node_6_with_context": (("c:6-8",), None, dict(context_steps=1, merge_distance=0)),
        "ends_of_a_one_round": (("a:0-1", "a:12-13"), None, dict(merge_distance=6, merge_rounds=1)),
        "ends_of_a_two_rounds": (("a:0-1", "a:12-13"), None, dict(merge_distance=6)),
        "ends_of_a_default": (("a:0-1", "a:12-13"), None, dict()),
        "whole_z": (("z",), None, dict()),
        "bed_and_strings": (("b:11-12", "e"), KNOWN_BED, dict(context_steps=2, merge_distance=1)),
        "context_reaches_node_8": (("a:3-4",), None, dict(context_steps=1, merge_distance=0)),
        "every_path": (("a", "b", "c", "e", "z"), None, dict()),
        "nothing": ((), "", dict()),
    }


# ------------------------------------------------------------------ graphs for the properties and the seams
def two_round_graph():
    """A = s1 y1 x y2 s2, B = s1 x s2, C = s1 y1 x y2 s2 (every node 3 bp) with regions on s1 and s2 of B and D = 5: B's gap is
    [x] (3 bp) and closes in round 1; C's gap is [y1, x, y2] (9 bp) and does not, but with x kept its gaps [y1] and [y2] close
    in round 2.  -> (text, regions); nodes: s1 = 1, y1 = 2, x = 3, y2 = 4, s2 = 5"""
    seq = {1: "ACG", 2: "TTA", 3: "GGC", 4: "CAT", 5: "TGA"}
    paths = [("B", [2, 6, 10]), ("C", [2, 4, 6, 8, 10])]
    edges = [(2, 4), (4, 6), (6, 8), (8, 10), (2, 6), (6, 10)]
    return sh.Gfa(seq, edges, paths).text(), ("B:0-1", "B:8-9")


def line_graph(n, length=1, paths=None, edges=True, first=1):
    """nodes first..first+n-1 of `length` bases (a list: per node) in a chain, the path "a" over all of them unless paths
    are given; the L lines of the chain unless edges is False"""
    lens = length if isinstance(length, list) else [length] * n
    seq = {first + k: "ACGT"[(first + k) % 4] * lens[k] for k in range(n)}
    e = [((first + k) << 1, (first + k + 1) << 1) for k in range(n - 1)] if edges else []
    return sh.Gfa(seq, e, paths if paths is not None else [("a", [(first + k) << 1 for k in range(n)])]).text()


def fwd(a, b):
    """the forward handles of the nodes a..b"""
    return [v << 1 for v in range(a, b + 1)]


def _bed(rows):
    return "".join("\t".join(map(str, r)) + "\n" for r in rows)


def seam_cases():
    """name -> (GFA text, region strings, BED text or None, keyword arguments of extract())"""
    cases = {}
    # one base at the first and the last base of a step (step 4 of ten steps of 3 bases: [12, 15)) and either side of them
    ten = line_graph(10, 3)
    for what, (a, b) in dict(first_base=(12, 13), last_base=(14, 15), before=(11, 12), behind=(15, 16), ends_at_boundary=(10, 12),
                             starts_at_boundary=(15, 17), inside=(13, 14)).items():
        cases[f"one_step_{what}"] = (ten, (f"a:{a}-{b}",), None, dict(merge_distance=0))
    # 1 .. 257 regions on one path
    rng = np.random.default_rng(5)
    long_ = line_graph(700, 2)
    for n in (1, 63, 64, 65, 257):
        starts = sorted(int(x) for x in rng.integers(0, 1390, size=n))
        cases[f"regions_{n}"] = (long_, (), _bed(("a", s, s + 1 + (k % 3)) for k, s in enumerate(starts)), dict(merge_distance=0))
    # nested and duplicate regions: steps 20 .. 24 are covered by the long early region alone
    cases["nested_regions"] = (long_, ("a:0-50", "a:10-12", "a:10-12", "a:20-22", "a:30-31", "a:60-62", "a:0-50"), None, dict(merge_distance=0))
    cases["nested_regions_sorted_late"] = (long_, ("a:30-31", "a:44-46", "a:2-50", "a:3-4", "a:46-47"), None, dict(merge_distance=0))
    # several paths, the first and the last among them; a path with no kept step between two that have some; an empty path
    many = sh.Gfa({v: "ACGT"[v % 4] * (1 + v % 3) for v in range(1, 61)}, [(v << 1, (v + 1) << 1) for v in range(1, 60)],
                  [("p0", fwd(1, 20)), ("p1", fwd(21, 40)), ("p2", [v << 1 | 1 for v in range(60, 40, -1)]), ("p3", fwd(5, 30))]).text()
    many = vi.with_empty_path(many)
    cases["first_and_last_path"] = (many, ("p0:3-9", "p3:0-2", "p3:20-30"), None, dict(merge_distance=0))
    cases["no_kept_step_between"] = (many, ("p0:0-3", "p2:5-9"), None, dict(merge_distance=0))
    cases["empty_path_named"] = (many, ("none", "p2:0-1"), "none\t0\t1\n", dict())
    # two adjacent paths, the last step of one and the first of the next kept: two subpaths; on a workgroup boundary of the
    # scan (step 256) and off it
    for n0 in (256, 200):
        two = sh.Gfa({v: "A" for v in range(1, 301)}, [], [("p0", fwd(1, n0)), ("p1", fwd(n0 + 1, 300))]).text()
        cases[f"adjacent_paths_{n0}"] = (two, (f"p0:{n0 - 1}-{n0}", "p1:0-1"), None, dict())
        cases[f"adjacent_paths_{n0}_wide"] = (two, (f"p0:{n0 - 3}-{n0}", "p1:0-2", "p0:0-1"), None, dict(merge_distance=1000))
    # not-kept runs at the start and at the end of a path: neither may merge; b walks them too
    ends = sh.Gfa({v: "CG" for v in range(1, 21)}, [], [("a", fwd(1, 20)), ("b", fwd(1, 20))]).text()
    cases["runs_at_both_ends"] = (ends, ("a:8-20",), None, dict())
    # a not-kept run whose nearest kept step on one side lies in the neighbouring path
    neigh = sh.Gfa({v: "T" for v in range(1, 21)}, [], [("p0", fwd(1, 10)), ("p1", fwd(11, 20))]).text()
    cases["neighbour_in_another_path"] = (neigh, ("p0:2-3", "p1:7-8"), None, dict())
    cases["neighbour_in_another_path_and_own"] = (neigh, ("p0:2-3", "p1:7-8", "p1:0-1"), None, dict())
    # gaps of exactly D and D + 1 bases: the nodes 2, 3, 4 between the regions hold 6 bases
    gap = line_graph(8, 2)
    cases["gap_of_D"] = (gap, ("a:0-2", "a:8-9"), None, dict(merge_distance=6))
    cases["gap_of_D_plus_1"] = (gap, ("a:0-2", "a:8-9"), None, dict(merge_distance=5))
    cases["gap_D_0"] = (gap, ("a:0-2", "a:4-5"), None, dict(merge_distance=0))
    # gaps of 1 .. 1025 steps with D large, behind a prefix that moves them off the workgroup boundaries
    for n in (1, 63, 64, 65, 256, 257, 1025):
        pre = 7 + n % 5
        cases[f"gap_of_{n}_steps"] = (line_graph(pre + n + 2 + 3), (f"a:{pre}-{pre + 1}", f"a:{pre + n + 1}-{pre + n + 2}"), None, dict())
    # context: 0, 1, 2 steps and more than the diameter; no L lines at all
    bub = vi.bubbles(3, 14, 5, 2)[0]
    mid = path_lengths(bub)[0] // 2
    for c in (0, 1, 2, 1000):
        cases[f"context_{c}"] = (with_edges(bub), (f"{names_of(bub)[0]}:{mid}-{mid + 2}",), None, dict(context_steps=c, merge_distance=0))
    cases["context_without_L_lines"] = (bub, (f"{names_of(bub)[0]}:{mid}-{mid + 2}",), None, dict(context_steps=2, merge_distance=0))
    # a self-loop on a seed and on a node beside it; an edge between reverse handles
    loops = sh.Gfa({v: "GA" for v in range(1, 7)}, [(2 << 1, 2 << 1), (3 << 1, 3 << 1 | 1), (2 << 1, 3 << 1), (4 << 1 | 1, 3 << 1 | 1), (5 << 1 | 1, 4 << 1),
                                                     (6 << 1, 6 << 1)], [("a", fwd(1, 2)), ("b", [6 << 1 | 1, 5 << 1, 4 << 1 | 1])]).text()
    for c in (1, 2, 3):
        cases[f"loops_and_reverse_edges_c{c}"] = (loops, ("a:2-4",), None, dict(context_steps=c, merge_distance=0))
    # the two rounds
    text, regs = two_round_graph()
    for R in (1, 2, 64):
        cases[f"two_rounds_R{R}"] = (text, regs, None, dict(merge_distance=5, merge_rounds=R))
    # a node visited three times by the region's path; the region is on the middle visit
    thrice = sh.Gfa({1: "AC", 2: "GGT", 3: "T", 4: "CA", 5: "G"}, [], [("a", [2, 4, 6, 5, 8, 4, 10]), ("b", [4, 10])]).text()
    cases["visited_three_times"] = (thrice, ("a:6-7",), None, dict(merge_distance=0))
    cases["visited_three_times_merged"] = (thrice, ("a:6-7",), None, dict(merge_distance=1))
    # V, S and E at 1, 255, 256, 257, 65 536 and 65 537 (a chain of n one-base nodes has n steps and n - 1 edges): the last two
    # reach the second level of the scan
    for n in (1, 2, 255, 256, 257, 258, 65536, 65537, 65538):
        rows = [("a", k, min(n, k + 100)) for k in range(0, n, 200)] + [("a", n - 1, n)]
        cases[f"chain_{n}"] = (line_graph(n), (), _bed(rows), dict(context_steps=1, merge_distance=0))
    cases["chain_65537_merged"] = (line_graph(65537), (), _bed([("a", 0, 1), ("a", 300, 301), ("a", 65536, 65537)]), dict(merge_distance=70000))
    cases["chain_65537_whole"] = (line_graph(65537), ("a",), None, dict())
    return cases
