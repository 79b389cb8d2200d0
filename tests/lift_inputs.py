"""Inputs and restatements for the tests of the interval lift.

restate(): the rule in Python dicts and lists over stats_helpers.parse, base by base: every base of the query is sent to
the base of the target's first visit of its node, and the fields are the smallest and the largest position, the count and
the count on the other strand.  It reads the BED lines itself and shares nothing with the library.  report_of(): the bytes
sr_lift_bed must write for a result.  random_bed(): seeded queries on a graph, with lines that are skipped.  seam_cases():
graphs and queries built for the seams of the kernels (the 8 steps between the two pair kernels, the wave of 64 and the
workgroup of 256, targets that make the lanes of a wave straddle queries, the identities of the reduction)."""
import numpy as np

import sort_helpers as sh
import stats_helpers as st
import variants_inputs as vi

BLOCK = 256             # LF_BLOCK: steps, queries and pairs per workgroup
SHORT_STEPS = 8         # sr_lift_params_default
ALL_SHORT, ALL_LONG = 2 ** 64 - 1, 0
FIELDS = ("tstart", "tend", "covered", "rev_bp")


class Invalid(Exception):
    """what the library answers with SR_ERR_INVALID"""


def read_bed(bed, names, plen):
    """-> (queries [(path, start, end, label)], unknown, out_of_range); Invalid names the line"""
    queries, unknown, out_of_range = [], 0, 0
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
            queries.append((names.index(f[0]), start, end, f[3] if len(f) > 3 and f[3] else f"{f[0]}:{f[1]}-{f[2]}"))
    return queries, unknown, out_of_range


def bases_of(g, steps):
    """every base of a path: (node, offset on the node's forward strand, orientation of the step)"""
    out = []
    for h in steps:
        n = len(g.seq[h >> 1])
        out += [(h >> 1, n - 1 - k if h & 1 else k, h & 1) for k in range(n)]
    return out


def first_visits(g, steps):
    """node -> (the path position of the first base of the first step on the node, the orientation of that step)"""
    at, first = 0, {}
    for h in steps:
        first.setdefault(h >> 1, (at, h & 1))
        at += len(g.seq[h >> 1])
    return first


def restate(text, bed, to=None):
    """-> dict with the fields of seqrush_amd.lift() that the rule fixes (the four tables as lists of rows)"""
    g = st.parse(text)
    names = [n for n, _ in g.paths]
    if to is not None and to not in names:
        raise Invalid(f"no path is named '{to}'")
    bases = {}
    plen = [sum(len(g.seq[h >> 1]) for h in s) for _, s in g.paths]
    queries, unknown, out_of_range = read_bed(bed, names, plen)
    targets = list(range(len(names))) if to is None else [names.index(to)]
    first = {b: first_visits(g, g.paths[b][1]) for b in targets}
    out = dict(queries=len(queries), targets=len(targets), paths=len(names), unknown=unknown, out_of_range=out_of_range, mapped=0,
               q_path=[q[0] for q in queries], q_start=[q[1] for q in queries], q_end=[q[2] for q in queries],
               labels=[q[3] for q in queries], target_path=targets, to_named=int(to is not None), **{k: [] for k in FIELDS})
    for a, start, end, _ in queries:
        if a not in bases:
            bases[a] = bases_of(g, g.paths[a][1])
        rows = {k: [] for k in FIELDS}
        for b in targets:
            pos, rev = [], 0
            for v, off, r in bases[a][start:end]:
                if v in first[b]:
                    at, r2 = first[b][v]
                    pos.append(at + (len(g.seq[v]) - 1 - off if r2 else off))
                    rev += r ^ r2
            for k, x in zip(FIELDS, (min(pos), max(pos) + 1, len(pos), rev) if pos else (0, 0, 0, 0)):
                rows[k].append(x)
            out["mapped"] += bool(pos)
        for k in FIELDS:
            out[k].append(rows[k])
    return out


PLAIN = ("queries", "targets", "paths", "unknown", "out_of_range", "mapped", "to_named")


def plain(d):
    """a result of seqrush_amd.lift() in the shape of restate()"""
    if isinstance(d["covered"], list):
        return d
    out = {k: int(d[k]) for k in PLAIN}
    for k in ("q_path", "q_start", "q_end", "target_path"):
        out[k] = [int(x) for x in d[k]]
    out["labels"] = list(d["labels"])
    for k in FIELDS:
        out[k] = [[int(x) for x in r] for r in d[k]]
    return out


def assert_same(got, want, what=""):
    """two results, each from lift() or restate(): every field the rule fixes"""
    got, want = plain(got), plain(want)
    for k in PLAIN + ("q_path", "q_start", "q_end", "labels", "target_path"):
        assert got[k] == want[k], f"{what}: {k}: {str(got[k])[:300]} != {str(want[k])[:300]}"
    for k in FIELDS:
        for i, (x, y) in enumerate(zip(got[k], want[k])):
            assert x == y, f"{what}: {k} of query {i} = {got['labels'][i]}: {x} != {y}"


def report_of(d, names, min_covered=1):
    """the bytes sr_lift_bed must write for the result d"""
    d, out = plain(d), []
    for i, a in enumerate(d["q_path"]):
        for k, b in enumerate(d["target_path"]):
            cov, rev = d["covered"][i][k], d["rev_bp"][i][k]
            if cov == 0 or cov < min_covered or (a == b and not d["to_named"]):
                continue
            out.append("\t".join(map(str, (names[b], d["tstart"][i][k], d["tend"][i][k], d["labels"][i], cov, "-" if 2 * rev > cov else "+",
                                           names[a], d["q_start"][i], d["q_end"][i], rev))) + "\n")
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


# ------------------------------------------------------------------ seeded queries
def random_bed(text, seed, n=12):
    """n seeded queries over the paths of the graph that have a base (half of them one base long), between lines that are
    ignored, one line on a name the graph does not have and one that ends beyond its path"""
    rng = np.random.default_rng(seed)
    names, plen = names_of(text), path_lengths(text)
    lines = ["# seeded queries", "track name=seeded", ""]
    live = [p for p, n_ in enumerate(plen) if n_ and names.index(names[p]) == p and not names[p].startswith(("#", "track", "browser"))
            and "\t" not in names[p] and " " not in names[p] and names[p]]
    for k in range(n if live else 0):
        p = live[int(rng.integers(0, len(live)))]
        start = int(rng.integers(0, plen[p]))
        end = start + 1 if k % 2 else int(rng.integers(start + 1, plen[p] + 1))
        lines.append(f"{names[p]}\t{start}\t{end}" + (f"\tq{k}" if k % 3 else "") + ("\t0\t+" if k % 4 == 1 else ""))
    lines.append("no_such_contig\t0\t10\tgene")
    if live:
        lines.append(f"{names[live[0]]}\t0\t{plen[live[0]] + 1}\tbeyond")
    return "\n".join(lines) + "\n"


# ------------------------------------------------------------------ seams of the kernels
def _bed(rows):
    return "".join("\t".join(map(str, r)) + "\n" for r in rows)


def chain_case():
    """the chain of variants_inputs (a first path that ends on a workgroup boundary of the scan, the path "ref" of 1100
    steps, walks of 1 to 1025 steps of which every third is reversed) with: a target that visits node 5 three times, the
    last time first in its own order only; a target that shares no node; a target without a step; a query path of one
    step; and, last in the file, a query path of 200 private nodes whose 201st and last step is its only shared node"""
    far = 1400
    thrice = [3 << 1, 5 << 1 | 1, 4 << 1, 5 << 1, 6 << 1, 5 << 1 | 1, 7 << 1]
    alone = [(far + k) << 1 | (k & 1) for k in range(70)]
    tail = [(far + 100 + k) << 1 for k in range(200)] + [900 << 1 | 1]
    lengths = [256, 1, 63, 64, 65, 255, 256, 257, 1025]
    text = vi.chain(11, 1100, lengths, ref_at=1, extra=[("thrice", thrice), ("alone", alone), ("one", [700 << 1 | 1]), ("tail", tail)])
    text = vi.with_empty_path(text)
    at = step_starts(text, "ref")
    rows = []
    for n in (1, 8, 9, 63, 64, 65, 128, 129, 1025):            # whole steps: both ends on step boundaries
        k = 20 + n % 7
        rows.append(("ref", at[k], at[k + n], f"steps{n}"))
        rows.append(("ref", at[k] + 1, at[k + n] + 1, f"steps{n}_right"))      # one base either side of the boundaries
        rows.append(("ref", at[k] - 1, at[k + n] - 1, f"steps{n}_left"))
    wide = next(k for k in range(1, 1100) if at[k + 1] - at[k] >= 3)
    rows.append(("ref", at[wide] + 1, at[wide] + 2, "inside_one_step"))
    rows += [("ref", 0, 1, "first_base"), ("ref", at[-1] - 1, at[-1], "last_base"), ("ref", 0, at[-1], "whole_path")]
    rows += [("ref", at[2], at[8], "over_thrice")]
    one, tl = step_starts(text, "one"), step_starts(text, "tail")
    rows += [("one", 0, one[-1], "path_of_one_step"), ("tail", 0, tl[-1], "shared_at_the_last_step"), ("tail", 0, tl[-2], "shares_nothing"),
             ("tail", tl[-2], tl[-1]), ("alone", 0, 5, "alone")]
    names = names_of(text)
    w = step_starts(text, names[0])
    rows += [(names[0], 0, w[-1], "path_to_the_workgroup_boundary"), (names[0], w[-2], w[-1], "its_last_step")]
    return text, _bed(rows)


def many_targets(P, seed=3):
    """P paths over a chain of 48 nodes, each a seeded walk (forward or reversed) that leaves nodes out; five queries of 1
    to 40 steps on the first, a middle and the last path, so that the 64 lanes of a wave hold pairs of several queries"""
    rng = np.random.default_rng(seed + P)
    seq = {v: vi._word(rng, 1 + v % 3) for v in range(1, 49)}
    paths = []
    for p in range(P):
        keep = [v for v in range(1, 49) if rng.random() < 0.8] or [1]
        paths.append((f"t{p}", [(v << 1) | 1 for v in reversed(keep)] if p % 4 == 3 else [v << 1 for v in keep]))
    text = sh.Gfa(seq, [], paths).text()
    rows = []
    for k, p in enumerate((0, P // 2, P - 1, 0, P - 1)):
        at = step_starts(text, f"t{p}")
        n = len(at) - 1
        a, b = ((0, n), (0, 1), (n // 2, n // 2 + min(9, n - n // 2)), (n - 1, n), (1 % n, n))[k]
        rows.append((f"t{p}", at[a], at[b], f"q{k}"))
    return text, _bed(rows)


def one_base_queries(n=5000, seed=17):
    """n one-base queries over six paths of a small bubble graph: the pairs cross many workgroups whichever kernel runs"""
    text = vi.bubbles(seed, 30, 6, 2)[0]
    rng = np.random.default_rng(seed)
    names, plen = names_of(text), path_lengths(text)
    rows = []
    for _ in range(n):
        p = int(rng.integers(0, len(names)))
        x = int(rng.integers(0, plen[p]))
        rows.append((names[p], x, x + 1))
    return text, _bed(rows)


def seam_cases():
    """name -> (GFA text, BED text, keyword arguments of lift())"""
    chain = chain_case()
    cases = {"chain_1_to_1025_steps": chain + ({},)}
    cases["chain_to_one_reversed_target"] = chain + (dict(to="w2_63"),)
    cases["chain_to_the_empty_target"] = chain + (dict(to="none"),)
    for P in (63, 64, 65, 130):
        cases[f"targets_{P}"] = many_targets(P) + ({},)
    cases["targets_1"] = many_targets(9) + (dict(to="t4"),)
    cases["one_base_5000"] = one_base_queries() + ({},)
    return cases
