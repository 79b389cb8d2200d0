"""Inputs and restatements for the tests of the variant sites.

restate(): the rule in Python dicts, sets and strings over stats_helpers.parse; it shares nothing with the library.
round_trip(): a path's alleles of a result applied to the reference give the path's own sequence back.  bubbles(): graphs
built bubble by bubble together with the sites and genotypes the construction knows.  report_of(): the bytes
sr_variants_vcf must write for a result.  seam_cases(): graphs built for the seams of the kernels (the wave of 64 and the
workgroup of 256 steps, the carry of the scan across workgroups, many traversals at one site)."""
from collections import Counter

import numpy as np

import sort_helpers as sh
import stats_helpers as st

BLOCK = 256             # VA_BLOCK: steps per workgroup


def oriented(g, h):
    return sh.rc(g.seq[h >> 1]) if h & 1 else g.seq[h >> 1]


def anchors_of(g, R):
    """-> (refseq, {node: (ref_pos, ref_end, ref_or)} for the nodes the reference visits exactly once)"""
    steps = g.paths[R][1]
    seen = Counter(h >> 1 for h in steps)
    at, anchor, parts = 0, {}, []
    for h in steps:
        s = oriented(g, h)
        if seen[h >> 1] == 1:
            anchor[h >> 1] = (at, at + len(s), h & 1)
        at += len(s)
        parts.append(s)
    return "".join(parts), anchor


def restate(text, ref=None, max_allele_len=10000):
    """-> dict with the fields of seqrush_amd.variants() that the rule fixes (alleles as bytes, gt as a list of rows)"""
    g = st.parse(text)
    P = len(g.paths)
    out = dict(ref_path=0, ref_len=0, ref_seq=b"", paths=P, anchors=0, traversals=0, sites=0, breaks=[0] * P, skipped=[0] * P,
               site_start=[], site_end=[], alleles=[], gt=[])
    if P == 0:
        return out
    R = 0 if ref is None else [n for n, _ in g.paths].index(ref)
    refseq, anchor = anchors_of(g, R)
    out.update(ref_path=R, ref_len=len(refseq), ref_seq=refseq.encode(), anchors=len(anchor))
    by_site, runs = {}, []                                   # (a, b) -> [(path, step, allele)]; (path, lo, hi)
    for p, (_, steps) in enumerate(g.paths):
        at = [k for k, h in enumerate(steps) if h >> 1 in anchor]
        strand = {k: (steps[k] & 1) ^ anchor[steps[k] >> 1][2] for k in at}
        run = None
        for n, j in enumerate(at):
            pj, ej, _ = anchor[steps[j] >> 1]
            joins = False
            if n:
                i = at[n - 1]
                pi, ei, _ = anchor[steps[i] >> 1]
                between = steps[i + 1:j]
                if strand[i] != strand[j] or (pj < ei if strand[j] == 0 else ej > pi):
                    out["breaks"][p] += 1
                else:
                    a, b = (ei, pj) if strand[j] == 0 else (ej, pi)
                    allele = "".join(oriented(g, h) for h in between) if strand[j] == 0 else \
                        "".join(oriented(g, h ^ 1) for h in reversed(between))
                    if a == b and allele == "":
                        joins = j == i + 1
                    elif max_allele_len and (b - a > max_allele_len or len(allele) > max_allele_len):
                        out["skipped"][p] += 1
                    else:
                        by_site.setdefault((a, b), []).append((p, i, allele))
                        out["traversals"] += 1
            if joins:
                run = (p, min(run[1], pj), max(run[2], ej))
                runs[-1] = run
            else:
                run = (p, pj, ej)
                runs.append(run)
    for (a, b) in sorted(by_site):
        trav = by_site[(a, b)]
        ref_allele = refseq[a:b]
        alts = sorted({t[2] for t in trav} - {ref_allele}, key=lambda s: (len(s), s.encode()))
        if not alts:
            continue
        row = [-1] * P
        for p, lo, hi in runs:
            if lo < a and b < hi:
                row[p] = 0
        first = {}
        for p, step, allele in trav:
            if p not in first or step < first[p][0]:
                first[p] = (step, allele)
        for p, (_, allele) in first.items():
            row[p] = 0 if allele == ref_allele else alts.index(allele) + 1
        out["site_start"].append(a)
        out["site_end"].append(b)
        out["alleles"].append([s.encode() for s in alts])
        out["gt"].append(row)
    out["sites"] = len(out["gt"])
    return out


FIELDS = ("ref_path", "ref_len", "ref_seq", "paths", "anchors", "traversals", "sites")


def plain(d):
    """a result of seqrush_amd.variants() in the shape of restate()"""
    out = {k: d[k] for k in FIELDS}
    for k in ("breaks", "skipped", "site_start", "site_end", "gt"):
        out[k] = [[int(x) for x in r] for r in d[k]] if k == "gt" else [int(x) for x in d[k]]
    out["alleles"] = [list(a) for a in d["alleles"]]
    return out


def assert_same(got, want, what=""):
    """two results, each from variants() or restate(): every field the rule fixes"""
    got = plain(got) if not isinstance(got["gt"], list) else got
    want = plain(want) if not isinstance(want["gt"], list) else want
    for k in FIELDS + ("breaks", "skipped", "site_start", "site_end", "alleles"):
        assert got[k] == want[k], f"{what}: {k}: {str(got[k])[:300]} != {str(want[k])[:300]}"
    for s, (x, y) in enumerate(zip(got["gt"], want["gt"])):
        assert x == y, f"{what}: gt of site {s} = ({got['site_start'][s]}, {got['site_end'][s]}): {x} != {y}"
    assert len(got["gt"]) == len(want["gt"]), what


def round_trip(d, text, p):
    """-> (the reference between the first and the last anchor step of path p with p's alleles put in, p's own sequence
    there, read on the reference's strand); None if p has fewer than two anchor steps"""
    g = st.parse(text)
    refseq, anchor = anchors_of(g, d["ref_path"])
    assert refseq.encode() == d["ref_seq"]
    steps = g.paths[p][1]
    at = [k for k, h in enumerate(steps) if h >> 1 in anchor]
    if len(at) < 2:
        return None
    own = "".join(oriented(g, h) for h in steps[at[0]:at[-1] + 1])
    lo = min(anchor[steps[k] >> 1][0] for k in (at[0], at[-1]))
    hi = max(anchor[steps[k] >> 1][1] for k in (at[0], at[-1]))
    if (steps[at[0]] & 1) ^ anchor[steps[at[0]] >> 1][2]:
        own = sh.rc(own)
    built, cur = [], lo
    for s in range(d["sites"]):
        a, b, k = int(d["site_start"][s]), int(d["site_end"][s]), int(d["gt"][s][p])
        if k <= 0 or a < lo or b > hi:
            continue
        assert a >= cur, "the alleles of one colinear path do not overlap"
        built.append(refseq[cur:a] + d["alleles"][s][k - 1].decode())
        cur = b
    built.append(refseq[cur:hi])
    return "".join(built), own


def report_of(d, names):
    """the bytes sr_variants_vcf must write for the result d"""
    P, R = d["paths"], d["ref_path"]
    ref = d["ref_seq"].decode()
    out = ["##fileformat=VCFv4.2\n", "##source=seqrush_amd variants v1\n"]
    if P:
        out.append(f"##contig=<ID={names[R]},length={d['ref_len']}>\n")
    out.append(f"##seqrush_amd=<anchors={d['anchors']},traversals={d['traversals']},sites={d['sites']},"
               f"breaks={sum(int(x) for x in d['breaks'])},skipped={sum(int(x) for x in d['skipped'])}>\n")
    out.append('##INFO=<ID=AC,Number=A,Type=Integer,Description="Samples that carry each ALT allele">\n')
    out.append('##INFO=<ID=AN,Number=1,Type=Integer,Description="Samples with a genotype">\n')
    out.append('##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">\n')
    samples = [p for p in range(P) if p != R]
    out.append("\t".join(["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"] + [names[p] for p in samples]) + "\n")
    for s in range(d["sites"]):
        a, b = int(d["site_start"][s]), int(d["site_end"][s])
        alts = [x.decode() for x in d["alleles"][s]]
        row = [int(x) for x in d["gt"][s]]
        if b > a and all(alts):
            pos, ref_allele = a + 1, ref[a:b]
        else:
            pos, ref_allele, alts = a, ref[a - 1:b], [ref[a - 1] + x for x in alts]
        ac = [sum(1 for p in samples if row[p] == k + 1) for k in range(len(alts))]
        an = sum(1 for p in samples if row[p] >= 0)
        out.append("\t".join([names[R], str(pos), ".", ref_allele, ",".join(alts), ".", ".",
                              "AC=" + ",".join(map(str, ac)) + f";AN={an}", "GT"] +
                             ["." if row[p] < 0 else str(row[p]) for p in samples]) + "\n")
    return "".join(out)


def names_of(text):
    return [n for n, _ in st.parse(text).paths]


# ------------------------------------------------------------------ graphs built bubble by bubble
def _word(rng, n, avoid=()):
    while True:
        w = "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=n))
        if w not in avoid:
            return w


def bubbles(seed, n_bubbles=40, n_paths=7, reverse_every=3, kinds=("snp", "ins", "del", "mnp", "tri")):
    """-> (GFA text, truth): a backbone node of >= 1 bp between bubbles; the reference (path 0) takes allele 0 of each
    bubble, every other path a random one; every reverse_every-th path runs on the reverse strand.  truth = dict(sites:
    [(a, b, [ALT alleles carried, by (length, bytes)])], gt: [row per site])"""
    rng = np.random.default_rng(seed)
    seq, nid = {}, 0

    def node(s):
        nonlocal nid
        nid += 1
        seq[nid] = s
        return nid
    walk = [[] for _ in range(n_paths)]              # node lists, forward
    first = node(_word(rng, int(rng.integers(1, 5))))
    for w in walk:
        w.append(first)
    at, sites, gt = len(seq[first]), [], []
    for _ in range(n_bubbles):
        kind = kinds[int(rng.integers(0, len(kinds)))]
        if kind == "snp":
            r = _word(rng, 1)
            alleles = [r, _word(rng, 1, (r,))]
        elif kind == "ins":
            alleles = ["", _word(rng, int(rng.integers(1, 6)))]
        elif kind == "del":
            alleles = [_word(rng, int(rng.integers(1, 6))), ""]
        elif kind == "mnp":
            n = int(rng.integers(2, 5))
            r = _word(rng, n)
            alleles = [r, _word(rng, n, (r,))]
        else:
            n = int(rng.integers(1, 4))
            r = _word(rng, n)
            x = _word(rng, n, (r,))
            alleles = [r, x, _word(rng, n, (r, x))]
        nodes = [node(a) if a else None for a in alleles]
        pick = [0] + [int(rng.integers(0, len(alleles))) for _ in range(n_paths - 1)]
        for p, k in enumerate(pick):
            if nodes[k] is not None:
                walk[p].append(nodes[k])
        carried = sorted({alleles[k] for k in pick} - {alleles[0]}, key=lambda s: (len(s), s.encode()))
        if carried:
            sites.append((at, at + len(alleles[0]), [s.encode() for s in carried]))
            gt.append([0 if k == 0 else carried.index(alleles[k]) + 1 for k in pick])
        at += len(alleles[0])
        spine = node(_word(rng, int(rng.integers(1, 5))))
        for w in walk:
            w.append(spine)
        at += len(seq[spine])
    paths = []
    for p, w in enumerate(walk):
        rev = p > 0 and reverse_every and p % reverse_every == 0
        paths.append((f"p{p}", [(v << 1) | 1 for v in reversed(w)] if rev else [v << 1 for v in w]))
    return sh.Gfa(seq, [], paths).text(), dict(sites=sites, gt=gt)


def bubble_inputs():
    return [(f"bubbles:{seed}", bubbles(seed, 12 + seed, 3 + seed % 5, 2 + seed % 3)[0]) for seed in range(1, 7)]


# ------------------------------------------------------------------ seams of the kernels
def chain(seed, n_ref, lengths, ref_at=1, extra=()):
    """a reference chain of n_ref nodes named "ref" at position ref_at among paths of the given numbers of steps: walks
    along the chain from random starts that take an alternative node (every 4th position has one), skip a node (a
    deletion) or follow the reference; every third walk is reversed.  extra: further (name, steps) paths; nodes they name
    beyond the chain are created"""
    rng = np.random.default_rng(seed)
    seq = {v: _word(rng, int(rng.integers(1, 4))) for v in range(1, n_ref + 1)}
    alt = {}
    for v in range(3, n_ref, 4):
        alt[v] = n_ref + 1 + len(alt)
        seq[alt[v]] = _word(rng, len(seq[v]), (seq[v],))
    paths = []
    for k, n in enumerate(lengths):
        v = int(rng.integers(1, max(2, n_ref - n - n // 4)))
        w = []
        while len(w) < n and v <= n_ref:
            u = float(rng.random())
            if v in alt and u < 0.4:
                w.append(alt[v])
            elif v % 7 == 3 and u > 0.8 and w:
                pass
            else:
                w.append(v)
            v += 1
        assert len(w) == n
        paths.append((f"w{k}_{n}", [(x << 1) | 1 for x in reversed(w)] if k % 3 == 2 else [x << 1 for x in w]))
    paths.insert(ref_at, ("ref", [v << 1 for v in range(1, n_ref + 1)]))
    for name, steps in extra:
        for h in steps:
            seq.setdefault(h >> 1, _word(rng, 1 + (h >> 1) % 3))
        paths.append((name, list(steps)))
    return sh.Gfa(seq, [], paths).text()


def with_empty_path(text, name="none"):
    """the same graph with a path of zero steps in front of its last path"""
    lines = text.rstrip("\n").split("\n")
    lines.insert(len(lines) - 1, f"P\t{name}\t\t*")
    return "\n".join(lines) + "\n"


def one_site(n_paths, seed=5):
    """n_paths - 1 paths through one of three nodes that the reference passes by: every path has a traversal of the site"""
    rng = np.random.default_rng(seed)
    seq = {1: "ACG", 2: "T", 3: "G", 4: "C", 5: "TTA"}
    paths = [("ref", [2, 10])]
    for p in range(n_paths - 1):
        mid = int(rng.integers(2, 5))
        paths.append((f"s{p}", [11, (mid << 1) | 1, 3] if p % 5 == 4 else [2, mid << 1, 10]))
    return sh.Gfa(seq, [], paths).text()


def seam_cases():
    """name -> (GFA text, keyword arguments of variants())"""
    lengths = [256, 1, 63, 64, 65, 255, 256, 257, 1025]      # the first path ends on a workgroup boundary
    far = 1400                                               # nodes beyond the chain and its alternatives
    long_gap = [5 << 1] + [(far + k) << 1 for k in range(2 * BLOCK + 90)] + [9 << 1]         # > 2 workgroups without an anchor
    no_anchor = [(far + 700 + k) << 1 | (k & 1) for k in range(70)]
    base = chain(11, 1100, lengths, ref_at=1, extra=[("gap", long_gap), ("off", no_anchor), ("tail", [1098 << 1, 1099 << 1, 1100 << 1])])
    cases = {"steps_1_to_1025": (with_empty_path(base), dict(ref="ref"))}
    cases["three_scan_levels"] = (chain(13, 1100, [1000] * 66), dict(ref="ref"))       # > 256 * 256 steps: the block sums have block sums
    cases["ref_of_one_step"] = (sh.Gfa({1: "ACG", 2: "T", 3: "GG"}, [], [("r", [2 << 1]), ("a", [1 << 1, 2 << 1, 3 << 1]),
                                                                       ("b", [2 << 1 | 1, 3 << 1, 2 << 1]), ("c", [3 << 1])]).text(), {})
    cases["one_site_4200_paths"] = (one_site(4200), {})
    text = bubbles(77, 30, 9, 2, kinds=("tri", "mnp"))[0]
    cases["tri_allelic_hashes"] = (text, {})
    cases["tri_allelic_every_hash_collides"] = (text, dict(hash_mask=0))
    cases["one_site_300_paths_every_hash_collides"] = (one_site(300, 9), dict(hash_mask=0))
    return cases
