"""Inputs of the --extend tests: a restatement of the rule in Python that owes nothing to the
library (dict-and-string spelling, a whole-array numpy union-find), hand-built GFAs that sit on the seams of the kernels of
sr_extend.hip (256-lane workgroups, 64-lane waves, a block-sums scan whose second level starts above 256 steps and third
above 65 536), and the two families the split tests build graphs from."""
import functools
import random

import numpy as np

from seqrush_amd import synth

BLOCK = 256
COMP = {ord(a): ord(b) for a, b in zip("ACGTacgt", "TGCATGCA")}      # the project's complement: every other byte maps to itself


def revcomp(s: bytes) -> bytes:
    return bytes(COMP.get(c, c) for c in reversed(s))


# ------------------------------------------------------------------ GFA text
def gfa(nodes, paths, links=()):
    """nodes: {id: bytes}; paths: [(name, [(id, reverse)])]; links: [(from, rev, to, rev)] (ignored by --extend)"""
    out = ["H\tVN:Z:1.0"]
    out += [f"S\t{i}\t{s.decode('latin-1')}" for i, s in nodes.items()]
    out += [f"L\t{a}\t{'-' if ra else '+'}\t{b}\t{'-' if rb else '+'}\t0M" for a, ra, b, rb in links]
    out += [f"P\t{name}\t{','.join(f'{i}{chr(45) if r else chr(43)}' for i, r in steps)}\t*" for name, steps in paths]
    return "\n".join(out) + "\n"


def parse(text):
    """-> ({id: bytes}, [(name, [(id, reverse)])]) in file order"""
    nodes, paths = {}, []
    for line in text.split("\n"):
        f = line.split("\t")
        if f[0] == "S":
            nodes[int(f[1])] = f[2].encode("latin-1")
        elif f[0] == "P":
            paths.append((f[1], [(int(x[:-1]), x[-1] == "-") for x in f[2].split(",") if x]))
    return nodes, paths


# ------------------------------------------------------------------ the restatement
def plain_labels(N, unions):
    """canonical labels (smallest element of the set) of 2N + 2 elements: the strands of every base united, then `unions`;
    hooking of the larger root under the smaller and pointer jumping over whole arrays"""
    n = 2 * N + 2
    par = np.arange(n, dtype=np.int64)
    par[1:2 * N:2] -= 1
    a = np.asarray(unions, dtype=np.int64).reshape(-1, 2)
    a, b = a[:, 0], a[:, 1]
    while True:
        while True:
            nxt = par[par]
            if np.array_equal(nxt, par):
                break
            par = nxt
        ra, rb = par[a], par[b]
        open_ = ra != rb
        if not open_.any():
            return par.astype(np.uint64)
        a, b, ra, rb = a[open_], b[open_], ra[open_], rb[open_]
        par[np.maximum(ra, rb)] = np.minimum(ra, rb)


def restate(text, new_records=()):
    """the rule of the issue, step by step: old sequences by spelling, the flat step index, spos, anchor, and for every
    spelled base of a step that is not its node's anchor the union with the base the anchor spells at the same node offset
    -> dict(records, n_old, unions [(x, y)], labels)"""
    nodes, paths = parse(text)
    records = [(name, b"".join(revcomp(nodes[i]) if r else nodes[i] for i, r in steps)) for name, steps in paths]
    flat = [st for _, steps in paths for st in steps]
    spos, at = [], 0
    for i, _ in flat:
        spos.append(at)
        at += len(nodes[i])
    anchor = {}
    for s, (i, _) in enumerate(flat):
        anchor.setdefault(i, s)
    unions = []
    for s, (i, o) in enumerate(flat):
        a = anchor[i]
        if a == s:
            continue
        n, oa = len(nodes[i]), flat[a][1]
        for j in range(n):
            b = n - 1 - j if o else j
            ja = n - 1 - b if oa else b
            unions.append(((spos[s] + j) << 1, (spos[a] + ja) << 1))
    records += [(n, bytes(s)) for n, s in new_records]
    total = sum(len(s) for _, s in records)
    return dict(records=records, n_old=len(paths), unions=unions, labels=plain_labels(total, unions), old_bases=at, steps=len(flat))


# ------------------------------------------------------------------ seam graphs
def _dna(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n)).encode()


NEW = [("new1", b"ACGTTGCAAGGCTTAACCGGATATCGCGTTAA")]
ONE_BP = {1: b"A", 2: b"C", 3: b"G", 4: b"T"}


def _one_bp_paths(counts, rng):
    """paths over the four 1 bp nodes with the given step counts, either orientation"""
    return [(f"p{k}", [(rng.randrange(1, 5), rng.random() < 0.3) for _ in range(c)]) for k, c in enumerate(counts)]


@functools.lru_cache(maxsize=None)
def seam_cases():
    """name -> (GFA text, new records)"""
    rng = random.Random(1607)
    c = {}
    c["path_of_one_step"] = (gfa({1: b"ACGTAC", 2: b"GG"}, [("a", [(1, False)]), ("b", [(2, False), (1, True)]), ("c", [(1, False)])]), NEW)
    lens = (1, 63, 64, 65, 255, 256, 257, 1025)
    nodes = {k + 1: _dna(rng, n) for k, n in enumerate(lens)}
    c["node_lengths"] = (gfa(nodes, [("fwd", [(k + 1, False) for k in range(len(lens))]),
                                     ("rev", [(k + 1, True) for k in reversed(range(len(lens)))]),
                                     ("mix", [(k + 1, k % 2 == 1) for k in range(len(lens))])]), NEW)
    for total in (1023, 1024, 1025):
        c[f"steps_{total}"] = (gfa(ONE_BP, _one_bp_paths((300, 1, total - 301), rng)), NEW)
    for total in (65535, 65536, 65537):
        c[f"flat_{total}"] = (gfa(ONE_BP, _one_bp_paths((21000, 22000, total - 43000), rng)), NEW)
    c["first_visit_reversed"] = (gfa({1: b"ACCGT", 2: b"TTGACA"}, [("a", [(1, False), (2, True)]), ("b", [(2, False), (1, False)]),
                                                                   ("c", [(2, True)])]), NEW)
    c["hairpin"] = (gfa({1: b"ACGGT", 2: b"CATTG", 3: b"GA"}, [("twice", [(1, False), (3, False), (1, False)]),
                                                                ("hairpin", [(2, False), (3, False), (2, True)]),
                                                                ("other", [(1, True), (2, False)])]), NEW)
    c["unvisited_node"] = (gfa({1: b"ACGT", 7: b"GGGGGGGG", 9: b"TTA"}, [("a", [(1, False), (9, False)]), ("b", [(9, True), (1, False)])],
                               links=[(1, False, 7, False)]), NEW)
    c["iupac_bytes"] = (gfa({1: b"ACNNNNGT", 2: b"acgtRYKM", 3: b"SWBDHVN", 4: b"gattaca"},
                            [("a", [(1, False), (2, False), (3, False), (4, False)]), ("b", [(4, True), (3, True), (2, True), (1, True)]),
                             ("c", [(2, True), (2, False)])]), [("new1", b"ACNNRYacgtGATTACA")])
    star = _dna(rng, 70)
    c["star_130_paths"] = (gfa({1: star}, [(f"s{k}", [(1, k % 3 == 1)]) for k in range(130)]), NEW)
    return c


# ------------------------------------------------------------------ families of the split tests
def snp12(seed=11):
    return synth.snp_family(12, 400, 0.02, seed, rc_every=4)


def indel8(seed=12):
    return synth.indel_family(8, 300, 0.02, 0.01, seed)


FAMILIES = {"snp12": snp12, "indel8": indel8}


def splits(n):
    return (1, n // 2, n - 1)


def py_filter(pairs, n_old):
    return [(q, t) for q, t in pairs if not (q < n_old and t < n_old)]


# ------------------------------------------------------------------ refusals
def refusal_cases():
    """name -> (GFA text, new records, what the message must name)"""
    ok = {1: b"ACGT", 2: b"GG"}
    return {
        "path_name_twice": (gfa(ok, [("a", [(1, False)]), ("a", [(2, False)])]), NEW, ["two paths", "'a'"]),
        "path_and_record_share_a_name": (gfa(ok, [("a", [(1, False)]), ("new1", [(2, False)])]), NEW, ["'new1'", "twice"]),
        "path_without_steps": (gfa(ok, [("a", [(1, False)]), ("empty", [])]), NEW, ["'empty'", "no steps"]),
        "step_on_a_missing_node": (gfa(ok, [("a", [(1, False), (5, False)])]), NEW, ["missing", "'a'", "5"]),
        "node_without_a_sequence": (gfa({1: b"ACGT", 2: b"*"}, [("a", [(1, False)]), ("b", [(1, False), (2, True)])]), NEW,
                                    ["without a sequence", "'b'"]),
        "no_p_line": (gfa(ok, []), NEW, ["no P line"]),
    }
