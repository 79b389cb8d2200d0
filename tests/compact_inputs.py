"""Inputs shared by the tests of compaction by tables (test_compact_device_host.py, test_compact_device_gpu.py):
hand-written GFAs, seeded random families, node id permutation and the path spelling check."""
import random

from seqrush_amd import synth

RC = bytes.maketrans(b"ACGTacgtNn", b"TGCATGCANN")


def gfa(segs, links, paths):
    out = ["H\tVN:Z:1.0"]
    out += [f"S\t{i}\t{s}" for i, s in segs]
    out += [f"L\t{a[:-1]}\t{a[-1]}\t{b[:-1]}\t{b[-1]}\t0M" for a, b in links]
    out += [f"P\t{n}\t{','.join(st)}\t*" for n, st in paths]
    return "\n".join(out) + "\n"


def _chain(ids, seqs=("ACG", "T", "GGA", "CC", "TAT")):
    steps = [f"{i}+" for i in ids]
    return gfa([(i, seqs[k % len(seqs)]) for k, i in enumerate(sorted(ids))], list(zip(steps, steps[1:])), [("p", steps)])


# name -> (text, may_use_host_round)
HAND = {
    # 2 -> 1 -> 3: the search from 1+ takes [1+, 3+] first, 2+ joins a round later
    "middle-min": (_chain([2, 1, 3]), False),
    # the minimum is the list's tail: its forward chain has one member and the mirror list [1-, 2-, 3-] is merged
    "min-last": (_chain([3, 2, 1]), False),
    "ascending": (_chain([1, 2, 3, 4, 5]), False),
    "zigzag": (_chain([4, 2, 5, 1, 3]), False),
    # a path that starts inside the chain: merge_component_v2 refuses it, nothing is merged
    "starts-inside": (gfa([(1, "AC"), (2, "G"), (3, "TT")], [("1+", "2+"), ("2+", "3+")],
                          [("a", ["1+", "2+", "3+"]), ("b", ["2+", "3+"])]), False),
    "ends-inside-rc": (gfa([(1, "AC"), (2, "G"), (3, "TT"), (4, "A")], [("1+", "2+"), ("2+", "3+"), ("3+", "4+")],
                           [("a", ["1+", "2+", "3+", "4+"]), ("b", ["3-", "2-"])]), False),
    # a path step without its L line: the occurrence of 3+ after 1+ is no traversal of [2+, 3+]
    "step-without-edge": (gfa([(1, "AC"), (2, "G"), (3, "TT")], [("1+", "2+"), ("2+", "3+")],
                              [("a", ["1+", "2+", "3+"]), ("b", ["1+", "3+"])]), False),
    "hairpin": (gfa([(1, "ACG"), (2, "TT")], [("1+", "2+"), ("2+", "2-")], [("p", ["1+", "2+", "2-", "1-"])]), True),
    "hairpin-self": (gfa([(1, "ACG")], [("1+", "1-")], [("p", ["1+", "1-"])]), True),
    # an isolated cycle with no path on it: a list without a head
    "cycle": (gfa([(1, "A"), (2, "CC"), (3, "G"), (4, "TTT")], [("1+", "2+"), ("2+", "3+"), ("3+", "1+")], [("p", ["4+"])]), True),
    "cycle-and-chain": (gfa([(1, "A"), (2, "CC"), (3, "G"), (4, "TTT"), (5, "AG"), (6, "C")],
                            [("1+", "2+"), ("2+", "3+"), ("3+", "1+"), ("6+", "4+"), ("4+", "5+")],
                            [("p", ["6+", "4+", "5+"]), ("q", ["5-", "4-", "6-"])]), True),
    "no-paths": (gfa([(1, "A"), (2, "CC"), (3, "G")], [("1+", "2+"), ("2-", "3+")], []), False),
    "empty": ("H\tVN:Z:1.0\n", False),
}


def parse(text):
    seg, links, paths = {}, [], []
    for l in text.split("\n"):
        f = l.split("\t")
        if f[0] == "S":
            seg[f[1]] = f[2].encode()
        elif f[0] == "L":
            links.append((f[1] + f[2], f[3] + f[4]))
        elif f[0] == "P":
            paths.append((f[1], f[2].split(",") if f[2] else []))
    return seg, links, paths


def spelled(text):
    """path name -> bases (upper case: a reversed member is stored reverse-complemented by rc_node_base, which
    upper-cases)"""
    seg, _, paths = parse(text)
    return [(n, b"".join(seg[s[:-1]] if s[-1] == "+" else seg[s[:-1]].translate(RC)[::-1] for s in st).upper()) for n, st in paths]


def permuted(text, seed):
    """the same graph with its node ids permuted (the chain rule depends on id order)"""
    seg, links, paths = parse(text)
    ids = sorted(seg, key=int)
    new = list(range(1, len(ids) + 1))
    random.Random(seed).shuffle(new)
    m = {o: str(n) for o, n in zip(ids, new)}
    return gfa([(m[i], seg[i].decode()) for i in ids], [(m[a[:-1]] + a[-1], m[b[:-1]] + b[-1]) for a, b in links],
               [(n, [m[s[:-1]] + s[-1] for s in st]) for n, st in paths])


def random_family(seed):
    """3 to 6 sequences of 40 to 200 bp: SNPs or indels, reverse-complemented members, a suffix and a prefix fragment"""
    r = random.Random(seed)
    n, L = r.randint(3, 6), r.randint(40, 200)
    if r.random() < 0.5:
        recs = synth.snp_family(n, L, r.choice([0.0, 0.02, 0.05, 0.1]), seed, rc_every=r.choice([0, 0, 2, 3]))
    else:
        recs = synth.indel_family(n, L, r.choice([0.01, 0.03]), r.choice([0.01, 0.03, 0.06]), seed)
        if r.random() < 0.5:
            recs = [(nm, s if i % 2 else synth.reverse_complement(s)) for i, (nm, s) in enumerate(recs)]
    kind = r.randrange(4)
    if kind and len(recs) > 2:
        base = recs[0][1]
        cut = r.randint(1, len(base) - 2)
        recs = list(recs[:-1]) if len(recs) > 3 else list(recs)
        if kind & 1:
            recs.append(("suffix", base[cut:]))
        if kind & 2:
            recs.append(("prefix", synth.reverse_complement(base[:cut]) if r.random() < 0.3 else base[:cut]))
    return recs
