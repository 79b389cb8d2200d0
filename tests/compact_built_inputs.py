"""Seeded GFA texts built by hand for compaction by tables (test_compact_built_host.py, test_compact_built_gpu.py; plain
helper module, no GPU use).  Induced graphs and the hand cases of compact_inputs.py give the kernels of sr_compact.hip lists
of a few dozen handles, two rounds and single-base nodes; the builders here put list lengths, handle counts and step counts
on the kernels' own seams: lists of 2^k - 1 / 2^k / 2^k + 1 members (pointer jumping), NH = 2 * NN at a scan tile edge of
1024 and past 256 tiles (the second pass of the tile-sum scan), more steps than 8192 x 256 threads (ct_kernel's grid-stride
loop), several rounds on multi-base nodes with dead slots, chains refused inside long lists (by a path that starts, ends or turns inside them, or
that hops onto a member from elsewhere), and an irregular list beside a regular one.

Every builder takes an id order: "asc", "desc" or "perm" (seeded shuffle).  The chain rule depends on id order: "desc" makes
the mirror list win as one reverse-complemented chain, "perm" gives prefix-minimum chains and several rounds.  Node
sequences are 1 to 5 bytes of ACGTacgtNn, so text offsets are uneven and rc_node_base has work to do.

CASES maps a name to (builder, arguments, oracle?).  The oracle's compact() restates the reference and is quadratic in list
length (0.03 s at 2 000 nodes, minutes at 131 100), so it runs on every case of at most ORACLE_MAX_NODES nodes and not on the
two large families; there the reference is the host procedure, which the same builders pin to the oracle at the small
sizes.  The grid-stride loop of the per-handle functors (NH > 2 097 152: 1.05 M nodes, 46 MB of text) is left out: it is the
same ct_kernel<F> template that the step-indexed case takes through its loop.  Texts are built once (case() is cached) with
joins over precomputed step strings."""
import functools
import random

from compact_inputs import gfa

ALPHABET = "ACGTacgtNn"
ORACLE_MAX_NODES = 8192
PERMUTE_MAX_NODES = 2000                              # cases up to here also run with their node ids permuted


def _ids(n, order, seed):
    """node id of every position of the construction order"""
    ids = list(range(1, n + 1))
    if order == "desc":
        ids.reverse()
    elif order == "perm":
        random.Random(seed).shuffle(ids)
    elif order != "asc":
        raise KeyError(order)
    return ids


def _segments(ids, seed):
    r = random.Random(f"seq:{seed}:{len(ids)}")
    seqs = ["".join(r.choice(ALPHABET) for _ in range(r.randint(1, 5))) for _ in ids]
    return sorted(zip(ids, seqs))


def _walk(fwd, rev, start, end, reverse):
    """steps over the positions [start, end) of a list, or back over them on the other strand"""
    return rev[start:end][::-1] if reverse else fwd[start:end]


def long_chain(n, order, seed=0, extra=()):
    """one path over n nodes; extra: sub-walks (name, start, end, reversed) that start or end inside the list or traverse it
    on the other strand"""
    ids = _ids(n, order, seed)
    fwd, rev = [f"{i}+" for i in ids], [f"{i}-" for i in ids]
    paths = [("p", fwd)] + [(name, _walk(fwd, rev, s, e, r)) for name, s, e, r in extra]
    return gfa(_segments(ids, seed), list(zip(fwd, fwd[1:])), paths)


def hopping_chain(n, order, seed=0, hops=()):
    """one path over n nodes and a second one made of the sub-walks (start, end, reversed) back to back: between two of
    them it steps onto a member from a node that is not the member before it, without an L line"""
    ids = _ids(n, order, seed)
    fwd, rev = [f"{i}+" for i in ids], [f"{i}-" for i in ids]
    hop = [st for s, e, r in hops for st in _walk(fwd, rev, s, e, r)]
    return gfa(_segments(ids, seed), list(zip(fwd, fwd[1:])), [("p", fwd), ("h", hop)])


def bubbles(runs, npaths, order, seed=0):
    """anchor runs of the given lengths separated by two-allele bubbles; path 0 takes every first allele, path 1 every
    second, the others draw; every third path runs on the reverse strand"""
    n = sum(runs) + 2 * (len(runs) - 1)
    ids = _ids(n, order, seed)
    fwd, rev = [f"{i}+" for i in ids], [f"{i}-" for i in ids]
    links, at, spans, alleles = [], 0, [], []
    for k, L in enumerate(runs):
        spans.append((at, at + L))
        links += zip(fwd[at:at + L - 1], fwd[at + 1:at + L])
        at += L
        if k + 1 < len(runs):
            alleles.append((at, at + 1))
            for a in (at, at + 1):
                links += [(fwd[a - 1 if a == at else a - 2], fwd[a]), (fwd[a], fwd[at + 2])]
            at += 2
    run_f = [",".join(fwd[s:e]) for s, e in spans]
    run_r = [",".join(rev[s:e][::-1]) for s, e in spans]
    r = random.Random(f"bubbles:{seed}:{n}")
    lines = []
    for p in range(npaths):
        pick = [p if p < 2 else r.randrange(2) for _ in alleles]
        parts = []
        for k in range(len(runs)):
            parts.append(run_r[k] if p % 3 == 2 else run_f[k])
            if k < len(alleles):
                parts.append((rev if p % 3 == 2 else fwd)[alleles[k][pick[k]]])
        if p % 3 == 2:
            parts.reverse()
        lines.append(f"P\tq{p}\t{','.join(parts)}\t*")
    return gfa(_segments(ids, seed), links, []) + "\n".join(lines) + "\n"


def cycle_and_chain(n_cycle, n_chain, seed=0):
    """a cycle that no path visits (a list without a head: irregular) beside a chain that one path walks forward and another
    in reverse; the chain's ids zigzag, so it needs rounds after the one that merges the cycle on the host"""
    cyc = [f"{i}+" for i in range(1, n_cycle + 1)]
    order = list(range(n_cycle + 1, n_cycle + n_chain + 1))
    order = [x for pair in zip(order[n_chain // 2:], order[:n_chain // 2]) for x in pair] + order[2 * (n_chain // 2):]
    fwd, rev = [f"{i}+" for i in order], [f"{i}-" for i in order]
    links = list(zip(cyc, cyc[1:] + cyc[:1])) + list(zip(fwd, fwd[1:]))
    return gfa(_segments(list(range(1, n_cycle + n_chain + 1)), seed), links, [("p", fwd), ("q", rev[::-1])])


def hairpin(n, seed=0):
    """one path out along n nodes and back on the other strand through the self-mirror edge n+ -> n-"""
    ids = _ids(n, "asc", seed)
    fwd, rev = [f"{i}+" for i in ids], [f"{i}-" for i in ids]
    return gfa(_segments(ids, seed), list(zip(fwd, fwd[1:])) + [(fwd[-1], rev[-1])], [("p", fwd + rev[::-1])])


def two_way_links(n, seed=0):
    """a chain whose L lines are given forward everywhere; every third is also given as its mirror (b- -> a-: it counts
    twice in fcnt and breaks the link), every fifth is repeated (which must not)"""
    ids = _ids(n, "asc", seed)
    fwd, rev = [f"{i}+" for i in ids], [f"{i}-" for i in ids]
    links = []
    for k in range(n - 1):
        links.append((fwd[k], fwd[k + 1]))
        if k % 3 == 0:
            links.append((rev[k + 1], rev[k]))
        if k % 5 == 0:
            links.append((fwd[k], fwd[k + 1]))
    return gfa(_segments(ids, seed), links, [("p", fwd)])


SUBWALKS = (("w0", 250, 400, False), ("w1", 100, 300, True), ("w2", 0, 50, False), ("w3", 580, 600, True))
HOPS = ((0, 50, False), (300, 350, False), (450, 500, True), (120, 180, False), (590, 600, True))
SEAM_RUNS =(1, 2, 3, 63, 64, 65, 255, 256, 257, 1)
CHAIN_SIZES = (127, 128, 129, 511, 512, 513, 2000)
# seeds of the shuffled chains: the host procedure takes at least 3 rounds on the chains of 511 nodes and more with them
# (asserted in test_compact_built_host.py)
PERM_SEED = {127: 127, 128: 128, 129: 129, 511: 511, 512: 512, 513: 513, 2000: 2000, 131100: 131100}


def _cases():
    c = {}
    for n in CHAIN_SIZES:
        for order in ("asc", "desc", "perm"):
            c[f"chain-{n}-{order}"] = (long_chain, (n, order, PERM_SEED[n]), n)
    for order in ("perm", "asc"):
        c[f"subwalks-600-{order}"] = (long_chain, (600, order, 600, SUBWALKS), 600)
        c[f"hops-600-{order}"] = (hopping_chain, (600, order, 600, HOPS), 600)
        c[f"bubbles-seams-{order}"] = (bubbles, (SEAM_RUNS, 6, order, 6), sum(SEAM_RUNS) + 18)
    c["cycle-300-chain-700"] = (cycle_and_chain, (300, 700), 1000)
    c["hairpin-400"] = (hairpin, (400,), 400)
    c["two-way-links-300"] = (two_way_links, (300,), 300)
    for order in ("asc", "perm"):
        c[f"chain-131100-{order}"] = (long_chain, (131100, order, PERM_SEED[131100]), 131100)
    c["bubbles-stride-perm"] = (bubbles, ((4000,) * 10, 53, "perm", 53), 40018)
    return c


CASES = _cases()                                      # name -> (builder, arguments, nodes)
NAMES = tuple(CASES)
LARGE = tuple(n for n in NAMES if CASES[n][2] > ORACLE_MAX_NODES)


def nodes(name):
    return CASES[name][2]


def with_oracle(name):
    return nodes(name) <= ORACLE_MAX_NODES


@functools.lru_cache(maxsize=None)
def case(name):
    f, args, _ = CASES[name]
    return f(*args)
