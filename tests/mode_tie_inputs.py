"""Inputs of the mode-by-mirroring tests (test_modes_mirrored_host.py, test_modes_mirrored_gpu.py): --iterative,
--patch-inversions (plain and joined rule) and sparsified / sharded lists on families that have ties, so that the modes'
own kernels (sr_iter_unite_kernel, sr_inv_scan_kernel, the shard deal) meet secondaries that were emitted by symmetry,
aligned after their primary, deferred to the tail launch or replayed.  No tests here.

Every generator is seeded and deterministic and returns [(name, bytes)] over ACGT only (partners exist only at 2-bit symbols).
The seeds were found by search on the CPU with the oracle and ob.wfa_align_traced (the way tie_inputs.py chose its seeds);
what they give is pinned in test_modes_mirrored_host.py (PINNED).  The oracle's answers are computed once per process.

iter_ties.  22 members of 627 .. 654 bp under tree:1,0,1.0.  Input A's recipe (tie_inputs.blocks_family: 3 sites with
unrelated blocks of 20-45 bp in place of 0-10 bp) makes 6 haplotypes; member m is haplotype m mod 6 with 0.3 % substitutions
of its own.  Blocks private to every one of 22 members cannot stabilize: every pair (i, j) unites the bases of i's block with
the bases of j's block that happen to match next to a flank, classes of members that share d such bases have 22 / 4^d members,
and the unions of the small classes arrive spread over the whole random order -- measured on blocks_family(22 members, 560 bp,
3 sites) without any substitution: 77 count changes over 210 entries, the last in the last chunk, never 10 unchanged checks,
with -k 0, 8 and 16 alike.  With haplotypes the block-to-block unions of a haplotype pair are made by the first member pair
that shows it, and the counts settle.  Pairs of different haplotypes carry the ties (I-and-D ties in the backtrace,
breakpoint-diagonal and component ties), pairs of one haplotype are substitutions only.

inv_ties.  5 members of about 1 000 bp: 4 members of an Input-A-style blocks family (3 % substitutions, 2 block sites), all
with inversion_helpers' purine block (120 bp of A / G, which shares no base with its own reverse complement) at offset 10; C
and D carry the block inverted (one clean two-sided gap against A and B; D "plus its own blocks", as every member of a
blocks family has), E is A with the block replaced by 120 C (a candidate that is no better when patched).  Nobody is
reverse-complemented: all pairs are forward and can be partners.  The same seed serves the plain and the joined rule.

sparse_ties.  mirror_inputs.input_a() and tie_inputs "deep_ties" as they stand, under -x tree:2,1,0.5 and two shards.  The
list of -x tree: is symmetric, (q, t) and (t, q) cost the same and no other pair of these two families costs as much, so the
shard deal (longest first, to the lighter rank) sends the two orders of EVERY pair to different ranks: 12 and 14 partners on
the whole list, none in any shard.  tie_inputs "unequal_blocks_400" is the third family: there the two orders of some pairs land on one
rank, and each shard keeps 3 of the 13 partners (one of them non-transposable) and loses 7."""
import concurrent.futures
import functools

import numpy as np

import inversion_helpers as ih
import inversion_join_helpers as jh
import mirror_inputs as mi
import oracle_binding as ob
import tie_inputs as ti
from seqrush_amd import synth

_CODE = np.zeros(256, np.uint8)
_CODE[list(b"ACGT")] = range(4)

# ------------------------------------------------------------------------------------------ iter_ties
ITER_SEED, ITER_N, ITER_HAPLOTYPES, ITER_L, ITER_SUB, ITER_SITES = 28, 22, 6, 560, 0.003, 3
ITER_SPEC, ITER_K = "tree:1,0,1.0", 0
NEVER_SPEC, NEVER_N = "tree:1,1,1.0", 10
CHUNK = 10                                      # random entries per check (SR_ITER_CHECK_INTERVAL)


def iter_family(seed=ITER_SEED, n=ITER_N):
    haps = ti.blocks_family("h", seed, ITER_HAPLOTYPES, ITER_L, 0.0, ITER_SITES, lambda r: r.randint(20, 46), lambda r: r.randint(0, 11))
    out = []
    for m in range(n):
        codes = _CODE[np.frombuffer(haps[m % ITER_HAPLOTYPES][1], np.uint8)]
        out.append((f"it{m}", synth.to_bytes(synth.substitute(codes, ITER_SUB, 190000 + 100 * seed + m))))
    return out


# ------------------------------------------------------------------------------------------ inv_ties
INV_SEED, INV_AT, INV_LEN = 1, 10, 120
INV_NAME = "inv_ties"


def inv_family(seed=INV_SEED):
    base = ti.blocks_family("v", 300 + seed, 4, 950, 0.03, 2, lambda r: r.randint(20, 46), lambda r: r.randint(0, 11))
    blk = bytes(b"AG"[int(c) & 1] for c in synth.base_sequence(INV_LEN, 7300 + seed))
    s = [x[:INV_AT] + blk + x[INV_AT + INV_LEN:] for _, x in base]
    return [("A", s[0]), ("B", s[1]), ("C", synth.invert_segment(s[2], INV_AT, INV_LEN)),
            ("D", synth.invert_segment(s[3], INV_AT, INV_LEN)), ("E", s[0][:INV_AT] + b"C" * INV_LEN + s[0][INV_AT + INV_LEN:])]


ih.EXTRA[INV_NAME] = inv_family                 # inversion_helpers.restate and the joined restatement take inputs by name

# ------------------------------------------------------------------------------------------ sparse_ties
SPARSE_SPEC = "tree:2,1,0.5"
SPARSE = {"A": mi.input_a, "deep_ties": lambda: list(ti.records("deep_ties")),
          "unequal_blocks_400": lambda: list(ti.records("unequal_blocks_400"))}

SETS = {"iter_ties": iter_family, "iter_never": lambda: iter_family(n=NEVER_N), INV_NAME: inv_family, **{"sparse:" + k: v for k, v in SPARSE.items()}}


@functools.lru_cache(maxsize=None)
def records(name):
    return tuple(SETS[name]())


def _pool_map(fn, items):
    """the oracle is re-entrant (thread-local arenas) and ctypes drops the GIL: 484 pairs in a second instead of five"""
    with concurrent.futures.ThreadPoolExecutor(8) as pool:
        return list(pool.map(fn, items))


@functools.lru_cache(maxsize=None)
def oracle_once(name, kw=(), unite=True):
    """mirror_inputs.OracleOnce of an input: align_pair of every ordered pair, labels, GFA -- once, shared unchanged.
    unite=False: no labels and no GFA of the all-vs-all run (the iterative runs never make that partition)"""
    from test_gpu_parity import oracle_params
    recs = list(records(name))
    o, op, n = ob.OracleSeqRush(records=recs), oracle_params(**dict(kw)), len(recs)
    once = mi.OracleOnce.__new__(mi.OracleOnce)
    keys = [(q, t) for q in range(n) for t in range(n)]
    once.n, once.pairs = n, dict(zip(keys, _pool_map(lambda p: o.align_pair(op, *p), keys)))
    if unite:
        o.align_and_unite(op)
        once.labels, once.gfa_out = o.canonical_labels(), o.gfa(canonical=True)
    o.close()
    return once


def iter_oracle(name="iter_ties"):
    return oracle_once(name, (), False)


@functools.lru_cache(maxsize=None)
def iter_restated(name="iter_ties"):
    """test_iterative_gpu.restate of the input under its spec, once per process"""
    from test_iterative_gpu import restate
    spec = ITER_SPEC if name == "iter_ties" else NEVER_SPEC
    return restate(list(records(name)), spec, ITER_K)


def expand(entries):
    return [p for i, j in entries for p in ((i, i), (i, j), (j, i), (j, j))]


def iter_list(name="iter_ties"):
    ref = iter_restated(name)
    return expand(ref["tree"]) + expand(ref["random"])


def iter_windows(name="iter_ties", how="planned"):
    """batch_first of the iterative list as plan_memory (sr_host.cpp) cuts it: the tree entries in batches the arena holds,
    then phase-2 windows of whole chunks -- "planned": 10 chunks, doubling after each window (the arena holds the whole list),
    "chunk": SR_CIGAR_ARENA_OPS=1, which the load raises to the largest chunk: one chunk per window, "one": one window"""
    pairs = iter_list(name)
    lens = [len(s) for _, s in records(name)]
    ops = [lens[q] + lens[t] + 2 for q, t in pairs]
    tp, total, ch = 4 * len(iter_restated(name)["tree"]), len(pairs), 4 * CHUNK
    arena = max(sum(ops[f:f + ch]) for f in range(tp, total, ch)) + 1 if how == "chunk" else sum(ops) + 1
    first, used = [0], 0
    for i in range(tp):
        used += ops[i]
        if used + 1 > arena:
            first.append(i)
            used = ops[i]
    first.append(tp)
    f, target = tp, 1 << 30 if how == "one" else 10
    while f < total:
        l, chunks = f, 0
        while l < total and (chunks == 0 or chunks < target):
            e = min(total, l + ch)
            if chunks > 0 and sum(ops[f:e]) + 1 > arena:
                break
            l, chunks = e, chunks + 1
        first.append(l)
        f, target = l, 2 * target
    return first


def tree_batches(name="iter_ties", how="planned"):
    return iter_windows(name, how).index(4 * len(iter_restated(name)["tree"]))


def windows_that_ran(name="iter_ties", how="planned"):
    """number of batches of iter_windows() the run enqueues: the tree batches and every window up to the one whose check stops"""
    ref, first = iter_restated(name), iter_windows(name, how)
    if not ref["stabilized"]:
        return len(first) - 1
    stop = 4 * len(ref["tree"]) + 4 * ref["processed"]          # end of the chunk whose count decides the stop
    return next(b for b in range(1, len(first)) if first[b] >= stop)


# ------------------------------------------------------------------------------------------ lists and batches
NONE, SECONDARY = 0xffffffff, 0x80000000


def mirror_rule(pairs, batch_first, workgroups):
    """the rule in the comment above mirror_map (sr_pairs.cpp), restated -> (entries, primaries per batch)"""
    out, per_batch = [NONE] * len(pairs), []
    for f, l in zip(batch_first, batch_first[1:]):
        first, n = {}, 0
        for i in range(f, l):
            if pairs[i][0] != pairs[i][1]:
                first.setdefault(pairs[i], i)
        for i in range(f, l if l - f > workgroups else f):       # no more pairs than workgroups: no partners at all
            q, t = pairs[i]
            if q < t and first[q, t] == i and (t, q) in first:
                out[i], out[first[t, q]], n = first[t, q] - f, (i - f) | SECONDARY, n + 1
        per_batch.append(n)
    return out, per_batch


def arena_batches(lens, pairs, arena_ops):
    """batch_first of a list under SR_CIGAR_ARENA_OPS = arena_ops (plan_memory: a pair reserves |q| + |t| + 2 ops)"""
    arena_ops = max(arena_ops, max(lens[q] + lens[t] + 2 for q, t in pairs) + 1)
    first, used = [0], 0
    for i, (q, t) in enumerate(pairs):
        used += lens[q] + lens[t] + 2
        if used + 1 > arena_ops:
            first.append(i)
            used = lens[q] + lens[t] + 2
    return first + [len(pairs)]


def shard(lens, pairs, rank, count):
    """shard_pairs (sr_pairs.cpp) restated: pairs by cost (|q| * |t|, self pairs |q|), longest first and stable, each to the
    least loaded rank (lowest rank on ties); a rank keeps its pairs in list order"""
    cost = [lens[q] if q == t else lens[q] * lens[t] for q, t in pairs]
    load, mine = [0] * count, []
    for i in sorted(range(len(pairs)), key=lambda i: -cost[i]):
        r = min(range(count), key=lambda r: (load[r], r))
        load[r] += cost[i] or 1
        if r == rank:
            mine.append(i)
    return [pairs[i] for i in sorted(mine)]


@functools.lru_cache(maxsize=None)
def sparse_list(family):
    o = ob.OracleSeqRush(records=list(records("sparse:" + family)))
    pairs = o.sparsified_pairs(SPARSE_SPEC)
    o.close()
    return tuple(pairs)


def sparse_shards(family):
    lens = [len(s) for _, s in records("sparse:" + family)]
    return [shard(lens, list(sparse_list(family)), r, 2) for r in (0, 1)]


def lost_partners(family):
    """unordered pairs whose two orders are both on the sparsified list and were dealt to different shards"""
    whole, (s0, s1) = set(sparse_list(family)), sparse_shards(family)
    return sorted((q, t) for q, t in whole if q < t and (t, q) in whole and ((q, t) in s0) != ((t, q) in s0))


# ------------------------------------------------------------------------------------------ censuses
def census_of(name, pairs, scores=ti.DEFAULT_SCORES):
    """tie_inputs.Census over the given unordered forward pairs of one of this module's inputs"""
    recs = records(name)
    r, pen = ob.parse_scores(scores)
    assert r == 0
    c = ti.Census.__new__(ti.Census)
    c.name, c.n, c.pen, c.pairs, c.trace = name, len(recs), pen, sorted(pairs), {}
    both = [o for p in c.pairs for o in (p, p[::-1])]
    c.trace = dict(zip(both, _pool_map(lambda o: ti.PairTrace(recs[o[0]][1], recs[o[1]][1], pen), both)))
    return c


@functools.lru_cache(maxsize=None)
def census(name):
    """both orders of every unordered pair of the input through the traced oracle (all of them are forward)"""
    n = len(records(name))
    return census_of(name, [(q, t) for q in range(n) for t in range(q + 1, n)])


def with_gaps(o, p):
    return b"I" in o.pairs[p]["cigar"] or b"D" in o.pairs[p]["cigar"]


@functools.lru_cache(maxsize=None)
def iter_counts():
    """the conditions on iter_ties, from the restatement and the oracle alone"""
    ref, o = iter_restated(), iter_oracle()
    nt = set(o.non_transposable())
    done = ref["random"][:ref["processed"]]
    return dict(tree=len(ref["tree"]), random=len(ref["random"]), processed=ref["processed"], stabilized=ref["stabilized"],
                checks=len(ref["check_counts"]), distinct_counts=len(set(ref["check_counts"])),
                non_transposable=sum(e in nt for e in done),
                transposable_with_gaps=sum(e not in nt and with_gaps(o, e) for e in done),
                non_transposable_last_two_chunks=sum(e in nt for e in done[-2 * CHUNK:]))


@functools.lru_cache(maxsize=None)
def inv_counts():
    """the conditions on inv_ties under -k 8, from the two restatements and the oracle alone"""
    ref, jref, o = ih.restate(INV_NAME), jh.restate(INV_NAME), oracle_once(INV_NAME, (("min_match_len", ih.K),))
    nt = set(o.non_transposable())
    acc = {(j["query_idx"], j["target_idx"]) for j in ref["jobs"] if j["accepted"]}
    both = {(q, t) for q, t in acc if q < t and (t, q) in acc}
    return dict(jobs=len(ref["jobs"]), accepted=sum(j["accepted"] for j in ref["jobs"]),
                rejected=sum(not j["accepted"] for j in ref["jobs"]), non_transposable=len(nt),
                non_transposable_both_accepted=len(both & nt), transposable_both_accepted=len(both - nt),
                reverse=len(o.reverse_pairs()), joined_jobs=len(jref["jobs"]), joined_accepted=sum(j["accepted"] for j in jref["jobs"]),
                joined_islands=jref["islands"])
