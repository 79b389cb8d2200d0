"""The tie lattice (test_tie_lattice_host.py, test_tie_lattice_gpu.py): small seeded families, each named for the place in
the two tie rules of DESIGN.md 4.3 it stresses -- rule 1, the M step of the backtrace (an I tag and a D tag at the maximum
offset, without MISMS); rule 2, the breakpoint choice of an accepted overlap call (component order, diagonal direction).
Every generator is deterministic, returns [(name, bytes)] over ACGT only (partners exist only for 2-bit symbols) and stays
within 8 members of 1 600 bp (deep_ties: 3 000 bp), so that an all-vs-all takes the oracle about a second.

The seeds were chosen by search with the traced oracle (ob.wfa_align_traced) so that every family is not vacuous for what
it is named for; the counts they give are pinned in test_tie_lattice_host.py (PINNED).

Also here: the census -- both orders of every unordered forward pair through the traced oracle, once per process -- that
the host test asserts on and the GPU test takes its bounds from."""
import functools
import random

import numpy as np

import mirror_inputs as mi
import oracle_binding as ob
import repeat_inputs as ri
from seqrush_amd import synth

DEFAULT_SCORES = "0,5,8,2,24,1"
ONE_PIECE = "0,5,8,2"


def _codes(rng, n):
    return rng.randint(0, 4, size=int(n)).astype(np.uint8)


def blocks_family(prefix, seed, n, anc_len, sub, sites, block_len, eaten):
    """Input A's recipe (mirror_inputs.input_a): n members of one random ancestor, substitutions per member, and shared
    sites where every member carries its own unrelated random block of block_len() bases in place of eaten() ancestral
    ones"""
    rng = np.random.RandomState(seed)
    anc = synth.base_sequence(anc_len, 170000 + seed)
    margin = max(40, anc_len // 10)
    where = sorted(int(x) for x in rng.choice(np.arange(margin, anc_len - margin, 25), sites, replace=False))
    recs = []
    for m in range(n):
        codes = synth.substitute(anc, sub, 171000 + 100 * seed + m)
        parts, pos = [], 0
        for s in where:
            parts.append(codes[pos:s])
            parts.append(_codes(rng, block_len(rng)))
            pos = s + int(eaten(rng))
        parts.append(codes[pos:])
        recs.append((f"{prefix}{m}", synth.to_bytes(np.concatenate(parts))))
    return recs


EQUAL_SEED = {15: 2, 16: 19, 17: 1}


def equal_blocks(L, seed=None):
    """6 x ~900 bp, 2 % substitutions, 3 sites where every member carries its own unrelated block of exactly L bases in place
    of L ancestral ones.  Under 0,5,8,2,24,1 sixteen mismatches cost 80 and so do I(16) + D(16): MISMS, I-first and D-first
    meet at one offset (rule 1 with and without MISMS); L = 15 and 17 sit on either side"""
    seed = EQUAL_SEED[L] if seed is None else seed
    return blocks_family(f"e{L}_", seed, 6, 900, 0.02, 3, lambda r: L, lambda r: L)


UNEQUAL = {400: (2, 2), 800: (1, 3), 1600: (0, 4)}             # length -> (seed, sites)


def unequal_blocks(L, seed=None):
    """Input A's recipe at a total length of at most L: 6 members, 4 % substitutions (12 % at L = 400, so that its pairs
    still score about 500), blocks of 20-45 bases in place of 0-10:
    I-and-D ties in the backtrace, breakpoint-diagonal and component ties, scores from about 500 upward"""
    s0, sites = UNEQUAL[L]
    seed = s0 if seed is None else seed
    return blocks_family(f"u{L}_", seed, 6, L - 45 * sites, 0.04 if L > 400 else 0.12, sites, lambda r: r.randint(20, 46), lambda r: r.randint(0, 11))


COPY_UNITS = (2, 7, 40)
COPY_COUNTS = (3, 4, 5, 7, 9)
COPY_SEED = {2: 0, 7: 5, 40: 0}


def copy_number(u, seed=None):
    """unique flanks of 450 bp (3 % substitutions per member) around c tandem copies of one u-bp unit, c = 3, 4, 5, 7, 9: the
    one-sided gap between two members can sit in front of any copy -- diagonal ties within one component, which the
    transposed walk resolves from the other end"""
    seed = COPY_SEED[u] if seed is None else seed
    unit = synth.base_sequence(u, 172000 + 10 * seed + u)
    f1, f2 = synth.base_sequence(450, 173000 + seed), synth.base_sequence(450, 174000 + seed)
    recs = []
    for i, c in enumerate(COPY_COUNTS):
        a = synth.substitute(f1, 0.03, 175000 + 100 * seed + i)
        b = synth.substitute(f2, 0.03, 176000 + 100 * seed + i)
        recs.append((f"cn{u}x{c}", synth.to_bytes(np.concatenate([a] + [unit] * c + [b]))))
    return recs


def crossover_gaps(seed=3):
    """one unique 700-bp sequence, unchanged, and with one clean gap each: 15, 16, 17 bases deleted at one place, 15, 16, 17
    foreign bases inserted at another.  8 + 2 L = 24 + L at L = 16: piece-1 and piece-2 tags tie there, in both
    directions; 4.3 claims that place is symmetric and needs no rule"""
    base = ri.unique(700, 177000 + seed)
    recs = [("x0", base)]
    for L in (15, 16, 17):
        recs.append((f"del{L}", base[:230] + base[230 + L:]))
        recs.append((f"ins{L}", base[:470] + ri.unique(L, 178000 + seed + L) + base[470:]))
    return recs


LENGTH_EDGES = (99, 99, 100, 100, 101, 101)


def threshold_lengths(seed=5):
    """max(|q|, |t|) in {99, 100, 101} around SRO_BIALIGN_FALLBACK_MIN_LENGTH = 100: one 120-bp sequence, mutated per member
    (6 % substitutions, 4 % indels) and cut to the member's length"""
    rng = random.Random(179000 + seed)
    base = ri.unique(120, 179500 + seed)
    recs = []
    for i, L in enumerate(LENGTH_EDGES):
        m = ri.mutate(base, 0.06, 0.04, rng)
        recs.append((f"len{L}_{i}", m[:L]))
    assert [len(s) for _, s in recs] == list(LENGTH_EDGES)
    return recs


SCORE_SEED = 0


def threshold_scores(seed=None):
    """8 x ~620 bp at 6 % substitutions and 0.8 % indels per member: the two halves of a pair's depth-0 breakpoint score about
    250 each, and the seed is chosen so that 249, 250 and 251 (SRO_BIALIGN_FALLBACK_MIN_SCORE = 250: base case up to it,
    search above) all occur as a depth-1 score_remaining"""
    seed = SCORE_SEED if seed is None else seed
    rng = random.Random(180000 + seed)
    base = ri.unique(620, 180500 + seed)
    return [(f"sc{i}", ri.mutate(base, 0.06, 0.008, rng)) for i in range(8)]


SKEW_SEED = 1


def skewed(seed=None):
    """|q| about 120 against |t| about 1 500: three long members (3 % substitutions) and four short ones, each a 100-bp window
    of the ancestor with an unrelated 20-bp block in its middle -- k_end far from 0, the offset limits under k <-> -k"""
    seed = SKEW_SEED if seed is None else seed
    rng = np.random.RandomState(181000 + seed)
    anc = synth.base_sequence(1500, 181500 + seed)
    recs = [(f"long{i}", synth.to_bytes(synth.substitute(anc, 0.03, 182000 + 10 * seed + i))) for i in range(3)]
    for i in range(4):
        at = int(rng.randint(100, 1300))
        w = synth.substitute(anc, 0.03, 182500 + 10 * seed + i)[at:at + 100]
        recs.append((f"short{i}", synth.to_bytes(np.concatenate([w[:50], _codes(rng, 20), w[50:]]))))
    return recs


DEEP_SEED = 0


def deep_ties(seed=None):
    """6 x ~2 500 bp, 4 % substitutions, 7 block sites (Input A's recipe): pairs score 750 or more, searches reach depth 2 and
    deeper, and the seed is chosen so that several pairs have an unflagged depth-0 search above a flagged deeper record --
    the case the replay exists for"""
    seed = DEEP_SEED if seed is None else seed
    return blocks_family("d", seed, 6, 2400, 0.04, 7, lambda r: r.randint(20, 46), lambda r: r.randint(0, 11))


def one_reversed(seed=7):
    """5 x ~1 200 bp with indels and two block sites, member 2 reverse-complemented: its pairs align on the reverse strand"""
    recs = blocks_family("r", 500 + seed, 5, 1200, 0.04, 2, lambda r: r.randint(20, 46), lambda r: r.randint(0, 11))
    return [(n, synth.reverse_complement(s) if i == 2 else s) for i, (n, s) in enumerate(recs)]


def palindromic(seed=9):
    """repeat_inputs.palindromes at 2 x 300 bp: members equal to their reverse complement (both orientation scores equal:
    forward wins) and near-palindromes one substitution away"""
    return ri.palindromes(seed=183000 + seed, half=300)[:8]


FORWARD = {
    "equal_blocks_15": lambda: equal_blocks(15), "equal_blocks_16": lambda: equal_blocks(16), "equal_blocks_17": lambda: equal_blocks(17),
    "unequal_blocks_400": lambda: unequal_blocks(400), "unequal_blocks_800": lambda: unequal_blocks(800),
    "unequal_blocks_1600": lambda: unequal_blocks(1600),
    "copy_number_2": lambda: copy_number(2), "copy_number_7": lambda: copy_number(7), "copy_number_40": lambda: copy_number(40),
    "crossover_gaps": crossover_gaps, "threshold_lengths": threshold_lengths, "threshold_scores": threshold_scores,
    "skewed": skewed, "deep_ties": deep_ties,
}
STRANDED = {"one_reversed": one_reversed, "palindromic": palindromic}
FAMILIES = dict(FORWARD, **STRANDED)
# the input conditions (at least 2 non-transposable pairs, at least 2 transposable ones with gaps) hold for these
CONDITIONED = ("equal_blocks_15", "equal_blocks_16", "equal_blocks_17", "unequal_blocks_400", "unequal_blocks_800",
               "unequal_blocks_1600", "skewed", "deep_ties")


@functools.lru_cache(maxsize=None)
def records(name):
    return tuple(FAMILIES[name]())


@functools.lru_cache(maxsize=None)
def oracle_once(name, kw=()):
    """mirror_inputs.OracleOnce of a family: align_pair of every ordered pair, labels, GFA -- computed once, shared unchanged"""
    return mi.OracleOnce(list(records(name)), dict(kw))


# ------------------------------------------------------------------------------------------ the census
M, I1, I2, D1, D2 = range(5)
COMP_T = {M: M, I1: D1, I2: D2, D1: I1, D2: I2}


def seg_key(r):
    return (r["pb"], r["pe"], r["tb"], r["te"], r["cb"], r["ce"])


def seg_key_t(r):
    """the segment of the transposed pair a record speaks about (sr_bprec_t's mapping, restated)"""
    return (r["tb"], r["te"], r["pb"], r["pe"], COMP_T[r["cb"]], COMP_T[r["ce"]])


def with_ancestors(recs):
    """recursion order -> every record gets "anc_tie": a tie bit on some search above it (the records are a pre-order walk:
    the parent of a record at depth d is the last search at depth d - 1 before it)"""
    last = {}
    for r in recs:
        up = last.get(r["depth"] - 1)
        r["anc_tie"] = bool(up and (up["tie"] or up["anc_tie"]))
        if r["kind"] == ob.TRACE_SEARCH:
            last[r["depth"]] = r
    return recs


class PairTrace:
    def __init__(self, q, t, pen):
        self.cigar, self.score, recs = ob.wfa_align_traced(q, t, pen)
        self.recs = with_ancestors(recs)
        self.searches = [r for r in self.recs if r["kind"] == ob.TRACE_SEARCH]
        self.leaves = [r for r in self.recs if r["kind"] != ob.TRACE_SEARCH]
        self.flagged = any(r["tie"] for r in self.recs)
        self.by_seg = {(r["kind"] == ob.TRACE_SEARCH, seg_key(r)): r for r in self.recs}

    def twin_of(self, r):
        """this trace's record of the transposed segment of r (a record of the other order), or None"""
        return self.by_seg.get((r["kind"] == ob.TRACE_SEARCH, seg_key_t(r)))


def transposed_search(r, other):
    """r: an unflagged search under unflagged ancestors -> its twin in the other order's trace, checked to be the transposed
    breakpoint with the same two scores"""
    w = other.twin_of(r)
    assert w is not None, ("no search of the transposed segment", r)
    assert (w["bv"], w["bh"], w["comp"], w["score_f"], w["score_r"]) == (r["bh"], r["bv"], COMP_T[r["comp"]], r["score_f"], r["score_r"]), (r, w)
    return w


class Census:
    """both orders of every unordered pair of a family that the oracle aligns on the forward strand both ways, through the
    traced oracle; scores: the penalty string"""

    def __init__(self, name, scores=DEFAULT_SCORES, forward_pairs=None):
        recs = records(name)
        r, pen = ob.parse_scores(scores); assert r == 0
        n = len(recs)
        self.name, self.n, self.pen = name, n, pen
        if forward_pairs is None:
            forward_pairs = [(q, t) for q in range(n) for t in range(q + 1, n)]
        self.pairs = list(forward_pairs)
        self.trace = {}
        for q, t in self.pairs:
            self.trace[q, t] = PairTrace(recs[q][1], recs[t][1], pen)
            self.trace[t, q] = PairTrace(recs[t][1], recs[q][1], pen)

    def transposable(self, q, t):
        return mi.transpose(self.trace[q, t].cigar) == self.trace[t, q].cigar

    def non_transposable(self):
        return [p for p in self.pairs if not self.transposable(*p)]

    def flagged(self):
        """unordered pairs with a bit in either order (the bits of the two orders agree record by record where both exist;
        below a flagged search the two recursion trees may differ)"""
        return [(q, t) for q, t in self.pairs if self.trace[q, t].flagged or self.trace[t, q].flagged]

    def primary_flagged(self):
        """unordered pairs whose primary (q, t), q < t -- what the device aligns first -- carries a bit"""
        return [(q, t) for q, t in self.pairs if self.trace[q, t].flagged]

    def transposable_searches(self, q, t):
        """searches of (q, t) with no bit on them and none above"""
        return [r for r in self.trace[q, t].searches if not r["tie"] and not r["anc_tie"]]

    def replayable(self, q, t):
        """how many searches of the secondary (t, q) the kernel's walk (its host twin sr_replay_match_host) takes from the
        records of the primary (q, t) when those carry the oracle's bits -- the device, which may flag more, takes no more;
        test_tie_lattice_host.py checks every one of these matches"""
        import ctypes as C
        from seqrush_amd import _lib
        L = _lib.load()
        recs = sorted(self.trace[q, t].searches, key=lambda r: (r["depth"], r["pb"] + r["tb"]))
        flat = [x for r in recs for x in (r["depth"], r["pb"], r["pe"], r["tb"], r["te"], r["cb"], r["ce"], r["bv"], r["bh"], r["comp"],
                                          r["score_f"], r["score_r"], r["tie"], 0, 0, 0)]
        arr = (C.c_int * max(1, len(flat)))(*flat)
        sec = self.trace[t, q].searches
        n = 0
        for level in sorted({r["depth"] for r in sec}):
            segs = sorted((r for r in sec if r["depth"] == level), key=lambda r: r["pb"] + r["tb"])
            sarr = (C.c_int * (6 * len(segs)))(*[x for r in segs for x in seg_key(r)])
            out = (C.c_int * len(segs))()
            n += L.sr_replay_match_host(arr, len(recs), sarr, len(segs), level, out)
        return n

    def deep_tie_pairs(self):
        """pairs whose primary has an unflagged depth-0 search and a flagged record below it: what the replay is for"""
        out = []
        for q, t in self.pairs:
            tr = self.trace[q, t]
            if tr.searches and not tr.searches[0]["tie"] and tr.flagged:
                out.append((q, t))
        return out

    def row(self):
        """the family's line of the census table of DESIGN.md 4.3"""
        nt, fl = set(self.non_transposable()), set(self.flagged())
        s_all = sum(len(self.trace[p].searches) + len(self.trace[p[::-1]].searches) for p in self.pairs)
        s_fl = sum(r["tie"] for p in self.pairs for o in (p, p[::-1]) for r in self.trace[o].searches)
        b_fl = sum(r["tie"] for p in self.pairs for o in (p, p[::-1]) for r in self.trace[o].leaves)
        return dict(pairs=len(self.pairs), non_transposable=len(nt), flagged=len(fl), unflagged_but_different=len(nt - fl),
                    searches=s_all, rule2_searches=s_fl, rule1_base_cases=b_fl,
                    max_depth=max((r["depth"] for p in self.trace.values() for r in p.recs), default=0))


@functools.lru_cache(maxsize=None)
def census(name, scores=DEFAULT_SCORES):
    fwd = None
    if name in STRANDED:
        o = oracle_once(name, (("scores", scores),) if scores != DEFAULT_SCORES else ())
        fwd = [(q, t) for q in range(o.n) for t in range(q + 1, o.n) if not o.pairs[q, t]["is_reverse"] and not o.pairs[t, q]["is_reverse"]]
    return Census(name, scores, fwd)
