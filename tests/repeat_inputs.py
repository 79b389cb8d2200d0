"""Seeded low-complexity, repeat and palindromic inputs (plain helper module): the inputs on which optimal alignments are
NOT locally unique, so that the choice between equal candidates -- wavefront predecessors, biWFA breakpoint diagonals,
orientation at equal scores, k-nearest at equal Jaccard fractions, union-find roots under contention -- is what a
comparison with the oracle tests.  Every generator is deterministic (random.Random(seed) / synth's counter streams) and
returns [(name, bytes)]."""
import random

from seqrush_amd import synth

rc = synth.reverse_complement
ACGT = b"ACGT"


def unique(L, seed):
    """iid uniform ACGT (synth's counter stream)"""
    return synth.to_bytes(synth.base_sequence(L, seed))


def mutate(seq, sub, indel, rng, alphabet=ACGT, max_indel=3):
    """per base: substitution by another letter of the alphabet (prob. sub), deletion (indel / 2), insertion of
    1..max_indel letters behind it (indel / 2)"""
    out = bytearray()
    for ch in seq:
        u = rng.random()
        if u < sub:
            out.append(rng.choice([c for c in alphabet if c != ch] or list(alphabet)))
        elif u < sub + indel / 2:
            continue
        elif u < sub + indel:
            out.append(ch)
            out.extend(rng.choice(alphabet) for _ in range(rng.randint(1, max_indel)))
        else:
            out.append(ch)
    return bytes(out) or bytes(alphabet[:1])


# ------------------------------------------------------------------------------------------ families
HOMO_L = (15, 16, 17, 63, 64, 65, 255, 256, 257)
HOMO_D = (1, 15, 16, 17, 63)


def homopolymers(lengths=HOMO_L, diffs=HOMO_D, n_member=64):
    """A x L and A x (L - d) for every L and d (one member per distinct length: all-vs-all holds every such pair; clean
    gaps of 15, 16 and 17 sit on both sides of the two gap pieces' crossover), plus an N x n_member member (4-bit
    symbol buffer)"""
    ls = sorted({L for L in lengths} | {L - d for L in lengths for d in diffs if L - d >= 1})
    return [(f"A{L}", b"A" * L) for L in ls] + ([(f"N{n_member}", b"N" * n_member)] if n_member else [])


def homopolymers_1500():
    """the same at L = 1500, a family of its own: its pairs with the short members would be gaps of a thousand bases,
    which cost the oracle a minute and test nothing the short ones do not"""
    return homopolymers(lengths=(1500,), n_member=0)


MICRO_UNITS = (b"AC", b"CAG", b"GATA", b"TTAGGG")


def microsatellites(seed=11):
    """periods 2, 3, 4, 6: per unit a clean array, one with more copies (length differences 16, 15, 16, 18), one that ends
    in a partial unit (CAG: 17 more bases) and a mutated copy (2 % substitutions, 1 % indels)"""
    rng = random.Random(seed)
    out = []
    for unit, n, more in zip(MICRO_UNITS, (50, 40, 30, 22), (8, 5, 4, 3)):
        nm = unit.decode()
        a = unit * n
        out += [(f"{nm}x{n}", a), (f"{nm}x{n + more}", unit * (n + more)),
                (f"{nm}x{n + more}p", unit * (n + more) + unit[:len(unit) - 1]),
                (f"{nm}x{n}m", mutate(a, 0.02, 0.01, rng))]
    return out


def embedded(seed=21):
    """unique flank + (GT)n + unique flank with n = 20, 28, 37 (and a mutated copy), and a segmental duplication
    A B A' against A B"""
    rng = random.Random(seed)
    f1, f2 = unique(80, seed + 1), unique(80, seed + 2)
    out = [(f"gt{n}", f1 + b"GT" * n + f2) for n in (20, 28, 37)]
    out.append(("gt28m", mutate(f1 + b"GT" * 28 + f2, 0.02, 0.01, rng)))
    a, b = unique(120, seed + 3), unique(60, seed + 4)
    out += [("ab", a + b), ("aba", a + b + mutate(a, 0.02, 0.0, rng))]
    return out


def satellite_array(unit, copies, div, rng):
    return b"".join(mutate(unit, div * 0.8, div * 0.2, rng) for _ in range(copies))


def satellite(seed=31, unit_len=171, copies=(5, 6, 7, 8, 9)):
    """alpha-satellite-like arrays: a 171-bp unit, 5 to 9 copies, every copy diverged by 2-3 % on its own, one member
    reverse-complemented"""
    rng = random.Random(seed)
    unit = unique(unit_len, seed + 1)
    out = []
    for i, c in enumerate(copies):
        s = satellite_array(unit, c, 0.02 + 0.01 * (i % 2), rng)
        out.append((f"sat{c}" + ("rc" if i == 2 else ""), rc(s) if i == 2 else s))
    return out


def _other(ch, avoid=()):
    return next(c for c in ACGT if c != ch and c not in avoid)


def palindromes(seed=41, half=60):
    """sequences equal to their own reverse complement -- s + rc(s), (AT)n, (ACGT)n, symmetric truncations -- and near-
    palindromes one substitution away from one:
      near1:  first half, position i          near2: the mirror position n-1-i, not the complementary letter
      near1b: position i again, another letter
    so that rc(near1) is one mismatch from near2 and two from near1b (forward: two and one)"""
    s = unique(half, seed)
    p = s + rc(s)
    n, i = len(p), half // 3
    a = _other(p[i])
    near1 = p[:i] + bytes([a]) + p[i + 1:]
    mirror = rc(bytes([a]))[0]                          # what rc(near1) holds at n-1-i
    near2 = p[:n - 1 - i] + bytes([_other(p[n - 1 - i], avoid=(mirror,))]) + p[n - i:]
    near1b = p[:i] + bytes([_other(p[i], avoid=(a,))]) + p[i + 1:]
    return [("pal", p), ("near1", near1), ("near2", near2), ("near1b", near1b), ("at", b"AT" * 40), ("acgt", b"ACGT" * 25),
            ("pal_head", p[:n - 20]), ("pal_tail", p[13:]), ("pal_mid", p[7:n - 7]), ("at_odd", b"AT" * 33 + b"A")]


PALINDROMIC = ("pal", "at", "acgt", "pal_mid")          # members of palindromes() equal to their reverse complement


def two_letter(seed=51, L=300):
    """iid over {A, T} only (every 8-mer set is small and shared with the reverse complement), mutated copies within
    the alphabet, one of them reverse-complemented"""
    rng = random.Random(seed)
    base = bytes(rng.choice(b"AT") for _ in range(L))
    out = [("at0", base)]
    for i in range(1, 4):
        m = mutate(base, 0.03, 0.01, rng, alphabet=b"AT")
        out.append((f"at{i}" + ("rc" if i == 2 else ""), rc(m) if i == 2 else m))
    return out


def long_satellite(seed=61):
    """{"ring34k": a pair of ~34 kb satellite arrays (32-bit searches on the 16-bit ring), "deep12k": a pair of ~12 kb at
    ~10 % divergence (searches thousands of levels deep)}"""
    rng = random.Random(seed)
    unit = unique(171, seed + 1)
    clean = satellite_array(unit, 200, 0.02, rng)       # one array, units 2 % apart; the members diverge from it
    ring = [("ring_a", mutate(clean, 0.004, 0.001, rng)), ("ring_b", mutate(clean, 0.004, 0.001, rng))]
    clean = satellite_array(unit, 70, 0.02, rng)
    deep = [("deep_a", mutate(clean, 0.045, 0.005, rng)), ("deep_b", mutate(clean, 0.045, 0.005, rng))]
    return {"ring34k": ring, "deep12k": deep}


SMALL_FAMILIES = {
    "homopolymers": homopolymers,
    "homopolymers_1500": homopolymers_1500,
    "microsatellites": microsatellites,
    "embedded": embedded,
    "satellite": satellite,
    "palindromes": palindromes,
    "two_letter": two_letter,
}
MUTATED_FAMILIES = ("microsatellites", "embedded", "satellite", "two_letter")


# ------------------------------------------------------------------------------------------ seeded mixtures
def random_repeat_set(seed):
    """-> (records, min_match_len): 2-6 members of length 1..400 derived from one repeat-structured base (drawn from the
    families above) by mutation, truncation at either end and reverse complement; mirrors test_randomised_small_sets"""
    rng = random.Random(77000 + seed)
    L = rng.choice([1, 2, 7, 15, 16, 17, 33, 64, 65, 120, 255, 256, 257, 400])
    kind = rng.choice(["homopolymer", "microsatellite", "embedded", "satellite", "palindrome", "two_letter"])
    alphabet = ACGT
    if kind == "homopolymer":
        base = bytes([rng.choice(ACGT)]) * L
    elif kind == "microsatellite":
        unit = rng.choice(MICRO_UNITS + (b"AT", b"ACGT"))
        base = (unit * (L // len(unit) + 1))[:L]
    elif kind == "embedded":
        f = max(1, L // 4)
        base = (unique(f, 78000 + seed) + b"GT" * L)[:max(1, L - f)] + unique(f, 79000 + seed)
    elif kind == "satellite":
        unit = unique(rng.choice([5, 12, 31]), 80000 + seed)
        base = satellite_array(unit, L // len(unit) + 1, 0.03, rng)[:L]
    elif kind == "palindrome":
        h = unique(max(1, L // 2), 81000 + seed)
        base = h + rc(h)
    else:
        alphabet = b"AT"
        base = bytes(rng.choice(b"AT") for _ in range(L))
    sub, indel = rng.choice([(0.0, 0.0), (0.02, 0.01), (0.05, 0.03)])
    recs = []
    for i in range(rng.randint(2, 6)):
        b = mutate(base, sub, indel, rng, alphabet=alphabet, max_indel=rng.choice([1, 3, 17]))
        lo = rng.randint(0, len(b) // 4) if rng.random() < 0.3 else 0
        hi = len(b) - (rng.randint(0, len(b) // 4) if rng.random() < 0.3 else 0)
        sq = b[lo:hi] or b"A"
        if rng.random() < 0.4:
            sq = rc(sq)
        recs.append((f"r{i}", sq))
    return recs, rng.choice([0, 0, 1, 5, 20])


# ------------------------------------------------------------------------------------------ sets for single stages
def graph_cases():
    """small sets whose graphs hold what random sequence never gives: "loops" a self-loop L line (a homopolymer run
    collapses into one node that follows itself), "selfrc" an edge that is its own reverse complement (x + x -: the two
    middle bases of a palindrome, united with each other's reverse strand through a reverse-strand alignment)"""
    pal = palindromes()
    return {
        "loops": ([("h8", b"A" * 8), ("h9", b"A" * 9), ("h17", b"A" * 17)] + microsatellites()[4:8], 0),
        "selfrc": ([m for m in pal if m[0] in ("pal", "near1", "near2", "near1b", "pal_mid")], 0),
        "micro_k8": (microsatellites()[:8] + [("at", b"AT" * 40)], 8),
    }


def tiny_cyclic_sets():
    """a few dozen bases each: graphs small enough for the pure-Python SGD restatement, with paths that visit one node
    many times"""
    return {
        "homopolymer": [("a", b"A" * 9), ("b", b"A" * 7)],
        "cag": [("a", b"CAG" * 6), ("b", b"CAG" * 8 + b"CA"), ("c", b"CAG" * 3 + b"CTG" + b"CAG" * 3)],
        "palindrome": [("p", b"ACGTTGCATGCAACGT"), ("q", b"ACGTTGCTTGCAACGT"), ("r", b"ACGTTGCAAGCAACGT")],
        "gt_flanks": [("a", b"ACCTGA" + b"GT" * 5 + b"CATTAG"), ("b", b"ACCTGA" + b"GT" * 8 + b"CATTAG")],
    }


def sketch_set(seed=71, with_long=False):
    """for -x tree: repeats whose sketches are tiny (a homopolymer has one distinct k-mer, N x L none, a sequence shorter
    than k none), three byte-identical members (exactly equal Jaccard fractions: the lower index must win) and mutated
    repeat members; with_long adds members of more than 1 000 distinct k-mers (the sketch cut) to the same walk"""
    rng = random.Random(seed)
    sat = satellite(seed + 1, copies=(3, 4))
    cag = b"CAG" * 60
    recs = [("cag_a", cag), ("homo", b"A" * 200), ("cag_b", cag), ("allN", b"N" * 150), ("short", b"ACGTACG"),
            ("cag_c", cag), ("cag_m", mutate(cag, 0.03, 0.01, rng)), ("gt", b"GT" * 90), ("gt_m", mutate(b"GT" * 90, 0.03, 0.0, rng)),
            ("at", b"AT" * 80), ("acgt", b"ACGT" * 40)] + sat + two_letter(seed + 2, 200)[:2]
    if with_long:
        u = unique(1600, seed + 3)
        recs += [("long_a", u), ("long_b", mutate(u, 0.03, 0.005, rng)), ("long_rep", u[:700] + b"CAG" * 100 + u[700:1400])]
    return recs


def iterative_family(seed=81, n=14):
    """n (>= 12) satellite arrays of 3 or 4 copies of one 60-bp unit, every copy diverged by 2 %, every fourth member
    reverse-complemented"""
    rng = random.Random(seed)
    unit = unique(60, seed + 1)
    out = []
    for i in range(n):
        s = satellite_array(unit, 3 + i % 2, 0.02, rng)
        out.append((f"it{i}", rc(s) if i % 4 == 3 else s))
    return out
