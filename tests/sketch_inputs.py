"""Plain reference and inputs for the stages of `-x tree:` pair selection (sr_sketch.hip: k-mer hashes, bottom-1000
sketches, all-pairs Jaccard, k-nearest / k-farthest selection) -- tests/test_sketch_host.py and tests/test_sketch_gpu.py.

The reference restates the written rule of the sr_sketch.hip header comment with Python ints, set, sorted and
fractions.Fraction only.  It shares no code and no formulation with the kernels or with oracle/seqrush.c: the two codes of a
window come from two separate loops, a sketch is sorted(set(...))[:1000], the Jaccard terms are set operations (no merge
walk), the selection is one sort by exact fractions (no repeated passes).

The inputs are built for the places where the kernels can go wrong: sr_sketch_sort_kernel scans the sorted, padded hash
array in chunks of 1024 and carries a count from chunk to chunk; the cut is at 1000 distinct values; sr_jaccard_kernel has
a grid-stride loop that only n >= 2049 members reach; sr_knn_select_kernel runs 64 rows per block.  Every generator is
deterministic; where a property depends on the draw (an equal pair on a chunk boundary) the generator walks seeds until the
reference shows the property, and test_sketch_host.py asserts it."""
import functools
import random
from fractions import Fraction

M64 = (1 << 64) - 1
SENTINEL = M64                      # the value the definition drops, and the fill value of unused sketch entries
SKETCH = 1000
CHUNK = 1024                        # elements per scan step of sr_sketch_sort_kernel
GOLDEN = 0x9E3779B97F4A7C15
CODE = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3, ord("a"): 0, ord("c"): 1, ord("g"): 2, ord("t"): 3}
COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


# ------------------------------------------------------------------------------------------ the reference
def splitmix64(x):
    x = (x + GOLDEN) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def revcomp(s: bytes) -> bytes:
    """reverse complement that keeps case and leaves every other byte as it is"""
    return s.translate(COMP)[::-1]


def window_hash(w: bytes):
    """hash of one window, None when a byte is outside ACGTacgt or the hash is the dropped value"""
    k = len(w)
    if any(b not in CODE for b in w):
        return None
    fwd = 0
    for b in w:                                   # forward strand, first base most significant
        fwd = fwd * 4 + CODE[b]
    rev = 0
    for b in reversed(w):                         # the other strand read 5' -> 3': complement of the last base first
        rev = rev * 4 + (3 - CODE[b])
    h = splitmix64(min(fwd, rev) ^ ((k * GOLDEN) & M64))
    return None if h == SENTINEL else h


@functools.lru_cache(maxsize=None)
def kmer_hashes(s: bytes, k: int):
    """the hashes of the valid windows of s in window order (duplicates kept)"""
    out = []
    for i in range(len(s) - k + 1):
        h = window_hash(s[i:i + k])
        if h is not None:
            out.append(h)
    return tuple(out)


def sketch(s: bytes, k: int):
    return sorted(set(kmer_hashes(s, k)))[:SKETCH]


def jaccard(A, B):
    """(shared, denom) of two sketches"""
    A, B = set(A), set(B)
    U = sorted(A | B)[:SKETCH]
    return len(set(U) & A & B), max(1, len(U))


def matrices(seqs, k):
    """sketches, then the n x n shared / denom matrices as lists of lists (diagonal 0)"""
    sk = [sketch(s, k) for s in seqs]
    n = len(seqs)
    sh = [[0] * n for _ in range(n)]
    dn = [[0] * n for _ in range(n)]
    for i in range(n):
        for j in range(i + 1, n):
            sh[i][j], dn[i][j] = jaccard(sk[i], sk[j])
            sh[j][i], dn[j][i] = sh[i][j], dn[i][j]
    return sk, sh, dn


def selection(shared, denom, kn, kf):
    """sel[i][j]: bit 0 = j is one of i's kn nearest others, bit 1 = one of its kf farthest; equal fractions: lower index"""
    n = len(shared)
    sel = [[0] * n for _ in range(n)]
    for i in range(n):
        others = [j for j in range(n) if j != i]
        frac = {j: Fraction(shared[i][j], denom[i][j]) for j in others}
        for j in sorted(others, key=lambda j: (-frac[j], j))[:kn]:
            sel[i][j] |= 1
        for j in sorted(others, key=lambda j: (frac[j], j))[:kf]:
            sel[i][j] |= 2
    return sel


def unit(h):
    return (h >> 11) / 9007199254740992             # exact: a 53-bit integer over 2^53


def pair_list(n, sel, seed, rf, exclude_self=False):
    """ordered (query, target) list, row-major: self pairs unless exclude_self; an unordered pair {i < j} is kept when either
    end selected the other or unit(splitmix64(seed ^ (i*n+j))) < rf, and then both directions are listed"""
    out = []
    for q in range(n):
        for t in range(n):
            if q == t:
                if not exclude_self:
                    out.append((q, t))
                continue
            i, j = min(q, t), max(q, t)
            if (sel is not None and (sel[i][j] or sel[j][i])) or unit(splitmix64((seed ^ (i * n + j)) & M64)) < rf:
                out.append((q, t))
    return out


def parse_spec(spec):
    """tree:kn[,kf[,rf[,kmer]]] -> (kn, kf, rf, kmer); kf 0, rf 0.0 and kmer 16 when left out"""
    assert spec.startswith("tree:")
    p = spec[5:].split(",")
    return int(p[0]), int(p[1]) if len(p) > 1 else 0, float(p[2]) if len(p) > 2 else 0.0, int(p[3]) if len(p) > 3 else 16


@functools.lru_cache(maxsize=None)
def _matrices_cached(seqs, k):
    return matrices(list(seqs), k)


def reference(recs, k):
    """(sketches, shared, denom) of a record list, computed once per (records, k)"""
    return _matrices_cached(tuple(s for _, s in recs), k)


def sel_of_spec(recs, spec):
    kn, kf, _, k = parse_spec(spec)
    if len(recs) < 2:
        return None
    _, sh, dn = reference(recs, k)
    return selection(sh, dn, kn, kf)


def tree_pairs(recs, spec, seed=42, exclude_self=False):
    return pair_list(len(recs), sel_of_spec(recs, spec), seed, parse_spec(spec)[2], exclude_self)


# ------------------------------------------------------------------------------------------ what the sort kernel sees
def padded(length):
    """the padded length N of a member: the smallest power of two >= length, at least 2"""
    n = 2
    while n < length:
        n <<= 1
    return n


def sorted_padded(s: bytes, k: int):
    """the array sr_sketch_sort_kernel scans: one value per index below N (a window's hash, or the sentinel where there is no
    valid window), ascending"""
    vals = []
    for i in range(padded(len(s))):
        h = window_hash(s[i:i + k]) if i + k <= len(s) else None
        vals.append(SENTINEL if h is None else h)
    return sorted(vals)


def distinct_before(a, end):
    """distinct non-sentinel values among a[:end]"""
    return len(set(v for v in a[:end] if v != SENTINEL))


# ------------------------------------------------------------------------------------------ inputs
def rnd(length, seed, alphabet=b"ACGT"):
    r = random.Random(seed)
    return bytes(r.choice(alphabet) for _ in range(length))


def mutate(s, every, seed):
    """substitute about one base in `every`"""
    r = random.Random(seed)
    out = bytearray(s)
    for i in range(len(out)):
        if r.randrange(every) == 0:
            out[i] = r.choice([c for c in b"ACGT" if c != out[i]])
    return bytes(out)


def _first_seed(base, make, ok):
    for seed in range(base, base + 200):
        s = make(seed)
        if ok(s):
            return s
    raise AssertionError("no seed below base + 200 has the property")


@functools.lru_cache(maxsize=None)
def cut_set():
    """k = 16.  Random members whose windows are all distinct: 999, 1000 and 1001 distinct hashes (one below, at and one
    above the cut); lengths 1024 and 1025, where the padded length jumps from 1024 to 2048 while the cut is reached in the
    first chunk"""
    def all_distinct(s):
        return len(set(kmer_hashes(s, 16))) == len(s) - 15
    return [(f"r{L}", _first_seed(1000 + L, lambda seed, L=L: rnd(L, seed), all_distinct)) for L in (1014, 1015, 1016, 1024, 1025)]


def _periodic(period, length, k, base):
    """a repeat of one random unit with exactly `period` distinct hashes at k"""
    def make(seed):
        u = rnd(period, seed)
        return (u * (length // period + 1))[:length]
    return _first_seed(base, make, lambda s: len(set(kmer_hashes(s, k))) == period)


@functools.lru_cache(maxsize=None)
def chunk_set():
    """duplicates, runs and the cut against the 1024-element scan chunks, and the shortest members.
    xx800 (k = 16): X + X, 800 distinct in N = 2048, with an equal pair on a[1023], a[1024];
    xx1500 (k = 16): X + X, 1500 distinct in N = 4096, the cut at 1000 inside the second chunk;
    p7 / p5 (k = 4): period-7 / period-5 repeats with 7 / 5 distinct hashes whose runs cross index 1024 and 2048;
    homo: one distinct hash;  len1..len3: N = 2, 2, 4 beside a stride of 4096"""
    def straddles(s):
        a = sorted_padded(s, 16)
        return a[CHUNK - 1] == a[CHUNK] != SENTINEL and len(set(kmer_hashes(s, 16))) == 800
    xx800 = _first_seed(2000, lambda seed: rnd(800, seed) * 2, straddles)
    xx1500 = _first_seed(2100, lambda seed: rnd(1500, seed) * 2, lambda s: len(set(kmer_hashes(s, 16))) == 1500)
    return [("len3", b"ACG"), ("xx800", xx800), ("xx1500", xx1500), ("p7", _periodic(7, 3000, 4, 2200)),
            ("p5", _periodic(5, 2500, 4, 2300)), ("homo", b"A" * 1500), ("len1", b"C"), ("len2", b"GT")]


@functools.lru_cache(maxsize=None)
def kmer_set(k):
    """for one k-mer size: a random member, its reverse complement, its lower case, a mutated copy, an unrelated member, and
    members of k-1, k and k+1 bases (none, one and two windows)"""
    a = rnd(200, 3000 + k)
    recs = [("a", a), ("a_rc", revcomp(a)), ("a_lower", a.lower()), ("a_mut", mutate(a, 25, 3100 + k)), ("b", rnd(200, 3200 + k))]
    for d in (-1, 0, 1):
        if k + d > 0:
            recs.append((f"len_k{d:+d}", rnd(k + d, 3300 + k + d)))
    return recs


KMER_SIZES = (1, 2, 15, 16, 31, 32)


@functools.lru_cache(maxsize=None)
def alphabet_set():
    """one random member in other spellings: lower and mixed case (valid, equal to upper case); N, IUPAC letters, 'U' and
    bytes >= 0x80 (0xC1 is 'A' with the top bit set) in place of bases; an invalid byte that is only ever the first byte of
    a window (position 0) and one that is only ever the last (the final position); a member of N only"""
    b = rnd(120, 4000)

    def put(pos_bytes):
        out = bytearray(b)
        for p, c in pos_bytes:
            out[p] = c
        return bytes(out)
    mixed = bytes(c if i % 2 else c + 32 for i, c in enumerate(b))
    return [("upper", b), ("lower", b.lower()), ("mixed", mixed), ("n_mid", put([(40, ord("N")), (41, ord("n"))])),
            ("iupac", put([(10, ord("R")), (30, ord("Y")), (50, ord("K")), (70, ord("M")), (90, ord("S")), (110, ord("W"))])),
            ("u", put([(25, ord("U")), (75, ord("u"))])), ("hi", put([(20, 0x80), (60, 0xFF), (100, 0xC1)])),
            ("bad_first", put([(0, ord("N"))])), ("bad_last", put([(119, 0xE7)])), ("all_n", b"N" * 50)]


@functools.lru_cache(maxsize=None)
def jaccard_set():
    """k = 16: two members without a sketch (N only; shorter than k), identical members, disjoint members, two members of
    more than 1000 distinct hashes each that share most of them, and a member beside its reverse complement"""
    x = rnd(300, 5000)
    long_a = rnd(1600, 5100)
    return [("all_n", b"N" * 40), ("short", b"ACGTACG"), ("x", x), ("x_same", x), ("y", rnd(300, 5001)), ("x_rc", revcomp(x)),
            ("long_a", long_a), ("long_b", mutate(long_a, 60, 5101)), ("x_mut", mutate(x, 40, 5002))]


@functools.lru_cache(maxsize=None)
def family130():
    """130 members (three blocks of sr_knn_select_kernel's 64 rows): diverged copies of one 150-base sequence, every fifth
    reverse-complemented, every seventh byte-identical to the first (equal fractions: the lower index wins)"""
    base = rnd(150, 6000)
    out = []
    for i in range(130):
        s = base if i % 7 == 0 else mutate(base, 12 + i % 9, 6001 + i)
        out.append((f"f{i}", revcomp(s) if i % 5 == 4 else s))
    return out


@functools.lru_cache(maxsize=None)
def big_set():
    """2049 members of 12 bases: n * n > 16384 * 256, the first run of sr_jaccard_kernel's grid-stride loop.  At k = 2 a
    sketch is a subset of the 10 canonical 2-mers (see big_masks)"""
    r = random.Random(7000)
    return [(f"s{i}", bytes(r.choice(b"ACGT") for _ in range(12))) for i in range(2049)]


def big_masks(recs, k=2):
    """every member's sketch as a bit mask over the distinct hashes of the whole set (at most 10 at k = 2): shared and denom
    of two members are the popcounts of the AND and the OR of their masks, exactly, because no union reaches 1000"""
    sk = [sketch(s, k) for _, s in recs]
    universe = sorted(set(h for row in sk for h in row))
    bit = {h: i for i, h in enumerate(universe)}
    return sk, universe, [sum(1 << bit[h] for h in row) for row in sk]


SMALL_SETS = {                       # name -> (records, k-mer sizes the stage tests run it at); all of at most 64 members
    "cut": (cut_set, (16,)),
    "chunks": (chunk_set, (4, 16)),
    "alphabet": (alphabet_set, (1, 5, 16, 32)),
    "jaccard": (jaccard_set, (16,)),
}
for _k in KMER_SIZES:
    SMALL_SETS[f"kmer{_k}"] = (functools.partial(kmer_set, _k), (_k,))

SPECS = ("tree:2,1,0.1,4", "tree:3,3,0.1", "tree:2,2,0.0,32", "tree:1,0,0,1")


# ------------------------------------------------------------------------------------------ synthetic selection matrices
SELECT_N = (1, 2, 63, 64, 65, 130)


def select_k(n):
    return [(0, 0), (1, 0), (0, 1), (3, 3), (n - 1, n - 1), (n + 5, n + 5)]


SELECT_VARIANTS = ("equal", "zero")


@functools.lru_cache(maxsize=None)
def select_matrix(n, variant):
    """symmetric shared <= denom <= 1000 (diagonal 0) as lists of lists, random with few distinct values, so that ties are
    common everywhere.  One row r (and, for symmetry, its column) is special -- "equal": one fraction written three ways
    (1/2, 2/4, 500/1000); "zero": nothing shared, over three different denominators.  -> (shared, denom, r); r is None
    where n < 3"""
    r = random.Random(8000 + n)
    sh = [[0] * n for _ in range(n)]
    dn = [[0] * n for _ in range(n)]
    for i in range(n):
        for j in range(i + 1, n):
            d = r.choice((1, 2, 3, 4, 6, 12, 999, 1000))
            s = r.randrange(d + 1)
            sh[i][j] = sh[j][i] = s
            dn[i][j] = dn[j][i] = d
    row = n // 3 if n >= 3 else None
    forms = {"equal": ((1, 2), (2, 4), (500, 1000)), "zero": ((0, 7), (0, 1000), (0, 1))}[variant]
    for j in range(n):
        if row is not None and j != row:
            sh[row][j], dn[row][j] = forms[j % 3]
            sh[j][row], dn[j][row] = forms[j % 3]
    return sh, dn, row
