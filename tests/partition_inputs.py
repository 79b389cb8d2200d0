"""Seeded partitions and CIGARs built by hand (plain helper module, no GPU use): what the stages behind the aligner --
the CIGAR walk of uf_unite_cigar, the lock-free union-find, the 64- and 32-bit label and merge kernels, the 13 kernels of
graph induction -- are given when no aligner chose the input.  Real alignments of small families only produce partitions
whose united bases are equal or complementary, a few thousand bases, canonical label arrays and CIGARs of a few dozen
operations; the constructors here put the sizes on the kernels' own boundaries (scan tiles of 1024, the second scan level at
256 tiles, the grid caps of the grid-stride loops, chunks of 256 CIGAR operations) and unite what no alignment would.

A partition case (`partition(family, N)`) is a dict:
    recs      [(name, bytes)] for SeqSet / OracleSeqRush: one sequence of a single base, then the other N-1 bases in two
              sequences, or in as many as keeps each at 32 768 bases or fewer (sr_ctx_load stages whole sequences in LDS and
              refuses longer ones at 8 bits per symbol).  N == 2: two of 1; sr_ctx_load accepts it, so 2 stays the smallest size
    arrays    label arrays of 2N+2 uint64 to merge: "element i is with arrays[j][i]", identity where nothing is said; NOT
              canonical in general (chains, labels on the other strand, labels larger than the element)
    unions    the same unions as an (m, 2) uint64 array of (pos_a, pos_b), pos = base_index << 1 | strand, for the references
              (the two strands of every base are united at load: SeqRush::new, src/seqrush.rs:324-328)
A CIGAR case (`cigar_case(name)`) is a dict of recs, paf (text), records (parsed, for the Python walk) and what the recipe
is named for.  Everything is a pure function of its arguments (numpy Generator / random.Random with fixed seeds)."""
import functools
import random

import numpy as np

import oracle_binding as ob

ACGT = b"ACGT"
COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
MIXED = b"ACGTacgtNnRYKMSWrykmsw"                     # both cases, N and IUPAC codes
U64 = np.uint64
MAX_SEQ = 32768

SMALL_SIZES = (2, 1023, 1024, 1025)                   # around one scan tile of 1024 (GI_TILE)
SCAN_SIZES = (262144, 262145)                         # 256 tiles / 257 tiles: gi_scan_sums takes a second round with a carry
CAP_SIZES = (524289, 2097153)                         # 2N+2 > 4096 * 256 (label kernels), N > 8192 * 256 (gi_grid)
FAMILIES = ("none", "letters", "star", "chain", "two_arrays", "skip", "palindrome", "mixed_alphabet", "random")
SCAN_FAMILIES = ("none", "chain", "random", "letters")
CAP_FAMILIES = ("random", "letters")
# the whole matrix; a family x size that is not here is not run, for the reason given:
#   star above 1025: it is there for contention on one root, and stays at N <= 4096 so that it never nears the retry bound
#   two_arrays, skip, palindrome, mixed_alphabet above 1025: their edge is in the merge rule / the letters, not in a size;
#     the size boundaries are covered by the four families that go there
MATRIX = ([(f, n) for f in FAMILIES for n in SMALL_SIZES] + [(f, n) for f in SCAN_FAMILIES for n in SCAN_SIZES] +
          [(f, n) for f in CAP_FAMILIES for n in CAP_SIZES])
HOST_MATRIX = [(f, n) for f, n in MATRIX if n <= SCAN_SIZES[-1]]
ORACLE_GFA_MAX = SCAN_SIZES[-1]                       # the oracle's induction is O(N): it is run on every size of HOST_MATRIX


def revcomp(s):
    return s.translate(COMP)[::-1]


def lengths(N):
    if N < 3:
        return [1] * N
    parts = max(2, -(-(N - 1) // MAX_SEQ))
    return [1] + [(N - 1) // parts + (i >= parts - (N - 1) % parts) for i in range(parts)]


def _split(bases, N):
    out, off = [], 0
    for i, L in enumerate(lengths(N)):
        out.append((f"p{i}", bytes(bases[off:off + L])))
        off += L
    return out


def _draw(rng, alphabet, N):
    return np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), N)]


def _ident(N):
    return np.arange(2 * N + 2, dtype=U64)


def _pairs(a, b):
    return np.stack([np.asarray(a, dtype=U64), np.asarray(b, dtype=U64)], axis=1).reshape(-1, 2)


def _upper(b):
    b = np.asarray(b, dtype=np.uint8)
    return np.where((b >= 97) & (b <= 122), b - 32, b).astype(np.uint8)


def _first_of(keys):
    """for every element the index of the first element with the same key"""
    _, first, inv = np.unique(keys, return_index=True, return_inverse=True)
    return first[inv].astype(U64)


def random_components(N, ncomp, rng):
    comp = rng.integers(0, max(1, ncomp), N)
    return _first_of(comp)


def _from_first(N, first, rng):
    """element (g, +) is with (first[g], random strand): one array, labels on either strand"""
    g = np.arange(N, dtype=U64)
    lab = _ident(N)
    tgt = (first << U64(1)) | rng.integers(0, 2, N).astype(U64)
    lab[::2][:N] = np.where(first == g, g << U64(1), tgt)
    sel = first != g
    return lab, _pairs(g[sel] << U64(1), tgt[sel])


def random_partition(N, ncomp, seed=0):
    """-> (one label array, its unions): N bases thrown into ncomp components, every base with the first of its component"""
    rng = np.random.default_rng([seed, N, ncomp])
    return _from_first(N, random_components(N, ncomp, rng), rng)


@functools.lru_cache(maxsize=4)
def partition(family, N, seed=0):
    rng = np.random.default_rng([seed, N, FAMILIES.index(family)])
    g = np.arange(N, dtype=U64)
    one = U64(1)
    if family == "letters":                           # runs of 1..20 equal letters in either case: homopolymer self-loops
        runs = rng.integers(1, 21, N)
        letters = np.repeat(_draw(rng, b"ACGTacgtN", N), runs)[:N]
        bases = letters.copy()
    elif family == "mixed_alphabet":
        bases = _draw(rng, MIXED, N)
    elif family == "palindrome":
        bases = bytearray()
        for L in lengths(N):                          # (one base in front if odd) + half + reverse complement of the half
            h = (ACGT * (L // 8 + 1))[:L // 2]
            bases += (b"A" if L & 1 else b"") + h + revcomp(h)
        bases = np.frombuffer(bytes(bases), dtype=np.uint8)
    else:
        bases = _draw(rng, ACGT, N)
    recs = _split(bases.tobytes(), N)
    arrays, unions = [_ident(N)], _pairs([], [])
    if family == "none":
        pass
    elif family == "letters":                         # (g, +) with (first base of the same upper-cased letter, -)
        first = _first_of(_upper(bases))
        lab = _ident(N)
        lab[::2][:N] = np.where(first == g, g << one, (first << one) | one)
        arrays, unions = [lab], _pairs((g << one)[first != g], ((first << one) | one)[first != g])
    elif family == "star":                            # every Pos with Pos 0, whatever its letter
        lab = _ident(N)
        lab[:2 * N] = 0
        arrays, unions = [lab], _pairs(np.arange(1, 2 * N, dtype=U64), np.zeros(2 * N - 1, dtype=U64))
    elif family == "chain":                           # (i, +) with (i + 1, +): labels larger than the element
        lab = _ident(N)
        lab[::2][:N - 1] = (g[:-1] + one) << one
        arrays, unions = [lab], _pairs(g[:-1] << one, (g[:-1] + one) << one)
    elif family == "two_arrays":                      # base 2i with 2i+1 in one array, 2i+1 with 2i+2 in the other
        a1, a2 = _ident(N), _ident(N)
        ev, od = g[0:N - 1:2], g[1:N - 1:2]
        a1[ev << one] = (ev + one) << one
        a2[od << one] = (od + one) << one
        arrays = [a1, a2]
        unions = np.concatenate([_pairs(ev << one, (ev + one) << one), _pairs(od << one, (od + one) << one)])
    elif family in ("random", "mixed_alphabet", "skip"):
        ncomp = {"random": 256 if N > 4096 else max(1, N // 8), "mixed_alphabet": max(1, N // 6), "skip": max(1, N // 5)}[family]
        lab, unions = _from_first(N, random_components(N, ncomp, rng), rng)
        if family == "skip":                          # every 3rd entry says n, n + 1 or 2^64 - 1: to be ignored
            n = 2 * N + 2
            idx = np.arange(0, 2 * N, 3)
            lab[idx] = np.array([n, n + 1, 2 ** 64 - 1], dtype=U64)[np.arange(len(idx)) % 3]
            keep = unions[:, 0] % U64(3) != 0
            unions = unions[keep]
        arrays = [lab]
    elif family == "palindrome":
        lab = _ident(N)
        ua, ub, off, halves = [], [], 0, []
        for L in lengths(N):
            i = np.arange(L // 2, dtype=U64)
            a, b = (U64(off + (L & 1)) + i) << one, ((U64(off + L - 1) - i) << one) | one   # mirror bases, other strand
            lab[a] = b
            ua.append(a); ub.append(b); halves.append((off + (L & 1), L // 2))
            off += L
        if len(halves) == 3:                          # the two long members share their first halves: the same nodes, walked
            (o1, h1), (o2, h2) = halves[1], halves[2]  # forward by one path and reverse-complemented by the other
            i = np.arange(min(h1, h2), dtype=U64)
            a, b = ((U64(o2) + i) << one) | one, ((U64(o1) + i) << one) | one
            lab[a] = b
            ua.append(a); ub.append(b)
        arrays, unions = [lab], _pairs(np.concatenate(ua), np.concatenate(ub))
    else:
        raise KeyError(family)
    for a in arrays:
        a.setflags(write=False)
    unions.setflags(write=False)
    return dict(family=family, N=N, recs=recs, arrays=arrays, unions=unions, bases=bases)


def as_u32(arrays):
    """the 32-bit form of the exchange: 2^64 - 1 becomes 0xffffffff, everything else fits while 2N+2 < 2^32"""
    return [a.astype(np.uint32) for a in arrays]


def oracle_unite(recs, unions, o=None):
    """the unions through the oracle's own union-find (sro_buf_unite on OracleSeqRush.uf) -> the OracleSeqRush"""
    o = o or ob.OracleSeqRush(records=recs)
    L, uf = o.L, o.uf
    for a, b in np.asarray(unions).tolist():
        L.sro_buf_unite(uf, a, b)
    return o


def self_reverse_edges(gfa_text):
    """L lines that are their own reverse complement (k1 == k2 in gi_edge_insert): x+ -> x- or x- -> x+"""
    n = 0
    for ln in gfa_text.split("\n"):
        f = ln.split("\t")
        n += len(f) >= 5 and f[0] == "L" and f[1] == f[3] and f[2] != f[4]
    return n


# ------------------------------------------------------------------------------------------ PAF replay on the oracle
def oracle_paf_replay(recs, paf_text, k=0, o=None, labels=True):
    """align_and_unite_from_paf (src/seqrush.rs:510-609) on the oracle: same record rules"""
    o = o or ob.OracleSeqRush(records=recs)
    idx = {}
    for i, (name, _) in enumerate(recs):
        idx[name] = i                                   # HashMap collect: a later duplicate wins
    for ln in paf_text.split("\n"):
        if ln == "":
            continue
        f = ln.split("\t")
        if len(f) < 12:
            continue
        cg = ""
        for x in f[12:]:
            if x.startswith("cg:Z:"):
                cg = x[5:]
                break
        if f[0] not in idx or f[5] not in idx:
            continue
        assert o.process_alignment(cg, idx[f[0]], idx[f[5]], k, f[4] == "-", int(f[2]), int(f[3]),
                                   int(f[7]), int(f[8])) >= 0
    return o.canonical_labels() if labels else o


# ------------------------------------------------------------------------------------------ CIGAR recipes
QFLANK, TFLANK = (3, 5), (7, 2)                       # flanks of the variants with nonzero starts
VARIANTS = (("+", False), ("-", False), ("+", True), ("-", True))       # (strand, nonzero starts)
CIGAR_K = (0, 8, 15)


def _other(rng, ch):
    return rng.choice([c for c in ACGT if c != ch])


def _fit(ops, rng, lie=()):
    """(query, target) that fit the PAF ops [(letter, len)]: '=' copies, 'X' differs at every base, 'I' is query only, 'D'
    target only, 'M' copies with every 7th base substituted; an op whose index is in `lie` says '=' over bases of which every
    5th differs"""
    q, t = bytearray(), bytearray()
    for i, (op, n) in enumerate(ops):
        seg = bytes(rng.choice(ACGT) for _ in range(n))
        if op == "=" and i not in lie:
            q += seg; t += seg
        elif op == "X":
            q += bytes(_other(rng, c) for c in seg); t += seg
        elif op == "I":
            q += seg
        elif op == "D":
            t += seg
        else:
            step = 5 if op == "=" else 7
            q += bytes(_other(rng, c) if j % step == step - 1 else c for j, c in enumerate(seg)); t += seg
    return bytes(q), bytes(t)


def alternating(n, other):
    """n operations, 1= and 1<other> in turn"""
    return [("=", 1) if i % 2 == 0 else (other, 1) for i in range(n)]


def hole600():
    """600 operations; those of the middle chunk of 256 (indices 256..511) unite nothing"""
    ops = [("=", 2) if i % 2 == 0 else ("X", 1) for i in range(256)]
    ops += [("IDX"[i % 3], 1 + i % 2) for i in range(256)]
    ops += [("=", 2) if i % 2 == 0 else ("X", 1) for i in range(88)]
    return ops


def runs_at(k, p):
    """match runs of k-1, k and k+1 bases as operations p, p+2 and p+4 (k == 1: k and k+1 at p and p+2), single-base matches
    before and behind, separated by X, I and D in turn so that the query and the target carries differ"""
    want = [r for r in (k - 1, k, k + 1) if r > 0]
    at = {p + 2 * j: r for j, r in enumerate(want)}
    ops = []
    for i in range(p + 2 * len(want) + 6):
        if (i - p) % 2 == 0:
            ops.append(("=", at.get(i, 1)))
        else:
            ops.append(("XID"[i % 3], 1))
    return ops, at


def _recipes():
    out = {"one": dict(ops=[("=", 1)])}
    for other in "XDI":
        for n in (255, 256, 257, 513):
            out[f"alt{other}{n}"] = dict(ops=alternating(n, other), count=n)
    out["hole600"] = dict(ops=hole600(), count=600, empty_chunk=1)
    out["long70000"] = dict(ops=[("=", 70000)], count=1)
    for k in (1, 8, 15):
        for p in (255, 256, 257):
            ops, at = runs_at(k, p)
            out[f"runs{k}at{p}"] = dict(ops=ops, runs_at=at, count=len(ops))
    out["m_only"] = dict(ops=[("M", 300)])            # M over bytes with mismatches: the host compares the bases
    out["claim"] = dict(ops=[("=", 40), ("X", 1), ("=", 300)], lie=(2,))   # '=' over unequal bytes
    out["self"] = dict(ops=[("=", 500)], self_record=True)
    return out


RECIPES = _recipes()
CIGAR_NAMES = tuple(RECIPES)


@functools.lru_cache(maxsize=None)
def cigar_case(name):
    """-> dict(recs, paf, records, ...): the recipe as four records over four disjoint pairs of sequences (strand + / -,
    zero / nonzero starts), one single-base sequence first.  A record is (q index, t index, strand, qs, ts, ops).
    The self record (query == target, identity) is one record: on strand '-' it would need a reverse palindrome, which is
    the palindrome partition's subject."""
    spec = RECIPES[name]
    rng = random.Random(f"cigar:{name}")
    ops = spec["ops"]
    cg = "".join(f"{n}{op}" for op, n in ops)
    recs, lines, records = [("one", b"G")], [], []
    if spec.get("self_record"):
        q, _ = _fit(ops, rng)
        recs.append(("s", q))
        lines.append(f"s\t{len(q)}\t0\t{len(q)}\t+\ts\t{len(q)}\t0\t{len(q)}\t{len(q)}\t{len(q)}\t60\tcg:Z:{cg}")
        records.append((1, 1, "+", 0, 0, ops))
    else:
        for v, (strand, starts) in enumerate(VARIANTS):
            q, t = _fit(ops, rng, spec.get("lie", ()))
            ql, qr, tl, tr = [bytes(rng.choice(ACGT) for _ in range(m)) for m in ((QFLANK + TFLANK) if starts else (0,) * 4)]
            qs, ts, qe, te = len(ql), len(tl), len(ql) + len(q), len(tl) + len(t)
            q, t = ql + q + qr, tl + t + tr
            if strand == "-":                         # PAF coordinates of a '-' record are in reverse-complement space
                q = revcomp(q)
            qi = len(recs)
            recs += [(f"q{v}", q), (f"t{v}", t)]
            lines.append(f"q{v}\t{len(q)}\t{qs}\t{qe}\t{strand}\tt{v}\t{len(t)}\t{ts}\t{te}\t0\t0\t60\tcg:Z:{cg}")
            records.append((qi, qi + 1, strand, qs, ts, ops))
    return dict(spec, name=name, recs=recs, paf="\n".join(lines) + "\n", records=records)
