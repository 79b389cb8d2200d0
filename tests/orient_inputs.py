"""Inputs and reference of the orientation tests (plain helper module: no device, no oracle, no code of the library).

The orientation stage scores a pair forward (F) and with the query reverse-complemented (R) under the one-piece
orientation penalties and picks the reverse strand iff R < F.  Here:

  ref_score   the global gap-affine distance by the plain O(nm) recurrence (three states, 64-bit integers, bytes compared
              raw, a gap of length L costs o + e L); expect() = (F, R) of an ordered pair, computed once per process
  lb, ub      the two bounds of sr_orient_blk_kernel's shortcuts restated: the 8-mer lower bound of R and the diagonal-0
              upper bound of F.  The shortcuts are exact only while lb <= R and ub >= F
  the cases   a lattice CHOSEN BY THE REFERENCE: p = s + rc(s) is its own reverse complement; substitution units in its
              first half move F and R apart by known amounts,
                 C (F+1, R+1)  the query gets another letter at i
                 X (F+2, R+1)  the query gets a at i, the target at the mirror position n-1-i a letter that is neither
                               the original nor the complement of a
                 Y (F+1, R+2)  query and target get two different new letters at i
              so u X-units, v Y-units and c C-units give F = 2u + v + c, R = u + 2v + c: any score, one apart or equal.
              At spacing 9 every unit spoils eight 8-mers of its own: on the block lattice lb = R and ub = F, the
              shortcut sits on its threshold (the wide cases, with 70 and more units, measure lb three or four below R).
              At spacing 3 the units share 8-mers: lb far below R, the reverse aligner starts early.
              Cutting the query's tail adds one gap to both scores and moves the end diagonal.

The case lists are data: names, sequences and the (F, R) they are built to have under 0,1,1,1 (test_orient_host.py holds
every one against ref_score).  blk_geometry restates the window arithmetic of the blocked orientation kernels (sr_orient.hip
sr_orient_blk_kernel, sr_blk_orient.inc ori_pass8: the same numbers) so that the cases can say -- and the host test can
assert -- which tile, lane and cell the end diagonal falls on."""
import functools
import random
from collections import namedtuple

import numpy as np

from seqrush_amd import synth

rc = synth.reverse_complement
ACGT = b"ACGT"
INT32_MAX = 2 ** 31 - 1
DEFAULT_ORI = "0,1,1,1"
OTHER_ORI = ("0,2,3,1", "0,1,2,2", "0,1,76,1")


# ------------------------------------------------------------------------------------------ the reference
def parse_ori(scores):
    """'0,x,o,e' -> (x, o, e)"""
    v = [int(t) for t in scores.split(",")]
    assert len(v) == 4 and v[0] == 0, scores
    return v[1], v[2], v[3]


def ref_score(q: bytes, t: bytes, x: int, o: int, e: int) -> int:
    """global one-piece gap-affine distance of q and t: mismatch x, a gap of length L costs o + e L.  Gotoh's recurrence
    row by row: V = best cell above + gap down the query, D = diagonal step, H = gap along the target (a running
    minimum over the row: a gap opened at column k and extended to j costs o + e (j - k)), cell = min of the three"""
    a = np.frombuffer(bytes(q), dtype=np.uint8)
    b = np.frombuffer(bytes(t), dtype=np.uint8)
    n, m = len(a), len(b)
    big = np.int64(1) << 40
    j = np.arange(m + 1, dtype=np.int64)
    best = o + e * j
    best[0] = 0
    vert = np.full(m + 1, big, dtype=np.int64)
    ej = e * j
    for i in range(1, n + 1):
        vert = np.minimum(best + (o + e), vert + e)
        cur = np.empty(m + 1, dtype=np.int64)
        cur[0] = o + e * i
        cur[1:] = best[:-1] + np.where(b == a[i - 1], 0, x)
        cur[1:] = np.minimum(cur[1:], vert[1:])
        # horizontal gaps: H[j] = min over k < j of cur[k] + o + e (j - k)
        run = np.minimum.accumulate(cur - ej)
        hor = np.full(m + 1, big, dtype=np.int64)
        hor[1:] = run[:-1] + o + ej[1:]
        best = np.minimum(cur, hor)
    return int(best[m])


@functools.lru_cache(maxsize=None)
def expect(q: bytes, t: bytes, ori: str = DEFAULT_ORI):
    """(F, R): forward and reverse-complement score of the ordered pair under the orientation penalties"""
    x, o, e = parse_ori(ori)
    return ref_score(q, t, x, o, e), ref_score(rc(q), t, x, o, e)


def lb(q: bytes, t: bytes) -> int:
    """8-mer lower bound of R: positions of the reverse-complemented query whose 8-mer does not occur in the target, over 8
    (one edit spoils at most eight of them), rounded up; no bound for a query shorter than an 8-mer"""
    if len(q) < 8:
        return 0
    r = rc(q)
    have = {t[i:i + 8] for i in range(len(t) - 7)}
    npos = len(q) - 7
    hits = sum(1 for i in range(npos) if r[i:i + 8] in have)
    return (npos - hits + 7) // 8


def ub(q: bytes, t: bytes) -> int:
    """upper bound of F: the alignment along diagonal 0, closed by one gap over the length difference"""
    n = min(len(q), len(t))
    ham = sum(1 for i in range(n) if q[i] != t[i])
    d = abs(len(q) - len(t))
    return ham + (1 + d if d else 0)


def shortcut(q: bytes, t: bytes) -> bool:
    """the pair is decided forward by the bounds alone (2-bit symbols, 0,1,1,1, the orientation kernel with its 8-mer sets)"""
    b = lb(q, t)
    return b > 0 and ub(q, t) < b


# ------------------------------------------------------------------------------------------ window arithmetic restated
OB = 8                       # levels per block of both blocked orientation kernels
OWNED = 60                   # lanes of a wave tile that own four diagonals each (two halo lanes per side)

Geometry = namedtuple("Geometry", "s0 nt tile lane cell last_group")


def blk_geometry(plen, tlen, score):
    """the block that holds level `score` under 0,1,1,1 (reach of level s: s - 1 from level 2 on): number of wave tiles
    of its window, and tile / lane / cell (0..3) that own the end diagonal tlen - plen; last_group: the end diagonal's
    group of four is the last one of the window"""
    s0 = score // OB * OB
    last = s0 + OB - 1
    reach = last - 1 if last >= 2 else 0
    shift = plen + 24
    wlo, whi = max(-plen - 1, -reach - OB - 2), min(tlen + 1, reach + OB + 2)
    glo, ghi = (wlo + shift) >> 2, (whi + shift) >> 2
    nt = (ghi - glo + OWNED) // OWNED
    g = (tlen - plen + shift) >> 2
    return Geometry(s0, nt, (g - glo) // OWNED, (g - glo) % OWNED + 2, (tlen - plen + shift) & 3, g == ghi)


# ------------------------------------------------------------------------------------------ the construction
Case = namedtuple("Case", "name group q t want")       # want = (F, R) under 0,1,1,1 the case is built to have, or None


def unique(L, seed):
    return synth.to_bytes(synth.base_sequence(L, seed))


def _other(rng, ch, avoid=()):
    return rng.choice([c for c in ACGT if c != ch and c not in avoid])


def palindrome(half, seed):
    s = unique(half, seed)
    return s + rc(s)


def plant(p, kinds, spacing, seed):
    """(query, target) from the palindrome p: the k-th unit, of kind kinds[k] in 'CXY', at position 5 + spacing k"""
    rng = random.Random(seed)
    n = len(p)
    assert 5 + spacing * len(kinds) + 4 <= n // 2, "the first half is too short for these units"
    q, t = bytearray(p), bytearray(p)
    for k, kind in enumerate(kinds):
        i = 5 + spacing * k
        a = _other(rng, p[i])
        q[i] = a
        if kind == "X":
            t[n - 1 - i] = _other(rng, p[n - 1 - i], avoid=(rc(bytes([a]))[0],))
        elif kind == "Y":
            t[i] = _other(rng, p[i], avoid=(a,))
        else:
            assert kind == "C"
    return bytes(q), bytes(t)


def composition(F, diff, k=None):
    """(u, v, c): X-, Y- and C-units with 2u + v + c = F and (u + 2v + c) - F = diff; k pairs of X and Y"""
    k = max(1, F // 6) if k is None else k
    u, v = (k, k) if diff == 0 else (k, k + 1) if diff > 0 else (k + 1, k)
    c = F - 2 * u - v
    assert c >= 0 and abs(diff) <= 1
    return u, v, c


def interleave(u, v, c, order="XCY"):
    """unit kinds in round-robin order, so that every kind occurs along the whole half"""
    left = {"X": u, "Y": v, "C": c}
    out = []
    while any(left.values()):
        for kind in order:
            if left[kind]:
                out.append(kind); left[kind] -= 1
    return "".join(out)


def cell(F, diff, spacing, half, seed, k=None, order="XCY"):
    u, v, c = composition(F, diff, k)
    return plant(palindrome(half, seed), interleave(u, v, c, order), spacing, seed + 1)


DIFFS = (-1, 0, 1)
DIFF_ID = {-1: "r-1", 0: "tie", 1: "r+1"}

# ---- block lattice: scores either side of the block boundaries 7|8, 15|16, 23|24 (and inside the first two blocks)
LATTICE_F = (6, 7, 8, 9, 15, 16, 17, 23, 24, 25)
LATTICE_HALF = 200                                      # >= 9 units + 10 for the 21 units of F = 25


def block_lattice():
    out = []
    for spacing in (9, 3):
        for F in LATTICE_F:
            for d in DIFFS:
                q, t = cell(F, d, spacing, LATTICE_HALF, 4100 + 10 * F + d)
                out.append(Case(f"lat-s{spacing}-F{F}-{DIFF_ID[d]}", "lattice", q, t, (F, F + d)))
    return out


# ---- length seam: the query's tail cut by 1..5 (one gap more on both strands: + 1 + cut), query length in every residue
# mod 4 and, in the other pair order, the target's: the end diagonal on each of a lane's four cells
SEAM_HALF = {-1: 140, 0: 141, 1: 140}


def length_seam():
    out = []
    for F in (8, 16):
        for d in DIFFS:
            for cut in (1, 2, 3, 4, 5):
                q, t = cell(F, d, 9, SEAM_HALF[d], 5200 + 10 * F + d, order="CYX")
                q = q[:len(q) - cut]
                out.append(Case(f"seam-F{F}-{DIFF_ID[d]}-cut{cut}", "seam", q, t, (F + 1 + cut, F + d + 1 + cut)))
    return out


# ---- wide: a tile owns 60 x 4 = 240 diagonals; the window of the block s0 .. s0+7 is the last level's reach s0 + 6 plus
# OB + 2 = 10 on each side, [-(s0 + 16), s0 + 16] while the sequences do not clip it: ghi - glo = (2 s0 + 32) >> 2 reaches 60,
# i.e. nt = 2, at s0 = 104: levels 104 .. 111 are the first whose block needs a second tile (blk_geometry(1400, 1400, 104).nt
# == 2, (.., 103).nt == 1; test_orient_host.py asserts both).  F = 105 is the smallest forward score whose three cells (R =
# 104, 105, 106) are all decided in that block.  There the second tile owns diagonals from 117 up, beyond the reach of 110:
# NULL cells only.  From s0 = 112 on it owns diagonals inside the reach (109 .. 112 up against 118), hence the cells at
# F = 113 as well.  The level-by-level kernels' window is narrower (reach + scope + 1 on each side): they are past one tile
# from level 119 on, which the tail-cut cases reach.
WIDE_F = (105, 113)
WIDE_HALF = 700                                         # 76 units at spacing 9
WIDE_K = {105: 34, 113: 37}
# tail cuts of the F = 105 tie cell that put the end diagonal, in the block of the final score, on the last owned lane of
# the first tile, on the first owned lane of the second tile (the lanes next to the tiles' halo lanes) and inside the second
# tile; in the other pair order the end diagonal is negative and stays in the first tile
WIDE_CUTS = (59, 61, 130)


def wide():
    out = []
    for F in WIDE_F:
        for d in DIFFS:
            q, t = cell(F, d, 9, WIDE_HALF, 6100 + 10 * F + d, k=WIDE_K[F])
            out.append(Case(f"wide-F{F}-{DIFF_ID[d]}", "wide", q, t, (F, F + d)))
    for cut in WIDE_CUTS:
        q, t = cell(105, 0, 9, WIDE_HALF, 7150, k=WIDE_K[105])
        out.append(Case(f"wide-kend{cut}", "wide", q[:len(q) - cut], t, None))
    return out


# ---- bound threshold: the spacing-9 lattice cells ARE the threshold (lb = R, ub = F): named here for the accounting test;
# plus a decided pair whose upper bound is strictly above its score
THRESHOLD_F = (8, 16)


def threshold_names():
    """{'below' (ub = lb - 1) | 'at' (ub = lb) | 'above' (ub = lb + 1): names of block-lattice cases}"""
    return {"below": [f"lat-s9-F{F}-r+1" for F in THRESHOLD_F], "at": [f"lat-s9-F{F}-tie" for F in THRESHOLD_F],
            "above": [f"lat-s9-F{F}-r-1" for F in THRESHOLD_F]}


def loose_upper_bound():
    """ub-above-F: a random target and the same with one base deleted a few bases before its end: F = 2, the diagonal-0 bound
    counts the shifted tail as mismatches and still lies below the 8-mer bound (about n / 8): decided, fwd reports the bound.
    ub-eq-lb-above-F: one X- and four Y-units (R - F = 3), and in the query's second half a base deleted and another
    inserted five further on: the forward score pays two gaps (12), diagonal 0 pays the shifted stretch (ub = 13) and the
    8-mer bound comes to 13 as well (R = 15): NOT decided -- `ub < lb` is strict -- so fwd reports F, not the bound"""
    t = unique(200, 7001)
    j = next(j for j in range(4, 10) if t[-j] != t[-j + 1])          # (deleting inside a run is a deletion at its end)
    out = [Case("ub-above-F", "threshold", t[:-j] + t[-j + 1:], t, (2, None))]
    q, t = plant(palindrome(LATTICE_HALF, 7303), interleave(1, 4, 2), 9, 7304)
    a, L = 230, 5
    q = q[:a] + q[a + 1:a + L] + bytes([_other(random.Random(a * 31 + L), q[a + L])]) + q[a + L:]
    return out + [Case("ub-eq-lb-above-F", "threshold", q, t, (12, 15))]


# ---- short: queries around the 8-mer length against a 200-bp target, taken from either strand of it
SHORT_L = (1, 7, 8, 9, 16)


def short():
    t = unique(200, 7101)
    r = rc(t)
    out = []
    for L in SHORT_L:
        out.append(Case(f"short-fwd{L}", "short", t[50:50 + L], t, None))
        out.append(Case(f"short-rev{L}", "short", r[31:31 + L], t, None))
    return out


# ---- other alphabets (4-bit and 8-bit symbols: no 8-mer bound).  The F = 8 and F = 16 cells with unit letters replaced:
#   'n'  the first C-unit's letter by N, the second's by the lower case of a NEW letter: both still cost one on either strand
#   'l'  also the third's by the lower case of the ORIGINAL letter: a mismatch forward (bytes are compared raw), none on the
#        reverse strand (the complement of a lower-case letter is the upper-case one)
# 8-bit: twelve IUPAC codes, each at a position and at its mirror position of BOTH sequences (equal on either strand).
IUPAC = b"RYSWKMBDHVry"


def alphabet_cases(bits):
    out = []
    for F in (8, 16):
        for d in DIFFS:
            for variant in ("n", "l"):
                u, v, c = composition(F, d)
                kinds = interleave(u, v, c)
                p = palindrome(LATTICE_HALF, 8100 + 10 * F + d)
                q, t = plant(p, kinds, 9, 8101 + 10 * F + d)
                q, t = bytearray(q), bytearray(t)
                cs = [5 + 9 * k for k, kind in enumerate(kinds) if kind == "C"]
                assert len(cs) >= 3
                q[cs[0]] = ord("N")
                q[cs[1]] = bytes([q[cs[1]]]).lower()[0]
                if variant == "l":
                    q[cs[2]] = bytes([p[cs[2]]]).lower()[0]
                if bits == 8:
                    n = len(p)
                    for k, code in enumerate(IUPAC):
                        i = 5 + 9 * k + 4
                        for s in (q, t):
                            s[i] = code; s[n - 1 - i] = code
                out.append(Case(f"a{bits}-F{F}-{DIFF_ID[d]}-{variant}", f"alphabet{bits}", bytes(q), bytes(t), None))
    return out


# ------------------------------------------------------------------------------------------ case sets and pair lists
@functools.lru_cache(maxsize=None)
def cases(group):
    return tuple({"lattice": block_lattice, "seam": length_seam, "wide": wide, "threshold": loose_upper_bound, "short": short,
                  "alphabet4": lambda: alphabet_cases(4), "alphabet8": lambda: alphabet_cases(8)}[group]())


TWO_BIT_GROUPS = ("lattice", "seam", "wide", "threshold", "short")
ALL_GROUPS = TWO_BIT_GROUPS + ("alphabet4", "alphabet8")
# what one context loads: the 2-bit cases in two lists of at most about 150 pairs
LISTS = {"lattice": ("lattice",), "rest": ("seam", "wide", "threshold", "short"), "seam-short": ("seam", "threshold", "short"),
         "lattice-wide": ("lattice", "wide"), "seam-wide": ("seam", "wide", "threshold"), "wide": ("wide",),
         "alphabet4": ("alphabet4",), "alphabet8": ("alphabet8",)}

Pair = namedtuple("Pair", "name q t")                   # one ordered pair of a list: 'case/qt', 'case/tq', 'case/qq', 'case/tt'


@functools.lru_cache(maxsize=None)
def pair_list(name):
    """-> (records, [(query index, target index)], [Pair]): every case of the list in both pair orders; the short cases
    also as self pairs"""
    recs, pairs, meta = [], [], []
    for group in LISTS[name]:
        for c in cases(group):
            i = len(recs)
            recs += [(c.name + ".q", c.q), (c.name + ".t", c.t)]
            pairs += [(i, i + 1), (i + 1, i)]
            meta += [Pair(c.name + "/qt", c.q, c.t), Pair(c.name + "/tq", c.t, c.q)]
            if group == "short":
                pairs += [(i, i)]
                meta += [Pair(c.name + "/qq", c.q, c.q)]
    if "short" in LISTS[name]:
        i = len(recs) - 1
        pairs.append((i, i)); meta.append(Pair(recs[i][0] + "/tt", recs[i][1], recs[i][1]))
    return recs, pairs, meta


def single(case_name, group="lattice"):
    """one case as a list of its own: (records, pairs, [Pair]) with the (q, t) order only"""
    c = next(c for c in cases(group) if c.name == case_name)
    return [(c.name + ".q", c.q), (c.name + ".t", c.t)], [(0, 1)], [Pair(c.name + "/qt", c.q, c.t)]


# ------------------------------------------------------------------------------------------ random pairs (host test)
def random_pairs(n=200, seed=9100):
    """seeded pairs of length 8..400: a base, a copy with substitutions and indels of up to 3 bases, truncated at either end,
    reverse-complemented in two cases of five (the generator of test_randomised_small_sets is the model)"""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        L = rng.randint(8, 400)
        base = bytes(rng.choice(ACGT) for _ in range(L))
        sub, indel = rng.choice([(0.0, 0.0), (0.01, 0.0), (0.03, 0.01), (0.08, 0.04), (0.3, 0.1)])
        b = bytearray()
        for ch in base:
            u = rng.random()
            if u < sub:
                b.append(_other(rng, ch))
            elif u < sub + indel / 2:
                continue
            elif u < sub + indel:
                b.append(ch); b.extend(rng.choice(ACGT) for _ in range(rng.randint(1, 3)))
            else:
                b.append(ch)
        lo = rng.randint(0, len(b) // 4) if rng.random() < 0.3 else 0
        hi = len(b) - (rng.randint(0, len(b) // 4) if rng.random() < 0.3 else 0)
        m = bytes(b[lo:hi])
        while len(m) < 8:
            m += bytes([rng.choice(ACGT)])
        if rng.random() < 0.4:
            m = rc(m)
        out.append((f"rnd{i}", base, m) if i % 2 else (f"rnd{i}", m, base))
    return out
