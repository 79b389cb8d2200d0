"""Seeded inputs whose searches run thousands of score levels with most diagonals OFF the matrix (plain helper module: no
device, no oracle calls): the target is a prefix or a suffix of the query, the query with a hole in it, or unrelated to it.
An optimal alignment is then one long gap (or nothing but mismatches and gaps), the wavefront is as wide as the score and
all of it but the sliver over the shorter sequence lies outside the matrix -- where the blocked kernel's packed 16-bit cells
hold NULLs that nothing real ever overwrites (sr_blk_tile.inc, q4_renull).  Random divergence, which every other deep test
uses, keeps most diagonals inside.

Every constructor is a pure function of its name (synth's counter streams) and returns [(name, bytes)], at most three
sequences; the suites align every ordered pair, so each gap is seen as an insertion and as a deletion.  The sizes are the
smallest that reach the level counts the tests state (test_deep_host.py asserts them)."""
from seqrush_amd import synth

SEED_X, SEED_Y = 8101, 8102                # the 12 kb and the 30 kb base sequence
SEED_U = 8110                               # unrelated pairs: SEED_U + length // 1000 and the next one


def unique(L, seed):
    """iid uniform ACGT (synth's counter stream)"""
    return synth.to_bytes(synth.base_sequence(L, seed))


def _x():
    return unique(12000, SEED_X)


def prefix12k():
    x = _x()
    return [("x", x), ("pre", x[:1000])]


def suffix12k():
    x = _x()
    return [("x", x), ("suf", x[-1000:])]


def hole12k():
    """x against its first and last kilobase joined: one internal gap of 10 000"""
    x = _x()
    return [("x", x), ("ends", x[:1000] + x[-1000:])]


def prefix9k():
    x = _x()
    return [("x9", x[:9000]), ("pre", x[:1000])]


def _unrelated(L):
    return [("u", unique(L, SEED_U + 2 * (L // 1000))), ("v", unique(L, SEED_U + 2 * (L // 1000) + 1))]


def unrelated3k():
    return _unrelated(3000)


def unrelated6k():
    return _unrelated(6000)


def unrelated8k():
    return _unrelated(8000)


def prefix24k():
    y = unique(24000, SEED_Y)
    return [("y24", y), ("pre", y[:4000])]


def prefix30k():
    y = unique(30000, SEED_Y)
    return [("y30", y), ("pre", y[:12000])]


def deep_then_shallow():
    """x, its first kilobase and a copy of that with 2 % substitutions: a workgroup that aligns all pairs one after the
    other runs a shallow search (score ~ 100) in the ring a deep one (11 024) has just left"""
    x = _x()
    snp = synth.to_bytes(synth.substitute(synth.base_sequence(12000, SEED_X)[:1000], 0.02, SEED_X + 1))
    return [("x", x), ("pre", x[:1000]), ("snp", snp)]


SETS = {f.__name__: f for f in (prefix12k, suffix12k, hole12k, prefix9k, unrelated3k, unrelated6k, unrelated8k, prefix24k,
                                prefix30k, deep_then_shallow)}
# length of the one gap an optimal alignment of (longer, shorter) consists of -- the sets with a closed-form score
GAP = {"prefix12k": 11000, "suffix12k": 11000, "hole12k": 10000, "prefix9k": 8000, "prefix24k": 20000, "prefix30k": 18000}


DEFAULT = "0,5,8,2,24,1"
ONE_PIECE, GENERIC, LEVEL_KERNEL = "0,5,8,2", "0,5,8,2,13,1", "0,4,6,2,24,1"
CLOSED_FORM_SCORES = (DEFAULT, ONE_PIECE, GENERIC)

# ------------------------------------------------------------------------------------------ the regime
# First level whose tiles reset creeping NULLs (copies of seqrush_amd/csrc/sr_blk_tile.inc:376-377, `#define SR_DEEP_INT16` /
# `#define SR_DEEP_RING16`; test_deep_host.py compares them with that file): int16 rows / the 16-bit ring of 32-bit searches.
SR_DEEP_INT16, SR_DEEP_RING16 = 3000, 1500
# Levels near which a NULL that crept through the sources q4_renull does NOT reset could reach the valid range.  These two
# are the round-4 advisor's estimates from reading the code, with no run behind them -- not measurements.
EST_INT16, EST_RING16 = 6600, 3300
# what a set must reach per side of its bidirectional search (score // 2) to count as past the estimate
NEED = {"int16": EST_INT16 + 1000, "ring16": EST_RING16 + 1500}
DEEP = {"int16": SR_DEEP_INT16, "ring16": SR_DEEP_RING16}

RING16_SETS = ("prefix12k", "suffix12k", "hole12k", "unrelated6k", "deep_then_shallow")
INT16_SETS = ("prefix24k", "prefix30k", "unrelated6k", "unrelated8k")
PENALTY_SETS = ("prefix9k", "hole12k")
# every (instance, set, scores) the device suite runs on the packed tiles ("ring16" = SR_FORCE_INT32=1: under GENERIC, whose
# 5-level instance has no 16-bit ring, that is the 32-bit tile on int32 rows -- same inputs, same depth conditions)
CASES = ([("ring16", s, DEFAULT) for s in RING16_SETS] + [("int16", s, DEFAULT) for s in INT16_SETS] +
         [(i, s, p) for s in PENALTY_SETS for p in (ONE_PIECE, GENERIC) for i in ("int16", "ring16")])
# The cases that cannot reach NEED at these sizes: the second gap piece halves the score of a one-gap alignment, and 6 kb
# of unrelated sequence is the ring16 size.  They stay (the same inputs on the other instance, the other penalties on the
# same inputs) and must spend at least 1000 levels per side in the reset branch: DEEP + 1000.
SHORT_OF_ESTIMATE = {("int16", "unrelated6k", DEFAULT), ("int16", "prefix9k", GENERIC), ("ring16", "prefix9k", GENERIC),
                     ("int16", "hole12k", GENERIC)}


def levels_needed(instance, name, scores=DEFAULT):
    return DEEP[instance] + 1000 if (instance, name, scores) in SHORT_OF_ESTIMATE else NEED[instance]


def gap_score(scores, g):
    """min(o1 + g e1, o2 + g e2): what one gap of g costs under "m,x,o1,e1[,o2,e2]" """
    v = [int(t) for t in scores.split(",")]
    return min(v[2] + g * v[3], v[4] + g * v[5]) if len(v) == 6 else v[2] + g * v[3]
