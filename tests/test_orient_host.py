"""Host tests (no device) of the orientation tests' own material (tests/orient_inputs.py): the plain DP reference against the
oracle's two aligners, every named case against the (F, R) it is built to have, the window arithmetic that says where the
wide and seam cases put the end diagonal, the oracle's strand decision against "reverse iff R < F" under four penalty sets,
and the two inequalities sr_orient_blk_kernel's shortcuts rest on: lb <= R and ub >= F."""
import random

import pytest

import instance_matrix as im
import oracle_binding as ob
import orient_inputs as oi
import repeat_inputs as ri


def pen_of(ori):
    x, o, e = oi.parse_ori(ori)
    return ob.Penalties.of(0, x, o, e)


def oracle_params(orientation_scores):
    """the oracle's defaults with these orientation penalties"""
    op = ob.default_params()
    op.threads = 4
    op.ori = pen_of(orientation_scores)
    op.min_match_len = 0
    op.memory_mode = ob.MEM_ULTRALOW
    return op


# ------------------------------------------------------------------------------------------ the reference itself
def test_reference_on_known_answers():
    assert oi.ref_score(b"ACGT", b"ACGT", 1, 1, 1) == 0
    assert oi.ref_score(b"ACGT", b"AGGT", 1, 1, 1) == 1
    assert oi.ref_score(b"ACGT", b"AGGT", 7, 1, 1) == 4                    # two gaps of one are cheaper than the mismatch
    assert oi.ref_score(b"ACGTACGT", b"ACGT", 1, 3, 2) == 3 + 2 * 4
    assert oi.ref_score(b"", b"ACG", 1, 1, 1) == 4 and oi.ref_score(b"ACG", b"", 1, 1, 1) == 4
    assert oi.ref_score(b"A", b"a", 1, 1, 1) == 1                          # bytes are compared raw
    assert oi.ref_score(b"AAAATTTT", b"AAAACCTTTT", 4, 2, 1) == 2 + 2      # one gap of two, not two gaps of one (6)
    assert oi.ref_score(b"ACGTT", b"AGTTC", 1, 0, 1) == 2                   # gap-open 0: one deletion, one insertion


@pytest.mark.parametrize("ori", (oi.DEFAULT_ORI,) + oi.OTHER_ORI + ("0,4,6,2", "0,3,0,1"))
def test_reference_equals_the_oracles_aligners(ori):
    """the row-vectorised recurrence against the oracle's Gotoh and its wavefront score on seeded pairs with indels,
    truncations and unrelated sequence: three implementations, two algorithms"""
    x, o, e = oi.parse_ori(ori)
    rng = random.Random(9300 + 100 * x + 10 * o + e)
    pen = pen_of(ori)
    pairs = [(a, b) for _, a, b in oi.random_pairs(24, seed=9200 + x + o)]
    pairs += [(bytes(rng.choice(b"ACGT") for _ in range(rng.randint(1, 60))), bytes(rng.choice(b"ACGT") for _ in range(rng.randint(1, 60))))
              for _ in range(12)]
    for a, b in pairs:
        want = oi.ref_score(a, b, x, o, e)
        assert want == ob.gotoh(a, b, pen) == ob.wfa_score(a, b, pen), (ori, len(a), len(b))


# ------------------------------------------------------------------------------------------ the cases
def test_named_cases_have_their_intended_scores():
    """every 2-bit case that names its (F, R) under 0,1,1,1 has them, in both pair orders (on ACGT the reverse score of (t, q)
    is that of (q, t): reverse-complementing both sequences of an alignment mirrors it)"""
    n = 0
    for group in oi.TWO_BIT_GROUPS:
        for c in oi.cases(group):
            if c.want is None:
                continue
            for q, t in ((c.q, c.t), (c.t, c.q)):
                got = oi.expect(q, t)
                assert all(w is None or w == g for w, g in zip(c.want, got)), (c.name, got, c.want)
            n += 1
    assert n == 60 + 30 + 6 + 2
    names = [c.name for g in oi.ALL_GROUPS for c in oi.cases(g)]
    assert len(set(names)) == len(names)


def test_every_lattice_point_is_there():
    have = {c.want for c in oi.cases("lattice") if "-s9-" in c.name}
    assert have == {(F, F + d) for F in (6, 7, 8, 9, 15, 16, 17, 23, 24, 25) for d in (-1, 0, 1)}
    assert have == {c.want for c in oi.cases("lattice") if "-s3-" in c.name}
    assert {c.want for c in oi.cases("seam")} == {(F + 1 + cut, F + d + 1 + cut) for F in (8, 16) for d in (-1, 0, 1) for cut in range(1, 6)}
    assert {len(c.q) % 4 for c in oi.cases("seam")} == {0, 1, 2, 3}
    assert sorted({len(c.q) for c in oi.cases("short")}) == [1, 7, 8, 9, 16] and {len(c.t) for c in oi.cases("short")} == {200}
    # the short queries come from either strand: some pair goes forward and some reverse on the reference's word alone
    sr = [oi.expect(c.q, c.t) for c in oi.cases("short")]
    assert any(r < f for f, r in sr) and any(f < r for f, r in sr)


@pytest.mark.parametrize("bits", [4, 8])
def test_alphabet_cases_cover_the_three_differences(bits):
    """lower case and IUPAC letters change the intended scores (a and A both complement to T): whatever the DP measures holds,
    but each alphabet keeps a pair with R = F - 1, one with R = F and one with R = F + 1 at F >= 8 -- in both pair orders"""
    for order in (0, 1):
        seen = set()
        for c in oi.cases(f"alphabet{bits}"):
            f, r = oi.expect(c.q, c.t) if order == 0 else oi.expect(c.t, c.q)
            if f >= 8:
                seen.add(r - f)
        assert {-1, 0, 1} <= seen, (bits, order, seen)
    # the lower-case unit of the 'l' variants costs the forward strand alone
    by = {c.name: oi.expect(c.q, c.t) for c in oi.cases(f"alphabet{bits}")}
    for name, (f, r) in by.items():
        if name.endswith("-l"):
            assert (f, r + 1) == by[name[:-2] + "-n"], name


def test_symbol_bits_of_every_list():
    want = {"alphabet4": 4, "alphabet8": 8}
    for name in oi.LISTS:
        recs, pairs, meta = oi.pair_list(name)
        assert im.symbol_bits(recs) == want.get(name, 2), name
        assert len(pairs) == len(meta) <= 160, (name, len(pairs))
        assert all(recs[q][1] == m.q and recs[t][1] == m.t for (q, t), m in zip(pairs, meta))
        assert max(len(s) for _, s in recs) <= (1400 if "wide" in oi.LISTS[name] else 400)


# ------------------------------------------------------------------------------------------ where the end diagonal falls
def test_wide_cases_need_a_second_tile():
    """sr_orient_blk_kernel / ori_pass8: shift = plen + 24, window = reach of the block's last level + OB + 2 on each side,
    60 owned lanes of four diagonals: the first block with two tiles starts at level 104"""
    assert oi.blk_geometry(1400, 1400, 103).nt == 1 and oi.blk_geometry(1400, 1400, 104).nt == 2
    assert oi.blk_geometry(1400, 1400, 104).s0 == 104
    for c in oi.cases("wide"):
        f, r = oi.expect(c.q, c.t)
        for plen, tlen in ((len(c.q), len(c.t)), (len(c.t), len(c.q))):
            assert oi.blk_geometry(plen, tlen, min(f, r)).nt >= 2, c.name
    spots = {}
    for c in oi.cases("wide"):
        if "kend" in c.name:
            f, r = oi.expect(c.q, c.t)
            g = oi.blk_geometry(len(c.q), len(c.t), min(f, r))
            spots[c.name] = (g.tile, g.lane)
            assert oi.blk_geometry(len(c.t), len(c.q), min(f, r)).tile == 0          # negative end diagonal
    assert spots["wide-kend59"] == (0, 61) and spots["wide-kend61"] == (1, 2), spots          # either side of the tile seam
    assert spots["wide-kend130"][0] == 1 and 2 < spots["wide-kend130"][1] < 61, spots
    # past the level kernel's ring of scope + 1 rows under 0,1,76,1 (79) as well
    assert all(min(oi.expect(c.q, c.t, "0,1,76,1")) > 79 for c in oi.cases("wide"))


def test_seam_cases_put_the_end_diagonal_on_every_cell():
    cells, signs = set(), set()
    for c in oi.cases("seam"):
        f, r = oi.expect(c.q, c.t)
        for q, t in ((c.q, c.t), (c.t, c.q)):
            g = oi.blk_geometry(len(q), len(t), min(f, r))
            assert g.nt == 1 and 2 <= g.lane <= 61
            cells.add(g.cell); signs.add(len(t) > len(q))
    assert cells == {0, 1, 2, 3} and signs == {True, False}
    # an end diagonal in the last group of the window: a one-base query against 200 bases
    assert any(oi.blk_geometry(len(c.q), len(c.t), min(oi.expect(c.q, c.t))).last_group for c in oi.cases("short"))


# ------------------------------------------------------------------------------------------ DP against the oracle
def oracle_strands(name, ori):
    recs, pairs, meta = oi.pair_list(name)
    o = ob.OracleSeqRush(records=recs)
    op = oracle_params(ori)
    out = [o.align_pair(op, q, t)["is_reverse"] for q, t in pairs]
    o.close()
    return out


@pytest.mark.parametrize("name", ["lattice", "rest", "alphabet4", "alphabet8"])
def test_oracle_strand_is_reverse_iff_r_below_f(name):
    recs, pairs, meta = oi.pair_list(name)
    for m, got in zip(meta, oracle_strands(name, oi.DEFAULT_ORI)):
        f, r = oi.expect(m.q, m.t)
        assert got == (r < f), (m.name, f, r)


@pytest.mark.parametrize("ori", oi.OTHER_ORI)
def test_oracle_strand_under_other_penalties(ori):
    recs, pairs, meta = oi.pair_list("lattice")
    n_rev = 0
    for m, got in zip(meta, oracle_strands("lattice", ori)):
        f, r = oi.expect(m.q, m.t, ori)
        assert got == (r < f), (ori, m.name, f, r)
        n_rev += got
    assert 0 < n_rev < len(meta)


# ------------------------------------------------------------------------------------------ the bounds
def check_bounds(name, q, t):
    l, u = oi.lb(q, t), oi.ub(q, t)
    f = oi.ref_score(q, t, 1, 1, 1)
    assert u >= f, f"{name}: ub {u} < F {f}"
    if l > 0:
        r = oi.ref_score(oi.rc(q), t, 1, 1, 1)
        assert l <= r, f"{name}: lb {l} > R {r}"


def test_bounds_hold_on_every_case():
    for name in ("lattice", "rest", "alphabet4", "alphabet8"):
        for m in oi.pair_list(name)[2]:
            f, r = oi.expect(m.q, m.t)
            assert oi.lb(m.q, m.t) <= r and oi.ub(m.q, m.t) >= f, m.name


@pytest.mark.parametrize("family", ["palindromes", "two_letter", "satellite", "microsatellites"])
def test_bounds_hold_on_repeat_families(family):
    recs = ri.SMALL_FAMILIES[family]()
    for qn, q in recs:
        for tn, t in recs:
            check_bounds(f"{family} {qn} {tn}", q, t)


def test_bounds_hold_on_random_pairs():
    pairs = oi.random_pairs(200)
    assert len(pairs) == 200 and all(8 <= len(a) <= 500 and 8 <= len(b) <= 500 for _, a, b in pairs)
    decided = 0
    for name, q, t in pairs:
        check_bounds(name, q, t)
        decided += oi.shortcut(q, t)
    assert 20 <= decided <= 180, decided                       # both regimes occur


def test_lattice_sits_on_the_threshold():
    """under 0,1,1,1: ub = F in both pair orders and, at spacing 9, lb = R in the order the cases are named in -- the order
    the threshold pairs are loaded alone in, which is what makes them exact.  In the other order the target's 8-mer set may
    hold a few more of the query's (two tie cells measure lb = R - 1); nothing depends on it: the device tests work out the
    shortcut per ordered pair.  At spacing 3 lb is far below R from F = 15 on: the reverse aligner starts blocks before it
    can finish"""
    for c in oi.cases("lattice"):
        f, r = oi.expect(c.q, c.t)
        for q, t in ((c.q, c.t), (c.t, c.q)):
            assert oi.ub(q, t) == f, c.name
            if "-s9-" in c.name:
                if q is c.q:
                    assert oi.lb(q, t) == r, c.name
                else:
                    assert r - 1 <= oi.lb(q, t) <= r, c.name
            elif f >= 15:
                assert 0 < oi.lb(q, t) < r - 1, c.name
    by = {c.name: c for c in oi.cases("lattice")}
    for kind, delta in (("below", -1), ("at", 0), ("above", 1)):
        for name in oi.threshold_names()[kind]:
            c = by[name]
            assert oi.ub(c.q, c.t) - oi.lb(c.q, c.t) == delta and oi.shortcut(c.q, c.t) == (delta < 0), name
    c, e = oi.cases("threshold")
    f, r = oi.expect(c.q, c.t)
    assert f == 2 and 3 <= oi.ub(c.q, c.t) <= 5 and oi.ub(c.q, c.t) < oi.lb(c.q, c.t) <= r and oi.shortcut(c.q, c.t)
    # on the threshold with a bound that is not the score: the kernel must run its aligners and report F
    assert oi.expect(e.q, e.t) == (12, 15) and oi.ub(e.q, e.t) == oi.lb(e.q, e.t) == 13 and not oi.shortcut(e.q, e.t)
