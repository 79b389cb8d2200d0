"""Host checks (-m "not gpu") for the stage tests of `-x tree:` pair selection: every recipe of tests/sketch_inputs.py has
the property it is named for (so that a change to a generator cannot quietly lose it), the plain reference has the
invariances of the definition, and the oracle's restatement of the definition (oracle/seqrush.c, a transcription of the
kernels' formulation) gives the pair lists of the independent reference."""
from fractions import Fraction

import pytest

import oracle_binding as ob
import repeat_inputs as ri
import sketch_inputs as si


# ------------------------------------------------------------------------------------------ 1. the recipes
def test_cut_members_sit_one_below_at_and_above_the_cut():
    recs = dict(si.cut_set())
    for L, distinct in ((1014, 999), (1015, 1000), (1016, 1001)):
        s = recs[f"r{L}"]
        assert len(s) == L and si.padded(L) == 1024 and set(s) <= set(b"ACGT")
        assert len(set(si.kmer_hashes(s, 16))) == distinct == L - 15
        assert len(si.sketch(s, 16)) == min(distinct, 1000)
    # 1001 distinct: the sketch drops exactly the largest hash
    assert si.sketch(recs["r1016"], 16) == sorted(set(si.kmer_hashes(recs["r1016"], 16)))[:-1]


def test_padding_jumps_between_1024_and_1025_with_the_cut_in_the_first_chunk():
    recs = dict(si.cut_set())
    assert (si.padded(1024), si.padded(1025)) == (1024, 2048)
    for L in (1024, 1025):
        a = si.sorted_padded(recs[f"r{L}"], 16)
        assert len(a) == si.padded(L) and len(a) // si.CHUNK == (1, 2)[L - 1024]
        assert si.distinct_before(a, si.CHUNK) >= 1000          # the scan ends on the count, not on the end of the array


def test_doubled_members_put_duplicates_and_the_cut_where_they_are_meant_to_be():
    recs = dict(si.chunk_set())
    a = si.sorted_padded(recs["xx800"], 16)
    assert len(recs["xx800"]) == 1600 and len(a) == 2048
    assert si.distinct_before(a, len(a)) == 800
    assert a[si.CHUNK - 1] == a[si.CHUNK] != si.SENTINEL      # the equal pair straddles the chunk boundary
    first = si.distinct_before(a, si.CHUNK)
    assert 450 <= first <= 600                                  # a count the second chunk has to start from
    assert a[si.CHUNK] in set(a[:si.CHUNK]) and first < 800
    b = si.sorted_padded(recs["xx1500"], 16)
    assert len(recs["xx1500"]) == 3000 and len(b) == 4096
    assert si.distinct_before(b, len(b)) == 1500
    assert si.distinct_before(b, si.CHUNK) < 1000 < si.distinct_before(b, 2 * si.CHUNK)      # the cut: inside the second chunk
    assert len(si.sketch(recs["xx1500"], 16)) == 1000


@pytest.mark.parametrize("name,period,length", [("p7", 7, 3000), ("p5", 5, 2500)])
def test_periodic_members_have_runs_across_both_chunk_boundaries(name, period, length):
    s = dict(si.chunk_set())[name]
    assert len(s) == length and s == (s[:period] * (length // period + 1))[:length]
    a = si.sorted_padded(s, 4)
    assert len(a) == 4096 and si.distinct_before(a, len(a)) == period == len(si.sketch(s, 4))
    for edge in (1024, 2048):
        assert a[edge - 1] == a[edge] != si.SENTINEL


def test_short_and_degenerate_members():
    recs = dict(si.chunk_set())
    assert len(set(si.kmer_hashes(recs["homo"], 16))) == 1 == len(set(si.kmer_hashes(recs["homo"], 4)))
    assert len(recs["homo"]) == 1500 and si.padded(1500) == 2048
    assert [si.padded(len(recs[f"len{i}"])) for i in (1, 2, 3)] == [2, 2, 4]
    assert max(si.padded(len(s)) for s in recs.values()) == 4096         # the stride beside N = 2
    assert [len(si.sketch(recs[f"len{i}"], 1)) for i in (1, 2, 3)] == [1, 2, 2]
    for k in si.KMER_SIZES:
        by = dict(si.kmer_set(k))
        assert [len(si.kmer_hashes(by[f"len_k{d:+d}"], k)) for d in (-1, 0, 1) if k + d > 0] == [0, 1, 2][(k == 1):]


def test_kmer_sizes_reach_the_edges_of_the_code():
    assert si.KMER_SIZES == (1, 2, 15, 16, 31, 32)
    every1 = set(si.kmer_hashes(b"ACGTacgt", 1))
    every2 = set(si.kmer_hashes(bytes(a for x in b"ACGT" for y in b"ACGT" for a in (x, y, ord("N"))), 2))
    assert len(every1) == 2 and len(every2) == 10
    for k in (1, 2):
        assert all(set(si.kmer_hashes(s, k)) <= (every1, every2)[k - 1] for _, s in si.kmer_set(k))
    # k = 32: both codes use all 64 bits -- T...T reads as code 2^64 - 1 forward and as 0 on the other strand
    t, a = b"T" * 32, b"A" * 32
    assert si.window_hash(t) == si.window_hash(a) == si.splitmix64((32 * si.GOLDEN) & si.M64)
    g = b"G" + b"T" * 31
    assert si.window_hash(g) == si.splitmix64(1 ^ ((32 * si.GOLDEN) & si.M64))      # A...AC on the other strand


def test_alphabet_members():
    by = dict(si.alphabet_set())
    up = by["upper"]
    assert len(by) == 10 and all(len(s) == 120 for n, s in by.items() if n != "all_n")
    for k in (1, 5, 16, 32):
        assert si.sketch(by["lower"], k) == si.sketch(by["mixed"], k) == si.sketch(up, k) != []
        assert si.kmer_hashes(by["all_n"], k) == ()
        # an invalid byte takes out exactly the windows that hold it
        assert si.kmer_hashes(by["bad_first"], k) == si.kmer_hashes(up, k)[1:] == si.kmer_hashes(up[1:], k)
        assert si.kmer_hashes(by["bad_last"], k) == si.kmer_hashes(up, k)[:-1] == si.kmer_hashes(up[:-1], k)
        for name, bad in (("n_mid", 2), ("iupac", 6), ("u", 2), ("hi", 3)):
            pos = [i for i in range(120) if by[name][i] != up[i]]
            assert len(pos) == bad
            holds = [i for i in range(120 - k + 1) if any(i <= p < i + k for p in pos)]
            assert si.kmer_hashes(by[name], k) == tuple(h for i, h in enumerate(si.kmer_hashes(up, k)) if i not in holds)
    assert any(b >= 0x80 for b in by["hi"]) and 0xC1 in by["hi"] and any(b >= 0x80 for b in by["bad_last"])


# ------------------------------------------------------------------------------------------ 2. the definition's invariances
ALL_SETS = sorted(si.SMALL_SETS)


@pytest.mark.parametrize("k", si.KMER_SIZES)
def test_reference_sketch_ignores_strand_and_case(k):
    seen = 0
    for name in ALL_SETS:
        for _, s in si.SMALL_SETS[name][0]():
            if len(s) > 400 and k > 2 and name != "cut":
                continue                                        # (the long repeats say nothing more here)
            assert si.sketch(s, k) == si.sketch(si.revcomp(s), k) == si.sketch(s.lower(), k) == si.sketch(s.upper(), k)
            seen += bool(si.sketch(s, k))
    assert seen > 20
    by = dict(si.kmer_set(k))
    assert by["a_rc"] != by["a"] and si.sketch(by["a_rc"], k) == si.sketch(by["a"], k) == si.sketch(by["a_lower"], k)


def test_reference_jaccard_cases():
    recs = si.jaccard_set()
    idx = {n: i for i, (n, _) in enumerate(recs)}
    sk, sh, dn = si.reference(recs, 16)
    at = lambda a, b: (sh[idx[a]][idx[b]], dn[idx[a]][idx[b]])      # noqa: E731
    assert sk[idx["all_n"]] == sk[idx["short"]] == []
    assert at("all_n", "short") == (0, 1)                             # both empty
    assert at("all_n", "x") == (0, len(sk[idx["x"]])) == (0, 285)     # one empty
    assert at("x", "x_same") == (285, 285) == at("x", "x_rc")         # identical; a member beside its reverse complement
    assert at("x", "y") == (0, 570)                                   # disjoint
    s, d = at("long_a", "long_b")
    A, B = set(sk[idx["long_a"]]), set(sk[idx["long_b"]])
    assert len(A) == len(B) == 1000 and d == 1000
    assert 0 < s < len(A & B)                                         # matches beyond the first 1000 of the union do not count
    s, d = at("x", "x_mut")
    assert 0 < s < d < 570
    assert all(sh[i][i] == dn[i][i] == 0 for i in range(len(recs)))


def test_big_set_fits_ten_bit_masks():
    recs = si.big_set()
    assert len(recs) == 2049 and len(recs) ** 2 > 16384 * 256 >= 2048 ** 2 and all(len(s) == 12 for _, s in recs)
    sk, universe, masks = si.big_masks(recs)
    assert len(universe) == 10 and max(masks) < 1024 and len(set(masks)) > 100
    for i, j in ((0, 1), (5, 2048), (2047, 2048), (1000, 3)):
        shared, denom = si.jaccard(sk[i], sk[j])
        assert (shared, denom) == (bin(masks[i] & masks[j]).count("1"), max(1, bin(masks[i] | masks[j]).count("1")))


# ------------------------------------------------------------------------------------------ 3. the selection rule
@pytest.mark.parametrize("variant", si.SELECT_VARIANTS)
@pytest.mark.parametrize("n", si.SELECT_N)
def test_reference_selection_properties(n, variant):
    sh, dn, row = si.select_matrix(n, variant)
    assert all(sh[i][j] == sh[j][i] <= dn[i][j] == dn[j][i] <= 1000 for i in range(n) for j in range(n))
    assert all(dn[i][j] >= 1 for i in range(n) for j in range(n) if i != j)
    if row is not None:
        fr = {Fraction(sh[row][j], dn[row][j]) for j in range(n) if j != row}
        assert fr == {Fraction(1, 2) if variant == "equal" else Fraction(0)}
        assert len({dn[row][j] for j in range(n) if j != row}) == min(3, n - 1)
    for kn, kf in si.select_k(n):
        sel = si.selection(sh, dn, kn, kf)
        for i in range(n):
            near = [j for j in range(n) if sel[i][j] & 1]
            far = [j for j in range(n) if sel[i][j] & 2]
            assert sel[i][i] == 0                                                   # the diagonal is never selected
            assert len(near) == min(kn, n - 1) and len(far) == min(kf, n - 1)       # an exhausted row ends the selection
            if kn + kf > n - 1 and n > 1:
                assert set(near) & set(far)                                         # one j may carry both bits
            if i == row:                                                            # all equal: the lowest indices win
                others = [j for j in range(n) if j != i]
                assert near == others[:len(near)] and far == others[:len(far)]
            for chosen, sign in ((near, 1), (far, -1)):
                for j in chosen:                                                    # nothing left out beats what was chosen
                    for o in range(n):
                        if o != i and o not in chosen:
                            d = sign * (Fraction(sh[i][o], dn[i][o]) - Fraction(sh[i][j], dn[i][j]))
                            assert d < 0 or (d == 0 and o > j)


def test_reference_pair_list_rule():
    sel = [[0, 1, 0, 0], [0, 0, 0, 0], [0, 0, 0, 2], [0, 0, 0, 0]]
    assert si.pair_list(4, sel, 42, 0.0) == [(0, 0), (0, 1), (1, 0), (1, 1), (2, 2), (2, 3), (3, 2), (3, 3)]
    assert si.pair_list(4, sel, 42, 0.0, exclude_self=True) == [(0, 1), (1, 0), (2, 3), (3, 2)]
    assert si.pair_list(4, sel, 42, 1.0) == [(q, t) for q in range(4) for t in range(4)]
    assert si.pair_list(1, None, 42, 0.5) == [(0, 0)] and si.pair_list(1, None, 42, 0.5, True) == []
    half = si.pair_list(40, None, 42, 0.5, True)
    assert 600 < len(half) < 960 and all((t, q) in set(half) for q, t in half)
    assert si.parse_spec("tree:3,3,0.1") == (3, 3, 0.1, 16) and si.parse_spec("tree:1,0,0,1") == (1, 0, 0.0, 1)
    assert si.unit(si.M64) < 1.0 and si.unit(0) == 0.0


# ------------------------------------------------------------------------------------------ 4. the oracle against the reference
def _oracle_sets():
    out = {name: si.SMALL_SETS[name][0] for name in ALL_SETS}
    out["repeats_with_long"] = lambda: ri.sketch_set(with_long=True)
    return out


@pytest.mark.parametrize("name", sorted(_oracle_sets()))
def test_oracle_pair_lists_equal_the_reference(name):
    """oracle/seqrush.c restates the kernels' formulation line by line; this pins it to an independent statement of the rule"""
    recs = _oracle_sets()[name]()
    assert 1 < len(recs) <= 64
    o = ob.OracleSeqRush(records=recs)
    assert [o.seq(i)[1] for i in range(len(recs))] == [s for _, s in recs]       # the FASTA loader kept every byte
    for spec in si.SPECS:
        for ex in (False, True):
            assert o.sparsified_pairs(spec, exclude_self=ex) == si.tree_pairs(recs, spec, exclude_self=ex), (spec, ex)
    o.close()
