"""CPU census of the two tie rules of mirrored emission on the tie lattice (tests/tie_inputs.py): the claim
that the alignment of (t, q) is the transpose of the alignment of (q, t) unless rule 1 (backtrace, M step) or rule 2
(breakpoint choice) decided something -- checked pair by pair, search by search and base case by base case with the traced
oracle (sro_wfa_align_traced), whose tie bits restate the transposed pair's order on their own, without csrc/sr_mirror_rule.h.
The table of DESIGN.md 4.3 "Census" is Census.row() of every family; its last column must be 0.  No GPU."""
import ctypes as C

import pytest

import mirror_inputs as mi
import oracle_binding as ob
import tie_inputs as ti
from seqrush_amd import _lib

# what the chosen seeds give: unordered forward pairs, pairs whose two CIGARs are not transposes, pairs with a tie bit in
# either order, searches with the rule-2 bit, base cases with the rule-1 bit (both orders), pairs with an unflagged depth-0
# search above a flagged record
PINNED = {
    "equal_blocks_15": (15, 3, 3, 0, 6, 3),
    "equal_blocks_16": (15, 4, 4, 8, 0, 0),
    "equal_blocks_17": (15, 4, 4, 8, 0, 0),
    "unequal_blocks_400": (15, 5, 5, 10, 0, 3),
    "unequal_blocks_800": (15, 6, 6, 10, 2, 6),
    "unequal_blocks_1600": (15, 4, 4, 4, 6, 4),
    "copy_number_2": (10, 0, 0, 0, 0, 0),
    "copy_number_7": (10, 2, 2, 4, 0, 0),
    "copy_number_40": (10, 2, 2, 4, 0, 0),
    "crossover_gaps": (21, 0, 0, 0, 0, 0),
    "threshold_lengths": (15, 1, 1, 2, 0, 0),
    "threshold_scores": (28, 0, 0, 0, 0, 0),
    "skewed": (21, 3, 3, 6, 0, 0),
    "deep_ties": (15, 5, 5, 6, 4, 5),
    "one_reversed": (6, 0, 0, 0, 0, 0),
    "palindromic": (25, 10, 10, 20, 0, 0),
}
ONE_PIECE_PINNED = {"equal_blocks_16": (15, 4, 4, 8, 0, 0), "deep_ties": (15, 4, 4, 2, 8, 4)}
CASES = [(n, ti.DEFAULT_SCORES) for n in ti.FAMILIES] + [(n, ti.ONE_PIECE) for n in ONE_PIECE_PINNED]
IDS = [n if s == ti.DEFAULT_SCORES else n + "-one-piece" for n, s in CASES]


MIN_LENGTH = 100                                # SRO_BIALIGN_FALLBACK_MIN_LENGTH (oracle/sr_oracle.h)


def counts(c):
    r = c.row()
    return (r["pairs"], r["non_transposable"], r["flagged"], r["rule2_searches"], r["rule1_base_cases"], len(c.deep_tie_pairs()))


@pytest.mark.parametrize("name", sorted(ti.FAMILIES))
def test_family_shape(name):
    recs = ti.records(name)
    assert 2 <= len(recs) <= 8 and len({n for n, _ in recs}) == len(recs)
    assert all(set(s) <= set(b"ACGT") and len(s) >= 1 for _, s in recs)
    assert max(len(s) for _, s in recs) <= (3000 if name == "deep_ties" else 1600)
    assert recs == tuple(ti.FAMILIES[name]())                      # deterministic


def test_what_the_families_are_named_for():
    lens = [len(s) for _, s in ti.records("threshold_lengths")]
    assert {max(a, b) for i, a in enumerate(lens) for b in lens[i + 1:]} == {99, 100, 101}
    # max(|q|, |t|) <= 100 is a base case at depth 0, 101 a search
    c = ti.census("threshold_lengths")
    for (q, t), tr in c.trace.items():
        assert (tr.recs[0]["kind"] == ob.TRACE_SEARCH) == (max(lens[q], lens[t]) > MIN_LENGTH), (q, t)
    # a depth-1 segment with score_remaining <= 250 is a base case, above it a search (its sides are longer than 100 here)
    c = ti.census("threshold_scores")
    seen = {}
    for tr in c.trace.values():
        top = tr.recs[0]
        kids = [r for r in tr.recs if r["depth"] == 1]
        assert top["kind"] == ob.TRACE_SEARCH and len(kids) == 2
        for rem, kid in zip((top["score_f"], top["score_r"]), kids):
            if max(kid["pe"] - kid["pb"], kid["te"] - kid["tb"]) > MIN_LENGTH:
                seen.setdefault(rem, set()).add(kid["kind"])
    assert seen[249] == {ob.TRACE_BASE} and seen[250] == {ob.TRACE_BASE} and seen[251] == {ob.TRACE_SEARCH}
    assert all(k == ({ob.TRACE_BASE} if rem <= 250 else {ob.TRACE_SEARCH}) for rem, k in seen.items())
    lens = sorted(len(s) for _, s in ti.records("skewed"))
    assert lens[:4] == [120] * 4 and lens[4:] == [1500] * 3
    d = ti.census("deep_ties")
    assert len(ti.records("deep_ties")) >= 6 and all(1600 <= len(s) <= 3000 for _, s in ti.records("deep_ties"))
    assert min(tr.score for tr in d.trace.values()) >= 750 and d.row()["max_depth"] >= 2
    assert len(d.deep_tie_pairs()) >= 3
    # crossover: gaps of 15, 16, 17 in both directions, and no rule is needed there
    x = ti.census("crossover_gaps")
    runs = {(op, len(run)) for tr in x.trace.values() for op in b"ID" for run in tr.cigar.replace(b"X", b"M").split(b"M") if run and run[0] == op}
    assert {(op, L) for op in b"ID" for L in (15, 16, 17)} <= runs
    assert x.row()["flagged"] == 0 and x.row()["non_transposable"] == 0
    # copy number: the rule-2 bit sits on searches
    assert sum(ti.census(f"copy_number_{u}").row()["rule2_searches"] for u in ti.COPY_UNITS) >= 2
    # the strand families have both strands, the others only the forward one
    for name in ti.STRANDED:
        o = ti.oracle_once(name)
        assert 0 < len(ti.census(name).pairs) and (name != "one_reversed" or len(o.reverse_pairs()) == 8)
    o = ti.oracle_once("palindromic")
    pal = [i for i, (n, _) in enumerate(ti.records("palindromic")) if n in ("pal", "pal_mid")]
    assert all(not o.pairs[q, t]["is_reverse"] for q in pal for t in pal)          # equal orientation scores: forward wins


@pytest.mark.parametrize("name,scores", CASES, ids=IDS)
def test_inputs_are_not_vacuous_and_counts_are_pinned(name, scores):
    c = ti.census(name, scores)
    got = counts(c)
    if name in ti.CONDITIONED and scores == ti.DEFAULT_SCORES:
        nt = c.non_transposable()
        with_gaps = [p for p in c.pairs if c.transposable(*p) and (b"I" in c.trace[p].cigar or b"D" in c.trace[p].cigar)]
        assert len(nt) >= 2 and len(with_gaps) >= 2, (name, len(nt), len(with_gaps))
    assert got == (PINNED if scores == ti.DEFAULT_SCORES else ONE_PIECE_PINNED)[name], (name, got)


@pytest.mark.parametrize("name,scores", CASES, ids=IDS)
def test_traced_equals_untraced(name, scores):
    """the traced entry point gives the CIGAR and score of sro_wfa_align, the leaves' slices tile the CIGAR in order, every
    search splits into exactly its two children"""
    c = ti.census(name, scores)
    recs = ti.records(name)
    for (q, t), tr in c.trace.items():
        cig, sc = ob.wfa_align(recs[q][1], recs[t][1], c.pen)
        assert (tr.cigar, tr.score) == (cig, sc), (name, q, t)
        at = 0
        for r in tr.leaves:
            assert r["cig_b"] == at and r["cig_e"] >= at
            sl = tr.cigar[r["cig_b"]:r["cig_e"]]
            assert sl.count(b"M") + sl.count(b"X") + sl.count(b"D") == r["pe"] - r["pb"]
            assert sl.count(b"M") + sl.count(b"X") + sl.count(b"I") == r["te"] - r["tb"]
            at = r["cig_e"]
        assert at == len(tr.cigar)
        top = tr.recs[0]
        assert (top["depth"], top["pb"], top["pe"], top["tb"], top["te"], top["cb"], top["ce"]) == (0, 0, len(recs[q][1]), 0, len(recs[t][1]), 0, 0)
        for i, r in enumerate(tr.recs):
            if r["kind"] != ob.TRACE_SEARCH:
                continue
            first = tr.recs[i + 1]
            second = next(x for x in tr.recs[i + 2:] if x["depth"] == r["depth"] + 1)
            assert ti.seg_key(first) == (r["pb"], r["bv"], r["tb"], r["bh"], r["cb"], r["comp"])
            assert ti.seg_key(second) == (r["bv"], r["pe"], r["bh"], r["te"], r["comp"], r["ce"])
    if name in ti.STRANDED and scores == ti.DEFAULT_SCORES:     # the pair-level oracle on these pairs is this alignment
        o = ti.oracle_once(name)
        for p, tr in c.trace.items():
            assert (o.pairs[p]["cigar"], o.pairs[p]["score"]) == (tr.cigar, tr.score)


@pytest.mark.parametrize("name,scores", CASES, ids=IDS)
def test_two_rules_suffice(name, scores):
    """pair level: no bit on any record of (q, t) -> cigar(t, q) is the transpose.  Search level (the replay's premise): a
    search without a bit on it or above it has a twin in the other order with the transposed breakpoint and the same two
    scores; a base case without a bit under unflagged searches has a twin whose slice of the CIGAR is the transpose.  Flags
    are symmetric: a record and its twin carry the same bit wherever both exist"""
    c = ti.census(name, scores)
    n_search = n_base = 0
    for q, t in c.pairs:
        for a, b in ((c.trace[q, t], c.trace[t, q]), (c.trace[t, q], c.trace[q, t])):
            assert a.score == b.score
            if not a.flagged:
                assert mi.transpose(a.cigar) == b.cigar, f"{name}: ({q},{t}) carries no tie bit and is not transposable"
            for r in a.recs:
                w = b.twin_of(r)
                if w is not None:
                    assert w["tie"] == r["tie"] and w["depth"] == r["depth"], (name, q, t, r, w)
                if r["anc_tie"]:
                    continue
                assert w is not None and not w["anc_tie"], (name, q, t, r)
                if r["kind"] == ob.TRACE_SEARCH:
                    if not r["tie"]:
                        ti.transposed_search(r, b)
                        n_search += 1
                elif not r["tie"]:
                    assert mi.transpose(a.cigar[r["cig_b"]:r["cig_e"]]) == b.cigar[w["cig_b"]:w["cig_e"]], (name, q, t, r)
                    n_base += 1
    assert n_search > 0 or name == "threshold_lengths"
    assert n_base > 0
    assert c.row()["unflagged_but_different"] == 0


def device_records(tr):
    """a trace's searches as the primary's breakpoint records (sr_mirror_rule.h SR_BR_*: level, segment, bv bh bcomp bsf bsr,
    tie, tallies), level by level in list order"""
    out = sorted(tr.searches, key=lambda r: (r["depth"], r["pb"] + r["tb"]))
    return out, [[r["depth"], r["pb"], r["pe"], r["tb"], r["te"], r["cb"], r["ce"], r["bv"], r["bh"], r["comp"], r["score_f"], r["score_r"],
                  r["tie"], 0, 0, 0] for r in out]


@pytest.mark.parametrize("name,scores", CASES, ids=IDS)
def test_host_twin_matches_only_transposable_searches(name, scores):
    """sr_replay_match_host (the kernel's walk: sr_replay_cmp / sr_replay_same) fed the oracle's records of the primary and,
    level by level, the segments the secondary has under search: every match is an unflagged record whose transposed
    breakpoint is what the secondary's own search of that segment finds, and every search without a bit on it or above it
    is matched"""
    L = _lib.load()
    assert L.sr_replay_record_ints() == 16
    c = ti.census(name, scores)
    matched = 0
    for q, t in c.pairs:
        prim, sec = c.trace[q, t], c.trace[t, q]
        recs, flat = device_records(prim)
        arr = (C.c_int * max(1, 16 * len(flat)))(*[x for r in flat for x in r])
        want = {id(r) for r in c.transposable_searches(q, t)}
        got = set()
        for level in range(max((r["depth"] for r in sec.searches), default=-1) + 1):
            segs = sorted((r for r in sec.searches if r["depth"] == level), key=lambda r: r["pb"] + r["tb"])
            keys = [r["pb"] + r["tb"] for r in segs]
            assert keys == sorted(set(keys))                                   # strictly growing: the walk's premise
            sarr = (C.c_int * (6 * len(segs)))(*[x for r in segs for x in ti.seg_key(r)])
            out = (C.c_int * len(segs))()
            n = L.sr_replay_match_host(arr, len(flat), sarr, len(segs), level, out)
            assert n == sum(1 for x in out if x >= 0)
            for s, m in zip(segs, out):
                if m < 0:
                    continue
                r = recs[m]
                assert not r["tie"] and r["depth"] == level and ti.seg_key_t(r) == ti.seg_key(s)
                assert (s["bv"], s["bh"], s["comp"], s["score_f"], s["score_r"]) == (r["bh"], r["bv"], ti.COMP_T[r["comp"]], r["score_f"], r["score_r"]), \
                    f"{name} ({q},{t}): a replayed breakpoint is not what the secondary's search finds"
                got.add(id(r))
        assert want <= got, (name, q, t)
        matched += len(got)
    assert matched > 0 or name == "threshold_lengths"
