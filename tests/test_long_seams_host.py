"""Long sequences at the length seams of each alphabet, host side (no GPU): the seam table of DESIGN.md section 3 comes out
of long_inputs.plan(), the inputs of test_long_seams_gpu.py are what they claim to be (exact lengths, the intended symbol
width, enough divergence to exercise the recursion and little enough to keep the device runs short), and plan() agrees
with instance_matrix.dispatch wherever both answer."""
import pytest

import instance_matrix as im
import long_inputs as li
import oracle_binding as ob


# ------------------------------------------------------------------------------------------ the seam table
# the table of the issue, row by row: (bits, last length of the lower side)
TABLE = {
    "off16": {2: 32000, 4: 32000, 8: 32000},
    "ring16": {2: 57000},
    "orient": {2: 81888, 4: 40944, 8: 20472},
    "blocked": {2: 102368, 4: 51184, 8: 25592},
    "admitted": {2: 177456, 4: 88728, 8: 44364},
}


def test_seam_table_is_the_documented_one():
    got = {}
    for s in li.SEAMS:
        got.setdefault(s.name, {})[s.bits] = s.L
    assert got == TABLE


@pytest.mark.parametrize("seam", li.SEAMS, ids=lambda s: "%s-s%d" % (s.name, s.bits))
def test_exactly_the_named_field_flips(seam):
    lo, hi = li.plan(seam.L, seam.bits, knobs=seam.knobs), li.plan(seam.L + 1, seam.bits, knobs=seam.knobs)
    assert lo.refused is None
    if seam.name == "admitted":
        assert hi.refused == li.LDS_REFUSAL and hi.kernel_impl is None
        assert lo.kernel_impl == 1 and lo.words * 12 <= li.STAGE_LIMIT < hi.words * 12
        return
    flipped = {f for f in li.FLIP_FIELDS if getattr(lo, f) != getattr(hi, f)}
    assert flipped == {seam.field} | set(seam.follows), (lo, hi)
    # and the seam is a seam of the word count where the table says so
    if seam.name == "orient":
        assert (lo.orientation_route, hi.orientation_route) == ("orient-blk", "in-kernel")
        assert lo.orientation_ring_bytes > 0 and hi.orientation_ring_bytes == 0
        assert lo.words * 12 == li.ORIENT_LIMIT and hi.words == lo.words + 1
    if seam.name == "blocked":
        assert (lo.kernel_impl, hi.kernel_impl) == (2, 1)
        assert lo.words == 6400 and hi.words == 6401
        assert lo.lds_dynamic_bytes == 6400 * 16 + 16 and hi.lds_dynamic_bytes == 6401 * 12
    if seam.name == "off16":
        assert (lo.offset_bytes, hi.offset_bytes) == (2, 4)
    if seam.name == "ring16":
        assert (lo.ring_cell_bytes, hi.ring_cell_bytes, lo.offset_bytes) == (2, 4, 4)


def test_instances_at_the_window_edge():
    """the loads whose four copies end at the top of the 128 KB window: a 4-bit load at 51 184 has the 16-bit ring of
    32-bit searches, one workgroup per CU by LDS and therefore 512 threads; an 8-bit load at 25 592 int16 rows and 512
    threads; a 2-bit load at 102 368 32-bit rows and their 256-thread build"""
    p4, p8, p2 = li.plan(51184, 4), li.plan(25592, 8), li.plan(102368, 2)
    assert (p4.offset_bytes, p4.ring_cell_bytes, p4.threads_per_workgroup, p4.workgroups_per_cu) == (4, 2, 512, 1)
    assert (p8.offset_bytes, p8.ring_cell_bytes, p8.threads_per_workgroup, p8.workgroups_per_cu) == (2, 2, 512, 1)
    assert (p2.offset_bytes, p2.ring_cell_bytes, p2.threads_per_workgroup, p2.workgroups_per_cu) == (4, 4, 256, 1)
    for p in (p4, p8, p2):
        assert p.lds_dynamic_bytes + li.BLK_STATIC == li.BLK_WINDOW + 16          # the read slack lies beyond the estimate
    # SR_ALIGN_THREADS=256: the other static size at the same edge
    for L, bits in ((51184, 4), (25592, 8)):
        q = li.plan(L, bits, knobs={"SR_ALIGN_THREADS": "256"})
        assert (q.kernel_impl, q.threads_per_workgroup, q.ring_cell_bytes) == (2, 256, 2)


def test_4bit_and_8bit_never_reach_the_ring_seam():
    """the 16-bit ring of 32-bit searches ends at 57 000 symbols; 4-bit loads leave the blocked kernel at 51 184 and 8-bit
    ones at 25 592, where their offsets are still int16"""
    assert li.LAST_BLOCKED[4] < li.RING_U16_MAXLEN and li.LAST_BLOCKED[8] < li.INT16_MAXLEN
    assert li.plan(li.RING_U16_MAXLEN, 4).kernel_impl == 1 and li.plan(li.INT16_MAXLEN, 8).kernel_impl == 1


def test_row_workspace_refusal_is_out_of_reach():
    """the blocked kernel's second refusal (ring cells * cell bytes >= 4 GB per workgroup) cannot be reached below the LDS
    limit: its longest load has 102 368 symbols, rows of (4 * 102 368 + 32 * 72 + 64 + 512 + 7) & ~7 = 412 352 cells, i.e.
    1 610 + 2 pieces of 256; the ring keeps at most 80 M rows + 4 * 80 I/D rows + 10 NULL rows + 2 for any penalties the
    kernel takes (SR_BLK_MAK_SLOTS): 1 612 * 412 * 256 + 1 024 = 170 021 888 cells of at most 4 bytes = 0.68 GB"""
    brow = (4 * li.LAST_BLOCKED[2] + 32 * 72 + 64 + 512 + 7) & ~7
    cells = (brow // 256 + 2) * (im.BLK_RING_SLOTS + 4 * im.BLK_RING_SLOTS + 10 + 2) * 256 + 1024
    assert brow == 412352 and cells == 170021888 and cells * 4 < 1 << 32
    assert li.plan(li.LAST_BLOCKED[2] + 1, 2).kernel_impl == 1


# ------------------------------------------------------------------------------------------ against the other restatement
GRID = [(L, bits, npairs, knobs)
        for bits in (2, 4, 8)
        for L in (300, 2000, 5000, 9000, 19744, 20000, 32000, 32001, 40000, 57000, 57001, 60000, 81888, 102368, 102369, 120000)
        for npairs in (4, 300, 700, 4096)
        for knobs in ({}, {"SR_ALIGN_THREADS": "256"}, {"SR_ALIGN_THREADS": "512"}, {"SR_ALIGN_THREADS": "1024"},
                      {"SR_FORCE_INT32": "1"}, {"SR_FORCE_INT32": "1", "SR_RING_U16": "0", "SR_ALIGN_THREADS": "512"},
                      {"SR_ALIGN_IMPL": "1"}, {"SR_PREORIENT": "1"}, {"SR_PREORIENT": "0", "SR_ALIGN_THREADS": "256"})]


def _dispatch_window(L, bits, npairs, knobs, p):
    """the one place where the two restatements disagree.  dispatch answers up to 20 KB of copies because "the rule cannot
    apply below"; that holds for the 512- and 256-thread shapes (160 KB / 3 - 28 KB = 25.3 KB) but not for the 1 024-thread
    one, whose static tables are 34 KB: 160 KB / 3 - 34 KB = 19 797 B.  A 2-bit load with fewer pairs than CUs and
    19 797 < copies <= 20 480 bytes (19 745 .. 20 176 bases) gets two workgroups per CU and therefore 512 threads by
    plan_kernel; dispatch says 1 024.  test_long_seams_gpu.test_thread_rule_just_below_20kb_of_copies asks the device"""
    return (bits == 2 and npairs <= 256 and not {"SR_ALIGN_THREADS", "SR_FORCE_INT32"} & set(knobs) and p.kernel_impl == 2 and L <= li.INT16_MAXLEN
            and li.LDS_PER_CU // 3 - 34 * 1024 < p.lds_dynamic_bytes <= 20 * 1024)


def test_plan_agrees_with_the_dispatch_restatement():
    both = declined = window = 0
    for L, bits, npairs, knobs in GRID:
        p = li.plan(L, bits, npairs=npairs, knobs=knobs)
        if p.refused:
            continue
        try:
            d = im.dispatch(bits=bits, maxlen=L, npairs=npairs, knobs=knobs)
        except NotImplementedError:
            declined += 1
            assert p.kernel_impl == 2 and "SR_ALIGN_THREADS" not in knobs and p.lds_dynamic_bytes > 20 * 1024
            continue
        got = (p.kernel_impl, p.offset_bytes, p.ring_cell_bytes, p.threads_per_workgroup, p.orientation_route, p.symbol_bits)
        want = (d.kernel_impl, d.offset_bytes, d.ring_cell_bytes, d.threads_per_workgroup, d.orient_route, d.instance.bits)
        if _dispatch_window(L, bits, npairs, knobs, p):
            window += 1
            assert (p.threads_per_workgroup, d.threads_per_workgroup) == (512, 1024)
            got, want = got[:3] + got[4:], want[:3] + want[4:]
        both += 1
        assert got == want, (L, bits, npairs, knobs, p, d)
    assert both > 500 and declined > 100 and window >= 1


# ------------------------------------------------------------------------------------------ the inputs
def test_cases_cover_both_sides_of_every_seam():
    have = {(c.bits, c.L) for c in li.CASES}
    for s in li.SEAMS:
        assert (s.bits, s.L) in have
        assert ((s.bits, s.L + 1) in have) == (s.name != "admitted")
    for bits, L in li.LAST_BLOCKED.items():
        here = [c for c in li.CASES if (c.bits, c.L) == (bits, L)]
        assert any(c.rc for c in here) and any(c.ragged for c in here)
    assert 20 <= len(li.CASES) <= 30


@pytest.mark.parametrize("case", li.CASES, ids=lambda c: c.name)
def test_case_is_what_it_claims(case):
    recs = li.recs_of(case)
    (_, a), (_, b) = recs
    assert len(a) == case.L and len(b) == case.L - (300 if case.ragged else 0)
    assert im.symbol_bits(recs) == case.bits
    distinct = len(set(a) | set(b))
    assert distinct <= 4 if case.bits == 2 else distinct <= 16 if case.bits == 4 else distinct > 16
    if case.bits != 2:
        per_word = 32 // case.bits
        acgt = set(b"ACGT")
        for s in (a, b):
            assert set(s[:per_word]) - acgt and set(s[(len(s) - 1) // per_word * per_word:]) - acgt
    o = li.oracle_once(case.name)
    fwd = o.pairs[0, 1]
    assert fwd["is_reverse"] == case.rc
    assert 500 <= fwd["score"] <= 4000, fwd["score"]
    subs, indels = li.op_counts(fwd["cigar"])
    assert subs >= 50 and indels >= 4, (subs, indels)
    # an indel within the last 64 bases of the second member (the first columns of the alignment when it is reversed)
    assert set(fwd["cigar"][:64] if case.rc else fwd["cigar"][-64:]) & set(b"ID")
    for (q, t), al in o.pairs.items():
        cig = al["cigar"]
        qs, ts = recs[q][1], recs[t][1]
        assert cig.count(b"M") + cig.count(b"X") + cig.count(b"D") == len(qs)
        assert cig.count(b"M") + cig.count(b"X") + cig.count(b"I") == len(ts)
        pat = li.oracle_rc(qs) if al["is_reverse"] else qs
        assert ob.cigar_score(cig, pat, ts, ob.default_params().pen) == al["score"]


GENUINE = [c for c in li.CASES if not c.rc or c.L <= 26000]


@pytest.mark.parametrize("case", GENUINE, ids=lambda c: c.name)
def test_oracle_by_pieces_is_the_oracle(case):
    """the shared answers equal sro_align_pair's and sro_align_and_unite's: on every forward case, and on the
    reverse-complemented ones short enough for the unbounded forward search of sro_align_pair (about a second per pair)"""
    from mirror_inputs import OracleOnce
    recs = li.recs_of(case)
    o, g = li.oracle_once(case.name), OracleOnce(recs, {})
    keys = ("cigar", "is_reverse", "score")
    assert {k: {f: a[f] for f in keys} for k, a in g.pairs.items()} == o.pairs
    assert (o.labels == g.labels).all() and o.gfa_out == g.gfa_out
    assert any(c.rc for c in GENUINE) and any(c.rc and c.ragged for c in GENUINE)


def test_built_kernels_keep_the_window_inside_128kb():
    """the admission test of the blocked kernel counts 28 KB of static tables and no read slack; the tiles wrap their
    window addresses at 128 KB (SR_LDS_WRAP), so a two-window read in the slack behind the fourth copy of a 6 400-word load
    would land on the static tables if static tables + copies + slack passed 128 KB.  What the built instances really
    declare keeps it inside (25 312 / 28 432 / 34 672 bytes at 256 / 512 / 1 024 threads: 224 bytes to spare at 512), is
    within the host's estimates, and leaves the level kernel's three copies of the longest admitted load inside the CU"""
    from seqrush_amd import _lib
    sizes = li.built_static_lds(_lib.LIB_PATH)
    blk = {k: v for k, v in sizes.items() if k[0] == "blk" and k[1] == "wg4"}
    bfs = {k: v for k, v in sizes.items() if k[0] == "bfs"}
    assert {k[2] for k in blk} == {2, 4, 8} and {k[3] for k in blk} == {128, 256, 512, 1024}
    assert {k[2] for k in bfs} == {2, 4, 8} and {k[1] for k in bfs} == {"lvl", "wide"}
    edge = li.plan(li.LAST_BLOCKED[4], 4).lds_dynamic_bytes                  # 6 400 words: four copies + slack
    for (_, _, bits, threads), size in blk.items():
        assert size <= li.static_lds(2, threads), (bits, threads, size)
        # (the 1 024-thread build is 2-bit on int16 rows: 32 000 bases, 2 002 words at most)
        most = edge if threads < 1024 else li.plan(li.INT16_MAXLEN, 2).lds_dynamic_bytes
        assert size + most <= li.BLK_WINDOW, (bits, threads, size)
    longest = li.plan(li.FIRST_REFUSED[2] - 1, 2).lds_dynamic_bytes
    for key, size in bfs.items():
        assert size <= li.static_lds(1, key[3]) and size + longest <= li.LDS_PER_CU, (key, size)
