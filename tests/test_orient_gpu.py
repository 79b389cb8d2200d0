"""GPU tests (-m gpu) of the orientation stage against a plain DP (tests/orient_inputs.py): strand AND scores of every pair,
per route, on inputs whose forward and reverse scores F and R are equal or one apart at the levels where the kernels change
what they do -- the block boundaries 7|8, 15|16, 23|24, the level at which the reverse aligner starts and catches up, the
8-mer shortcut on, below and above its threshold, windows of two and three wave tiles, the end diagonal on every cell of a
lane and either side of a tile seam, 4-bit and 8-bit symbols, 32-bit rows, other penalties and the level kernel's ring past
its depth.

The contract (include/seqrush_amd.h, sr_ctx_orientation_scores), for a pair with reference scores (F, R):
    reverse chosen  iff R < F;   then rev == R and fwd == -1
    forward chosen:              rev == INT32_MAX and fwd == F -- except that a pair the orientation kernel decides by its
                                 bounds alone (2-bit symbols, 0,1,1,1, 8-mer sets: ub < lb) reports fwd == ub
Every comparison is of integers and bytes, exact.  The routes must also agree with each other on the alignments: orientation
must not leak into scores or CIGARs."""
import pytest

import instance_matrix as im
import orient_inputs as oi
from seqrush_amd.seqrush import Context, Params, SeqSet

pytestmark = pytest.mark.gpu

KNOBS = ("SR_PREORIENT", "SR_NO_KBITS", "SR_ORIENT_LEVELS", "SR_ALIGN_IMPL", "SR_FORCE_INT32", "SR_NO_REORDER", "SR_CIGAR_ARENA_OPS",
         "SR_NWG", "SR_NO_MIRROR", "SR_ALIGN_THREADS", "SR_BLK_LEVELS", "SR_RING_U16")


def set_env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def run_pairs(recs, pairs, ori=oi.DEFAULT_ORI, batched=False):
    """one context over an explicit pair list (environment already set) -> report, counters of the alignment stage, strands,
    orientation scores, alignment scores, raw CIGAR bytes"""
    ctx = Context(0)
    ctx.load_pairs(SeqSet(recs), Params(orientation_scores=ori), pairs)
    rep = ctx.workspace_report()
    cnt = None
    if not batched:
        ctx.align(); ctx.sync()
        cnt = ctx.counters()
    al = ctx.align_all(); ctx.sync()
    fw, rv = ctx.orientation_scores()
    assert al.n == len(pairs) and [(int(q), int(t)) for q, t in zip(al.query_idx, al.target_idx)] == list(pairs)
    out = dict(rep=rep, cnt=cnt, rev=[bool(x) for x in al.is_reverse], fw=[int(x) for x in fw], rv=[int(x) for x in rv],
               score=[int(x) for x in al.score], cigar=[al.raw_cigar_bytes(i) for i in range(al.n)], batches=ctx.num_batches)
    al.close(); ctx.close()
    return out


def check_reference(out, meta, ori=oi.DEFAULT_ORI, bound=False, what=""):
    """strand and both orientation scores of every pair against the DP; bound: the route decides ub < lb pairs by the bounds"""
    n_rev = n_cut = 0
    for i, m in enumerate(meta):
        f, r = oi.expect(m.q, m.t, ori)
        tag = f"{what} {m.name}: F {f} R {r}, device strand {out['rev'][i]} fwd {out['fw'][i]} rev {out['rv'][i]}"
        assert out["rev"][i] == (r < f), tag
        if r < f:
            assert (out["fw"][i], out["rv"][i]) == (-1, r), tag
            n_rev += 1
        elif bound and oi.shortcut(m.q, m.t):
            assert (out["fw"][i], out["rv"][i]) == (oi.ub(m.q, m.t), oi.INT32_MAX), tag
            n_cut += 1
        else:
            assert (out["fw"][i], out["rv"][i]) == (f, oi.INT32_MAX), tag
        assert out["score"][i] >= 0 and out["cigar"][i], tag
    return n_rev, n_cut


_ALIGNMENTS = {}                                         # (orientation penalties, pair name) -> (route, score, CIGAR bytes)
YARDSTICK = {"SR_PREORIENT": "0"}                        # the alignment kernel's own orientation passes, 16-bit rows
# the lists that between them hold every pair of every other list
COVER = {"lattice": ("lattice",), "rest": ("rest",), "seam-short": ("rest",), "seam-wide": ("rest",), "lattice-wide": ("lattice", "wide"),
         "alphabet4": ("alphabet4",), "alphabet8": ("alphabet8",)}


def yardstick(monkeypatch, list_name, ori):
    """once per process and penalties: the covering lists of `list_name` under the yardstick route, every pair filed under
    its name -- so that a route is held against another one's alignments even when its test runs alone"""
    for name in COVER[list_name]:
        recs, pairs, meta = oi.pair_list(name)
        if all((ori, m.name) in _ALIGNMENTS for m in meta):
            continue
        set_env(monkeypatch, YARDSTICK)
        out = run_pairs(recs, pairs, ori=ori)
        check_reference(out, meta, ori=ori, what=f"yardstick {name}")
        for i, m in enumerate(meta):
            _ALIGNMENTS.setdefault((ori, m.name), (f"yardstick ({name})", out["score"][i], out["cigar"][i]))


def check_routes_agree(meta, ori, out, what):
    """PAIR BY PAIR (by name, whatever list the pair was loaded in): alignment score and CIGAR bytes equal those of the
    yardstick route -- hence of every other route that runs the pair.  The strand, which the alignment does depend on, is
    held against the DP by check_reference"""
    for i, m in enumerate(meta):
        first = _ALIGNMENTS[ori, m.name]                   # (KeyError: yardstick() was not called for this list)
        assert out["score"][i] == first[1], f"{what} and {first[0]} disagree on the alignment score of {m.name}"
        assert out["cigar"][i] == first[2], f"{what} and {first[0]} disagree on the CIGAR of {m.name}"


def check_report(rep, route, impl, offset_bytes, bits, what):
    got = (rep["orientation_route"], rep["kernel_impl"], rep["offset_bytes"], rep["symbol_bits"])
    assert got == (route, impl, offset_bytes, bits), (what, got)
    assert rep["mirror_partners"] == 0, what


# ------------------------------------------------------------------------------------------ routes, 2-bit symbols
# id -> (environment, report: orientation_route, kernel_impl, offset_bytes; 8-mer shortcut; lists)
PRE = {"SR_PREORIENT": "1"}
I32 = {"SR_FORCE_INT32": "1"}
ROUTES = {
    "blk": (PRE, ("orient-blk", 2, 2), True, ("lattice", "rest")),
    "blk-nokbits": (dict(PRE, SR_NO_KBITS="1"), ("orient-blk", 2, 2), False, ("lattice", "rest")),
    "levels": (dict(PRE, SR_ORIENT_LEVELS="1"), ("orient-levels", 2, 2), False, ("lattice", "rest")),
    "in-kernel": ({"SR_PREORIENT": "0"}, ("in-kernel", 2, 2), False, ("lattice", "rest")),
    "bfs": ({"SR_ALIGN_IMPL": "1"}, ("in-kernel", 1, 2), False, ("lattice", "seam-short")),
    "blk-int32": (dict(PRE, **I32), ("orient-blk", 2, 4), True, ("lattice", "seam-wide")),
    "levels-int32": (dict(PRE, SR_ORIENT_LEVELS="1", **I32), ("orient-levels", 2, 4), False, ("lattice", "seam-wide")),
    "in-kernel-int32": (dict({"SR_PREORIENT": "0"}, **I32), ("in-kernel", 2, 4), False, ("lattice", "seam-wide")),
}


@pytest.mark.parametrize("route,name", [(r, n) for r in ROUTES for n in ROUTES[r][3]])
def test_route_against_the_reference(gpu, monkeypatch, route, name):
    """sr_orient_blk_kernel with and without its 8-mer bound, sr_orient_kernel, the blocked kernel's own passes (ori_pass8),
    the level kernel's search, and the int32_t instances of the first three: every 2-bit case in both pair orders"""
    env, (oroute, impl, osz), bound, _ = ROUTES[route]
    yardstick(monkeypatch, name, oi.DEFAULT_ORI)
    set_env(monkeypatch, env)
    recs, pairs, meta = oi.pair_list(name)
    out = run_pairs(recs, pairs)
    check_report(out["rep"], oroute, impl, osz, 2, route)
    assert out["batches"] == 1
    n_rev, n_cut = check_reference(out, meta, bound=bound, what=route)
    assert n_rev > 0
    assert (n_cut > 0) == bound, (route, n_cut)
    check_routes_agree(meta, oi.DEFAULT_ORI, out, route)


# ------------------------------------------------------------------------------------------ 4-bit and 8-bit symbols
@pytest.mark.parametrize("pre", ["1", "0"], ids=["orient-blk", "in-kernel"])
@pytest.mark.parametrize("bits", [4, 8])
def test_other_alphabets_against_the_reference(gpu, monkeypatch, bits, pre):
    """the builds without an 8-mer bound: N, lower case (complemented to upper case: the strands' scores differ by what the
    DP says, not by the 2-bit lattice's intent) and IUPAC codes"""
    name = f"alphabet{bits}"
    yardstick(monkeypatch, name, oi.DEFAULT_ORI)
    set_env(monkeypatch, {"SR_PREORIENT": pre})
    recs, pairs, meta = oi.pair_list(name)
    out = run_pairs(recs, pairs)
    check_report(out["rep"], "orient-blk" if pre == "1" else "in-kernel", 2, 2, bits, name)
    n_rev, n_cut = check_reference(out, meta, what=f"{name} SR_PREORIENT={pre}")
    assert n_rev > 0 and n_cut == 0
    check_routes_agree(meta, oi.DEFAULT_ORI, out, f"{name} SR_PREORIENT={pre}")


# ------------------------------------------------------------------------------------------ other orientation penalties
@pytest.mark.parametrize("pre", ["1", "0"], ids=["orient-kernel", "in-kernel"])
@pytest.mark.parametrize("ori", oi.OTHER_ORI)
def test_other_penalties_against_the_reference(gpu, monkeypatch, ori, pre):
    """the DP run with the same penalties: 0,2,3,1 (level-by-level orientation kernel / blk_pass in-kernel), 0,1,2,2 (no
    blocked alignment kernel: the level kernel orients) and 0,1,76,1 (the deepest ring that fits: 79 rows, every wide score
    beyond it)"""
    env = {"SR_PREORIENT": pre}
    yardstick(monkeypatch, "lattice-wide", ori)
    set_env(monkeypatch, env)
    recs, pairs, meta = oi.pair_list("lattice-wide")
    d = im.dispatch(ori_scores=ori, maxlen=max(len(s) for _, s in recs), npairs=len(pairs), knobs=env)
    if ori == "0,1,76,1" and pre == "1":
        assert d.orient_route == "orient-levels"
    if ori == "0,1,2,2":
        assert (d.orient_route, d.kernel_impl) == ("in-kernel", 1)
    out = run_pairs(recs, pairs, ori=ori)
    check_report(out["rep"], d.orient_route, d.kernel_impl, 2, 2, (ori, pre))
    n_rev, n_cut = check_reference(out, meta, ori=ori, what=f"{ori} SR_PREORIENT={pre}")
    assert n_rev > 0 and n_cut == 0
    check_routes_agree(meta, ori, out, f"{ori} SR_PREORIENT={pre}")


# ------------------------------------------------------------------------------------------ shortcut accounting
def orientation_cells(monkeypatch, env, recs, pairs, meta, bound):
    set_env(monkeypatch, env)
    out = run_pairs(recs, pairs)
    check_report(out["rep"], "orient-blk", 2, 2, 2, env)
    check_reference(out, meta, bound=bound, what=str(env))
    return out["cnt"]["ticks_orientation"]


def test_decided_pairs_run_no_aligner(gpu, monkeypatch):
    """a list made only of pairs with ub < lb counts no orientation cells; without the 8-mer sets it does"""
    recs, pairs, meta = oi.pair_list("lattice")
    keep = [i for i, m in enumerate(meta) if oi.shortcut(m.q, m.t)]
    assert len(keep) >= 20 and len(keep) < len(meta)
    sub_pairs, sub_meta = [pairs[i] for i in keep], [meta[i] for i in keep]
    assert orientation_cells(monkeypatch, PRE, recs, sub_pairs, sub_meta, True) == 0
    assert orientation_cells(monkeypatch, dict(PRE, SR_NO_KBITS="1"), recs, sub_pairs, sub_meta, False) > 0


@pytest.mark.parametrize("kind", ["below", "at", "above"])
def test_threshold_pairs_one_at_a_time(gpu, monkeypatch, kind):
    """ub = lb - 1 is decided by the bounds; ub = lb and ub = lb + 1 are not (the shortcut is `ub < lb`) and run an aligner;
    SR_NO_KBITS=1 always does"""
    for name in oi.threshold_names()[kind]:
        recs, pairs, meta = oi.single(name)
        cells = orientation_cells(monkeypatch, PRE, recs, pairs, meta, True)
        assert (cells == 0) == (kind == "below"), (name, cells)
        assert orientation_cells(monkeypatch, dict(PRE, SR_NO_KBITS="1"), recs, pairs, meta, False) > 0, name


def test_late_reverse_start_saves_cells(gpu, monkeypatch):
    """spacing 3, F >= 15: lb (7 .. 13) is far below R: the reverse aligner starts in block 0 or block 8, one or two blocks
    before either aligner can finish, and runs most of the way in lockstep -- never more cells than both from level 0.
    (Catch-up next to a tie is what the spacing-9 cells of the route tests run: there lb = R = 15, 16, 17, 23, 24, 25 and
    the reverse aligner starts in the very block that decides.)"""
    recs, pairs, meta = oi.pair_list("lattice")
    keep = [i for i, m in enumerate(meta) if "-s3-" in m.name and int(m.name.split("-F")[1].split("-")[0]) >= 15]
    assert len(keep) == 2 * 18
    sub_pairs, sub_meta = [pairs[i] for i in keep], [meta[i] for i in keep]
    assert not any(oi.shortcut(m.q, m.t) for m in sub_meta)
    with_bound = orientation_cells(monkeypatch, PRE, recs, sub_pairs, sub_meta, True)
    without = orientation_cells(monkeypatch, dict(PRE, SR_NO_KBITS="1"), recs, sub_pairs, sub_meta, False)
    assert 0 < with_bound <= without, (with_bound, without)


# ------------------------------------------------------------------------------------------ dequeue order
def test_dequeue_order_changes_nothing(gpu, monkeypatch):
    """sr_order.hip sorts every batch's queue by the orientation scores (for a decided pair: the upper bound): the block
    lattice in at least three batches, sorted and with SR_NO_REORDER=1 in list order -- identical strands, orientation scores,
    scores and CIGARs, all equal to the reference"""
    yardstick(monkeypatch, "lattice", oi.DEFAULT_ORI)
    recs, pairs, meta = oi.pair_list("lattice")
    arena = str(45 * (2 * max(len(s) for _, s in recs) + 2))
    outs = []
    for extra in ({}, {"SR_NO_REORDER": "1"}):
        set_env(monkeypatch, dict(PRE, SR_CIGAR_ARENA_OPS=arena, **extra))
        out = run_pairs(recs, pairs, batched=True)
        check_report(out["rep"], "orient-blk", 2, 2, 2, extra)
        assert out["rep"]["batches"] >= 3 and out["batches"] == out["rep"]["batches"], out["rep"]
        assert ("SR_NO_REORDER" in out["rep"]["knobs"]) == bool(extra)
        check_reference(out, meta, bound=True, what=f"batched {extra}")
        check_routes_agree(meta, oi.DEFAULT_ORI, out, f"batched {extra}")
        outs.append(out)
    for k in ("rev", "fw", "rv", "score", "cigar"):
        assert outs[0][k] == outs[1][k], k
