"""GPU tests (-m gpu) of the modes on inputs that have ties, with mirroring active: --iterative,
--patch-inversions under the plain and the joined rule, sparsified and sharded lists, and what sits downstream (kept
alignments, PAF output and reload, both command lines, the sorted and compacted GFA).  Every load goes through load_device
and enqueue_align_batch, so a secondary of these runs is the transposed CIGAR of its primary, was aligned by its primary's
workgroup after a tie, deferred to the wide tail launch or replayed from its primary's records -- and the mode's own kernels
(sr_iter_unite_kernel behind the stop flag, sr_inv_scan_kernel in both instances, the patch pass, the shard deal) read what
another pair's workgroup or a second launch wrote.

Every case runs three ways under the same knobs -- mirroring on, SR_MIRROR_REPLAY=0, SR_NO_MIRROR=1 -- against the mode's
oracle restatement and against each other, bit for bit wherever the mode's own suite compares bit for bit, the oracle-counted
counters included.  Inputs, lists and batch layouts: tests/mode_tie_inputs.py; the partners every list has and the conditions
that keep a case from being vacuous are computed and pinned on the CPU (test_modes_mirrored_host.py) and asserted here on the
"on" run.  The inputs have 9 to 924 pairs: SR_NWG (2 or 8) stays below the pairs of a batch, without which a launch this small
has no partners at all, and the main launch is pinned to the production shape (SR_ALIGN_THREADS=256), without which there is
nothing wider for a tail launch."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import inversion_helpers as ih
import mirror_inputs as mi
import mode_tie_inputs as mt
import oracle_binding as ob
import test_inversion_join_gpu as tj
import test_inversions_gpu as tv
import test_mirror_gpu as tm
import test_modes_mirrored_host as th
import test_tail_launch as tl
import tie_inputs as ti
from seqrush_amd import seqrush as sr
from seqrush_amd.seqrush import Context, Params, SeqSet, build_gfa
from conftest import canon_gfa
from test_gpu_parity import oracle_params

pytestmark = pytest.mark.gpu

ROOT = tm.ROOT
EXE = os.path.join(ROOT, "seqrush_amd", "seqrush_mi355x")
ALL_KNOBS = tm.KNOBS + tl.TAIL_KNOBS + ("SR_MIRROR_REPLAY",)
MAIN256 = tl.MAIN256
WAYS = (("on", {}), ("no-replay", {"SR_MIRROR_REPLAY": "0"}), ("no-mirror", {"SR_NO_MIRROR": "1"}))


class Env:
    """the two monkeypatch calls the helpers use, on os.environ (the bounds children have no monkeypatch)"""
    @staticmethod
    def delenv(k, raising=False):
        os.environ.pop(k, None)

    @staticmethod
    def setenv(k, v):
        os.environ[k] = v


def set_env(mp, env):
    for k in ALL_KNOBS:
        mp.delenv(k, raising=False)
    for k, v in env.items():
        mp.setenv(k, v)


def three_ways(mp, env, run):
    """run() under env with mirroring on, without the replay and without mirroring -> {way: result}"""
    out = {}
    for way, extra in WAYS:
        set_env(mp, dict(MAIN256, **env, **extra))
        out[way] = run()
    set_env(mp, {})
    assert out["no-mirror"]["rep"]["mirror_partners"] == 0 and out["no-replay"]["rep"]["mirror_replay"] == 0
    for way in ("no-replay", "no-mirror"):
        c = out[way]["cnt"]
        assert c["mirror_replays"] == 0 and c["replay_cached_searches"] == 0
    assert out["no-mirror"]["cnt"]["mirror_pairs"] == 0 and out["no-mirror"]["cnt"]["mirror_ties"] == 0 and out["no-mirror"]["deferred"] == 0
    for k in tm.ORACLE_COUNTED:
        assert out["on"]["cnt"][k] == out["no-replay"]["cnt"][k] == out["no-mirror"]["cnt"][k], k
    for k in ("mirror_pairs", "mirror_ties", "mirror_tie_top", "mirror_tie_base_only"):     # where the ties sit does not depend on the replay
        assert out["on"]["cnt"][k] == out["no-replay"]["cnt"][k], k
    return out


def mirrored(case, r, layout, batches_ran, nwg, nt_ran, deep_ran, tail):
    """the non-vacuity of an "on" run: partners as the host file says, every one of them emitted or tied, the ties at least
    the pairs the oracle cannot transpose, a replay where the census has a tied primary with an unflagged depth-0 search.
    batches_ran: how many batches of the layout the run enqueued; nt_ran, deep_ran: partnered unordered pairs among them that
    are non-transposable / replay candidates; tail: the SR_TAIL of the case (None: the default rule)"""
    per_batch = th.partners(layout, nwg)
    cnt, rep = r["cnt"], r["rep"]
    print(case, layout, "workgroups", rep["workgroups"], "mirror_partners", rep["mirror_partners"], "ran", sum(per_batch[:batches_ran]),
          "mirror_pairs", cnt["mirror_pairs"], "mirror_ties", cnt["mirror_ties"], "non-transposable", nt_ran, "tail_deferred", r["deferred"],
          "mirror_replays", cnt["mirror_replays"], "replay candidates", deep_ran, "cached searches", cnt["replay_cached_searches"])
    assert rep["workgroups"] == nwg and rep["threads_per_workgroup"] == 256 and rep["symbol_bits"] == 2
    assert rep["batches"] == len(per_batch) and rep["mirror_partners"] == sum(per_batch) > 0
    ran = sum(per_batch[:batches_ran])
    assert cnt["mirror_pairs"] + cnt["mirror_ties"] == ran
    assert cnt["mirror_ties"] >= nt_ran and cnt["mirror_pairs"] <= ran - nt_ran
    if tail == "all":
        assert rep["tail_threads"] == 1024 and r["deferred"] == cnt["mirror_ties"] and cnt["mirror_replays"] == 0
    elif tail == "0":
        assert rep["tail_threads"] == 0 and r["deferred"] == 0
    else:
        assert rep["tail_threads"] == 1024 and 0 <= r["deferred"] <= cnt["mirror_ties"]
    if tail != "all":
        assert rep["mirror_replay"] == 1 and cnt["mirror_replays"] <= cnt["mirror_ties"]
        if deep_ran:
            assert cnt["mirror_replays"] >= 1 and cnt["replay_cached_searches"] >= 1


# --------------------------------------------------------------------------------------------- 1. iterative
ITER_STATS = ("tree_entries", "random_entries", "random_processed", "random_aligned", "checks", "windows", "post_tree",
              "final_components", "stabilized", "check_counts", "pairs")


def iter_run(name, keep=True):
    recs = list(mt.records(name))
    ss, ctx = SeqSet(recs), Context(0)
    p = Params(sparsification=mt.ITER_SPEC if name == "iter_ties" else mt.NEVER_SPEC)
    p.c.min_match_len = mt.ITER_K
    ctx.load_iterative(ss, p, keep_alignments=keep)
    rep = ctx.workspace_report()
    ctx.run_iterative()
    ctx.sync()
    st = ctx.iterative_stats()
    st["pairs"] = ctx.pairs()
    out = dict(st=st, rep=rep, cnt=ctx.counters(), deferred=ctx.tail_deferred(), labels=ctx.download_labels(),
               gfa=ctx.build_gfa(compact=False)[0], kernel=ctx.align_kernel)
    if keep:
        al = ctx.iterative_alignments()
        out["al"] = [(int(al.query_idx[i]), int(al.target_idx[i]), bool(al.is_reverse[i]), int(al.score[i]), al.raw_cigar_bytes(i))
                     for i in range(al.n)]
        al.close()
    ctx.close()
    return out


def iter_check(r, name):
    """what test_iterative_gpu.check_case asserts, against the same restatement, plus the kept alignments"""
    ref, o, st = mt.iter_restated(name), mt.iter_oracle(name), r["st"]
    assert r["kernel"] == "sr_align_blk_kernel"
    assert (st["tree_entries"], st["random_entries"]) == (len(ref["tree"]), len(ref["random"]))
    assert st["pairs"] == mt.iter_list(name)
    assert st["post_tree"] == ref["post_tree"]
    assert st["check_counts"] == ref["check_counts"] and st["checks"] == len(ref["check_counts"])
    assert st["stabilized"] == ref["stabilized"] and st["random_processed"] == ref["processed"]
    assert st["final_components"] == ref["final"]
    assert st["random_processed"] <= st["random_aligned"] <= st["random_entries"]
    assert np.array_equal(r["labels"], ref["labels"])
    assert canon_gfa(r["gfa"]) == canon_gfa(ref["gfa"])
    # the processed prefix, in processing order, pair by pair what the oracle gives
    m = 4 * (st["tree_entries"] + st["random_processed"])
    assert [(q, t) for q, t, _, _, _ in r["al"]] == st["pairs"][:m]
    for q, t, rev, score, cigar in r["al"]:
        oa = o.pairs[q, t]
        assert (rev, score) == (oa["is_reverse"], oa["score"]), (q, t)
        assert cigar == oa["cigar"], f"kept CIGAR differs from the oracle's on pair ({q},{t})"


def iter_case(mp, name, how, nwg, tail, env=None):
    env = dict(env or {}, SR_NWG=str(nwg))
    if tail is not None:
        env["SR_TAIL"] = tail
    if how == "chunk":
        env["SR_CIGAR_ARENA_OPS"] = "1"                      # raised to one chunk: every window is one chunk
    out = three_ways(mp, env, lambda: iter_run(name))
    for way, r in out.items():
        iter_check(r, name)
        for k in ITER_STATS:
            assert r["st"][k] == out["on"]["st"][k], (way, k)
        assert np.array_equal(r["labels"], out["on"]["labels"]) and r["gfa"] == out["on"]["gfa"] and r["al"] == out["on"]["al"], way
    on, ref = out["on"], mt.iter_restated(name)
    first, ran = mt.iter_windows(name, how), mt.windows_that_ran(name, how)
    tb = mt.tree_batches(name, how)
    assert on["st"]["windows"] == ran - tb and on["st"]["random_aligned"] == (first[ran] - first[tb]) // 4
    entries = ref["tree"] + ref["random"][:on["st"]["random_aligned"]]          # every one of them is a primary / secondary pair
    nt, deep = set(mt.iter_oracle(name).non_transposable()), set(mt.census(name).deep_tie_pairs())
    mirrored(f"iterative {name} SR_TAIL={tail}", on, f"{name}/{how}", ran, nwg, sum(e in nt for e in entries),
             sum(e in deep for e in entries), tail)
    assert on["cnt"]["mirror_pairs"] >= 1 and on["cnt"]["mirror_ties"] >= 1
    return out


@pytest.mark.parametrize("how,nwg", [("planned", 2), ("chunk", 8)])
@pytest.mark.parametrize("tail", [None, "all", "0"])
def test_iterative(gpu, monkeypatch, tail, how, nwg):
    """windows as planned (100 entries, then the rest: the stop falls into the second) on two workgroups, and one chunk per
    window on eight (40 pairs a launch: within the default tail rule)"""
    out = iter_case(monkeypatch, "iter_ties", how, nwg, tail)
    on = out["on"]
    st = on["st"]
    assert st["stabilized"] and st["random_processed"] < st["random_entries"] and len(set(st["check_counts"])) > 1
    assert st["windows"] == (2 if how == "planned" else 18)
    if tail == "all":
        assert on["deferred"] == on["cnt"]["mirror_ties"] > 0
    # the union-find holds exactly the processed alignments: the labels of an explicit list over the processed prefix
    set_env(monkeypatch, dict(MAIN256, SR_NWG=str(nwg)))
    m = 4 * (st["tree_entries"] + st["random_processed"])
    ctx = Context(0)
    ctx.load_pairs(SeqSet(list(mt.records("iter_ties"))), Params(), st["pairs"][:m])
    ctx.run(); ctx.sync()
    assert np.array_equal(ctx.download_labels(), on["labels"])
    ctx.close()


def test_iterative_never_stabilizing_equals_the_plain_tree_run(gpu, monkeypatch):
    out = iter_case(monkeypatch, "iter_never", "planned", 2, None)
    st = out["on"]["st"]
    assert not st["stabilized"] and st["random_processed"] == st["random_entries"]
    set_env(monkeypatch, dict(MAIN256, SR_NWG="2"))
    ctx = Context(0)
    ctx.load(SeqSet(list(mt.records("iter_never"))), Params(sparsification=mt.NEVER_SPEC))
    assert ctx.workspace_report()["mirror_partners"] > 0
    ctx.run(); ctx.sync()
    assert np.array_equal(ctx.download_labels(), out["on"]["labels"]) and ctx.build_gfa(compact=False)[0] == out["on"]["gfa"]
    ctx.close()


# --------------------------------------------------------------------------------------------- 2. and 3. inversions
INV_SAME = ("jobs", "cigars", "al", "pairs", "batches", "gfa", "gfa_compact")
INV_STATS = ("scanned", "sites", "candidates", "accepted", "rejected_score", "rejected_divergence", "united_bases", "patch_batches")


@pytest.fixture(scope="module")
def inv_census():
    """name -> (unordered pairs that are non-transposable or on the reverse strand, replay candidates) of an inversion input"""
    memo = {}

    def get(name, d=None):
        if (name, d) not in memo:
            if name == mt.INV_NAME:
                o, deep = mt.oracle_once(name, (("min_match_len", ih.K),)), set(mt.census(name).deep_tie_pairs())
            else:
                kw = {"min_match_len": ih.K}
                if d is not None:
                    kw["max_divergence"] = d
                o, deep = mi.OracleOnce(list(ih.inputs(name)), kw), set()
            rev = {(min(q, t), max(q, t)) for q, t in o.reverse_pairs()}
            memo[name, d] = (set(o.non_transposable()) | rev, deep)
        return memo[name, d]
    return get


def inv_case(mp, census, name, env, check, layout=None, tail=None, **kw):
    """check: test_inversions_gpu.check_against_restatement or the joined one"""
    nwg = int(env["SR_NWG"])
    out = three_ways(mp, env, lambda: check(name, **kw)[0])
    on = out["on"]
    for way, r in out.items():
        for k in INV_SAME:
            assert r.get(k) == on.get(k), (way, k)
        for k in INV_STATS:
            assert r["stats"][k] == on["stats"][k], (way, k)
        assert np.array_equal(r["labels"], on["labels"]), way
        if "join_stats" in on:
            assert [r["join_stats"][k] for k in ("islands_absorbed", "rejected_site_cost")] == [on["join_stats"][k] for k in ("islands_absorbed", "rejected_site_cost")], way
    layout = layout or name + "/main"
    pairs, first = th.layouts()[layout]
    assert on["pairs"] == pairs
    tied, deep = census(name, kw.get("d"))
    entries, _ = mt.mirror_rule(pairs, first, nwg)
    prim = [pairs[i] for i, e in enumerate(entries) if e != mt.NONE and not e & mt.SECONDARY]
    mirrored(f"inversions {name} {kw}", on, layout, len(first) - 1, nwg, sum(p in tied for p in prim), sum(p in deep for p in prim), tail)
    return out


@pytest.mark.parametrize("tail", [None, "all"])
def test_inversions_plain_rule(gpu, monkeypatch, inv_census, tail):
    """the scan walks transposed CIGARs, CIGARs of the fallback, of the replay and (SR_TAIL=all) of the tail launch"""
    env = {"SR_NWG": "2"} if tail is None else {"SR_NWG": "2", "SR_TAIL": tail}
    out = inv_case(monkeypatch, inv_census, mt.INV_NAME, env, tv.check_against_restatement, tail=tail)
    on = out["on"]
    assert on["stats"]["accepted"] == th.PINNED_INV["accepted"] and on["stats"]["rejected_score"] == th.PINNED_INV["rejected"]
    assert on["cnt"]["mirror_pairs"] >= 1 and on["cnt"]["mirror_ties"] >= th.PINNED_INV["non_transposable"]
    if tail == "all":
        assert on["deferred"] > 0


@pytest.mark.parametrize("name,d", [("inv", None), ("pinv", None), ("rejected", None), ("ratio", None), ("diverged", 0.1)])
@pytest.mark.parametrize("tail", [None, "all"])
def test_inversions_plain_rule_on_the_mode_suites_inputs(gpu, monkeypatch, inv_census, name, d, tail):
    """3 sequences, 9 pairs, 3 partners on two workgroups; C of inv and pinv is reverse-complemented: its secondaries are
    aligned after their primaries on the reverse strand.  (inv, pinv and rejected emit nothing by symmetry: each of their
    three pairs is on the reverse strand or has the two-sided gap, whose I-before-D order is itself a tie; ratio and
    diverged emit one.  mirror_pairs >= 1 is asserted where the oracle has a transposable pair to spare: on inv_ties.)"""
    env = {"SR_NWG": "2"} if tail is None else {"SR_NWG": "2", "SR_TAIL": tail}
    kw = {} if d is None else {"d": d}
    inv_case(monkeypatch, inv_census, name, env, tv.check_against_restatement, tail=tail, **kw)


@pytest.mark.parametrize("via_align_all", [False, True])
def test_inversions_forced_batches(gpu, monkeypatch, inv_census, via_align_all):
    """three batches share the arena one after the other: the scan of a batch reads what that batch's launches wrote"""
    one = tv.check_against_restatement(mt.INV_NAME)[0] if not via_align_all else None
    env = {"SR_NWG": "2", "SR_CIGAR_ARENA_OPS": str(th.inv_arena_ops())}
    out = inv_case(monkeypatch, inv_census, mt.INV_NAME, env, tv.check_against_restatement, layout="inv_ties/batches",
                   via_align_all=via_align_all)
    assert out["on"]["batches"] == 3
    if one is not None:
        assert out["on"]["jobs"] == one["jobs"] and out["on"]["cigars"] == one["cigars"] and np.array_equal(out["on"]["labels"], one["labels"])
    out = inv_case(monkeypatch, inv_census, mt.INV_NAME, dict(env, SR_TAIL="all"), tv.check_against_restatement,
                   layout="inv_ties/batches", tail="all", via_align_all=via_align_all)
    assert out["on"]["deferred"] > 0


@pytest.mark.parametrize("tail", [None, "all"])
def test_inversions_joined_rule(gpu, monkeypatch, inv_census, tail):
    """site costs are sums over the ops of a CIGAR that its primary transposed or the tail launch wrote"""
    env = {"SR_NWG": "2"} if tail is None else {"SR_NWG": "2", "SR_TAIL": tail}
    out = inv_case(monkeypatch, inv_census, mt.INV_NAME, env, tj.check_against_restatement, tail=tail, join=8)
    on = out["on"]
    assert (on["stats"]["candidates"], on["stats"]["accepted"]) == (th.PINNED_INV["joined_jobs"], th.PINNED_INV["joined_accepted"])
    assert on["join_stats"]["islands_absorbed"] == th.PINNED_INV["joined_islands"] >= 1
    assert on["cnt"]["mirror_pairs"] >= 1
    if tail == "all":
        assert on["deferred"] > 0


# --------------------------------------------------------------------------------------------- 4. sparsified list and shards
@pytest.fixture(scope="module")
def sparse_oracle():
    """family -> (OracleOnce of the family, labels and GFA of the oracle over the sparsified list)"""
    memo = {}

    def get(fam):
        if fam not in memo:
            once = mi.oracle_once("A") if fam == "A" else ti.oracle_once(fam)
            o = ob.OracleSeqRush(records=list(mt.records("sparse:" + fam)))
            o.align_and_unite_list(oracle_params(), list(mt.sparse_list(fam)))
            memo[fam] = (once, o.canonical_labels(), o.gfa(canonical=True))
            o.close()
        return memo[fam]
    return get


def sparse_run(fam, shard=(0, 1)):
    ss, ctx = SeqSet(list(mt.records("sparse:" + fam))), Context(0)
    p = Params(sparsification=mt.SPARSE_SPEC)
    p.c.shard_rank, p.c.shard_count = shard
    ctx.load(ss, p)
    rep = ctx.workspace_report()
    ctx.run(); ctx.sync()
    al = ctx.alignments()
    out = dict(rep=rep, cnt=ctx.counters(), deferred=ctx.tail_deferred(), labels=ctx.download_labels(), pairs=ctx.pairs(),
               al=[(int(al.query_idx[i]), int(al.target_idx[i]), bool(al.is_reverse[i]), int(al.score[i]), al.raw_cigar_bytes(i), al.cigar(i))
                   for i in range(al.n)], ss=ss)
    al.close(); ctx.close()
    return out


def sparse_case(mp, fam, layout, shard, once):
    out = three_ways_or_plain(mp, {"SR_NWG": "2"}, lambda: sparse_run(fam, shard), sum(th.PARTNERS[layout]) > 0)
    pairs, first = th.layouts()[layout]
    for way, r in out.items():
        assert r["pairs"] == pairs, way
        assert [(q, t) for q, t, *_ in r["al"]] == pairs
        for q, t, rev, score, cigar, text in r["al"]:               # test_gpu_parity.check_parity's comparisons, per pair
            oa = once.pairs[q, t]
            assert cigar == oa["cigar"], f"{way}: CIGAR differs on pair ({q},{t})"
            assert (rev, score, text) == (oa["is_reverse"], oa["score"], ob.cigar_bytes_to_string(oa["cigar"])), (way, q, t)
        assert np.array_equal(r["labels"], out["on"]["labels"]), way
    return out


def three_ways_or_plain(mp, env, run, has_partners):
    """three_ways() -- or, for a list on which no pair has a partner, the one run there is"""
    if has_partners:
        return three_ways(mp, env, run)
    set_env(mp, dict(MAIN256, **env))
    out = {"on": run()}
    set_env(mp, {})
    r = out["on"]
    assert r["rep"]["mirror_partners"] == 0 and r["rep"]["tail_threads"] == 0 and r["deferred"] == 0
    assert r["cnt"]["mirror_pairs"] == 0 and r["cnt"]["mirror_ties"] == 0 and r["cnt"]["mirror_replays"] == 0
    return out


def partnered(fam, layout, once):
    pairs, first = th.layouts()[layout]
    entries, _ = mt.mirror_rule(pairs, first, 2)
    prim = [pairs[i] for i, e in enumerate(entries) if e != mt.NONE and not e & mt.SECONDARY]
    nt = set(once.non_transposable())
    deep = set(ti.census(fam).deep_tie_pairs()) if fam != "A" else set()
    return sum(p in nt for p in prim), sum(p in deep for p in prim)


@pytest.mark.parametrize("fam", sorted(mt.SPARSE))
def test_sparsified_list(gpu, monkeypatch, sparse_oracle, fam):
    once, labels, gfa = sparse_oracle(fam)
    layout = f"sparse:{fam}/whole"
    out = sparse_case(monkeypatch, fam, layout, (0, 1), once)
    on = out["on"]
    assert np.array_equal(on["labels"], labels), "UF partition differs"
    g = build_gfa(on["ss"], on["labels"])
    assert canon_gfa(g[0]) == canon_gfa(gfa[0]) and g[1:] == gfa[1:]
    nt, deep = partnered(fam, layout, once)
    mirrored(f"sparsified {fam}", on, layout, 1, 2, nt, deep, None)
    assert on["cnt"]["mirror_pairs"] >= 1 and on["cnt"]["mirror_ties"] >= 1


@pytest.mark.parametrize("fam", sorted(mt.SPARSE))
def test_two_shards(gpu, monkeypatch, sparse_oracle, fam):
    """the deal sends (q, t) and (t, q) where the loads say: a pair that lost its partner to the other rank is aligned on its
    own, both ways, and the merged labels are the unsharded partition"""
    once, labels, _ = sparse_oracle(fam)
    lost = mt.lost_partners(fam)
    assert len(lost) == th.PINNED_SPARSE[fam][3] >= 1
    parts = []
    for r in (0, 1):
        layout = f"sparse:{fam}/shard{r}"
        out = sparse_case(monkeypatch, fam, layout, (r, 2), once)
        on = out["on"]
        assert on["rep"]["mirror_partners"] == sum(th.PARTNERS[layout])
        if sum(th.PARTNERS[layout]):
            nt, deep = partnered(fam, layout, once)
            mirrored(f"shard {r} of {fam}", on, layout, 1, 2, nt, deep, None)
        for q, t in lost:                                          # both orders were aligned, each on its rank
            assert ((q, t) in on["pairs"]) != ((t, q) in on["pairs"])
        parts.append(on)
    if fam == "unequal_blocks_400":
        assert all(p["rep"]["mirror_partners"] == 3 for p in parts) and sum(p["cnt"]["mirror_ties"] for p in parts) >= 2
    set_env(monkeypatch, {})
    ctx = Context(0)
    ctx.load_pairs(parts[0]["ss"], Params(), [])
    lab = np.ascontiguousarray(np.concatenate([p["labels"] for p in parts]), dtype=np.uint64)
    sr.check(ctx.L.sr_ctx_merge_labels_host(ctx._h, lab.ctypes.data_as(C.POINTER(C.c_uint64)), 2))
    ctx.sync()
    assert np.array_equal(ctx.download_labels(), labels)
    ctx.close()


# --------------------------------------------------------------------------------------------- 5. downstream bytes
CLI = {
    "iterative": ("iter_ties", ["--iterative", "-x", mt.ITER_SPEC]),
    "inversions": (mt.INV_NAME, ["-k", str(ih.K), "--patch-inversions", "--inversion-join", "8"]),
}


def cli_run(which, fa, tmp, tag, args, env):
    gfa, paf = tmp / f"{tag}.gfa", tmp / f"{tag}.paf"
    cmd = [sys.executable, "-m", "seqrush_amd"] if which == "python" else [EXE]
    base = {k: v for k, v in os.environ.items() if k not in ALL_KNOBS}
    r = subprocess.run(cmd + ["-s", fa, "-o", str(gfa)] + args + ["--output-alignments", str(paf)], capture_output=True, text=True,
                       env=dict(base, PYTHONPATH=ROOT, **MAIN256, **env), cwd=str(tmp), timeout=300)
    assert r.returncode == 0, (tag, r.stderr[-1500:])
    return gfa.read_bytes(), paf.read_bytes()


@pytest.mark.parametrize("mode", sorted(CLI))
def test_command_lines_give_the_same_bytes_with_and_without_mirroring(gpu, tmp_path, mode):
    name, args = CLI[mode]
    fa = write_fasta(tmp_path / "in.fa", mt.records(name))
    on = cli_run("native", fa, tmp_path, "on", args + ["--no-sort"], {"SR_NWG": "2"})
    off = cli_run("native", fa, tmp_path, "off", args + ["--no-sort"], {"SR_NWG": "2", "SR_NO_MIRROR": "1"})
    py = cli_run("python", fa, tmp_path, "py", args + ["--no-sort"], {"SR_NWG": "2"})
    assert on == off, "GFA or PAF differs between mirroring on and SR_NO_MIRROR=1"
    assert on == py, "GFA or PAF differs between the two command lines"
    lines = on[1].decode().strip().split("\n")
    if mode == "iterative":
        c = th.PINNED_ITER
        assert len(lines) == 4 * (c["tree"] + c["processed"])
    else:
        c = th.PINNED_INV
        assert len(lines) == 25 + c["joined_accepted"] and sum("sr:Z:inv" in x for x in lines) == c["joined_accepted"]
    # the PAF reloads to the same labels: the graph of -p is the graph of the run
    again = tmp_path / "again.gfa"
    k = ["-k", str(ih.K)] if mode == "inversions" else []
    r = subprocess.run([EXE, "-s", fa, "-o", str(again), "--no-sort", "-p", str(tmp_path / "on.paf")] + k, capture_output=True,
                       text=True, cwd=str(tmp_path), timeout=300)
    assert r.returncode == 0, r.stderr[-1500:]
    assert canon_gfa(again.read_text()) == canon_gfa(on[0].decode())


def test_sorted_graph_compacted_on_the_device(gpu, tmp_path):
    """--sort --compact-on device downstream of mirrored records: the same bytes from both command lines, on and off"""
    name, args = CLI["inversions"]
    fa = write_fasta(tmp_path / "in.fa", mt.records(name))
    args = args + ["--sort", "--compact-on", "device"]
    on = cli_run("native", fa, tmp_path, "on", args, {"SR_NWG": "2"})
    off = cli_run("native", fa, tmp_path, "off", args, {"SR_NWG": "2", "SR_NO_MIRROR": "1"})
    py = cli_run("python", fa, tmp_path, "py", args, {"SR_NWG": "2"})
    assert on == off and on == py


def write_fasta(path, recs):
    path.write_bytes(b"".join(b">" + n.encode() + b"\n" + s + b"\n" for n, s in recs))
    return str(path)


# --------------------------------------------------------------------------------------------- 6. bounds-checked build
def bounds_child(mode):
    """(child process, SEQRUSH_AMD_LIB = the bounds-checked library) one mode on two workgroups, every tie through the tail
    launch: the equalities of the mode's case, the bounds-checked instance, no access outside a workgroup's extent"""
    if mode == "iterative":
        out = iter_case(Env, "iter_ties", "planned", 2, "all")
    else:
        memo = {}

        def census(name, d=None):
            if name not in memo:
                o = mt.oracle_once(name, (("min_match_len", ih.K),))
                memo[name] = (set(o.non_transposable()), set(mt.census(name).deep_tie_pairs()))
            return memo[name]
        out = inv_case(Env, census, mt.INV_NAME, {"SR_NWG": "2", "SR_TAIL": "all"}, tj.check_against_restatement, tail="all", join=8)
    for way, r in out.items():
        assert r["rep"]["kernel_build"] == "bounds", way
        assert r["cnt"]["bounds_first"][0] == 0, (way, r["cnt"]["bounds_first"])
    assert out["on"]["deferred"] == out["on"]["cnt"]["mirror_ties"] > 0 and out["on"]["cnt"]["mirror_pairs"] >= 1
    print("bounds build clean:", mode)


@pytest.mark.parametrize("mode", ["iterative", "inversions"])
def test_bounds_checked_build(gpu, mode):
    """A subprocess, because the library is chosen at load time"""
    lib = os.path.join(ROOT, "seqrush_amd", "libseqrush_amd_bounds.so")
    assert os.path.exists(lib), "build() did not make libseqrush_amd_bounds.so"
    code = f"import sys; sys.path.insert(0, 'tests'); import test_modes_mirrored_gpu as t; t.bounds_child({mode!r})"
    env = {k: v for k, v in os.environ.items() if k not in ALL_KNOBS}
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(env, SEQRUSH_AMD_LIB=lib), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "bounds build clean: " + mode in r.stdout, (r.stdout[-800:], r.stderr[-1500:])
