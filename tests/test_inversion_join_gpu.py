"""--inversion-join on the MI355X (-m gpu): the joined scan kernel against its host twin on the shapes where a chunked wave
scan can go wrong, and the whole joined mode against the Python restatement over the oracle
(inversion_join_helpers.restate): jobs with their site costs, accepted flags, labels and GFA; the false-positive guard;
penalty sets, kernel families, symbol widths, -d, shards, batches, both CLIs, and switching the mode off again."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import inversion_helpers as ih
import inversion_join_helpers as jh
import oracle_binding as ob
from seqrush_amd import seqrush as sr
from seqrush_amd._lib import SeqRushError
from seqrush_amd.seqrush import Context, Params, SeqSet
from conftest import canon_gfa

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "seqrush_amd", "seqrush_mi355x")
JOB_KEYS = ("pair", "query_idx", "target_idx", "query_start", "query_end", "target_start", "target_end", "main_score",
            "patch_score", "is_reverse", "accepted", "site_cost")
INVERSION_PAIRS = [(0, 1), (0, 3), (1, 0), (1, 2), (2, 1), (2, 3), (3, 0), (3, 2)]


def run_product(name, scores=jh.DEFAULT, k=ih.K, d=None, min_size=0, join=8, patch=True, shard=(0, 1), keep=False,
                via_align_all=False):
    ss = SeqSet(list(jh.inputs(name)))
    ctx = Context(0)
    p = Params(scores=scores, max_divergence=d)
    p.c.min_match_len = k
    p.c.shard_rank, p.c.shard_count = shard
    ctx.load(ss, p)
    if patch:
        ctx.enable_inversions(min_size, keep_alignments=keep, join_below=join)
    out = finish(ctx, patch, keep, via_align_all)
    ctx.close()
    return out


def finish(ctx, patch=True, keep=False, via_align_all=False):
    if via_align_all:
        ctx.align_all(unite=True).close()
    else:
        ctx.run()
    ctx.sync()
    out = dict(labels=ctx.download_labels(), batches=ctx.num_batches, kernel=ctx.align_kernel,
               symbol_bits=ctx.workspace_report()["symbol_bits"])
    # what the mirrored main pass did (test_modes_mirrored_gpu.py)
    out.update(rep=ctx.workspace_report(), cnt=ctx.counters(), deferred=ctx.tail_deferred(), pairs=ctx.pairs())
    out["gfa"], out["nodes"], _ = ctx.build_gfa(compact=False)
    if patch:
        out["stats"] = ctx.inversion_stats()
        out["join_stats"] = ctx.inversion_join_stats()
        out["jobs"] = ctx.inversion_jobs()
        if keep and out["stats"]["candidates"]:
            al = ctx.inversion_alignments()
            out["cigars"] = [al.cigar(i) for i in range(al.n)]
            al.close()
    return out


def check_against_restatement(name, kernel="sr_align_blk_kernel", **kw):
    ref = jh.restate(name, **{k: v for k, v in kw.items() if k in ("scores", "k", "d", "min_size", "join")})
    got = run_product(name, keep=True, **kw)
    assert got["kernel"] == kernel
    assert [tuple(j[f] for f in JOB_KEYS) for j in got["jobs"]] == [tuple(j[f] for f in JOB_KEYS) for j in ref["jobs"]]
    acc = [j for j in ref["jobs"] if j["accepted"]]
    st, js = got["stats"], got["join_stats"]
    assert (st["candidates"], st["accepted"]) == (len(ref["jobs"]), len(acc))
    assert st["rejected_score"] == js["rejected_site_cost"] == sum(not j["by_score"] for j in ref["jobs"])
    assert st["rejected_divergence"] == sum(j["by_score"] and not j["by_div"] for j in ref["jobs"])
    assert st["scanned"] == len(ref["mains"])
    assert js["islands_absorbed"] == ref["islands"]
    assert (js["host_us"] > 0) == bool(ref["jobs"])
    assert got.get("cigars", []) == [j["cigar"] for j in acc]
    assert np.array_equal(got["labels"], ref["labels"])
    assert canon_gfa(got["gfa"]) == canon_gfa(ref["gfa"])
    return got, ref


# ---------------------------------------------------------------- the scan kernel
def mk(op, ln):
    return (ln << 4) | op


def scan_shapes():
    gap = [mk(2, 30), mk(3, 30)]
    short = [mk(2 + (i & 1), 1) if i % 3 else mk(0, 2) for i in range(140)]      # 140 short ops, islands among them
    cigars = [
        [mk(0, 20)] + [mk(2, 1), mk(3, 1)] * 31 + [mk(0, 3)] + gap + [mk(0, 9)],             # island is op 63 (last lane)
        [mk(0, 20)] + [mk(2, 1), mk(3, 1)] * 31 + [mk(1, 1), mk(0, 3)] + gap + [mk(0, 9)],   # island is op 64 (next chunk's lane 0)
        [mk(0, 20)] + short + [mk(0, 12)] + gap + [mk(0, 2)] + gap + [mk(0, 40)],            # no anchor in two whole chunks
        [mk(0, 10)] + gap + [mk(0, 4)] + gap + [mk(0, 8)],                                   # an anchor as the last op
        [mk(0, 10)] + gap + [mk(0, 4)] + gap + [mk(0, 7)],                                   # an island as the last op
        [mk(0, 7)] + gap + [mk(0, 4)] + gap + [mk(0, 7)],                                    # no anchor at all
        [mk(0, 3)] + gap + [mk(0, 50)],                                                      # a leading island
        [], [mk(0, 8)], [mk(0, 7)], gap,
        [mk(0, 9)] + [mk(2, 40), mk(0, 1), mk(3, 40), mk(0, 9)] * 70,                        # a site at every chunk border
    ]
    rng = np.random.default_rng(78)
    for _ in range(200):
        ops, last = [], -1
        for _ in range(int(rng.integers(1, 260))):
            op = int(rng.choice([0, 0, 1, 2, 3]))
            if op == last:
                continue
            ln = int(rng.integers(1, 8)) if op == 0 and rng.random() < 0.6 else int(rng.integers(1, 40))
            ops.append(mk(op, ln)); last = op
        cigars.append(ops)
    return cigars


def twin_jobs(cigars, m, j, scores, skip=()):
    out, islands = [], 0
    pen = jh.penalties(scores)
    for i, c in enumerate(cigars):
        if i in skip:
            continue
        sites, cost = sr.inversion_sites_host_join(c, m, j, scores)
        out += [(i, s, k) for s, k in zip(sites, cost) if s["candidate"]]
        islands += sum(s[7] for s in jh.scan(c, m, j, pen) if s[5])
    return out, islands


@pytest.mark.parametrize("m, j, scores", [(16, 8, jh.DEFAULT), (16, 1, jh.DEFAULT), (33, 12, "0,5,8,2"), (8, 8, jh.DEFAULT)])
def test_joined_scan_kernel_against_host_twin(m, j, scores):
    cigars = scan_shapes()
    want, islands = twin_jobs(cigars, m, j, scores)
    got, st = sr.inversion_scan_device_join(cigars, m, j, scores)
    assert got == want                                          # sites, costs, owners, emitted order
    assert st["candidates"] == len(want) and st["scanned"] == len(cigars) and st["islands"] == islands
    if (m, j) == (16, 8):
        by = lambda i: [s for o, s, _ in got if o == i]          # noqa: E731
        assert len(by(0)) == 1 and by(0)[0]["query_end"] - by(0)[0]["query_start"] == 31 + 3 + 30
        assert len(by(1)) == 1 and by(1)[0]["query_end"] - by(1)[0]["query_start"] == 31 + 1 + 3 + 30
        assert len(by(2)) == 2 and len(by(3)) == 1 and len(by(4)) == 1 and by(5) == [] and by(6) == []
        assert by(4)[0]["query_end"] - by(4)[0]["query_start"] == 30 + 4 + 30 + 7      # closed by the end, island included
    if j == 1:                                                  # the plain rule's jobs
        assert [(o, s) for o, s, _ in got] == sr.inversion_scan_device(cigars, m)


def test_joined_scan_skips_failed_and_dropped_alignments():
    cigars = scan_shapes()[:7] * 3
    n = len(cigars)
    score, bound = np.full(n, 100, np.int32), np.full(n, 1000, np.int32)
    score[2] = -1                                               # a failed alignment
    score[9] = 1001                                             # dropped by -d
    want, islands = twin_jobs(cigars, 16, 8, jh.DEFAULT, skip=(2, 9))
    got, st = sr.inversion_scan_device_join(cigars, 16, 8, jh.DEFAULT, score=score, max_score=bound)
    assert got == want and st["scanned"] == n - 2 and st["islands"] == islands
    assert {o for o, _, _ in got} >= {0, 1, 3, 4, 16} and not {o for o, _, _ in got} & {2, 9}
    assert [o for o, _, _ in got] == sorted(o for o, _, _ in got)


def test_join_above_threshold_is_refused():
    ss = SeqSet(list(jh.inputs("pick")))
    ctx = Context(0)
    p = Params()
    p.c.min_match_len = 8
    ctx.load(ss, p)
    with pytest.raises(SeqRushError) as e:
        ctx.enable_inversions(join_below=17)
    assert e.value.code == -1
    ctx.enable_inversions(join_below=16)
    ctx.close()
    with pytest.raises(SeqRushError):
        sr.inversion_scan_device_join([[mk(0, 9)]], 16, 17)


# ---------------------------------------------------------------- the whole mode
def test_c5_like_eight_inversions():
    got, ref = check_against_restatement("c5like", k=16)
    assert [(j["query_idx"], j["target_idx"]) for j in got["jobs"]] == INVERSION_PAIRS
    assert got["stats"]["accepted"] == 8 and {j["is_reverse"] for j in got["jobs"]} == {0, 1}
    assert all(0 < j["site_cost"] <= j["main_score"] for j in got["jobs"])
    plain = run_product("c5like", k=16, join=0)
    assert plain["stats"]["candidates"] == 0
    assert got["nodes"] < plain["nodes"]


def test_sweep_input_without_a_plain_job():
    """seed 0 (base_sequence(500, 7000)), L = 104 inverted at 200, and its reverse-complemented third member"""
    got, ref = check_against_restatement("pick")
    assert got["stats"]["accepted"] >= 2 and {j["is_reverse"] for j in got["jobs"] if j["accepted"]} == {0, 1}
    plain = run_product("pick", join=0)
    assert plain["stats"]["candidates"] == 0 and got["nodes"] < plain["nodes"]


def test_snp_clusters_are_jobs_and_none_is_accepted():
    got, ref = check_against_restatement("snp", k=8)
    assert got["stats"]["candidates"] == len(ref["jobs"]) > 0 and got["stats"]["accepted"] == 0
    assert got["join_stats"]["rejected_site_cost"] == len(ref["jobs"])
    plain = run_product("snp", k=8, patch=False)
    assert np.array_equal(got["labels"], plain["labels"]) and got["gfa"] == plain["gfa"]


def test_join_one_has_the_plain_sites_and_the_site_accept_rule():
    got, ref = check_against_restatement("rejected", join=1)
    plain = run_product("rejected", join=0)
    strip = lambda jobs: [tuple(j[f] for f in JOB_KEYS[:8]) for j in jobs]      # noqa: E731
    assert strip(got["jobs"]) == strip(plain["jobs"]) and len(got["jobs"]) >= 2
    assert all(j["site_cost"] == 0 for j in plain["jobs"]) and all(j["site_cost"] > 0 for j in got["jobs"])


def test_single_piece_penalties():
    got, _ = check_against_restatement("pick", scores="0,5,8,2")
    assert got["stats"]["accepted"] >= 1


def test_level_per_pass_penalties():
    got, _ = check_against_restatement("pick", scores="0,4,6,2,45,3", kernel="sr_align_bfs_kernel")
    assert got["stats"]["candidates"] >= 1


def test_divergence_bound():
    """-d folds into the site-cost bound: a job the site-cost rule accepts and the divergence bound drops"""
    got, ref = check_against_restatement("diverged", d=0.1)
    assert any(j["by_score"] and not j["by_div"] for j in ref["jobs"]) and any(j["accepted"] for j in ref["jobs"])
    assert got["stats"]["rejected_divergence"] >= 1 and got["stats"]["accepted"] >= 1
    assert got["stats"]["scanned"] == len(ref["mains"])


def test_four_bit_and_eight_bit_symbols():
    got, _ = check_against_restatement("pick_soft")
    assert got["symbol_bits"] == 4 and got["stats"]["accepted"] >= 1
    got, _ = check_against_restatement("pick_bytes")
    assert got["symbol_bits"] == 8 and got["stats"]["accepted"] >= 1


def test_two_shards_merge_to_the_unsharded_forest():
    whole = run_product("c5like", k=16)
    parts = [run_product("c5like", k=16, shard=(r, 2)) for r in (0, 1)]
    assert sum(p["stats"]["candidates"] for p in parts) == whole["stats"]["candidates"] == 8
    assert sum(p["stats"]["accepted"] for p in parts) == 8
    ss = SeqSet(list(jh.inputs("c5like")))
    ctx = Context(0)
    ctx.load_pairs(ss, Params(), [])
    lab = np.ascontiguousarray(np.concatenate([p["labels"] for p in parts]), dtype=np.uint64)
    sr.check(ctx.L.sr_ctx_merge_labels_host(ctx._h, lab.ctypes.data_as(C.POINTER(C.c_uint64)), 2))
    ctx.sync()
    assert np.array_equal(ctx.download_labels(), whole["labels"])
    ctx.close()


def test_several_batches_and_align_all_give_the_same_jobs(monkeypatch):
    one = run_product("pick", keep=True)
    monkeypatch.setenv("SR_CIGAR_ARENA_OPS", "2100")
    many = run_product("pick", keep=True)
    also = run_product("pick", keep=True, via_align_all=True)
    monkeypatch.delenv("SR_CIGAR_ARENA_OPS")
    assert one["batches"] == 1 and many["batches"] >= 4 and one["stats"]["accepted"] >= 2
    for other in (many, also):
        assert other["jobs"] == one["jobs"] and other["cigars"] == one["cigars"]
        assert np.array_equal(other["labels"], one["labels"])
        assert other["join_stats"]["islands_absorbed"] == one["join_stats"]["islands_absorbed"]


def test_join_off_after_a_joined_run_is_the_plain_mode():
    ss = SeqSet(list(jh.inputs("pick")))
    ctx = Context(0)
    p = Params()
    p.c.min_match_len = ih.K
    ctx.load(ss, p)
    ctx.enable_inversions(join_below=8)
    joined = finish(ctx)
    ctx.reset_uf()
    ctx.enable_inversions(join_below=0)
    again = finish(ctx)
    ctx.close()
    plain = run_product("pick", join=0)
    assert joined["stats"]["accepted"] >= 2
    assert again["jobs"] == plain["jobs"] == [] and again["stats"]["candidates"] == 0
    assert again["join_stats"] == dict(islands_absorbed=0, rejected_site_cost=0, host_us=0)
    assert np.array_equal(again["labels"], plain["labels"]) and again["gfa"] == plain["gfa"]
    assert not np.array_equal(again["labels"], joined["labels"])


@pytest.mark.parametrize("which", ["python", "native"])
def test_cli(tmp_path, which):
    fa = tmp_path / "in.fa"
    fa.write_bytes(b"".join(b">" + n.encode() + b"\n" + s + b"\n" for n, s in jh.inputs("pick")))
    out, paf = tmp_path / "o.gfa", tmp_path / "o.paf"
    cmd = [sys.executable, "-m", "seqrush_amd"] if which == "python" else [EXE]
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run(cmd + ["-s", str(fa), "-o", str(out), "--no-sort", "--no-compact", "-k", str(ih.K), "--patch-inversions",
                              "--inversion-join", "8", "-v", "--output-alignments", str(paf)],
                       capture_output=True, text=True, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    ref = jh.restate("pick")
    acc = [j for j in ref["jobs"] if j["accepted"]]
    assert len(acc) >= 2
    said = r.stdout.split("\n")
    assert f"Patched inversions: {len(acc)} of {len(ref['jobs'])} candidate gaps" in said
    assert (f"Inversion join: {ref['islands']} match islands absorbed into candidate gaps, "
            f"{len(ref['jobs']) - len(acc)} jobs rejected by site cost") in said
    assert canon_gfa(out.read_text()) == canon_gfa(ref["gfa"])
    lines = paf.read_text().strip().split("\n")
    assert len(lines) == 9 + len(acc) and not any("sr:Z:inv" in l for l in lines[:9])
    names = [n for n, _ in jh.inputs("pick")]
    for l, j in zip(lines[9:], acc):
        f = l.split("\t")
        assert f[-1] == "sr:Z:inv" and f[-2] == "cg:Z:" + j["cigar"]
        assert (f[0], int(f[2]), int(f[3]), f[4], f[5], int(f[7]), int(f[8])) == (
            names[j["query_idx"]], j["query_start"], j["query_end"], "-" if j["is_reverse"] else "+", names[j["target_idx"]],
            j["target_start"], j["target_end"])
