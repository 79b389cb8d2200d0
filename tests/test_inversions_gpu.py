"""--patch-inversions on the MI355X (-m gpu): scan, patch pass and patch unite against the Python restatement over the
oracle (inversion_helpers.restate): jobs, strands, coordinates, scores, accepted flags, patch CIGARs, canonical labels and
the --no-sort GFA with and without compaction; variants (symbol widths, single-piece penalties, -d, shards, batches, long
gaps through the scan's chunk carry) and both CLIs."""
import os
import subprocess
import sys

import numpy as np
import pytest

import inversion_helpers as ih
import oracle_binding as ob
from seqrush_amd import seqrush as sr
from seqrush_amd._lib import SeqRushError
from seqrush_amd.seqrush import Context, Params, SeqSet
from conftest import canon_gfa

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "seqrush_amd", "seqrush_mi355x")
JOB_KEYS = ("pair", "query_idx", "target_idx", "query_start", "query_end", "target_start", "target_end", "main_score",
            "patch_score", "is_reverse", "accepted")


def run_product(name, scores="0,5,8,2,24,1", k=ih.K, d=None, min_size=0, patch=True, shard=(0, 1), keep=True, via_align_all=False):
    ss = SeqSet(list(ih.inputs(name)))
    ctx = Context(0)
    p = Params(scores=scores, max_divergence=d)
    p.c.min_match_len = k
    p.c.shard_rank, p.c.shard_count = shard
    ctx.load(ss, p)
    if patch:
        ctx.enable_inversions(min_size, keep_alignments=keep)
    if via_align_all:
        ctx.align_all(unite=True).close()
    else:
        ctx.run()
    ctx.sync()
    out = dict(labels=ctx.download_labels(), pairs=ctx.pairs(), batches=ctx.num_batches, kernel=ctx.align_kernel,
               symbol_bits=ctx.workspace_report()["symbol_bits"])
    # what the mirrored main pass did (test_modes_mirrored_gpu.py)
    out.update(rep=ctx.workspace_report(), cnt=ctx.counters(), deferred=ctx.tail_deferred())
    out["gfa"], out["nodes"], _ = ctx.build_gfa(compact=False)
    out["gfa_compact"] = ctx.build_gfa(compact=True)[0]
    if patch:
        out["stats"] = ctx.inversion_stats()
        out["jobs"] = ctx.inversion_jobs()
        if keep and out["stats"]["candidates"]:
            al = ctx.inversion_alignments()
            out["cigars"] = [al.cigar(i) for i in range(al.n)]
            out["al"] = [(int(al.query_idx[i]), int(al.target_idx[i]), int(al.is_reverse[i]), int(al.score[i]),
                          int(al.query_start[i]), int(al.query_end[i]), int(al.target_start[i]), int(al.target_end[i]))
                         for i in range(al.n)]
            al.close()
    ctx.close()
    return out


def check_against_restatement(name, **kw):
    kernel = kw.pop("kernel", "sr_align_blk_kernel")
    ref = ih.restate(name, **{k: v for k, v in kw.items() if k in ("scores", "k", "d", "min_size")})
    got = run_product(name, **kw)
    assert got["kernel"] == kernel
    assert [tuple(j[f] for f in JOB_KEYS) for j in got["jobs"]] == [tuple(j[f] for f in JOB_KEYS) for j in ref["jobs"]]
    acc = [j for j in ref["jobs"] if j["accepted"]]
    st = got["stats"]
    assert (st["candidates"], st["accepted"]) == (len(ref["jobs"]), len(acc))
    assert st["rejected_score"] == sum(not j["by_score"] for j in ref["jobs"])
    assert st["rejected_divergence"] == sum(j["by_score"] and not j["by_div"] for j in ref["jobs"])
    assert st["scanned"] == len(ref["mains"])
    assert (st["patch_batches"] >= 1) == bool(ref["jobs"]) and (st["united_bases"] > 0) == bool(acc)
    assert got.get("cigars", []) == [j["cigar"] for j in acc]
    assert got.get("al", []) == [(j["query_idx"], j["target_idx"], j["is_reverse"], j["patch_score"], j["query_start"], j["query_end"],
                          j["target_start"], j["target_end"]) for j in acc]
    assert np.array_equal(got["labels"], ref["labels"])
    assert canon_gfa(got["gfa"]) == canon_gfa(ref["gfa"])
    assert canon_gfa(got["gfa_compact"]) == canon_gfa(ob.compact_gfa(ref["gfa"])[0])
    return got, ref


def path_steps(gfa, name):
    for line in gfa.split("\n"):
        f = line.split("\t")
        if f[0] == "P" and f[1] == name:
            return [(s[:-1], s[-1]) for s in f[2].split(",")]
    raise KeyError(name)


def test_inversion_and_rc_member():
    got, ref = check_against_restatement("inv")
    assert {j["is_reverse"] for j in got["jobs"] if j["accepted"]} == {0, 1}      # main strands '+' and '-'
    plain = run_product("inv", patch=False)
    assert got["nodes"] < plain["nodes"]
    a_nodes = {n for n, _ in path_steps(got["gfa"], "A")}
    assert sum(1 for n, o in path_steps(got["gfa"], "B") if o == "-" and n in a_nodes) >= 80
    assert not any(o == "-" and n in {m for m, _ in path_steps(plain["gfa"], "A")} for n, o in path_steps(plain["gfa"], "B"))


def test_rejected_candidate():
    got, _ = check_against_restatement("rejected")
    assert got["stats"]["rejected_score"] >= 1 and got["symbol_bits"] == 2


def test_ratio_failure_is_a_site_but_no_job():
    got, ref = check_against_restatement("ratio")
    assert got["stats"]["sites"] > got["stats"]["candidates"]


def test_lower_case_and_n_four_bit_symbols():
    got, _ = check_against_restatement("soft")
    assert got["symbol_bits"] == 4


def test_eight_bit_symbols():
    got, _ = check_against_restatement("bytes")
    assert got["symbol_bits"] == 8


def test_single_piece_penalties():
    check_against_restatement("inv", scores="0,5,8,2")


def test_divergence_bound_drops_a_patch():
    got, _ = check_against_restatement("diverged", d=0.1)
    assert got["stats"]["rejected_divergence"] >= 1 and got["stats"]["accepted"] >= 1


def test_explicit_min_size_overrides_2k():
    got, _ = check_against_restatement("inv", min_size=121)
    assert got["stats"]["candidates"] == 0 or all(j["query_end"] - j["query_start"] >= 121 for j in got["jobs"])
    got0 = run_product("inv", min_size=121, keep=False)
    assert np.array_equal(got0["labels"], got["labels"])


def test_level_per_pass_penalties():
    """0,4,6,2,45,3 runs on the level-per-pass kernel, main pass and patch pass"""
    got, _ = check_against_restatement("pinv", scores="0,4,6,2,45,3", kernel="sr_align_bfs_kernel")
    assert got["stats"]["accepted"] >= 2


def test_level_per_pass_kernel_on_default_penalties(monkeypatch):
    monkeypatch.setenv("SR_ALIGN_IMPL", "1")
    check_against_restatement("inv", kernel="sr_align_bfs_kernel")
    check_against_restatement("rejected", kernel="sr_align_bfs_kernel")


def test_purine_inversion_two_bit():
    got, _ = check_against_restatement("pinv")
    assert got["symbol_bits"] == 2 and {j["is_reverse"] for j in got["jobs"] if j["accepted"]} == {0, 1}


def test_threshold_zero_paf_and_iterative_contexts_are_refused(tmp_path):
    ss = SeqSet(list(ih.inputs("inv")))
    ctx = Context(0)
    ctx.load(ss, Params())
    with pytest.raises(SeqRushError) as e:
        ctx.enable_inversions()                 # -k 0 and no minimum size
    assert e.value.code == -1
    ctx.load_iterative(ss, Params(sparsification="tree:1,0,1.0"))
    with pytest.raises(SeqRushError) as e:
        ctx.enable_inversions(16)
    assert e.value.code == -6
    paf = tmp_path / "e.paf"
    paf.write_text("")
    ctx.load_paf(ss, Params(), str(paf))
    with pytest.raises(SeqRushError) as e:
        ctx.enable_inversions(16)
    assert e.value.code == -6
    ctx.close()


def test_no_candidates_is_the_plain_run_bit_for_bit():
    on, off = run_product("none"), run_product("none", patch=False)
    assert on["stats"]["candidates"] == 0 and on["stats"]["patch_batches"] == 0 and on["stats"]["united_bases"] == 0
    assert on["stats"]["scanned"] == 16 and on["jobs"] == []
    assert np.array_equal(on["labels"], off["labels"]) and on["gfa"] == off["gfa"]
    assert np.array_equal(on["labels"], ih.restate("none")["labels"])


def test_two_shards_merge_to_the_unsharded_forest():
    import ctypes as C
    whole = run_product("inv", keep=False)
    parts = [run_product("inv", shard=(r, 2), keep=False) for r in (0, 1)]
    assert sum(p["stats"]["candidates"] for p in parts) == whole["stats"]["candidates"]
    assert sum(p["stats"]["accepted"] for p in parts) == whole["stats"]["accepted"]
    ss = SeqSet(list(ih.inputs("inv")))
    ctx = Context(0)
    ctx.load_pairs(ss, Params(), [])
    lab = np.ascontiguousarray(np.concatenate([p["labels"] for p in parts]), dtype=np.uint64)
    sr.check(ctx.L.sr_ctx_merge_labels_host(ctx._h, lab.ctypes.data_as(C.POINTER(C.c_uint64)), 2))
    ctx.sync()
    assert np.array_equal(ctx.download_labels(), whole["labels"])
    ctx.close()


def test_several_batches_give_the_same_jobs(monkeypatch):
    one = run_product("inv")
    monkeypatch.setenv("SR_CIGAR_ARENA_OPS", "2100")
    many = run_product("inv")
    also = run_product("inv", via_align_all=True)
    monkeypatch.delenv("SR_CIGAR_ARENA_OPS")
    assert one["batches"] == 1 and many["batches"] >= 4
    for other in (many, also):
        assert other["jobs"] == one["jobs"] and other["cigars"] == one["cigars"]
        assert np.array_equal(other["labels"], one["labels"])


def test_scan_kernel_against_host_twin_on_synthetic_cigars():
    """the chunk carry: gaps of more than 64 ops, gaps across chunk borders, gaps to the end, CIGARs of 0 and 1 ops, and a
    few hundred random ones -- device scan == host twin == Python scan"""
    rng = np.random.default_rng(77)
    mk = lambda op, ln: (ln << 4) | op                      # noqa: E731
    cigars = [
        [mk(0, 20)] + [mk(2 + (i & 1), 1) for i in range(150)] + [mk(0, 9)],                  # 150-op gap, 75 / 75
        [mk(0, 5)] + [mk(1, 1), mk(2, 2), mk(3, 2)] * 60,                                     # 180 ops running to the end
        [mk(0, 3)] * 1 + [mk(2, 40), mk(3, 40), mk(0, 1)] * 70,                               # a site at every chunk border
        [], [mk(0, 7)], [mk(2, 30), mk(3, 30)], [mk(0, 1), mk(2, 16), mk(3, 24)], [mk(0, 1), mk(2, 16), mk(3, 25)],
        [mk(2, 500)] + [mk(0, 4), mk(1, 17)] * 40,
    ]
    for _ in range(300):
        n = int(rng.integers(1, 200))
        ops, last = [], -1
        for _ in range(n):
            op = int(rng.choice([0, 0, 1, 2, 3]))
            if op == last:
                continue
            ops.append(mk(op, int(rng.integers(1, 40)))); last = op
        cigars.append(ops)
    for m in (1, 16, 33):
        want = [(i, dict(query_start=qa, query_end=qa + qg, target_start=ta, target_end=ta + tg, kind=1, candidate=True))
                for i, c in enumerate(cigars) for qa, qg, ta, tg, kind, cand in ih.scan(c, m) if cand]
        twin = [(i, s) for i, c in enumerate(cigars) for s in sr.inversion_sites_host(c, m) if s["candidate"]]
        got = sr.inversion_scan_device(cigars, m)
        assert twin == want
        assert got == want
    assert any(s["query_end"] - s["query_start"] == 75 for i, s in sr.inversion_scan_device(cigars, 16) if i == 0)


@pytest.mark.parametrize("which", ["python", "native"])
def test_cli(tmp_path, which):
    fa = tmp_path / "in.fa"
    fa.write_bytes(b"".join(b">" + n.encode() + b"\n" + s + b"\n" for n, s in ih.inputs("inv")))
    out, paf = tmp_path / "o.gfa", tmp_path / "o.paf"
    cmd = [sys.executable, "-m", "seqrush_amd"] if which == "python" else [EXE]
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run(cmd + ["-s", str(fa), "-o", str(out), "--no-sort", "--no-compact", "-k", str(ih.K), "--patch-inversions",
                              "--output-alignments", str(paf)], capture_output=True, text=True, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    ref = ih.restate("inv")
    acc = [j for j in ref["jobs"] if j["accepted"]]
    assert f"Patched inversions: {len(acc)} of {len(ref['jobs'])} candidate gaps" in r.stdout.split("\n")
    assert canon_gfa(out.read_text()) == canon_gfa(ref["gfa"])
    lines = paf.read_text().strip().split("\n")
    assert len(lines) == 9 + len(acc) and not any("sr:Z:inv" in l for l in lines[:9])
    names = [n for n, _ in ih.inputs("inv")]
    for l, j in zip(lines[9:], acc):
        f = l.split("\t")
        assert f[-1] == "sr:Z:inv" and f[-2] == "cg:Z:" + j["cigar"]
        assert (f[0], int(f[2]), int(f[3]), f[4], f[5], int(f[7]), int(f[8])) == (
            names[j["query_idx"]], j["query_start"], j["query_end"], "-" if j["is_reverse"] else "+", names[j["target_idx"]],
            j["target_start"], j["target_end"])
