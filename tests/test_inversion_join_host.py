"""--inversion-join without a device: the joined host twin against the Python restatement of the rule, the edges of the rule
(anchor length, leading and trailing islands), the cost invariant on oracle alignments, the 70-input inversion sweep, and the
refusals."""
import os
import subprocess
import sys

import numpy as np
import pytest

import inversion_helpers as ih
import inversion_join_helpers as jh
import oracle_binding as ob
from seqrush_amd import seqrush as sr
from seqrush_amd import synth
from seqrush_amd._lib import SeqRushError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "seqrush_amd", "seqrush_mi355x")
SINGLE = "0,5,8,2"


def twin(ops, m, j, scores=jh.DEFAULT):
    sites, cost = sr.inversion_sites_host_join(ops, m, j, scores)
    return [(s["query_start"], s["query_end"], s["target_start"], s["target_end"], s["kind"], s["candidate"], c)
            for s, c in zip(sites, cost)]


def want(ops, m, j, scores=jh.DEFAULT):
    return [(qa, qa + (qg if kind != 3 else 0), ta, ta + (tg if kind != 2 else 0), kind, bool(cand), cost)
            for qa, qg, ta, tg, kind, cand, cost, _ in jh.scan(ops, m, j, jh.penalties(scores))]


def random_cigars(seed, count, max_ops=200):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        ops, last = [], -1
        for _ in range(int(rng.integers(1, max_ops))):
            op = int(rng.choice([0, 0, 1, 2, 3]))
            if op == last:
                continue
            ln = int(rng.integers(1, 6)) if op == 0 and rng.random() < 0.5 else int(rng.integers(1, 40))
            ops.append((ln << 4) | op); last = op
        out.append(ops)
    return out


@pytest.mark.parametrize("scores", [jh.DEFAULT, SINGLE])
def test_twin_equals_the_python_scan_on_random_cigars(scores):
    seen = 0
    for ops in random_cigars(91, 300):
        for m, j in ((16, 8), (16, 1), (33, 12), (8, 8)):
            got = twin(ops, m, j, scores)
            assert got == want(ops, m, j, scores)
            seen += sum(1 for s in got if s[5])
    assert seen > 100


def test_join_one_gives_the_plain_sites():
    for ops in random_cigars(92, 200):
        for m in (1, 16, 33):
            plain = sr.inversion_sites_host(ops, m)
            sites, cost = sr.inversion_sites_host_join(ops, m, 1)
            assert sites == plain
            assert len(cost) == len(sites) and all(c >= 0 for c in cost)


def test_anchor_length_boundary():
    """a match op of exactly J columns is an anchor, one of J - 1 an island"""
    at = ih.letters_to_ops("20M30D8M30I20M")            # len == J: two one-sided sites
    below = ih.letters_to_ops("20M30D7M30I20M")         # len == J - 1: one two-sided site, the island on both sides
    assert [(s[4], s[5]) for s in twin(at, 16, 8)] == [(2, False), (3, False)]
    got = twin(below, 16, 8)
    assert got == [(20, 57, 20, 57, 1, True, 2 * min(8 + 30 * 2, 24 + 30))]
    assert got == want(below, 16, 8)


def test_leading_island_without_an_anchor_before_it_is_not_seen():
    ops = ih.letters_to_ops("3M30D30I50M")
    assert twin(ops, 16, 8) == [] == want(ops, 16, 8)
    assert len(sr.inversion_sites_host(ops, 16)) == 1       # the plain rule opens a site at the 3M


def test_trailing_island_is_closed_by_the_end():
    ops = ih.letters_to_ops("50M30D5M32I4M")
    got = twin(ops, 16, 8)
    assert got == [(50, 50 + 30 + 5 + 4, 50, 50 + 5 + 32 + 4, 1, True, (24 + 30) + (24 + 32))] == want(ops, 16, 8)


def test_no_anchor_at_all():
    ops = ih.letters_to_ops("7M30D5M32I4M")
    assert twin(ops, 16, 8) == []


def test_site_cost_formula_per_penalty_set():
    ops = ih.letters_to_ops("10M3X2M40D1M40I10M")
    assert [s[6] for s in twin(ops, 16, 8)] == [3 * 5 + (24 + 40) * 2]
    assert [s[6] for s in twin(ops, 16, 8, SINGLE)] == [3 * 5 + (8 + 40 * 2) * 2]
    assert [s[6] for s in twin(ih.letters_to_ops("10M5D5I3X10M"), 5, 5)] == [2 * (8 + 5 * 2) + 15]     # short gaps: first piece


def test_accept_site_integer_halving():
    assert sr.inversion_accept_site(0, 2) and not sr.inversion_accept_site(1, 2) and not sr.inversion_accept_site(1, 3)
    assert sr.inversion_accept_site(519, 1040) and not sr.inversion_accept_site(520, 1040) and not sr.inversion_accept_site(520, 1041)
    assert not sr.inversion_accept_site(-1, 1000) and not sr.inversion_accept_site(0, 0) and not sr.inversion_accept_site(0, 1)
    for p, c in ((0, 2), (1, 3), (519, 1040), (520, 1040), (-1, 9)):
        assert sr.inversion_accept_site(p, c) == jh.accept_site(p, c)


def test_join_above_threshold_and_zero_are_refused():
    ops = ih.letters_to_ops("16M20D20I16M")
    for j in (17, 0):
        with pytest.raises(SeqRushError) as e:
            sr.inversion_sites_host_join(ops, 16, j)
        assert e.value.code == -1
    assert len(sr.inversion_sites_host_join(ops, 16, 16)[0]) == 1


def _oracle_alignments(recs, scores):
    o = ob.OracleSeqRush(records=list(recs))
    op = ih.oracle_params(scores)
    out = [o.align_pair(op, q, t) for q in range(o.n) for t in range(o.n) if q != t]
    o.close()
    return out


@pytest.mark.parametrize("scores", [jh.DEFAULT, SINGLE])
def test_cost_invariant_on_oracle_alignments(scores):
    """the sum of the op costs of a whole CIGAR is the alignment's score; through the twin: one anchor op in front and J = 1
    make the whole CIGAR minus its match ops the sum of the sites' costs"""
    pen = jh.penalties(scores)
    families = [synth.snp_family(3, 600, 0.05, 7104), synth.indel_family(3, 600, 0.03, 0.01, 7105), ih.inputs("inv"),
                jh.inputs("pick")]
    n = 0
    for recs in families:
        for a in _oracle_alignments(recs, scores):
            ops = ih.raw_bytes_to_ops(a["cigar"])
            assert jh.cigar_cost(ops, pen) == a["score"]
            sites, cost = sr.inversion_sites_host_join([(1 << 4) | 0] + ops, 1, 1, scores)
            assert sum(cost) == a["score"], (a["score"], cost)      # (ops before the first match op: the added anchor's site)
            n += 1
    assert n >= 24


@pytest.fixture(scope="module")
def sweep():
    """10 seeds x 7 lengths: forward WFA of a against b = a with L bases inverted at 200, -S 0,5,8,2,24,1"""
    pen = jh.penalties()
    out = {}
    for seed in jh.SWEEP_SEEDS:
        for length in jh.SWEEP_LENGTHS:
            a, b = jh.sweep_pair(seed, length)
            raw, score = ob.wfa_align(a, b, pen)
            out[seed, length] = (a, b, ih.raw_bytes_to_ops(raw), score)
    return out


def test_sweep_twin_equals_restatement(sweep):
    for (seed, length), (a, b, ops, score) in sweep.items():
        assert twin(ops, 16, 8) == want(ops, 16, 8), (seed, length)
        assert jh.cigar_cost(ops, jh.penalties()) == score


def test_sweep_joined_rule_finds_the_inversions_and_accepts_them(sweep):
    pen = jh.penalties()
    with_plain = with_joined = 0
    for (seed, length), (a, b, ops, score) in sweep.items():
        with_plain += any(s[5] for s in ih.scan(ops, 16))
        cands = [s for s in jh.scan(ops, 16, 8, pen) if s[5]]
        with_joined += bool(cands)
        for qa, qg, ta, tg, kind, cand, cost, isl in cands:
            raw, sc = ob.wfa_align(synth.reverse_complement(a[qa:qa + qg]), b[ta:ta + tg], pen)
            assert jh.accept_site(sc, cost) and sr.inversion_accept_site(sc, cost), (seed, length, sc, cost)
            assert cost <= score
    print(f"inputs with a candidate: plain {with_plain} of 70, joined {with_joined} of 70")
    assert with_joined >= 60
    assert with_plain < with_joined


def twin_agrees_with_restatement(ref, m, j, scores=jh.DEFAULT):
    """the product's host twin and accept test over the restatement's own main alignments: the same jobs, site costs and
    accept decisions (the -d bound aside)"""
    jobs = iter(ref["jobs"])
    n = 0
    for q, t, a in ref["mains"]:
        sites, cost = sr.inversion_sites_host_join(ih.raw_bytes_to_ops(a["cigar"]), m, j, scores)
        for s, c in zip(sites, cost):
            if not s["candidate"]:
                continue
            job = next(jobs)
            assert (job["query_idx"], job["target_idx"], job["qa"], job["qa"] + job["qgap"], job["ta"], job["ta"] + job["tgap"],
                    job["site_cost"]) == (q, t, s["query_start"], s["query_end"], s["target_start"], s["target_end"], c)
            assert sr.inversion_accept_site(job["patch_score"], c) == bool(job["by_score"])
            assert sr.inversion_accept(job["patch_score"], a["score"]) == bool(job["by_main"])
            n += 1
    assert next(jobs, None) is None and n == len(ref["jobs"])


def test_picked_sweep_input_has_no_plain_job_and_an_accepted_joined_one(sweep):
    a, b, ops, score = sweep[jh.PICK_SEED, jh.PICK_L]
    assert not any(s[5] for s in ih.scan(ops, 16))
    assert any(s[5] for s in jh.scan(ops, 16, 8, jh.penalties()))
    ref = jh.restate("pick")
    assert jh.restate("pick", join=0)["jobs"] == [] and sum(j["accepted"] for j in ref["jobs"]) >= 2
    assert {j["is_reverse"] for j in ref["jobs"] if j["accepted"]} == {0, 1}
    twin_agrees_with_restatement(ref, 16, 8)


def test_c5_like_restatement_yields_the_eight_inversion_jobs():
    ref = jh.restate("c5like", k=16)
    assert [(j["query_idx"], j["target_idx"]) for j in ref["jobs"]] == [(0, 1), (0, 3), (1, 0), (1, 2), (2, 1), (2, 3), (3, 0), (3, 2)]
    assert all(j["accepted"] for j in ref["jobs"]) and ref["islands"] > 0
    assert jh.restate("c5like", k=16, join=0)["jobs"] == []
    assert ref["nodes"] < jh.restate("c5like", k=16, patch=False)["nodes"]
    twin_agrees_with_restatement(ref, 32, 8)


def test_snp_family_restatement_rejects_every_joined_job_where_main_half_would_not():
    ref = jh.restate("snp", k=8)
    assert len(ref["jobs"]) > 0 and not any(j["accepted"] for j in ref["jobs"])
    assert all(j["by_main"] for j in ref["jobs"])              # the reference's test would have united all of them
    assert np.array_equal(ref["labels"], jh.restate("snp", k=8, patch=False)["labels"])
    twin_agrees_with_restatement(ref, 16, 8)


def _fasta(tmp_path):
    p = tmp_path / "in.fa"
    p.write_bytes(b"".join(b">" + n.encode() + b"\n" + s + b"\n" for n, s in jh.inputs("pick")))
    return str(p)


@pytest.mark.parametrize("extra, what", [(["--inversion-join", "8"], "--patch-inversions"),
                                         (["--patch-inversions", "--inversion-join", "17"], "threshold")])
def test_cli_refusals_before_any_device_use(tmp_path, extra, what):
    fa = _fasta(tmp_path)
    env = dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="")
    for cmd in ([sys.executable, "-m", "seqrush_amd"], [EXE]):
        r = subprocess.run(cmd + ["-s", fa, "-o", str(tmp_path / "o.gfa"), "--no-sort", "-k", "8"] + extra,
                           capture_output=True, text=True, env=env, cwd=str(tmp_path))
        assert r.returncode == 1, r.stderr
        assert "--inversion-join" in r.stderr and what in r.stderr
        assert "Loaded" not in r.stdout


def test_args_and_api_refusals():
    a = sr.Args()
    assert a.inversion_join == 0
    a.inversion_join = 8
    with pytest.raises(SeqRushError) as e:
        sr.check_inversion_join(a)                              # without patch_inversions
    assert e.value.code == -1
    a.patch_inversions, a.min_match_length, a.inversion_join = True, 8, 17
    with pytest.raises(SeqRushError):
        sr.check_inversion_join(a)
    a.inversion_join = 16
    sr.check_inversion_join(a)
