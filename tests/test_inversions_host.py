"""--patch-inversions without a device: the host twins against the reference's own unit tests (golden file), the edge cases
of the rule, the refusals of both CLIs, and the properties of the oracle restatement that keep the GPU tests from being
vacuous."""
import json
import os
import subprocess
import sys

import pytest

import inversion_helpers as ih
from seqrush_amd import seqrush as sr
from seqrush_amd._lib import SeqRushError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "seqrush_amd", "seqrush_mi355x")
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "inversion_known_answers.json")))
KIND = {"divergent": 1, "query_only": 2, "target_only": 3}


@pytest.mark.parametrize("case", GOLD["sites"], ids=lambda c: c["cigar"])
def test_sites_golden(case):
    ops = ih.letters_to_ops(case["cigar"])
    got = sr.inversion_sites_host(ops, case["min_gap_size"])
    assert len(got) == case["count"]
    assert [(s["query_start"], s["query_end"] - s["query_start"], s["target_start"], s["target_end"] - s["target_start"], s["kind"])
            for s in got] == [(qa, qg if k != 3 else 0, ta, tg if k != 2 else 0, k) for qa, qg, ta, tg, k, _ in ih.scan(ops, case["min_gap_size"])]
    f = case.get("first", {})
    for key in ("query_start", "query_end", "target_start", "target_end"):
        if key in f:
            assert got[0][key] == f[key]
    if "kind" in f:
        assert got[0]["kind"] == KIND[f["kind"]]
        assert got[0]["query_end"] - got[0]["query_start"] == f["query_size"]
        assert got[0]["target_end"] - got[0]["target_start"] == f["target_size"]


@pytest.mark.parametrize("case", GOLD["is_potential_inversion"], ids=lambda c: c["cite"])
def test_is_potential_inversion_golden(case):
    qg, tg = case["query"][1] - case["query"][0], case["target"][1] - case["target"][0]
    assert sr.inversion_candidate(qg, tg, case["min_inversion_size"]) == case["expect"]


def test_second_golden_site_is_found_after_the_first():
    got = sr.inversion_sites_host(ih.letters_to_ops("10M20D20I10M30X10M"), 15)
    assert [(s["query_start"], s["target_start"], s["kind"]) for s in got] == [(10, 10, 1), (40, 40, 1)]
    assert [s["candidate"] for s in got] == [True, True]


def test_gap_before_first_match_is_not_seen_and_gap_at_end_is():
    assert sr.inversion_sites_host(ih.letters_to_ops("30D30I50M"), 16) == []
    got = sr.inversion_sites_host(ih.letters_to_ops("50M30D32I"), 16)
    assert len(got) == 1 and (got[0]["query_start"], got[0]["query_end"], got[0]["target_start"], got[0]["target_end"]) == (50, 80, 50, 82)
    assert got[0]["candidate"]


def test_one_sided_sites_have_their_kind_and_are_no_candidates():
    got = sr.inversion_sites_host(ih.letters_to_ops("10M40D3I10M5D40I10M"), 16)
    assert [(s["kind"], s["candidate"]) for s in got] == [(2, False), (3, False)]
    assert got[0]["target_end"] == got[0]["target_start"] and got[1]["query_end"] == got[1]["query_start"]


def test_ratio_boundary():
    assert sr.inversion_candidate(150, 100, 16) and sr.inversion_candidate(100, 150, 16)
    assert not sr.inversion_candidate(151, 100, 16) and not sr.inversion_candidate(100, 151, 16)
    # lengths where the f64 quotient of the reference rounds: the integer form stays exact
    assert sr.inversion_candidate(3 * (2 ** 30), 2 * (2 ** 30), 1) and not sr.inversion_candidate(3 * (2 ** 30) + 1, 2 * (2 ** 30), 1)
    assert not sr.inversion_candidate(15, 15, 16) and sr.inversion_candidate(16, 16, 16)


def test_threshold_zero_is_refused():
    with pytest.raises(SeqRushError) as e:
        sr.inversion_candidate(10, 10, 0)
    assert e.value.code == -1
    with pytest.raises(SeqRushError) as e:
        sr.inversion_sites_host(ih.letters_to_ops("10M5D5I10M"), 0)
    assert e.value.code == -1


def test_accept_rule_integer_halving():
    assert sr.inversion_accept(0, 2) and not sr.inversion_accept(1, 2) and not sr.inversion_accept(1, 3)
    assert sr.inversion_accept(133, 268) and not sr.inversion_accept(134, 268) and not sr.inversion_accept(134, 269)
    assert not sr.inversion_accept(-1, 1000) and not sr.inversion_accept(0, 0) and not sr.inversion_accept(0, 1)


def _fasta(tmp_path):
    p = tmp_path / "in.fa"
    p.write_bytes(b"".join(b">" + n.encode() + b"\n" + s + b"\n" for n, s in ih.inputs("inv")))
    return str(p)


@pytest.mark.parametrize("extra, what", [(["--iterative"], "--iterative"), (["-p", "x.paf"], "-p"), ([], "-k")])
def test_cli_refusals_before_any_device_use(tmp_path, extra, what):
    fa = _fasta(tmp_path)
    k = [] if what == "-k" else ["-k", "8"]
    env = dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="")
    for cmd in ([sys.executable, "-m", "seqrush_amd"], [EXE]):
        r = subprocess.run(cmd + ["-s", fa, "-o", str(tmp_path / "o.gfa"), "--no-sort", "--patch-inversions"] + k + extra,
                           capture_output=True, text=True, env=env, cwd=str(tmp_path))
        assert r.returncode == 1, r.stderr
        assert "--patch-inversions" in r.stderr and what in r.stderr
        assert "Loaded" not in r.stdout


def test_args_fields():
    a = sr.Args()
    assert a.patch_inversions is False and a.inversion_min_size == 0


# ---------------------------------------------------------------- the restatement on the GPU tests' inputs
@pytest.mark.parametrize("name", ["inv", "pinv", "rejected", "ratio", "diverged", "soft", "bytes"])
def test_inputs_yield_accepted_patches(name):
    ref = ih.restate(name)
    assert sum(j["accepted"] for j in ref["jobs"]) >= 1
    plain = ih.restate(name, patch=False)
    assert ref["nodes"] < plain["nodes"]


def test_rc_member_has_minus_main_alignments_and_plus_patches():
    ref = ih.restate("inv")
    assert any(a["is_reverse"] for _, _, a in ref["mains"])
    assert {j["is_reverse"] for j in ref["jobs"] if j["accepted"]} == {0, 1}


def test_rejected_input_carries_a_rejected_job():
    ref = ih.restate("rejected")
    assert any(not j["accepted"] and not j["by_score"] for j in ref["jobs"])


def test_ratio_input_has_a_divergent_site_that_is_no_candidate():
    ref = ih.restate("ratio")
    found = False
    for q, t, a in ref["mains"]:
        for s in ih.scan(ih.raw_bytes_to_ops(a["cigar"]), 16):
            found |= s[4] == ih.DIVERGENT and not s[5]
    assert found


def test_divergence_bound_rejects_a_patch_the_score_rule_accepts():
    ref = ih.restate("diverged", d=0.1)
    assert any(j["by_score"] and not j["by_div"] for j in ref["jobs"])
    assert any(j["accepted"] for j in ref["jobs"])


def test_level_per_pass_penalties_yield_accepted_patches_on_the_purine_input():
    ref = ih.restate("pinv", scores="0,4,6,2,45,3")
    assert sum(j["accepted"] for j in ref["jobs"]) >= 2 and {j["is_reverse"] for j in ref["jobs"] if j["accepted"]} == {0, 1}


def test_constructed_inputs_are_plain_acgt():
    for name in ("pinv", "rejected", "ratio"):
        assert set(b"".join(s for _, s in ih.inputs(name))) <= set(b"ACGT")


def test_no_candidates_input():
    assert ih.restate("none")["jobs"] == []


def test_mirrored_positions_share_a_component_only_when_patched():
    """an accepted inversion of A[200, 320) in B: position i of A on '+' and the mirrored position of B on '-'"""
    ref, plain = ih.restate("inv"), ih.restate("inv", patch=False)
    o, po = ref["oracle"], plain["oracle"]
    offa, offb = o.seq(0)[2], o.seq(1)[2]
    L = o.L
    hits = 0
    for i in range(220, 300):
        j = 200 + 120 - 1 - (i - 200)
        pa, pb = L.sro_make_pos(offa + i, 0), L.sro_make_pos(offb + j, 1)
        assert not po.same(pa, pb)
        hits += o.same(pa, pb)
    assert hits == 80
