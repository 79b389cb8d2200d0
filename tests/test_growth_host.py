"""CPU tests (-m "not gpu") of the growth curves through the host twin (device = -1): hand-worked known
answers, the exact integer identity over all G! orders, the identities with graph_stats, invariants of every row, a
restatement by Python sets, the closed-form expectation against exact rationals, the Heaps' law fit against numpy.polyfit,
the report bytes, the refusals and the command line."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import growth_inputs as gi
from test_stats_host import GOLDEN
from seqrush_amd import _lib
from seqrush_amd.seqrush import (Growth, SeqRushError, graph_stats, growth, growth_expected, growth_fit, growth_groups,
                                 growth_report)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOWN = json.load(open(os.path.join(ROOT, "tests", "golden", "growth_known_answers.json")))["cases"]
TWIN = -1
INPUTS = gi.host_inputs()
GFA = {c["name"]: c["gfa"] for c in GOLDEN}


@pytest.mark.parametrize("case", KNOWN, ids=[c["name"] + ("" if c["group_of"] is None else ":grouped") for c in KNOWN])
def test_known_answers(case):
    text = GFA[case["name"]]
    kw = {} if case["group_of"] is None else dict(group_of=case["group_of"])
    d = growth(text, TWIN, **kw)
    G = case["groups"]
    assert d["groups"] == G and d["length"] == case["length"] and d["variant"] == 0
    assert d["exhaustive"] == (1 if G else 0) and d["permutations"] == (math.factorial(G) if G else 0)
    assert d["bp_by_groups"].tolist() == case["bp_by_groups"]
    assert d["perm"].tolist() == case["perm"] and d["pan"].tolist() == case["pan"] and d["core"].tolist() == case["core"]
    gi.assert_restated(d, text, case["name"], case["group_of"])
    if G:
        gi.assert_exhaustive(d, case["name"])


def test_the_example_of_the_definitions():
    d = growth(GFA["three_paths_layout"], TWIN)
    assert d["perm"][0].tolist() == [0, 1, 2] and d["pan"][0].tolist() == [10, 10, 10] and d["core"][0].tolist() == [10, 8, 7]


@pytest.mark.parametrize("G", [1, 2, 3, 4, 5, 6])
def test_exhaustive_rows_satisfy_the_integer_identity(G):
    for seed in (1, 2):
        text = gi.small_random(G, seed)
        d = growth(text, TWIN)                       # G! <= 1000: exhaustive
        gi.assert_exhaustive(d, f"G={G} seed={seed}")
        gi.assert_invariants(d)
        gi.assert_restated(d, text, f"G={G} seed={seed}")
    # G! above the permutations asked for: sampled
    if G >= 4:
        d = growth(gi.small_random(G, 1), TWIN, permutations=math.factorial(G) - 1)
        assert d["exhaustive"] == 0 and d["permutations"] == math.factorial(G) - 1


def test_exhaustive_needs_at_most_8_groups():
    text = gi.small_random(9, 1)
    d = growth(text, TWIN, permutations=50)
    assert d["exhaustive"] == 0 and d["permutations"] == 50
    d = growth(gi.small_random(7, 1), TWIN, permutations=5040)
    gi.assert_exhaustive(d, "G=7")


SAMPLED = [(n, t) for n, t in INPUTS if n in ("random:3", "random:4", "random:5", "random:6", "random:9", "hand:node_of_70000_bp",
                                              "hand:empty_and_one_step_paths", "hand:nodes_on_no_path")]


@pytest.mark.parametrize("name,text", SAMPLED, ids=[n for n, _ in SAMPLED])
def test_identities_with_graph_stats(name, text):
    gs = graph_stats(text, TWIN)
    d = growth(text, TWIN, permutations=40)
    shared = gs["shared"]
    assert d["bp_by_groups"].tolist() == gs["bp_by_paths"].tolist()
    for r in range(d["permutations"]):
        a = int(d["perm"][r, 0])
        assert int(d["pan"][r, 0]) == int(d["core"][r, 0]) == int(shared[a, a])
        if d["groups"] >= 2:
            b = int(d["perm"][r, 1])
            assert int(d["core"][r, 1]) == int(shared[a, b])
            assert int(d["pan"][r, 1]) == int(shared[a, a]) + int(shared[b, b]) - int(shared[a, b])


@pytest.mark.parametrize("name,text", INPUTS, ids=[n for n, _ in INPUTS])
def test_invariants_and_restatement(name, text):
    big = name in ("random:7", "random:8")
    d = growth(text, TWIN, permutations=12 if big else 70)
    gi.assert_invariants(d, name)
    gi.assert_restated(d, text, name, rows=[0, d["permutations"] - 1] if big and d["permutations"] else None)
    gi.assert_same(growth(text, TWIN, permutations=12 if big else 70), d, name + " (run to run)")
    if d["groups"] >= 4 and not d["exhaustive"]:
        other = growth(text, TWIN, permutations=12 if big else 70, seed=7)
        assert other["perm"].tolist() != d["perm"].tolist(), "two seeds drew the same orders"
        gi.assert_invariants(other, name)


@pytest.mark.parametrize("mode", ["sample", "haplotype"])
def test_groups_of_several_paths(mode):
    text = gi.rename_paths(st_random(12), gi.PANSN)
    group_of, names = growth_groups(gi.PANSN, mode)
    want_of, want_names = gi.groups_of(gi.PANSN, mode)
    assert group_of.tolist() == want_of and names == want_names
    assert len(names) == {"sample": 5, "haplotype": 8}[mode]         # counted by hand from gi.PANSN
    d = growth(text, TWIN, group_by=mode, permutations=60)
    assert d["groups"] == len(names) and d["paths"] == 12
    gi.assert_invariants(d, mode)
    gi.assert_restated(d, text, mode, want_of)
    gi.assert_same(growth(text, TWIN, permutations=60, group_of=want_of), d, mode)
    assert growth_groups(gi.PANSN, "path")[0].tolist() == list(range(12))
    assert growth_groups([], "sample")[1] == []


def st_random(P):
    import stats_helpers as st
    return st.random_gfa(77, 60, P, 25)


def test_sampled_order_is_the_rule():
    """permutation r orders the groups by (splitmix64(splitmix64(seed, r), g), g): restated on Python ints"""
    M = (1 << 64) - 1

    def mix(seed, idx):
        z = (seed + (idx + 1) * 0x9E3779B97F4A7C15) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)
    d = growth(st_random(12), TWIN, permutations=9, seed=5)
    for r in range(9):
        assert d["perm"][r].tolist() == sorted(range(12), key=lambda g: (mix(mix(5, r), g), g))


EXPECT_BP = [[0, 5], [3, 0, 9], [0, 0, 3, 7], [1, 7, 2, 0, 0], [4, 100, 0, 37, 0, 2 ** 31 - 200],
             [int(x) for x in np.random.default_rng(3).integers(0, 10 ** 6, size=131)]]


@pytest.mark.parametrize("bp", EXPECT_BP, ids=[f"G={len(b) - 1}" for b in EXPECT_BP])
def test_expected_against_exact_rationals(bp):
    pan, core = growth_expected(bp)
    G = len(bp) - 1
    assert len(pan) == len(core) == G
    for k in range(1, G + 1):
        ep, ec = gi.expected_exact(bp, k)
        assert abs(pan[k - 1] - float(ep)) <= 1e-12 * float(ep) and abs(core[k - 1] - float(ec)) <= 1e-12 * float(ec), k


def test_expected_at_4096_groups():
    G = 4096
    bp = [0] * (G + 1)
    for c, v in ((1, 12345), (2, 777), (100, 31), (4000, 99), (4095, 5), (4096, 1000)):
        bp[c] = v
    pan, core = growth_expected(bp)
    for k in (1, 2, 3, 64, 97, 1000, 4000, 4095, 4096):
        ep, ec = gi.expected_exact(bp, k)
        assert abs(pan[k - 1] - float(ep)) <= 1e-12 * float(ep) and abs(core[k - 1] - float(ec)) <= 1e-12 * float(ec), k


def test_expected_is_the_mean_of_all_orders():
    d = growth(gi.small_random(5, 3), TWIN)
    pan, core = growth_expected(d["bp_by_groups"])
    assert np.allclose(pan, d["pan"].mean(axis=0), rtol=1e-12) and np.allclose(core, d["core"].mean(axis=0), rtol=1e-12, atol=1e-12)


def _polyfit(pan_exp):
    new = np.diff(np.asarray(pan_exp, dtype=np.float64))
    k = np.arange(2, len(pan_exp) + 1, dtype=np.float64)
    use = new > 0
    slope, icept = np.polyfit(np.log(k[use]), np.log(new[use]), 1)
    return -slope, math.exp(icept), int(use.sum())


def test_fit_against_polyfit():
    rng = np.random.default_rng(5)
    curves = [np.cumsum(1000.0 * np.arange(1, 60) ** -0.5), np.cumsum(rng.uniform(0.5, 50.0, size=4096)),
              np.cumsum(np.where(np.arange(40) % 3 == 0, 0.0, rng.uniform(1, 9, size=40))),                 # points skipped
              growth_expected(growth(st_random(12), TWIN)["bp_by_groups"])[0]]
    for pe in curves:
        alpha, kappa, points = growth_fit(pe)
        a, k, n = _polyfit(pe)
        assert points == n and abs(alpha - a) <= 1e-9 and abs(kappa - k) <= 1e-9 * k
    alpha, kappa, points = growth_fit(curves[0])
    assert abs(alpha - 0.5) <= 1e-12 and points == 58 and abs(kappa - 1000.0) <= 1e-9 * 1000.0


def test_no_fit_below_two_points():
    for pe in ([5.0], [5.0, 6.0], [9.0, 9.0, 9.0, 9.0], [1.0, 2.0, 2.0, 2.0, 1.5]):
        assert growth_fit(pe)[2] < 2
    one = "H\tVN:Z:1.0\nS\t1\tACGT\nS\t2\tGG\nP\ta\t1+,2+\t*\n"
    two = one + "P\tb\t1+\t*\n"
    core = "H\tVN:Z:1.0\nS\t1\tACGT\nS\t2\tGG\n" + "".join(f"P\tp{k}\t1+,2-\t*\n" for k in range(5))
    for text, G in ((one, 1), (two, 2), (core, 5)):
        rep = growth_report(text, TWIN)
        assert f"groups={G}\t" in rep and "alpha=NA\tkappa=NA\t" in rep and rep.split("\n")[2].endswith("\tNA")


REPORT_CASES = ["golden:three_paths_layout", "golden:loops_and_pieces", "random:3", "random:5", "hand:node_of_70000_bp", "golden:empty_graph"]


@pytest.mark.parametrize("name", REPORT_CASES)
def test_report_bytes(name):
    text = dict(INPUTS)[name]
    with Growth(text, TWIN, permutations=130, seed=3) as g:
        d, rep = g.as_dict(), g.report()
    pan_exp, core_exp = growth_expected(d["bp_by_groups"])
    assert rep == gi.report_of(d, pan_exp, core_exp, growth_fit(pan_exp)), name
    assert rep == growth_report(text, TWIN, permutations=130, seed=3) and "seed=3\t" in rep
    if name == "random:5":
        assert "\topen\n" in rep or "\tclosed\n" in rep


def _error_of(fn):
    """-> (status, sr_last_error()) of a call that must fail"""
    with pytest.raises(SeqRushError) as e:
        fn()
    msg = _lib.load().sr_last_error().decode()
    assert msg and msg in str(e.value)
    return e.value.code, msg


def test_errors_and_limits():
    text = GFA["three_paths_layout"]
    many = "H\tVN:Z:1.0\nS\t1\tAC\n" + "".join(f"P\tp{k}\t1+\t*\n" for k in range(4097))
    code, msg = _error_of(lambda: growth(many, TWIN))
    assert code == -6 and "4097 groups" in msg                       # SR_ERR_UNSUPPORTED
    assert growth(many.rsplit("P\t", 1)[0], TWIN, permutations=3)["groups"] == 4096
    g97 = "H\tVN:Z:1.0\nS\t1\tAC\n" + "".join(f"P\tp{k}\t1+\t*\n" for k in range(97))
    code, msg = _error_of(lambda: growth(g97, TWIN, permutations=172961))      # 97 x 172961 = 2^24 + 1
    assert code == -6 and "2^24" in msg
    assert 97 * 172961 == 2 ** 24 + 1 and growth(g97, TWIN, permutations=172960)["permutations"] == 172960
    code, msg = _error_of(lambda: growth(text, TWIN, permutations=0))
    assert code == -1 and "permutations" in msg                      # SR_ERR_INVALID
    code, msg = _error_of(lambda: growth(text, TWIN, group_of=[0, 3, 1], n_groups=3))
    assert code == -1 and "group 3" in msg
    code, msg = _error_of(lambda: growth(text, TWIN, group_of=[0, 2, 2], n_groups=3))
    assert code == -1 and "group 1 has no path" in msg
    code, _ = _error_of(lambda: growth(text, -2))
    assert code == -1
    with pytest.raises(SeqRushError):
        growth(text, TWIN, group_by="genome")
    for empty in (GFA["empty_graph"], "H\tVN:Z:1.0\nS\t1\tACG\nS\t2\tT\nL\t1\t+\t2\t+\t0M\n"):
        d = growth(empty, TWIN)
        assert d["groups"] == d["permutations"] == d["paths"] == 0 and d["pan"].shape == (0, 0)
        assert d["bp_by_groups"].tolist() == [d["length"]]
        rep = growth_report(empty, TWIN)
        assert rep.count("\n") == 4 and "alpha=NA" in rep


def test_growth_command_line_writes_the_bytes_of_the_api(tmp_path):
    text = gi.rename_paths(st_random(12), gi.PANSN)
    gfa, out = tmp_path / "g.gfa", tmp_path / "g.tsv"
    gfa.write_text(text)
    env = dict(os.environ, PYTHONPATH=ROOT)
    tool = [sys.executable, "-m", "seqrush_amd.growth", str(gfa), "--device", "-1"]
    r = subprocess.run(tool + ["-o", str(out)], capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert out.read_text() == growth_report(text, TWIN)
    r = subprocess.run(tool + ["--group-by", "sample", "--permutations", "33", "--seed", "4"], capture_output=True, text=True, cwd=ROOT,
                       env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == growth_report(text, TWIN, group_by="sample", permutations=33, seed=4) and "groups=5\t" in r.stdout
    r = subprocess.run(tool + ["--permutations", "0"], capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
    assert r.returncode == 1 and "permutations" in r.stderr


EXE = os.path.join(ROOT, "seqrush_amd", "seqrush_mi355x")
BAD_FLAGS = [(["--growth", "g.tsv", "--growth-permutations", "0"], "--growth-permutations needs a positive integer"),
             (["--growth-seed", "3"], "--growth-seed is an option of --growth"),
             (["--growth-group-by", "sample", "--bin", "b.tsv"], "--growth-group-by is an option of --growth")]


@pytest.mark.parametrize("flags,message", BAD_FLAGS, ids=[" ".join(f) for f, _ in BAD_FLAGS])
def test_both_front_ends_refuse_the_same_flags(flags, message, tmp_path):
    fa = tmp_path / "in.fa"
    fa.write_text(">a\nACGT\n")
    env = dict(os.environ, PYTHONPATH=ROOT)
    for cmd in ([EXE], [sys.executable, "-m", "seqrush_amd"]):       # refused while the arguments are read: no device is opened
        r = subprocess.run(cmd + ["-s", str(fa), "-o", str(tmp_path / "o.gfa"), "--no-sort"] + flags, capture_output=True, text=True,
                           cwd=ROOT, env=env, timeout=300)
        assert r.returncode == 1 and message in r.stderr, (cmd, r.returncode, r.stderr[-500:])
