"""CPU tests (-m "not gpu") of the interval lift through the host twin (device = -1): known answers
with lines worked out by hand, a restatement of the rule in Python base by base, how the BED lines are read, and the
properties that prove the rule: a duplicate of the query path returns the interval, its reverse complement the mirrored
interval, every lifted base of the committed SNP graphs is the same base, and a whole path covers exactly the bases of the
nodes it shares."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import growth_inputs as gi
import lift_inputs as li
import variants_inputs as vi
from seqrush_amd.seqrush import Lift, SeqRushError, lift, lift_bed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOWN = json.load(open(os.path.join(ROOT, "tests", "golden", "lift_known_answers.json")))["cases"]
TWIN = -1
INPUTS = gi.host_inputs() + vi.bubble_inputs()
# worked out by hand on the graph of the known answers (a = 1+ 2+ 3+ 4+ 5+, b = 5- 4- 3- 1-, c = 1+ 3+ 6+ 3+ 5+)
HAND = ["b\t8\t10\tgeneA\t2\t-\ta\t2\t5\t2\n", "c\t2\t4\tgeneA\t2\t+\ta\t2\t5\t0\n", "c\t0\t15\ta:0-13\t10\t+\ta\t0\t13\t0\n",
        "a\t4\t7\ttwice\t4\t+\tc\t5\t11\t0\n", "b\t8\t9\tsecond_visit\t1\t-\tc\t8\t9\t1\n", "a\t0\t1\tb:11-12\t1\t-\tb\t11\t12\t1\n"]


@pytest.mark.parametrize("case", KNOWN, ids=[c["name"] for c in KNOWN])
def test_known_answers(case):
    with Lift(case["gfa"], case["bed"], TWIN, **case["kw"]) as v:
        d, out = v.as_dict(), v.bed()
    assert d["variant"] == 0 and (d["short_pairs"], d["long_pairs"]) == (0, 0)
    li.assert_same(d, case["expect"], case["name"])
    assert out == case["out"]
    rule = {k: x for k, x in case["kw"].items() if k == "to"}
    li.assert_same(d, li.restate(case["gfa"], case["bed"], **rule), case["name"])


def test_the_known_answers_cover_what_they_name():
    by = {c["name"]: c for c in KNOWN}
    every = by["all_targets"]
    for line in HAND:
        assert line in every["out"]
    assert every["out"].count("geneA") == 4                     # a query given twice is answered twice
    assert (every["expect"]["queries"], every["expect"]["unknown"], every["expect"]["out_of_range"]) == (9, 1, 3)
    assert "alone" in every["expect"]["labels"] and "alone" not in every["out"] and "snp" not in every["out"]
    assert not any(line.split("\t")[0] in ("e", "z") for line in every["out"].splitlines())
    assert all(line.split("\t")[0] != line.split("\t")[6] for line in every["out"].splitlines())
    assert "b\t0\t12\twhole_b\t12\t+\tb\t0\t12\t0\n" in by["to_b"]["out"]       # the own path, when it was asked for
    assert "a\t4\t7\ttwice\t4\t+\tc\t5\t11\t0\n" in by["to_own_path"]["out"]
    assert set(by["min_covered_3"]["out"].splitlines()) == {x for x in every["out"].splitlines() if int(x.split("\t")[4]) >= 3}
    assert by["empty_graph"]["out"] == by["empty_bed"]["out"] == "" and by["empty_graph"]["expect"]["unknown"] == 13


@pytest.mark.parametrize("name,text", INPUTS, ids=[n for n, _ in INPUTS])
def test_twin_equals_the_restatement(name, text):
    names = li.names_of(text)
    bed = li.random_bed(text, len(name))
    for to in ([None] if not names else [None, names[-1]]):
        with Lift(text, bed, TWIN, to) as v:
            d, out = v.as_dict(), v.bed()
        li.assert_same(d, li.restate(text, bed, to), f"{name} to={to}")
        assert out == li.report_of(d, names), f"{name} to={to}: bytes"
        assert d["unknown"] == 1


GFA = KNOWN[0]["gfa"]


def test_how_the_bed_lines_are_read():
    d = lift(GFA, "#c\ntrack a 1 2\nbrowser x\n\n  \na\t1\t2\r\na\t1\t2\tL\t0\t+\tmore\r\na 1 2 spaced rest\nq\t1\t2\na\t2\t2\na\t3\t2\na\t0\t14\n", TWIN)
    assert d["labels"] == ["a:1-2", "L", "spaced"] and (d["unknown"], d["out_of_range"]) == (1, 3)
    assert d["q_start"].tolist() == [1, 1, 1] and d["q_end"].tolist() == [2, 2, 2] and d["q_path"].tolist() == [0, 0, 0]
    assert lift(GFA, "a\t0\t13\n", TWIN)["queries"] == 1                           # end = plen is in range
    for bed, line, what in (("a\t1\n", 1, "fewer than three fields"), ("#x\n\na\t1\t2\na\tx\t2\n", 4, "start 'x' is not a number"),
                            ("a\t1\t2\nq\t1\t-2\n", 2, "end '-2' is not a number"), ("a\t1\t99999999999999999999\n", 1, "is not a number"),
                            ("nobody\t1.5\t2\n", 1, "start '1.5' is not a number"), ("a\n", 1, "fewer than three fields")):
        with pytest.raises(SeqRushError, match=f"BED line {line}: .*{what}") as e:
            lift(GFA, bed, TWIN)
        assert e.value.code == -1
        with pytest.raises(li.Invalid, match=f"BED line {line}: "):
            li.restate(GFA, bed)


def test_options_and_refusals():
    with pytest.raises(SeqRushError, match="no path is named 'nobody'") as e:
        lift(GFA, "a\t1\t2\n", TWIN, to="nobody")
    assert e.value.code == -1
    with pytest.raises(SeqRushError, match="no path is named 'a'"):
        lift("H\tVN:Z:1.0\n", "", TWIN, to="a")
    with pytest.raises(SeqRushError, match="device must be >= -1"):
        lift(GFA, "", -2)
    with pytest.raises(SeqRushError, match="min_covered"):
        lift(GFA, "", TWIN, min_covered=-1)
    from seqrush_amd import _lib
    L = _lib.load()
    prm = _lib.LiftParamsC()
    L.sr_lift_params_default(prm)
    assert (prm.to_name, prm.min_covered, prm.short_steps, prm.reserved) == (None, 1, 8, 0)
    assert L.sr_lift_gfa(None, None, prm, TWIN, None) != 0 and L.sr_abi_version() == 2
    for text, bed in (("", ""), ("H\tVN:Z:1.0\n", "a\t0\t1\n"), ("S\t1\tACGT\n", "a\t0\t1\n"), (GFA, ""), (GFA, "# none\n")):
        with Lift(text, bed, TWIN) as v:
            assert v.bed() == "" and v.as_dict()["queries"] == 0 and v.as_dict()["covered"].shape == (0, len(li.names_of(text)))


def test_the_limits_are_refused():
    paths = "".join(f"P\te{k}\t\t*\n" for k in range(2 ** 13))                 # 8193 targets with q
    text = "S\t1\tA\nP\tq\t1+\t*\n" + paths
    with pytest.raises(SeqRushError, match="8192 queries x 8193 targets; the tables support at most 2\\^26 pairs") as e:
        lift(text, "q\t0\t1\n" * 2 ** 13, TWIN)                                  # 2^26 + 2^13 pairs
    assert e.value.code == -6
    assert lift(text, "q\t0\t1\n" * 64, TWIN)["covered"].sum() == 64
    nodes = "".join(f"S\t{v}\tA\n" for v in range(1, 2 ** 15 + 2))              # 8193 x 32769 = 2^28 + 2^15 + 2^13 + 1
    with pytest.raises(SeqRushError, match="8193 targets x 32769 nodes; the first-visit table supports at most 2\\^28 entries") as e:
        lift(nodes + "P\tq\t1+\t*\n" + paths, "q\t0\t1\n", TWIN)
    assert e.value.code == -6
    assert lift(nodes + "P\tq\t1+\t*\n" + paths, "q\t0\t1\n", TWIN, to="q")["covered"].tolist() == [[1]]


# ------------------------------------------------------------------ the properties that prove the rule
def with_paths(text, extra):
    return text + "".join(f"P\t{n}\t" + ",".join(f"{h >> 1}{'-' if h & 1 else '+'}" for h in s) + "\t*\n" for n, s in extra)


def queries_of(text, name, seed, n=40):
    rng = np.random.default_rng(seed)
    L = li.step_starts(text, name)[-1]
    rows = [(name, 0, L), (name, 0, 1), (name, L - 1, L)]
    for _ in range(n):
        a = int(rng.integers(0, L))
        rows.append((name, a, int(rng.integers(a + 1, L + 1))))
    return li._bed(rows), rows, L


@pytest.mark.parametrize("seed", range(1, 7))
def test_a_duplicate_and_a_reverse_complement_of_the_query_path(seed):
    text = vi.bubbles(seed, 12 + seed, 3 + seed % 5, 2 + seed % 3)[0]
    g = vi.st.parse(text)
    for name, steps in g.paths:
        both = with_paths(text, [("same", steps), ("mirror", [h ^ 1 for h in reversed(steps)])])
        bed, rows, L = queries_of(both, name, seed)
        same, mirror = lift(both, bed, TWIN, to="same"), lift(both, bed, TWIN, to="mirror")
        assert same["queries"] == len(rows) == mirror["queries"]
        for i, (_, a, b) in enumerate(rows):
            assert [int(same[k][i, 0]) for k in li.FIELDS] == [a, b, b - a, 0], (name, a, b)
            assert [int(mirror[k][i, 0]) for k in li.FIELDS] == [L - b, L - a, b - a, b - a], (name, a, b)
        out = lift_bed(both, bed, TWIN, to="mirror").splitlines()
        assert len(out) == len(rows) and all(x.split("\t")[5] == "-" for x in out)
        assert all(x.split("\t")[5] == "+" for x in lift_bed(both, bed, TWIN, to="same").splitlines())


@pytest.mark.parametrize("file", ["layout_snp8_600.gfa", "layout_snp8_600_rc3.gfa"])
def test_every_lifted_base_is_the_same_base(file):
    text = open(os.path.join(ROOT, "tests", "golden", file)).read()
    g = vi.st.parse(text)
    spelled = [g.spell(s) for _, s in g.paths]
    names = [n for n, _ in g.paths]
    assert all(len(set(h >> 1 for h in s)) == len(s) for _, s in g.paths)      # no node is visited twice
    for a in (0, 2):
        bed = li._bed([(names[a], x, x + 1) for x in range(len(spelled[a]))])
        d = lift(text, bed, TWIN)
        assert d["queries"] == 600 and d["targets"] == 8
        for b in range(8):
            cov, at, rev = d["covered"][:, b], d["tstart"][:, b], d["rev_bp"][:, b]
            assert set(cov.tolist()) <= {0, 1} and ((d["tend"][:, b] - at)[cov == 1] == 1).all()
            for x in np.flatnonzero(cov):                        # every mapped pair, none excepted
                got = spelled[b][int(at[x])]
                assert (vi.sh.rc(got) if rev[x] else got) == spelled[a][x], (file, a, b, int(x))
            assert int(cov.sum()) >= 500, (file, a, b, int(cov.sum()))
            if b == a:
                assert cov.all() and (at == np.arange(600)).all() and not rev.any()


@pytest.mark.parametrize("name,text", INPUTS, ids=[n for n, _ in INPUTS])
def test_a_whole_path_covers_the_nodes_it_shares(name, text):
    g = vi.st.parse(text)
    names = [n for n, _ in g.paths]
    plen = li.path_lengths(text)
    rows = [(n, 0, plen[p]) for p, n in enumerate(names) if plen[p] and names.index(n) == p and n and not n.startswith(("#", "track", "browser"))]
    d = lift(text, li._bed(rows), TWIN)
    assert d["queries"] == len(rows)
    for i, (n, _, _) in enumerate(rows):
        for b, (_, steps) in enumerate(g.paths):
            on = {h >> 1 for h in steps}
            assert int(d["covered"][i, b]) == sum(len(g.seq[h >> 1]) for h in g.paths[names.index(n)][1] if h >> 1 in on), (name, n, b)


def _run(cmd, ok=True, **kw):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, **kw)
    assert (r.returncode == 0) == ok, r.stderr[-2000:]
    return r.stdout if ok else r.stderr


def test_the_tool_and_the_option_validation(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    gfa, bed, out = tmp_path / "g.gfa", tmp_path / "in.bed", tmp_path / "out.bed"
    gfa.write_text(GFA)
    bed.write_text(KNOWN[0]["bed"])
    tool = [sys.executable, "-m", "seqrush_amd.lift", str(gfa), "-b", str(bed), "--device", "-1"]
    _run(tool + ["-o", str(out)], cwd=ROOT, env=env)
    assert out.read_text() == KNOWN[0]["out"] == _run(tool, cwd=ROOT, env=env)
    _run(tool + ["-o", str(out), "--to", "b", "--min-covered", "2"], cwd=ROOT, env=env)
    assert out.read_text() == lift_bed(GFA, KNOWN[0]["bed"], TWIN, to="b", min_covered=2) != ""
    assert "no path is named 'zz'" in _run(tool + ["--to", "zz"], ok=False, cwd=ROOT, env=env)
    py = [sys.executable, "-m", "seqrush_amd", "-s", "x.fa"]
    exe = [os.path.join(ROOT, "seqrush_amd", "seqrush_mi355x"), "-s", "x.fa"]
    for front, kw in ((py, dict(cwd=ROOT, env=env)), (exe, {})):
        assert "Error: --lift needs --lift-out FILE" in _run(front + ["--no-sort", "--lift", "a.bed"], ok=False, **kw)
        for flag in ("--lift-out", "--lift-to", "--lift-min-covered"):
            assert f"Error: {flag} is an option of --lift: give both" in _run(front + ["--no-sort", flag, "5"], ok=False, **kw)
        assert "Error: --lift-min-covered needs a non-negative integer, got '-3'" in \
            _run(front + ["--no-sort", "--lift", "a.bed", "--lift-out", "o.bed", "--lift-min-covered", "-3"], ok=False, **kw)
