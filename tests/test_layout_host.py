"""Host tests of the 2-D layout: the host twin bit for bit against the Python restatement of
tests/layout_helpers.py, known answers, quality against the sequential yardstick, the command-line tool, argument errors.
No device needed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import layout_helpers as lh
import sort_helpers as sh
from seqrush_amd import layout as layout_tool
from seqrush_amd.seqrush import (SeqRushError, layout_gfa, layout_quality, layout_resolve, layout_select, layout_stats, layout_svg,
                                 layout_tsv)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWIN, SEQ = -1, -2
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "layout_known_answers.json")))


# ------------------------------------------------------------------------------------------ 1. restatement, bit for bit
HAND = [
    ("two_nodes", lh.two_nodes, dict(seed=77, iter_max=5, terms_per_round=7)),
    ("two_nodes_default", lh.two_nodes, {}),
    ("reverse_steps", lh.reverse_steps, dict(seed=5, iter_max=6, terms_per_round=16)),
    ("repeats_and_loop", lh.repeats_and_loop, dict(seed=9, iter_max=4, terms_per_round=3)),
    ("hub", lambda: lh.hub(6, 9), dict(seed=3, iter_max=4, terms_per_round=100)),
    ("chain", lambda: lh.chain(40), dict(seed=11, iter_max=3, terms_per_round=64)),
]


@pytest.mark.parametrize("name,make,params", HAND, ids=[c[0] for c in HAND])
def test_host_twin_matches_python_restatement(name, make, params):
    g = make()
    kw = dict(params)
    if "terms_per_round" not in kw:
        kw["terms_per_round"] = layout_resolve(g.text())["terms_per_round"]
    want = lh.Layout(g, **kw).run_batched()
    got = layout_gfa(g.text(), device=TWIN, **params)
    assert lh.words(got) == lh.words(want)
    assert lh.words(got) != lh.words(lh.initial_state(g, kw.get("seed", 9399220)))


def test_selection_matches_python_restatement():
    g = lh.reverse_steps()
    L = lh.Layout(g, seed=21)
    for k, cooling in ((0, False), (17, True)):
        got = layout_select(g.text(), k, 5, 200, cooling=cooling, seed=21)
        want = [L.select(k, 5 + t, cooling) for t in range(200)]
        assert got == want
        live = [s for s in got if s]
        if not cooling:
            assert any(s[0] ^ s[1] == 1 for s in live)                   # the two ends of one node: the length-holding term
        assert live and all(s[2] > 0 for s in live)


# ------------------------------------------------------------------------------------------ 2. known answers
def test_known_answers():
    text = GOLDEN["gfa"]
    assert text == lh.two_nodes().text()
    res = layout_resolve(text)
    assert res == GOLDEN["resolved"]
    assert res["eta_max"] == 7.0 ** 2 and res["min_term_updates"] == 10 * 2 and res["space"] == 7
    sel = [list(s) if s else None for s in layout_select(text, 0, 0, len(GOLDEN["selection_k0"]))]
    assert sel == GOLDEN["selection_k0"]
    sel = [list(s) if s else None for s in layout_select(text, 20, 0, len(GOLDEN["selection_k20_cooling"]), cooling=True)]
    assert sel == GOLDEN["selection_k20_cooling"]
    xy = layout_gfa(text, device=TWIN)
    assert [format(w, "016x") for w in lh.words(xy)] == GOLDEN["xy_words"]
    assert layout_tsv(xy) == GOLDEN["tsv"]
    assert layout_svg(text, xy) == GOLDEN["svg"]
    st = layout_stats()
    assert (st["terms_per_iter"], st["iterations"], st["subrounds_per_iter"], st["nodes"], st["steps"]) == (20, 31, 1, 2, 2)
    assert st["stage_ms"] >= st["sgd_ms"] >= 0


def test_tsv_and_svg_shape():
    g = lh.reverse_steps()
    xy = layout_gfa(g.text(), device=TWIN)
    rows = layout_tsv(xy).split("\n")
    assert rows[0] == "idx\tX\tY" and rows[-1] == "" and len(rows) == 2 * len(g.seq) + 2
    assert [r.split("\t")[0] for r in rows[1:-1]] == [str(i) for i in range(2 * len(g.seq))]
    assert rows[3] == "2\t%.4f\t%.4f" % (xy[1][0], xy[1][1])
    svg = layout_svg(g.text(), xy)
    assert svg.count("<line ") == len(g.seq) + len(set(g.edges))
    # the L line 2- -> 4+ leaves node 2 at its end point 0 and enters node 4 at its end point 0
    assert '<line x1="%.4f" y1="%.4f" x2="%.4f" y2="%.4f"/>' % (xy[1][0], xy[1][1], xy[3][0], xy[3][1]) in svg
    box = [float(v) for v in svg.split('viewBox="')[1].split('"')[0].split()]
    pts = xy.reshape(-1, 2)
    w, h = np.ptp(pts[:, 0]), np.ptp(pts[:, 1])
    assert box == pytest.approx([pts[:, 0].min() - 0.01 * w, pts[:, 1].min() - 0.01 * h, 1.02 * w, 1.02 * h], abs=1e-3)


# ------------------------------------------------------------------------------------------ 3. quality
# The yardstick's own seed-to-seed spread, (max - min) / mean of its stress over the seeds 9399220, 1, 2, 3, 4 with default
# parameters (DESIGN.md section 12 "Numbers"): 0.288 on the plain input, 0.177 on the one with reverse-complemented
# sequences.  The margin is twice that spread.  (The 1-D layout's 5 % is not copied.)
QUALITY = [("layout_snp8_600.gfa", 2 * 0.288), ("layout_snp8_600_rc3.gfa", 2 * 0.177)]


@pytest.mark.parametrize("name,margin", QUALITY, ids=[q[0] for q in QUALITY])
def test_quality_against_the_yardstick(name, margin):
    """synth.snp_family(8, 600, 0.05, 211) without and with rc_every=3, aligned, united, induced and compacted by the host
    oracle; the GFA text is committed"""
    text = open(os.path.join(ROOT, "tests", "golden", name)).read()

    def stress(xy):
        return layout_quality(text, xy, seed=1, samples=200000)["stress"]
    before = stress(lh.initial_state(sh.Gfa.parse(text)))
    twin = stress(layout_gfa(text, device=TWIN))
    yard = stress(layout_gfa(text, device=SEQ))
    print(f"{name}: stress initial {before:.6g} twin {twin:.6g} yardstick {yard:.6g}; initial / twin = {before / twin:.4g}")
    assert twin < before
    assert twin <= yard * (1.0 + margin)
    q = layout_quality(text, layout_gfa(text, device=TWIN), seed=1, samples=200000)
    assert 0 < q["pairs"] <= 200000


def test_quality_of_a_perfect_line_is_zero():
    g = lh.chain(20)
    L = lh.Layout(g, iter_max=2)
    xy = np.array([[p[0], 0.0] for p in L.xy]).reshape(-1, 4)        # every node on the x axis at its offset
    text = "\n".join(line for line in g.text().split("\n") if "\tb\t" not in line)    # path a alone: a line is exact
    q = layout_quality(text, xy, seed=3, samples=5000)
    assert q["stress"] == 0.0 and q["node_len_err"] == 0.0 and q["pairs"] > 0


# ------------------------------------------------------------------------------------------ 4. the tool
def _tool(args):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "seqrush_amd.layout"] + args, capture_output=True, text=True, timeout=120, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def test_tool_is_reproducible_and_follows_the_seed(tmp_path):
    gfa = tmp_path / "g.gfa"
    gfa.write_text(lh.reverse_steps().text())
    a, b, c, svg = (tmp_path / n for n in ("a.tsv", "b.tsv", "c.tsv", "a.svg"))
    out = _tool([str(gfa), "-o", str(a), "--svg", str(svg), "--device", "-1"])
    assert out == f"Layout written to {a}\n"
    _tool([str(gfa), "-o", str(b), "--device", "-1"])
    assert a.read_text() == b.read_text()                            # process to process
    assert layout_tool.main([str(gfa), "-o", str(c), "--device", "-1", "--seed", "4"]) == 0
    assert c.read_text() != a.read_text()
    xy = layout_gfa(gfa.read_text(), device=TWIN)
    assert a.read_text() == layout_tsv(xy) and svg.read_text() == layout_svg(gfa.read_text(), xy)
    assert layout_tool.main([str(gfa), "-o", str(c), "--device", "-1", "--iter-max", "3"]) == 0
    assert c.read_text() == layout_tsv(layout_gfa(gfa.read_text(), device=TWIN, iter_max=3))


def test_tool_graphs_without_terms_keep_the_initial_state(tmp_path):
    for name, text, g in (("empty", "H\tVN:Z:1.0\n", None), ("single", lh.single_steps().text(), lh.single_steps())):
        gfa, out = tmp_path / f"{name}.gfa", tmp_path / f"{name}.tsv"
        gfa.write_text(text)
        assert layout_tool.main([str(gfa), "-o", str(out), "--device", "-1"]) == 0
        want = lh.initial_state(g) if g else np.zeros((0, 4))
        assert out.read_text() == layout_tsv(want)
        assert lh.words(layout_gfa(text, device=SEQ)) == lh.words(want)
    assert out.read_text().split("\n")[1].startswith("0\t0.0000\t")


# ------------------------------------------------------------------------------------------ 5. argument errors
def test_bad_arguments_are_refused(tmp_path, capsys):
    text = lh.two_nodes().text()
    with pytest.raises(SeqRushError, match="device must be"):
        layout_gfa(text, device=-3)
    with pytest.raises(SeqRushError, match="number of nodes"):
        layout_gfa(text, n_nodes=3, device=TWIN)
    with pytest.raises(SeqRushError, match="iter_max"):
        layout_gfa(text, device=TWIN, iter_max=1)
    with pytest.raises(SeqRushError, match="number of nodes"):
        layout_svg(text, np.zeros((3, 4)))
    with pytest.raises(SeqRushError, match="number of nodes"):
        layout_quality(text, np.zeros((1, 4)))
    with pytest.raises(AttributeError):
        layout_gfa(text, device=TWIN, no_such_field=1)
    with pytest.raises(SeqRushError, match="GFA line"):
        layout_gfa("S\tx\tACGT\n", device=TWIN)
    gfa = tmp_path / "g.gfa"
    gfa.write_text(text)
    assert layout_tool.main([str(gfa), "-o", str(tmp_path / "o.tsv"), "--device", "-7"]) == 1
    assert "device must be" in capsys.readouterr().err
