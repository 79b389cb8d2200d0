"""CPU tests (-m "not gpu") of the statistics stage through the host twin (device = -1): hand-worked
known answers, the Python restatement of stats_helpers.py on random and hand-made graphs, the split sum of squares, the
layout metric against sort_helpers.quality, the report and the refusals.  Every comparison is exact."""
import json
import os

import pytest

import sort_helpers as sh
import stats_helpers as st
import test_sort_host as tsh
from seqrush_amd.seqrush import SeqRushError, graph_stats, graph_stats_report, stats_sq_sums_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "stats_known_answers.json")))["cases"]
TWIN = -1


def parse_report(text):
    """the report's rows by section -> {section: [fields after the section name]}"""
    out = {}
    for line in text.strip().split("\n"):
        if line.startswith("#"):
            continue
        f = line.split("\t")
        out.setdefault(f[0], []).append(f[1:])
    return out


def check_report(text, want, names):
    """every integer of the report equals `want` (a stats_helpers.as_plain dict)"""
    r = parse_report(text)
    kv = lambda sec: {f[0]: f[1] for f in r[sec]}    # noqa: E731
    P = want["paths"]
    assert {k: int(v) for k, v in kv("summary").items()} == {k: want[k] for k in ("length", "nodes", "edges", "paths", "steps")}
    s = kv("steps")
    assert int(s["rev_steps"]) == want["rev_steps"] and int(s["depth_bp"]) == want["depth_bp"]
    assert {k: int(v) for k, v in kv("topology").items()} == {k: want[k] for k in ("self_loops", "tips", "components")}
    cl = {f[0]: (int(f[1]), int(f[2])) for f in r["classes"]}
    assert cl["core"] == (want["bp_by_paths"][P], want["nodes_by_paths"][P])
    assert cl["unused"] == (want["bp_by_paths"][0], want["nodes_by_paths"][0])
    assert cl["private"] == ((want["bp_by_paths"][1], want["nodes_by_paths"][1]) if P >= 1 else (0, 0))
    bp, nd = [0] * (P + 1), [0] * (P + 1)
    for c, b, n in r.get("by_paths", []):
        bp[int(c)], nd[int(c)] = int(b), int(n)
    assert bp == want["bp_by_paths"] and nd == want["nodes_by_paths"]
    idx = {n: i for i, n in enumerate(names)}
    shared = [[0] * P for _ in range(P)]
    for a, b, v, jac in r.get("similarity", []):
        i, j = idx[a], idx[b]
        shared[i][j] = shared[j][i] = int(v)
        den = want["shared"][i][i] + want["shared"][j][j] - int(v)
        assert jac == ("NA" if den == 0 else f"{int(v) / den:.6f}")
    assert shared == want["shared"]
    rows = {f[0]: f[1:] for f in r.get("layout_path", [])}
    for p, n in enumerate(names):
        if want["path_pairs"][p] == 0:
            assert n not in rows
        else:
            assert [int(x) for x in rows[n][:4]] == [want[k][p] for k in ("path_pairs", "path_abs", "path_sq", "path_len")]
    lay = kv("layout")
    assert [int(lay[k]) for k in ("pairs", "sum_abs", "sum_sq", "path_length")] == \
        [want[k] for k in ("total_pairs", "total_abs", "total_sq", "total_len")]


@pytest.mark.parametrize("case", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_known_answers(case):
    got = graph_stats(case["gfa"], TWIN)
    st.assert_equal(got, case["expect"], case["name"])
    st.assert_equal(st.stats(st.parse(case["gfa"])), case["expect"], case["name"] + " (restatement)")
    text = graph_stats_report(case["gfa"], TWIN)
    check_report(text, st.as_plain(case["expect"]), [n for n, _ in st.parse(case["gfa"]).paths])
    if "report" in case:                             # the formulas of measure_layout_quality.rs:186-209, on paper
        r = parse_report(text)
        lay = {f[0]: f[1] for f in r["layout"]}
        want = case["report"]
        for k in ("mse", "rmse", "mae", "normalized_mse", "normalized_mae", "relative_error_pct"):
            assert lay[k] == want[k], k
        sim = {(f[0], f[1]): f[3] for f in r["similarity"]}
        assert sim[("x", "y")] == want["jaccard_x_y"] and sim[("y", "z")] == want["jaccard_y_z"]
        cl = {f[0]: f[1] for f in r["classes"]}
        assert (cl["core"], cl["private"], cl["unused"]) == (want["core_bp"], want["private_bp"], want["unused_bp"])


@pytest.mark.parametrize("seed,nodes,paths,steps", st.RANDOM_CASES)
def test_twin_matches_restatement_on_random_graphs(seed, nodes, paths, steps):
    text = st.random_gfa(seed, nodes, paths, steps, sparse_ids=seed % 2 == 0)
    want = st.stats(st.parse(text))
    assert want["nodes"] == nodes and want["paths"] == paths
    st.assert_equal(graph_stats(text, TWIN), want, f"seed {seed}")


@pytest.mark.parametrize("name", sorted(st.hand_cases()))
def test_twin_matches_restatement_on_hand_made_cases(name):
    text = st.hand_cases()[name]
    got, want = graph_stats(text, TWIN), st.stats(st.parse(text))
    st.assert_equal(got, want, name)
    if name == "node_of_70000_bp":
        assert any(int(row[0]) > 0 for row in got["path_sq_parts"]), "the high part of the square split stayed zero"
    if name == "three_components":
        assert got["components"] == 3
    if name == "duplicate_l_lines":
        assert got["edges"] == 2
    if name == "empty_and_one_step_paths":
        assert got["paths"] == 4 and [int(x) for x in got["path_pairs"]] == [0, 1, 0, 0]
    check_report(graph_stats_report(text, TWIN), st.as_plain(want), [n for n, _ in st.parse(text).paths])


def test_split_sum_of_squares_is_exact_beyond_64_bits():
    big = [2 ** 31 - 2] * 10
    mixed = [0, 1, 65535, 65536, 65537, 2 ** 31 - 2, 123456789, 2 ** 16 * 7 + 3, 2 ** 31 - 2, 2 ** 31 - 2, 2 ** 31 - 2, 2 ** 31 - 2, 99]
    for vals in (big, mixed, []):
        hh, hl, ll = stats_sq_sums_host(vals)
        assert hh == sum((e >> 16) ** 2 for e in vals) and hl == sum((e >> 16) * (e & 0xffff) for e in vals)
        assert ll == sum((e & 0xffff) ** 2 for e in vals)
        assert (hh << 32) + (hl << 17) + ll == sum(e * e for e in vals)
    assert sum(e * e for e in big) > 2 ** 64


def _sort_graphs():
    return [("small%d" % k, g) for k, g in enumerate(tsh._small_graphs())] + [(n, tsh.graph(n)[1]) for n in ("snp", "snp_rc", "indel")]


def test_mae_equals_sort_helpers_quality():
    for name, g in _sort_graphs():
        d = graph_stats(g.text(), TWIN)
        pairs, tot = d["total_pairs"], d["total_abs"]
        assert tot / max(pairs, 1) == sh.quality(g), name
        st.assert_equal(d, st.stats(g), name)


def test_report_is_reproducible_and_parses_back():
    text = st.random_gfa(11, 60, 5)
    a, b = graph_stats_report(text, TWIN), graph_stats_report(text, TWIN)
    assert a == b and a.startswith("#seqrush_amd graph statistics v1\n")
    g = st.parse(text)
    check_report(a, st.as_plain(st.stats(g)), [n for n, _ in g.paths])


def test_refusals():
    seg = "S\t1\tA\n"
    many = "H\tVN:Z:1.0\n" + seg + "".join(f"P\tp{k}\t1+\t*\n" for k in range(4097))
    with pytest.raises(SeqRushError) as e:
        graph_stats(many, TWIN)
    assert e.value.code == -6                        # SR_ERR_UNSUPPORTED
    ok = graph_stats("H\tVN:Z:1.0\n" + seg + "".join(f"P\tp{k}\t1+\t*\n" for k in range(4096)), TWIN)
    assert ok["paths"] == 4096 and int(ok["shared"][4095][0]) == 1 and int(ok["nodes_by_paths"][4096]) == 1
    with pytest.raises(SeqRushError) as e:
        graph_stats("H\tVN:Z:1.0\n" + seg + "P\tp\t1+,2+\t*\n", TWIN)
    assert e.value.code == -1 and "missing segment" in str(e.value)
    with pytest.raises(SeqRushError):
        graph_stats(seg, -2)
