"""CPU tests (-m "not gpu") of the subgraph extraction through the host twin (device = -1): known
answers with GFA texts worked out by hand, a restatement of the rule in Python, and the properties that prove the rule:
every subpath spells its interval of the source path, the whole of every path gives the input back, the kept set grows with
every option, a gap-closing distance of the longest allele leaves one subpath per path, the second round adds what the first
made possible, and every other stage accepts the result.  Then how region strings are read and what is refused."""
import json
import os
import subprocess
import sys

import pytest

import extract_inputs as ei
import growth_inputs as gi
import sort_helpers as sh
import stats_helpers as st
import variants_inputs as vi
from test_stage_refusals_host import EMPTY_SEQ, GOOD, NOT_DENSE
from seqrush_amd import _lib
from seqrush_amd.seqrush import Extract, SeqRushError, extract, extract_gfa, graph_stats, lift, path_bins, variants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
KNOWN = json.load(open(os.path.join(GOLDEN, "extract_known_answers.json")))
REFUSALS = os.path.join(GOLDEN, "extract_refusals.json")
TWIN = -1
INPUTS = gi.host_inputs() + [(n, ei.with_edges(t)) for n, t in vi.bubble_inputs()]
BUBBLES = [(n, ei.with_edges(t)) for n, t in vi.bubble_inputs()]
SNP = [(n, open(os.path.join(GOLDEN, n)).read()) for n in ("layout_snp8_600.gfa", "layout_snp8_600_rc3.gfa")]

# worked out by hand on the graph of the known answers (extract_inputs.KNOWN_GFA: a = 1+ 2+ 3+ 4+ 5+ with the step offsets
# 0 3 4 7 9, b = 5- 4- 3- 1- with 0 4 6 9, c = 1+ 3+ 6+ 3+ 5+ with 0 3 6 8 11)
HAND = {
    # the one base of node 2; no L line has both ends kept
    "node_2_alone": "H\tVN:Z:1.0\nS\t1\tT\nP\ta:3-4\t1+\t*\n",
    "node_6_alone": "H\tVN:Z:1.0\nS\t1\tAG\nP\tc:6-8\t1+\t*\n",
    # node 6 hangs on node 3 by two L lines: 3 becomes node 1 and 6 node 2; a and b pass node 3, c walks 3 6 3
    "node_6_with_context": "H\tVN:Z:1.0\nS\t1\tGGA\nS\t2\tAG\nL\t1\t+\t2\t+\t0M\nL\t2\t+\t1\t+\t0M\nP\ta:4-7\t1+\t*\nP\tb:6-9\t1-\t*\nP\tc:3-11\t1+,2+,1+\t*\n",
    # nodes 1 and 5 are seeds; a's gap 2 3 4 holds 6 bases and b's gap 4 3 holds 5, both close with D = 6; c's gap 3 6 3 holds 8
    # and stays open in the one round, so c is cut in two around node 6
    "ends_of_a_one_round": "H\tVN:Z:1.0\nS\t1\tACG\nS\t2\tT\nS\t3\tGGA\nS\t4\tCC\nS\t5\tTTTT\nL\t1\t+\t2\t+\t0M\nL\t2\t+\t3\t+\t0M\nL\t3\t+\t4\t+\t0M\n"
                           "L\t4\t+\t5\t+\t0M\nL\t1\t+\t3\t+\t0M\nP\ta:0-13\t1+,2+,3+,4+,5+\t*\nP\tb:0-12\t5-,4-,3-,1-\t*\nP\tc:0-6\t1+,3+\t*\nP\tc:8-15\t3+,5+\t*\n",
    # the whole of z: its node and the self-loop on it
    "whole_z": "H\tVN:Z:1.0\nS\t1\tCA\nL\t1\t+\t1\t+\t0M\nP\tz:0-2\t1+\t*\n",
}


def run(text, regions=(), bed=None, **kw):
    with Extract(text, regions, bed, TWIN, **kw) as v:
        return v.as_dict(), v.gfa()


# ------------------------------------------------------------------ 1. known answers and the restatement
@pytest.mark.parametrize("case", KNOWN["cases"], ids=[c["name"] for c in KNOWN["cases"]])
def test_known_answers(case):
    d, out = run(KNOWN["gfa"], tuple(case["regions"]), case["bed"], **case["kw"])
    assert d["variant"] == 0
    ei.assert_same(d, case["expect"], case["name"])
    assert out == case["out"]
    ei.assert_same(d, ei.restate(KNOWN["gfa"], tuple(case["regions"]), case["bed"], **ei.rule_kw(case["kw"])), case["name"])
    if case["name"] in HAND:
        assert out == HAND[case["name"]]


def test_the_known_answers_cover_what_they_name():
    assert KNOWN["gfa"] == ei.KNOWN_GFA and {c["name"] for c in KNOWN["cases"]} == set(ei.known_cases()) >= set(HAND) and len(HAND) >= 4
    by = {c["name"]: c["expect"] for c in KNOWN["cases"]}
    g = st.parse(KNOWN["gfa"])
    assert len(g.seq) == 8 and [n for n, _ in g.paths] == ["a", "b", "c", "e", "z"] and g.paths[3][1] == []
    assert all(h & 1 for h in g.paths[1][1]) and [h >> 1 for h in g.paths[2][1]].count(3) == 2
    assert by["ends_of_a_one_round"]["merge_rounds_run"] == 1 and by["ends_of_a_two_rounds"]["merge_rounds_run"] == 2
    assert by["ends_of_a_two_rounds"]["level"] == [0, 1, 1, 1, 0, 2, ei.NONE, ei.NONE]
    assert by["ends_of_a_default"]["level"] == [0, 1, 1, 1, 0, 1, ei.NONE, ei.NONE]
    assert by["context_reaches_node_8"]["level"][7] == 1 and by["bed_and_strings"]["unknown"] == 1 and by["bed_and_strings"]["out_of_range"] == 4
    assert by["every_path"]["out_of_range"] == 1 and by["every_path"]["sub_names"] == ["a:0-13", "b:0-12", "c:0-15", "z:0-2"]
    assert by["nothing"]["nodes"] == 0


@pytest.mark.parametrize("name,text", INPUTS, ids=[n for n, _ in INPUTS])
def test_twin_equals_the_restatement(name, text):
    regions, bed = ei.random_regions(text, len(name))
    for k, kw in enumerate(ei.OPTION_SETS):
        d, out = run(text, regions, bed, **kw)
        want = ei.restate(text, regions, bed, **ei.rule_kw(kw))
        ei.assert_same(d, want, f"{name} {kw}")
        assert out == ei.report_of(want, text), f"{name} {kw}: bytes"
        assert d["unknown"] == 1 and d["steps"] == d["sub_off"][-1]


# ------------------------------------------------------------------ 2. spelling
def check_spelling(text, d, out, what):
    """every subpath of the extracted text spells [start, end) of its source path: independent of the rule"""
    src, sub = st.parse(text), st.parse(out)
    assert len(sub.paths) == d["subpaths"]
    whole = {}
    for j, (name, steps) in enumerate(sub.paths):
        p, a, b = int(d["sub_path"][j]), int(d["sub_start"][j]), int(d["sub_end"][j])
        if p not in whole:
            whole[p] = src.spell(src.paths[p][1])
        assert name == f"{src.paths[p][0]}:{a}-{b}" and steps and sub.spell(steps) == whole[p][a:b], f"{what}: {name}"
    return sub


@pytest.mark.parametrize("name,text", INPUTS + SNP, ids=[n for n, _ in INPUTS + SNP])
def test_every_subpath_spells_its_interval(name, text):
    regions, bed = ei.random_regions(text, 7 + len(name))
    seen = 0
    for kw in ei.OPTION_SETS:
        d, out = run(text, regions, bed, **kw)
        seen += len(check_spelling(text, d, out, f"{name} {kw}").paths)
    assert seen > 0 or not ei.usable_names(text)


def test_reversed_paths_spell_their_interval():
    text = SNP[1][1]
    g = st.parse(text)
    rev = [n for n, s in g.paths if sum(h & 1 for h in s) * 2 > len(s)]
    assert rev
    d, out = run(text, (f"{rev[0]}:100-160",), None, merge_distance=5)
    sub = check_spelling(text, d, out, "rc3")
    assert {n.rpartition(":")[0] for n, _ in sub.paths} == {n for n, _ in g.paths}
    assert any(h & 1 for _, s in sub.paths for h in s)


# ------------------------------------------------------------------ 3. the whole graph
@pytest.mark.parametrize("name,text", BUBBLES + SNP, ids=[n for n, _ in BUBBLES + SNP])
def test_whole_paths_give_the_input_back(name, text):
    g = st.parse(text)
    d, out = run(text, tuple(n for n, _ in g.paths))
    sub = st.parse(out)
    plen = ei.path_lengths(text)
    assert [n for n, _ in sub.paths] == [f"{n}:0-{plen[p]}" for p, (n, _) in enumerate(g.paths)]
    ids = sorted(g.seq)
    old = {k + 1: ids[int(v) - 1] for k, v in enumerate(d["node_old"])}      # result id -> the id of the input's S line

    def h_old(h):
        return (old[h >> 1] << 1) | (h & 1)
    back = sh.Gfa({old[i]: s for i, s in sub.seq.items()}, [(h_old(a), h_old(b)) for a, b in sub.edges],
                  [(n.rpartition(":")[0], [h_old(h) for h in s]) for n, s in sub.paths])
    on_path = {h >> 1 for _, s in g.paths for h in s}          # a bubble graph holds alleles that no path took
    assert back.seq == {v: x for v, x in g.seq.items() if v in on_path} and back.paths == g.paths
    assert back.edges == [e for e in dict.fromkeys(g.edges) if e[0] >> 1 in on_path and e[1] >> 1 in on_path]
    assert (d["nodes"], d["steps"], d["subpaths"]) == (len(on_path), d["in_steps"], d["in_paths"])
    assert d["edges"] == d["in_edges"] or len(on_path) < d["in_nodes"]
    assert d["seeds"] == d["nodes"] and d["merge_rounds_run"] == 0


# ------------------------------------------------------------------ 4. monotone
@pytest.mark.parametrize("name,text", BUBBLES, ids=[n for n, _ in BUBBLES])
def test_the_kept_set_grows_with_every_option(name, text):
    regions, bed = ei.random_regions(text, 3)

    def kept(**kw):
        return {i for i, x in enumerate(extract(text, regions, bed, TWIN, **kw)["level"]) if x != ei.NONE}
    for key, values, rest in (("context_steps", (0, 1, 2, 5), dict(merge_distance=2)), ("merge_distance", (0, 1, 3, 10, 1000), dict(context_steps=1)),
                              ("merge_rounds", (0, 1, 2, 3), dict(merge_distance=2))):
        sets = [kept(**{key: v}, **rest) for v in values]
        assert all(a <= b for a, b in zip(sets, sets[1:])), key
        assert sets[0] < sets[-1] or key == "merge_rounds", key


# ------------------------------------------------------------------ 5. one subpath per path
@pytest.mark.parametrize("name,text", BUBBLES, ids=[n for n, _ in BUBBLES])
def test_the_longest_allele_as_distance_gives_one_subpath_per_path(name, text):
    names, plen = ei.names_of(text), ei.path_lengths(text)
    region = (f"{names[0]}:{plen[0] // 4}-{plen[0] - plen[0] // 4}",)
    d = extract(text, region, None, TWIN, merge_distance=5)
    per_path = [list(d["sub_path"]).count(p) for p in range(len(names))]
    assert max(per_path) == 1 and per_path[0] == 1
    per_path0 = [list(extract(text, region, None, TWIN, merge_distance=0)["sub_path"]).count(p) for p in range(len(names))]
    assert max(per_path0) > 1


# ------------------------------------------------------------------ 6. two rounds
def test_the_second_round_adds_what_the_first_made_possible():
    text, regions = ei.two_round_graph()
    s1, y1, x, y2, s2 = range(5)
    one = extract(text, regions, None, TWIN, merge_distance=5, merge_rounds=1)
    assert one["level"].tolist() == [0, ei.NONE, 1, ei.NONE, 0] and one["merge_rounds_run"] == 1
    two = extract(text, regions, None, TWIN, merge_distance=5, merge_rounds=2)
    assert two["level"].tolist() == [0, 2, 1, 2, 0] and two["merge_rounds_run"] == 2
    for R in (3, 64):
        more = extract(text, regions, None, TWIN, merge_distance=5, merge_rounds=R)
        ei.assert_same(more, two, f"R={R}")
    assert extract(text, regions, None, TWIN, merge_distance=5, merge_rounds=0)["level"].tolist() == [0, ei.NONE, ei.NONE, ei.NONE, 0]
    assert extract(text, regions, None, TWIN, merge_distance=2)["merge_rounds_run"] == 0
    assert extract(text, regions, None, TWIN, merge_distance=9)["level"].tolist() == [0, 1, 1, 1, 0]


# ------------------------------------------------------------------ 7. the result is a graph for every other stage
@pytest.mark.parametrize("name,text", BUBBLES + SNP[:1], ids=[n for n, _ in BUBBLES + SNP[:1]])
def test_the_other_stages_accept_the_result(name, text):
    names, plen = ei.names_of(text), ei.path_lengths(text)
    out = extract_gfa(text, (f"{names[0]}:{plen[0] // 3}-{plen[0] // 3 + 40}",), None, TWIN, context_steps=1, merge_distance=5)
    sub = st.parse(out)
    assert sorted(sub.seq) == list(range(1, len(sub.seq) + 1)) and sub.paths
    s = graph_stats(out, TWIN)
    assert (int(s["nodes"]), int(s["paths"]), int(s["steps"])) == (len(sub.seq), len(sub.paths), sum(len(x) for _, x in sub.paths))
    assert int(path_bins(out, TWIN, bins=4)["bins"]) == 4
    assert int(variants(out, TWIN)["paths"]) == len(sub.paths)
    first = sub.paths[0][0]
    assert int(lift(out, f"{first}\t0\t1\n", TWIN)["queries"]) == 1
    again = extract_gfa(out, (first,), None, TWIN)             # and the extraction itself
    assert first + ":0-" in again


# ------------------------------------------------------------------ 8. region strings, BED lines, the empty result
COLON = ("S\t1\tACGT\nS\t2\tGG\nS\t3\tT\nP\tchr1\t1+,2+,3+\t*\nP\tchr1:0-4\t2+,3+\t*\nP\th:1\t3+,1+\t*\nP\tnone\t\t*\nP\tchr1\t3+\t*\n")


def test_how_region_strings_are_read():
    d = extract(COLON, ("chr1:0-4",), None, TWIN, merge_distance=0)                 # a path has this very name: the name wins
    assert d["sub_names"] == ["chr1:4-7", "chr1:0-4:0-3", "h:1:0-1", "chr1:0-1"] and d["node_old"].tolist() == [2, 3]
    d = extract(COLON, ("chr1:0-3",), None, TWIN, merge_distance=0)                 # the first path of the name
    assert d["node_old"].tolist() == [1] and d["sub_names"] == ["chr1:0-4", "h:1:1-5"]
    d = extract(COLON, ("h:1:0-1", "h:1"), None, TWIN, merge_distance=0)            # a name with a colon, with and without a range
    assert d["regions"] == 2 and d["node_old"].tolist() == [1, 3]
    d = extract(COLON, ("none", "chr1:6-7"), None, TWIN)                              # the whole of a path without a base is out of range
    assert (d["regions"], d["out_of_range"], d["unknown"]) == (1, 1, 0)
    assert extract(COLON, "chr1:6-7", None, TWIN)["regions"] == 1                   # one string instead of a tuple
    for region, what in (("nobody", "region 'nobody': no path has this name"), ("chr1:5", "region 'chr1:5': '5' is not START-END"),
                         ("chr1:a-5", "'a-5' is not START-END"), ("chr1:1-", "'1-' is not START-END"), ("chr1:-1-5", "'-1-5' is not START-END"),
                         ("chr1:1-18446744073709551616", "is not START-END"), ("chr1:1-2-3", "'1-2-3' is not START-END"),
                         ("chr2:0-1", "region 'chr2:0-1': no path is named 'chr2'"), ("chr1:3-3", "region 'chr1:3-3': start must lie below end"),
                         ("chr1:4-3", "start must lie below end"), ("chr1:0-8", "region 'chr1:0-8': end lies beyond the 7 bases of the path"),
                         ("none:0-1", "end lies beyond the 0 bases of the path"), ("", "region '': no path has this name")):
        with pytest.raises(SeqRushError, match="extract: .*" + what.replace("'", ".")) as e:
            extract(COLON, (region,), None, TWIN)
        assert e.value.code == -1
        with pytest.raises(ei.Invalid, match=what.replace("'", ".")):
            ei.restate(COLON, (region,))


def test_how_the_bed_lines_are_read():
    bed = "#c\ntrack a 1 2\nbrowser x\n\n  \nchr1\t1\t2\r\nchr1\t1\t2\tL\t0\t+\tmore\r\nchr1 1 2 spaced rest\nq\t1\t2\nchr1\t2\t2\nchr1\t3\t2\nchr1\t0\t8\nnone\t0\t1\n"
    d = extract(COLON, (), bed, TWIN)
    assert (d["regions"], d["unknown"], d["out_of_range"]) == (3, 1, 4) and d["node_old"].tolist() == [1]
    ei.assert_same(d, ei.restate(COLON, (), bed))
    assert extract(COLON, (), "chr1\t0\t7\n", TWIN)["nodes"] == 3                   # end = plen is in range
    for text, line, what in (("chr1\t1\n", 1, "fewer than three fields"), ("#x\n\nchr1\t1\t2\nchr1\tx\t2\n", 4, "start 'x' is not a number"),
                             ("chr1\t1\t2\nq\t1\t-2\n", 2, "end '-2' is not a number"), ("chr1\t1\t99999999999999999999\n", 1, "is not a number"),
                             ("nobody\t1.5\t2\n", 1, "start '1.5' is not a number"), ("chr1\n", 1, "fewer than three fields")):
        with pytest.raises(SeqRushError, match=f"extract: BED line {line}: .*{what}") as e:
            extract(COLON, (), text, TWIN)
        assert e.value.code == -1
        with pytest.raises(ei.Invalid, match=f"BED line {line}: "):
            ei.restate(COLON, (), text)


def test_an_empty_result_is_the_header():
    for text, regions, bed in (("", (), None), ("H\tVN:Z:1.0\n", (), "a\t0\t1\n"), ("S\t1\tACGT\n", (), "a\t0\t1\n"), (COLON, (), None), (COLON, (), "# none\n"),
                               (COLON, ("none",), "nobody\t0\t1\nchr1\t9\t10\n")):
        d, out = run(text, regions, bed)
        assert out == "H\tVN:Z:1.0\n" and (d["nodes"], d["edges"], d["subpaths"], d["steps"], d["bases"]) == (0, 0, 0, 0, 0)
        assert d["level"].tolist() == [ei.NONE] * d["in_nodes"] and d["sub_off"].tolist() == [0]


def test_options_and_limits():
    L = _lib.load()
    prm = _lib.ExtractParamsC()
    L.sr_extract_params_default(prm)
    assert (prm.context_steps, prm.merge_distance, prm.merge_rounds, prm.reserved) == (0, 100000, 3, 0) and L.sr_abi_version() == 2
    assert L.sr_extract_gfa(None, None, None, 0, prm, TWIN, None) != 0
    with pytest.raises(SeqRushError, match="device must be >= -1"):
        extract(COLON, (), None, -2)
    with pytest.raises(SeqRushError, match="merge_distance"):
        extract(COLON, (), None, TWIN, merge_distance=-1)
    for kw, what in ((dict(context_steps=65536), "context_steps supports at most 65535"), (dict(merge_rounds=65), "merge_rounds supports at most 64")):
        with pytest.raises(SeqRushError, match=what) as e:
            extract(COLON, (), None, TWIN, **kw)
        assert e.value.code == -6
    assert extract(COLON, ("chr1:0-1",), None, TWIN, context_steps=65535, merge_rounds=64, merge_distance=2 ** 64 - 1)["nodes"] == 1


def test_more_than_2_24_regions_are_refused():
    with pytest.raises(SeqRushError, match="16777217 regions; at most 2\\^24 are supported") as e:
        extract("S\t1\tA\nP\ta\t1+\t*\n", (), "a\t0\t1\n" * (2 ** 24 + 1), TWIN)
    assert e.value.code == -6


# ------------------------------------------------------------------ 9. what is refused, and in which order
REFUSED = {
    "extract/not_dense": (NOT_DENSE, ("a",), {}),
    "extract/empty_sequence": (EMPTY_SEQ, ("a",), {}),
    "extract/empty_sequence_and_unknown_region": (EMPTY_SEQ, ("nobody:0-1",), {}),
    "extract/empty_sequence_and_bad_bed": (EMPTY_SEQ, (), dict(bed="a\t1\n")),
    "extract/context_cap_and_empty_sequence": (EMPTY_SEQ, ("a",), dict(context_steps=65536)),
    "extract/rounds_cap_and_empty_sequence": (EMPTY_SEQ, ("a",), dict(merge_rounds=65)),
    "extract/unknown_region": (GOOD, ("nobody:0-1",), {}),
    "extract/bad_bed_and_unknown_region": (GOOD, ("nobody:0-1",), dict(bed="a\t1\n")),
}
NO_DEVICE = {"extract/no_device": (GOOD, ("a",), {}), "extract/no_device_and_unknown_region": (GOOD, ("nobody:0-1",), {})}


def observe(text, regions, device, kw):
    kw = dict(kw)
    try:
        extract(text, regions, kw.pop("bed", None), device, **kw)
    except SeqRushError as e:
        return [e.code, _lib.load().sr_last_error().decode("latin-1")]
    return [0, ""]


def record():
    """the content of the golden file (json.dump(record(), ..., indent=1, sort_keys=True)), taken on a machine without a device"""
    out = {name: observe(text, regions, TWIN, kw) for name, (text, regions, kw) in REFUSED.items()}
    out.update({name: observe(text, regions, 0, kw) for name, (text, regions, kw) in NO_DEVICE.items()})
    return out


def test_the_record_of_refusals_holds_every_case():
    gold = json.load(open(REFUSALS))
    assert set(gold) == set(REFUSED) | set(NO_DEVICE)
    assert gold["extract/not_dense"] == [0, ""] and gold["extract/empty_sequence"] == [-1, "extract: a node has no sequence"]
    assert gold["extract/no_device"] == [-2, "extract: no HIP device (device -1 selects the host twin)"]
    assert gold["extract/no_device_and_unknown_region"][0] == -1            # the regions are read before a device is opened
    assert gold["extract/context_cap_and_empty_sequence"][0] == gold["extract/rounds_cap_and_empty_sequence"][0] == -6
    assert gold["extract/empty_sequence_and_bad_bed"] == gold["extract/empty_sequence"] == gold["extract/empty_sequence_and_unknown_region"]
    assert "BED line 1" in gold["extract/bad_bed_and_unknown_region"][1]


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_a_defect_is_refused_as_recorded(name):
    text, regions, kw = REFUSED[name]
    assert observe(text, regions, TWIN, kw) == json.load(open(REFUSALS))[name]


@pytest.mark.parametrize("name", sorted(NO_DEVICE))
def test_no_device_is_refused_as_recorded(name):
    if _lib.load().sr_device_count() > 0 and name == "extract/no_device":
        pytest.skip("a HIP device is present: device 0 is not refused")
    text, regions, kw = NO_DEVICE[name]
    assert observe(text, regions, 0, kw) == json.load(open(REFUSALS))[name]


# ------------------------------------------------------------------ 10. the tool
def test_the_tool_writes_the_bytes_of_extract_gfa(tmp_path):
    text = BUBBLES[2][1]
    names, plen = ei.names_of(text), ei.path_lengths(text)
    gfa, bed, out = tmp_path / "g.gfa", tmp_path / "in.bed", tmp_path / "sub.gfa"
    gfa.write_text(text)
    bed.write_text(f"{names[1]}\t3\t9\tlocus\n")
    region = f"{names[0]}:{plen[0] // 2}-{plen[0] // 2 + 6}"
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "seqrush_amd.extract", str(gfa), "-r", region, "-r", names[-1] + ":0-1", "-b", str(bed), "--device", "-1",
           "--context-steps", "1", "--merge-distance", "4", "--merge-rounds", "2"]
    r = subprocess.run(cmd + ["-o", str(out)], capture_output=True, text=True, timeout=120, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    want = extract_gfa(text, (region, names[-1] + ":0-1"), bed.read_text(), TWIN, context_steps=1, merge_distance=4, merge_rounds=2)
    assert out.read_text() == want and want.count("\nP\t") >= len(names)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=ROOT, env=env)
    assert r.returncode == 0 and r.stdout == want
    r = subprocess.run(cmd[:4] + ["-r", "nobody", "--device", "-1"], capture_output=True, text=True, timeout=120, cwd=ROOT, env=env)
    assert r.returncode == 1 and "region 'nobody'" in r.stderr
