"""GPU tests of the subgraph extraction: the HIP kernels against the host twin on every input of
test_extract_host.py and on graphs and regions built for the seams of the kernels (extract_inputs.seam_cases): one-base
regions on and beside step boundaries, 1 to 257 regions on a path, nested regions that only the prefix maximum covers, path
boundaries on and off a workgroup boundary of the scans, runs that must not merge, gaps of exactly D and D + 1 bases and of 1
to 1025 steps, context of 0 to 1000 steps with self-loops and reverse handles, the two-round graph, and chains of 1 to
65 538 nodes.  Device against twin is exact on every table, every counter and the GFA bytes, and so are the device run to
run and the device against the restatement in Python; both command lines, the tool and --gpus 2 write the same file."""
import functools
import json
import os
import subprocess
import sys

import pytest

import extract_inputs as ei
import growth_inputs as gi
import variants_inputs as vi
from seqrush_amd import synth
from seqrush_amd.seqrush import Extract, extract_gfa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "seqrush_amd", "seqrush_mi355x")
KNOWN = json.load(open(os.path.join(ROOT, "tests", "golden", "extract_known_answers.json")))
TWIN = -1
INPUTS = gi.host_inputs() + [(n, ei.with_edges(t)) for n, t in vi.bubble_inputs()]
SEAMS = ei.seam_cases()


def check(text, regions, bed, what, **kw):
    """device against twin, run to run and against the restatement -> the device result"""
    with Extract(text, regions, bed, TWIN, **kw) as v:
        twin, twin_out = v.as_dict(), v.gfa()
    want = ei.restate(text, regions, bed, **ei.rule_kw(kw))
    runs = []
    for _ in range(2):
        with Extract(text, regions, bed, 0, **kw) as v:
            runs.append((v.as_dict(), v.gfa()))
    (dev, out), (again, out2) = runs
    assert dev["variant"] == 1 and twin["variant"] == 0
    ei.assert_same(dev, twin, f"{what} (device against twin)")
    assert out == twin_out, f"{what}: bytes"
    ei.assert_same(dev, want, f"{what} (device against restatement)")
    assert out == ei.report_of(want, text), f"{what}: bytes against the restatement"
    ei.assert_same(again, dev, f"{what} (device run to run)")
    assert out2 == out
    return dev


@pytest.mark.gpu
@pytest.mark.parametrize("case", KNOWN["cases"], ids=[c["name"] for c in KNOWN["cases"]])
def test_device_gives_the_known_answers(gpu, case):
    dev = check(KNOWN["gfa"], tuple(case["regions"]), case["bed"], case["name"], **case["kw"])
    ei.assert_same(dev, case["expect"], case["name"])


@pytest.mark.gpu
@pytest.mark.parametrize("name,text", INPUTS, ids=[n for n, _ in INPUTS])
def test_device_equals_twin_on_the_host_inputs(gpu, name, text):
    regions, bed = ei.random_regions(text, len(name))
    for kw in ei.OPTION_SETS:
        dev = check(text, regions, bed, f"{name} {kw}", **kw)
        if dev["regions"]:
            assert dev["extract_us"] > 0


@functools.lru_cache(maxsize=None)
def seam(name):
    text, regions, bed, kw = SEAMS[name]
    return check(text, regions, bed, name, **kw)


def kept(dev):
    return [i + 1 for i, x in enumerate(dev["level"]) if x != ei.NONE]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SEAMS))
def test_device_equals_twin_on_the_seams(gpu, name):
    dev = seam(name)
    text, regions, bed, kw = SEAMS[name]
    if name.startswith("one_step_"):
        want = {"first_base": [5], "last_base": [5], "before": [4], "behind": [6], "ends_at_boundary": [4], "starts_at_boundary": [6], "inside": [5]}
        assert kept(dev) == want[name[len("one_step_"):]]
    if name.startswith("regions_"):
        assert dev["regions"] == int(name.split("_")[1]) and dev["seeds"] == dev["nodes"] > 0
    if name == "nested_regions":
        assert kept(dev) == list(range(1, 26)) + [31] and dev["regions"] == 7          # steps 13 .. 25 only by the long region
    if name == "nested_regions_sorted_late":
        assert kept(dev) == list(range(2, 26))
    if name == "no_kept_step_between":
        assert sorted(set(dev["sub_path"].tolist())) == [0, 2]            # p1 lies between them, p3 shares nothing
    if name == "empty_path_named":
        assert (dev["regions"], dev["out_of_range"]) == (1, 2)
    if name.startswith("adjacent_paths_"):
        n0 = int(name.split("_")[2])
        first = dev["sub_path"].tolist().index(1)
        assert dev["sub_path"].tolist()[first - 1] == 0 and int(dev["sub_end"][first - 1]) == n0 and int(dev["sub_start"][first]) == 0
        assert dev["subpaths"] == 2 and int(dev["sub_off"][first]) == (n0 if name.endswith("wide") else 1) and dev["steps"] == int(dev["sub_off"][first]) + (2 if name.endswith("wide") else 1)
    if name == "runs_at_both_ends":
        assert kept(dev) == list(range(5, 11)) and dev["by_merge"] == 0 and dev["sub_names"] == ["a:8-20", "b:8-20"]
    if name == "neighbour_in_another_path":
        assert kept(dev) == [3, 18] and dev["merge_rounds_run"] == 0 and dev["subpaths"] == 2
    if name == "neighbour_in_another_path_and_own":
        assert kept(dev) == [3] + list(range(11, 19)) and dev["merge_rounds_run"] == 1
    if name == "gap_of_D":
        assert kept(dev) == [1, 2, 3, 4, 5] and dev["by_merge"] == 3
    if name == "gap_of_D_plus_1":
        assert kept(dev) == [1, 5] and dev["by_merge"] == 0 and dev["subpaths"] == 2
    if name == "gap_D_0":
        assert kept(dev) == [1, 3] and dev["merge_rounds_run"] == 0
    if name.startswith("gap_of_") and name.endswith("_steps"):
        n = int(name.split("_")[2])
        assert dev["by_merge"] == n and dev["nodes"] == n + 2 and dev["subpaths"] == 1 and dev["merge_rounds_run"] == 1
    if name.startswith("context_") and name != "context_without_L_lines":
        c = int(name.split("_")[1])
        assert (dev["by_context"] > 0) == (c > 0) and max(x for x in dev["level"].tolist() if x != ei.NONE) <= c
        if c == 1000:
            assert dev["nodes"] > seam("context_2")["nodes"] > seam("context_1")["nodes"] > seam("context_0")["nodes"]
    if name == "context_without_L_lines":
        assert dev["by_context"] == 0 and dev["in_edges"] == 0
    if name.startswith("loops_and_reverse_edges_c"):
        c = int(name[-1])
        assert kept(dev) == [2, 3, 4, 5][:c + 1] and dev["level"].tolist()[1:c + 2] == list(range(c + 1))       # node 6 hangs on its own loop only
    if name.startswith("two_rounds_R"):
        assert dev["level"].tolist() == ([0, ei.NONE, 1, ei.NONE, 0] if name.endswith("R1") else [0, 2, 1, 2, 0])
        assert dev["merge_rounds_run"] == min(2, int(name.split("R")[1]))
    if name == "visited_three_times":
        assert kept(dev) == [2] and dev["sub_names"] == ["a:2-5", "a:6-9", "a:11-14", "b:0-3"]
    if name == "visited_three_times_merged":
        assert kept(dev) == [2, 3] and dev["merge_rounds_run"] == 1        # node 3 (1 base) closes, node 4 (2 bases) does not
    if name.startswith("chain_") and name[6:].isdigit():
        n = int(name[6:])
        assert (dev["in_nodes"], dev["in_steps"], dev["in_edges"]) == (n, n, n - 1) and dev["edges"] == dev["nodes"] - dev["subpaths"]
    if name == "chain_65537_merged":
        assert dev["nodes"] == 65537 and dev["by_merge"] == 65534 and dev["subpaths"] == 1
    if name == "chain_65537_whole":
        assert dev["seeds"] == 65537 and dev["sub_names"] == ["a:0-65537"]


def write_fasta(path, recs):
    path.write_bytes(b"".join(b">" + n.encode() + b"\n" + s + b"\n" for n, s in recs))


def _run(cmd, **kw):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, **kw)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def regions_of(recs):
    return [f"{recs[0][0]}:100-140", f"{recs[1][0]}:250-251", recs[-1][0] + ":0-30"]


@pytest.mark.gpu
def test_both_command_lines_and_the_tool_write_the_same_files(gpu, tmp_path):
    recs = synth.snp_family(5, 400, 0.05, 97, rc_every=2)
    fa, bed = tmp_path / "in.fa", tmp_path / "in.bed"
    write_fasta(fa, recs)
    bed.write_text(f"# loci\n{recs[2][0]}\t300\t320\tgene\nchrUn\t0\t5\n")
    env = dict(os.environ, PYTHONPATH=ROOT)
    py = [sys.executable, "-m", "seqrush_amd"]
    regs = regions_of(recs)
    flags = [x for r in regs for x in ("--extract-region", r)]
    files = {}
    for tag, cmd, kw in (("c", [EXE], {}), ("p", py, dict(cwd=ROOT, env=env))):
        gfa, out, gfa2, out2 = (tmp_path / f"{tag}{x}" for x in (".gfa", ".sub.gfa", "_t.gfa", "_t.sub.gfa"))
        stdout = _run(cmd + ["-s", str(fa), "-o", str(gfa), "--sort", "--extract-out", str(out), "--extract-bed", str(bed), "-v"] + flags, **kw)
        assert f"Extracted graph written to {out}" in stdout and stdout.count("Extract stage:") == 1
        files[tag + "_line"] = next(x.split(" us on device")[1] for x in stdout.splitlines() if x.startswith("Extract stage:"))
        quiet = _run(cmd + ["-s", str(fa), "-o", str(gfa2), "--no-sort", "--extract-out", str(out2), "--extract-region", regs[0], "--extract-context-steps", "2",
                            "--extract-merge-distance", "3", "--extract-merge-rounds", "1"], **kw)
        assert "Extract stage:" not in quiet
        files[tag] = (gfa.read_text(), out.read_text(), gfa2.read_text(), out2.read_text())
    assert files["c"] == files["p"] and files["c_line"] == files["p_line"]
    text, text2 = files["c"][0], files["c"][2]
    assert files["c"][1] == extract_gfa(text, regs, bed.read_text(), TWIN) == extract_gfa(text, regs, bed.read_text(), 0)
    assert files["c"][1].count("\nP\t") >= len(recs)
    assert files["c"][3] == extract_gfa(text2, (regs[0],), None, TWIN, context_steps=2, merge_distance=3, merge_rounds=1) != files["c"][1]
    tool = tmp_path / "t.gfa"
    _run([sys.executable, "-m", "seqrush_amd.extract", str(tmp_path / "c.gfa"), "-b", str(bed), "--device", "0", "-o", str(tool)] + [x for r in regs for x in ("-r", r)],
         cwd=ROOT, env=env)
    assert tool.read_text() == files["c"][1]
    for cmd, kw in (([EXE], {}), (py, dict(cwd=ROOT, env=env))):           # usage errors, before any work
        for extra in (["--extract-region", regs[0]], ["--extract-out", str(tmp_path / "x.gfa")], ["--extract-merge-rounds", "2"]):
            r = subprocess.run(cmd + ["-s", str(fa), "-o", str(tmp_path / "u.gfa")] + extra, capture_output=True, text=True, timeout=600, **kw)
            assert r.returncode != 0 and "--extract" in r.stderr and not (tmp_path / "u.gfa").exists()


@pytest.mark.gpu
def test_extract_after_extend(gpu, tmp_path):
    recs = synth.snp_family(5, 400, 0.05, 97, rc_every=2)
    old, new = tmp_path / "old.fa", tmp_path / "new.fa"
    write_fasta(old, recs[:3])
    write_fasta(new, recs[3:])
    g0, g1, out = tmp_path / "g0.gfa", tmp_path / "g1.gfa", tmp_path / "sub.gfa"
    regs = regions_of(recs)
    _run([EXE, "-s", str(old), "-o", str(g0), "--no-sort"])
    _run([EXE, "-s", str(new), "-o", str(g1), "--no-sort", "--extend", str(g0), "--extract-out", str(out)] + [x for r in regs for x in ("--extract-region", r)])
    assert out.read_text() == extract_gfa(g1.read_text(), regs, None, TWIN)
    assert {x.split("\t")[1].rpartition(":")[0] for x in out.read_text().splitlines() if x[0] == "P"} == {n for n, _ in recs}


@pytest.mark.gpu
def test_multi_gpu_writes_the_file_once(gpu, tmp_path):
    recs = synth.snp_family(6, 500, 0.05, 711, rc_every=3)
    fa = tmp_path / "in.fa"
    write_fasta(fa, recs)
    env = dict(os.environ, SR_BENCH_SINGLE_DEVICE="1", PYTHONPATH=ROOT, MASTER_PORT="29653")
    g1, g2, t1, t2 = (tmp_path / n for n in ("g1.gfa", "g2.gfa", "t1.gfa", "t2.gfa"))
    regs = regions_of(recs)
    base = [sys.executable, "-m", "seqrush_amd", "-s", str(fa), "--no-sort"] + [x for r in regs for x in ("--extract-region", r)]
    _run(base + ["-o", str(g1), "--extract-out", str(t1)], env=env, cwd=ROOT)
    stdout = _run(base + ["-o", str(g2), "--extract-out", str(t2), "--gpus", "2"], env=env, cwd=ROOT)
    assert g1.read_text() == g2.read_text() and t1.read_text() == t2.read_text()
    assert stdout.count("Extracted graph written to") == 1
    assert t1.read_text() == extract_gfa(g1.read_text(), regs, None, TWIN) != "H\tVN:Z:1.0\n"
