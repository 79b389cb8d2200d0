"""GPU tests of the growth curves: the HIP kernels against the host twin on every input of
test_growth_host.py, on shapes built for the seams of the kernels (growth_inputs.seam_cases), in exhaustive mode against the
integer identity, on the two graphs where every column is new and where nothing is ever lost, and on a graph a Context
builds through both command lines and --gpus 2.  Device against twin is exact on pan, core, perm and bp_by_groups, and so
are the device run to run and the device against the restatement by Python sets; the report is equal byte for byte."""
import os
import subprocess
import sys

import pytest

import growth_inputs as gi
from seqrush_amd import synth
from seqrush_amd.seqrush import Growth, growth, growth_report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "seqrush_amd", "seqrush_mi355x")
TWIN = -1
INPUTS = gi.host_inputs()
SEAMS = gi.seam_cases()


def check(text, what, rows=None, **kw):
    """device against twin, run to run and against the restatement (of `rows`, those beyond the table left out; None: all)
    -> the device result"""
    with Growth(text, 0, **kw) as g:
        dev, rep = g.as_dict(), g.report()
    with Growth(text, TWIN, **kw) as g:
        twin, twin_rep = g.as_dict(), g.report()
    assert dev["variant"] == 1 and twin["variant"] == 0
    gi.assert_same(dev, twin, f"{what} (device against twin)")
    assert rep == twin_rep, f"{what}: report"
    gi.assert_same(growth(text, 0, **kw), dev, f"{what} (device run to run)")
    gi.assert_invariants(dev, what)
    group_of = gi.groups_of(gi.PANSN, kw["group_by"])[0] if "group_by" in kw else None
    rows = rows if rows is None else [r for r in rows if r < dev["permutations"]]
    gi.assert_restated(dev, text, f"{what} (device against restatement)", group_of, rows)
    return dev


@pytest.mark.gpu
@pytest.mark.parametrize("name,text", INPUTS, ids=[n for n, _ in INPUTS])
def test_device_equals_twin_on_the_host_inputs(gpu, name, text):
    big = name in ("random:7", "random:8")
    dev = check(text, name, rows=[0, 11] if big else None, permutations=12 if big else 70)
    if dev["groups"]:
        assert dev["growth_us"] > 0
    if dev["groups"] >= 4 and not dev["exhaustive"]:
        assert growth(text, 0, permutations=12 if big else 70, seed=7)["perm"].tolist() != dev["perm"].tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("G", [1, 2, 3, 4, 5, 6])
def test_device_on_the_small_random_graphs(gpu, G):
    for seed in (1, 2):
        gi.assert_exhaustive(check(gi.small_random(G, seed), f"G={G} seed={seed}"), f"G={G} seed={seed}")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["sample", "haplotype"])
def test_device_on_groups_of_several_paths(gpu, mode):
    import stats_helpers as st
    text = gi.rename_paths(st.random_gfa(77, 60, 12, 25), gi.PANSN)
    dev = check(text, mode, group_by=mode, permutations=60)
    assert dev["groups"] == {"sample": 5, "haplotype": 8}[mode] and dev["paths"] == 12


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SEAMS))
def test_device_equals_twin_on_the_seams(gpu, name):
    text, R = SEAMS[name]
    dev = check(text, name, rows=sorted({0, R // 2, R - 1}), permutations=R)
    V, G = (int(x[1:]) for x in name.split("_")[:2])
    assert dev["groups"] == G and dev["permutations"] == (1 if G == 1 else 2 if G == 2 else R)
    assert int(dev["bp_by_groups"][G]) > 0           # the backbone nodes, first and last of the graph among them, are core


@pytest.mark.gpu
@pytest.mark.parametrize("G,V", [(4, 50), (5, 50), (8, 200)])
def test_exhaustive_on_the_device(gpu, G, V):
    text = gi.shaped(V, G, 900 + G, steps=60)
    dev = check(text, f"exhaustive G={G}", rows=[0, 1, 23], permutations=40320)
    gi.assert_exhaustive(dev, f"G={G}")
    if G == 8:
        assert dev["permutations"] == 40320


@pytest.mark.gpu
def test_every_column_new_and_nothing_ever_lost(gpu):
    private = check(gi.all_private(4097, 130), "all private", rows=[0, 69], permutations=70)
    assert (private["pan"][:, 1:] > private["pan"][:, :-1]).all() and not private["core"][:, 1:].any()
    assert int(private["bp_by_groups"][1]) == private["length"]
    core = check(gi.all_core(300, 65), "all core", rows=[0, 69], permutations=70)
    assert (core["pan"] == core["length"]).all() and (core["core"] == core["length"]).all()
    assert int(core["bp_by_groups"][65]) == core["length"]


def write_fasta(path, recs):
    path.write_bytes(b"".join(b">" + n.encode() + b"\n" + s + b"\n" for n, s in recs))


def _run(cmd, **kw):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, **kw)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


@pytest.mark.gpu
def test_both_command_lines_write_the_same_files(gpu, tmp_path):
    recs = synth.snp_family(5, 400, 0.05, 97, rc_every=2)
    pansn = ["s1#1#chr", "s1#2#chr", "s2#1#chr", "s2#2#chr", "s3#1#chr"]
    fa, fa2 = tmp_path / "in.fa", tmp_path / "pansn.fa"
    write_fasta(fa, recs)
    write_fasta(fa2, [(n, s) for n, (_, s) in zip(pansn, recs)])
    env = dict(os.environ, PYTHONPATH=ROOT)
    py = [sys.executable, "-m", "seqrush_amd"]
    files = {}
    for tag, cmd, kw in (("c", [EXE], {}), ("p", py, dict(cwd=ROOT, env=env))):
        gfa, tsv, gfa2, tsv2 = (tmp_path / f"{tag}{x}" for x in (".gfa", ".tsv", "_s.gfa", "_s.tsv"))
        out = _run(cmd + ["-s", str(fa), "-o", str(gfa), "--sort", "--growth", str(tsv), "-v"], **kw)
        assert f"Growth written to {tsv}" in out and out.count("Growth stage:") == 1
        _run(cmd + ["-s", str(fa2), "-o", str(gfa2), "--sort", "--growth", str(tsv2), "--growth-group-by", "sample", "--growth-permutations", "5",
                    "--growth-seed", "11"], **kw)
        files[tag] = (gfa.read_text(), tsv.read_text(), gfa2.read_text(), tsv2.read_text())
    assert files["c"] == files["p"]
    text, text2 = files["c"][0], files["c"][2]
    assert files["c"][1] == growth_report(text, TWIN) == growth_report(text, 0) and "groups=5\tpaths=5\tpermutations=120\texhaustive=1" in files["c"][1]
    # 3 samples: 3! = 6 > 5 permutations asked for, so the orders are sampled
    assert files["c"][3] == growth_report(text2, TWIN, group_by="sample", permutations=5, seed=11)
    assert "groups=3\tpaths=5\tpermutations=5\texhaustive=0\tseed=11" in files["c"][3]
    tool = tmp_path / "t.tsv"
    _run([sys.executable, "-m", "seqrush_amd.growth", str(tmp_path / "c.gfa"), "--device", "0", "-o", str(tool)], cwd=ROOT, env=env)
    assert tool.read_text() == files["c"][1]


@pytest.mark.gpu
def test_multi_gpu_writes_the_file_once(gpu, tmp_path):
    recs = synth.snp_family(6, 500, 0.05, 711, rc_every=3)
    fa = tmp_path / "in.fa"
    write_fasta(fa, recs)
    env = dict(os.environ, SR_BENCH_SINGLE_DEVICE="1", PYTHONPATH=ROOT, MASTER_PORT="29641")
    g1, g2, t1, t2 = (tmp_path / n for n in ("g1.gfa", "g2.gfa", "t1.tsv", "t2.tsv"))
    base = [sys.executable, "-m", "seqrush_amd", "-s", str(fa), "--no-sort"]
    _run(base + ["-o", str(g1), "--growth", str(t1), "--growth-permutations", "64"], env=env, cwd=ROOT)
    stdout = _run(base + ["-o", str(g2), "--growth", str(t2), "--growth-permutations", "64", "--gpus", "2"], env=env, cwd=ROOT)
    assert g1.read_text() == g2.read_text() and t1.read_text() == t2.read_text()
    assert stdout.count("Growth written to") == 1
    assert t1.read_text() == growth_report(g1.read_text(), TWIN, permutations=64)
