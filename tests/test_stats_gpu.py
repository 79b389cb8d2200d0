"""GPU tests of the statistics stage: the HIP kernels against the host twin and the Python
restatement on every input of test_stats_host.py, on graphs a Context builds, through both command lines and --gpus 2.
Every comparison is exact."""
import os
import subprocess
import sys

import pytest

import sort_helpers as sh
import stats_helpers as st
from test_stats_host import GOLDEN, check_report
from seqrush_amd import synth
from seqrush_amd.seqrush import Context, Params, SeqSet, SortParams, graph_stats, graph_stats_report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "seqrush_amd", "seqrush_mi355x")
TWIN = -1


def _inputs():
    out = [("golden:" + c["name"], c["gfa"]) for c in GOLDEN]
    out += [("random:%d" % c[0], st.random_gfa(c[0], c[1], c[2], c[3], sparse_ids=c[0] % 2 == 0)) for c in st.RANDOM_CASES]
    out += [("hand:" + n, t) for n, t in sorted(st.hand_cases().items())]
    # every tile pair of the largest path count: 64 x 64 tiles, the last one full
    out.append(("paths:4096", "H\tVN:Z:1.0\nS\t1\tAC\nS\t2\tG\n" + "".join(f"P\tp{k}\t{1 + k % 2}+\t*\n" for k in range(4096))))
    return out


INPUTS = _inputs()


@pytest.mark.gpu
@pytest.mark.parametrize("name,text", INPUTS, ids=[n for n, _ in INPUTS])
def test_device_equals_twin_and_restatement(gpu, name, text):
    dev = graph_stats(text, 0)
    twin = graph_stats(text, TWIN)
    st.assert_equal(dev, twin, name + " (device against twin)")
    if not name.startswith("paths:"):
        st.assert_equal(dev, st.stats(st.parse(text)), name + " (device against restatement)")
    else:
        assert int(dev["shared"][0][2]) == 2 and int(dev["shared"][1][4095]) == 1 and int(dev["shared"][0][1]) == 0
    assert [[int(x) for x in row] for row in dev["path_sq_parts"]] == [[int(x) for x in row] for row in twin["path_sq_parts"]]
    again = graph_stats(text, 0)
    st.assert_equal(again, dev, name + " (device run to run)")
    assert graph_stats_report(text, 0) == graph_stats_report(text, TWIN)


def _built(recs, params=None, **kw):
    ctx = Context(0)
    ctx.load(SeqSet(recs), params or Params())
    ctx.run()
    ctx.sync()
    out = [ctx.build_gfa(**k)[0] for k in kw["builds"]]
    ctx.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("rc_every", [0, 3])
def test_context_graphs_match_the_twin(gpu, rc_every):
    recs = synth.snp_family(8, 600, 0.05, 211, rc_every=rc_every) if rc_every else synth.snp_family(8, 600, 0.05, 211)
    for text in _built(recs, builds=[dict(compact=False), dict(compact=True)]):
        dev, twin = graph_stats(text, 0), graph_stats(text, TWIN)
        st.assert_equal(dev, twin, "context graph")
        assert dev["paths"] == 8 and dev["steps"] > 0 and dev["stats_us"] > 0
        assert int(dev["bp_by_paths"][0]) == 0                 # every node of an induced graph lies on a path
        g = st.parse(text)
        check_report(graph_stats_report(text, 0), st.as_plain(twin), [n for n, _ in g.paths])
        assert dev["total_abs"] / max(dev["total_pairs"], 1) == sh.quality(g)


@pytest.mark.gpu
def test_sort_lowers_the_layout_error(gpu):
    recs = synth.snp_family(16, 1000, 0.05, 2001)
    unsorted, sorted_ = _built(recs, builds=[dict(compact=True), dict(compact=True, sort=SortParams(device=0))])
    du, ds = graph_stats(unsorted, 0), graph_stats(sorted_, 0)
    st.assert_equal(du, graph_stats(unsorted, TWIN), "unsorted")
    st.assert_equal(ds, graph_stats(sorted_, TWIN), "sorted")
    for k in ("length", "nodes", "edges", "paths", "steps", "depth_bp", "components"):
        assert du[k] == ds[k], k
    assert ds["total_abs"] < du["total_abs"]


def write_fasta(path, recs):
    path.write_bytes(b"".join(b">" + n.encode() + b"\n" + s + b"\n" for n, s in recs))


def _run(cmd, **kw):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, **kw)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


@pytest.mark.gpu
def test_both_command_lines_write_the_same_report(gpu, tmp_path):
    recs = synth.snp_family(5, 400, 0.05, 97, rc_every=2)
    fa = tmp_path / "in.fa"
    write_fasta(fa, recs)
    env = dict(os.environ, PYTHONPATH=ROOT)
    py = [sys.executable, "-m", "seqrush_amd"]
    files = {}
    for tag, cmd, kw in (("c", [EXE], {}), ("p", py, dict(cwd=ROOT, env=env))):
        plain, gfa, rep = tmp_path / f"{tag}_plain.gfa", tmp_path / f"{tag}.gfa", tmp_path / f"{tag}.tsv"
        _run(cmd + ["-s", str(fa), "-o", str(plain), "--sort"], **kw)
        out = _run(cmd + ["-s", str(fa), "-o", str(gfa), "--sort", "--stats", str(rep), "-v"], **kw)
        assert "Statistics stage:" in out and f"Statistics written to {rep}" in out
        files[tag] = (plain.read_text(), gfa.read_text(), rep.read_text())
    assert files["c"][1] == files["c"][0] == files["p"][0] == files["p"][1]      # --stats leaves the GFA alone
    assert files["c"][2] == files["p"][2]
    assert files["c"][2] == graph_stats_report(files["c"][1], 0) == graph_stats_report(files["c"][1], TWIN)
    tool = _run([sys.executable, "-m", "seqrush_amd.stats", str(tmp_path / "c.gfa"), "--device", "0"], cwd=ROOT, env=env)
    assert tool == files["c"][2]


@pytest.mark.gpu
def test_multi_gpu_writes_the_report_once(gpu, tmp_path):
    recs = synth.snp_family(6, 500, 0.05, 711, rc_every=3)
    fa = tmp_path / "in.fa"
    write_fasta(fa, recs)
    env = dict(os.environ, SR_BENCH_SINGLE_DEVICE="1", PYTHONPATH=ROOT, MASTER_PORT="29633")
    out1, out2, rep1, rep2 = tmp_path / "g1.gfa", tmp_path / "g2.gfa", tmp_path / "s1.tsv", tmp_path / "s2.tsv"
    base = [sys.executable, "-m", "seqrush_amd", "-s", str(fa), "--no-sort"]
    _run(base + ["-o", str(out1), "--stats", str(rep1)], env=env, cwd=ROOT)
    stdout = _run(base + ["-o", str(out2), "--stats", str(rep2), "--gpus", "2"], env=env, cwd=ROOT)
    assert out1.read_text() == out2.read_text() and rep1.read_text() == rep2.read_text()
    assert stdout.count("Statistics written to") == 1
