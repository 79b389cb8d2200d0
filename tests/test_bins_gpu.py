"""GPU tests of the path-by-bin tables: the HIP kernels against the host twin on every input of
test_bins_host.py, on shapes built for the seams of the step kernel (bins_inputs.seam_cases), on a graph a Context builds
through both command lines and --gpus 2.  Device against twin is exact, and so is the device run to run."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bins_inputs as bi
from seqrush_amd import synth
from seqrush_amd.seqrush import PathBins, path_bins, path_bins_png, path_bins_tsv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "seqrush_amd", "seqrush_mi355x")
TWIN = -1
INPUTS = bi.host_inputs()
SEAMS = bi.seam_cases()


def check(text, kw, what):
    dev, twin = path_bins(text, 0, **kw), path_bins(text, TWIN, **kw)
    bi.assert_same(dev, twin, f"{what} {kw} (device against twin)")
    bi.assert_same(dev, bi.restate(text, **kw), f"{what} {kw} (device against restatement)")
    bi.assert_same(path_bins(text, 0, **kw), dev, f"{what} {kw} (device run to run)")
    return dev


@pytest.mark.gpu
@pytest.mark.parametrize("name,text", INPUTS, ids=[n for n, _ in INPUTS])
def test_device_equals_twin_on_the_host_inputs(gpu, name, text):
    L = bi.layout_of(text)[2]
    variants = set()
    for kw in [dict(bin_width=w) for w in sorted({1, 7, L} - {0})] + [dict(bins=64)]:
        dev = check(text, kw, name)
        variants.add(dev["bins"] > bi.LDS_MAX_BINS)
    if L > bi.LDS_MAX_BINS:
        assert variants == {False, True}             # both kernels ran on this graph
    if L:
        assert path_bins_tsv(text, 0, bins=64) == path_bins_tsv(text, TWIN, bins=64)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SEAMS))
def test_device_equals_twin_on_the_seams(gpu, name):
    text, settings = SEAMS[name]
    L = bi.layout_of(text)[2]
    seen = set()
    for kw in settings:
        dev = check(text, kw, name)
        seen.add(dev["bins"] > bi.LDS_MAX_BINS)
    if name.startswith("threshold_"):
        assert dev["bins"] == L and (L > bi.LDS_MAX_BINS) == (name == f"threshold_{bi.LDS_MAX_BINS + 1}")
    else:
        assert seen == {False, True}, "a seam case must reach the LDS variant and the global one"


@pytest.mark.gpu
def test_image_of_the_device_tables(gpu):
    text = dict(INPUTS)["random:5"]
    with PathBins(text, 0, bins=200) as dev, PathBins(text, TWIN, bins=200) as twin:
        for mode in ("path", "strand", "depth"):
            assert np.array_equal(dev.rgb(mode=mode), twin.rgb(mode=mode))
        assert dev.png() == twin.png()
        assert dev.as_dict()["bin_us"] > 0


def write_fasta(path, recs):
    path.write_bytes(b"".join(b">" + n.encode() + b"\n" + s + b"\n" for n, s in recs))


def _run(cmd, **kw):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, **kw)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


@pytest.mark.gpu
def test_both_command_lines_write_the_same_files(gpu, tmp_path):
    recs = synth.snp_family(5, 400, 0.05, 97, rc_every=2)
    fa = tmp_path / "in.fa"
    write_fasta(fa, recs)
    env = dict(os.environ, PYTHONPATH=ROOT)
    py = [sys.executable, "-m", "seqrush_amd"]
    files = {}
    for tag, cmd, kw in (("c", [EXE], {}), ("p", py, dict(cwd=ROOT, env=env))):
        gfa, tsv, png, tsv1, png2 = (tmp_path / f"{tag}{x}" for x in (".gfa", ".tsv", ".png", "_w1.tsv", "_strand.png"))
        out = _run(cmd + ["-s", str(fa), "-o", str(gfa), "--sort", "--bin", str(tsv), "--viz", str(png), "-v"], **kw)
        assert f"Bins written to {tsv}" in out and f"Visualization written to {png}" in out and out.count("Bin stage:") == 2
        _run(cmd + ["-s", str(fa), "-o", str(gfa), "--sort", "--bin", str(tsv1), "--bin-width", "1", "--viz", str(png2), "--viz-width", "90",
                    "--viz-mode", "strand", "--viz-path-height", "4", "--viz-path-gap", "2"], **kw)
        files[tag] = (gfa.read_text(), tsv.read_text(), png.read_bytes(), tsv1.read_text(), png2.read_bytes())
    assert files["c"] == files["p"]
    text = files["c"][0]
    assert files["c"][1] == path_bins_tsv(text, TWIN, bins=1500) == path_bins_tsv(text, 0, bins=1500)
    assert files["c"][2] == path_bins_png(text, TWIN, bins=1500)
    assert files["c"][3] == path_bins_tsv(text, TWIN, bin_width=1)
    assert files["c"][4] == path_bins_png(text, TWIN, bins=90, mode="strand", path_height=4, path_gap=2)
    d = path_bins(text, 0, bin_width=1)
    assert d["paths"] == 5 and d["bins"] == d["length"] and (d["inv"] <= d["cov"]).all()
    tool_png, tool_tsv = tmp_path / "t.png", tmp_path / "t.tsv"
    _run([sys.executable, "-m", "seqrush_amd.viz", str(tmp_path / "c.gfa"), "--device", "0", "-o", str(tool_png), "--tsv", str(tool_tsv)],
         cwd=ROOT, env=env)
    assert tool_png.read_bytes() == files["c"][2] and tool_tsv.read_text() == files["c"][1]


@pytest.mark.gpu
def test_multi_gpu_writes_the_files_once(gpu, tmp_path):
    recs = synth.snp_family(6, 500, 0.05, 711, rc_every=3)
    fa = tmp_path / "in.fa"
    write_fasta(fa, recs)
    env = dict(os.environ, SR_BENCH_SINGLE_DEVICE="1", PYTHONPATH=ROOT, MASTER_PORT="29637")
    names = ("g1.gfa", "g2.gfa", "b1.tsv", "b2.tsv", "v1.png", "v2.png")
    g1, g2, b1, b2, v1, v2 = (tmp_path / n for n in names)
    base = [sys.executable, "-m", "seqrush_amd", "-s", str(fa), "--no-sort"]
    _run(base + ["-o", str(g1), "--bin", str(b1), "--bin-count", "64", "--viz", str(v1)], env=env, cwd=ROOT)
    stdout = _run(base + ["-o", str(g2), "--bin", str(b2), "--bin-count", "64", "--viz", str(v2), "--gpus", "2"], env=env, cwd=ROOT)
    assert g1.read_text() == g2.read_text() and b1.read_text() == b2.read_text() and v1.read_bytes() == v2.read_bytes()
    assert stdout.count("Bins written to") == 1 and stdout.count("Visualization written to") == 1
    assert b1.read_text() == path_bins_tsv(g1.read_text(), TWIN, bins=64)
