"""CPU tests (-m "not gpu") of the path-by-bin tables through the host twin (device = -1): hand-worked
known answers, a per-base numpy restatement on every input of the statistics tests, the identities with graph_stats, the
refusals, the TSV, the image, the PNG and the command line.  Every comparison is exact."""
import json
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import bins_inputs as bi
from test_stats_host import GOLDEN
from seqrush_amd.seqrush import PathBins, SeqRushError, graph_stats, path_bins, path_bins_png, path_bins_rgb, path_bins_tsv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOWN = json.load(open(os.path.join(ROOT, "tests", "golden", "bins_known_answers.json")))["cases"]
TWIN = -1
INPUTS = bi.host_inputs()
GFA = {c["name"]: c["gfa"] for c in GOLDEN}


@pytest.mark.parametrize("case", KNOWN, ids=[c["name"] for c in KNOWN])
def test_known_answers(case):
    text = GFA[case["name"]]
    for s in case["settings"]:
        d = path_bins(text, TWIN, bin_width=s["bin_width"])
        assert d["bins"] == s["bins"] and d["bin_width"] == s["bin_width"]
        assert d["cov"].shape == d["inv"].shape == (d["paths"], s["bins"])
        if "cov" in s:
            assert d["cov"].tolist() == s["cov"] and d["inv"].tolist() == s["inv"]
        if "cov_zero" in s:
            for p, zeros in enumerate(s["cov_zero"]):
                assert d["cov"][p].tolist() == [0 if b in zeros else 1 for b in range(s["bins"])]
        if "inv_nonzero" in s:
            for p, nz in enumerate(s["inv_nonzero"]):
                assert d["inv"][p].tolist() == [nz.get(str(b), 0) for b in range(s["bins"])]
        for p, row in s.get("cov_rows", {}).items():
            assert d["cov"][int(p)].tolist() == row
        bi.assert_same(d, bi.restate(text, bin_width=s["bin_width"]), case["name"] + " (restatement)")


def settings_of(L):
    return [dict(bin_width=w) for w in sorted({1, 7, L, L + 5} - {0})] + [dict(bins=n) for n in sorted({1, 64, L, 2 * L} - {0})]


@pytest.mark.parametrize("name,text", INPUTS, ids=[n for n, _ in INPUTS])
def test_twin_matches_the_per_base_restatement(name, text):
    L = bi.layout_of(text)[2]
    for kw in settings_of(L):
        got = path_bins(text, TWIN, **kw)
        bi.assert_same(got, bi.restate(text, **kw), f"{name} {kw}")
        if kw.get("bins") == 2 * L:
            assert got["bins"] == L and got["bin_width"] == 1
        if name == "golden:empty_graph":
            assert got["bins"] == 0 and got["cov"].shape == (0, 0)


@pytest.mark.parametrize("name,text", INPUTS, ids=[n for n, _ in INPUTS])
def test_identities_with_graph_stats(name, text):
    gs = graph_stats(text, TWIN)
    L = int(gs["length"])
    if L == 0:
        assert path_bins(text, TWIN, bin_width=3)["bins"] == 0
        return
    whole = path_bins(text, TWIN, bin_width=L + 3)
    assert int(whole["cov"].sum()) == int(gs["depth_bp"]) and whole["bins"] == 1
    names, paths, _ = bi.layout_of(text)
    assert whole["cov"][:, 0].tolist() == [sum(n for _, n, _ in steps) for steps in paths]      # the paths' lengths in bp
    per_base = path_bins(text, TWIN, bin_width=1)
    assert int(per_base["cov"].sum()) == int(gs["depth_bp"]) == int(path_bins(text, TWIN, bins=64)["cov"].sum())
    lens = _node_lengths(text)
    node_of_base = np.repeat(np.arange(len(lens)), lens)
    assert ((per_base["cov"] > 0).sum(axis=0) == np.asarray(gs["paths_on"])[node_of_base]).all()
    assert (per_base["cov"].sum(axis=0) == np.asarray(gs["depth"])[node_of_base]).all()


def _node_lengths(text):
    seq = {}
    for line in text.split("\n"):
        f = line.split("\t")
        if f[0] == "S":
            seq[int(f[1])] = len(f[2])
    return [seq[i] for i in sorted(seq)]


def test_refusals():
    text = GFA["three_paths_layout"]
    for kw in (dict(), dict(bin_width=2, bins=3)):
        with pytest.raises(SeqRushError) as e:
            path_bins(text, TWIN, **kw)
        assert e.value.code == -1                    # SR_ERR_INVALID
    with pytest.raises(SeqRushError):
        path_bins(text, -2, bins=3)
    # 1000 paths x 70000 bins > 2^26 cells
    wide = "H\tVN:Z:1.0\nS\t1\t" + "A" * 70000 + "\n" + "".join(f"P\tp{k}\t1+\t*\n" for k in range(1000))
    with pytest.raises(SeqRushError) as e:
        path_bins(wide, TWIN, bin_width=1)
    assert e.value.code == -6                        # SR_ERR_UNSUPPORTED
    with PathBins(wide, TWIN, bin_width=8) as pb:    # 8750 bins: 8 750 000 cells
        ok = pb.as_dict()
        assert ok["bins"] == 8750 and int(ok["cov"].sum()) == 70000 * 1000
        with pytest.raises(SeqRushError) as e:       # 8750 x (1000 x 41 + 999) x 3 bytes > 2^30
            pb.rgb(path_height=41)
        assert e.value.code == -6
    with PathBins(GFA["empty_graph"], TWIN, bins=5) as pb:
        assert pb.rgb().shape == (0, 0, 3)
        with pytest.raises(SeqRushError):
            pb.png()


TSV_CASES = ["golden:three_paths_layout", "golden:loops_and_pieces", "random:3", "hand:empty_and_one_step_paths", "golden:empty_graph"]


@pytest.mark.parametrize("name", TSV_CASES)
def test_tsv_bytes(name):
    text = dict(INPUTS)[name]
    for kw in (dict(bin_width=4), dict(bins=7), dict(bin_width=1)):
        want = bi.restate(text, **kw)
        assert path_bins_tsv(text, TWIN, **kw) == bi.tsv_of(want, want["names"]), f"{name} {kw}"
    with PathBins(text, TWIN, bin_width=3) as pb:
        want = bi.restate(text, bin_width=3)
        other = [f"n{k}" for k in range(want["paths"])]
        assert pb.tsv(other) == bi.tsv_of(want, other)


def decode_png(data):
    """-> (width, height, raw scanlines with their filter bytes, the zlib stream); checks the signature, every CRC, IHDR and IEND"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + body), kind
        chunks.append((kind, body))
        at += 12 + n
    assert at == len(data) and chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    z = b"".join(body for kind, body in chunks if kind == b"IDAT")
    return w, h, zlib.decompress(z), z                # decompress verifies the Adler-32


def stored_blocks(z):
    """the lengths of the stored deflate blocks of a zlib stream made of nothing else"""
    at, out = 2, []
    while True:
        final, n, nn = z[at], *struct.unpack("<HH", z[at + 1:at + 5])
        assert final in (0, 1) and n == (~nn & 0xffff)
        out.append(n)
        at += 5 + n
        if final:
            break
    assert at + 4 == len(z)
    return out


@pytest.mark.parametrize("mode", ["path", "strand", "depth"])
def test_image_and_png(mode):
    for name, kw, viz in (("golden:three_paths_layout", dict(bin_width=1), dict()),
                          ("golden:loops_and_pieces", dict(bin_width=4), dict(path_height=3, path_gap=0, depth_max=1)),
                          ("random:4", dict(bins=100), dict(path_height=2, path_gap=2, depth_max=2)),        # 64 paths
                          ("hand:empty_and_one_step_paths", dict(bins=5), dict(path_height=1, path_gap=1, depth_max=3))):
        text = dict(INPUTS)[name]
        want = bi.restate(text, **kw)
        with PathBins(text, TWIN, **kw) as pb:
            img, png = pb.rgb(mode=mode, **viz), pb.png(mode=mode, **viz)
        assert img.dtype == np.uint8 and np.array_equal(img, bi.rgb_of(want, want["names"], mode=mode, **viz)), f"{name} {mode}"
        assert np.array_equal(img, path_bins_rgb(text, TWIN, mode=mode, **kw, **viz)) and png == path_bins_png(text, TWIN, mode=mode, **kw, **viz)
        w, h, raw, _ = decode_png(png)
        assert (h, w) == img.shape[:2]
        rows = np.frombuffer(raw, dtype=np.uint8).reshape(h, 1 + 3 * w)
        assert not rows[:, 0].any() and np.array_equal(rows[:, 1:].reshape(h, w, 3), img)


def test_png_of_more_than_one_stored_block():
    text = dict(INPUTS)["random:5"]                  # 65 paths -> 65 x 10 + 64 rows of 1 + 3 x 300 bytes: ~640 KB raw
    with PathBins(text, TWIN, bins=300) as pb:
        img, png = pb.rgb(), pb.png()
    w, h, raw, z = decode_png(png)
    assert len(raw) == h * (1 + 3 * w) > 65535
    blocks = stored_blocks(z)
    assert len(blocks) == -(-len(raw) // 65535) > 1 and sum(blocks) == len(raw) and all(n == 65535 for n in blocks[:-1])
    assert np.array_equal(np.frombuffer(raw, dtype=np.uint8).reshape(h, 1 + 3 * w)[:, 1:].reshape(h, w, 3), img)
    colours = {tuple(bi.base_colour(f"p{k}")) for k in range(65)}
    assert len(colours) > 60 and all(32 <= c <= 223 for col in colours for c in col)


def test_viz_command_line_writes_the_bytes_of_the_api(tmp_path):
    text = dict(INPUTS)["random:3"]
    gfa, png, tsv = tmp_path / "g.gfa", tmp_path / "a.png", tmp_path / "a.tsv"
    gfa.write_text(text)
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "seqrush_amd.viz", str(gfa), "--device", "-1", "-o", str(png), "--tsv", str(tsv)],
                       capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert png.read_bytes() == path_bins_png(text, TWIN, bins=1500) and tsv.read_text() == path_bins_tsv(text, TWIN, bins=1500)
    r = subprocess.run([sys.executable, "-m", "seqrush_amd.viz", str(gfa), "--device", "-1", "-o", str(png), "--bin-width", "9",
                        "--viz-mode", "strand", "--viz-path-height", "2", "--viz-path-gap", "0"],
                       capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert png.read_bytes() == path_bins_png(text, TWIN, bin_width=9, mode="strand", path_height=2, path_gap=0)


EXE = os.path.join(ROOT, "seqrush_amd", "seqrush_mi355x")
BAD_FLAGS = [(["--bin", "b.tsv", "--bin-count", "0"], "--bin-count needs a positive integer"),
             (["--bin", "b.tsv", "--bin-width", "0"], "--bin-width needs a positive integer"),
             (["--bin", "b.tsv", "--bin-width", "3", "--bin-count", "4"], "--bin-width and --bin-count exclude each other"),
             (["--bin-width", "3"], "--bin-width is an option of --bin"),
             (["--bin-count", "3", "--viz", "v.png"], "--bin-count is an option of --bin"),
             (["--viz-mode", "strand", "--bin", "b.tsv"], "--viz-mode is an option of --viz"),
             (["--viz", "v.png", "--viz-width", "0"], "--viz-width needs a positive integer"),
             (["--viz", "v.png", "--viz-path-height", "0"], "--viz-path-height needs a positive integer")]


@pytest.mark.parametrize("flags,message", BAD_FLAGS, ids=[" ".join(f) for f, _ in BAD_FLAGS])
def test_both_front_ends_refuse_the_same_flags(flags, message, tmp_path):
    fa = tmp_path / "in.fa"
    fa.write_text(">a\nACGT\n")
    env = dict(os.environ, PYTHONPATH=ROOT)
    for cmd in ([EXE], [sys.executable, "-m", "seqrush_amd"]):       # refused while the arguments are read: no device is opened
        r = subprocess.run(cmd + ["-s", str(fa), "-o", str(tmp_path / "o.gfa"), "--no-sort"] + flags, capture_output=True, text=True,
                           cwd=ROOT, env=env, timeout=300)
        assert r.returncode == 1 and message in r.stderr, (cmd, r.returncode, r.stderr[-500:])
