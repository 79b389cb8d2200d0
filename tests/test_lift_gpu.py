"""GPU tests of the interval lift: the HIP kernels against the host twin on every input of
test_lift_host.py and on graphs and queries built for the seams of the kernels (lift_inputs.seam_cases): intervals of 1 to
1025 steps with their ends on, before and behind step boundaries, a path boundary on a workgroup boundary of the scan, 1 to
130 targets, an empty target, one that shares nothing, one that visits a node three times, a long interval whose only
shared node is its last step, and 5 000 one-base queries.  Device against twin is exact on every field and on the output
bytes, and so are the device run to run, the device against the restatement in Python, and the three settings of
short_steps; both command lines, the tool and --gpus 2 write the same file."""
import functools
import os
import subprocess
import sys

import pytest

import growth_inputs as gi
import lift_inputs as li
import variants_inputs as vi
from seqrush_amd import synth
from seqrush_amd.seqrush import Lift, lift, lift_bed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "seqrush_amd", "seqrush_mi355x")
TWIN = -1
INPUTS = gi.host_inputs() + vi.bubble_inputs()
SEAMS = li.seam_cases()


def check(text, bed, what, **kw):
    """device against twin, run to run, against the restatement and over short_steps -> the device result"""
    with Lift(text, bed, TWIN, **kw) as v:
        twin, twin_out = v.as_dict(), v.bed()
    want = li.restate(text, bed, kw.get("to"))
    pairs = twin["queries"] * twin["targets"]
    dev = None
    for short in (li.SHORT_STEPS, li.ALL_LONG, li.ALL_SHORT):
        with Lift(text, bed, 0, short_steps=short, **kw) as v:
            d, out = v.as_dict(), v.bed()
        assert d["variant"] == 1 and twin["variant"] == 0
        li.assert_same(d, twin, f"{what} short_steps={short} (device against twin)")
        assert out == twin_out, f"{what} short_steps={short}: bytes"
        li.assert_same(d, want, f"{what} short_steps={short} (device against restatement)")
        assert d["short_pairs"] + d["long_pairs"] == pairs
        if short == li.ALL_LONG:
            assert d["short_pairs"] == 0
        if short == li.ALL_SHORT:
            assert d["long_pairs"] == 0
        dev = dev or d
    again = lift(text, bed, 0, **kw)
    li.assert_same(again, dev, f"{what} (device run to run)")
    assert (again["short_pairs"], again["long_pairs"]) == (dev["short_pairs"], dev["long_pairs"])
    return dev


@pytest.mark.gpu
@pytest.mark.parametrize("name,text", INPUTS, ids=[n for n, _ in INPUTS])
def test_device_equals_twin_on_the_host_inputs(gpu, name, text):
    names = li.names_of(text)
    bed = li.random_bed(text, len(name))
    dev = check(text, bed, name)
    if dev["queries"]:
        assert dev["lift_us"] > 0
    if names:
        check(text, bed, f"{name} to={names[-1]}", to=names[-1])


@functools.lru_cache(maxsize=None)
def seam(name):
    text, bed, kw = SEAMS[name]
    return check(text, bed, name, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SEAMS))
def test_device_equals_twin_on_the_seams(gpu, name):
    text, bed, kw = SEAMS[name]
    dev = seam(name)
    names = li.names_of(text)
    by = {label: i for i, label in enumerate(dev["labels"])}
    if name == "chain_1_to_1025_steps":
        g = vi.st.parse(text)
        assert [len(s) for _, s in g.paths][:3] == [256, 1100, 1] and names[-1] == "tail" and names[-2] == "none"
        assert dev["short_pairs"] > 0 and dev["long_pairs"] > 0             # both kernels ran
        T = dev["targets"]
        longer = sum(1 for label in dev["labels"] if label.startswith("steps") and int(label[5:].split("_")[0]) > li.SHORT_STEPS)
        assert dev["long_pairs"] >= longer * T and dev["short_pairs"] >= 3 * 2 * T
        at = li.step_starts(text, "ref")
        for n in (1, 8, 9, 63, 64, 65, 128, 129, 1025):
            i, ref = by[f"steps{n}"], names.index("ref")
            assert int(dev["q_end"][i] - dev["q_start"][i]) == at[20 + n % 7 + n] - at[20 + n % 7]
            assert [int(dev[k][i, ref]) for k in li.FIELDS] == [int(dev["q_start"][i]), int(dev["q_end"][i]), int(dev["covered"][i, ref]), 0]
        empty, alone, thrice = names.index("none"), names.index("alone"), names.index("thrice")
        assert not dev["covered"][:, empty].any() and not dev["covered"][by["whole_path"], alone].any()
        # thrice = 3+ 5- 4+ 5+ 6+ 5- 7+: node 5 lifts to its first visit, right behind node 3, on the reverse strand
        i = by["over_thrice"]
        n3, n5 = at[3] - at[2], at[5] - at[4]
        assert int(dev["tstart"][i, thrice]) == 0 and int(dev["rev_bp"][i, thrice]) == n5 and int(dev["covered"][i, thrice]) == at[7] - at[2]
        assert n3 > 0
        # the long interval whose only shared node is its 201st step: one node of the chain, wherever a target has it
        i, j = by["shared_at_the_last_step"], by["shares_nothing"]
        assert int(dev["q_end"][i]) > 200 and int(dev["covered"][i, names.index("ref")]) == int(dev["q_end"][i] - dev["q_end"][j]) > 0
        assert not dev["covered"][j, :names.index("tail")].any() and dev["covered"][j, names.index("tail")] == dev["q_end"][j]
        assert int(dev["rev_bp"][i, names.index("ref")]) == int(dev["covered"][i, names.index("ref")])
        assert dev["covered"][by["path_of_one_step"], names.index("one")] == dev["q_end"][by["path_of_one_step"]]
    if name == "chain_to_the_empty_target":
        assert dev["targets"] == 1 and dev["mapped"] == 0
    if name == "chain_to_one_reversed_target":
        assert dev["targets"] == 1 and dev["mapped"] > 0 and dev["short_pairs"] > 0 and dev["long_pairs"] > 0
    if name.startswith("targets_"):
        P = int(name.split("_")[1])
        assert dev["targets"] == P and dev["queries"] == 5 and dev["short_pairs"] == 2 * P and dev["long_pairs"] == 3 * P
        assert dev["mapped"] > 3 * P
    if name == "one_base_5000":
        assert dev["queries"] == 5000 and dev["short_pairs"] == 30000 > 64 * li.BLOCK // 4 and dev["long_pairs"] == 0


def write_fasta(path, recs):
    path.write_bytes(b"".join(b">" + n.encode() + b"\n" + s + b"\n" for n, s in recs))


def _run(cmd, **kw):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, **kw)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def bed_of(recs, n=12):
    """n lines over the records: whole sequences, single bases, a label here and there, one unknown name"""
    rows = []
    for k in range(n - 1):
        name, s = recs[k % len(recs)]
        a = (37 * k) % (len(s) - 1)
        b = len(s) if k < 2 else a + 1 if k % 3 == 0 else min(len(s), a + 5 + 20 * k)
        rows.append((name, 0 if k < 2 else a, b) + ((f"gene{k}",) if k % 2 else ()))
    rows.append(("chrUn", 0, 5, "elsewhere"))
    return li._bed(rows)


@pytest.mark.gpu
def test_both_command_lines_and_the_tool_write_the_same_files(gpu, tmp_path):
    recs = synth.snp_family(5, 400, 0.05, 97, rc_every=2)
    fa, bed = tmp_path / "in.fa", tmp_path / "in.bed"
    write_fasta(fa, recs)
    bed.write_text(bed_of(recs))
    assert bed.read_text().count("\n") == 12
    env = dict(os.environ, PYTHONPATH=ROOT)
    py = [sys.executable, "-m", "seqrush_amd"]
    to = recs[1][0]                                             # a reverse-complemented record
    files = {}
    for tag, cmd, kw in (("c", [EXE], {}), ("p", py, dict(cwd=ROOT, env=env))):
        gfa, out, gfa2, out2 = (tmp_path / f"{tag}{x}" for x in (".gfa", ".bed", "_t.gfa", "_t.bed"))
        stdout = _run(cmd + ["-s", str(fa), "-o", str(gfa), "--sort", "--lift", str(bed), "--lift-out", str(out), "-v"], **kw)
        assert f"Lifted intervals written to {out}" in stdout and stdout.count("Lift stage:") == 1
        quiet = _run(cmd + ["-s", str(fa), "-o", str(gfa2), "--no-sort", "--lift", str(bed), "--lift-out", str(out2), "--lift-to", to,
                            "--lift-min-covered", "2"], **kw)
        assert "Lift stage:" not in quiet
        files[tag] = (gfa.read_text(), out.read_text(), gfa2.read_text(), out2.read_text())
    assert files["c"] == files["p"]
    text, text2 = files["c"][0], files["c"][2]
    assert files["c"][1] == lift_bed(text, bed.read_text(), TWIN) == lift_bed(text, bed.read_text(), 0) and files["c"][1].count("\n") > 20
    assert files["c"][3] == lift_bed(text2, bed.read_text(), TWIN, to=to, min_covered=2)
    assert {x.split("\t")[0] for x in files["c"][3].splitlines()} == {to} and "\t-\t" in files["c"][3]
    tool = tmp_path / "t.bed"
    _run([sys.executable, "-m", "seqrush_amd.lift", str(tmp_path / "c.gfa"), "-b", str(bed), "--device", "0", "-o", str(tool)], cwd=ROOT, env=env)
    assert tool.read_text() == files["c"][1]


@pytest.mark.gpu
def test_lift_after_extend(gpu, tmp_path):
    recs = synth.snp_family(5, 400, 0.05, 97, rc_every=2)
    old, new, bed = tmp_path / "old.fa", tmp_path / "new.fa", tmp_path / "in.bed"
    write_fasta(old, recs[:3])
    write_fasta(new, recs[3:])
    bed.write_text(bed_of(recs))
    g0, g1, out = tmp_path / "g0.gfa", tmp_path / "g1.gfa", tmp_path / "out.bed"
    _run([EXE, "-s", str(old), "-o", str(g0), "--no-sort"])
    _run([EXE, "-s", str(new), "-o", str(g1), "--no-sort", "--extend", str(g0), "--lift", str(bed), "--lift-out", str(out)])
    assert out.read_text() == lift_bed(g1.read_text(), bed.read_text(), TWIN) and out.read_text().count("\n") > 20
    assert {x.split("\t")[0] for x in out.read_text().splitlines()} == {n for n, _ in recs}


@pytest.mark.gpu
def test_multi_gpu_writes_the_file_once(gpu, tmp_path):
    recs = synth.snp_family(6, 500, 0.05, 711, rc_every=3)
    fa, bed = tmp_path / "in.fa", tmp_path / "in.bed"
    write_fasta(fa, recs)
    bed.write_text(bed_of(recs))
    env = dict(os.environ, SR_BENCH_SINGLE_DEVICE="1", PYTHONPATH=ROOT, MASTER_PORT="29647")
    g1, g2, t1, t2 = (tmp_path / n for n in ("g1.gfa", "g2.gfa", "t1.bed", "t2.bed"))
    base = [sys.executable, "-m", "seqrush_amd", "-s", str(fa), "--no-sort", "--lift", str(bed)]
    _run(base + ["-o", str(g1), "--lift-out", str(t1)], env=env, cwd=ROOT)
    stdout = _run(base + ["-o", str(g2), "--lift-out", str(t2), "--gpus", "2"], env=env, cwd=ROOT)
    assert g1.read_text() == g2.read_text() and t1.read_text() == t2.read_text()
    assert stdout.count("Lifted intervals written to") == 1
    assert t1.read_text() == lift_bed(g1.read_text(), bed.read_text(), TWIN) != ""
