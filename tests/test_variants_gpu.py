"""GPU tests of the variant sites: the HIP kernels against the host twin on every input of
test_variants_host.py and on graphs built for the seams of the kernels (variants_inputs.seam_cases): paths of 1 to 1025
steps, a path boundary on a workgroup boundary, more than two workgroups without an anchor step, a path without an anchor
and one without a step, a reference of one step, more than 4096 traversals at one site, and three alleles of one length
with every hash colliding.  Device against twin is exact on every field and on the VCF bytes, and so are the device run to
run and the device against the restatement in Python; both command lines, the tool and --gpus 2 write the same file."""
import os
import subprocess
import sys

import pytest

import growth_inputs as gi
import variants_inputs as vi
from seqrush_amd import synth
from seqrush_amd.seqrush import Variants, variants, variants_vcf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "seqrush_amd", "seqrush_mi355x")
TWIN = -1
INPUTS = gi.host_inputs() + vi.bubble_inputs()
SEAMS = vi.seam_cases()


def check(text, what, **kw):
    """device against twin, run to run and against the restatement -> the device result"""
    with Variants(text, 0, **kw) as v:
        dev, vcf = v.as_dict(), v.vcf()
    with Variants(text, TWIN, **kw) as v:
        twin, twin_vcf = v.as_dict(), v.vcf()
    assert dev["variant"] == 1 and twin["variant"] == 0 and twin["hash_collision_sites"] == 0
    vi.assert_same(dev, twin, f"{what} (device against twin)")
    assert vcf == twin_vcf, f"{what}: VCF bytes"
    again = variants(text, 0, **kw)
    vi.assert_same(again, dev, f"{what} (device run to run)")
    assert again["hash_collision_sites"] == dev["hash_collision_sites"]
    rule = {k: v for k, v in kw.items() if k != "hash_mask"}
    vi.assert_same(dev, vi.restate(text, **rule), f"{what} (device against restatement)")
    return dev


@pytest.mark.gpu
@pytest.mark.parametrize("name,text", INPUTS, ids=[n for n, _ in INPUTS])
def test_device_equals_twin_on_the_host_inputs(gpu, name, text):
    names = vi.names_of(text)
    dev = check(text, name)
    if dev["traversals"]:
        assert dev["variants_us"] > 0
    if len(names) > 1:
        check(text, f"{name} ref={names[-1]}", ref=names[-1])
    assert dev["hash_collision_sites"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SEAMS))
def test_device_equals_twin_on_the_seams(gpu, name):
    text, kw = SEAMS[name]
    dev = check(text, name, **kw)
    if name == "steps_1_to_1025":
        g = vi.st.parse(text)
        assert [len(s) for _, s in g.paths][:3] == [256, 1100, 1] and 0 in [len(s) for _, s in g.paths]
        assert dev["ref_path"] == 1 and dev["sites"] > 100 and dev["anchors"] == 1100
        gap = [n for n, _ in g.paths].index("gap")
        assert max(len(x) for al in dev["alleles"] for x in al) > 2 * vi.BLOCK      # the allele across the long stretch
        assert (dev["gt"][:, gap] > 0).sum() == 1
        assert (dev["gt"][:, [n for n, _ in g.paths].index("off")] == -1).all()
    if name == "ref_of_one_step":
        assert dev["anchors"] == 1 and dev["breaks"].tolist() == [0, 0, 1, 0] and dev["sites"] == 0
    if name == "one_site_4200_paths":
        assert dev["sites"] == 1 and dev["traversals"] == 4199 and dev["alleles"] == [[b"C", b"G", b"T"]]
    if "every_hash_collides" in name:
        plain = variants(text, 0)
        vi.assert_same(dev, plain, f"{name}: the result does not depend on the hash")
        assert dev["hash_collision_sites"] > 0 and plain["hash_collision_sites"] == 0
        assert max(len(al) for al in dev["alleles"]) >= 2


@pytest.mark.gpu
def test_device_on_the_constructed_truth_and_max_allele_len(gpu):
    text, truth = vi.bubbles(3, 40, 7)
    dev = check(text, "bubbles")
    assert [(int(a), int(b), al) for a, b, al in zip(dev["site_start"], dev["site_end"], dev["alleles"])] == truth["sites"]
    assert dev["gt"].tolist() == truth["gt"]
    for limit in (0, 1, 3):
        d = check(text, f"limit {limit}", max_allele_len=limit)
        assert (int(d["skipped"].sum()) > 0) == (limit == 1 or limit == 3)


@pytest.mark.gpu
@pytest.mark.parametrize("file", ["layout_snp8_600.gfa", "layout_snp8_600_rc3.gfa"])
def test_device_round_trip_on_the_snp_graphs(gpu, file):
    text = open(os.path.join(ROOT, "tests", "golden", file)).read()
    names = vi.names_of(text)
    for ref in (names[0], names[2]):
        dev = check(text, f"{file} ref={ref}", ref=ref)
        for p in range(8):
            built, own = vi.round_trip(dev, text, p)
            assert built == own


def write_fasta(path, recs):
    path.write_bytes(b"".join(b">" + n.encode() + b"\n" + s + b"\n" for n, s in recs))


def _run(cmd, **kw):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, **kw)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


@pytest.mark.gpu
def test_both_command_lines_and_the_tool_write_the_same_files(gpu, tmp_path):
    recs = synth.snp_family(5, 400, 0.05, 97, rc_every=2)
    fa = tmp_path / "in.fa"
    write_fasta(fa, recs)
    env = dict(os.environ, PYTHONPATH=ROOT)
    py = [sys.executable, "-m", "seqrush_amd"]
    ref = recs[2][0]
    files = {}
    for tag, cmd, kw in (("c", [EXE], {}), ("p", py, dict(cwd=ROOT, env=env))):
        gfa, vcf, gfa2, vcf2 = (tmp_path / f"{tag}{x}" for x in (".gfa", ".vcf", "_r.gfa", "_r.vcf"))
        out = _run(cmd + ["-s", str(fa), "-o", str(gfa), "--sort", "--vcf", str(vcf), "-v"], **kw)
        assert f"VCF written to {vcf}" in out and out.count("Variants stage:") == 1
        _run(cmd + ["-s", str(fa), "-o", str(gfa2), "--sort", "--vcf", str(vcf2), "--vcf-ref", ref, "--vcf-max-allele-len", "1"], **kw)
        files[tag] = (gfa.read_text(), vcf.read_text(), gfa2.read_text(), vcf2.read_text())
    assert files["c"] == files["p"]
    text = files["c"][0]
    assert files["c"][1] == variants_vcf(text, TWIN) == variants_vcf(text, 0) and files["c"][1].count("\n") > 12
    assert files["c"][3] == variants_vcf(text, TWIN, ref=ref, max_allele_len=1) and f"##contig=<ID={ref}," in files["c"][3]
    tool = tmp_path / "t.vcf"
    _run([sys.executable, "-m", "seqrush_amd.variants", str(tmp_path / "c.gfa"), "--device", "0", "-o", str(tool)], cwd=ROOT, env=env)
    assert tool.read_text() == files["c"][1]


@pytest.mark.gpu
def test_multi_gpu_writes_the_file_once(gpu, tmp_path):
    recs = synth.snp_family(6, 500, 0.05, 711, rc_every=3)
    fa = tmp_path / "in.fa"
    write_fasta(fa, recs)
    env = dict(os.environ, SR_BENCH_SINGLE_DEVICE="1", PYTHONPATH=ROOT, MASTER_PORT="29643")
    g1, g2, t1, t2 = (tmp_path / n for n in ("g1.gfa", "g2.gfa", "t1.vcf", "t2.vcf"))
    base = [sys.executable, "-m", "seqrush_amd", "-s", str(fa), "--no-sort"]
    _run(base + ["-o", str(g1), "--vcf", str(t1)], env=env, cwd=ROOT)
    stdout = _run(base + ["-o", str(g2), "--vcf", str(t2), "--gpus", "2"], env=env, cwd=ROOT)
    assert g1.read_text() == g2.read_text() and t1.read_text() == t2.read_text()
    assert stdout.count("VCF written to") == 1
    assert t1.read_text() == variants_vcf(g1.read_text(), TWIN)
