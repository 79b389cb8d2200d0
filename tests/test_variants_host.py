"""CPU tests (-m "not gpu") of the variant sites through the host twin (device = -1): hand-checked
known answers, a restatement of the rule in Python, graphs built bubble by bubble whose sites and genotypes the
construction knows, the round trip (a path's alleles applied to the reference give the path back) on the committed SNP
graphs, max_allele_len, the refusals, the VCF bytes and the command line."""
import json
import os
import subprocess
import sys

import pytest

import growth_inputs as gi
import variants_inputs as vi
from seqrush_amd.seqrush import SeqRushError, Variants, variants, variants_vcf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOWN = json.load(open(os.path.join(ROOT, "tests", "golden", "variants_known_answers.json")))["cases"]
TWIN = -1
INPUTS = gi.host_inputs() + vi.bubble_inputs()


@pytest.mark.parametrize("case", KNOWN, ids=[c["name"] for c in KNOWN])
def test_known_answers(case):
    d = variants(case["gfa"], TWIN, ref=case["ref"])
    assert d["variant"] == 0 and d["hash_collision_sites"] == 0
    assert d["ref_seq"].decode() == case["ref_seq"] and d["anchors"] == case["anchors"] and d["traversals"] == case["traversals"]
    got = [[int(a), int(b), [x.decode() for x in al]] for a, b, al in zip(d["site_start"], d["site_end"], d["alleles"])]
    assert got == case["sites"] and d["gt"].tolist() == case["gt"]
    assert d["breaks"].tolist() == case["breaks"] and d["skipped"].tolist() == case["skipped"]
    assert variants_vcf(case["gfa"], TWIN, ref=case["ref"]) == case["vcf"]
    vi.assert_same(d, vi.restate(case["gfa"], case["ref"]), case["name"])


def test_the_known_answers_cover_what_they_name():
    by = {c["name"]: c for c in KNOWN}
    assert by["reference_revisits_a_node"]["traversals"] > 0 and by["reference_revisits_a_node"]["sites"] == []
    assert by["strand_switch_and_back_jump"]["breaks"] == [0, 1, 1]
    assert by["first_crossing_wins"]["gt"] == [[0, 2, 1]]
    assert "\t3\t.\tG\tGT\t" in by["insertion"]["vcf"] and "\t3\t.\tGT\tG\t" in by["deletion"]["vcf"]
    assert by["empty_graph"]["vcf"].count("\n") == 7 and "##contig" not in by["empty_graph"]["vcf"]


@pytest.mark.parametrize("name,text", INPUTS, ids=[n for n, _ in INPUTS])
def test_twin_equals_the_restatement(name, text):
    names = vi.names_of(text)
    for ref in ([None] if len(names) < 2 else [None, names[-1]]):
        with Variants(text, TWIN, ref) as v:
            d, vcf = v.as_dict(), v.vcf()
        vi.assert_same(d, vi.restate(text, ref), f"{name} ref={ref}")
        assert vcf == vi.report_of(d, names), f"{name} ref={ref}: VCF bytes"


@pytest.mark.parametrize("seed", range(20))
def test_twin_returns_the_constructed_sites_and_genotypes(seed):
    text, truth = vi.bubbles(seed, 40, 7)
    d = variants(text, TWIN)
    got = [(int(a), int(b), al) for a, b, al in zip(d["site_start"], d["site_end"], d["alleles"])]
    assert got == truth["sites"]
    assert d["gt"].tolist() == truth["gt"]
    assert not d["breaks"].any() and not d["skipped"].any()


@pytest.mark.parametrize("ref_index", [0, 2])
@pytest.mark.parametrize("file", ["layout_snp8_600.gfa", "layout_snp8_600_rc3.gfa"])
def test_round_trip_on_the_snp_graphs(file, ref_index):
    text = open(os.path.join(ROOT, "tests", "golden", file)).read()
    assert set("".join(st for st in vi.st.parse(text).seq.values())) <= set("ACGT")
    names = vi.names_of(text)
    d = variants(text, TWIN, ref=names[ref_index])
    assert d["ref_path"] == ref_index and d["paths"] == 8
    clean = [p for p in range(8) if d["breaks"][p] == 0 and d["skipped"][p] == 0]
    assert clean == list(range(8))                   # all 8 of 8 paths
    for p in clean:
        built, own = vi.round_trip(d, text, p)
        assert built == own, f"{file} ref {ref_index}: path {p}"
    if ref_index == 0:
        gt = d["gt"]
        assert (d["sites"], d["traversals"]) == (197, 378)
        assert (int((gt > 0).sum()), int((gt == 0).sum()), int((gt < 0).sum())) == (378, 1005, 193)


def test_max_allele_len_moves_records_into_skipped():
    text = vi.chain(3, 200, [150, 120], extra=[("gap", [5 << 1] + [(400 + k) << 1 for k in range(30)] + [9 << 1])])
    free = variants(text, TWIN, ref="ref", max_allele_len=0)
    assert not free["skipped"].any()
    want = vi.restate(text, "ref", 0)
    vi.assert_same(free, want, "no limit")
    longest = max(max(len(x) for x in al) for al in free["alleles"])
    assert longest >= 30
    for limit in (1, 2, longest - 1, longest):
        d = variants(text, TWIN, ref="ref", max_allele_len=limit)
        vi.assert_same(d, vi.restate(text, "ref", limit), f"limit {limit}")
        assert d["traversals"] + int(d["skipped"].sum()) == free["traversals"]
        assert (int(d["skipped"].sum()) == 0) == (limit == longest)


def test_options_and_refusals():
    text = KNOWN[0]["gfa"]
    with pytest.raises(SeqRushError, match="no path is named 'nobody'"):
        variants(text, TWIN, ref="nobody")
    with pytest.raises(SeqRushError, match="device must be >= -1"):
        variants(text, -2)
    with pytest.raises(SeqRushError, match="max_allele_len"):
        variants(text, TWIN, max_allele_len=-1)
    with pytest.raises(SeqRushError):
        variants("S\tx\tACGT\n", TWIN)
    many = vi.one_site(2 ** 13 + 2)                  # 1 site x 8194 paths is fine; the limit is on sites x paths
    assert variants(many, TWIN)["sites"] == 1
    from seqrush_amd import _lib
    L = _lib.load()
    prm = _lib.VariantParamsC()
    L.sr_variant_params_default(prm)
    assert (prm.ref_name, prm.max_allele_len, prm.hash_mask, prm.reserved) == (None, 10000, 2 ** 64 - 1, 0)
    assert L.sr_variants_gfa(None, prm, TWIN, None) != 0


def many_cells(sites, paths):
    """`sites` SNP sites carried by one sample, and paths of zero steps up to `paths` paths"""
    seq, ref, alt = {1: "A"}, [1], [1]
    for k in range(sites):
        seq[3 * k + 2], seq[3 * k + 3], seq[3 * k + 4] = "C", "G", "T"
        ref += [3 * k + 2, 3 * k + 4]
        alt += [3 * k + 3, 3 * k + 4]
    text = vi.sh.Gfa(seq, [], [("ref", [v << 1 for v in ref]), ("alt", [v << 1 for v in alt])]).text()
    return text + "".join(f"P\te{k}\t\t*\n" for k in range(paths - 2))


def test_sites_times_paths_above_the_limit_is_refused():
    assert variants(many_cells(2048, 40), TWIN)["gt"].shape == (2048, 40)
    with pytest.raises(SeqRushError, match="2048 sites x 32771 paths; the table supports at most 2\\^26 cells"):
        variants(many_cells(2048, 32771), TWIN)      # 2048 x 32771 = 2^26 + 6144


def _run(cmd, ok=True, **kw):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, **kw)
    assert (r.returncode == 0) == ok, r.stderr[-2000:]
    return r.stdout if ok else r.stderr


def test_the_tool_and_the_option_validation(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    text, _ = vi.bubbles(5, 20, 5)
    gfa, out = tmp_path / "g.gfa", tmp_path / "g.vcf"
    gfa.write_text(text)
    tool = [sys.executable, "-m", "seqrush_amd.variants", str(gfa), "--device", "-1"]
    _run(tool + ["-o", str(out)], cwd=ROOT, env=env)
    assert out.read_text() == variants_vcf(text, TWIN) == _run(tool, cwd=ROOT, env=env)
    _run(tool + ["-o", str(out), "--ref", "p2", "--max-allele-len", "2"], cwd=ROOT, env=env)
    assert out.read_text() == variants_vcf(text, TWIN, ref="p2", max_allele_len=2)
    assert "no path is named 'zz'" in _run(tool + ["--ref", "zz"], ok=False, cwd=ROOT, env=env)
    py = [sys.executable, "-m", "seqrush_amd", "-s", "x.fa"]
    exe = [os.path.join(ROOT, "seqrush_amd", "seqrush_mi355x"), "-s", "x.fa"]
    for front, kw in ((py, dict(cwd=ROOT, env=env)), (exe, {})):
        assert "Error: --vcf-ref is an option of --vcf: give both" in _run(front + ["--vcf-ref", "a"], ok=False, **kw)
        assert "Error: --vcf-max-allele-len is an option of --vcf: give both" in _run(front + ["--vcf-max-allele-len", "5"], ok=False, **kw)
    assert "Error: --vcf-max-allele-len needs a non-negative integer, got '-3'" in \
        _run(py + ["--vcf", "o.vcf", "--vcf-max-allele-len", "-3"], ok=False, cwd=ROOT, env=env)
    assert "Error: --vcf-max-allele-len needs a non-negative integer, got 'x'" in _run(exe + ["--vcf", "o.vcf", "--vcf-max-allele-len", "x"], ok=False)
