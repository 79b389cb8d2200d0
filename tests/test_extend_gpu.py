"""GPU tests of --extend.  On the seam graphs of extend_inputs the device plan spells the bytes of the
restatement, and the labels after load_extend + sync, with no run, are the host twin's.  On the two split families, extending
the product's graph of the first m sequences by the rest gives the labels and the GFA bytes of the one-shot build of all n and
the oracle's partition -- from the uncompacted graph, from the compacted one (host and device) and from the sorted one, with a
4-bit alphabet, and with a reverse-complemented new member.  Sparsified runs align the filtered list and equal the oracle over
the old list followed by the new one; reset_uf() on an extend context re-seeds; both command lines write the one-shot file."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import extend_inputs as ei
import oracle_binding as ob
from conftest import canon_gfa
from seqrush_amd.seqrush import (Context, ExtendPlan, HostUnionFind, Params, SeqSet, SortParams, extend_seed_host)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "seqrush_amd", "seqrush_mi355x")
SEAMS = ei.seam_cases()


# ------------------------------------------------------------------ seams
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SEAMS))
def test_device_plan_and_seed_on_the_seams(gpu, name):
    text, new = SEAMS[name]
    want = ei.restate(text, new)
    with ExtendPlan(text, new, device=0) as plan, ExtendPlan(text, new, device=-1) as host:
        assert plan.records == want["records"] == host.records, "merged bytes"
        uf = HostUnionFind(host.seqset.total_length)
        twin = extend_seed_host(host, uf)
        ctx = Context(0)
        ctx.load_extend(plan, Params())
        ctx.sync()
        assert np.array_equal(ctx.download_labels(), uf.canonical_labels())
        st = ctx.extend_stats()
        assert st["unions_attempted"] == len(want["unions"]) == twin["unions_attempted"]
        assert st["unions_joined"] == twin["unions_joined"]
        assert (st["old_paths"], st["old_bases"], st["old_steps"]) == (want["n_old"], want["old_bases"], want["steps"])
        n = len(want["records"])
        assert st["pairs_before"] == n * n and st["pairs_after"] == n * n - want["n_old"] ** 2 == ctx.num_pairs
        ctx.close()


# ------------------------------------------------------------------ split equality
def params(k, **kw):
    return Params(min_match_len=k, **kw)


def build(recs, k, **gfa):
    """the product's build of recs -> (labels, GFA text)"""
    ctx = Context(0)
    ctx.load(SeqSet(recs), params(k))
    ctx.run(); ctx.sync()
    lab = ctx.download_labels()
    text = ctx.build_gfa(**gfa)[0]
    ctx.close()
    return lab, text


def family(name):
    if name == "snp12_n_runs":                                     # runs of N: the 4-bit symbol build
        recs = ei.snp12(21)
        return [(n, s[:50 + 7 * i] + b"N" * (3 + i % 4) + s[60 + 7 * i:]) if i % 3 == 0 else (n, s) for i, (n, s) in enumerate(recs)]
    return ei.FAMILIES[name]()


@functools.lru_cache(maxsize=None)
def one_shot(name, k):
    lab, text = build(family(name), k, compact=False)
    lab.setflags(write=False)
    return lab, text


@functools.lru_cache(maxsize=None)
def oracle_all(name, k):
    o = ob.OracleSeqRush(records=family(name))
    p = ob.default_params(); p.min_match_len = k; p.threads = 4
    o.align_and_unite(p)
    lab, text = o.canonical_labels(), o.gfa(canonical=True)[0]
    o.close()
    lab.setflags(write=False)
    return lab, text


FORMS = {"plain": dict(compact=False), "compact_host": dict(compact=True), "compact_device": dict(compact=True, compact_on="device"),
         "sorted": dict(compact=True, sort=None)}


def extend(text, new, k, run=True):
    with ExtendPlan(text, new, device=0) as plan:
        ctx = Context(0)
        ctx.load_extend(plan, params(k))
        if run:
            ctx.run()
        ctx.sync()
        out = ctx.download_labels(), ctx.build_gfa(compact=False)[0], ctx.extend_stats()
        ctx.close()
        return out


def check_split(name, k, m, forms=FORMS):
    recs = family(name)
    want_lab, want_text = one_shot(name, k)
    o_lab, o_text = oracle_all(name, k)
    assert np.array_equal(want_lab, o_lab) and canon_gfa(want_text) == canon_gfa(o_text)
    for form, kw in forms.items():
        kw = dict(kw, sort=SortParams(device=0)) if form == "sorted" else kw
        _, text_m = build(recs[:m], k, **kw)
        lab, text, st = extend(text_m, recs[m:], k)
        assert np.array_equal(lab, want_lab), (name, k, m, form)
        assert text == want_text, (name, k, m, form)
        n = len(recs)
        assert st["pairs_after"] == n * n - m * m and st["new_sequences"] == n - m


SPLITS = [(f, k, m) for f in sorted(ei.FAMILIES) for k in (0, 8) for m in ei.splits(len(ei.FAMILIES[f]()))]


@pytest.mark.gpu
@pytest.mark.parametrize("name,k,m", SPLITS, ids=[f"{f}-k{k}-m{m}" for f, k, m in SPLITS])
def test_extending_equals_the_one_shot_build(gpu, name, k, m):
    check_split(name, k, m)


@pytest.mark.gpu
def test_four_bit_alphabet_and_reverse_complement_member(gpu):
    recs = family("snp12_n_runs")
    ctx = Context(0)
    ctx.load(SeqSet(recs), Params())
    assert ctx.workspace_report()["symbol_bits"] == 4
    ctx.close()
    check_split("snp12_n_runs", 0, 6)
    rc = ei.snp12()
    assert rc[11][1] != ei.revcomp(rc[11][1]) and sum(a == b for a, b in zip(ei.revcomp(rc[11][1]), rc[0][1])) > 350
    check_split("snp12", 8, 11, {"plain": FORMS["plain"], "sorted": FORMS["sorted"]})     # the new member is a reverse complement


# ------------------------------------------------------------------ sparsified
@pytest.mark.gpu
def test_sparsified_extend_equals_the_oracle_over_both_lists(gpu):
    recs, m, spec = ei.indel8(), 5, "tree:2,1,0.5"
    ctx = Context(0)
    ctx.load(SeqSet(recs[:m]), Params(sparsification=spec))
    p_old = ctx.pairs()
    ctx.run(); ctx.sync()
    text_m = ctx.build_gfa(compact=False)[0]
    ctx.close()
    full = Context(0)
    full.load(SeqSet(recs), Params(sparsification=spec))
    p_all = full.pairs()
    full.close()
    with ExtendPlan(text_m, recs[m:], device=0) as plan:
        ctx = Context(0)
        ctx.load_extend(plan, Params(sparsification=spec))
        p_new = ctx.pairs()
        assert p_new == plan.pair_list(p_all) == ei.py_filter(p_all, m) and 0 < len(p_new) < len(p_all)
        ctx.run(); ctx.sync()
        lab = ctx.download_labels()
        ctx.close()
    o = ob.OracleSeqRush(records=recs)
    op = ob.default_params(); op.threads = 4
    o.align_and_unite_list(op, p_old + p_new)
    assert np.array_equal(lab, o.canonical_labels())
    o.close()


# ------------------------------------------------------------------ reset_uf
@pytest.mark.gpu
def test_reset_uf_reseeds_an_extend_context_only(gpu):
    recs, m = ei.indel8(), 4
    want_lab, _ = one_shot("indel8", 0)
    _, text_m = build(recs[:m], 0, compact=False)
    with ExtendPlan(text_m, recs[m:], device=0) as plan:
        ctx = Context(0)
        ctx.load_extend(plan, params(0))
        ctx.sync()
        seeded = ctx.download_labels()
        ctx.run(); ctx.sync()
        assert np.array_equal(ctx.download_labels(), want_lab)
        ctx.reset_uf(); ctx.sync()
        assert np.array_equal(ctx.download_labels(), seeded) and not np.array_equal(seeded, want_lab)
        ctx.run(); ctx.sync()
        assert np.array_equal(ctx.download_labels(), want_lab)
        # the same context loaded normally afterwards: reset_uf is the SeqRush::new state again
        ctx.load(SeqSet(recs), params(0))
        ctx.run(); ctx.sync()
        ctx.reset_uf(); ctx.sync()
        fresh = HostUnionFind(sum(len(s) for _, s in recs)).canonical_labels()
        assert np.array_equal(ctx.download_labels(), fresh)
        ctx.run(); ctx.sync()
        assert np.array_equal(ctx.download_labels(), want_lab)
        ctx.close()


# ------------------------------------------------------------------ both command lines
def write_fasta(path, recs):
    path.write_bytes(b"".join(b">" + n.encode() + b"\n" + s + b"\n" for n, s in recs))


def _run(cmd):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    return r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("front", ["python", "exe"])
def test_command_lines_write_the_one_shot_file(gpu, front, tmp_path):
    recs, m = ei.indel8(), 5
    cmd = [sys.executable, "-m", "seqrush_amd"] if front == "python" else [EXE]
    write_fasta(tmp_path / "all.fa", recs); write_fasta(tmp_path / "old.fa", recs[:m]); write_fasta(tmp_path / "new.fa", recs[m:])
    for tag, flags in (("nosort", ["--no-sort"]), ("sort", ["--sort", "--stats"])):
        def out(stem):
            o = ["-o", str(tmp_path / f"{stem}_{tag}.gfa"), "-k", "8"] + flags
            return o + [str(tmp_path / f"{stem}_{tag}.tsv")] if tag == "sort" else o
        _run(cmd + ["-s", str(tmp_path / "all.fa")] + out("all"))
        _run(cmd + ["-s", str(tmp_path / "old.fa")] + out("old"))
        log = _run(cmd + ["-s", str(tmp_path / "new.fa"), "--extend", str(tmp_path / f"old_{tag}.gfa"), "-v"] + out("ext"))
        assert (tmp_path / f"ext_{tag}.gfa").read_bytes() == (tmp_path / f"all_{tag}.gfa").read_bytes(), (front, tag)
        if tag == "sort":
            assert (tmp_path / f"ext_{tag}.tsv").read_bytes() == (tmp_path / f"all_{tag}.tsv").read_bytes()
        n = len(recs)
        assert f"Extending {m} paths by {n - m} sequences: {n * n - m * m} pairs to align" in log
        line = next(l for l in log.split("\n") if l.startswith("Extend: "))
        assert f"{m} paths" in line and f"pairs {n * n - m * m} of {n * n}" in line and "seed_us=" in line
    # only the new pairs' records with --output-alignments
    _run(cmd + ["-s", str(tmp_path / "new.fa"), "--extend", str(tmp_path / "old_nosort.gfa"), "--no-sort", "-k", "8", "-o",
                str(tmp_path / "paf.gfa"), "--output-alignments", str(tmp_path / "new.paf")])
    assert (tmp_path / "paf.gfa").read_bytes() == (tmp_path / "all_nosort.gfa").read_bytes()
    names = [n for n, _ in recs]
    got = [(l.split("\t")[0], l.split("\t")[5]) for l in (tmp_path / "new.paf").read_text().split("\n") if l]
    assert len(got) == n * n - m * m and all(not (names.index(q) < m and names.index(t) < m) for q, t in got)


# ------------------------------------------------------------------ the bounds-checked library
def bounds_child():
    check_split("indel8", 0, 4, {"plain": FORMS["plain"]})
    ctx = Context(0)
    ctx.load(SeqSet(ei.indel8()), Params())
    assert ctx.workspace_report()["kernel_build"] == "bounds"
    ctx.close()
    print("bounds build clean")


@pytest.mark.gpu
def test_bounds_checked_build_when_present(gpu):
    lib = os.path.join(ROOT, "seqrush_amd", "libseqrush_amd_bounds.so")
    assert os.path.exists(lib), "build() did not make libseqrush_amd_bounds.so"
    code = "import sys; sys.path.insert(0, 'tests'); import torch; import test_extend_gpu as t; t.bounds_child()"
    env = {k: v for k, v in os.environ.items() if not k.startswith("SR_")}
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(env, SEQRUSH_AMD_LIB=lib), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "bounds build clean" in r.stdout, (r.stdout[-800:], r.stderr[-1500:])
