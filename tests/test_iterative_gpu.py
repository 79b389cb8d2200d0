"""--iterative on the MI355X (-m gpu): the device run (tree batches, then windows of chunks with unite / count / decide on
the stream) against an independent Python restatement over the oracle, the plain tree: path, window invariance, PAF
round trip, both CLIs and the bounds-checked build."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_binding as ob
from seqrush_amd import synth
from seqrush_amd.seqrush import Context, Params, SeqSet
from conftest import canon_gfa

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "seqrush_amd", "seqrush_mi355x")

# (records, -x spec, -k): one input that stabilizes after its counts changed, one with fewer than 10 checks (never), one with
# reverse-complemented members and -k > 0
CASES = {
    "stabilizes": (lambda: synth.snp_family(40, 300, 0.02, 905), "tree:1,0,1.0", 0),
    "never": (lambda: synth.snp_family(10, 400, 0.03, 903), "tree:1,1,1.0", 0),
    "rc_k5": (lambda: synth.snp_family(48, 250, 0.01, 906, rc_every=4), "tree:1,0,1.0", 5),
}


def splitmix64(x):
    M = (1 << 64) - 1
    x = (x + 0x9e3779b97f4a7c15) & M
    x = ((x ^ (x >> 30)) * 0xbf58476d1ce4e5b9) & M
    x = ((x ^ (x >> 27)) * 0x94d049bb133111eb) & M
    return x ^ (x >> 31)


def expand(entries):
    return [p for i, j in entries for p in ((i, i), (i, j), (j, i), (j, j))]


def restate(recs, spec, k=0, seed=42):
    """align_and_unite_iterative (src/seqrush.rs:867-1132) as a Python loop over the oracle: tree entries from the k-NN
    part of the spec (rf = 0), random entries = the rest of the spec's list in the documented hash order, chunks of 10,
    count_components after every full chunk, stop after 10 unchanged counts"""
    parts = spec.split(":")[1].split(",")
    kn, kf, rf, km = parts + ["0", "0", "0", "16"][len(parts):]
    o = ob.OracleSeqRush(records=recs)
    n = o.n
    op = ob.default_params(); op.threads = 8; op.min_match_len = k
    tree = sorted({(q, t) for q, t in o.sparsified_pairs(f"tree:{kn},{kf},0,{km}", seed) if q < t})
    full = {(q, t) for q, t in o.sparsified_pairs(spec, seed) if q < t}
    rnd = sorted(full - set(tree), key=lambda e: (splitmix64(seed ^ (e[0] * n + e[1])), e[0], e[1]))
    o.align_and_unite_list(op, expand(tree))
    post = o.count_components()
    counts, prev, stable, processed, stop = [], post, 0, len(rnd), False
    for c0 in range(0, len(rnd), 10):
        chunk = rnd[c0:c0 + 10]
        o.align_and_unite_list(op, expand(chunk))
        if len(chunk) < 10:
            break
        c = o.count_components()
        counts.append(c)
        if c == prev:
            stable += 1
            if stable >= 10:
                processed, stop = c0 + 10, True
                break
        else:
            stable = 0
        prev = c
    return dict(tree=tree, random=rnd, post_tree=post, check_counts=counts, stabilized=stop, processed=processed,
                final=o.count_components(), labels=o.canonical_labels(), gfa=o.gfa(canonical=True)[0])


def run_product(recs, spec, k=0, keep=False):
    ss = SeqSet(recs)
    ctx = Context(0)
    p = Params(sparsification=spec)
    p.c.min_match_len = k
    ctx.load_iterative(ss, p, keep_alignments=keep)
    ctx.run_iterative()
    ctx.sync()
    st = ctx.iterative_stats()
    labels = ctx.download_labels()
    gfa = ctx.build_gfa(compact=False)[0]
    st["pairs"] = ctx.pairs()
    al = ctx.iterative_alignments() if keep else None
    ctx.close()
    return st, labels, gfa, al


def check_case(name):
    mk, spec, k = CASES[name]
    recs = mk()
    ref = restate(recs, spec, k)
    st, labels, gfa, _ = run_product(recs, spec, k)
    assert (st["tree_entries"], st["random_entries"]) == (len(ref["tree"]), len(ref["random"]))
    assert st["pairs"] == expand(ref["tree"]) + expand(ref["random"])
    assert st["post_tree"] == ref["post_tree"]
    assert st["check_counts"] == ref["check_counts"]
    assert st["checks"] == len(ref["check_counts"])
    assert st["stabilized"] == ref["stabilized"] and st["random_processed"] == ref["processed"]
    assert st["final_components"] == ref["final"]
    assert st["random_processed"] <= st["random_aligned"] <= st["random_entries"]
    assert np.array_equal(labels, ref["labels"])
    assert canon_gfa(gfa) == canon_gfa(ref["gfa"])
    return st, ref


@pytest.mark.parametrize("name", list(CASES))
def test_matches_oracle_restatement(gpu, name):
    st, ref = check_case(name)
    if name == "stabilizes":
        assert st["stabilized"] and st["random_processed"] < st["random_entries"]
        assert len(set(st["check_counts"])) > 1                 # the counts moved before they settled
        assert st["windows"] > 1
    if name == "never":
        assert not st["stabilized"] and st["random_processed"] == st["random_entries"]


def test_equals_plain_path_and_processed_prefix(gpu):
    # never stabilizes: every entry is processed -> the partition of plain -x tree:
    recs, spec, _ = CASES["never"][0](), CASES["never"][1], 0
    st, labels, gfa, _ = run_product(recs, spec)
    ctx = Context(0); ctx.load(SeqSet(recs), Params(sparsification=spec)); ctx.run(); ctx.sync()
    assert np.array_equal(ctx.download_labels(), labels)
    assert ctx.build_gfa(compact=False)[0] == gfa
    ctx.close()
    # stabilizes: the labels of an explicit pair list over the processed prefix
    recs, spec, _ = CASES["stabilizes"][0](), CASES["stabilizes"][1], 0
    st, labels, _, _ = run_product(recs, spec)
    m = 4 * (st["tree_entries"] + st["random_processed"])
    ctx = Context(0); ctx.load_pairs(SeqSet(recs), Params(), st["pairs"][:m]); ctx.run(); ctx.sync()
    assert np.array_equal(ctx.download_labels(), labels)
    ctx.close()


def test_window_invariance(gpu, monkeypatch):
    recs, spec, _ = CASES["stabilizes"][0](), CASES["stabilizes"][1], 0
    st0, labels0, gfa0, _ = run_product(recs, spec)
    monkeypatch.setenv("SR_CIGAR_ARENA_OPS", "1")            # raised to one chunk: every window is one chunk
    st1, labels1, gfa1, _ = run_product(recs, spec)
    assert st1["windows"] > st0["windows"] > 1
    assert st1["random_aligned"] == st1["random_processed"]  # one-chunk windows discard nothing
    for key in ("tree_entries", "random_entries", "random_processed", "checks", "post_tree", "final_components", "stabilized",
                "check_counts"):
        assert st1[key] == st0[key], key
    assert np.array_equal(labels0, labels1) and gfa0 == gfa1


def write_fasta(path, recs):
    path.write_bytes(b"".join(b">" + n.encode() + b"\n" + s + b"\n" for n, s in recs))
    return str(path)


def test_output_alignments_and_replay(gpu, tmp_path):
    from seqrush_amd.__main__ import main as pymain
    recs = CASES["stabilizes"][0]()
    fa = write_fasta(tmp_path / "in.fa", recs)
    st, _, _, al = run_product(recs, CASES["stabilizes"][1], keep=True)
    assert al.n == 4 * (st["tree_entries"] + st["random_processed"])
    assert list(zip(al.query_idx.tolist(), al.target_idx.tolist())) == st["pairs"][:al.n]
    paf, g1, g2 = tmp_path / "o.paf", tmp_path / "i.gfa", tmp_path / "p.gfa"
    assert pymain(["-s", fa, "-o", str(g1), "--no-sort", "--iterative", "-x", CASES["stabilizes"][1],
                   "--output-alignments", str(paf)]) == 0
    assert len(paf.read_text().strip().split("\n")) == al.n
    assert pymain(["-s", fa, "-o", str(g2), "--no-sort", "-p", str(paf)]) == 0
    assert canon_gfa(g2.read_text()) == canon_gfa(g1.read_text())
    r = subprocess.run([EXE, "-s", fa, "-o", str(tmp_path / "c.gfa"), "--no-sort", "--iterative", "-x", CASES["stabilizes"][1],
                        "--output-alignments", str(tmp_path / "c.paf")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "c.paf").read_text() == paf.read_text()


def _iter_lines(text):
    keys = ("Using iterative", "Processing ", "Phase ", "Graph stabilized", "Skipped ", "Final component", "  After ")
    return [x for x in text.split("\n") if x.startswith(keys)]


@pytest.mark.parametrize("sort", [False, True])
def test_cli_output_and_cross_cli_gfa(gpu, tmp_path, capsys, sort):
    from seqrush_amd.__main__ import main as pymain
    recs, spec = CASES["stabilizes"][0](), CASES["stabilizes"][1]
    fa = write_fasta(tmp_path / "in.fa", recs)
    st, _, _, _ = run_product(recs, spec)
    mode = ["--sort"] if sort else ["--no-sort"]
    capsys.readouterr()
    assert pymain(["-s", fa, "-o", str(tmp_path / "py.gfa"), "--iterative", "-x", spec, "-v"] + mode) == 0
    py_out = capsys.readouterr().out
    r = subprocess.run([EXE, "-s", fa, "-o", str(tmp_path / "cpp.gfa"), "--iterative", "-x", spec, "-v"] + mode,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "py.gfa").read_bytes() == (tmp_path / "cpp.gfa").read_bytes()
    assert _iter_lines(py_out) == _iter_lines(r.stdout)
    lines = _iter_lines(r.stdout)
    R, M = st["random_entries"], st["random_processed"]
    assert lines[0] == "Using iterative alignment with stabilization detection"
    assert lines[1] == f"Processing {st['tree_entries']} tree pairs (k=1, k_far=0) + {R} random pairs (frac=1)"
    assert f"Phase 1 complete: {st['post_tree']} components after tree pairs" in lines
    assert f"Graph stabilized after {M} random pairs ({st['check_counts'][-1]} components)" in lines
    skipped = [x for x in lines if x.startswith("Skipped ")]
    assert skipped and skipped[0].startswith(f"Skipped {R - M} random pairs (")
    assert sum(x.startswith("  After ") for x in lines) == st["checks"]
    assert lines[-1] == f"Final component count: {st['final_components']}"


def test_non_tree_spec_uses_default_tree(gpu, tmp_path):
    recs = synth.snp_family(24, 300, 0.02, 911)
    fa = write_fasta(tmp_path / "in.fa", recs)
    outs = {}
    for spec in ("none", "tree:3,3,0.1,16"):
        r = subprocess.run([EXE, "-s", fa, "-o", str(tmp_path / f"{spec}.gfa"), "--no-sort", "--iterative", "-x", spec],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        note = "Note: Iterative mode works best with tree sampling. Using default tree:3,3,0.1,16"
        assert (note in r.stderr) == (spec == "none")
        outs[spec] = ((tmp_path / f"{spec}.gfa").read_bytes(), _iter_lines(r.stdout))
    assert outs["none"] == outs["tree:3,3,0.1,16"]
    st, _, _, _ = run_product(recs, "none")
    assert st["tree_defaulted"] and (st["tree_k_nearest"], st["tree_k_farthest"], st["tree_rand_frac"], st["tree_kmer"]) == (3, 3, 0.1, 16)
    r = subprocess.run([EXE, "-s", fa, "-o", str(tmp_path / "bad.gfa"), "--no-sort", "--iterative", "-x", "bogus"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and not (tmp_path / "bad.gfa").exists()


@pytest.mark.parametrize("n", [1, 2])
def test_one_and_two_sequences(gpu, n):
    recs = synth.snp_family(n, 500, 0.03, 913)
    ref = restate(recs, "tree:3,3,0.1,16")
    st, labels, gfa, _ = run_product(recs, "tree:3,3,0.1,16")
    assert st["tree_entries"] == len(ref["tree"]) == (n - 1) and st["random_entries"] == 0
    assert st["post_tree"] == st["final_components"] == ref["final"]
    assert np.array_equal(labels, ref["labels"]) and canon_gfa(gfa) == canon_gfa(ref["gfa"])


def test_bounds_checked_build(gpu):
    """one restatement case through libseqrush_amd_bounds.so (the bounds-checked blocked kernel).  A subprocess: the library
    is chosen at load time."""
    lib = os.path.join(ROOT, "seqrush_amd", "libseqrush_amd_bounds.so")
    assert os.path.exists(lib)
    code = ("import sys; sys.path.insert(0, 'tests'); import torch; import test_iterative_gpu as t\n"
            "from seqrush_amd.seqrush import SeqSet, Params, Context\n"
            "c = Context(0); c.load_iterative(SeqSet(t.CASES['rc_k5'][0]()), Params(sparsification='tree:1,0,1.0'))\n"
            "assert c.workspace_report()['kernel_build'] == 'bounds'; c.close()\n"
            "t.check_case('rc_k5'); t.check_case('stabilizes'); print('bounds iterative clean')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, SEQRUSH_AMD_LIB=lib), capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0 and "bounds iterative clean" in r.stdout, (r.stdout[-800:], r.stderr[-1500:])
