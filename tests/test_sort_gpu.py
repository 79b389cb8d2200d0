"""The Ygs layout (--sort) on the MI355X: device SGD positions bit-identical to the host twin, byte-identical sorted GFAs
from both CLIs, across runs, processes and --gpus 2, and the same-graph / ordering checks on the C2 graph."""
import os
import subprocess
import sys

import pytest

import sort_helpers as sh
from seqrush_amd import synth
from seqrush_amd.seqrush import Context, Params, SeqSet, SortParams, sgd_layout, sort_gfa, sort_stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "seqrush_amd", "seqrush_mi355x")
TWIN = -1

CONFIGS = {
    "c1": synth.config_c1,
    "snp_rc": lambda: synth.snp_family(8, 1000, 0.05, 141, rc_every=3),
    "c3": synth.config_c3_like,
    "c5": synth.config_c5_like,
    "c2": synth.config_c2,
}
_UNSORTED = {}


def unsorted_gfa(name, compact=True):
    """the --no-sort graph of a config, induced on the device"""
    key = (name, compact)
    if key not in _UNSORTED:
        recs = CONFIGS[name]()
        ss = SeqSet(recs)
        ctx = Context(0)
        ctx.load(ss, Params())
        ctx.run()
        ctx.sync()
        _UNSORTED[key] = (recs, ctx.build_gfa(compact=compact)[0])
        ctx.close()
    return _UNSORTED[key]


def write_fasta(path, recs):
    path.write_bytes(b"".join(b">" + n.encode() + b"\n" + s + b"\n" for n, s in recs))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c1", "snp_rc", "c3", "c5", "c2"])
def test_device_sgd_bit_identical_to_host_twin(gpu, name):
    _, text = unsorted_gfa(name)
    dev = sgd_layout(text, device=0)
    st = sort_stats()
    twin = sgd_layout(text, device=TWIN)
    assert dev.tobytes() == twin.tobytes()
    assert st["sgd_ms"] > 0
    assert sgd_layout(text, device=0).tobytes() == dev.tobytes()
    # a batch that splits iterations into many sub-rounds, too
    assert sgd_layout(text, device=0, terms_per_round=1000, iter_max=10).tobytes() == \
        sgd_layout(text, device=TWIN, terms_per_round=1000, iter_max=10).tobytes()


def _cli_pair(tmp_path, recs, extra, tag):
    fa = tmp_path / "in.fa"
    write_fasta(fa, recs)
    out_c, out_p = tmp_path / f"c_{tag}.gfa", tmp_path / f"p_{tag}.gfa"
    r = subprocess.run([EXE, "-s", str(fa), "-o", str(out_c), "--sort"] + extra, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([sys.executable, "-m", "seqrush_amd", "-s", str(fa), "-o", str(out_p), "--sort"] + extra,
                       capture_output=True, text=True, timeout=600, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stderr
    return out_c.read_text(), out_p.read_text()


@pytest.mark.gpu
@pytest.mark.parametrize("compact", [True, False])
def test_cli_sort_byte_identical_everywhere(gpu, tmp_path, compact):
    recs = synth.snp_family(8, 1000, 0.05, 141, rc_every=3)
    extra = [] if compact else ["--no-compact"]
    c1, p1 = _cli_pair(tmp_path, recs, extra, "a")
    c2, p2 = _cli_pair(tmp_path, recs, extra, "b")            # fresh processes
    assert c1 == p1 == c2 == p2
    ss = SeqSet(recs)
    ctx = Context(0)
    ctx.load(ss, Params())
    ctx.run()
    ctx.sync()
    unsorted = ctx.build_gfa(compact=compact)[0]
    in_proc = [ctx.build_gfa(compact=compact, sort=SortParams(device=0))[0] for _ in range(2)]
    ctx.close()
    assert in_proc[0] == in_proc[1] == c1
    assert sort_gfa(unsorted, device=TWIN) == c1              # the host twin's sort of the same unsorted graph
    sh.check_same_graph(sh.Gfa.parse(unsorted), sh.Gfa.parse(c1), want_spellings={n: s.decode() for n, s in recs})


@pytest.mark.gpu
def test_cli_sort_flags_reach_the_sort(gpu, tmp_path):
    recs = synth.snp_family(5, 600, 0.05, 77)
    base_c, base_p = _cli_pair(tmp_path, recs, [], "base")
    seed_c, seed_p = _cli_pair(tmp_path, recs, ["--sort-seed", "5", "--sgd-iter-max", "20"], "seed")
    skip_c, skip_p = _cli_pair(tmp_path, recs, ["--skip-sgd", "--skip-groom", "--skip-topo"], "skip")
    assert base_c == base_p and seed_c == seed_p and skip_c == skip_p
    ss = SeqSet(recs)
    ctx = Context(0)
    ctx.load(ss, Params())
    ctx.run()
    ctx.sync()
    unsorted = ctx.build_gfa(compact=True)[0]
    ctx.close()
    assert seed_c == sort_gfa(unsorted, device=TWIN, seed=5, iter_max=20)
    assert skip_c == sort_gfa(unsorted, device=TWIN, skip_sgd=1, skip_groom=1, skip_topo=1)


@pytest.mark.gpu
def test_c2_sorted_by_device_is_the_same_graph_in_order(gpu):
    """C2 at -k 0 is single-orientation but not acyclic (paths revisit nodes), so ids cannot increase along every path:
    it must come out as the same graph with every step forward; an acyclic snp input comes out strictly increasing"""
    recs, text = unsorted_gfa("c2")
    before = sh.Gfa.parse(text)
    perm, _ = before.permuted(3)
    for g in (before, perm):
        out = sh.Gfa.parse(sort_gfa(g.text(), device=0))
        sh.check_same_graph(g, out, want_spellings={n: s.decode() for n, s in recs})
        assert all(h & 1 == 0 for _, st in out.paths for h in st)
    recs = synth.snp_family(8, 2000, 0.05, 2001)
    ss = SeqSet(recs)
    ctx = Context(0)
    ctx.load(ss, Params(min_match_len=8))
    ctx.run()
    ctx.sync()
    g = sh.Gfa.parse(ctx.build_gfa(compact=True)[0])
    ctx.close()
    assert sh.acyclic_forward(g)
    out = sh.Gfa.parse(sort_gfa(g.permuted(4)[0].text(), device=0))
    for pname, st in out.paths:
        ids = [h >> 1 for h in st]
        assert all(h & 1 == 0 for h in st) and all(a < b for a, b in zip(ids, ids[1:])), pname


@pytest.mark.gpu
def test_multi_gpu_sort_matches_single(gpu, tmp_path):
    recs = synth.snp_family(6, 500, 0.05, 711, rc_every=3)
    fa = tmp_path / "in.fa"
    write_fasta(fa, recs)
    env = dict(os.environ, SR_BENCH_SINGLE_DEVICE="1", PYTHONPATH=ROOT, MASTER_PORT="29631")
    out1, out2 = tmp_path / "g1.gfa", tmp_path / "g2.gfa"
    r = subprocess.run([sys.executable, "-m", "seqrush_amd", "-s", str(fa), "-o", str(out1), "--sort"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([sys.executable, "-m", "seqrush_amd", "-s", str(fa), "-o", str(out2), "--sort", "--gpus", "2"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    assert out1.read_text() == out2.read_text()


@pytest.mark.gpu
def test_python_api_args_sort(gpu, tmp_path):
    """run_seqrush(Args(sort=True)) -- no_sort at its default -- writes what the CLIs write for --sort"""
    from seqrush_amd.seqrush import Args, run_seqrush
    recs = synth.snp_family(5, 600, 0.05, 79, rc_every=2)
    c, p = _cli_pair(tmp_path, recs, [], "api")
    out = tmp_path / "api.gfa"
    sr = run_seqrush(Args(sequences=str(tmp_path / "in.fa"), output=str(out), sort=True))
    sr.ctx.close()
    assert out.read_text() == c == p
