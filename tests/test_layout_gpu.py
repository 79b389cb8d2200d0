"""GPU tests of the 2-D layout: the device end points against the host twin, compared as raw 8-byte
words, and run to run, on the smallest shapes that reach each way the kernels can go wrong; then a graph a Context builds,
through both command lines.  No test compares coordinates between different executions except the bitwise twin
comparison: a 2-D layout is defined only up to an isometry."""
import os
import subprocess
import sys

import pytest

import layout_helpers as lh
from seqrush_amd import synth
from seqrush_amd.seqrush import Context, Params, SeqSet, SortParams, layout_gfa, layout_stats, layout_svg, layout_tsv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "seqrush_amd", "seqrush_mi355x")
TWIN = -1

CASES = [
    # the smallest live term; same-step / other-end terms hold each node to its length
    ("two_nodes", lh.two_nodes, {}),
    # reverse steps and a node visited in both orientations: the end flip
    ("reverse_steps", lh.reverse_steps, {}),
    # a node repeated inside one path and a self-loop L line: both end points of a term in one record, or one end point
    ("repeats_and_loop", lh.repeats_and_loop, {}),
    # 64 paths x 60 shared nodes: contended atomics; sub-rounds of 1000 terms (no multiple of 256, fewer than the terms per
    # iteration: several sub-rounds and a ragged tail); 7 iterations cross the cooling boundary
    ("hub", lh.hub, dict(terms_per_round=1000, iter_max=6)),
    # 600 end points: the apply kernel's tail falls past one workgroup; default parameters
    ("chain300", lh.chain, {}),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,make,params", CASES, ids=[c[0] for c in CASES])
def test_device_equals_twin_bit_for_bit(gpu, name, make, params):
    text = make().text()
    dev = layout_gfa(text, device=0, **params)
    st = layout_stats()
    twin = layout_gfa(text, device=TWIN, **params)
    assert lh.words(dev) == lh.words(twin), name + " (device against twin)"
    assert lh.words(layout_gfa(text, device=0, **params)) == lh.words(dev), name + " (device run to run)"
    assert st["sgd_ms"] > 0 and st["nodes"] == len(dev)
    if name == "hub":
        assert st["subrounds_per_iter"] > 1 and st["terms_per_iter"] % 1000 != 0 and st["iterations"] == 7
    assert lh.words(dev) != lh.words(lh.initial_state(make()))


def write_fasta(path, recs):
    path.write_bytes(b"".join(b">" + n.encode() + b"\n" + s + b"\n" for n, s in recs))


def _run(cmd, **kw):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, **kw)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


@pytest.mark.gpu
def test_context_graph_through_both_command_lines(gpu, tmp_path):
    recs = synth.snp_family(8, 600, 0.05, 211, rc_every=3)
    ctx = Context(0)
    ctx.load(SeqSet(recs), Params())
    ctx.run()
    ctx.sync()
    text = ctx.build_gfa(compact=True, sort=SortParams(device=0))[0]
    ctx.close()
    dev = layout_gfa(text, device=0)
    assert layout_stats()["sgd_ms"] > 0
    assert lh.words(dev) == lh.words(layout_gfa(text, device=TWIN))
    tsv, svg = layout_tsv(dev), layout_svg(text, dev)
    fa = tmp_path / "in.fa"
    write_fasta(fa, recs)
    env = dict(os.environ, PYTHONPATH=ROOT)
    for tag, cmd, kw in (("c", [EXE], {}), ("p", [sys.executable, "-m", "seqrush_amd"], dict(cwd=ROOT, env=env))):
        plain, gfa, lay, pic = (tmp_path / f"{tag}{s}" for s in ("_plain.gfa", ".gfa", ".lay.tsv", ".svg"))
        _run(cmd + ["-s", str(fa), "-o", str(plain), "--sort"], **kw)
        out = _run(cmd + ["-s", str(fa), "-o", str(gfa), "--sort", "--layout", str(lay), "--layout-svg", str(pic)], **kw)
        assert out.count(f"Layout written to {lay}\n") == 1
        assert plain.read_text() == gfa.read_text() == text          # --layout leaves the GFA alone
        assert lay.read_text() == tsv and pic.read_text() == svg
