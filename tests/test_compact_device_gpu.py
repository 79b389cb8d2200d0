"""Compaction on the MI355X (--compact-on device, sr_compact.hip): byte-identical to the host procedure through
sr_compact_gfa, through a Context (the induced graph stays on the device), and through both CLIs."""
import os
import subprocess
import sys

import pytest

import compact_inputs as ci
import oracle_binding as ob
from seqrush_amd import synth
from seqrush_amd.seqrush import Context, Params, SeqRushError, SeqSet, SortParams, compact_gfa, compact_stats
from test_host_abi import COMPACT_CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "seqrush_amd", "seqrush_mi355x")
HOST = -1
REFUSAL = "Error: --compact-on device and --no-compact exclude each other"


def _oracle_gfa(recs, k):
    o = ob.OracleSeqRush(records=recs)
    p = ob.default_params(); p.min_match_len = k; p.threads = 2
    o.align_and_unite(p)
    return o.gfa(canonical=True)[0]


def _check(text, native=True):
    st = {}
    got = compact_gfa(text, 0, st)
    assert got == compact_gfa(text, HOST)
    assert compact_gfa(text, 0) == got                           # run to run
    if native:
        assert st["host_rounds"] == 0
    assert st["jumps"] <= st["rounds"] * 33
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(COMPACT_CASES))
@pytest.mark.parametrize("k", [0, 6])
def test_device_matches_host_on_induced_graphs(gpu, name, k):
    text = _oracle_gfa(COMPACT_CASES[name](), k)
    st, host = _check(text), {}
    compact_gfa(text, HOST, host)
    assert (st["rounds"], st["chains"]) == (host["rounds"], host["chains"])
    assert st["compact_us"] > 0
    _check(ci.permuted(text, 7 + k))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ci.HAND))
def test_device_matches_host_on_hand_written(gpu, name):
    text, may_fall_back = ci.HAND[name]
    st = _check(text, native=not may_fall_back)
    if name.startswith("cycle"):
        assert st["host_rounds"] >= 1


@pytest.mark.gpu
def test_device_matches_host_on_random_families(gpu):
    for seed in range(12):
        text = _oracle_gfa(ci.random_family(1000 + seed), (0, 6, 3)[seed % 3])
        _check(text)
        _check(ci.permuted(text, seed))


def _context(recs):
    ctx = Context(0)
    ctx.load(SeqSet(recs), Params())
    ctx.run()
    ctx.sync()
    return ctx


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["snp", "snp-rc", "c2-like"])
def test_context_compacts_on_device(gpu, name):
    """the induced arrays go from graph induction into compaction without visiting the host"""
    recs = {"snp": lambda: synth.snp_family(8, 600, 0.05, 211), "snp-rc": lambda: synth.snp_family(8, 600, 0.05, 212, rc_every=3),
            "c2-like": lambda: synth.snp_family(16, 1000, 0.05, 2001)}[name]()
    ctx = _context(recs)
    try:
        host = ctx.build_gfa(compact=True, compact_on="host")
        dev = ctx.build_gfa(compact=True, compact_on="device")
        st = compact_stats()
        assert dev == host and dev == ctx.build_gfa(compact=True, compact_on="device")
        assert st["host_rounds"] == 0 and st["chains"] > 0 and st["rounds"] >= 2 and st["compact_us"] > 0
        assert dev[0] == compact_gfa(ctx.build_gfa(compact=False)[0], 0)
        assert ci.spelled(dev[0]) == [(n, s.upper()) for n, s in recs]
        if name != "c2-like":
            sp = SortParams(device=0)
            assert ctx.build_gfa(compact=True, sort=sp, compact_on="device") == ctx.build_gfa(compact=True, sort=sp, compact_on="host")
        with pytest.raises(SeqRushError, match="exclude each other"):
            ctx.build_gfa(compact=False, compact_on="device")
    finally:
        ctx.close()


def _cli(cmd, **kw):
    return subprocess.run(cmd, capture_output=True, text=True, timeout=300, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("cli", ["native", "python"])
def test_cli_compact_on_device(gpu, tmp_path, cli):
    recs = synth.snp_family(6, 500, 0.05, 213, rc_every=4)
    fa = tmp_path / "in.fa"
    fa.write_bytes(b"".join(b">" + n.encode() + b"\n" + s + b"\n" for n, s in recs))
    head = [EXE] if cli == "native" else [sys.executable, "-m", "seqrush_amd"]
    kw = {} if cli == "native" else dict(cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT))
    outs = {}
    for where in ("host", "device"):
        out = tmp_path / f"{where}.gfa"
        r = _cli(head + ["-s", str(fa), "-o", str(out), "--no-sort", "--compact-on", where, "-v"], **kw)
        assert r.returncode == 0, r.stderr
        assert ("Compaction on device: rounds=" in r.stdout) == (where == "device")
        outs[where] = out.read_text()
    assert outs["device"] == outs["host"]
    r = _cli(head + ["-s", str(fa), "-o", str(tmp_path / "x.gfa"), "--no-sort", "--no-compact", "--compact-on", "device"], **kw)
    assert r.returncode == 1 and REFUSAL in r.stderr
    assert not (tmp_path / "x.gfa").exists()
