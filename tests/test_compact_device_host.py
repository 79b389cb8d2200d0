"""Compaction by per-handle tables (sr_compact_tab.h) run on the host in index order, sr_compact_gfa(device=-2), against
the greedy host procedure (device=-1, sr_compact.cpp) and the oracle's literal restatement of compact() + renumbering.
No GPU: the device runs the same functors (tests/test_compact_device_gpu.py)."""
import pytest

import compact_inputs as ci
import oracle_binding as ob
from seqrush_amd import _lib
from seqrush_amd.seqrush import Args, SeqRushError, compact_gfa, compact_mode
from test_host_abi import COMPACT_CASES

HOST, TABLES = -1, -2


def _oracle_gfa(recs, k):
    o = ob.OracleSeqRush(records=recs)
    p = ob.default_params(); p.min_match_len = k; p.threads = 2
    o.align_and_unite(p)
    return o.gfa(canonical=True)[0]


def _check(text, native=True):
    """-2 == -1 byte for byte, paths spell what they spelled; native: no round may fall back to the host procedure"""
    want, st = compact_gfa(text, HOST), {}
    got = compact_gfa(text, TABLES, st)
    assert got == want
    assert ci.spelled(got) == ci.spelled(text)
    if native:
        assert st["host_rounds"] == 0
    assert st["jumps"] <= st["rounds"] * 33 and st["reserved"] == 0
    return got, st


@pytest.mark.parametrize("name", sorted(COMPACT_CASES))
@pytest.mark.parametrize("k", [0, 6])
def test_tables_match_greedy_and_oracle_on_induced_graphs(name, k):
    text = _oracle_gfa(COMPACT_CASES[name](), k)
    got, st = _check(text)
    assert got == ob.compact_gfa(text)[0]
    host = {}
    compact_gfa(text, HOST, host)
    assert (st["rounds"], st["chains"]) == (host["rounds"], host["chains"])
    _check(ci.permuted(text, 7 + k))


@pytest.mark.parametrize("block", range(10))
def test_tables_match_greedy_on_random_families(block):
    """220 seeded families, each as induced and with permuted node ids (the chain rule depends on id order)"""
    for seed in range(22 * block, 22 * block + 22):
        text = _oracle_gfa(ci.random_family(1000 + seed), (0, 6, 3)[seed % 3])
        _check(text)
        _check(ci.permuted(text, seed))


@pytest.mark.parametrize("name", sorted(ci.HAND))
def test_hand_written(name):
    text, may_fall_back = ci.HAND[name]
    got, st = _check(text, native=not may_fall_back)
    assert got == ob.compact_gfa(text)[0] or name == "empty"
    if name == "middle-min":
        assert st["rounds"] == 3 and st["chains"] == 2           # [1+, 3+], then 2+ joins, then nothing
        assert "\nS\t1\tTACGGGA\n" in got
    if name == "min-last":                                       # the mirror list wins: one node, reverse complemented
        assert st["chains"] == 1 and "\nP\tp\t1-\t*\n" in got
    if name in ("starts-inside", "ends-inside-rc", "step-without-edge"):
        assert st["chains"] == 0 and len(ci.parse(got)[0]) == len(ci.parse(text)[0])
    if name.startswith("cycle"):
        assert st["host_rounds"] >= 1


def test_stats_and_errors():
    st = {}
    compact_gfa(ci.HAND["zigzag"][0], TABLES, st)
    assert st["longest_list"] == 5 and st["chains"] == 3 and st["copy_us"] == 0
    with pytest.raises(SeqRushError):
        compact_gfa("S\tx\tACGT\n", TABLES)
    with pytest.raises(SeqRushError):
        compact_gfa(ci.HAND["zigzag"][0], -3)
    assert _lib.load().sr_abi_version() == 2


def test_python_surface():
    assert Args().compact_on == "host"
    assert [compact_mode(c, o) for c, o in ((False, "host"), (True, "host"), (True, "device"))] == [0, 1, 2]
    with pytest.raises(SeqRushError, match="exclude each other"):
        compact_mode(False, "device")
    with pytest.raises(SeqRushError):
        compact_mode(True, "gpu")


@pytest.mark.parametrize("cli", ["native", "python"])
def test_cli_refuses_device_compaction_without_compaction(tmp_path, cli):
    """before any device use, like --sort --no-sort"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    head = [os.path.join(root, "seqrush_amd", "seqrush_mi355x")] if cli == "native" else [sys.executable, "-m", "seqrush_amd"]
    fa = tmp_path / "in.fa"
    fa.write_text(">a\nACGT\n>b\nACGT\n")
    r = subprocess.run(head + ["-s", str(fa), "-o", str(tmp_path / "o.gfa"), "--no-sort", "--no-compact", "--compact-on", "device"],
                       capture_output=True, text=True, timeout=120, cwd=root, env=dict(os.environ, PYTHONPATH=root))
    assert r.returncode == 1 and "Error: --compact-on device and --no-compact exclude each other" in r.stderr
    assert not (tmp_path / "o.gfa").exists()
