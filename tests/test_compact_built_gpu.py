"""GPU parity tests (-m gpu) of compaction by tables on the device (sr_compact.hip) on the built link lists of
tests/compact_built_inputs.py: byte for byte against the host procedure, against the oracle's restatement of compact() +
renumbering, run to run, with the round's statistics of the table functors on the host (test_compact_built_host.py pins the
three references against each other).  The cases put a scan tile edge at NH = 2 NN (1 024 / 1 026 / 1 028 handles), take
gi_scan_sums through its second pass (NH = 262 202 > 256 tiles), rank lists of 2^k - 1 / 2^k / 2^k + 1 members with up to
18 jumps in a round, run ct_kernel's grid-stride loop (2.12 M steps > 8 192 x 256 threads), go through 3 to 7 rounds on
multi-base nodes with dead slots and mixed-case text, refuse chains inside long lists and fall back to the host procedure
for a round in the middle of a run.  The same lists enter through Context.build_gfa(compact_on="device"), which adopts the
arrays induction left on the device, at 600 and 140 000 bases.

The oracle is quadratic in list length: it is not run on the chains of 131 100 nodes, on the 2.12 M-step case or on the
140 000-base partition, where the host procedure is the reference (pinned to the oracle by the same builders at the small
sizes).  The grid-stride loop of the per-handle functors (NH > 2 097 152) is not run: it is the same ct_kernel<F> template.
One sr_compact_gfa call or one context at a time; nothing is retried."""
import pytest

import compact_built_inputs as cb
import compact_inputs as ci
import oracle_binding as ob
from seqrush_amd.seqrush import compact_gfa, compact_stats
from test_compact_built_host import (ADOPT, HOST, SMALL, adopt_case, jump_bound, log2_ceil, oracle, permuted_seed, reference)
from test_partitions_gpu import merge, open_context

pytestmark = pytest.mark.gpu

SAME = ("rounds", "chains", "longest_list", "host_rounds")


@pytest.mark.parametrize("name", cb.NAMES)
def test_device_matches_host_and_oracle(gpu, name):
    text = cb.case(name)
    want, _, tab = reference(name)
    st = {}
    got = compact_gfa(text, 0, st)
    print(f"\n{name}: nodes {cb.nodes(name)} rounds {st['rounds']} host_rounds {st['host_rounds']} chains {st['chains']} "
          f"longest {st['longest_list']} jumps {st['jumps']} device_us {st['compact_us']} copy_us {st['copy_us']}")
    assert got == want
    if cb.with_oracle(name):
        assert got == oracle(name)
    assert compact_gfa(text, 0) == got                           # run to run
    assert [st[k] for k in SAME] == [tab[k] for k in SAME]
    assert st["jumps"] <= jump_bound(name, st) and st["compact_us"] > 0


@pytest.mark.parametrize("name", SMALL)
def test_device_matches_host_and_oracle_with_permuted_ids(gpu, name):
    text = ci.permuted(cb.case(name), permuted_seed(name))
    tab, st = {}, {}
    want = compact_gfa(text, HOST)
    assert compact_gfa(text, -2, tab) == want
    got = compact_gfa(text, 0, st)
    assert got == want and got == ob.compact_gfa(text)[0]
    assert compact_gfa(text, 0) == got
    assert [st[k] for k in SAME] == [tab[k] for k in SAME]
    assert st["jumps"] <= jump_bound(name, st)


@pytest.mark.parametrize("name", sorted(ADOPT))
def test_context_adopts_built_partitions(gpu, name):
    """Context.build_gfa(compact_on="device") on one list across the whole sequence: single-base nodes, a dead slot 0, no
    upload; 2 (L + 2) handles, 280 004 at 140 000 bases"""
    c = adopt_case(name)
    L = c["L"]
    ss, ctx = open_context(c["recs"])
    try:
        merge(ctx, c["arrays"], 64)
        plain = ctx.build_gfa(compact=False)
        host = ctx.build_gfa(compact=True, compact_on="host")
        dev = ctx.build_gfa(compact=True, compact_on="device")
        st = compact_stats()
        again = ctx.build_gfa(compact=True, compact_on="device")
    finally:
        ctx.close()
    print(f"\n{name}: rounds {st['rounds']} host_rounds {st['host_rounds']} chains {st['chains']} longest {st['longest_list']} "
          f"jumps {st['jumps']} device_us {st['compact_us']}")
    assert plain[1] == L + 1
    assert dev == host and again == dev
    assert dev[0] == compact_gfa(plain[0], HOST)
    assert (st["rounds"], st["host_rounds"], st["chains"], st["longest_list"]) == (2, 0, 1, L)
    assert log2_ceil(L) <= st["jumps"] <= 2 * (log2_ceil(2 * (L + 3)) + 1)
    assert ci.parse(dev[0])[0] == {"1": b"G", "2": c["recs"][1][1]}
    if L <= cb.ORACLE_MAX_NODES:
        assert dev[0] == ob.compact_gfa(plain[0])[0]
