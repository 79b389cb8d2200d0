"""Compaction on built link lists, on the host (no GPU): the greedy host procedure (sr_compact_gfa device = -1), the table
functors in index order (-2) and the oracle's literal restatement of compact() + renumbering on the cases of
tests/compact_built_inputs.py, plus what follows from each construction whatever the code does.  The device runs the same
cases against the references pinned here (tests/test_compact_built_gpu.py).

The oracle is quadratic in list length: it runs on every case of at most cb.ORACLE_MAX_NODES nodes and not on the two large
families (chains of 131 100 nodes, 2.1 M steps over 40 018 nodes), where the host procedure is the reference; the same
builders pin it to the oracle at the small sizes."""
import functools
import math

import numpy as np
import pytest

import compact_built_inputs as cb
import compact_inputs as ci
import oracle_binding as ob
import partition_inputs as pi
from seqrush_amd.seqrush import HostUnionFind, SeqSet, build_gfa, compact_gfa

HOST, TABLES = -1, -2
SMALL = tuple(n for n in cb.NAMES if cb.nodes(n) <= cb.PERMUTE_MAX_NODES)


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (text of the host procedure, its stats, the stats of the tables on the host), after -1 == -2 byte for byte"""
    text, host, tab = cb.case(name), {}, {}
    want = compact_gfa(text, HOST, host)
    assert compact_gfa(text, TABLES, tab) == want
    return want, host, tab


@functools.lru_cache(maxsize=None)
def oracle(name):
    return ob.compact_gfa(cb.case(name))[0]


def permuted_seed(name):
    return 1 + cb.NAMES.index(name)


def log2_ceil(n):
    return max(0, math.ceil(math.log2(n)))


def jump_bound(name, st):
    """rounds x (ceil(log2 NH) + 1) with the handles of the last round: slot 0, the nodes, one new node per chain"""
    return st["rounds"] * (log2_ceil(2 * (cb.nodes(name) + 1 + st["chains"])) + 1)


@pytest.mark.parametrize("name", cb.NAMES)
def test_three_executions_agree(name):
    text = cb.case(name)
    want, host, tab = reference(name)
    if cb.with_oracle(name):
        assert want == oracle(name)
    assert ci.spelled(want) == ci.spelled(text)
    assert (tab["rounds"], tab["chains"]) == (host["rounds"], host["chains"])
    assert (tab["host_rounds"] >= 1) == name.startswith("cycle") and tab["reserved"] == 0
    assert tab["jumps"] <= jump_bound(name, tab)


@pytest.mark.parametrize("name", SMALL)
def test_three_executions_agree_with_permuted_ids(name):
    text = ci.permuted(cb.case(name), permuted_seed(name))
    want, st = compact_gfa(text, HOST), {}
    assert compact_gfa(text, TABLES, st) == want and want == ob.compact_gfa(text)[0]
    assert ci.spelled(want) == ci.spelled(text)
    assert st["host_rounds"] == 0 or name.startswith("cycle")


@pytest.mark.parametrize("name", [n for n in cb.NAMES if n.startswith("chain-")])
def test_single_chain(name):
    """one list of n members: it ends as one node of the summed length, forward when the ids ascend, reverse-complemented
    (the mirror list wins) when they descend; ranking it takes at least ceil(log2 n) jumps"""
    n, order = cb.nodes(name), name.rsplit("-", 1)[1]
    text = cb.case(name)
    got, _, st = reference(name)
    seg, _, paths = ci.parse(text)
    whole = b"".join(seg[s[:-1]] for s in paths[0][1])
    out, _, opaths = ci.parse(got)
    assert list(out) == ["1"] and len(out["1"]) == len(whole)
    assert st["longest_list"] == n and st["host_rounds"] == 0
    assert st["jumps"] >= log2_ceil(n)
    if order == "asc":
        assert (out["1"], opaths) == (whole, [("p", ["1+"])]) and (st["rounds"], st["chains"]) == (2, 1)
    if order == "desc":
        assert (out["1"], opaths) == (whole.translate(ci.RC)[::-1], [("p", ["1-"])]) and (st["rounds"], st["chains"]) == (2, 1)
    if order == "perm" and 511 <= n <= 2000:
        assert st["rounds"] >= 3                                 # the condition on the seeds (cb.PERM_SEED)


def test_structure_of_the_other_families():
    for order in ("perm", "asc"):
        got, _, st = reference(f"subwalks-600-{order}")          # refused and broken inside the list, but not everywhere
        assert st["chains"] > 0 and st["host_rounds"] == 0 and 1 < len(ci.parse(got)[0]) < 600
        assert [n for n, _ in ci.spelled(got)] == ["p"] + [w[0] for w in cb.SUBWALKS]
        got, _, st = reference(f"hops-600-{order}")              # a member entered from elsewhere: the same, with two paths
        assert st["chains"] > 0 and st["host_rounds"] == 0 and 1 < len(ci.parse(got)[0]) < 600
        got, _, st = reference(f"bubbles-seams-{order}")         # every run one node, every allele kept
        assert st["longest_list"] == max(cb.SEAM_RUNS) and st["host_rounds"] == 0
        assert len(ci.parse(got)[0]) == len(cb.SEAM_RUNS) + 2 * (len(cb.SEAM_RUNS) - 1)
    got, _, st = reference("cycle-300-chain-700")
    assert st["host_rounds"] >= 1 and st["rounds"] > st["host_rounds"] and st["longest_list"] == 700
    got, _, st = reference("hairpin-400")
    assert st["host_rounds"] == 0 and st["longest_list"] == 400 and ci.parse(got)[2] == [("p", ["1+", "1-"])]
    got, _, st = reference("two-way-links-300")
    # links break at every third L line only: node 1 alone, then lists of 3 (the last of 2); a repeated line breaks nothing
    assert st["longest_list"] == 3 and st["host_rounds"] == 0 and len(ci.parse(got)[0]) == 1 + math.ceil(299 / 3)
    got, _, st = reference("bubbles-stride-perm")
    assert st["longest_list"] == 4000 and len(ci.parse(got)[0]) == 10 + 18
    assert sum(len(st_) for _, st_ in ci.parse(cb.case("bubbles-stride-perm"))[2]) > 8192 * 256


# ------------------------------------------------------------------------------------------ what Context.build_gfa adopts
ADOPT = {"identical-600": (600, False), "identical-140000": (140000, False), "rc-member-600": (600, True)}


@functools.lru_cache(maxsize=None)
def adopt_case(name):
    """a single base, then two members of L bases united position by position (the second reverse-complemented and united
    on the other strand for rc-member): single-base nodes in one list across the whole sequence, 2 (L + 2) handles"""
    L, rc = ADOPT[name]
    seq = pi._draw(np.random.default_rng([41, L]), pi.ACGT, L).tobytes()
    recs = [("one", b"G"), ("m0", seq), ("m1", pi.revcomp(seq) if rc else seq)]
    i = np.arange(L, dtype=pi.U64)
    one = pi.U64(1)
    a = ((pi.U64(L) - i) << one) | one if rc else (i + one) << one
    b = (i + pi.U64(L + 1)) << one
    lab = pi._ident(2 * L + 1)
    lab[b] = a
    lab.setflags(write=False)
    return dict(L=L, recs=recs, arrays=[lab], unions=pi._pairs(b, a))


@pytest.mark.parametrize("name", sorted(ADOPT))
def test_adopted_partitions_on_the_host(name):
    """host induction + compaction of the partitions the device test adopts: one list of L single-base nodes"""
    c = adopt_case(name)
    L = c["L"]
    h = HostUnionFind(2 * L + 1)
    h.merge_labels(c["arrays"])
    ss = SeqSet(c["recs"])
    text, nn, _ = build_gfa(ss, h.canonical_labels())
    assert nn == L + 1
    st = {}
    got = compact_gfa(text, TABLES, st)
    assert got == compact_gfa(text, HOST) and got == build_gfa(ss, h.canonical_labels(), compact=True)[0]
    assert (st["longest_list"], st["chains"], st["host_rounds"], st["rounds"]) == (L, 1, 0, 2)
    seg, _, paths = ci.parse(got)
    assert seg == {"1": b"G", "2": c["recs"][1][1]}
    assert paths == [("one", ["1+"]), ("m0", ["2+"]), ("m1", ["2-" if ADOPT[name][1] else "2+"])]
    if L <= cb.ORACLE_MAX_NODES:
        assert got == ob.compact_gfa(text)[0]
