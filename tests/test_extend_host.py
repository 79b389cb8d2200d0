"""Host tests of --extend, no GPU: the restatement of the rule in Python (extend_inputs.restate)
against the host twin (a plan with device -1, sr_extend_seed_host, sr_uf_canonical_labels_host) on the seam graphs; the
bijection between a graph and the partition that produced it, on the CPU oracle alone: seeding from the oracle's graph of the
first m sequences gives the labels the oracle has over all n after aligning only the old pairs, and compaction or the Ygs
sort of that graph in between change nothing; the pair filter against a filter in Python; every refusal with its message,
from the ABI and from the command line."""
import functools

import numpy as np
import pytest

import extend_inputs as ei
import oracle_binding as ob
from seqrush_amd.__main__ import main
from seqrush_amd.seqrush import (ExtendPlan, HostUnionFind, Params, SeqRushError, compact_gfa, extend_seed_host, pair_list,
                                 sort_gfa)

SEAMS = ei.seam_cases()


def twin(text, new):
    """-> (records of the merged set, n_old, canonical labels, seed counts, plan stats) through the host twin"""
    with ExtendPlan(text, new, device=-1) as plan:
        uf = HostUnionFind(plan.seqset.total_length)
        st = extend_seed_host(plan, uf)
        return plan.records, plan.n_old, uf.canonical_labels(), st, plan.stats()


@pytest.mark.parametrize("name", sorted(SEAMS))
def test_twin_equals_the_restatement_on_the_seams(name):
    text, new = SEAMS[name]
    want = ei.restate(text, new)
    records, n_old, labels, st, ps = twin(text, new)
    assert records == want["records"] and n_old == want["n_old"]
    assert st["unions_attempted"] == len(want["unions"])
    assert np.array_equal(labels, want["labels"]), name
    total = sum(len(s) for _, s in records)
    assert st["unions_joined"] == total - len(np.unique(want["labels"][:2 * total]))      # every join removes one set
    assert (ps["old_paths"], ps["old_bases"], ps["old_steps"], ps["new_sequences"]) == (n_old, want["old_bases"], want["steps"], len(new))


def test_each_seam_recipe_has_its_property():
    def g(name):
        return ei.parse(SEAMS[name][0])
    nodes, paths = g("path_of_one_step")
    assert [len(s) for _, s in paths].count(1) == 2
    nodes, paths = g("node_lengths")
    assert sorted(len(s) for s in nodes.values()) == [1, 63, 64, 65, 255, 256, 257, 1025]
    assert {r for _, s in paths for _, r in s} == {False, True}
    for total in (1023, 1024, 1025):
        nodes, paths = g(f"steps_{total}")
        assert sum(len(s) for _, s in paths) == total and 1 in [len(s) for _, s in paths]
    for total in (65535, 65536, 65537):
        assert ei.restate(*SEAMS[f"flat_{total}"])["old_bases"] == total
        assert ei.restate(*SEAMS[f"flat_{total}"])["steps"] > ei.BLOCK * ei.BLOCK - 2      # the scan's third level at 65 537
    nodes, paths = g("first_visit_reversed")
    flat = [st for _, s in paths for st in s]
    assert next(r for i, r in flat if i == 2) is True and (2, False) in flat
    nodes, paths = g("hairpin")
    d = dict(paths)
    assert d["twice"].count((1, False)) == 2 and (2, False) in d["hairpin"] and (2, True) in d["hairpin"]
    nodes, paths = g("unvisited_node")
    assert 7 in nodes and 7 not in {i for _, s in paths for i, _ in s}
    nodes, paths = g("iupac_bytes")
    seq = b"".join(nodes.values())
    assert b"N" in seq and any(c in seq for c in b"acgt") and any(c in seq for c in b"RYKMSWBDHV")
    assert ei.revcomp(b"acgN") == b"NCGT"                             # lower case comes back upper case, N is its own complement
    nodes, paths = g("star_130_paths")
    assert len(paths) == 130 and len(nodes) == 1 and {r for _, s in paths for _, r in s} == {False, True}


# ------------------------------------------------------------------ the bijection, on the oracle alone
def oparams(k):
    p = ob.default_params()
    p.min_match_len = k
    p.threads = 4
    return p


@functools.lru_cache(maxsize=None)
def oracle_graph(family, k, m):
    """the oracle's --no-sort --no-compact GFA of the first m sequences"""
    recs = ei.FAMILIES[family]()
    o = ob.OracleSeqRush(records=recs[:m])
    o.align_and_unite(oparams(k))
    text = o.gfa(canonical=True)[0]
    o.close()
    return text


@functools.lru_cache(maxsize=None)
def oracle_old_only(family, k, m):
    """the oracle's labels over all n after aligning only the ordered pairs of the first m"""
    recs = ei.FAMILIES[family]()
    o = ob.OracleSeqRush(records=recs)
    o.align_and_unite_list(oparams(k), [(q, t) for q in range(m) for t in range(m)])
    lab = o.canonical_labels()
    o.close()
    lab.setflags(write=False)
    return lab


CASES = [(f, k, m) for f in sorted(ei.FAMILIES) for k in (0, 8) for m in ei.splits(len(ei.FAMILIES[f]()))]


@pytest.mark.parametrize("family,k,m", CASES, ids=[f"{f}-k{k}-m{m}" for f, k, m in CASES])
def test_seeding_from_the_oracle_graph_restores_its_partition(family, k, m):
    recs = ei.FAMILIES[family]()
    text = oracle_graph(family, k, m)
    want = oracle_old_only(family, k, m)
    records, n_old, labels, _, _ = twin(text, recs[m:])
    assert records == [(n, bytes(s)) for n, s in recs] and n_old == m        # the paths spell their sequences
    assert np.array_equal(labels, want)
    assert np.array_equal(ei.restate(text, recs[m:])["labels"], want)
    # grooming flips nodes and compaction merges them: the partition of the bases stays
    for groomed in (compact_gfa(text, -1), sort_gfa(text, device=-1), sort_gfa(compact_gfa(text, -1), device=-1)):
        records, _, labels, _, _ = twin(groomed, recs[m:])
        assert records == [(n, bytes(s)) for n, s in recs]
        assert np.array_equal(labels, want)


# ------------------------------------------------------------------ the pair filter
@pytest.mark.parametrize("spec", ["none", "random:0.5", "tree:2,1,0.5"])
@pytest.mark.parametrize("exclude_self", [False, True])
def test_pair_filter_equals_the_python_filter(spec, exclude_self):
    recs = ei.snp12()
    n = len(recs)
    if spec.startswith("tree"):                                     # a given selection: the oracle's list
        o = ob.OracleSeqRush(records=recs)
        pairs = o.sparsified_pairs(spec, seed=42, exclude_self=exclude_self)
        o.close()
    else:
        pairs = pair_list(n, Params(sparsification=spec, exclude_self=int(exclude_self)))
    assert len(pairs) > n
    for m in ei.splits(n):
        with ExtendPlan(oracle_graph("snp12", 0, m), recs[m:], device=-1) as plan:
            got = plan.pair_list(pairs)
            assert got == ei.py_filter(pairs, m) and 0 < len(got) <= len(pairs)
            assert len(got) < len(pairs) or (m == 1 and exclude_self)
            assert plan.pair_list([]) == []
            with pytest.raises(SeqRushError, match="out of range"):
                plan.pair_list([(0, n)])


# ------------------------------------------------------------------ refusals
REFUSALS = ei.refusal_cases()


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_of_the_plan(name, tmp_path, capsys):
    text, new, words = REFUSALS[name]
    with pytest.raises(SeqRushError) as e:
        ExtendPlan(text, new, device=-1)
    assert e.value.code == -1
    for w in words:
        assert w in str(e.value), (w, str(e.value))
    g, fa = tmp_path / "in.gfa", tmp_path / "new.fa"
    g.write_text(text)
    fa.write_bytes(b"".join(b">" + n.encode() + b"\n" + s + b"\n" for n, s in new))
    assert main(["-s", str(fa), "--extend", str(g), "-o", str(tmp_path / "out.gfa"), "--no-sort"]) == 1
    err = capsys.readouterr().err
    for w in words:
        assert w in err, (w, err)
    assert not (tmp_path / "out.gfa").exists()


def test_an_unvisited_node_without_a_sequence_is_ignored():
    text = ei.gfa({1: b"ACGT", 2: b"*"}, [("a", [(1, False)]), ("b", [(1, True)])])
    records, n_old, labels, st, _ = twin(text, ei.NEW)
    assert records[:2] == [("a", b"ACGT"), ("b", b"ACGT")] and st["unions_attempted"] == 4
    assert np.array_equal(labels, ei.restate(text, ei.NEW)["labels"])


@pytest.mark.parametrize("flags,what", [(["--iterative"], "--iterative"), (["-p", "x.paf"], "-p"),
                                        (["--patch-inversions", "-k", "8"], "--patch-inversions"), (["--gpus", "2"], "--gpus N > 1")])
def test_refused_combinations(flags, what, tmp_path, capsys):
    g, fa = tmp_path / "in.gfa", tmp_path / "new.fa"
    g.write_text(SEAMS["hairpin"][0])
    fa.write_bytes(b">new1\nACGT\n")
    assert main(["-s", str(fa), "--extend", str(g), "-o", str(tmp_path / "out.gfa"), "--no-sort"] + flags) == 1
    assert f"Error: --extend cannot be combined with {what}" in capsys.readouterr().err
    assert not (tmp_path / "out.gfa").exists()


def test_seed_host_refuses_a_short_node_array():
    text, new = SEAMS["hairpin"]
    with ExtendPlan(text, new, device=-1) as plan:
        uf = HostUnionFind(plan.seqset.total_length - 1)
        with pytest.raises(SeqRushError, match="shorter"):
            extend_seed_host(plan, uf)
