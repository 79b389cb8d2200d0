"""CPU tests (-m "not gpu") on partitions and CIGARs built by hand (tests/partition_inputs.py): the references of the device
suite (test_partitions_gpu.py) are pinned against each other first.  On every family x size up to 262 145 bases the
product's host twins (HostUnionFind.merge_labels + canonical_labels, build_gfa on labels, sr_uf_count_components_host) equal
the oracle fed with the same unions (sro_buf_unite, canonical labels, its own induction, compared through canon_gfa) and a
plain numpy union-find written here that owes nothing to either; at the two grid-cap sizes the host twin is compared with the
plain union-find only.  The oracle's induction is linear, so it runs at 262 145 too (a second or so per case).  Every CIGAR
recipe has the property it is named for, and the oracle's PAF replay equals the plain union-find fed from a walk of the CIGAR
over the bytes in Python.  Every assertion is exact."""
import functools

import numpy as np
import pytest

import oracle_binding as ob
import partition_inputs as pi
from seqrush_amd.seqrush import HostUnionFind, SeqRushError, SeqSet, build_gfa, uf_count_components_host
from conftest import canon_gfa


# ------------------------------------------------------------------------------------------ the plain references
def plain_labels(N, unions):
    """canonical labels (smallest Pos of the component) of 2N+2 elements: strands of every base united, then `unions`.
    Hooking of the larger root under the smaller and pointer jumping until no union is left open -- whole-array numpy, no
    ranks, no path halving, no CAS: nothing in common with uf_rush"""
    n = 2 * N + 2
    par = np.arange(n, dtype=np.int64)
    par[1:2 * N:2] -= 1
    a = np.asarray(unions, dtype=np.uint64).astype(np.int64).reshape(-1, 2)
    a, b = a[:, 0], a[:, 1]
    while True:
        while True:                                   # jump to the roots
            nxt = par[par]
            if np.array_equal(nxt, par):
                break
            par = nxt
        ra, rb = par[a], par[b]
        open_ = ra != rb
        if not open_.any():
            return par.astype(np.uint64)
        a, b, ra, rb = a[open_], b[open_], ra[open_], rb[open_]
        par[np.maximum(ra, rb)] = np.minimum(ra, rb)  # one of several writers wins; the others stay open for the next round


def sanitized(arrays, n):
    """label arrays with the entries a merge must ignore (>= n) made identity"""
    idx = np.arange(n, dtype=np.uint64)
    return [np.where(a >= np.uint64(n), idx, a) for a in arrays]


@functools.lru_cache(maxsize=8)
def reference(family, N):
    """-> (plain canonical labels, component count among the 2N base Pos); kept for the device suite"""
    c = pi.partition(family, N)
    lab = plain_labels(N, c["unions"])
    lab.setflags(write=False)
    return lab, int(len(np.unique(lab[:2 * N])))


def walk(recs, record):
    """one PAF record over the bytes -> (maximal match runs [(query pos, target pos, length)], operations as the device
    sees them [(kind, length)] with kind '=' for equal bytes under M / =, 'X' for unequal ones and X, 'I', 'D').  Query
    positions of a '-' record are positions in the reverse complement (src/seqrush.rs:1162-1176, 1210)"""
    qi, ti, strand, qs, ts, ops = record
    q, t = recs[qi][1], recs[ti][1]
    if strand == "-":
        q = pi.revcomp(q)
    cols, p1, p2 = [], qs, ts
    for op, n in ops:
        if op in "M=":
            cols += ["=" if q[p1 + j] == t[p2 + j] else "X" for j in range(n)]
            p1 += n; p2 += n
        else:
            cols += [op] * n
            p1 += n if op in "XI" else 0
            p2 += n if op in "XD" else 0
    runs, dev, p1, p2, i = [], [], qs, ts, 0
    while i < len(cols):
        j = i
        while j < len(cols) and cols[j] == cols[i]:
            j += 1
        kind, n = cols[i], j - i
        dev.append((kind, n))
        if kind == "=":
            runs.append((p1, p2, n))
        p1 += n if kind in "=XI" else 0
        p2 += n if kind in "=XD" else 0
        i = j
    return runs, dev


@functools.lru_cache(maxsize=None)
def walks(name):
    c = pi.cigar_case(name)
    return [walk(c["recs"], rec) for rec in c["records"]]


def cigar_unions(name, k):
    """-> (unions of every match run of at least k bases, bases in them, number of them)"""
    c = pi.cigar_case(name)
    recs = c["recs"]
    off = np.concatenate([[0], np.cumsum([len(s) for _, s in recs])]).astype(np.int64)
    out, bases, nruns = [np.zeros((0, 2), dtype=np.uint64)], 0, 0
    for rec, (runs, _) in zip(c["records"], walks(name)):
        qi, ti, strand = rec[:3]
        qlen = len(recs[qi][1])
        for p1, p2, n in runs:
            if n < k:
                continue
            j = np.arange(n, dtype=np.int64)
            if strand == "-":
                a = ((off[qi] + qlen - 1 - (p1 + j)) << 1) | 1
            else:
                a = (off[qi] + p1 + j) << 1
            out.append(np.stack([a, (off[ti] + p2 + j) << 1], axis=1).astype(np.uint64))
            bases += n; nruns += 1
    return np.concatenate(out), bases, nruns


@functools.lru_cache(maxsize=None)
def cigar_reference(name, k):
    """-> (plain canonical labels, united bases, match runs) of a recipe under -k; kept for the device suite"""
    c = pi.cigar_case(name)
    un, bases, nruns = cigar_unions(name, k)
    lab = plain_labels(sum(len(s) for _, s in c["recs"]), un)
    lab.setflags(write=False)
    return lab, bases, nruns


# ------------------------------------------------------------------------------------------ 1. partitions
@pytest.mark.parametrize("family,N", pi.HOST_MATRIX, ids=[f"{f}-{n}" for f, n in pi.HOST_MATRIX])
def test_host_twins_oracle_and_plain_union_find_agree(family, N):
    c = pi.partition(family, N)
    recs, n = c["recs"], 2 * N + 2
    assert sum(len(s) for _, s in recs) == N and len(recs) >= 2 and min(len(s) for _, s in recs) == 1
    assert all(len(a) == n and a.dtype == np.uint64 for a in c["arrays"])
    want, ncomp = reference(family, N)
    # host twin
    h = HostUnionFind(N)
    if family == "skip":                              # the host twin refuses what the device kernels skip: entries >= n
        assert any((a >= np.uint64(n)).any() for a in c["arrays"])
        with pytest.raises(SeqRushError):
            HostUnionFind(N).merge_labels(c["arrays"])
    h.merge_labels(sanitized(c["arrays"], n))
    labels = h.canonical_labels()
    assert np.array_equal(labels, want)
    assert uf_count_components_host(h.nodes, N) == ncomp
    # oracle
    o = pi.oracle_unite(recs, c["unions"])
    assert np.array_equal(o.canonical_labels(), want)
    assert o.count_components() == ncomp
    ss = SeqSet(recs)
    text, nn, ne = build_gfa(ss, labels)
    otext, onn, one = o.gfa(canonical=True)
    o.close()
    assert (nn, ne) == (onn, one) and nn == ncomp
    assert canon_gfa(text) == canon_gfa(otext)
    if family == "none":
        assert (nn, ne) == (N, N - len(recs))
    if family == "letters":
        assert nn == len(set(bytes(c["bases"]).upper()))
    if N <= 1025:
        ctext, cn, ce = build_gfa(ss, labels, compact=True)
        otc = ob.compact_gfa(text)
        assert canon_gfa(ctext) == canon_gfa(otc[0]) and (cn, ce) == otc[1:]


@pytest.mark.parametrize("family,N", [(f, n) for f, n in pi.MATRIX if n > pi.SCAN_SIZES[-1]])
def test_host_twin_equals_plain_union_find_at_the_grid_caps(family, N):
    c = pi.partition(family, N)
    want, ncomp = reference(family, N)
    h = HostUnionFind(N)
    h.merge_labels(c["arrays"])
    assert np.array_equal(h.canonical_labels(), want)
    assert uf_count_components_host(h.nodes, N) == ncomp


@pytest.mark.parametrize("N", [1023, 1024, 1025])
def test_families_have_the_property_they_are_named_for(N):
    def gfa_of(family):
        c = pi.partition(family, N)
        return c, build_gfa(SeqSet(c["recs"]), reference(family, N)[0])
    c, (text, nn, ne) = gfa_of("palindrome")
    assert pi.self_reverse_edges(text) >= 1           # k1 == k2
    paths = [ln.split("\t")[2].split(",") for ln in text.split("\n") if ln.startswith("P")]
    fwd = {(a, b) for p in paths for a, b in zip(p, p[1:])}
    flip = lambda s: s[:-1] + ("-" if s[-1] == "+" else "+")      # noqa: E731
    assert any((flip(b), flip(a)) in fwd for a, b in fwd if a[:-1] != b[:-1])    # an edge met in both orientations
    c, (text, nn, ne) = gfa_of("letters")
    assert nn <= 5 and sum(1 for ln in text.split("\n") if ln.startswith("L") and ln.split("\t")[1] == ln.split("\t")[3]) >= 1
    c, (text, nn, ne) = gfa_of("star")
    assert nn == 1
    c, (text, nn, ne) = gfa_of("mixed_alphabet")
    # a node and a member that are complementary only when case is ignored: the step is reversed by the upper-casing alone
    lab, bases = reference("mixed_alphabet", N)[0], bytes(c["bases"])
    comp = {"A": "T", "T": "A", "C": "G", "G": "C"}
    mixed = sum(1 for g in range(N) if comp.get(chr(bases[int(lab[2 * g]) >> 1]).upper()) == chr(bases[g]).upper()
                and (chr(bases[g]).islower() or chr(bases[int(lab[2 * g]) >> 1]).islower()))
    assert mixed >= 1 and any(ch in bases for ch in b"NRYn")
    c = pi.partition("two_arrays", N)
    want = reference("two_arrays", N)[0]
    assert len(set(want[:2 * N].tolist())) == 1       # one component, but only from both arrays together
    for a in c["arrays"]:
        h = HostUnionFind(N); h.merge_labels([a])
        assert uf_count_components_host(h.nodes, N) > N // 3
    for family in ("chain", "letters", "random", "palindrome"):       # not canonical: some label is not its component's minimum
        c = pi.partition(family, N)
        assert any((a != reference(family, N)[0]).any() for a in c["arrays"])


# ------------------------------------------------------------------------------------------ 2. CIGAR recipes
@pytest.mark.parametrize("name", pi.CIGAR_NAMES)
def test_cigar_recipe_is_what_it_is_named_for(name):
    c = pi.cigar_case(name)
    recs = c["recs"]
    assert len(recs[0][1]) == 1
    assert len(c["records"]) == (1 if c.get("self_record") else 4)
    for rec, (runs, dev) in zip(c["records"], walks(name)):
        qi, ti, strand, qs, ts, ops = rec
        assert qs + sum(n for k, n in dev if k in "=XI") <= len(recs[qi][1])
        assert ts + sum(n for k, n in dev if k in "=XD") <= len(recs[ti][1])
        if "count" in c:                              # the device sees exactly the operations of the text
            assert dev == [("=" if k == "M" else k, n) for k, n in ops] and len(dev) == c["count"]
        if "empty_chunk" in c:
            ch = c["empty_chunk"]
            assert all(k != "=" for k, _ in dev[256 * ch:256 * ch + 256])
            assert any(k == "=" for k, _ in dev[:256 * ch]) and any(k == "=" for k, _ in dev[256 * ch + 256:])
        for at, n in c.get("runs_at", {}).items():
            assert dev[at] == ("=", n)
        if name == "long70000":
            assert runs == [(qs, ts, 70000)]
        if name in ("m_only", "claim"):               # the text's M / = hold unequal bytes: the device sees more operations
            assert len(dev) > 3 * len(ops) and any(k == "X" for k, _ in dev)
            assert {n for k, n in dev if k == "="} & set(range(1, 8))
        if c.get("self_record"):
            assert qi == ti and qs == ts and strand == "+"
    if name.startswith("runs"):
        k = int(name[4:name.index("at")])
        assert sorted(c["runs_at"].values()) == [r for r in (k - 1, k, k + 1) if r]
        assert sorted(c["runs_at"]) == [int(name[name.index("at") + 2:]) + 2 * j for j in range(len(c["runs_at"]))]
    strands = [(r[2], r[3] > 0, r[4] > 0) for r in c["records"]]
    assert c.get("self_record") or strands == [("+", False, False), ("-", False, False), ("+", True, True), ("-", True, True)]


@pytest.mark.parametrize("k", pi.CIGAR_K)
@pytest.mark.parametrize("name", pi.CIGAR_NAMES)
def test_oracle_paf_replay_equals_python_walk(name, k):
    c = pi.cigar_case(name)
    want, bases, nruns = cigar_reference(name, k)
    o = pi.oracle_paf_replay(c["recs"], c["paf"], k, labels=False)
    assert np.array_equal(o.canonical_labels(), want)
    o.close()
    # the oracle's own count of united bases, record by record
    o = ob.OracleSeqRush(records=c["recs"])
    got = 0
    for qi, ti, strand, qs, ts, ops in c["records"]:
        got += o.process_alignment("".join(f"{n}{op}" for op, n in ops), qi, ti, k, strand == "-", qs, None, ts, None)
    o.close()
    assert got == bases
    if name.startswith("runs") and k in (8, 15) and f"runs{k}at" in name:
        assert nruns == 2 * 4 and bases == (2 * k + 1) * 4           # the runs of k and k+1, not the one of k-1
