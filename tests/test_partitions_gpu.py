"""GPU parity tests (-m gpu) of what follows the aligner, on partitions and CIGARs built by hand (tests/partition_inputs.py):
sr_unite_kernel's CIGAR walk, the lock-free union-find under sr_merge_kernel / sr_merge32_kernel, the label kernels of both
widths and the 13 kernels of graph induction.  No test aligns anything: a context is loaded with one pair (the single-base
sequence against itself) or from a PAF file, the partition goes into the device forest through merge_labels on a torch
tensor or through unite(), and what comes back is compared bit for bit with the references that test_partitions_host.py
pinned against each other: the plain numpy union-find, the oracle's union-find fed with the same unions, the host induction
on the downloaded labels (byte for byte) and the oracle's induction (canonically).  One context at a time, closed before the
next; nothing is retried; nothing relies on a device error flag being raised (sync() raising on one fails the case).

At 524 289 and 2 097 153 bases the oracle is not run (the host file compares the host twin with the plain union-find there);
the GFA text is still compared whole, it is a memcmp of a few tens of MB."""
import numpy as np
import pytest
import torch

import oracle_binding as ob
import partition_inputs as pi
from seqrush_amd.seqrush import Context, Params, SeqSet, build_gfa
from conftest import canon_gfa
from test_partitions_host import cigar_reference, reference

pytestmark = pytest.mark.gpu

RANK_SHIFT, PARENT_MASK = np.uint64(58), np.uint64(0x03FFFFFFFFFFFFFF)
ORDERED = ("star", "chain", "two_arrays")             # also merged with the gathered arrays in the other order
MERGE_CASES = [(f, n, w, o) for f, n in pi.MATRIX for w in (64, 32) for o in (("given", "other") if f in ORDERED else ("given",))]


def open_context(recs):
    """a loaded context that costs no alignment workspace to speak of: one pair, the single-base sequence with itself"""
    ss = SeqSet(recs)
    one = [i for i, (_, s) in enumerate(recs) if len(s) == 1][0]
    ctx = Context(0)
    ctx.load_pairs(ss, Params(), [(one, one)])
    return ss, ctx


def merge(ctx, arrays, width=64):
    """the gathered arrays, back to back on the device, through the merge kernel of that width"""
    cat = np.concatenate(arrays)
    assert len(cat) == len(arrays) * ctx.uf_size
    host = cat.view(np.int64) if width == 64 else cat.astype(np.uint32).view(np.int32)
    t = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    (ctx.merge_labels if width == 64 else ctx.merge_labels_u32)(t.data_ptr(), len(arrays))
    ctx.sync()
    return t


def all_labels(ctx):
    """-> (download_labels, labels_device, labels_device_u32) as numpy arrays"""
    n = ctx.uf_size
    host = ctx.download_labels()
    t64 = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    t32 = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.labels_device(t64.data_ptr()); ctx.sync()
    ctx.labels_device_u32(t32.data_ptr()); ctx.sync()
    return host, t64.cpu().numpy().view(np.uint64), t32.cpu().numpy().view(np.uint32)


def check_forest(nodes, want):
    """a uf_rush node array whose sets are the reference's: parents inside the array, ranks a union by rank can reach, and
    every element's root in the element's component with one root per component"""
    n = len(nodes)
    par = (nodes & PARENT_MASK)
    assert int(par.max()) < n
    assert int((nodes >> RANK_SHIFT).max()) <= int(np.log2(n))
    par = par.astype(np.int64)
    for _ in range(64):
        nxt = par[par]
        if np.array_equal(nxt, par):
            break
        par = nxt
    else:
        raise AssertionError("cycle in the forest")
    assert np.array_equal(want[par], want)
    assert len(np.unique(par)) == len(np.unique(want))


# ------------------------------------------------------------------------------------------ 1. merge and labels
@pytest.mark.parametrize("family,N,width,order", MERGE_CASES, ids=[f"{f}-{n}-u{w}-{o}" for f, n, w, o in MERGE_CASES])
def test_merge_and_labels(gpu, family, N, width, order):
    """grid-stride loops of the merge kernels (8192 x 256 over count x (2N+2)) and the label kernels (4096 x 256 over 2N+2)
    past one trip, label arrays that are not canonical, entries >= n, arrays that are one component only together, thousands
    of unites onto one root"""
    c = pi.partition(family, N)
    want, _ = reference(family, N)
    arrays = list(c["arrays"])
    if order == "other":
        arrays = (arrays if len(arrays) > 1 else arrays + [np.arange(2 * N + 2, dtype=np.uint64)])[::-1]
    ss, ctx = open_context(c["recs"])
    assert ctx.uf_size == 2 * N + 2
    merge(ctx, arrays, width)
    host, d64, d32 = all_labels(ctx)
    nodes = ctx.download_uf()
    ctx.close()
    assert np.array_equal(host, want), f"{int((host != want).sum())} labels differ"
    assert np.array_equal(d64, want) and np.array_equal(d32, want.astype(np.uint32))
    assert host[-2] == 2 * N and host[-1] == 2 * N + 1
    check_forest(nodes, want)
    if N <= pi.ORACLE_GFA_MAX and width == 64 and order == "given":
        o = pi.oracle_unite(c["recs"], c["unions"])
        assert np.array_equal(host, o.canonical_labels())
        o.close()


# ------------------------------------------------------------------------------------------ 2. induction
@pytest.mark.parametrize("family,N", pi.MATRIX, ids=[f"{f}-{n}" for f, n in pi.MATRIX])
def test_induction(gpu, family, N):
    """the scan of 1024-base tiles at 1023 / 1024 / 1025, its second level at 262 144 / 262 145, gi_grid's stride loop at
    2 097 153; an edge table hit by thousands of positions per slot (letters) or holding N - n distinct keys (none); edges
    that are their own reverse complement or met in both orientations (palindrome); node bases taken at the label and steps
    reversed on letters no aligner would unite (star, mixed_alphabet)"""
    c = pi.partition(family, N)
    want, ncomp = reference(family, N)
    ss, ctx = open_context(c["recs"])
    merge(ctx, c["arrays"], 64)
    dev = ctx.build_gfa()
    devc = ctx.build_gfa(compact=True) if N <= 1025 else None
    labels = ctx.download_labels()
    ctx.close()
    assert np.array_equal(labels, want)
    host = build_gfa(ss, labels)
    assert dev[1:] == host[1:] and dev[1] == ncomp, (dev[1:], host[1:], ncomp)
    assert dev[0] == host[0]
    if family == "none":
        assert dev[1:] == (N, N - len(c["recs"]))
    if family == "letters":
        assert dev[1] == len(set(bytes(c["bases"]).upper()))
    if family == "palindrome" and N > 2:
        assert pi.self_reverse_edges(dev[0]) >= 1
    if N <= pi.ORACLE_GFA_MAX:
        o = pi.oracle_unite(c["recs"], c["unions"])
        g = o.gfa(canonical=True)
        o.close()
        assert canon_gfa(dev[0]) == canon_gfa(g[0]) and dev[1:] == g[1:]
    if devc is not None:
        oc = ob.compact_gfa(dev[0])
        assert canon_gfa(devc[0]) == canon_gfa(oc[0]) and devc[1:] == oc[1:]
        assert devc == build_gfa(ss, labels, compact=True)


# ------------------------------------------------------------------------------------------ 3. the unite kernel
def unite_paf(recs, paf_text, k, path):
    path.write_text(paf_text)
    ss = SeqSet(recs)
    ctx = Context(0)
    ctx.load_paf(ss, Params(min_match_len=k), str(path))
    ctx.unite(); ctx.sync()
    return ss, ctx


@pytest.mark.parametrize("k", pi.CIGAR_K)
@pytest.mark.parametrize("name", pi.CIGAR_NAMES)
def test_unite_kernel_on_cigar_recipes(gpu, tmp_path, name, k):
    """uf_unite_cigar: chunks of 256 operations with the query and target carries crossing them (255 / 256 / 257 / 513
    operations), a chunk that unites nothing between two that do, more united bases in a chunk than threads (one = of
    70 000), runs of k-1 / k / k+1 right behind a chunk boundary, each on both strands and from nonzero starts; the p1 == p2
    skip of a self record; M and = over unequal bytes (src/seqrush.rs:1268-1330: the host compares the bases, as the oracle
    does).  Labels equal the oracle's replay and the plain union-find fed from the Python walk; counters 4 and 5 (united
    bases, match runs) equal what the walk counts"""
    c = pi.cigar_case(name)
    want, bases, nruns = cigar_reference(name, k)
    _, ctx = unite_paf(c["recs"], c["paf"], k, tmp_path / "r.paf")
    labels = ctx.download_labels()
    cnt = ctx.counters()
    nodes = ctx.download_uf()
    ctx.close()
    assert np.array_equal(labels, pi.oracle_paf_replay(c["recs"], c["paf"], k))
    assert np.array_equal(labels, want)
    assert (cnt["united_bases"], cnt["match_runs"]) == (bases, nruns)
    check_forest(nodes, want)


# ------------------------------------------------------------------------------------------ 4. composition
@pytest.mark.parametrize("order", ["unite-then-merge", "merge-then-unite"])
@pytest.mark.parametrize("name,k", [("hole600", 0), ("runs8at256", 8)])
def test_unite_merge_and_induction_on_one_forest(gpu, tmp_path, name, k, order):
    """a PAF context's unite and a merge of a random partition on the same forest, in both orders, then induction (a PAF
    context keeps no byte copy: induction uploads its own): the oracle doing both.  No stage may need a fresh forest"""
    c = pi.cigar_case(name)
    recs = c["recs"]
    N = sum(len(s) for _, s in recs)
    lab, unions = pi.random_partition(N, max(1, N // 7), seed=5)
    path = tmp_path / "c.paf"
    path.write_text(c["paf"])
    ss = SeqSet(recs)
    ctx = Context(0)
    ctx.load_paf(ss, Params(min_match_len=k), str(path))
    if order == "unite-then-merge":
        ctx.unite(); ctx.sync()
        merge(ctx, [lab], 64)
    else:
        merge(ctx, [lab], 32)
        ctx.unite(); ctx.sync()
    dev = ctx.build_gfa()
    host, d64, d32 = all_labels(ctx)
    ctx.close()
    o = pi.oracle_paf_replay(recs, c["paf"], k, labels=False)
    pi.oracle_unite(recs, unions, o)
    want = o.canonical_labels()
    g = o.gfa(canonical=True)
    o.close()
    assert np.array_equal(host, want) and np.array_equal(d64, want) and np.array_equal(d32, want.astype(np.uint32))
    alone = cigar_reference(name, k)[0]
    assert not np.array_equal(want, alone) and len(np.unique(want)) < len(np.unique(alone))
    assert dev == build_gfa(ss, host)
    assert canon_gfa(dev[0]) == canon_gfa(g[0]) and dev[1:] == g[1:]


# ------------------------------------------------------------------------------------------ 5. seeded partitions
def check_random_partition(seed):
    """a seeded random partition of 2..4096 bases over a mixed alphabet, merged (either width) and induced against the host
    twins; scripts/gpu_fuzz.py runs it over a seed range"""
    from seqrush_amd.seqrush import HostUnionFind
    rng = np.random.default_rng([77, seed])
    N = int(rng.integers(2, 4097))
    bases = pi._draw(rng, pi.MIXED if seed % 2 else pi.ACGT, N)
    recs = pi._split(bases.tobytes(), N)
    arrays = [pi.random_partition(N, int(rng.integers(1, N + 1)), seed=1000 + 3 * seed + j)[0] for j in range(1 + seed % 3)]
    h = HostUnionFind(N)
    h.merge_labels(arrays)
    want = h.canonical_labels()
    ss, ctx = open_context(recs)
    merge(ctx, arrays, 64 if seed % 4 < 2 else 32)
    dev = ctx.build_gfa()
    devc = ctx.build_gfa(compact=True)
    host, d64, d32 = all_labels(ctx)
    ctx.close()
    assert np.array_equal(host, want) and np.array_equal(d64, want) and np.array_equal(d32, want.astype(np.uint32))
    assert dev == build_gfa(ss, want) and devc == build_gfa(ss, want, compact=True)


@pytest.mark.parametrize("seed", list(range(8)))
def test_seeded_random_partitions(gpu, seed):
    check_random_partition(seed)
