"""GPU parity tests (-m gpu) for the four kernels of `-x tree:` pair selection, stage by stage: sr_kmer_hash_kernel and
sr_sketch_sort_kernel (the sketch rows), sr_jaccard_kernel (the shared / denom matrices), sr_knn_select_kernel (the
selection), each against the plain reference of tests/sketch_inputs.py on the inputs built for its edges, and the load
path's pair list against the reference's.  The intermediates come from sr_sketch_device / sr_knn_select_device, which run
the routine the load path runs.  Every comparison is exact."""
import numpy as np
import pytest

import sketch_inputs as si
from seqrush_amd.seqrush import Context, Params, SeqSet, knn_select_device, sketch_device

pytestmark = pytest.mark.gpu

FILL = np.uint64(si.SENTINEL)
STAGE_CASES = [(name, k) for name in sorted(si.SMALL_SETS) for k in si.SMALL_SETS[name][1]] + [("family130", 8)]
PATH_SETS = ["cut", "chunks", "alphabet", "jaccard", "kmer16", "kmer32", "family130"]


def records(name):
    return si.family130() if name == "family130" else si.SMALL_SETS[name][0]()


def check_rows(recs, k, sketch, sketch_n, want):
    """sketch rows against the reference sketches `want`: counts, the sketch, and the untouched rest of every row"""
    assert sketch.shape == (len(recs), si.SKETCH) and sketch.dtype == np.uint64
    for i, (name, _) in enumerate(recs):
        w = want[i]
        assert int(sketch_n[i]) == len(w), (name, k)
        assert sketch[i, :len(w)].tolist() == w, (name, k)
        assert (sketch[i, len(w):] == FILL).all(), (name, k, "a write at or past the count")


def u32(m):
    return np.array(m, dtype=np.uint32).reshape(len(m), len(m))


# ------------------------------------------------------------------------------------------ 1. sketch rows and matrices
@pytest.mark.parametrize("name,k", STAGE_CASES, ids=[f"{n}-k{k}" for n, k in STAGE_CASES])
def test_sketch_rows_and_matrices_equal_the_reference(gpu, name, k):
    recs = records(name)
    want_sk, want_sh, want_dn = si.reference(recs, k)
    sketch, sketch_n, shared, denom = sketch_device(SeqSet(recs), k)
    check_rows(recs, k, sketch, sketch_n, want_sk)
    assert np.array_equal(shared, u32(want_sh)) and np.array_equal(denom, u32(want_dn))
    assert np.array_equal(shared, shared.T) and np.array_equal(denom, denom.T)
    assert not shared.diagonal().any() and not denom.diagonal().any()


@pytest.mark.parametrize("k", si.KMER_SIZES)
def test_sketch_rows_ignore_strand_and_case(gpu, k):
    """the device rows of every member, of its reverse complement and of its lower case are the same rows"""
    recs = si.kmer_set(k) + si.alphabet_set() + [(n, s) for n, s in si.chunk_set() if len(s) <= 3]
    if k == 16:
        recs = recs + si.cut_set()
    fwd = sketch_device(SeqSet(recs), k)
    rc = sketch_device(SeqSet([(n, si.revcomp(s)) for n, s in recs]), k)
    low = sketch_device(SeqSet([(n, s.lower()) for n, s in recs]), k)
    assert any(si.revcomp(s) != s for _, s in recs) and fwd[1].any()
    for other in (rc, low):
        for a, b in zip(fwd, other):                 # rows and counts; the matrices follow from them
            assert np.array_equal(a, b)


def test_single_member_and_argument_checks(gpu):
    from seqrush_amd._lib import SeqRushError
    s = si.rnd(40, 1)
    sketch, sketch_n, shared, denom = sketch_device(SeqSet([("one", s)]), 5)
    check_rows([("one", s)], 5, sketch, sketch_n, [si.sketch(s, 5)])
    assert shared.tolist() == [[0]] and denom.tolist() == [[0]]
    for k in (0, 33):
        with pytest.raises(SeqRushError):
            sketch_device(SeqSet([("one", s)]), k)


# ------------------------------------------------------------------------------------------ 2. the grid-stride loop
def test_jaccard_grid_stride_loop_on_2049_members(gpu):
    """n * n > 16384 * 256 threads: the entries past the grid come from the loop's second trip.  Every sketch at k = 2 is a
    subset of 10 hashes, so the reference for all 4.2 M entries is popcount(a & b) / popcount(a | b) on bit masks"""
    recs = si.big_set()
    n = len(recs)
    want_sk, universe, masks = si.big_masks(recs)
    sketch, sketch_n, shared, denom = sketch_device(SeqSet(recs), 2)
    assert n * n > 16384 * 256 and len(universe) <= 10
    assert np.array_equal(sketch_n, np.array([len(w) for w in want_sk], dtype=np.uint32))
    full = np.full((n, si.SKETCH), FILL, dtype=np.uint64)
    for i, w in enumerate(want_sk):
        full[i, :len(w)] = w
    assert np.array_equal(sketch, full)
    m = np.array(masks, dtype=np.uint16)
    pop = np.array([bin(v).count("1") for v in range(1024)], dtype=np.uint32)
    want_sh = pop[m[:, None] & m[None, :]]
    want_dn = np.maximum(pop[m[:, None] | m[None, :]], 1)
    np.fill_diagonal(want_sh, 0); np.fill_diagonal(want_dn, 0)
    assert np.array_equal(shared, want_sh) and np.array_equal(denom, want_dn)


# ------------------------------------------------------------------------------------------ 3. selection
@pytest.mark.parametrize("variant", si.SELECT_VARIANTS)
@pytest.mark.parametrize("n", si.SELECT_N)
def test_selection_equals_the_reference_on_synthetic_matrices(gpu, n, variant):
    sh, dn, _ = si.select_matrix(n, variant)
    for kn, kf in si.select_k(n):
        sel = knn_select_device(u32(sh), u32(dn), kn, kf)
        assert sel.shape == (n, n) and not sel.diagonal().any()
        assert np.array_equal(sel, np.array(si.selection(sh, dn, kn, kf), dtype=np.uint8).reshape(n, n)), (kn, kf)


# ------------------------------------------------------------------------------------------ 4. the whole path
@pytest.mark.parametrize("name", PATH_SETS)
def test_load_path_pair_lists_equal_the_reference(gpu, name):
    """Context.load(-x tree:...).pairs() == the reference's pair list, with and without exclude_self; and the selection
    stage run on the matrices of the sketch stage gives the selection that this pair list implies"""
    recs = records(name)
    n = len(recs)
    assert 1 < n <= 130
    ss = SeqSet(recs)
    for spec in si.SPECS:
        kn, kf, rf, k = si.parse_spec(spec)
        got = {}
        for ex in (False, True):
            ctx = Context(0)
            ctx.load(ss, Params(sparsification=spec, exclude_self=int(ex)))
            got[ex] = ctx.pairs()
            ctx.close()
            assert got[ex] == si.tree_pairs(recs, spec, exclude_self=ex), (spec, ex)
        _, _, shared, denom = sketch_device(ss, k)
        sel = knn_select_device(shared, denom, kn, kf)
        assert np.array_equal(sel, np.array(si.sel_of_spec(recs, spec), dtype=np.uint8).reshape(n, n)), spec
        for ex in (False, True):
            assert si.pair_list(n, sel.tolist(), 42, rf, exclude_self=ex) == got[ex], (spec, ex)
