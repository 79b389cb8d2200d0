"""CPU side of the mode-by-mirroring tests (tests/mode_tie_inputs.py; device side: test_modes_mirrored_gpu.py): the conditions
on the three inputs as exact counts (PINNED: a later change of a generator cannot quietly make the device tests vacuous), and
the mirror map of every mode's actual pair list in its actual batch layout -- sr_mirror_map against a restatement of the rule
in the comment above mirror_map (sr_pairs.cpp) -- with the number of partners per list at 2 and 8 workgroups (PARTNERS), which
the device file takes its expectations from.  No GPU."""
import pytest

import inversion_helpers as ih
import mode_tie_inputs as mt
import tie_inputs as ti
from seqrush_amd.seqrush import mirror_map

# --------------------------------------------------------------------------------------------- the conditions, pinned
PINNED_ITER = dict(tree=16, random=215, processed=180, stabilized=True, checks=18, distinct_counts=7, non_transposable=22,
                   transposable_with_gaps=146, non_transposable_last_two_chunks=4)
PINNED_INV = dict(jobs=8, accepted=6, rejected=2, non_transposable=4, non_transposable_both_accepted=1,
                  transposable_both_accepted=2, reverse=0, joined_jobs=30, joined_accepted=2, joined_islands=94)
# family -> (pairs on the -x tree:2,1,0.5 list, unordered pairs with both orders on it, pairs per shard, unordered pairs whose
# two orders went to different shards)
PINNED_SPARSE = {"A": (30, 12, (15, 15), 12), "deep_ties": (34, 14, (17, 17), 14), "unequal_blocks_400": (32, 13, (16, 16), 7)}
# pairs with an unflagged depth-0 search above a flagged record (tie_inputs.Census.deep_tie_pairs): what a replay needs
PINNED_DEEP = {"iter_ties": 12, mt.INV_NAME: 2}


def test_inputs_are_deterministic_and_two_bit():
    for name in mt.SETS:
        recs = mt.records(name)
        assert recs == tuple(mt.SETS[name]()) and len({n for n, _ in recs}) == len(recs)
        assert all(set(s) <= set(b"ACGT") for _, s in recs)
    lens = [len(s) for _, s in mt.records("iter_ties")]
    assert 20 <= len(lens) <= 24 and 600 <= min(lens) and max(lens) <= 700
    assert mt.records("iter_never") == mt.records("iter_ties")[:mt.NEVER_N]
    lens = [len(s) for _, s in mt.records(mt.INV_NAME)]
    assert 4 <= len(lens) <= 5 and 900 <= min(lens) and max(lens) <= 1200


def test_iter_ties_conditions():
    c = mt.iter_counts()
    assert c["random"] >= 100 and c["stabilized"] and c["processed"] < c["random"] and c["distinct_counts"] > 1
    assert c["non_transposable"] >= 5 and c["transposable_with_gaps"] >= 5 and c["non_transposable_last_two_chunks"] >= 1
    assert c == PINNED_ITER, c
    # the run takes more than one window as planned, and the stop falls into the second
    assert mt.iter_windows("iter_ties", "planned") == [0, 64, 464, 924] and mt.windows_that_ran("iter_ties", "planned") == 3
    # one chunk per window: the arena holds 40 pairs, so the 64 tree pairs take two batches, then 18 of the 22 windows run
    assert mt.iter_windows("iter_ties", "chunk")[:4] == [0, 40, 64, 104] and mt.tree_batches("iter_ties", "chunk") == 2
    assert len(mt.iter_windows("iter_ties", "chunk")) - 1 == 24 and mt.windows_that_ran("iter_ties", "chunk") == 20
    never = mt.iter_restated("iter_never")
    assert not never["stabilized"] and never["processed"] == len(never["random"]) < 100 and never["check_counts"]
    # every member pair is forward in both orders: each entry can be a primary / secondary pair
    assert not mt.iter_oracle().reverse_pairs()


def test_inv_ties_conditions():
    c = mt.inv_counts()
    assert c["non_transposable_both_accepted"] >= 1 and c["transposable_both_accepted"] >= 1 and c["rejected"] >= 1
    assert c["joined_islands"] >= 1 and c["reverse"] == 0
    assert c == PINNED_INV, c
    # D carries the inversion and blocks of its own, C the inversion, E the replaced block
    a, b, cc, d, e = (s for _, s in mt.records(mt.INV_NAME))
    blk = a[mt.INV_AT:mt.INV_AT + mt.INV_LEN]
    assert set(blk) <= set(b"AG") and b[mt.INV_AT:mt.INV_AT + mt.INV_LEN] == blk
    assert set(cc[mt.INV_AT:mt.INV_AT + mt.INV_LEN]) <= set(b"CT") and cc[mt.INV_AT:mt.INV_AT + mt.INV_LEN] == d[mt.INV_AT:mt.INV_AT + mt.INV_LEN]
    assert e[mt.INV_AT:mt.INV_AT + mt.INV_LEN] == b"C" * mt.INV_LEN and e[mt.INV_AT + mt.INV_LEN:] == a[mt.INV_AT + mt.INV_LEN:]


@pytest.mark.parametrize("family", sorted(mt.SPARSE))
def test_sparse_ties_conditions(family):
    whole, shards = mt.sparse_list(family), mt.sparse_shards(family)
    both = [(q, t) for q, t in whole if q < t and (t, q) in set(whole)]
    assert sorted(shards[0] + shards[1]) == sorted(whole)
    assert (len(whole), len(both), tuple(len(s) for s in shards), len(mt.lost_partners(family))) == PINNED_SPARSE[family]


def test_a_family_keeps_partners_in_a_shard_and_loses_others():
    name = "unequal_blocks_400"
    nt = set(ti.oracle_once(name).non_transposable())
    for r in (0, 1):
        sh = mt.sparse_shards(name)[r]
        entries, _ = mt.mirror_rule(sh, [0, len(sh)], 2)
        prim = [sh[i] for i, e in enumerate(entries) if e != mt.NONE and not e & mt.SECONDARY]
        assert len(prim) == 3 and len(set(prim) & nt) == 1
    assert len(mt.lost_partners(name)) == 7


@pytest.mark.parametrize("name", sorted(PINNED_DEEP))
def test_replay_candidates(name):
    assert len(mt.census(name).deep_tie_pairs()) == PINNED_DEEP[name]


# --------------------------------------------------------------------------------------------- the mirror maps
def inv_list():
    n = len(mt.records(mt.INV_NAME))
    return [(q, t) for q in range(n) for t in range(n)]


INV_BATCH_PAIRS = 9                              # SR_CIGAR_ARENA_OPS of the forced-batch case: room for 9 pairs of the longest


def inv_arena_ops():
    return INV_BATCH_PAIRS * (2 * max(len(s) for _, s in mt.records(mt.INV_NAME)) + 2)


def layouts():
    """name -> (pair list, batch_first) of every list the device file runs"""
    out = {f"iter_ties/{how}": (mt.iter_list(), mt.iter_windows("iter_ties", how)) for how in ("chunk", "planned", "one")}
    out["iter_never/planned"] = (mt.iter_list("iter_never"), mt.iter_windows("iter_never", "planned"))
    inv = inv_list()
    out["inv_ties/main"] = (inv, [0, len(inv)])
    out["inv_ties/batches"] = (inv, mt.arena_batches([len(s) for _, s in mt.records(mt.INV_NAME)], inv, inv_arena_ops()))
    for name in ("inv", "pinv", "rejected", "ratio", "diverged"):
        out[name + "/main"] = ([(q, t) for q in range(3) for t in range(3)], [0, 9])
    for fam in mt.SPARSE:
        whole = list(mt.sparse_list(fam))
        out[f"sparse:{fam}/whole"] = (whole, [0, len(whole)])
        for r, sh in enumerate(mt.sparse_shards(fam)):
            out[f"sparse:{fam}/shard{r}"] = (sh, [0, len(sh)])
    return out


# layout -> primaries per batch at 2 workgroups; 8 workgroups give the same unless listed in PARTNERS_8
PARTNERS = {
    "iter_ties/chunk": (10, 6) + (10,) * 21 + (5,), "iter_ties/planned": (16, 100, 115), "iter_ties/one": (16, 215),
    "iter_never/planned": (15, 30),
    "inv_ties/main": (10,), "inv_ties/batches": (1, 1, 1),
    "inv/main": (3,), "pinv/main": (3,), "rejected/main": (3,), "ratio/main": (3,), "diverged/main": (3,),
    "sparse:A/whole": (12,), "sparse:A/shard0": (0,), "sparse:A/shard1": (0,),
    "sparse:deep_ties/whole": (14,), "sparse:deep_ties/shard0": (0,), "sparse:deep_ties/shard1": (0,),
    "sparse:unequal_blocks_400/whole": (13,), "sparse:unequal_blocks_400/shard0": (3,), "sparse:unequal_blocks_400/shard1": (3,),
}
PARTNERS_8 = {"inv_ties/batches": (1, 1, 0)}     # the last batch has 7 pairs: a workgroup per pair, no partners


def partners(layout, workgroups):
    """primaries per batch of a layout: what workspace_report()["mirror_partners"] sums"""
    if workgroups == 8 and layout in PARTNERS_8:
        return PARTNERS_8[layout]
    return PARTNERS[layout]


@pytest.mark.parametrize("workgroups", [2, 8])
def test_mirror_map_on_every_modes_list(workgroups):
    every = layouts()
    assert sorted(every) == sorted(PARTNERS)
    for name, (pairs, first) in every.items():
        want, per_batch = mt.mirror_rule(pairs, first, workgroups)
        got, n = mirror_map(pairs, first, workgroups)
        assert [int(x) for x in got] == want, name
        assert n == sum(per_batch) and per_batch == list(partners(name, workgroups)), (name, workgroups, per_batch)


def test_iterative_entries_are_all_partners():
    """every chunk is (i, i), (i, j), (j, i), (j, j): a window with more pairs than workgroups pairs every entry"""
    for how in ("chunk", "planned", "one"):
        first = mt.iter_windows("iter_ties", how)
        assert list(PARTNERS[f"iter_ties/{how}"]) == [(l - f) // 4 for f, l in zip(first, first[1:])]
    assert sum(PARTNERS["iter_ties/planned"]) == PINNED_ITER["tree"] + PINNED_ITER["random"]


def test_forced_inversion_batches():
    pairs, first = layouts()["inv_ties/batches"]
    assert len(first) - 1 >= 3 and 0 < sum(PARTNERS["inv_ties/batches"]) < sum(PARTNERS["inv_ties/main"]) == 10
    assert ih.K == 8
