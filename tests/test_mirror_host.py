"""Host tests of mirrored emission: the mirror map the load path uploads (sr_mirror_map) and the two tie
rules the blocked kernel shares with the host (csrc/sr_mirror_rule.h), by enumeration.  No GPU."""
import ctypes as C
import itertools
import os
import re

import pytest

import mirror_inputs as mi
from seqrush_amd import _lib
from seqrush_amd.seqrush import Params, pair_list, mirror_map, MIRROR_NONE as NONE, MIRROR_SECONDARY as SEC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check_map(pairs, batch_first, entries, primaries):
    """the definition, written out: per batch the first (q, t) with q < t and the first (t, q) are partners"""
    bf = batch_first if batch_first is not None else [0, len(pairs)]
    want = [NONE] * len(pairs)
    n = 0
    for f, l in zip(bf[:-1], bf[1:]):
        first = {}
        for i in range(f, l):
            first.setdefault(pairs[i], i)
        for (q, t), i in first.items():
            if q < t and (t, q) in first:
                want[i] = first[t, q] - f
                want[first[t, q]] = (i - f) | SEC
                n += 1
    assert entries == want and primaries == n
    return want


def test_all_vs_all():
    n = 7
    pairs = pair_list(n, Params())
    assert len(pairs) == n * n
    ent, prim = mirror_map(pairs)
    check_map(pairs, None, ent, prim)
    assert prim == n * (n - 1) // 2
    for i, (q, t) in enumerate(pairs):
        if q == t:
            assert ent[i] == NONE
        elif q < t:
            assert ent[i] == pairs.index((t, q))
        else:
            assert ent[i] == pairs.index((t, q)) | SEC


def test_explicit_list_with_duplicate_unpaired_and_self_pairs():
    #        0       1       2       3       4       5       6       7       8
    pairs = [(3, 1), (0, 2), (1, 3), (4, 4), (1, 3), (2, 0), (0, 5), (3, 1), (2, 2)]
    ent, prim = mirror_map(pairs)
    check_map(pairs, None, ent, prim)
    # (1,3)@2 is the primary of (3,1)@0 although that one comes first; their copies @4, @7, the lone (0,5) and the self pairs: none
    assert ent == [2 | SEC, 5, 0, NONE, NONE, 1 | SEC, NONE, NONE, NONE] and prim == 2
    assert mirror_map([]) == ([], 0)
    assert mirror_map([(1, 1)]) == ([NONE], 0)


def test_partners_split_by_batches():
    pairs = [(0, 1), (0, 2), (1, 0), (2, 0), (1, 2), (2, 1)]
    ent, prim = mirror_map(pairs, [0, 2, 4, 6])
    check_map(pairs, [0, 2, 4, 6], ent, prim)
    assert ent == [NONE, NONE, NONE, NONE, 1, 0 | SEC] and prim == 1          # indices inside the batch
    ent, prim = mirror_map(pairs, [0, 3, 6])
    assert ent == [2, NONE, 0 | SEC, NONE, 2, 1 | SEC] and prim == 2
    ent, prim = mirror_map(pairs, [0, 0, 6, 6])                                # empty batches
    assert prim == 3
    L = _lib.load()
    bad = (C.c_uint32 * 3)(0, 4, 5)
    q = (C.c_uint32 * 6)(); out = (C.c_uint32 * 6)()
    assert L.sr_mirror_map(q, q, 6, bad, 2, 0, out, None) != 0


def test_a_batch_with_a_workgroup_per_pair_gets_no_partners():
    """a launch with no fewer workgroups than pairs lasts as long as its longest pair: a primary that aligned its secondary
    after itself could only lengthen it, so such a batch is left alone -- batch by batch"""
    n = 6
    pairs = pair_list(n, Params())
    full = mirror_map(pairs)
    assert full[1] == 15 and mirror_map(pairs, workgroups=35) == full
    for wg in (36, 37, 1024):
        assert mirror_map(pairs, workgroups=wg) == ([NONE] * 36, 0)
    # batches of 24 and 12 pairs on 12 workgroups: the first pairs what it holds, the second -- (4,5) and (5,4) -- nothing
    ent, prim = mirror_map(pairs, [0, 24, 36], workgroups=12)
    want, nwant = mirror_map(pairs, [0, 24, 36])
    assert ent[:24] == want[:24] and ent[24:] == [NONE] * 12 and want[24:] != [NONE] * 12
    assert prim == sum(1 for e in ent if e != NONE and not e & SEC) and 0 < prim < nwant


def test_two_rank_shard():
    """sharding is unchanged: a rank pairs what it holds, a pair whose partner went to the other rank has none"""
    n, tot, together = 9, 0, 0
    seen = set()
    for rank in range(2):
        pairs = pair_list(n, Params(shard_rank=rank, shard_count=2))
        ent, prim = mirror_map(pairs)
        check_map(pairs, None, ent, prim)
        for i, (q, t) in enumerate(pairs):
            assert (ent[i] == NONE) == (q == t or (t, q) not in pairs)
        tot += prim
        together += sum(1 for q, t in set(pairs) if q < t and (t, q) in pairs)
        seen.update(pairs)
    assert len(seen) == n * n and tot == together and 0 < tot <= n * (n - 1) // 2


# ------------------------------------------------------------------------------------------------ the rules
TAGS = {"I1-open": 1, "I1-ext": 2, "I2-open": 3, "I2-ext": 4, "D1-open": 5, "D1-ext": 6, "D2-open": 7, "D2-ext": 8, "mismatch": 9}


def test_transposed_rank_table_against_the_oracles_priority():
    """oracle/wfa.c's header comment writes the priority out; the transposed pair's is the same line with I and D swapped"""
    text = open(os.path.join(ROOT, "oracle", "wfa.c")).read()
    m = re.search(r"priority high->low:(.*?)\(SURVEY", text, re.S)
    order = [w for w in re.sub(r"[*>\s]+", " ", m.group(1)).split() if w]
    assert sorted(order) == sorted(TAGS) and order[0] == "mismatch"
    # the oracle's tag numbers are its priorities
    assert [TAGS[w] for w in order] == list(range(9, 0, -1))
    for name, tag in re.findall(r"BT_(\w+) = (\d)", text):
        key = "mismatch" if name == "MISMS" else name[:2] + "-" + name[3:].lower()
        assert TAGS[key] == int(tag)
    L = _lib.load()
    swapped = [w.translate(str.maketrans("ID", "DI")) if w != "mismatch" else w for w in order]
    rank_t = {w: L.sr_mirror_bt_rank_transposed(TAGS[w]) for w in TAGS}
    assert sorted(TAGS, key=lambda w: -rank_t[w]) == swapped
    assert swapped == ["mismatch", "I2-ext", "I2-open", "I1-ext", "I1-open", "D2-ext", "D2-open", "D1-ext", "D1-open"]


def test_backtrace_orders_agree_unless_an_i_and_a_d_tag_share_the_maximum_without_misms():
    L = _lib.load()
    arr = (C.c_int * 10)()
    n_tie = 0
    for offs in itertools.product((-1, 0, 1), repeat=9):
        arr[0] = -1
        for tag in range(1, 10):
            arr[tag] = offs[tag - 1]
        a, b, flag = L.sr_mirror_bt_pick(arr, 0), L.sr_mirror_bt_pick(arr, 1), L.sr_mirror_bt_tie_host(arr)
        mx = max(offs)
        if mx < 0:
            assert a == b == 0 and not flag
            continue
        at_max = [tag for tag in range(1, 10) if offs[tag - 1] == mx]
        assert a == max(at_max)                                              # the oracle's rule
        expect = any(t <= 4 for t in at_max) and any(5 <= t <= 8 for t in at_max) and 9 not in at_max
        assert (a != b) == expect and bool(flag) == expect, (offs, a, b, flag)
        n_tie += expect
    assert n_tie > 0


def test_breakpoint_keys_pick_what_the_two_walks_pick():
    """candidates of one overlap call: this pair's walk takes the smallest value, then the earliest (distance, component in
    the order D2 I2 D1 I1 M), then the smallest diagonal; the transposed pair's walk I2 D2 I1 D1 M and the largest diagonal.
    The packed keys pick exactly those, and the call is flagged iff they name different (component, diagonal)"""
    L = _lib.load()
    M, I1, I2, D1, D2 = range(5)
    walk, walk_t = [D2, I2, D1, I1, M], [I2, D2, I1, D1, M]
    cands = [(v, i, c, k) for v in (10, 11) for i in (0, 1) for c in range(5) for k in (-3, 0, 2)]
    import random
    rnd = random.Random(5)
    flagged = 0
    for trial in range(3000):
        cs = rnd.sample(cands, rnd.randint(1, 5))
        n = len(cs)
        cols = [(C.c_int * n)(*[c[j] for c in cs]) for j in range(4)]
        pa, pb = C.c_int(), C.c_int()
        flag = L.sr_mirror_bp_pick_host(cols[0], cols[1], cols[2], cols[3], n, 24, C.byref(pa), C.byref(pb))
        a = min(range(n), key=lambda j: (cs[j][0], cs[j][1], walk.index(cs[j][2]), cs[j][3]))
        b = min(range(n), key=lambda j: (cs[j][0], cs[j][1], walk_t.index(cs[j][2]), -cs[j][3]))
        assert (pa.value, pb.value) == (a, b)
        assert bool(flag) == (cs[a][2:] != cs[b][2:])
        flagged += bool(flag)
    assert 0 < flagged < 3000


def test_input_a_has_non_transposable_pairs():
    """the GPU tests on Input A are not vacuous: the oracle's CIGARs of at least 3 unordered pairs are not transposes"""
    o = mi.oracle_once("A")
    assert len(o.non_transposable()) >= 3
    assert len(o.non_transposable()) == 7          # this seed's draw (mirror_inputs.A_SEED)
    assert not o.reverse_pairs()
    assert not mi.oracle_once("subst").reverse_pairs()
    assert mi.oracle_once("rc").reverse_pairs()
