"""Host side of the resident-context tests: the inputs of resident_inputs.py discriminate.  A member of the context that
survives a reload (a flag, a pointer, a count of the previous load) only changes a result when the previous load differed from
the next in what that member steers.  So, from the oracle alone: consecutive inputs of the reload chain differ in their sizes
and in their labels, equal-sized ones cannot stand in for each other, A has what B lacks (mirror partners, both strands), the
PAF file of C replays to C's partition, and the failing loads are refused before a device is needed.  The oracle answers
computed here are the ones test_resident_gpu.py compares the device with (resident_inputs.oracle is cached)."""
import numpy as np
import pytest

import extend_inputs as ei
import oracle_binding as ob
import resident_inputs as ri
from partition_inputs import oracle_paf_replay
from seqrush_amd.seqrush import mirror_map, MIRROR_NONE, MIRROR_SECONDARY

LOADS = ri.chain_loads()
STEPS = list(zip(LOADS, LOADS[1:]))
# B has three sequences because the issue of these tests says so, and so has every inversion family of inversion_helpers: the
# one step of the chain where n and the pair count cannot differ.  Total length, labels, alphabet, penalties and kernel do.
SAME_COUNT_STEPS = {("EI", "B")}


def test_chain_order_is_the_documented_one():
    assert ri.CHAIN == ("A", "B", "F-empty", "C", "A", "D", "EI", "B", "EX", "F-pair", "A")
    assert LOADS.count("A") == 3 and LOADS.count("B") == 2


@pytest.mark.parametrize("prev,nxt", STEPS, ids=[f"{a}-{b}" for a, b in STEPS])
def test_consecutive_loads_differ(prev, nxt):
    a, b = ri.sizes(prev), ri.sizes(nxt)
    assert a["total_len"] != b["total_len"] and a["uf_size"] != b["uf_size"]
    if (prev, nxt) not in SAME_COUNT_STEPS:
        assert a["n"] != b["n"] and a["pairs"] != b["pairs"]
    la, lb = ri.oracle(prev)["labels"], ri.oracle(nxt)["labels"]
    m = min(len(la), len(lb))
    assert len(la) == a["uf_size"] and len(lb) == b["uf_size"]
    assert not np.array_equal(la[:m], lb[:m])           # labels left over from the previous load are a wrong answer
    assert ri.oracle(prev)["recs"] != ri.oracle(nxt)["recs"]


def test_equal_sized_inputs_cannot_stand_in_for_each_other():
    names = sorted(set(LOADS) | {"P"})
    for i, x in enumerate(names):
        for y in names[i + 1:]:
            lx, ly = ri.oracle(x)["labels"], ri.oracle(y)["labels"]
            if len(lx) == len(ly):
                assert not np.array_equal(lx, ly), (x, y)


def test_b_is_smaller_than_a_in_every_size():
    a, b = ri.sizes("A"), ri.sizes("B")
    assert all(b[k] < a[k] for k in ("n", "total_len", "uf_size", "pairs"))
    assert a["total_len"] <= 8 * 500 and b["total_len"] <= 8 * 500
    alphabet = set(b"".join(s for _, s in ri.input_b()))
    assert alphabet - set(b"ACGT") and 4 < len(alphabet) <= 16          # N, R, lower case: 4-bit symbols
    assert set(b"".join(s for _, s in ri.input_a())) <= set(b"ACGT")


def test_a_has_mirror_partners_in_every_batch_and_both_strands():
    res = ri.oracle("A")
    per = ri.A_BATCH_PAIRS
    bf = list(range(0, len(res["pairs"]), per)) + [len(res["pairs"])]
    assert len(bf) - 1 >= 3
    # the arena rule of plan_memory: a batch ends before the pair whose reserve no longer fits
    arena, base = int(ri.A_ENV["SR_CIGAR_ARENA_OPS"]), 2 * ri.A_LEN + 2
    assert per * base + 1 <= arena < (per + 1) * base + 1
    entries, primaries = mirror_map(res["pairs"], bf, int(ri.A_ENV["SR_NWG"]))
    assert primaries > 0 and per > int(ri.A_ENV["SR_NWG"])
    assert sum(1 for e in entries if e != MIRROR_NONE and e & MIRROR_SECONDARY) == primaries
    assert mirror_map(res["pairs"], bf, per)[1] == 0          # a workgroup per pair: no partners, hence SR_NWG
    assert set(res["is_reverse"].tolist()) == {0, 1}


def test_a_and_the_inversion_input_differ_in_a_strand():
    a, e = ri.oracle("A"), ri.oracle("EI")
    m = min(len(a["is_reverse"]), len(e["is_reverse"]))
    assert not np.array_equal(a["is_reverse"][:m], e["is_reverse"][:m])
    assert sum(j["accepted"] for j in e["jobs"]) >= 1
    assert not np.array_equal(e["labels"], e["plain"]["labels"])      # a patch pass that runs by mistake, or not at all, shows


def test_paf_of_c_replays_to_the_oracles_partition():
    res = ri.oracle("C")
    assert len(res["paf"].strip().split("\n")) == 16
    assert np.array_equal(oracle_paf_replay(ri.input_c(), res["paf"], 0), res["labels"])
    assert set(res["is_reverse"].tolist()) == {0, 1}


def test_iterative_input_never_stabilizes_and_differs_from_the_plain_list():
    d = ri.oracle("D")
    assert not d["stabilized"] and d["processed"] == len(d["random"]) > 0
    assert len(d["pairs"]) == 4 * (len(d["tree"]) + len(d["random"])) != d["n"] ** 2


def test_extend_input_seed_differs_from_identity_and_from_the_result():
    res = ri.oracle("EX")
    recs, m = ri.input_ex()
    seed = ei.restate(res["old_gfa"], recs[m:])
    assert seed["records"] == recs
    ident = ei.plain_labels(res["total_len"], [])
    assert not np.array_equal(seed["labels"], ident)                  # reset_uf() of an extend context is not init only
    assert not np.array_equal(seed["labels"], res["labels"])          # and the run adds to the seed
    assert len(seed["labels"]) == res["uf_size"]


def test_explicit_pair_list_differs_from_all_pairs():
    assert not np.array_equal(ri.oracle("P")["labels"], ri.oracle("C")["labels"])
    assert len(ri.oracle("P")["pairs"]) == len(ri.P_PAIRS) < 16


def test_failing_inputs_are_refused_by_the_oracle_too():
    with pytest.raises(ValueError):
        ob.OracleSeqRush(records=ri.input_f_empty())
    n = len(ri.input_c())
    assert any(q >= n or t >= n for q, t in ri.F_BAD_PAIRS)


def test_oracle_answers_are_cached_and_read_only():
    for name in sorted(set(LOADS) | {"P"}):
        r = ri.oracle(name)
        assert ri.oracle(name) is r
        with pytest.raises(ValueError):
            r["labels"][0] = 1
    # counters 4 and 5 of a pass: every base of a match run, every run (uf_unite_cigar counts self pairs too)
    a = ri.oracle("A")
    assert a["united_bases"] >= ri.A_N * ri.A_LEN and a["match_runs"] >= len(a["pairs"])
    assert all(int(n) >= 1 for n in a["nops"])
