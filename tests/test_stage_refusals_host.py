"""CPU test (-m "not gpu") that pins what the graph stages (stats, bins, growth, variants, lift, and the plan of extend) say
when they refuse an input: the status code and the bytes of sr_last_error(), against tests/golden/stage_refusals.json.  The
record was taken before the stages were moved onto the shared path-table builder and stream helper (sr_path_tables.h,
sr_stage_dev.h), so it holds them to the wording and to the order of the checks they had when each built its tables itself.

The defects are the ones a GFA text can carry past the parser: a node with an empty sequence, an unknown ref / to name, and
pairs of defects whose order of report is part of the contract (the option checks and the caps of a stage come before the
node loop, the name lookup before the empty sequence).  Node ids that are not dense also pass the parser, but it maps
them to 1..n itself, so every stage accepts them: the record says so (status 0).  The device cases ask for device 0 on a
machine that has none; where a HIP device is present they are skipped.

Never reaches a stage, because the parser refuses it first (so "node ids must be dense", "a path step names a missing
node" and "an edge names a missing node" cannot be provoked through a *_gfa entry point, and no way in is invented here):
  - a P line that names a segment without an S line   ("GFA: a P line names a missing segment ...")
  - an L line that names a segment without an S line  ("GFA: an L line names a missing segment")
  - two S lines with one id                           ("GFA: duplicate S id ...")
  - an id that is not a positive number below 2^31    ("GFA line n: S needs a positive numeric id and a sequence")"""
import json
import os

import pytest

from seqrush_amd import _lib
from seqrush_amd.seqrush import ExtendPlan, SeqRushError, graph_stats, growth, lift, path_bins, variants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "stage_refusals.json")
TWIN = -1

GOOD = "S\t1\tAC\nS\t2\tG\nS\t3\tTT\nL\t1\t+\t2\t+\t0M\nL\t2\t+\t3\t+\t0M\nL\t1\t+\t3\t+\t0M\nP\ta\t1+,2+,3+\t*\nP\tb\t1+,3+\t*\n"
NOT_DENSE = GOOD.replace("S\t2\t", "S\t20\t").replace("\t2\t+", "\t20\t+").replace("2+", "20+") \
                .replace("S\t3\t", "S\t700\t").replace("\t3\t+", "\t700\t+").replace("3+", "700+")
EMPTY_SEQ = GOOD.replace("S\t2\tG\n", "S\t2\t\n")
MANY_PATHS = "S\t1\t\nP\tq\t1+\t*\n" + "".join(f"P\te{k}\t\t*\n" for k in range(4096))      # 4097 paths, an empty sequence
BED = "a\t0\t2\n"

STAGES = {
    "stats": lambda text, device, **kw: graph_stats(text, device),
    "bins": lambda text, device, **kw: path_bins(text, device, **(kw or dict(bins=2))),
    "growth": lambda text, device, **kw: growth(text, device, **(kw or dict(permutations=4))),
    "variants": lambda text, device, **kw: variants(text, device, **kw),
    "lift": lambda text, device, **kw: lift(text, BED, device, **kw),
    "extend": lambda text, device, **kw: ExtendPlan(text, [("n", b"ACGT")], device).close(),
}

# name -> (stage, text, keyword arguments); every one through the host twin
DEFECTS = {f"{stage}/not_dense": (stage, NOT_DENSE, {}) for stage in STAGES}
DEFECTS.update({f"{stage}/empty_sequence": (stage, EMPTY_SEQ, {}) for stage in STAGES})
DEFECTS.update({
    "variants/unknown_ref": ("variants", GOOD, dict(ref="nobody")),
    "lift/unknown_to": ("lift", GOOD, dict(to="nobody")),
    # two defects: which one is reported
    "variants/unknown_ref_and_empty_sequence": ("variants", EMPTY_SEQ, dict(ref="nobody")),
    "lift/unknown_to_and_empty_sequence": ("lift", EMPTY_SEQ, dict(to="nobody")),
    # the checks of a stage that come before its tables are filled
    "stats/path_cap": ("stats", MANY_PATHS, {}),
    "bins/both_options": ("bins", EMPTY_SEQ, dict(bins=2, bin_width=2)),
    "growth/no_permutations": ("growth", EMPTY_SEQ, dict(permutations=0)),
    "growth/group_out_of_range": ("growth", EMPTY_SEQ, dict(permutations=4, group_of=[0, 5], n_groups=2)),
    "growth/group_without_path": ("growth", EMPTY_SEQ, dict(permutations=4, group_of=[0, 0], n_groups=2)),
    "growth/group_cap": ("growth", MANY_PATHS, dict(permutations=4)),
})
NO_DEVICE = {f"{stage}/no_device": (stage, GOOD, {}) for stage in STAGES}


def observe(stage, text, device, kw):
    """[status, the bytes of sr_last_error() as text]; a stage that accepts the input: [0, ""]"""
    try:
        STAGES[stage](text, device, **kw)
    except SeqRushError as e:
        return [e.code, _lib.load().sr_last_error().decode("latin-1")]
    return [0, ""]


def record():
    """the content of the golden file (json.dump(record(), ..., indent=1, sort_keys=True)), as it was taken from the build
    before the stages shared their tables: the defects through the twin, the device cases on a machine without a device"""
    out = {name: observe(stage, text, TWIN, kw) for name, (stage, text, kw) in DEFECTS.items()}
    if _lib.load().sr_device_count() == 0:
        out.update({name: observe(stage, text, 0, kw) for name, (stage, text, kw) in NO_DEVICE.items()})
    return out


def _golden():
    return json.load(open(GOLDEN))


def test_the_record_holds_every_case():
    assert set(_golden()) == set(DEFECTS) | set(NO_DEVICE)
    refused = [k for k, v in _golden().items() if v[0]]
    assert {"variants/empty_sequence", "lift/empty_sequence", "variants/unknown_ref", "lift/unknown_to"} <= set(refused)
    assert all(_golden()[k][0] == -2 and "no HIP device (device -1 selects the host twin)" in _golden()[k][1] for k in NO_DEVICE)


@pytest.mark.parametrize("name", sorted(DEFECTS))
def test_a_defect_is_refused_as_recorded(name):
    stage, text, kw = DEFECTS[name]
    assert observe(stage, text, TWIN, kw) == _golden()[name]


@pytest.mark.parametrize("name", sorted(NO_DEVICE))
def test_no_device_is_refused_as_recorded(name):
    if _lib.load().sr_device_count() > 0:
        pytest.skip("a HIP device is present: device 0 is not refused")
    stage, text, kw = NO_DEVICE[name]
    assert observe(stage, text, 0, kw) == _golden()[name]
