"""CPU tests of the rotating tile priority's rule (seqrush_amd/csrc/sr_prio_rule.h) through its exported host
twin sr_tile_prio_role_host: the s_setprio level of a workgroup's tile code from its rank among the workgroups of its CU, the
epoch and the workgroups per CU."""
from collections import Counter

import pytest

from seqrush_amd import _lib

WG = (1, 2, 4, 8, 16)
# epochs around 0, around a multiple of every wg_per_cu, and where the 32-bit epoch wraps
EPOCH0 = (0, 1, 5, 16, 4093, 12345, 2 ** 31 - 3, 2 ** 32 - 40)


def role(rank, epoch, wg):
    return _lib.load().sr_tile_prio_role_host(rank, epoch & 0xffffffff, wg)


@pytest.mark.parametrize("wg", WG)
def test_every_epoch_permutes_the_role_multiset(wg):
    want = Counter(role(r, 0, wg) for r in range(wg))
    for e0 in EPOCH0:
        for e in range(e0, e0 + 2 * wg + 3):
            assert Counter(role(r, e, wg) for r in range(wg)) == want, (wg, e)
    assert all(0 <= lv <= 3 for lv in want)
    if wg == 4:
        assert want == Counter({0: 1, 1: 1, 2: 1, 3: 1})      # four co-resident workgroups hold four distinct levels
    if wg >= 4:
        assert set(want) == {0, 1, 2, 3} and len(set(want.values())) == 1
    if wg == 2:
        assert len(want) == 2


@pytest.mark.parametrize("wg", WG)
def test_every_rank_holds_every_role_equally_often(wg):
    """over wg_per_cu consecutive epochs a rank's roles are the multiset one epoch deals to the ranks"""
    want = Counter(role(r, 0, wg) for r in range(wg))
    for e0 in EPOCH0:
        if e0 + wg > 2 ** 32 and (2 ** 32) % wg:
            continue                                          # (a wrap inside the window skips positions unless wg divides 2^32)
        for r in range(wg):
            assert Counter(role(r, e, wg) for e in range(e0, e0 + wg)) == want, (wg, e0, r)


def test_one_workgroup_per_cu_is_always_zero():
    for e0 in EPOCH0:
        for e in range(e0, e0 + 5):
            for r in (0, 1, 3, 1000):
                assert role(r, e, 1) == 0
                assert role(r, e, 0) == 0


@pytest.mark.parametrize("wg", WG + (3, 5, 12))
def test_levels_stay_within_0_to_3(wg):
    for e0 in EPOCH0:
        for e in range(e0, e0 + wg + 2):
            for r in list(range(wg)) + [wg, 2 * wg + 1, 4095]:      # (the kernel passes arrival % wg; any rank is reduced the same way)
                assert 0 <= role(r, e, wg) <= 3
                assert role(r, e, wg) == role(r % wg, e, wg)


def test_epoch_shift_is_exported():
    assert _lib.load().sr_tile_prio_epoch_shift() == 11
