"""Host tests of the blocked kernel's tail launch: the shape rule the load path applies (sr_tail_shape: the
widest instance sr_align_blk.hip has for the plan that is wider than the main launch and whose LDS fits) and the knob table."""
import os

from seqrush_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C2_WORDS = 5000 // 16 + 3            # words per staged copy of a 5 kb sequence (16 bases per word + pads)


def shape(impl=2, levels=10, wave=0, off16=1, ring_u16=0, bits=2, two=1, main=256, words=C2_WORDS, forced=0):
    return _lib.load().sr_tail_shape(impl, levels, wave, off16, ring_u16, bits, two, main, words, forced)


def test_widest_instance_of_the_plan():
    assert shape() == 1024                                   # int16 rows, two-piece, 2-bit symbols: the 1 024-thread build
    assert shape(main=512) == 1024
    assert shape(two=0) == 512                               # one-piece: 512 is the widest
    assert shape(bits=4) == 512 and shape(bits=8) == 512     # the 1 024-thread build is 2-bit only
    assert shape(off16=0, ring_u16=1) == 512                 # 32-bit searches on the uint16 ring
    assert shape(off16=0, ring_u16=1, two=0) == 512


def test_nothing_wider_means_no_tail():
    assert shape(main=1024) == 0                             # the main launch already has the widest
    assert shape(two=0, main=512) == 0
    assert shape(off16=0, ring_u16=1, main=512) == 0
    assert shape(off16=0, ring_u16=0) == 0                   # 32-bit rows: one build, 256 threads
    assert shape(levels=5) == 0 and shape(levels=5, main=128) == 0      # the 5-level instances
    assert shape(wave=1, main=64) == 0 and shape(wave=1, main=128) == 0   # one- and two-wave builds
    assert shape(impl=1) == 0                                # the level-per-pass kernel has no mirror partners either


def test_lds_must_fit():
    """static tables (25 / 28 / 34 KB at 256 / 512 / 1 024 threads) + four copies of 16 bytes per word + 16 under 128 KB"""
    fits_1024 = (128 * 1024 - 34 * 1024 - 16) // 16
    assert shape(words=fits_1024) == 1024
    assert shape(words=fits_1024 + 1) == 512                 # the copies no longer fit beside the 1 024-thread tables
    fits_512 = (128 * 1024 - 28 * 1024 - 16) // 16
    assert shape(words=fits_512) == 512
    assert shape(words=fits_512 + 1) == 0
    assert shape(words=fits_512 + 1, forced=256) == 256


def test_forced_shape_among_existing_instances():
    for t in (256, 512, 1024):
        assert shape(forced=t) == t
    assert shape(forced=256, main=1024) == 256               # forced: whatever the main launch has
    assert shape(two=0, forced=1024) == 512                  # no one-piece 1 024-thread build: the widest below
    assert shape(off16=0, ring_u16=1, forced=1024) == 512
    assert shape(off16=0, ring_u16=0, forced=512) == 256
    assert shape(levels=5, forced=512) == 0 and shape(wave=1, main=64, forced=256) == 0
    assert shape(forced=100) == 0


def test_knobs_are_documented():
    doc = _lib.load().sr_knobs_doc().decode()
    names = [ln.split("\t")[0] for ln in doc.strip().split("\n")]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for k in ("SR_TAIL", "SR_TAIL_THREADS", "SR_TAIL_ROUNDS"):
        assert names.count(k) == 1
        assert len([ln for ln in doc.split("\n") if ln.startswith(k + "\t")][0].split("\t")) == 3
        assert f"`{k}" in design
    rounds = [ln for ln in doc.split("\n") if ln.startswith("SR_TAIL_ROUNDS\t")][0].split("\t")[1]
    assert rounds == "8"
