"""Shared data of the instance-matrix tests (no tests here): a plain restatement of which alignment kernel instance the
host picks for a load (DESIGN.md sections 3-4), the table of every compiled instance of the two alignment kernel templates
with a recipe that reaches it through the public API, the penalty lattice around every dispatch boundary, and the seeded
inputs the host and device tests run.

The restatement is the tests' own statement of the contract.  test_instance_matrix_host.py holds it against
srk_align_blk_supports over a grid and holds the table against the kernel symbols of the built library;
test_instance_matrix_gpu.py holds it against the workspace report of every load it makes."""
import random
import re
from collections import namedtuple

from seqrush_amd import synth

# ------------------------------------------------------------------------------------------ limits the contract names
BLK_RING_SLOTS = 80            # ring depth of the blocked kernel (rows of per-level maxima it keeps per aligner)
MAX_SCOPE = 127                # deepest ring of any device kernel
NARROW_RING_LEVELS = 32        # the narrow level kernel keeps rings of up to 32 levels; deeper ones take the wide build
INT16_MAXLEN = 32000           # longest sequence whose offsets fit the int16 rows
RING_U16_MAXLEN = 57000        # longest sequence whose 32-bit searches keep a 16-bit ring (offset - 24576)
UNSUPPORTED_SCOPE_MSG = "penalties too large for the device ring (scope > 127)"

Pen = namedtuple("Pen", "x o1 e1 o2 e2 two scope")


def parse_pen(scores: str) -> Pen:
    """'m,x,o1,e1[,o2,e2]' -> Pen; scope = levels back the farthest predecessor lies, plus one"""
    v = [int(t) for t in scores.split(",")]
    assert v[0] == 0 and len(v) in (4, 6), scores
    two = len(v) == 6
    o2, e2 = (v[4], v[5]) if two else (0, 0)
    far = max(v[1], v[2] + v[3], o2 + e2 if two else 0)
    return Pen(v[1], v[2], v[3], o2, e2, two, far + 1)


DEFAULT_SCORES = "0,5,8,2,24,1"
DEFAULT_ORI = "0,1,1,1"


def second_piece(pen: Pen) -> int:
    return pen.o2 + pen.e2


def blk_levels(pen: Pen, ori: Pen) -> int:
    """levels per block of the blocked kernel's instance for these penalties, 0 = none:
    the exact instance (mismatch 5, first piece 10, second piece a multiple of five in 10..25) computes 10 levels per
    pass, the generic one 5; both want e1 = 2, e2 = 1, an orientation extension of 1 and rings within 80 rows"""
    if ori.two or ori.e1 != 1 or ori.scope + 2 > BLK_RING_SLOTS:
        return 0
    if pen.e1 != 2 or (pen.two and pen.e2 != 1):
        return 0
    exact_second = (not pen.two) or second_piece(pen) in (10, 15, 20, 25)
    if pen.x == 5 and pen.o1 + pen.e1 == 10 and exact_second:
        depth = 2 * pen.scope + 2 * 10 + 2                 # lazy I/D rows: M rows of two blocks + twice the scope
        if -(-depth // 10) * 10 <= BLK_RING_SLOTS:
            return 10
    if pen.x < 5 or pen.o1 + pen.e1 < 5 or (pen.two and second_piece(pen) < 5):
        return 0                                           # a predecessor inside the block under construction
    if pen.scope + 5 + 1 > BLK_RING_SLOTS:
        return 0
    return 5


Dispatch = namedtuple("Dispatch", "kernel_impl block_levels two_piece lazy_id_rows offset_bytes ring_cell_bytes "
                                  "threads_per_workgroup ring_depth_m ring_depth_id wide wave instance orient_route")
# one compiled instance: family 'blk' | 'bfs'; block 10 | 5 (blk) or 1 (bfs); offset / ring cell type; threads; two gap
# pieces; tick profiling; symbol bits; build 'wg4' | 'wave1' (blocked: workgroup / lean wave build) or 'lvl' | 'wide'
Instance = namedtuple("Instance", "family block offset ring threads two prof bits build")


def _knob_int(knobs, name):
    return int(knobs[name]) if name in knobs else None


def dispatch(scores=DEFAULT_SCORES, ori_scores=DEFAULT_ORI, bits=2, maxlen=2000, npairs=16, cus=256, knobs=None) -> Dispatch:
    """what a load with these penalties, alphabet, longest sequence, pair count and knobs runs.  Raises ValueError with
    the host's message for penalties no kernel takes."""
    knobs = knobs or {}
    pen, ori = parse_pen(scores), parse_pen(ori_scores)
    if pen.scope > MAX_SCOPE or ori.scope > MAX_SCOPE:
        raise ValueError(UNSUPPORTED_SCOPE_MSG)
    off16 = maxlen <= INT16_MAXLEN and "SR_FORCE_INT32" not in knobs
    words = -(-maxlen // (32 // bits)) + 2                 # one copy of the longest sequence in LDS, padded
    block = blk_levels(pen, ori)
    if block == 10 and _knob_int(knobs, "SR_BLK_LEVELS") == 5:
        block = 5
    # blocked kernel: four copies + its static tables stay below 128 KB of LDS
    impl = 2 if block > 0 and words * 16 + 28 * 1024 <= 128 * 1024 else 1
    if "SR_ALIGN_IMPL" in knobs and int(knobs["SR_ALIGN_IMPL"]) <= 1:
        impl = 1
    threads = 256
    if impl == 2 and npairs <= 2 * cus + cus // 2:
        threads = 512
    if impl == 2 and npairs <= cus:
        threads = 1024
    v = _knob_int(knobs, "SR_ALIGN_THREADS")
    if v in (128, 256, 512) or (v == 1024 and impl == 2) or (v == 64 and impl == 2 and bits == 2):
        threads = v
    if threads == 1024 and not (impl == 2 and block == 10 and off16 and bits == 2 and pen.two):
        threads = 512                                      # one 1024-thread build
    if impl == 2 and threads == 128 and block == 10 and not (bits == 2 and off16):
        block = 5                                          # the two-wave exact build is 2-bit, int16 only
    wave = impl == 2 and (threads == 64 or (threads == 128 and block == 10))
    lds = words * 16 + 16 if impl == 2 else words * 12
    u16_ok = block == 10 and maxlen <= RING_U16_MAXLEN and _knob_int(knobs, "SR_RING_U16") != 0
    # Not restated: loads whose sequence copies leave room for two workgroups per CU at most are given 512 threads by a
    # tuning rule (static LDS estimates of the host).  It cannot apply below 20 KB of copies or under SR_ALIGN_THREADS;
    # beyond that this statement of the contract declines to predict the thread count.
    if impl == 2 and not wave and "SR_ALIGN_THREADS" not in knobs and lds > 20 * 1024:
        raise NotImplementedError("thread count of an LDS-bound load is a tuning choice: give SR_ALIGN_THREADS")
    ring_u16 = impl == 2 and not off16 and u16_ok and threads >= 256
    # 32-bit searches on 32-bit rows exist at 256 threads only (and in the lean 64-thread build): the load says so
    if impl == 2 and not wave and not off16 and not ring_u16:
        threads = 256
    osz = 2 if off16 else 4
    rsz = 2 if ring_u16 else osz
    # ring depths
    lazy = impl == 2 and _knob_int(knobs, "SR_LAZY_ID") != 0 and 2 * pen.scope + 2 * block + 2 <= BLK_RING_SLOTS
    depth_m = max(pen.scope + max(block, 1), ori.scope + 1) + 1
    depth_id = depth_m
    if lazy:
        depth_id = max(depth_m, pen.scope + 2 * block + 2)
        depth_m = max(depth_m, 2 * pen.scope + 2 * block + 2)
    if impl == 2 and block == 10:
        depth_m, depth_id = -(-depth_m // 10) * 10, -(-depth_id // 10) * 10
    ring_scope = max(pen.scope, ori.scope)
    wide = impl == 1 and ring_scope + 1 > NARROW_RING_LEVELS
    # the instance the launcher starts
    ot = "int16" if off16 else "int32"
    if impl == 2:
        rt = "uint16" if ring_u16 else ot
        prof = (not wave and block == 10 and off16 and threads == 256 and bits == 2 and pen.two
                and (_knob_int(knobs, "SR_PROFILE_TICKS") or 0) != 0)
        inst = Instance("blk", block, ot, rt, threads, pen.two, prof, bits, "wave1" if wave else "wg4")
    else:
        inst = Instance("bfs", 1, ot, ot, threads, pen.two, False, bits, "wide" if wide else "lvl")
    # orientation in front of the aligner: its own kernel (blocked for 0,1,1,1, level by level otherwise) or in-kernel passes
    po = _knob_int(knobs, "SR_PREORIENT")
    pre = impl == 2 and (po != 0 if po is not None else (npairs >= 4 * cus and words * 12 <= 20 * 1024)) and words * 12 <= 60 * 1024
    ori_blocked = (ori.x, ori.o1, ori.e1) == (1, 1, 1) and "SR_ORIENT_LEVELS" not in knobs
    route = ("orient-blk" if ori_blocked else "orient-levels") if pre else "in-kernel"
    return Dispatch(impl, block if impl == 2 else 1, int(pen.two), int(lazy), osz, rsz if impl == 2 else osz, threads,
                    depth_m, depth_id, wide, wave, inst, route)


def report_mismatches(rep: dict, d: Dispatch, kernel_name: str):
    """fields of a workspace report (and the context's kernel name) that differ from the restatement"""
    want = dict(kernel_impl=d.kernel_impl, block_levels=d.block_levels, two_piece=d.two_piece, lazy_id_rows=d.lazy_id_rows,
                offset_bytes=d.offset_bytes, ring_cell_bytes=d.ring_cell_bytes, threads_per_workgroup=d.threads_per_workgroup,
                ring_depth_m=d.ring_depth_m, ring_depth_id=d.ring_depth_id, symbol_bits=d.instance.bits)
    bad = {k: (rep.get(k), v) for k, v in want.items() if rep.get(k) != v}
    name = "sr_align_blk_kernel" if d.kernel_impl == 2 else "sr_align_bfs_kernel"
    if kernel_name != name:
        bad["align_kernel"] = (kernel_name, name)
    if (rep.get("orientation_ring_bytes", 0) > 0) != (d.orient_route != "in-kernel"):
        bad["orientation_ring_bytes"] = (rep.get("orientation_ring_bytes"), d.orient_route)
    # the launchers' own choices, as the load states them
    for k, v in (("wave_build", int(d.wave)), ("level_kernel_wide", int(d.wide)), ("orientation_route", d.orient_route)):
        if rep.get(k) != v:
            bad[k] = (rep.get(k), v)
    return bad


# ------------------------------------------------------------------------------------------ instance table
ONE_PIECE = "0,5,8,2"                  # exact instance, one gap piece
WIDE_ONE_PIECE = "0,5,30,2"            # one piece, ring of 34 levels: wide level kernel under SR_ALIGN_IMPL=1
WIDE_TWO_PIECE = "0,5,8,2,40,1"        # two pieces, ring of 43 levels


def _rows():
    """(Instance, recipe) for every instantiation the two launchers can start, per build of the Makefile.  recipe:
    scores, alphabet bits and knobs; every recipe runs a family of 5 sequences (25 pairs)"""
    rows = []

    def add(inst, scores, **knobs):
        rows.append((inst, dict(scores=scores, bits=inst.bits, knobs={k: str(v) for k, v in knobs.items()})))

    for bits in (2, 4, 8):
        for two in (True, False):
            s = DEFAULT_SCORES if two else ONE_PIECE
            # blocked kernel, workgroup build: exact instance
            if bits == 2 and two:
                add(Instance("blk", 10, "int16", "int16", 1024, True, False, 2, "wg4"), s, SR_ALIGN_THREADS=1024)
                add(Instance("blk", 10, "int16", "int16", 256, True, True, 2, "wg4"), s, SR_ALIGN_THREADS=256, SR_PROFILE_TICKS=1)
            for t in (256, 512):
                add(Instance("blk", 10, "int16", "int16", t, two, False, bits, "wg4"), s, SR_ALIGN_THREADS=t)
                add(Instance("blk", 10, "int32", "uint16", t, two, False, bits, "wg4"), s, SR_ALIGN_THREADS=t, SR_FORCE_INT32=1)
            add(Instance("blk", 10, "int32", "int32", 256, two, False, bits, "wg4"), s, SR_ALIGN_THREADS=256, SR_FORCE_INT32=1, SR_RING_U16=0)
            # generic 5-level instance
            for t in (128, 256, 512):
                add(Instance("blk", 5, "int16", "int16", t, two, False, bits, "wg4"), s, SR_ALIGN_THREADS=t, SR_BLK_LEVELS=5)
            add(Instance("blk", 5, "int32", "int32", 256, two, False, bits, "wg4"), s, SR_ALIGN_THREADS=256, SR_BLK_LEVELS=5, SR_FORCE_INT32=1)
            # lean wave build (2-bit symbols only)
            if bits == 2:
                add(Instance("blk", 10, "int16", "int16", 128, two, False, 2, "wave1"), s, SR_ALIGN_THREADS=128)
                add(Instance("blk", 10, "int16", "int16", 64, two, False, 2, "wave1"), s, SR_ALIGN_THREADS=64)
                add(Instance("blk", 10, "int32", "int32", 64, two, False, 2, "wave1"), s, SR_ALIGN_THREADS=64, SR_FORCE_INT32=1)
                add(Instance("blk", 5, "int16", "int16", 64, two, False, 2, "wave1"), s, SR_ALIGN_THREADS=64, SR_BLK_LEVELS=5)
                add(Instance("blk", 5, "int32", "int32", 64, two, False, 2, "wave1"), s, SR_ALIGN_THREADS=64, SR_BLK_LEVELS=5, SR_FORCE_INT32=1)
            # level-per-pass kernel: narrow and wide builds
            for build, sc in (("lvl", s), ("wide", WIDE_TWO_PIECE if two else WIDE_ONE_PIECE)):
                for t in (128, 256, 512):
                    add(Instance("bfs", 1, "int16", "int16", t, two, False, bits, build), sc, SR_ALIGN_IMPL=1, SR_ALIGN_THREADS=t)
                    add(Instance("bfs", 1, "int32", "int32", t, two, False, bits, build), sc, SR_ALIGN_IMPL=1, SR_ALIGN_THREADS=t, SR_FORCE_INT32=1)
    return rows


INSTANCE_ROWS = _rows()
INSTANCES = [inst for inst, _ in INSTANCE_ROWS]
# compiled instances no recipe reaches: (Instance, the line of dispatch that makes it so).  None today: every launcher
# line is reachable through SR_ALIGN_THREADS / SR_FORCE_INT32 / SR_RING_U16 / SR_BLK_LEVELS / SR_ALIGN_IMPL.
UNREACHABLE = []
# requested shapes the load turns into another one (the report states the shape that runs)
SUBSTITUTIONS = [
    # (scores, bits, knobs) -> threads that run
    (dict(scores=DEFAULT_SCORES, bits=2, knobs={"SR_FORCE_INT32": "1", "SR_RING_U16": "0", "SR_ALIGN_THREADS": "512"}), 256),
    (dict(scores=DEFAULT_SCORES, bits=2, knobs={"SR_FORCE_INT32": "1", "SR_RING_U16": "0"}), 256),
    (dict(scores=DEFAULT_SCORES, bits=2, knobs={"SR_FORCE_INT32": "1", "SR_BLK_LEVELS": "5", "SR_ALIGN_THREADS": "128"}), 256),
    (dict(scores=DEFAULT_SCORES, bits=2, knobs={"SR_FORCE_INT32": "1", "SR_BLK_LEVELS": "5", "SR_ALIGN_THREADS": "512"}), 256),
    (dict(scores=DEFAULT_SCORES, bits=4, knobs={"SR_ALIGN_THREADS": "1024"}), 512),
    (dict(scores=DEFAULT_SCORES, bits=4, knobs={"SR_ALIGN_THREADS": "128"}), 128),        # exact -> generic instance at 128
    (dict(scores=DEFAULT_SCORES, bits=2, knobs={"SR_FORCE_INT32": "1", "SR_ALIGN_THREADS": "128"}), 256),
]


def instance_id(inst: Instance) -> str:
    return "%s%d-%s-%s-%dt-%s%s-s%d-%s" % (inst.family, inst.block, inst.offset, inst.ring, inst.threads,
                                          "2p" if inst.two else "1p", "-prof" if inst.prof else "", inst.bits, inst.build)


_TYPES = {"short": "int16", "int": "int32", "unsigned short": "uint16"}
_SYM = re.compile(r"sr_s(\d)::(\w+)::(?:__device_stub__)?sr_align_(blk|bfs)_kernel<([^>]*)>")


def instances_in_symbols(text: str):
    """set of Instance named by demangled kernel symbols (one per line, `nm -C` output)"""
    out = set()
    for m in _SYM.finditer(text):
        bits, build, fam = int(m.group(1)), m.group(2), m.group(3)
        a = [t.strip() for t in m.group(4).split(",")]
        ot, nt, two = _TYPES[a[0]], int(a[1]), a[2] == "true"
        if fam == "bfs":
            out.add(Instance("bfs", 1, ot, ot, nt, two, False, bits, build))
        else:
            # <OT, NT, TWO, B, E1, E2, PROF, X, OE1, RT>
            out.add(Instance("blk", int(a[3]), ot, _TYPES[a[9]], nt, two, a[6] == "true", bits, build))
    return out


# ------------------------------------------------------------------------------------------ penalty lattice
# name -> (scores, kernel 'blk' | 'bfs' | 'refused', block levels, lazy I/D rows, wide level kernel)
LATTICE = {
    "2nd-15": ("0,5,8,2,14,1", "blk", 10, 1, False),
    "2nd-20": ("0,5,8,2,19,1", "blk", 10, 1, False),
    "2nd-10": ("0,5,8,2,9,1", "blk", 10, 1, False),
    "2nd-25": ("0,5,8,2,24,1", "blk", 10, 1, False),
    "2nd-14": ("0,5,8,2,13,1", "blk", 5, 1, False),
    "2nd-16": ("0,5,8,2,15,1", "blk", 5, 1, False),
    "2nd-30": ("0,5,8,2,29,1", "blk", 5, 1, False),
    "2nd-9": ("0,5,8,2,8,1", "blk", 5, 1, False),
    "2nd-5": ("0,5,8,2,4,1", "blk", 5, 1, False),
    "2nd-4-dominates": ("0,5,8,2,3,1", "bfs", 1, 0, False),
    "1st-5-minimum": ("0,5,3,2", "blk", 5, 1, False),
    "x-4": ("0,4,8,2", "bfs", 1, 0, False),
    "1st-4": ("0,5,2,2", "bfs", 1, 0, False),
    "x-6": ("0,6,8,2", "blk", 5, 1, False),
    "1st-9": ("0,5,7,2", "blk", 5, 1, False),
    "1st-10-exact": ("0,5,8,2", "blk", 10, 1, False),
    "1st-11": ("0,5,9,2", "blk", 5, 1, False),
    "e1-1": ("0,5,9,1", "bfs", 1, 0, False),
    "e1-3": ("0,5,7,3", "bfs", 1, 0, False),
    "e2-2": ("0,5,8,2,24,2", "bfs", 1, 0, False),
    "lazy-on-33": ("0,5,8,2,32,1", "blk", 5, 1, False),
    "lazy-off-34": ("0,5,8,2,33,1", "blk", 5, 0, False),
    "depth-73": ("0,5,8,2,72,1", "blk", 5, 0, False),
    "depth-74": ("0,5,8,2,73,1", "bfs", 1, 0, True),
    # level kernel either side of its 32-level ring: scope + 1 = 32 and 33 (e2 = 2 keeps the blocked kernel out)
    "narrow-31": ("0,5,8,2,28,2", "bfs", 1, 0, False),
    "wide-32": ("0,5,8,2,29,2", "bfs", 1, 0, True),
    "scope-127": ("0,3,125,1", "bfs", 1, 0, True),
    "scope-128": ("0,3,126,1", "refused", 0, 0, False),
    "x-40": ("0,40,8,2", "blk", 5, 0, False),
    "unit-affine": ("0,1,1,1", "bfs", 1, 0, False),
    "unit-linear": ("0,1,0,1", "bfs", 1, 0, False),
    "open0": ("0,3,0,1", "bfs", 1, 0, False),
}
# orientation penalties -> (blocked alignment path kept, orientation route of the separate kernel)
ORI_LATTICE = {
    "0,1,1,1": (True, "orient-blk"),
    "0,1,0,1": (True, "orient-levels"),
    "0,2,1,1": (True, "orient-levels"),
    "0,1,2,1": (True, "orient-levels"),
    "0,1,2,2": (False, "in-kernel"),           # e1 != 1: no blocked path at all
    "0,1,77,1": (False, "in-kernel"),          # scope 79: two rows more than the blocked kernel's 80 slots hold
    "0,1,76,1": (True, "orient-levels"),       # scope 78: the last one that fits
}
NEW_EXACT = ("2nd-15", "2nd-20")


def crossover(pen: Pen):
    """smallest gap length at which the second piece is cheaper than the first (None: never)"""
    if not pen.two or pen.e2 >= pen.e1 and pen.o2 >= pen.o1:
        return None
    for l in range(1, 400):
        if pen.o2 + pen.e2 * l < pen.o1 + pen.e1 * l:
            return l
    return None


# ------------------------------------------------------------------------------------------ inputs
def family(seed, n=5, lo=1200, hi=2500, sub=0.02, indel=0.004):
    """n sequences of lo..hi bases from one base: substitutions, indels of 1..40, a truncated member and a
    reverse-complemented one"""
    rng = random.Random(seed)
    L = hi
    recs = synth.indel_family(n, L, sub, indel, 7000 + seed, max_indel=40)
    out = []
    for i, (name, s) in enumerate(recs):
        keep = rng.randrange(lo, min(hi, len(s)) + 1) if i else min(hi, len(s))
        a = rng.randrange(0, len(s) - keep + 1) if i == 1 else 0
        s = s[a:a + keep]
        if i == 1:
            s = s[: max(lo, len(s) - 300)]                         # truncated member
        if i == 2:
            s = synth.reverse_complement(s)
        out.append((name, s))
    return out


def lift(recs, bits, seed=0):
    """the same family in the 4-bit alphabet (N runs, soft-masked stretches) or the 8-bit one (more than 16 distinct
    bytes: IUPAC codes in both cases)"""
    if bits == 2:
        return recs
    rng = random.Random(1000 + seed)
    out = []
    for i, (name, s) in enumerate(recs):
        b = bytearray(s)
        for _ in range(3):                                         # N runs of 1..30
            p, l = rng.randrange(0, len(b) - 40), rng.randrange(1, 31)
            b[p:p + l] = b"N" * l
        if i % 2 == 0:                                             # soft-masked stretches
            for _ in range(2):
                p, l = rng.randrange(0, len(b) - 200), rng.randrange(20, 200)
                b[p:p + l] = bytes(b[p:p + l]).lower()
        if bits == 8 and i < 2:
            p = rng.randrange(0, len(b) - 40)
            b[p:p + 22] = b"RYSWKMBDHVNryswkmbdhvn"
        out.append((name, bytes(b)))
    return out


def symbol_bits(recs):
    """bits per symbol the host packs these records with"""
    comp = {ord("A"): ord("T"), ord("T"): ord("A"), ord("C"): ord("G"), ord("G"): ord("C"),
            ord("a"): ord("T"), ord("t"): ord("A"), ord("c"): ord("G"), ord("g"): ord("C")}
    seen = set()
    for _, s in recs:
        seen |= set(s)
    seen |= {comp.get(b, b) for b in seen}
    return 2 if seen <= set(b"ACGT") else 4 if len(seen) <= 16 else 8


def gap_runs(cigar: bytes):
    """lengths of the I and D runs of a raw CIGAR ('MXID' bytes)"""
    return [len(m.group(0)) for m in re.finditer(rb"I+|D+", cigar)]
