"""Shared data of the long-sequence seam tests (no tests here): a plain restatement of the length-dependent part of the
host's kernel plan (sr_host.cpp plan_kernel, align_static_lds and the orientation route of alloc_workspace; DESIGN.md
sections 3 and 4.1), the table of length seams per alphabet, and seeded two-sequence inputs whose longest member has
exactly a given length.

instance_matrix.dispatch restates which instance the penalties and the knobs select and declines every load whose LDS
copies leave the thread count to a tuning rule; plan() restates exactly that part -- everything that follows from the
longest sequence of a load.  test_long_seams_host.py holds the two against each other wherever both answer and holds the
seam table against plan(); test_long_seams_gpu.py holds plan() against the workspace report of every load it makes."""
import ctypes as C
import functools
from collections import namedtuple

import instance_matrix as im
from seqrush_amd import synth

# ------------------------------------------------------------------------------------------ limits the contract names
KB = 1024
LDS_PER_CU = 160 * KB                  # LDS of a CU: what workgroups per CU are counted against
STAGE_LIMIT = 130 * KB                 # three sequence copies must fit (srk_align_max_lds): the level kernel's staging
BLK_WINDOW = 128 * KB                  # the blocked kernel addresses its LDS window within the first 128 KB
BLK_STATIC = 28 * KB                   # ... and the admission test reserves this much of it for its static tables
ORIENT_LIMIT = 60 * KB                 # three copies of the orientation kernel's own staging
INT16_MAXLEN = im.INT16_MAXLEN
RING_U16_MAXLEN = im.RING_U16_MAXLEN
LDS_REFUSAL = "sequences too long to stage in LDS"
ROWS_REFUSAL = "sequences too long for the device row workspace"
SR_ERR_UNSUPPORTED = -6

Plan = namedtuple("Plan", "refused kernel_impl offset_bytes ring_cell_bytes symbol_bits threads_per_workgroup "
                          "workgroups_per_cu lds_dynamic_bytes orientation_route orientation_ring_bytes words")
# the categorical fields: what a seam may flip (lds_dynamic_bytes and orientation_ring_bytes follow the word count)
FLIP_FIELDS = ("refused", "kernel_impl", "offset_bytes", "ring_cell_bytes", "symbol_bits", "threads_per_workgroup",
               "workgroups_per_cu", "orientation_route")


def words_of(L, bits):
    """words of one staged copy of the longest sequence: its symbols, padded by two words"""
    per_word = 32 // bits
    return -(-L // per_word) + 2


def static_lds(impl, threads, wave=False):
    """the host's estimate of the alignment kernels' static LDS tables (align_static_lds)"""
    if wave:
        return 6 * KB
    if impl != 2:
        return 28 * KB
    return (34 if threads >= 1024 else 28 if threads >= 512 else 25) * KB


def plan(L, bits, npairs=4, cus=256, knobs=None, scores=im.DEFAULT_SCORES, ori_scores=im.DEFAULT_ORI) -> Plan:
    """what a load whose longest sequence has L symbols of `bits` bits runs, for one batch of npairs pairs on cus CUs.
    Workgroup builds only (no SR_ALIGN_THREADS of 64 or 128)."""
    knobs = knobs or {}
    pen, ori = im.parse_pen(scores), im.parse_pen(ori_scores)
    words = words_of(L, bits)
    off16 = L <= INT16_MAXLEN and "SR_FORCE_INT32" not in knobs
    osz = 2 if off16 else 4
    if words * 12 > STAGE_LIMIT:
        return Plan(LDS_REFUSAL, None, None, None, bits, None, None, None, None, None, words)
    block = im.blk_levels(pen, ori)
    impl = 2 if block > 0 and words * 16 + BLK_STATIC <= BLK_WINDOW else 1
    if "SR_ALIGN_IMPL" in knobs and int(knobs["SR_ALIGN_IMPL"]) <= 1:
        impl = 1
    lds = words * 16 + 16 if impl == 2 else words * 12       # four copies + read slack | three copies
    wg = max(1, int(knobs["SR_WG_PER_CU"])) if "SR_WG_PER_CU" in knobs else 4
    threads = 256
    if impl == 2 and npairs <= 2 * cus + cus // 2:
        threads = 512
    if impl == 2 and npairs <= cus:
        threads = 1024
    forced = int(knobs["SR_ALIGN_THREADS"]) if "SR_ALIGN_THREADS" in knobs else None
    assert forced in (None, 256, 512, 1024), "workgroup builds only"
    if forced in (256, 512) or (forced == 1024 and impl == 2):
        threads = forced
    if threads == 1024 and not (impl == 2 and block == 10 and off16 and bits == 2 and pen.two):
        threads = 512
    wg = min(wg, max(1, LDS_PER_CU // (lds + static_lds(impl, threads))))
    u16_ok = block == 10 and L <= RING_U16_MAXLEN and knobs.get("SR_RING_U16") != "0"
    # the tuning rule instance_matrix.dispatch declines: two workgroups per CU at most -> 512 threads
    if impl == 2 and wg <= 2 and forced is None and (off16 or u16_ok):
        threads = 512
    wg = min(wg, max(1, LDS_PER_CU // (lds + static_lds(impl, threads))))
    ring_u16 = impl == 2 and not off16 and u16_ok and threads >= 256
    if impl == 2 and not off16 and not ring_u16:
        threads = 256                                         # 32-bit searches on 32-bit rows: one workgroup build
    rsz = (2 if ring_u16 else osz) if impl == 2 else osz
    # orientation in front of the aligner
    po = knobs.get("SR_PREORIENT")
    auto = npairs >= 4 * cus and words * 12 <= 20 * KB
    pre = impl == 2 and (int(po) != 0 if po is not None else auto) and words * 12 <= ORIENT_LIMIT
    ori_blocked = (ori.x, ori.o1, ori.e1) == (1, 1, 1) and not ori.two and "SR_ORIENT_LEVELS" not in knobs
    route = ("orient-blk" if ori_blocked else "orient-levels") if pre else "in-kernel"
    oring = 0
    if pre:
        orow = (2 * ((2 * L + 32) & ~3) + 512 + 7) & ~7
        oring = min(npairs, cus * 16) * (((ori.scope + 1) * 3 + 1) * orow + 256) * osz
    return Plan(None, impl, osz, rsz, bits, threads, wg, lds, route, oring, words)


def plan_mismatches(rep: dict, kernel_name: str, p: Plan):
    """fields of a workspace report (and the context's kernel name) that differ from plan()"""
    want = dict(kernel_impl=p.kernel_impl, offset_bytes=p.offset_bytes, ring_cell_bytes=p.ring_cell_bytes,
                symbol_bits=p.symbol_bits, threads_per_workgroup=p.threads_per_workgroup,
                workgroups_per_cu=p.workgroups_per_cu, lds_dynamic_bytes=p.lds_dynamic_bytes,
                orientation_route=p.orientation_route, orientation_ring_bytes=p.orientation_ring_bytes)
    bad = {k: (rep.get(k), v) for k, v in want.items() if rep.get(k) != v}
    name = "sr_align_blk_kernel" if p.kernel_impl == 2 else "sr_align_bfs_kernel"
    if kernel_name != name:
        bad["align_kernel"] = (kernel_name, name)
    return bad


# ------------------------------------------------------------------------------------------ the seam table
# (name, bits, last length of the lower side, knobs the seam needs, the field the seam is about, the fields that follow
# from it at four pairs).  Derived from plan_kernel: every quantity counts words, so each alphabet has its own lengths.
Seam = namedtuple("Seam", "name bits L knobs field follows")
PRE = {"SR_PREORIENT": "1"}
SEAMS = [
    # int16 -> int32 offsets: same length in every alphabet (8-bit: already in the level kernel)
    Seam("off16", 2, 32000, {}, "offset_bytes", ()),
    Seam("off16", 4, 32000, {}, "offset_bytes", ()),
    Seam("off16", 8, 32000, {}, "offset_bytes", ("ring_cell_bytes",)),     # level kernel: its rows are offset-wide
    # 16-bit ring -> 32-bit ring of the 32-bit searches; the 32-bit rows have the 256-thread build only.  4-bit and 8-bit
    # inputs leave the blocked kernel before 57 000
    Seam("ring16", 2, 57000, {}, "ring_cell_bytes", ("threads_per_workgroup",)),
    # own orientation kernel allowed: words * 12 <= 60 KB
    Seam("orient", 2, 81888, PRE, "orientation_route", ()),
    Seam("orient", 4, 40944, PRE, "orientation_route", ()),
    Seam("orient", 8, 20472, PRE, "orientation_route", ()),
    # last blocked load / first level-per-pass load: words <= 6400.  The level kernel keeps offset-wide rows and runs 256
    # threads: 4-bit loads leave the 16-bit ring and 512 threads, 8-bit ones int16 rows at 512 threads
    Seam("blocked", 2, 102368, {}, "kernel_impl", ()),
    Seam("blocked", 4, 51184, {}, "kernel_impl", ("ring_cell_bytes", "threads_per_workgroup")),
    Seam("blocked", 8, 25592, {}, "kernel_impl", ("threads_per_workgroup",)),
    # last admitted / first refused: words * 12 <= 130 KB
    Seam("admitted", 2, 177456, {}, "refused", None),
    Seam("admitted", 4, 88728, {}, "refused", None),
    Seam("admitted", 8, 44364, {}, "refused", None),
]
LAST_BLOCKED = {2: 102368, 4: 51184, 8: 25592}
LEVEL_LENGTH = {2: 102369, 4: 51185, 8: 25593}          # one level-kernel length per alphabet for the reuse runs
FIRST_REFUSED = {2: 177457, 4: 88729, 8: 44365}


def rates(L):
    """substitution and indel rates scaled down with L so that the score stays near that of the 60 000-base pair of
    test_gpu_parity (about 2 400 at the default penalties): about 200 substitutions and 22 indels per sequence"""
    return 200.0 / L, 22.0 / L


Case = namedtuple("Case", "name seam bits L knobs rc ragged seed")


def _cases():
    """every admitted length on both sides of every seam, rc and ragged alternating; every alphabet's last-blocked length
    is there twice: reverse-complemented and ragged"""
    out = []
    k = 0
    for s in SEAMS:
        for L in (s.L, s.L + 1):
            if plan(L, s.bits, knobs=s.knobs).refused:
                continue
            rc, ragged = bool(k & 1), bool(k & 2)
            if s.name == "blocked" and L == s.L:
                rc, ragged = True, False
            out.append(Case("%s-s%d-%d%s%s" % (s.name, s.bits, L, "-rc" if rc else "", "-ragged" if ragged else ""),
                            s.name, s.bits, L, dict(s.knobs), rc, ragged, 8800 + k))
            k += 1
    for bits, L in sorted(LAST_BLOCKED.items()):
        out.append(Case("blocked-s%d-%d-ragged" % (bits, L), "blocked", bits, L, {}, False, True, 8900 + bits))
    return out


def oracle_rc(s: bytes) -> bytes:
    """reverse complement by the oracle's table (IUPAC codes and case included)"""
    import oracle_binding as ob
    buf = C.create_string_buffer(len(s))
    ob.lib().sro_reverse_complement(s, len(s), buf)
    return buf.raw


IUPAC = b"RYSWKMBDHVNryswkmbdhvn"


def _lift(s: bytes, bits: int) -> bytes:
    """a member in the 4-bit alphabet (N runs, soft-masked stretches) or the 8-bit one (more than 16 distinct bytes:
    IUPAC codes); non-ACGT bytes inside the first and the last word.  The same coordinates in both members, most of them
    in the first thirtieth of the sequence, where the indels have not shifted the members against each other yet: the
    alphabet costs a few mismatches, not a third of the score"""
    if bits == 2:
        return s
    b = bytearray(s)
    n = len(b)
    for p, l in ((n // 50, 5), (n // 40, 30), (n - 200, 11)):                  # N runs
        b[p:p + l] = b"N" * l
    for p, l in ((n // 60, 40), (n // 30, 150)):                               # soft-masked stretches
        b[p:p + l] = bytes(b[p:p + l]).lower()
    if bits == 8:
        p = n // 45
        b[p:p + len(IUPAC)] = IUPAC
        b[0:2] = b"RY"; b[n - 2:n] = b"KM"
    else:
        b[0:2] = b"Nn"; b[n - 2:n] = b"nN"
    return bytes(b)


@functools.lru_cache(maxsize=None)
def pair(L, bits, seed, rc=False, ragged=False):
    """two sequences whose longest is exactly L: members of one indel family, truncated (never padded).  ragged: the
    second member is 300 shorter; rc: it is reverse-complemented, so that the reverse-strand copy at the top of the LDS
    window is the one extended.  An indel lies within the last 64 bases in every alphabet"""
    sub, indel = rates(L)
    fam = synth.indel_family_fast(2, L + 256, sub, indel, seed)
    a, b = fam[0][1], fam[1][1]
    n2 = L - 300 if ragged else L
    assert len(a) >= L and len(b) >= n2 + 3, (len(a), len(b), L)
    a = a[:L]
    b = b[:n2 - 40] + b[n2 - 37:n2 + 3]                     # a 3-base deletion 40 bases before the end
    a, b = _lift(a, bits), _lift(b, bits)
    if rc:
        b = oracle_rc(b)
    assert len(a) == L and len(b) == n2
    return (("a", a), ("b", b))


def recs_of(case: Case):
    return list(pair(case.L, case.bits, case.seed, case.rc, case.ragged))


CASES = _cases()
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)


class OracleByPieces:
    """What test_gpu_parity.check_parity asks of an OracleSeqRush -- align_pair of the listed pairs, labels and GFA of
    their union, default parameters -- put together from the oracle's own pieces, computed once and shared unchanged.

    sro_align_pair scores the forward orientation without a bound before it looks at the reverse one; between a sequence
    and the reverse complement of its relative that is a search of O(L^2) cells: 18 s per pair at 102 368 bases.  The
    rule it decides is `reverse iff rev < fwd` (forward on ties).  Here the same rule is decided from the same function
    in the order that is cheap for the pair: where the second member was reverse-complemented, sro_wfa_score of the
    reverse orientation first and of the forward one up to that score (INT_MAX beyond it: rev < fwd); elsewhere as
    sro_align_pair does.  Then sro_wfa_align in the chosen orientation and sro_process_alignment in list order, as
    sro_align_and_unite does.  test_long_seams_host.py holds this against sro_align_pair / sro_align_and_unite
    themselves on every forward case and on the shortest reverse-complemented ones."""

    def __init__(self, recs, pairs=None, rev_first=False):
        import oracle_binding as ob
        o = ob.OracleSeqRush(records=recs)
        op = ob.default_params()
        n = len(recs)
        self.n = n
        order = pairs if pairs is not None else [(q, t) for q in range(n) for t in range(n)]
        self.pairs = {}
        for q, t in order:
            if (q, t) not in self.pairs:
                self.pairs[q, t] = self._align(ob, op, recs[q][1], recs[t][1], rev_first and q != t)
            a = self.pairs[q, t]
            assert o.process_alignment(ob.cigar_bytes_to_string(a["cigar"]), q, t, op.min_match_len, a["is_reverse"]) >= 0
        self.labels = o.canonical_labels()
        self.gfa_out = o.gfa(canonical=True)
        o.close()

    @staticmethod
    def _align(ob, op, qs, ts, rev_first):
        rc = oracle_rc(qs)
        if rev_first:
            rev = ob.wfa_score(rc, ts, op.ori)
            fwd = ob.wfa_score(qs, ts, op.ori, max_score=rev)
        else:
            fwd = ob.wfa_score(qs, ts, op.ori)
            rev = ob.wfa_score(rc, ts, op.ori, max_score=fwd - 1) if fwd > 0 else 2 ** 31 - 1
        is_rev = rev < fwd
        cig, score = ob.wfa_align(rc if is_rev else qs, ts, op.pen)
        return dict(is_reverse=is_rev, score=score, cigar=cig)

    def align_pair(self, op, q, t):
        return self.pairs[q, t]

    def align_and_unite(self, op):
        return None

    def canonical_labels(self):
        v = self.labels.view(); v.flags.writeable = False
        return v

    def gfa(self, canonical=True):
        assert canonical
        return self.gfa_out


@functools.lru_cache(maxsize=None)
def oracle_once(name):
    """the oracle's answers on a case, computed once and shared unchanged by every run of it"""
    case = CASE_BY_NAME[name]
    return OracleByPieces(recs_of(case), rev_first=case.rc)


def short_pair(bits, seed=77):
    """a 300-base pair in the same alphabet (for the explicit pair lists: a short pair inside a full-size window)"""
    fam = synth.indel_family_fast(2, 340, 0.03, 0.01, seed)
    a, b = fam[0][1][:300], fam[1][1][:300]
    assert len(a) == 300 and len(b) == 300
    if bits != 2:
        a = a[:100] + b"NNNN" + a[104:200] + a[200:260].lower() + a[260:]
        b = b[:100] + b"NNNN" + b[104:]
    return [("c", a), ("d", b)]


def op_counts(cigar: bytes):
    """(substitutions, indel runs) of a raw CIGAR"""
    return cigar.count(b"X"), len(im.gap_runs(cigar))


# ------------------------------------------------------------------------------------------ the built kernels' static LDS
def built_static_lds(lib_path):
    """{(family 'blk' | 'bfs', build, symbol bits, threads): bytes} -- static LDS (group segment) of every workgroup
    instance of the two alignment kernels, read from the kernel descriptors of the gfx950 code objects bundled in the
    built library (llvm-readelf --notes on each bundle entry)"""
    import os, re, shutil, struct, subprocess, tempfile
    tools = [shutil.which("llvm-readelf"), "/opt/rocm/llvm/bin/llvm-readelf", "/opt/rocm/lib/llvm/bin/llvm-readelf"]
    tool = next((t for t in tools if t and os.path.exists(t)), None)
    assert tool, "no llvm-readelf to read the kernel descriptors with"
    data = open(lib_path, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    sym = re.compile(r"_ZN5sr_s(\d)(\d)(\w+?)19sr_align_(blk|bfs)_kernelI[si]Li(\d+)E")
    out = {}
    pos = data.find(magic)
    with tempfile.TemporaryDirectory() as tmp:
        while pos >= 0:
            (entries,) = struct.unpack_from("<Q", data, pos + 24)
            o = pos + 32
            for _ in range(entries):
                off, size, tl = struct.unpack_from("<QQQ", data, o)
                triple = data[o + 24:o + 24 + tl].decode()
                o += 24 + tl
                if "gfx950" not in triple or not size:
                    continue
                fn = os.path.join(tmp, "co.elf")
                with open(fn, "wb") as f:
                    f.write(data[pos + off:pos + off + size])
                notes = subprocess.run([tool, "--notes", fn], capture_output=True, text=True, check=True).stdout
                for m in re.finditer(r"\.group_segment_fixed_size:\s*(\d+).*?\.name:\s*(\S+)", notes, re.S):
                    s = sym.match(m.group(2))
                    if s:
                        build = s.group(3)[:int(s.group(2))]
                        key = (s.group(4), build, int(s.group(1)), int(s.group(5)))
                        out[key] = max(out.get(key, 0), int(m.group(1)))
            pos = data.find(magic, pos + 1)
    return out
