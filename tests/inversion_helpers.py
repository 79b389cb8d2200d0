"""--patch-inversions: inputs, the scan and the whole mode restated in Python over the oracle as it stands
(sro_align_pair, the scan below, sro_reverse_complement + sro_wfa_align per job, sro_process_alignment with query_is_rc and
starts for the patches).  Test infrastructure only."""
import ctypes as C
import functools

import numpy as np

import oracle_binding as ob
from seqrush_amd import synth

DIVERGENT, QUERY_ONLY, TARGET_ONLY = 1, 2, 3
K = 8          # -k of the GPU inputs, so the threshold is 16


def letters_to_ops(cigar: str):
    """the reference's raw CIGAR letters (M / = match, X, I = target only, D = query only; src/cigar_analysis.rs:51-70) ->
    op array in the sr_alignments encoding ((len << 4) | 0 '=' 1 X 2 query only 3 target only)"""
    code = {"M": 0, "=": 0, "X": 1, "D": 2, "I": 3}
    out, n = [], 0
    for ch in cigar:
        if ch.isdigit():
            n = n * 10 + int(ch)
        else:
            out.append((max(n, 1) << 4) | code[ch])
            n = 0
    return out


def raw_bytes_to_ops(raw: bytes):
    """per-column raw WFA bytes (M X I D, I = target only) -> run-length ops in the sr_alignments encoding"""
    code = {ord("M"): 0, ord("X"): 1, ord("D"): 2, ord("I"): 3}
    out = []
    for b in raw:
        c = code[b]
        if out and (out[-1] & 15) == c:
            out[-1] += 16
        else:
            out.append(16 | c)
    return out


def scan(ops, m):
    """find_potential_inversion_sites + is_potential_inversion (src/cigar_analysis.rs:23-147), written from the issue's
    text: -> [(qa, qgap, ta, tgap, kind, candidate)] in CIGAR order"""
    assert m > 0
    sites, q, t = [], 0, 0
    for i, o in enumerate(ops):
        op, ln = o & 15, o >> 4
        if op == 0:
            qg = tg = 0
            for o2 in ops[i + 1:]:
                p2, l2 = o2 & 15, o2 >> 4
                if p2 == 0:
                    break
                if p2 in (1, 2):
                    qg += l2
                if p2 in (1, 3):
                    tg += l2
            kind = DIVERGENT if qg >= m and tg >= m else QUERY_ONLY if qg >= m else TARGET_ONLY if tg >= m else 0
            if kind:
                sites.append((q + ln, qg, t + ln, tg, kind, kind == DIVERGENT and 2 * max(qg, tg) <= 3 * min(qg, tg)))
        if op in (0, 1, 2):
            q += ln
        if op in (0, 1, 3):
            t += ln
    return sites


# ---------------------------------------------------------------- inputs
def _purine(s: bytes, start: int, length: int, seed: int) -> bytes:
    blk = bytes(b"AG"[int(c) & 1] for c in synth.base_sequence(length, seed))
    return s[:start] + blk + s[start + length:]


def _snps(s: bytes, start: int, length: int, every: int) -> bytes:
    nxt = {65: 67, 67: 71, 71: 84, 84: 65}
    b = bytearray(s)
    for i in range(start + 2, start + length, every):
        b[i] = nxt[b[i]]
    return bytes(b)


EXTRA = {}     # name -> generator of [(name, bytes)]: inputs that live in another module (mode_tie_inputs.py)


@functools.lru_cache(maxsize=None)
def inputs(name):
    if name in EXTRA:
        return tuple(EXTRA[name]())
    # (seed and length chosen so that the main alignment shows the inversion as ONE two-sided gap: on most inputs the few
    # bases that match by chance at the centre of an inverted segment split it into two one-sided gaps, which the rule skips)
    a = synth.to_bytes(synth.base_sequence(500, 7110))
    b = synth.invert_segment(a, 200, 120)
    if name == "inv":               # B = A with 120 bp inverted; C = rc(B): its main alignments are on '-'
        return (("A", a), ("B", b), ("C", synth.reverse_complement(b)))
    # The issue asks for random replacement bases.  Random ACGT against random ACGT always matches somewhere, WFA keeps those
    # islands, and an island is a match op that splits the gap into one-sided sites (see above).  So the constructed cases
    # use segments that CANNOT match: a purine-only (A / G) block against its own reverse complement (C / T only) or against
    # a run of C.  They stay on plain ACGT (2-bit symbols); N and lower case have their own inputs below.
    pa = _purine(a, 30, 100, 7201)
    pa = _purine(pa, 200, 120, 7202)
    pb = synth.invert_segment(pa, 200, 120)
    if name == "pinv":              # the inverted block shares no base with the original: one clean two-sided gap under any -S
        return (("A", pa), ("B", pb), ("C", synth.reverse_complement(pb)))
    if name == "rejected":          # D: the first purine block replaced by 100 C: a candidate, no better when patched
        return (("A", pa), ("B", pb), ("D", pa[:30] + b"C" * 100 + pa[130:]))
    if name == "ratio":             # E: the 120 bp purine block replaced by 60 C: two-sided but 2:1
        return (("A", pa), ("B", pb), ("E", pa[:200] + b"C" * 60 + pa[320:]))
    if name == "diverged":          # F: the inverted segment carries a SNP every 5 bp: accepted by score, not by -d 0.1
        return (("A", a), ("B", b), ("F", _snps(b, 200, 120, 5)))
    if name == "soft":              # N and lower case: 4-bit symbols
        s = bytearray(a); s[20:24] = b"NNNN"; s[400:420] = bytes(s[400:420]).lower()
        s2 = bytearray(b); s2[230:236] = bytes(s2[230:236]).lower(); s2[60] = ord("N")
        return (("A", bytes(s)), ("B", bytes(s2)), ("C", synth.reverse_complement(bytes(s2))))
    if name == "bytes":             # more than 16 distinct bytes: 8-bit symbols
        s = bytearray(a); s[10:30] = b"RYKMSWBDHVNrykmswbdh"
        return (("A", bytes(s)), ("B", synth.invert_segment(bytes(s), 200, 120)), ("C", b))
    if name == "none":              # no candidates
        return tuple(synth.snp_family(4, 400, 0.03, 7104))
    raise KeyError(name)


def oracle_params(scores="0,5,8,2,24,1", k=K, d=None):
    op = ob.default_params()
    r, pen = ob.parse_scores(scores)
    assert r == 0
    op.pen = pen; op.min_match_len = k; op.threads = 4
    op.max_divergence = -1.0 if d is None else d
    return op


@functools.lru_cache(maxsize=None)
def restate(name, scores="0,5,8,2,24,1", k=K, d=None, min_size=0, patch=True):
    """the whole mode on the oracle -> dict(jobs, labels, gfa, plain_labels...) ; jobs in pair order, then CIGAR order"""
    recs = list(inputs(name))
    o = ob.OracleSeqRush(records=recs)
    L = ob.lib()
    op = oracle_params(scores, k, d)
    m = min_size or 2 * k
    n = o.n
    seqs = [o.seq(i)[1] for i in range(n)]
    jobs, mains = [], []
    for pi, (q, t) in enumerate((q, t) for q in range(n) for t in range(n)):
        a = o.align_pair(op, q, t)
        lq, lt = len(seqs[q]), len(seqs[t])
        if d is not None and a["score"] > L.sro_max_score_for_divergence(C.byref(op.pen), min(lq, lt), d):
            continue                                    # dropped by -d: neither united nor scanned
        mains.append((q, t, a))
        assert o.process_alignment(ob.cigar_bytes_to_string(a["cigar"]), q, t, k, a["is_reverse"]) >= 0
        if not patch:
            continue
        aq = synth.reverse_complement(seqs[q]) if a["is_reverse"] else seqs[q]
        for qa, qg, ta, tg, kind, cand in scan(raw_bytes_to_ops(a["cigar"]), m):
            if not cand:
                continue
            rc = C.create_string_buffer(qg)
            L.sro_reverse_complement(aq[qa:qa + qg], qg, rc)
            raw, sc = ob.wfa_align(rc.raw, seqs[t][ta:ta + tg], op.pen)
            fq = lq - qa - qg if a["is_reverse"] else qa
            by_score = 0 <= sc < a["score"] // 2
            by_div = d is None or sc <= L.sro_max_score_for_divergence(C.byref(op.pen), min(qg, tg), d)
            jobs.append(dict(pair=pi, query_idx=q, target_idx=t, query_start=fq, query_end=fq + qg, target_start=ta,
                             target_end=ta + tg, main_score=a["score"], patch_score=sc, is_reverse=int(not a["is_reverse"]),
                             accepted=int(by_score and by_div), by_score=by_score, by_div=by_div,
                             cigar=ob.cigar_bytes_to_string(raw), qa=qa, qgap=qg, ta=ta, tgap=tg))
    for j in jobs:
        if j["accepted"]:
            # a '-' patch starts at len_q - qa - qgap in reverse-complement space, a '+' patch at the same forward offset
            lq = len(seqs[j["query_idx"]])
            assert o.process_alignment(j["cigar"], j["query_idx"], j["target_idx"], k, bool(j["is_reverse"]),
                                       qs=lq - j["qa"] - j["qgap"], ts=j["ta"]) >= 0
    gfa, nn, ne = o.gfa(canonical=True)
    return dict(jobs=jobs, labels=o.canonical_labels(), gfa=gfa, nodes=nn, oracle=o, seqs=seqs, mains=mains)
