"""--inversion-join: inputs, the joined scan with site costs and the whole joined mode restated in Python over the oracle,
in the style of inversion_helpers.restate (same alignments, same job construction and starts; the scan and the accept test
are the joined ones).  Test infrastructure only."""
import ctypes as C
import functools

import inversion_helpers as ih
import oracle_binding as ob
from seqrush_amd import synth

DEFAULT = "0,5,8,2,24,1"
SWEEP_LENGTHS = (100, 104, 108, 110, 112, 116, 120)
SWEEP_SEEDS = tuple(range(10))
# one sweep input on which the plain rule finds no job and the joined rule an accepted one (test_inversion_join_host checks
# both properties on the oracle): seed 0 -> base_sequence(500, 7000), 104 bp inverted at 200
PICK_SEED, PICK_L = 0, 104


def penalties(scores=DEFAULT):
    r, pen = ob.parse_scores(scores)
    assert r == 0
    return pen


def op_cost(op, ln, pen):
    """what the main alignment paid for one run-length op: X len x; a gap run the cheaper of the two pieces; a match 0"""
    if op == 0:
        return 0
    if op == 1:
        return ln * pen.mismatch
    c = pen.gap_open1 + ln * pen.gap_ext1
    if pen.gap_open2 >= 0:
        c = min(c, pen.gap_open2 + ln * pen.gap_ext2)
    return c


def cigar_cost(ops, pen):
    return sum(op_cost(o & 15, o >> 4, pen) for o in ops)


def scan(ops, m, j, pen):
    """the joined rule, written from the issue's text: -> [(qa, qgap, ta, tgap, kind, candidate, cost, islands)] in CIGAR
    order.  An anchor is a match op of at least j columns; a shorter one is an island and counts on both sides."""
    assert m > 0 and 1 <= j <= m
    sites, q, t = [], 0, 0
    anchor = lambda o: (o & 15) == 0 and (o >> 4) >= j          # noqa: E731
    for i, o in enumerate(ops):
        op, ln = o & 15, o >> 4
        if anchor(o):
            qg = tg = cost = isl = 0
            for o2 in ops[i + 1:]:
                if anchor(o2):
                    break
                p2, l2 = o2 & 15, o2 >> 4
                if p2 in (0, 1, 2):
                    qg += l2
                if p2 in (0, 1, 3):
                    tg += l2
                cost += op_cost(p2, l2, pen)
                isl += p2 == 0
            kind = ih.DIVERGENT if qg >= m and tg >= m else ih.QUERY_ONLY if qg >= m else ih.TARGET_ONLY if tg >= m else 0
            if kind:
                sites.append((q + ln, qg, t + ln, tg, kind, kind == ih.DIVERGENT and 2 * max(qg, tg) <= 3 * min(qg, tg), cost, isl))
        if op in (0, 1, 2):
            q += ln
        if op in (0, 1, 3):
            t += ln
    return sites


def accept_site(patch_score, site_cost):
    return 0 <= patch_score < site_cost // 2


def sweep_pair(seed, length):
    a = synth.to_bytes(synth.base_sequence(500, 7000 + seed))
    return a, synth.invert_segment(a, 200, length)


@functools.lru_cache(maxsize=None)
def inputs(name):
    if name == "c5like":            # the last sequence is reverse-complemented: '-' main alignments
        return tuple(synth.config_c5_like(4, 3000))
    if name == "snp":               # SNP clusters: joined "candidates" that must all be rejected
        return tuple(synth.snp_family(4, 2000, 0.05, 7104))
    if name == "pick":              # like inversion_helpers.inputs("inv"), on the picked sweep input
        a, b = sweep_pair(PICK_SEED, PICK_L)
        return (("A", a), ("B", b), ("C", synth.reverse_complement(b)))
    if name == "pick_soft":         # N and lower case outside the inverted segment: 4-bit symbols
        a, b = sweep_pair(PICK_SEED, PICK_L)
        s = bytearray(a); s[20:24] = b"NNNN"; s[400:420] = bytes(s[400:420]).lower()
        s2 = bytearray(b); s2[60] = ord("N"); s2[430:436] = bytes(s2[430:436]).lower()
        return (("A", bytes(s)), ("B", bytes(s2)), ("C", synth.reverse_complement(bytes(s2))))
    if name == "pick_bytes":        # more than 16 distinct bytes: 8-bit symbols
        a, b = sweep_pair(PICK_SEED, PICK_L)
        s = bytearray(a); s[10:30] = b"RYKMSWBDHVNrykmswbdh"
        return (("A", bytes(s)), ("B", synth.invert_segment(bytes(s), 200, PICK_L)), ("C", b))
    return ih.inputs(name)


@functools.lru_cache(maxsize=None)
def restate(name, scores=DEFAULT, k=ih.K, d=None, min_size=0, join=8, patch=True):
    """the whole joined mode on the oracle -> dict(jobs, labels, gfa, nodes, islands...); jobs in pair order, then CIGAR
    order.  join = 0 with patch = True is the plain mode (inversion_helpers.scan and the main / 2 test)."""
    recs = list(inputs(name))
    o = ob.OracleSeqRush(records=recs)
    L = ob.lib()
    op = ih.oracle_params(scores, k, d)
    m = min_size or 2 * k
    n = o.n
    seqs = [o.seq(i)[1] for i in range(n)]
    jobs, mains, islands = [], [], 0
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
        ops = ih.raw_bytes_to_ops(a["cigar"])
        assert cigar_cost(ops, op.pen) == a["score"]
        found = scan(ops, m, join, op.pen) if join else [s + (0, 0) for s in ih.scan(ops, m)]
        for qa, qg, ta, tg, kind, cand, cost, isl in found:
            if not cand:
                continue
            islands += isl
            rc = C.create_string_buffer(qg)
            L.sro_reverse_complement(aq[qa:qa + qg], qg, rc)
            raw, sc = ob.wfa_align(rc.raw, seqs[t][ta:ta + tg], op.pen)
            fq = lq - qa - qg if a["is_reverse"] else qa
            by_score = accept_site(sc, cost) if join else 0 <= sc < a["score"] // 2
            by_div = d is None or sc <= L.sro_max_score_for_divergence(C.byref(op.pen), min(qg, tg), d)
            jobs.append(dict(pair=pi, query_idx=q, target_idx=t, query_start=fq, query_end=fq + qg, target_start=ta,
                             target_end=ta + tg, main_score=a["score"], patch_score=sc, is_reverse=int(not a["is_reverse"]),
                             accepted=int(by_score and by_div), by_score=by_score, by_div=by_div, site_cost=cost,
                             cigar=ob.cigar_bytes_to_string(raw), qa=qa, qgap=qg, ta=ta, tgap=tg,
                             by_main=0 <= sc < a["score"] // 2))
    for j in jobs:
        if j["accepted"]:
            lq = len(seqs[j["query_idx"]])
            assert o.process_alignment(j["cigar"], j["query_idx"], j["target_idx"], k, bool(j["is_reverse"]),
                                       qs=lq - j["qa"] - j["qgap"], ts=j["ta"]) >= 0
    gfa, nn, ne = o.gfa(canonical=True)
    return dict(jobs=jobs, labels=o.canonical_labels(), gfa=gfa, nodes=nn, seqs=seqs, mains=mains, islands=islands)
