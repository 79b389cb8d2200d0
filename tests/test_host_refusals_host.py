"""CPU test (-m "not gpu") that pins what the host runtime says when it refuses its arguments: the status code and the bytes
of sr_last_error(), against tests/golden/host_refusals.json.  The record was taken from the build before sr_host.cpp was cut
into its units (sr_params.cpp, sr_pairs.cpp, sr_host.cpp, sr_inv_host.cpp, sr_paf.cpp, sr_gfa_host.cpp, sr_twins.cpp) and the
device check, the scratch arena and the readback of a context's buffer became one helper each (sr_ctx.h), so it holds every
entry point that moved to the wording and to the order of the checks it had in the one file.

Every case is reachable without a device: the parsers, the pair-list rules, the host twins, the writers, and the argument
checks that the device entry points make before they ask for a device.  The device cases ask for device 0 on a machine
that has none (one of them with an argument defect behind the device check, which therefore is not the one reported);
where a HIP device is present they are skipped.

Not pinned, because it cannot be reached this way: "bad cigar_off" of the scan entry points (behind the device check), the
2^31-base limits of graph induction, and sr_ctx_download_labels(NULL), which reads the context before it checks it."""
import ctypes as C
import json
import os

import pytest

from seqrush_amd import _lib
from seqrush_amd._lib import AlignmentsC, InvSiteC, ParamsC, SeqSetC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "host_refusals.json")

u32, u64, i32 = C.c_uint32, C.c_uint64, C.c_int32
NOWHERE = b"/nonexistent-directory-of-the-refusal-test/out.paf"


def params(**kw):
    p = ParamsC()
    _lib.load().sr_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class P(dict):
    """the fields a case sets in the default parameters; made into a ParamsC when the case runs, so that importing this
    module does not load the library"""


def made(p):
    return params(**p) if isinstance(p, P) else p


def seqset(seqs=(b"ACGT", b"ACGA"), names=True):
    """a SeqSetC over the given sequences; the returned tuple keeps its buffers alive"""
    off = (u64 * (len(seqs) + 1))(0)
    for i, s in enumerate(seqs):
        off[i + 1] = off[i] + len(s)
    nm = (C.c_char_p * len(seqs))(*[b"s%d" % i for i in range(len(seqs))])
    ss = SeqSetC(len(seqs), b"".join(seqs) or b"A", off, nm if names else None)
    return ss, off, nm


def arr(t, *v):
    return (t * len(v))(*v)


# ---- out arguments: every case gets fresh ones
def outs():
    class O:
        pu32a, pu32b, pu32c, pu32d = (C.POINTER(u32)() for _ in range(4))
        n1, n2 = u64(), u64()
        sites, owner, cost = C.POINTER(InvSiteC)(), C.POINTER(u64)(), C.POINTER(i32)()
        sketch, sel, text = C.POINTER(u64)(), C.POINTER(C.c_uint8)(), C.c_void_p()
        ctx = C.c_void_p()
    return O


def _parse(fn, text):
    return lambda L, o: getattr(L, fn)(text, C.byref(params()))


def _pair_list(n, p, q=True, t=True, count=True):
    return lambda L, o: L.sr_pair_list(n, C.byref(made(p)) if p is not None else None, C.byref(o.pu32a) if q else None,
                                       C.byref(o.pu32b) if t else None, C.byref(o.n1) if count else None)


def _iter_lists(p, last=True):
    return lambda L, o: L.sr_iterative_pair_lists(4, None, C.byref(made(p)) if p is not None else None, C.byref(o.pu32a), C.byref(o.pu32b),
                                                  C.byref(o.n1), C.byref(o.pu32c), C.byref(o.pu32d), C.byref(o.n2) if last else None)


def _mirror(q, t, count, batch_first, nbatch):
    return lambda L, o: L.sr_mirror_map(q, t, count, batch_first, nbatch, 0, arr(u32, 0, 0, 0, 0), C.byref(o.n1))


OPS = arr(u32, (8 << 4) | 0, (40 << 4) | 2, (8 << 4) | 0)      # 8= 40I 8=
OFF = arr(u64, 0, 3)


def _scan(ops=OPS, off=OFF, n=1, min_size=16, sites=True, device=0):
    return lambda L, o: L.sr_inversion_scan_device(device, ops, off, n, min_size, C.byref(o.sites) if sites else None,
                                                   C.byref(o.owner), C.byref(o.n1))


def _scan_join(ops=OPS, off=OFF, n=1, min_size=16, join=4, pen="default", cost=True, device=0):
    p = P() if pen == "default" else pen
    return lambda L, o: L.sr_inversion_scan_device_join(device, ops, off, n, min_size, join, C.byref(made(p)) if p is not None else None, None, None,
                                                        C.byref(o.sites), C.byref(o.owner), C.byref(o.cost) if cost else None,
                                                        C.byref(o.n1), None)


def _sites_join(ops=OPS, n_ops=3, min_size=16, join=4, pen="default", count=True):
    p = P() if pen == "default" else pen
    return lambda L, o: L.sr_inversion_sites_host_join(ops, n_ops, min_size, join, C.byref(made(p)) if p is not None else None, C.byref(o.sites),
                                                       C.byref(o.cost), C.byref(o.n1) if count else None)


def _sketch(seqs=(b"ACGTACGT", b"ACGAACGA"), kmer=4, null_seqs=False, null_out=False, device=0):
    def run(L, o):
        keep = seqset(seqs)
        return L.sr_sketch_device(device, None if null_seqs else C.byref(keep[0]), kmer, None if null_out else C.byref(o.sketch),
                                  C.byref(o.pu32a), C.byref(o.pu32b), C.byref(o.pu32c))
    return run


def _knn(n=2, shared=True, device=0):
    m = arr(u32, 1, 1, 1, 1)
    return lambda L, o: L.sr_knn_select_device(device, m if shared else None, m, n, 1, 1, C.byref(o.sel))


def _gfa(fn, seqs=True, labels=True, names=True, text=True, compact=None, label0=0):
    def run(L, o):
        keep = seqset((b"AC", b"AC"), names)
        lab = arr(u64, label0, 1, 2, 3, 0, 1, 2, 3, 8, 9)
        a = [C.byref(keep[0]) if seqs else None, lab if labels else None]
        if compact is not None:
            a.append(compact)
        return getattr(L, fn)(*a, C.byref(o.text) if text else None, C.byref(o.n1), C.byref(o.n2))
    return run


def _alignments():
    """one alignment (0, 1) of 4 matches; the returned tuple keeps its arrays alive"""
    k = (arr(u32, 0), arr(u32, 1), arr(C.c_uint8, 0), arr(i32, 0), arr(u64, 0), arr(u64, 4), arr(u64, 0), arr(u64, 4),
         arr(u64, 0, 1), arr(u32, 4 << 4))
    return AlignmentsC(1, *k), k


def _paf(fn="sr_write_paf", a=True, seqs=True, path=NOWHERE, names=True):
    def run(L, o):
        al, keep = _alignments()
        ss = seqset(names=names)
        args = [C.byref(al) if a else None, C.byref(ss[0]) if seqs else None, path]
        if fn == "sr_append_paf_tagged":
            args.append(b"sr:Z:inv")
        return getattr(L, fn)(*args)
    return run


def _nodes(fn, *a):
    return lambda L, o: getattr(L, fn)(*a)


SCORES = {"too_few": b"0,4,6", "too_many": b"0,4,6,2,24,1,7", "match": b"x,4,6,2", "mismatch": b"0,x,6,2", "gap1_open": b"0,4,x,2",
          "gap1_extend": b"0,4,6,x", "gap2_open": b"0,4,6,2,x,1", "gap2_extend": b"0,4,6,2,24,x", "empty_field": b",4,6,2",
          "sign_only": b"0,4,6,+", "overflow": b"0,4,6,99999999999", "long_field": b"0,4,6,0000000000000001", "empty": b""}
ORI = {"too_few": b"0,1,1", "too_many": b"0,1,1,1,1", "not_a_number": b"0,x,1,1", "overflow": b"0,1,1,-99999999999"}
SPARSE = {"random_not_a_number": b"random:x", "random_zero": b"random:0", "random_above_one": b"random:1.5", "random_hex": b"random:0x1p-1",
          "connectivity_not_a_number": b"connectivity:", "connectivity_zero": b"connectivity:0.0", "connectivity_above_one": b"connectivity:2",
          "tree_no_values": b"tree:", "tree_too_many": b"tree:1,2,0.5,16,3", "tree_neighbor": b"tree:x", "tree_neighbor_overflow": b"tree:99999999999999999999",
          "tree_stranger": b"tree:1,-2", "tree_random_not_a_number": b"tree:1,2,x", "tree_random_out_of_range": b"tree:1,2,1.5",
          "tree_kmer": b"tree:1,2,0.5,x", "tree_kmer_zero": b"tree:1,2,0.5,0", "unknown_word": b"bogus", "plain_above_one": b"2.0",
          "plain_zero": b"0", "leading_space": b" 0.5", "hex_float": b"0x1p-1"}

# name -> a call (library, out arguments) -> status; none of them needs a device
DEFECTS = {f"parse_scores/{k}": _parse("sr_parse_scores", v) for k, v in SCORES.items()}
DEFECTS.update({f"parse_orientation_scores/{k}": _parse("sr_parse_orientation_scores", v) for k, v in ORI.items()})
DEFECTS.update({f"parse_sparsification/{k}": _parse("sr_parse_sparsification", v) for k, v in SPARSE.items()})
DEFECTS.update({
    "pair_list/null_params": _pair_list(4, None),
    "pair_list/null_query_out": _pair_list(4, P(), q=False),
    "pair_list/null_count": _pair_list(4, P(), count=False),
    "pair_list/no_shards": _pair_list(4, P(shard_count=0)),
    "pair_list/rank_beyond_count": _pair_list(4, P(shard_rank=2, shard_count=2)),
    "pair_list/tree": _pair_list(4, P(sparsify_kind=4)),
    "pair_list/too_many_pairs": _pair_list(70000, P()),
    "pair_list/bad_shard_before_tree": _pair_list(4, P(sparsify_kind=4, shard_count=0)),
    "iterative_pair_lists/null_params": _iter_lists(None),
    "iterative_pair_lists/null_count": _iter_lists(P(), last=False),
    "mirror_map/null_query": _mirror(None, arr(u32, 1, 0), 2, None, 0),
    "mirror_map/too_many_pairs": _mirror(arr(u32, 0, 1), arr(u32, 1, 0), 0xfffffff1, None, 0),
    "mirror_map/no_batches": _mirror(arr(u32, 0, 1), arr(u32, 1, 0), 2, arr(u32, 0, 2), 0),
    "mirror_map/first_batch_not_at_zero": _mirror(arr(u32, 0, 1), arr(u32, 1, 0), 2, arr(u32, 1, 2), 1),
    "mirror_map/last_batch_short": _mirror(arr(u32, 0, 1), arr(u32, 1, 0), 2, arr(u32, 0, 1), 1),
    "mirror_map/batches_go_back": _mirror(arr(u32, 0, 1, 0, 1), arr(u32, 1, 0, 1, 0), 4, arr(u32, 0, 3, 2, 4), 3),
    "inversion_scan_device/null_sites": _scan(sites=False),
    "inversion_scan_device/null_cigar_off": _scan(off=None),
    "inversion_scan_device/null_ops": _scan(ops=None),
    "inversion_scan_device/zero_threshold": _scan(min_size=0),
    "inversion_scan_device/zero_count": _scan(n=0),
    "inversion_scan_device/count_above_2_31": _scan(n=0x80000000),
    "inversion_scan_device/zero_threshold_before_zero_count": _scan(min_size=0, n=0),
    "inversion_scan_device_join/null_cost": _scan_join(cost=False),
    "inversion_scan_device_join/join_zero": _scan_join(join=0),
    "inversion_scan_device_join/join_above_threshold": _scan_join(join=17),
    "inversion_scan_device_join/zero_threshold": _scan_join(min_size=0, join=1),
    "inversion_scan_device_join/null_penalties": _scan_join(pen=None),
    "inversion_scan_device_join/match_score": _scan_join(pen=P(match_score=2)),
    "inversion_scan_device_join/null_cigar_off": _scan_join(off=None),
    "inversion_scan_device_join/zero_count": _scan_join(n=0),
    "inversion_sites_host/null_sites": lambda L, o: L.sr_inversion_sites_host(OPS, 3, 16, None, C.byref(o.n1)),
    "inversion_sites_host/null_ops": lambda L, o: L.sr_inversion_sites_host(None, 3, 16, C.byref(o.sites), C.byref(o.n1)),
    "inversion_sites_host/zero_threshold": lambda L, o: L.sr_inversion_sites_host(OPS, 3, 0, C.byref(o.sites), C.byref(o.n1)),
    "inversion_candidate/zero_threshold": lambda L, o: L.sr_inversion_candidate(40, 40, 0),
    "inversion_sites_host_join/null_count": _sites_join(count=False),
    "inversion_sites_host_join/zero_threshold": _sites_join(min_size=0),
    "inversion_sites_host_join/join_zero": _sites_join(join=0),
    "inversion_sites_host_join/join_above_threshold": _sites_join(join=17),
    "inversion_sites_host_join/null_penalties": _sites_join(pen=None),
    "inversion_sites_host_join/match_score": _sites_join(pen=P(match_score=2)),
    "inversion_sites_host_join/mismatch_zero": _sites_join(pen=P(mismatch_penalty=0)),
    "inversion_sites_host_join/gap_open_negative": _sites_join(pen=P(gap_open1=-1)),
    "inversion_sites_host_join/gap_extend_zero": _sites_join(pen=P(gap_ext1=0)),
    "inversion_sites_host_join/gap2_extend_zero": _sites_join(pen=P(gap_ext2=0)),
    "inversion_sites_host_join/scope_above_127": _sites_join(pen=P(mismatch_penalty=200)),
    "inversion_sites_host_join/gap2_scope_above_127": _sites_join(pen=P(gap_open2=200)),
    "sketch_device/null_seqs": _sketch(null_seqs=True),
    "sketch_device/null_out": _sketch(null_out=True),
    "sketch_device/no_sequences": _sketch(seqs=()),
    "sketch_device/kmer_0": _sketch(kmer=0),
    "sketch_device/kmer_33": _sketch(kmer=33),
    "sketch_device/empty_sequence": _sketch(seqs=(b"ACGT", b"", b"ACGA")),
    "sketch_device/kmer_before_empty_sequence": _sketch(seqs=(b"ACGT", b""), kmer=0),
    "knn_select_device/null_shared": _knn(shared=False),
    "knn_select_device/n_0": _knn(n=0),
    "build_gfa/null_seqs": _gfa("sr_build_gfa", seqs=False),
    "build_gfa/null_labels": _gfa("sr_build_gfa", labels=False),
    "build_gfa/null_text": _gfa("sr_build_gfa", text=False),
    "build_gfa/no_names": _gfa("sr_build_gfa", names=False),
    "build_gfa/label_out_of_range": _gfa("sr_build_gfa", label0=10),
    "build_gfa_opts/null_labels": _gfa("sr_build_gfa_opts", labels=False, compact=1),
    "build_gfa_opts/compact_on_device": _gfa("sr_build_gfa_opts", compact=2),
    "build_gfa_from_nodes/null_nodes": _gfa("sr_build_gfa_from_nodes", labels=False, compact=0),
    "build_gfa_from_nodes/no_names": _gfa("sr_build_gfa_from_nodes", names=False, compact=0),
    "ctx_build_gfa/null_text": lambda L, o: L.sr_ctx_build_gfa(None, None, None, C.byref(o.n1), C.byref(o.n2)),
    "ctx_build_gfa/null_ctx": lambda L, o: L.sr_ctx_build_gfa(None, None, C.byref(o.text), C.byref(o.n1), C.byref(o.n2)),
    "write_paf/null_alignments": _paf(a=False),
    "write_paf/null_seqs": _paf(seqs=False),
    "write_paf/null_path": _paf(path=None),
    "write_paf/no_names": _paf(names=False),
    "write_paf/unwritable_path": _paf(),
    "append_paf_tagged/unwritable_path": _paf("sr_append_paf_tagged"),
    "uf_init_host/short_array": _nodes("sr_uf_init_host", arr(u64, 0, 1, 2, 3), 4, 2),
    "uf_unite_host/out_of_range": _nodes("sr_uf_unite_host", arr(u64, 0, 1, 2, 3), 4, 1, 4),
    "uf_merge_labels_host/null_labels": _nodes("sr_uf_merge_labels_host", arr(u64, 0, 1, 2, 3), 4, None, 1),
    "uf_merge_labels_host/label_out_of_range": _nodes("sr_uf_merge_labels_host", arr(u64, 0, 1, 2, 3), 4, arr(u64, 0, 1, 9, 3), 1),
    "uf_count_components_host/short_array": lambda L, o: L.sr_uf_count_components_host(arr(u64, 0, 1, 2, 3), 4, 3, C.byref(o.n1)),
    "uf_canonical_labels_host/null_out": _nodes("sr_uf_canonical_labels_host", arr(u64, 0, 1, 2, 3), 4, None),
    "iterative_stop_host/null_counts": lambda L, o: L.sr_iterative_stop_host(None, 3, 10, C.byref(o.n1)),
    # a context that is not there: the sentence of each entry point, the readback accessors among them
    "ctx/set_stream": lambda L, o: L.sr_ctx_set_stream(None, None),
    "ctx/sync": lambda L, o: L.sr_ctx_sync(None),
    "ctx/load": lambda L, o: L.sr_ctx_load(None, None, None),
    "ctx/load_pairs_null_list": lambda L, o: L.sr_ctx_load_pairs(None, None, None, None, None, 3),
    "ctx/load_paf": lambda L, o: L.sr_ctx_load_paf(None, None, None, None),
    "ctx/load_iterative": lambda L, o: L.sr_ctx_load_iterative(None, None, None, 0),
    "ctx/run_iterative": lambda L, o: L.sr_ctx_run_iterative(None),
    "ctx/align": lambda L, o: L.sr_ctx_align(None),
    "ctx/unite": lambda L, o: L.sr_ctx_unite(None),
    "ctx/run": lambda L, o: L.sr_ctx_run(None),
    "ctx/reset_uf": lambda L, o: L.sr_ctx_reset_uf(None),
    "ctx/pairs": lambda L, o: L.sr_ctx_pairs(None, C.byref(o.pu32a), C.byref(o.pu32b), C.byref(o.n1)),
    "ctx/kernel_ms": lambda L, o: L.sr_ctx_kernel_ms(None, 0, C.byref(C.c_float())),
    "ctx/counters": lambda L, o: L.sr_ctx_counters(None, arr(u64, *[0] * 16)),
    "ctx/counters_ext": lambda L, o: L.sr_ctx_counters_ext(None, arr(u64, *[0] * 32)),
    "ctx/counters_all": lambda L, o: L.sr_ctx_counters_all(None, arr(u64, *[0] * 64), 64),
    "ctx/tail_deferred": lambda L, o: L.sr_ctx_tail_deferred(None, C.byref(o.n1)),
    "ctx/tail_timeline": lambda L, o: L.sr_ctx_tail_timeline(None, arr(u64, 0, 0, 0, 0), 1),
    "ctx/prio_timeline": lambda L, o: L.sr_ctx_prio_timeline(None, arr(u64, 0, 0, 0, 0), 1),
    "ctx/download_uf": lambda L, o: L.sr_ctx_download_uf(None, arr(u64, 0)),
    "ctx/orientation_scores": lambda L, o: L.sr_ctx_orientation_scores(None, None, None),
    "ctx/labels_device": lambda L, o: L.sr_ctx_labels_device(None, None),
    "ctx/merge_labels_host": lambda L, o: L.sr_ctx_merge_labels_host(None, None, 0),
    "ctx/alignments": lambda L, o: L.sr_ctx_alignments(None, None),
    "ctx/pair_results": lambda L, o: L.sr_ctx_pair_results(None, None, None, None),
    "ctx/align_all": lambda L, o: L.sr_ctx_align_all(None, 0, None),
    "ctx/enable_inversions": lambda L, o: L.sr_ctx_enable_inversions(None, None),
    "ctx/inversion_stats": lambda L, o: L.sr_ctx_inversion_stats(None, None),
    "ctx/inversion_join_stats": lambda L, o: L.sr_ctx_inversion_join_stats(None, None),
    "ctx/inversion_jobs": lambda L, o: L.sr_ctx_inversion_jobs(None, None, None),
    "ctx/inversion_alignments": lambda L, o: L.sr_ctx_inversion_alignments(None, None),
    "ctx/iterative_stats": lambda L, o: L.sr_ctx_iterative_stats(None, None, None, 0),
    "ctx/iterative_alignments": lambda L, o: L.sr_ctx_iterative_alignments(None, None),
    "align_all/null_seqs": lambda L, o: L.sr_align_all(None, None, None),
    "align_and_unite/null_seqs": lambda L, o: L.sr_align_and_unite(None, None, None),
    "unite_paf/null_path": lambda L, o: L.sr_unite_paf(None, None, None, None),
})


def _one_call(fn):
    """sr_align_all, sr_align_and_unite, sr_unite_paf: a context of their own on the device of the parameters"""
    def run(L, o):
        keep = seqset()
        p, al, parent = params(), C.POINTER(AlignmentsC)(), arr(u64, *[0] * 18)
        if fn == "sr_align_all":
            return L.sr_align_all(C.byref(keep[0]), C.byref(p), C.byref(al))
        if fn == "sr_align_and_unite":
            return L.sr_align_and_unite(C.byref(keep[0]), C.byref(p), parent)
        return L.sr_unite_paf(C.byref(keep[0]), C.byref(p), NOWHERE, parent)
    return run


# device 0 on a machine without a device
NO_DEVICE = {
    "ctx_create/no_device": lambda L, o: L.sr_ctx_create(0, C.byref(o.ctx)),
    "align_all/no_device": _one_call("sr_align_all"),
    "align_and_unite/no_device": _one_call("sr_align_and_unite"),
    "unite_paf/no_device": _one_call("sr_unite_paf"),
    "inversion_scan_device/no_device": _scan(),
    "inversion_scan_device/no_device_before_bad_cigar_off": _scan(off=arr(u64, 3, 0)),
    "inversion_scan_device_join/no_device": _scan_join(),
    "sketch_device/no_device": _sketch(),
    "knn_select_device/no_device": _knn(),
}


def observe(call):
    """[status, the bytes of sr_last_error() as text]"""
    L = _lib.load()
    return [call(L, outs()), L.sr_last_error().decode("latin-1")]


def record():
    """the content of the golden file (json.dump(record(), ..., indent=1, sort_keys=True)), as it was taken from the build
    before the split: the defects on any machine, the device cases on a machine without a device"""
    out = {name: observe(call) for name, call in DEFECTS.items()}
    if _lib.load().sr_device_count() == 0:
        out.update({name: observe(call) for name, call in NO_DEVICE.items()})
    return out


def _golden():
    return json.load(open(GOLDEN))


def test_the_record_holds_every_case():
    g = _golden()
    assert set(g) == set(DEFECTS) | set(NO_DEVICE)
    assert all(v[0] < 0 and v[1] for v in g.values()), "every case is a refusal with a sentence"
    assert all(g[k] == [-2, "no HIP device available (seqrush_amd has no CPU fallback)"] for k in NO_DEVICE)


@pytest.mark.parametrize("name", sorted(DEFECTS))
def test_a_defect_is_refused_as_recorded(name):
    assert observe(DEFECTS[name]) == _golden()[name]


@pytest.mark.parametrize("name", sorted(NO_DEVICE))
def test_no_device_is_refused_as_recorded(name):
    if _lib.load().sr_device_count() > 0:
        pytest.skip("a HIP device is present: device 0 is not refused")
    assert observe(NO_DEVICE[name]) == _golden()[name]
