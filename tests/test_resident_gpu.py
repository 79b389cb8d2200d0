"""The resident context on the MI355X (-m gpu) the way a long-running host drives it: on a
stream the caller owns (the null stream like bench.py, a non-blocking torch side stream like an embedding host), several
`reset_uf; run` steps without a host call between, many loads of different kinds on ONE context, two contexts interleaved, a
change of streams on a loaded context, and the device memory a context keeps over reloads.

Every comparison is exact: against the CPU oracle's answers of resident_inputs.py (computed once, asserted to discriminate by
test_resident_host.py), against the Python restatements the mode tests use (test_iterative_gpu.restate, inversion_helpers,
inversion_join_helpers, extend_inputs), or against a fresh context on its own stream.  The one margin is the memory test's,
measured inside that test from fresh contexts; test_device_memory_over_reloads prints both series, and DESIGN.md section 2
("Resident suite") records them."""
import numpy as np
import pytest
import torch

import extend_inputs as ei
import inversion_helpers as ih
import inversion_join_helpers as jh
import resident_inputs as ri
from conftest import canon_gfa
from seqrush_amd._lib import SeqRushError
from seqrush_amd.seqrush import Context, ExtendPlan, Params, SeqSet, SortParams, sort_gfa
from test_inversions_gpu import JOB_KEYS

pytestmark = pytest.mark.gpu

REGIMES = ("own", "null", "side")
STEPS = 3
JOIN = 8
INV_STATS = ("scanned", "sites", "candidates", "accepted", "rejected_score", "rejected_divergence", "united_bases", "patch_batches")
EXT_STATS = ("old_paths", "old_bases", "old_steps", "new_sequences", "pairs_before", "pairs_after", "unions_attempted", "unions_joined")
FREE_KEY = "device_free_bytes_at_load"


def set_knobs(mp, env):
    for k in ri.KNOBS:
        mp.delenv(k, raising=False)
    for k, v in env.items():
        mp.setenv(k, v)


def on_stream(ctx, regime):
    """-> the torch stream object to keep alive (None: none)"""
    if regime == "null":
        ctx.set_stream(0)
    elif regime == "side":
        s = torch.cuda.Stream()
        ctx.set_stream(s.cuda_stream)
        return s
    return None


def report(ctx):
    rep = ctx.workspace_report()
    rep.pop(FREE_KEY, None)
    return rep


def cigars(al):
    out = dict(cigar=[al.cigar(i) for i in range(al.n)], score=al.score.copy(), is_reverse=al.is_reverse.copy(),
               pairs=list(zip(al.query_idx.tolist(), al.target_idx.tolist())))
    al.close()
    return out


def same(a, b, path=""):
    """exact equality of two result trees (dicts, lists, arrays, scalars)"""
    assert type(a) is type(b), path
    if isinstance(a, dict):
        assert a.keys() == b.keys(), path
        for k in a:
            same(a[k], b[k], f"{path}/{k}")
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and np.array_equal(a, b), path
    elif isinstance(a, (list, tuple)) and a and isinstance(a[0], (dict, np.ndarray)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, f"{path}[{i}]")
    else:
        assert a == b, path


# ------------------------------------------------------------------ one load kind: load, steps, collect, verify
class Kind:
    """name: an input of resident_inputs (oracle(name)); load(ctx, tmp) loads it (knobs already set), step(ctx) enqueues one
    step, collect(ctx) reads everything back after a sync, verify(got) compares with the oracle or restatement"""
    env = {}

    def load(self, ctx, tmp):
        raise NotImplementedError

    def step(self, ctx):
        ctx.reset_uf()
        ctx.run()


class Plain(Kind):
    """sr_ctx_load + sr_ctx_run: A (blocked kernel, every optional buffer, batches) and B (level-per-pass kernel, 4-bit symbols)"""

    def __init__(self, name):
        self.name = name
        self.env = ri.A_ENV if name == "A" else {}
        self.kw = ri.B_KW if name == "B" else {}

    def load(self, ctx, tmp):
        ctx.load(SeqSet(ri.oracle(self.name)["recs"]), Params(**self.kw))
        rep = ctx.workspace_report()
        if self.name == "A":
            assert rep["kernel_impl"] == 2 and rep["mirror_partners"] > 0 and rep["tail_threads"] > 0
            assert rep["orientation_route"] != "in-kernel" and rep["batches"] >= 3 and ctx.num_batches == rep["batches"]
            assert rep["symbol_bits"] == 2
        else:
            assert ctx.align_kernel == "sr_align_bfs_kernel" and rep["symbol_bits"] != 2
            assert rep["mirror_partners"] == 0 and rep["tail_threads"] == 0 and rep["orientation_route"] == "in-kernel"
            assert rep["batches"] == 1

    def collect(self, ctx):
        ctx.sync()
        sc, rv, co = ctx.pair_results()
        cnt = ctx.counters()
        got = dict(score=sc.copy(), is_reverse=rv.copy(), nops=co.copy(), labels=ctx.download_labels(), pairs=ctx.pairs(),
                   united_bases=cnt["united_bases"], match_runs=cnt["match_runs"], align_ms_positive=ctx.kernel_ms(0) > 0)
        if ctx.num_batches == 1:
            got["resident"] = cigars(ctx.alignments())
        got["gfa"] = ctx.build_gfa()
        got["gfa_compact_device"] = ctx.build_gfa(compact=True, compact_on="device")
        got["gfa_sorted"] = ctx.build_gfa(sort=SortParams())
        ctx.reset_uf()
        got["align_all"] = cigars(ctx.align_all(unite=True))
        ctx.sync()
        got["labels_align_all"] = ctx.download_labels()
        return got

    def verify(self, got):
        o = ri.oracle(self.name)
        assert got["pairs"] == o["pairs"] and got["align_ms_positive"]
        assert np.array_equal(got["score"], o["score"]) and np.array_equal(got["is_reverse"], o["is_reverse"])
        assert np.array_equal(got["nops"], o["nops"])
        for key in ("align_all",) + (("resident",) if "resident" in got else ()):
            al = got[key]
            assert al["pairs"] == o["pairs"] and al["cigar"] == o["cigar"], key
            assert np.array_equal(al["score"], o["score"]) and np.array_equal(al["is_reverse"], o["is_reverse"]), key
        assert np.array_equal(got["labels"], o["labels"]) and np.array_equal(got["labels_align_all"], o["labels"])
        assert (got["united_bases"], got["match_runs"]) == (o["united_bases"], o["match_runs"])
        assert canon_gfa(got["gfa"][0]) == canon_gfa(o["gfa"]) and got["gfa"][1:] == (o["nodes"], o["edges"])
        assert canon_gfa(got["gfa_compact_device"][0]) == canon_gfa(o["gfa_compact"])
        # the sorted graph: the host twin's sort of the same unsorted text (tests/test_sort_gpu.py)
        assert canon_gfa(got["gfa_sorted"][0]) == canon_gfa(sort_gfa(got["gfa"][0], device=SortParams.HOST_TWIN))


class Pairs(Kind):
    name = "P"

    def load(self, ctx, tmp):
        ctx.load_pairs(SeqSet(ri.oracle("P")["recs"]), Params(), list(ri.P_PAIRS))

    def collect(self, ctx):
        ctx.sync()
        return dict(pairs=ctx.pairs(), resident=cigars(ctx.alignments()), labels=ctx.download_labels(), gfa=ctx.build_gfa())

    def verify(self, got):
        o = ri.oracle("P")
        assert got["pairs"] == o["pairs"] == got["resident"]["pairs"] and got["resident"]["cigar"] == o["cigar"]
        assert np.array_equal(got["resident"]["score"], o["score"]) and np.array_equal(got["resident"]["is_reverse"], o["is_reverse"])
        assert np.array_equal(got["labels"], o["labels"])
        assert canon_gfa(got["gfa"][0]) == canon_gfa(o["gfa"])


class Paf(Kind):
    name = "C"

    def load(self, ctx, tmp):
        path = tmp / "c.paf"
        path.write_text(ri.oracle("C")["paf"])
        ctx.load_paf(SeqSet(ri.oracle("C")["recs"]), Params(), str(path))
        assert ctx.align_kernel == "" and ctx.num_batches == 1

    def collect(self, ctx):
        ctx.sync()
        with pytest.raises(SeqRushError):
            ctx.alignments()
        return dict(pairs=ctx.pairs(), labels=ctx.download_labels(), gfa=ctx.build_gfa())

    def verify(self, got):
        o = ri.oracle("C")
        assert got["pairs"] == o["pairs"]
        assert np.array_equal(got["labels"], o["labels"])
        assert canon_gfa(got["gfa"][0]) == canon_gfa(o["gfa"])


class Iterative(Kind):
    name = "D"

    def load(self, ctx, tmp):
        o = ri.oracle("D")
        ctx.load_iterative(SeqSet(o["recs"]), Params(sparsification=o["spec"], min_match_len=o["k"]))

    def step(self, ctx):
        ctx.run_iterative()                             # (a second run resets the union-find itself)

    def collect(self, ctx):
        ctx.sync()
        st = ctx.iterative_stats()
        for k in ("windows", "random_aligned"):         # schedule, not result
            st.pop(k, None)
        return dict(stats=st, pairs=ctx.pairs(), labels=ctx.download_labels(), gfa=ctx.build_gfa(compact=False))

    def verify(self, got):
        ref, st = ri.oracle("D"), got["stats"]
        assert (st["tree_entries"], st["random_entries"]) == (len(ref["tree"]), len(ref["random"]))
        assert got["pairs"] == ref["pairs"]
        assert st["post_tree"] == ref["post_tree"] and st["check_counts"] == ref["check_counts"]
        assert st["checks"] == len(ref["check_counts"])
        assert st["stabilized"] == ref["stabilized"] and st["random_processed"] == ref["processed"]
        assert st["final_components"] == ref["final"]
        assert np.array_equal(got["labels"], ref["labels"])
        assert canon_gfa(got["gfa"][0]) == canon_gfa(ref["gfa"])


class Inversions(Kind):
    def __init__(self, join=0):
        self.join = join
        self.name = "EI"

    def ref(self):
        return jh.restate(ri.EI_NAME, join=self.join) if self.join else ri.oracle("EI")

    def load(self, ctx, tmp):
        ctx.load(SeqSet(ri.oracle("EI")["recs"]), Params(min_match_len=ih.K))
        ctx.enable_inversions(0, keep_alignments=True, join_below=self.join)

    def collect(self, ctx):
        ctx.sync()
        got = dict(jobs=ctx.inversion_jobs(), stats={k: ctx.inversion_stats()[k] for k in INV_STATS}, labels=ctx.download_labels(),
                   pairs=ctx.pairs(), gfa=ctx.build_gfa(compact=False))
        js = ctx.inversion_join_stats()
        got["join_stats"] = (js["islands_absorbed"], js["rejected_site_cost"])
        got["patches"] = cigars(ctx.inversion_alignments()) if got["stats"]["candidates"] else None
        return got

    def verify(self, got):
        ref = self.ref()
        keys = JOB_KEYS + (("site_cost",) if self.join else ())
        assert [tuple(j[f] for f in keys) for j in got["jobs"]] == [tuple(j[f] for f in keys) for j in ref["jobs"]]
        acc = [j for j in ref["jobs"] if j["accepted"]]
        st = got["stats"]
        assert acc and (st["candidates"], st["accepted"]) == (len(ref["jobs"]), len(acc))
        assert st["rejected_score"] == sum(not j["by_score"] for j in ref["jobs"])
        assert st["rejected_divergence"] == sum(j["by_score"] and not j["by_div"] for j in ref["jobs"])
        assert st["scanned"] == len(ref["mains"]) and st["united_bases"] > 0
        if self.join:
            assert got["join_stats"] == (ref["islands"], st["rejected_score"])
        assert got["patches"]["cigar"] == [j["cigar"] for j in acc]
        assert got["patches"]["pairs"] == [(j["query_idx"], j["target_idx"]) for j in acc]
        assert got["patches"]["score"].tolist() == [j["patch_score"] for j in acc]
        assert got["patches"]["is_reverse"].tolist() == [j["is_reverse"] for j in acc]
        assert np.array_equal(got["labels"], ref["labels"])
        assert canon_gfa(got["gfa"][0]) == canon_gfa(ref["gfa"])


class Extend(Kind):
    name = "EX"

    def load(self, ctx, tmp):
        o = ri.oracle("EX")
        with ExtendPlan(o["old_gfa"], o["recs"][o["m"]:], device=0) as plan:
            assert plan.records == o["recs"]
            ctx.load_extend(plan, Params(min_match_len=ri.EX_K))

    def collect(self, ctx):
        ctx.sync()
        st = ctx.extend_stats()
        return dict(stats={k: st[k] for k in EXT_STATS}, pairs=ctx.pairs(), labels=ctx.download_labels(),
                    gfa=ctx.build_gfa(compact=False))

    def verify(self, got):
        o = ri.oracle("EX")
        seed = ei.restate(o["old_gfa"], o["recs"][o["m"]:])
        st = got["stats"]
        assert got["pairs"] == o["ext_pairs"]
        assert (st["old_paths"], st["old_bases"], st["old_steps"]) == (seed["n_old"], seed["old_bases"], seed["steps"])
        assert st["unions_attempted"] == len(seed["unions"]) and st["new_sequences"] == o["n"] - o["m"]
        assert (st["pairs_before"], st["pairs_after"]) == (o["n"] ** 2, len(o["ext_pairs"]))
        assert np.array_equal(got["labels"], o["labels"])
        assert canon_gfa(got["gfa"][0]) == canon_gfa(o["gfa"])


KINDS = {"A": Plain("A"), "B": Plain("B"), "P": Pairs(), "C": Paf(), "D": Iterative(), "EI": Inversions(), "EIJ": Inversions(JOIN),
         "EX": Extend()}
_FRESH = {}


def run_kind(key, mp, tmp, regime, steps=STEPS, ctx=None):
    """load on a context in the regime (a given context: as it stands), `steps` steps with no host call between, collect,
    verify -> (results, report without the free-bytes key)"""
    kind = KINDS[key]
    set_knobs(mp, kind.env)
    own = ctx is None
    if own:
        ctx = Context(0)
        keep = on_stream(ctx, regime)
    kind.load(ctx, tmp)
    rep = report(ctx)
    for _ in range(steps):
        kind.step(ctx)
    got = kind.collect(ctx)
    if own:
        ctx.close()
        del keep
    kind.verify(got)
    return got, rep


def steps_of(key):
    return STEPS if key in ("A", "B") else 1


def fresh(key, mp, tmp):
    """what a fresh context on its own stream gives for a load kind: computed once, shared unchanged"""
    if key not in _FRESH:
        _FRESH[key] = run_kind(key, mp, tmp, "own", steps=steps_of(key))
    return _FRESH[key]


# ------------------------------------------------------------------ 1. stream regimes
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("key", ["A", "B"])
def test_stream_regimes_agree_with_the_oracle_and_each_other(gpu, monkeypatch, tmp_path, key, regime):
    """load; 3 x (reset_uf; run) back to back; sync; then everything the context can return, against the oracle (run_kind
    verifies) and byte for byte against the own-stream control"""
    got, rep = fresh(key, monkeypatch, tmp_path) if regime == "own" else run_kind(key, monkeypatch, tmp_path, regime)
    want, want_rep = fresh(key, monkeypatch, tmp_path)
    same(got, want)
    assert rep == want_rep


# ------------------------------------------------------------------ 2. only the caller's stream is waited on
def test_labels_on_the_callers_stream_need_only_its_sync(gpu, monkeypatch):
    o = ri.oracle("A")
    set_knobs(monkeypatch, ri.A_ENV)
    s = torch.cuda.Stream()
    ctx = Context(0)
    ctx.set_stream(s.cuda_stream)
    ctx.load(SeqSet(o["recs"]), Params())
    with torch.cuda.stream(s):
        t = torch.empty(ctx.uf_size, dtype=torch.int64, device="cuda")
        t32 = torch.empty(ctx.uf_size, dtype=torch.int32, device="cuda")
    ctx.run()
    ctx.labels_device(t.data_ptr())
    s.synchronize()
    assert np.array_equal(t.cpu().numpy().astype(np.uint64), o["labels"])
    ctx.reset_uf()
    ctx.run()
    ctx.labels_device_u32(t32.data_ptr())
    s.synchronize()
    assert np.array_equal(t32.cpu().numpy().view(np.uint32).astype(np.uint64), o["labels"])
    ctx.close()


def test_label_exchange_on_one_side_stream_needs_only_its_sync(gpu, monkeypatch):
    """the merge_labels_u32 exchange of test_label_exchange_u32 with both contexts, the gather and the result on one side
    stream and no host wait but the stream's own"""
    o = ri.oracle("A")
    set_knobs(monkeypatch, {})
    s = torch.cuda.Stream()
    ss = SeqSet(o["recs"])
    ctxs = []
    for r in range(2):
        p = Params()
        p.c.shard_rank, p.c.shard_count = r, 2
        c = Context(0)
        c.set_stream(s.cuda_stream)
        c.load(ss, p)
        ctxs.append(c)
    n = ctxs[0].uf_size
    with torch.cuda.stream(s):
        labs = [torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2)]
        out = torch.empty(n, dtype=torch.int64, device="cuda")
    for c, t in zip(ctxs, labs):
        c.run()
        c.labels_device_u32(t.data_ptr())
    with torch.cuda.stream(s):
        gathered = torch.cat(labs)
    ctxs[0].merge_labels_u32(gathered.data_ptr(), 2)
    ctxs[0].labels_device(out.data_ptr())
    s.synchronize()
    assert np.array_equal(out.cpu().numpy().astype(np.uint64), o["labels"])
    assert sorted(ctxs[0].pairs() + ctxs[1].pairs()) == sorted(o["pairs"])
    for c in ctxs:
        c.close()


# ------------------------------------------------------------------ 3. every load kind once on the side stream
@pytest.mark.parametrize("key", ["P", "D", "EI", "EIJ", "C", "EX"])
def test_load_kinds_on_the_side_stream(gpu, monkeypatch, tmp_path, key):
    got, rep = run_kind(key, monkeypatch, tmp_path, "side", steps=steps_of(key))
    want, want_rep = fresh(key, monkeypatch, tmp_path)
    same(got, want)
    assert rep == want_rep


# ------------------------------------------------------------------ 4. the reload chain on one context
def refuses_everything(ctx):
    for call in (ctx.run, ctx.align, ctx.download_labels, ctx.alignments, ctx.pairs, ctx.build_gfa, ctx.reset_uf, ctx.unite):
        with pytest.raises(SeqRushError):
            call()
    # nothing of the load before shows either (free_dev clears the host-side description with the buffers)
    assert ctx.num_batches == 0 and ctx.num_pairs == 0 and ctx.uf_size == 0 and ctx.workspace_report() == {}


def test_reload_chain_on_one_context(gpu, monkeypatch, tmp_path):
    """A -> B -> F (empty record) -> C -> A -> D -> E-inversions -> B -> E-extend -> F (bad pair) -> A on ONE context on a side
    stream: after every successful load the results of a fresh context (which run_kind verifies against the oracle) and its
    workspace report; after every failing load nothing runs; what the previous load switched on is off"""
    s = torch.cuda.Stream()
    ctx = Context(0)
    ctx.set_stream(s.cuda_stream)
    visits_a, prev = [], None
    for name in ri.CHAIN:
        if name == "F-empty":
            with pytest.raises(SeqRushError) as e:
                ctx.load(SeqSet(ri.input_f_empty()), Params())
            assert e.value.code == -5
            refuses_everything(ctx)
            continue
        if name == "F-pair":
            with pytest.raises(SeqRushError):
                ctx.load_pairs(SeqSet(ri.input_c()), Params(), ri.F_BAD_PAIRS)
            refuses_everything(ctx)
            continue
        key = name
        got, rep = run_kind(key, monkeypatch, tmp_path, "side", steps=min(2, steps_of(key)), ctx=ctx)
        want, want_rep = fresh(key, monkeypatch, tmp_path)
        same(got, want, name)
        assert rep == want_rep, name
        if name == "A":
            visits_a.append((got, rep))
        if prev == "D":                                  # a plainly loaded context is no iterative one
            for call in (ctx.run_iterative, ctx.iterative_alignments, ctx.iterative_stats):
                with pytest.raises(SeqRushError):
                    call()
        if prev == "EI":                                 # (B) run() did no patching: run_kind compared the labels with the plain oracle's
            assert ctx.inversion_jobs() == [] and ctx.inversion_stats()["candidates"] == 0
            with pytest.raises(SeqRushError):
                ctx.inversion_alignments()
        if prev == "EX":                                 # (A, after the failed load) reset_uf() is init only again
            with pytest.raises(SeqRushError):
                ctx.extend_stats()
            ctx.reset_uf(); ctx.sync()
            ident = ctx.download_labels()
            c2 = Context(0)
            set_knobs(monkeypatch, KINDS[key].env)
            c2.load(SeqSet(ri.oracle(name)["recs"]), Params())
            c2.sync()
            assert np.array_equal(ident, c2.download_labels())
            assert np.array_equal(ident, ei.plain_labels(ri.oracle(name)["total_len"], []))
            c2.close()
        prev = name
    assert len(visits_a) == 3
    for got, rep in visits_a[1:]:
        same(got, visits_a[0][0], "A again")
        assert rep == visits_a[0][1]
    ctx.close()


# ------------------------------------------------------------------ 5. two contexts interleaved in one thread
def test_two_contexts_interleaved_on_two_side_streams(gpu, monkeypatch):
    oa, ob_ = ri.oracle("A"), ri.oracle("B")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a, b = Context(0), Context(0)
    a.set_stream(s1.cuda_stream)
    b.set_stream(s2.cuda_stream)
    set_knobs(monkeypatch, ri.A_ENV)
    a.load(SeqSet(oa["recs"]), Params())
    set_knobs(monkeypatch, {})
    b.load(SeqSet(ob_["recs"]), Params(**ri.B_KW))
    assert a.align_kernel == "sr_align_blk_kernel" and b.align_kernel == "sr_align_bfs_kernel"
    with torch.cuda.stream(s1):
        ta = torch.empty(a.uf_size, dtype=torch.int64, device="cuda")
    with torch.cuda.stream(s2):
        tb = torch.empty(b.uf_size, dtype=torch.int64, device="cuda")
    a.run(); b.run(); a.run()
    b.labels_device(tb.data_ptr())
    a.labels_device(ta.data_ptr())
    a.sync(); b.sync()
    assert np.array_equal(ta.cpu().numpy().astype(np.uint64), oa["labels"])
    assert np.array_equal(tb.cpu().numpy().astype(np.uint64), ob_["labels"])
    for c, o in ((a, oa), (b, ob_)):
        sc, rv, co = c.pair_results()
        assert np.array_equal(sc, o["score"]) and np.array_equal(rv, o["is_reverse"]) and np.array_equal(co, o["nops"])
    cnt = a.counters()                                   # of the second run alone: counters restart with every pass
    assert (cnt["united_bases"], cnt["match_runs"]) == (oa["united_bases"], oa["match_runs"])
    a.close(); b.close()


# ------------------------------------------------------------------ 6. set_stream on a loaded context
def test_set_stream_on_a_loaded_context_after_a_sync(gpu, monkeypatch):
    o = ri.oracle("A")
    set_knobs(monkeypatch, ri.A_ENV)
    ctx = Context(0)
    ctx.load(SeqSet(o["recs"]), Params())

    def check():
        ctx.sync()
        assert np.array_equal(ctx.download_labels(), o["labels"])
        sc, rv, co = ctx.pair_results()
        assert np.array_equal(sc, o["score"]) and np.array_equal(rv, o["is_reverse"]) and np.array_equal(co, o["nops"])
    ctx.run()
    check()
    s = torch.cuda.Stream()
    for ptr in (s.cuda_stream, 0):
        ctx.set_stream(ptr)                              # only ever after a sync
        for _ in range(2):
            ctx.reset_uf(); ctx.run()
        check()
    ctx.close()


# ------------------------------------------------------------------ 7. device memory over reloads
LOADS = 6


def test_device_memory_over_reloads(gpu, monkeypatch):
    """six loads of A on one context against six fresh contexts, each closed before the next: the reload path may keep no more
    device memory between its second and its sixth load than the fresh path's own reports scatter (+ one allocation granule,
    the smallest step the fresh series shows).  No torch tensor is allocated between the loads."""
    o = ri.oracle("A")
    set_knobs(monkeypatch, ri.A_ENV)
    ss, p = SeqSet(o["recs"]), Params()

    def one(ctx):
        ctx.load(ss, p)
        free = int(ctx.workspace_report()[FREE_KEY])
        ctx.run(); ctx.sync()
        return free
    fresh_series = []
    for _ in range(LOADS):
        c = Context(0)
        fresh_series.append(one(c))
        c.close()
    ctx = Context(0)
    reload_series = [one(ctx) for _ in range(LOADS)]
    ctx.close()
    print(f"\nfree bytes at load, fresh contexts: {fresh_series}\nfree bytes at load, one context:    {reload_series}")
    tail = fresh_series[1:]
    spread = max(tail) - min(tail)
    steps = [abs(x - y) for x, y in zip(fresh_series, fresh_series[1:]) if x != y]
    granule = min(steps) if steps else 0                 # a fresh series without a step shows no granule: none is granted
    drop = reload_series[1] - reload_series[-1]
    print(f"fresh spread {spread}, granule {granule}, reload drop from load 2 to load {LOADS}: {drop}")
    assert drop <= spread + granule
