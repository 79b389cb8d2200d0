"""--iterative without a device: the stop rule, the split of the tree: pairs into tree and random entries, the component
count of a SeqRush forest, and the CLI refusals that must come before anything touches a GPU."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import oracle_binding as ob
from seqrush_amd.seqrush import (Params, iterative_pair_lists, iterative_report, iterative_stop_host, rust_f64,
                                 uf_count_components_host)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ stop rule
def ref_stop(counts, post_tree, n_random):
    """align_and_unite_iterative's phase-2 loop (src/seqrush.rs:1034-1122), transcribed: one check after every 10 random
    entries (counts[k] = count of check k); -> random entries processed, checks taken, stabilized"""
    prev, stable = post_tree, 0
    checks = 0
    for pair_idx in range(n_random):
        if (pair_idx + 1) % 10 == 0:
            c = counts[checks]
            checks += 1
            if c == prev:
                stable += 1
                if stable >= 10:
                    return pair_idx + 1, checks, True
            else:
                stable = 0
            prev = c
    return n_random, checks, False


def product_stop(counts, post_tree, n_random):
    nchk = n_random // 10
    k = iterative_stop_host(counts[:nchk], post_tree)
    return (k * 10, k, True) if k else (n_random, nchk, False)


@pytest.mark.parametrize("n_random,counts,post", [
    (0, [], 5),
    (7, [], 5),                                  # fewer than 10 random entries: no check at all
    (9, [], 1),
    (10, [5], 5),
    (100, [5] * 10, 5),                          # the earliest possible stop: 10 equal checks, 100 entries
    (99, [5] * 9, 5),                            # one entry short of it: a trailing partial chunk has no check
    (200, [5] * 9 + [4] + [4] * 10, 5),          # a change at the 10th check resets `stable`
    (200, [4] + [4] * 9 + [3] * 10, 5),
    (130, [6, 5, 4, 3, 2, 1, 1, 1, 1, 1, 1, 1, 1], 7),   # never 10 in a row
    (300, [9 - (k % 2) for k in range(30)], 9),          # alternating: no stop
    (110, [5] * 11, 6),                          # the first check compares with post_tree (a change), then 10 equal
])
def test_stop_rule_cases(n_random, counts, post):
    assert product_stop(counts, post, n_random) == ref_stop(counts, post, n_random)


def test_stop_rule_earliest_stop_is_at_100_entries():
    assert product_stop([3] * 20, 3, 200) == (100, 10, True)
    assert product_stop([4] + [3] * 20, 4, 220) == (120, 12, True)      # equal, change, then 10 equal
    assert iterative_stop_host((c for c in [3] * 10), 3) == 10      # any iterable


def test_stop_rule_random_count_sequences():
    rng = random.Random(7)
    for _ in range(400):
        n_random = rng.randrange(0, 700)
        nchk = n_random // 10
        post = rng.randrange(1, 40)
        counts, c = [], post
        for _ in range(nchk):
            if rng.random() < rng.choice([0.02, 0.1, 0.3]):
                c = max(1, c - rng.randrange(1, 3))
            counts.append(c)
        assert product_stop(counts, post, n_random) == ref_stop(counts, post, n_random)


# ------------------------------------------------------------------ pair lists
def splitmix64(x):
    M = (1 << 64) - 1
    x = (x + 0x9e3779b97f4a7c15) & M
    x = ((x ^ (x >> 30)) * 0xbf58476d1ce4e5b9) & M
    x = ((x ^ (x >> 27)) * 0x94d049bb133111eb) & M
    return x ^ (x >> 31)


def unit53(h):
    return (h >> 11) * (1.0 / 9007199254740992.0)


def ref_lists(n, sel, seed, rf):
    """the documented split (sr_pairs.cpp "pair list"): tree entries row-major, random entries by (hash, i, j)"""
    tree, rnd = [], []
    for i in range(n):
        for j in range(i + 1, n):
            if sel is not None and (sel[i, j] or sel[j, i]):
                tree.append((i, j))
                continue
            h = splitmix64(seed ^ (i * n + j))
            if unit53(h) < rf:
                rnd.append((h, i, j))
    rnd.sort()
    return tree, [(i, j) for _, i, j in rnd]


def tree_pairs_today(n, sel, seed, rf):
    """the unordered pairs of today's tree: list (enumerate_pairs, SR_SPARSE_TREE)"""
    out = set()
    for i in range(n):
        for j in range(i + 1, n):
            if (sel is not None and (sel[i, j] or sel[j, i])) or unit53(splitmix64(seed ^ (i * n + j))) < rf:
                out.add((i, j))
    return out


@pytest.mark.parametrize("seed", range(6))
def test_pair_lists_match_restatement(seed):
    rng = np.random.default_rng(seed)
    for _ in range(8):
        n = int(rng.integers(1, 40))
        sel = (rng.random((n, n)) < rng.choice([0.0, 0.05, 0.2])).astype(np.uint8)
        rf = float(rng.choice([0.0, 0.1, 0.37, 1.0]))
        pseed = int(rng.integers(0, 1 << 62))
        p = Params(sparsification=f"tree:3,3,{rf}")
        p.c.sparsify_seed = pseed
        tree, rnd = iterative_pair_lists(n, sel, p)
        assert (tree, rnd) == ref_lists(n, sel, pseed, rf)
        assert not set(tree) & set(rnd)
        assert set(tree) | set(rnd) == tree_pairs_today(n, sel, pseed, rf)
        assert len(set(rnd)) == len(rnd)


def test_pair_lists_without_selection_and_shuffled_order():
    p = Params(sparsification="tree:0,0,0.5")
    tree, rnd = iterative_pair_lists(30, None, p)
    assert tree == []
    assert rnd == ref_lists(30, None, 42, 0.5)[1]
    assert rnd != sorted(rnd)                      # a seeded shuffle, not row order
    assert iterative_pair_lists(1, None, p) == ([], [])


# ------------------------------------------------------------------ component count
@pytest.mark.parametrize("seed", range(5))
def test_count_components_host_matches_oracle(seed):
    rng = random.Random(seed)
    recs = [(f"s{i}", bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(1, 30)))) for i in range(rng.randrange(1, 6))]
    o = ob.OracleSeqRush(records=recs)
    T = o.total_length
    L = ob.lib()
    assert uf_count_components_host(o.nodes(), T) == o.count_components() == T
    for _ in range(rng.randrange(0, 3 * T)):
        a = L.sro_make_pos(rng.randrange(T), rng.randrange(2))     # forward and reverse-strand positions
        b = L.sro_make_pos(rng.randrange(T), rng.randrange(2))
        L.sro_buf_unite(o.uf, a, b)
        if rng.random() < 0.2:
            assert uf_count_components_host(o.nodes(), T) == o.count_components()
    assert uf_count_components_host(o.nodes(), T) == o.count_components()


# ------------------------------------------------------------------ report formatting
def test_report_lines_and_rust_float_display():
    assert rust_f64(50.0) == "50" and rust_f64(0.1) == "0.1" and rust_f64(1.0) == "1" and rust_f64(1e-7) == "0.0000001"
    st = dict(post_tree=9, check_counts=[8] + [7] * 10, stabilized=True, random_entries=300, final_components=7)
    lines = iterative_report(st)
    assert lines == ["Phase 1 complete: 9 components after tree pairs",
                     "\nPhase 2: Processing random pairs with early stopping...",
                     "Graph stabilized after 110 random pairs (7 components)",
                     "Skipped 190 random pairs (63.33333333333333% reduction)",
                     "\nFinal component count: 7"]
    st = dict(post_tree=5, check_counts=[5] * 10, stabilized=True, random_entries=200, final_components=5)
    assert "Skipped 100 random pairs (50% reduction)" in iterative_report(st)
    verbose = iterative_report(st, verbose=True)
    assert verbose[2] == "  After 10 random pairs: 5 components (prev: 5)"
    st = dict(post_tree=5, check_counts=[4, 3], stabilized=False, random_entries=25, final_components=2)
    assert not any("stabilized" in x for x in iterative_report(st))


# ------------------------------------------------------------------ CLI refusals (before any device use)
def _fasta(tmp_path):
    fa = tmp_path / "in.fa"
    fa.write_text(">a\nACGTACGT\n>b\nACGTTCGT\n")
    return str(fa)


@pytest.mark.parametrize("extra", [["-p", "x.paf"], ["--gpus", "2"]])
def test_python_cli_refuses(tmp_path, extra):
    r = subprocess.run([sys.executable, "-m", "seqrush_amd", "-s", _fasta(tmp_path), "-o", str(tmp_path / "o.gfa"), "--no-sort",
                        "--iterative"] + extra, cwd=ROOT, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 1, r.stdout + r.stderr
    assert "--iterative cannot be combined" in r.stderr
    assert "Loaded" not in r.stdout and not (tmp_path / "o.gfa").exists()


@pytest.mark.parametrize("extra", [["--shard", "0/2", "--labels-out", "p.bin"], ["--labels-in", "p.bin"], ["-p", "x.paf"]])
def test_cpp_cli_refuses(tmp_path, extra):
    exe = os.path.join(ROOT, "seqrush_amd", "seqrush_mi355x")
    r = subprocess.run([exe, "-s", _fasta(tmp_path), "-o", str(tmp_path / "o.gfa"), "--no-sort", "--iterative"] + extra,
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert r.returncode == 1, r.stdout + r.stderr
    assert "--iterative cannot be combined" in r.stderr
    assert "Loaded" not in r.stdout and not (tmp_path / "o.gfa").exists()


def test_cpp_cli_usage_names_iterative():
    exe = os.path.join(ROOT, "seqrush_amd", "seqrush_mi355x")
    r = subprocess.run([exe, "--no-such-flag"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--iterative" in r.stderr
