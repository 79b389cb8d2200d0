"""Inputs and restatements for the tests of the path-by-bin tables.

restate(): a per-base numpy statement of cov / inv that shares nothing with the library.  tsv_of() / rgb_of(): Python
statements of the two outputs from the integers.  seam_cases(): GFA text built for the seams of the step kernel (a wave = 64
steps, a workgroup = 256, a chunk of the LDS variant = CHUNK steps of one path, the variant threshold = LDS_MAX_BINS bins)."""
import numpy as np

import sort_helpers as sh
import stats_helpers as st

CHUNK = 4096            # SR_BIN_CHUNK
LDS_MAX_BINS = 4096     # SR_BIN_LDS_MAX_BINS
MASK = (1 << 64) - 1


def layout_of(text):
    """-> (path names, per path list of (pos, len, rev), L) with nodes laid end to end in ascending id order"""
    g = st.parse(text)
    pos, acc = {}, 0
    for i in sorted(g.seq):
        pos[i] = acc
        acc += len(g.seq[i])
    return [n for n, _ in g.paths], [[(pos[h >> 1], len(g.seq[h >> 1]), h & 1) for h in steps] for _, steps in g.paths], acc


def resolve(L, bin_width=0, bins=0):
    """-> (w, B) of a request"""
    assert (bin_width != 0) != (bins != 0)
    w = bin_width if bin_width else (1 if L == 0 else -(-L // bins))
    return w, -(-L // w)


def restate(text, bin_width=0, bins=0):
    """-> dict(length, paths, bins, bin_width, cov, inv): per-base coverage by difference arrays, then sums over each bin"""
    names, paths, L = layout_of(text)
    w, B = resolve(L, bin_width, bins)
    cov, inv = np.zeros((len(paths), B), dtype=np.uint64), np.zeros((len(paths), B), dtype=np.uint64)
    starts = np.arange(0, L, w)
    for p, steps in enumerate(paths):
        if not steps or L == 0:
            continue
        d = np.zeros((2, L + 1), dtype=np.int64)
        a = np.array(steps, dtype=np.int64).reshape(-1, 3)
        np.add.at(d[0], a[:, 0], 1)
        np.add.at(d[0], a[:, 0] + a[:, 1], -1)
        np.add.at(d[1], a[:, 0], a[:, 2])
        np.add.at(d[1], a[:, 0] + a[:, 1], -a[:, 2])
        per_base = np.cumsum(d, axis=1)[:, :L]
        cov[p] = np.add.reduceat(per_base[0], starts).astype(np.uint64)
        inv[p] = np.add.reduceat(per_base[1], starts).astype(np.uint64)
    return dict(length=L, paths=len(paths), bins=B, bin_width=w, cov=cov, inv=inv, names=names)


def assert_same(got, want, what=""):
    for k in ("length", "paths", "bins", "bin_width"):
        assert int(got[k]) == int(want[k]), f"{what}: {k} {got[k]} != {want[k]}"
    for k in ("cov", "inv"):
        assert got[k].shape == want[k].shape and got[k].dtype == np.uint64, f"{what}: shape of {k}"
        bad = np.argwhere(got[k] != want[k])
        assert len(bad) == 0, f"{what}: {k} differs in {len(bad)} cells, first at (path, bin) {tuple(bad[0])}: " \
                              f"{got[k][tuple(bad[0])]} != {want[k][tuple(bad[0])]}"


def bin_lens(d):
    L, w, B = int(d["length"]), int(d["bin_width"]), int(d["bins"])
    return np.array([min((b + 1) * w, L) - b * w for b in range(B)], dtype=np.int64)


def tsv_of(d, names):
    """the bytes sr_path_bins_tsv must write for the integers of d"""
    out = [f"#seqrush_amd path bins v1\tbin_width={d['bin_width']}\tbins={d['bins']}\tlength={d['length']}\tpaths={d['paths']}\n",
           "path\tbin\tcov_bp\tinv_bp\tmean_cov\tmean_inv\n"]
    bl = bin_lens(d)
    for p, name in enumerate(names):
        for b in np.flatnonzero(d["cov"][p]):
            c, v = int(d["cov"][p, b]), int(d["inv"][p, b])
            out.append(f"{name}\t{b + 1}\t{c}\t{v}\t{c / int(bl[b]):.6f}\t{v / c:.6f}\n")
    return "".join(out)


def base_colour(name):
    h = 0xcbf29ce484222325
    for ch in name.encode():
        h = ((h ^ ch) * 0x100000001b3) & MASK
    z = (h + 0x9E3779B97F4A7C15) & MASK                       # splitmix64 of (seed = h, index 0)
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    z ^= z >> 31
    return [32 + ((((z >> (8 * i)) & 0xff) * 3) >> 2) for i in range(3)]


def rgb_of(d, names, mode="path", path_height=10, path_gap=1, depth_max=4):
    """the image sr_path_bins_rgb must draw for the integers of d -> uint8 [height, bins, 3]"""
    P, B = int(d["paths"]), int(d["bins"])
    H = P * path_height + (P - 1) * path_gap if P else 0
    img = np.full((H, B, 3), 255, dtype=np.uint8)
    bl = bin_lens(d)
    for p in range(P):
        cov, inv = d["cov"][p].astype(np.int64), d["inv"][p].astype(np.int64)
        if mode == "path":
            a = np.minimum(cov, bl)
            row = np.stack([255 - (255 - c) * a // bl for c in base_colour(names[p])], axis=1)
        elif mode == "strand":
            row = np.zeros((B, 3), dtype=np.int64)
            row[2 * inv > cov, 0] = 255
        else:
            g = 255 - np.minimum(255, cov * 255 // (bl * depth_max))
            row = np.stack([g, g, g], axis=1)
        row[cov == 0] = 255
        y = p * (path_height + path_gap)
        img[y:y + path_height] = row.astype(np.uint8)[None]
    return img


def host_inputs():
    """every input of the statistics tests: (name, GFA text)"""
    from test_stats_host import GOLDEN
    out = [("golden:" + c["name"], c["gfa"]) for c in GOLDEN]
    out += [("random:%d" % c[0], st.random_gfa(c[0], c[1], c[2], c[3], sparse_ids=c[0] % 2 == 0)) for c in st.RANDOM_CASES]
    out += [("hand:" + n, t) for n, t in sorted(st.hand_cases().items())]
    return out


# ------------------------------------------------------------------ seams of the step kernel
BALLAST = 6000          # a last node this long lifts L above LDS_MAX_BINS, so that w = 1 and w = 2 take the global variant


def _gfa(lens, paths):
    return sh.Gfa({i + 1: "ACGT"[i % 4] * n for i, n in enumerate(lens)}, [], paths).text()


def _fwd(ids):
    return [i << 1 for i in ids]


def _walk(seed, n_nodes, n_steps):
    rng = np.random.default_rng(seed)
    k, out = 0, []
    for _ in range(n_steps):
        out.append(((k + 1) << 1) | int(rng.random() < 0.2))
        k = (k + int(rng.integers(0, 3))) % n_nodes
    return out


def _threshold(L):
    rng = np.random.default_rng(L)
    lens = [int(x) for x in rng.integers(1, 41, size=150)]
    assert sum(lens) < L - 1
    lens.append(L - sum(lens))
    return _gfa(lens, [(f"t{p}", _walk(100 * L + p, len(lens), 700)) for p in range(3)])


def seam_cases():
    """name -> (GFA text, [settings]); a setting = dict(bin_width=w) or dict(bins=n).  With the ballast node w = 1 and w = 2
    give B > LDS_MAX_BINS (global atomics), the wide settings B <= LDS_MAX_BINS (rows in LDS)."""
    both = [dict(bin_width=1000), dict(bin_width=1), dict(bin_width=2), dict(bin_width=7), dict(bins=64)]
    ones = [1] * 300 + [BALLAST]
    cases = {
        # runs of more than 64 equal keys across wave (64) and workgroup (256) boundaries: w = 1000 puts 300 steps into one bin;
        # path r stays on one node, a run under every width
        "runs_across_waves": (_gfa(ones, [("a", _fwd(range(1, 301))), ("r", _fwd([7] * 200 + [301])), ("b", _fwd([301]))]), both),
        # a ends where b begins, in the same bin and (global variant) in one wave: lanes 39 and 40
        "path_boundary_in_a_wave": (_gfa([1] * 79 + [BALLAST], [("a", _fwd(range(1, 41))), ("b", _fwd(range(40, 80))), ("c", _fwd([80]))]), both),
        # two bins in turn, lane by lane: no two neighbouring lanes share a key, every other one does
        "alternating_bins": (_gfa([1, 1, BALLAST], [("a", _fwd([1, 2] * 65)), ("b", [2, 5, 3, 4] * 33 + [6])]), both),
        "empty_paths_between": ("H\tVN:Z:1.0\nS\t1\tACG\nS\t2\tTT\nS\t3\t" + "A" * BALLAST + "\nP\te0\t\t*\nP\ta\t1+,2+\t*\nP\te1\t\t*\nP\te2\t\t*\n"
                                "P\tb\t2-,3+,1-\t*\nP\te3\t\t*\n", both),
        # the wave-cooperative span: 5000 bins at w = 1 (global), 715 at w = 7 (LDS); forward, reverse and from a second path
        "long_node": (_gfa([3, 5000, 2, 4], [("a", [2, 4, 6, 5, 8]), ("b", [6, 4, 2])]), [dict(bin_width=1), dict(bin_width=7), dict(bins=64)]),
        "one_path": (_gfa([5, 1, 9, BALLAST], [("only", [2, 4, 7, 8, 3])]), both),
        "paths_130": (_gfa([3, 1, 4, 1, 5, 9, 2, 6, BALLAST], [(f"p{k}", _walk(k, 8, 1 + k % 7) + ([18] if k % 40 == 0 else [])) for k in range(130)]), both),
    }
    # step counts at the wave, workgroup and chunk boundaries, all in one path over 50 short nodes
    for n in (1, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1):
        rng = np.random.default_rng(n)
        lens = [int(x) for x in rng.integers(1, 9, size=50)] + [BALLAST]
        cases[f"steps_{n}"] = (_gfa(lens, [("s", _walk(n, 50, n))]), both)
    # B at the variant threshold - 1, at it and + 1
    for L in (LDS_MAX_BINS - 1, LDS_MAX_BINS, LDS_MAX_BINS + 1):
        cases[f"threshold_{L}"] = (_threshold(L), [dict(bin_width=1)])
    return cases
