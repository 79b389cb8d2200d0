"""Inputs of the mirror tests (test_mirror_host.py, test_mirror_gpu.py): small families on which the alignment of (t, q) is,
or is not, the transpose of the alignment of (q, t) -- and the CPU oracle's answers on them, computed once per process.

Input A: 6 sequences from one 3 000 bp random ancestor, 4 % substitutions per member, and 4 shared positions where every
member carries its own unrelated random block of 20-45 bp in place of 0-10 ancestral bases.  Unrelated blocks of different
lengths at the same place give co-optimal gap placements: ties in the M step of the backtrace (an I tag and a D tag at the
maximum offset), in the diagonal of a breakpoint and in its component.  The seed is chosen so that the oracle's CIGARs of
at least 3 of the 15 unordered pairs are NOT transposes of each other (asserted by the tests: they would be vacuous
without); this draw (A_SEED) has 7, alignment scores 1 554 .. 1 757."""
import functools

import numpy as np

import oracle_binding as ob
from seqrush_amd import synth

A_SEED = 7
A_N, A_L, A_SUB, A_SITES = 6, 3000, 0.04, 4
A_DIVERGENCE = 0.088            # -d that rejects about half of Input A's pairs (scores 1 554 .. 1 757 on ~3 100 bp)


def input_a(seed=A_SEED):
    rng = np.random.RandomState(seed)
    anc = synth.base_sequence(A_L, 90000 + seed)
    sites = sorted(int(x) for x in rng.choice(np.arange(300, A_L - 300, 50), A_SITES, replace=False))
    recs = []
    for m in range(A_N):
        codes = synth.substitute(anc, A_SUB, 91000 + 100 * seed + m)
        parts, pos = [], 0
        for s in sites:
            parts.append(codes[pos:s])
            parts.append(rng.randint(0, 4, size=int(rng.randint(20, 46))).astype(np.uint8))
            pos = s + int(rng.randint(0, 11))
        parts.append(codes[pos:])
        recs.append((f"a{m}", synth.to_bytes(np.concatenate(parts))))
    return recs


def subst_only():
    """8 x 1 200 bp, substitutions only: (almost) no ties"""
    return synth.snp_family(8, 1200, 0.04, 7411)


def one_reversed():
    """5 x 1 500 bp with indels, member 2 reverse-complemented: its pairs align on the reverse strand"""
    return [(n, synth.reverse_complement(s) if i == 2 else s) for i, (n, s) in enumerate(synth.indel_family(5, 1500, 0.04, 0.01, 7412))]


SETS = {"A": input_a, "subst": subst_only, "rc": one_reversed}
_SWAP = bytes.maketrans(b"ID", b"DI")


def transpose(raw: bytes) -> bytes:
    """raw CIGAR bytes (one byte per column: M X I D) of the transposed alignment"""
    return raw.translate(_SWAP)


class OracleOnce:
    """the oracle's answers on one input under one parameter set, computed once and shared unchanged by every test that runs
    the input: align_pair of all ordered pairs, labels and GFA of the all-vs-all run (what test_gpu_parity.check_parity asks
    of an OracleSeqRush)"""

    def __init__(self, recs, kw):
        from test_gpu_parity import oracle_params
        o = ob.OracleSeqRush(records=recs)
        op = oracle_params(**kw)
        n = len(recs)
        self.n = n
        self.pairs = {(q, t): o.align_pair(op, q, t) for q in range(n) for t in range(n)}
        o.align_and_unite(op)
        self.labels = o.canonical_labels()
        self.gfa_out = o.gfa(canonical=True)
        o.close()

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

    def non_transposable(self):
        """unordered pairs q < t, both on the forward strand, whose two CIGARs are not transposes of each other"""
        return [(q, t) for q in range(self.n) for t in range(q + 1, self.n)
                if not self.pairs[q, t]["is_reverse"] and not self.pairs[t, q]["is_reverse"]
                and transpose(self.pairs[q, t]["cigar"]) != self.pairs[t, q]["cigar"]]

    def reverse_pairs(self):
        return [(q, t) for (q, t), a in self.pairs.items() if a["is_reverse"]]


@functools.lru_cache(maxsize=None)
def oracle_once(name, kw=()):
    return OracleOnce(SETS[name](), dict(kw))


def resolve(inp, kw):
    """inp: a name of SETS, or (key, records, function of the sorted parameter tuple -> the oracle's answers) for an input
    that lives elsewhere (tests/tie_inputs.py) -> (key, record list, OracleOnce under kw)"""
    kt = tuple(sorted(kw.items()))
    if isinstance(inp, str):
        return inp, SETS[inp](), oracle_once(inp, kt)
    key, recs, oracle = inp
    return key, list(recs), oracle(kt)
