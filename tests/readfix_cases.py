"""Inputs of the read-cleaning tests (a helper, not a conftest): deterministic generators and a memo around a `freq` callable.

  planted_case()   reads of a random genome with known substitutions that the rules must undo completely (the test states why)
  noisy_case()     reads with random errors over repeats, tandem arrays and two-allele loci; every status and counter occurs
  distinct_freq()  get_freq over the canonical distinct 23-mers of a plain buffer, counted with numpy (what the device builds)
  MemoFreq         a `freq` that asks the wrapped one only for codes it has not seen
"""
import numpy as np

import debruijn_ref as D
import graph_cases as G

COMP = np.zeros(256, np.uint8)
for _a, _b in zip(b"ACGT", b"TGCA"):
    COMP[_a] = _b


class MemoFreq:
    """freq(codes) with a dict in front: the helper of readfix_ref asks for the same windows again after every fix."""

    def __init__(self, freq):
        self.freq, self.memo = freq, {}

    def __call__(self, codes):
        codes = np.ascontiguousarray(codes, dtype=np.uint64).reshape(-1)
        lst = codes.tolist()
        miss = [c for c in set(lst) if c not in self.memo]
        if miss:
            self.memo.update(zip(miss, self.freq(np.array(miss, dtype=np.uint64)).tolist()))
        m = self.memo
        return np.array([m[c] for c in lst], dtype=np.uint32)

    def prime(self, buf, start, end):
        """every valid window of the reads, in one call of the wrapped freq"""
        a = np.frombuffer(bytes(buf), dtype=np.uint8)
        w = np.lib.stride_tricks.sliding_window_view(a, 23)
        ok = np.isin(a, np.frombuffer(b"ACGT", np.uint8))
        bad = np.concatenate([[0], np.cumsum(~ok)])
        keep = np.zeros(w.shape[0], bool)
        for s, e in zip(start.tolist(), end.tolist()):
            if s <= e <= a.shape[0] and e - s >= 23:
                keep[s:e - 22] = True
        keep &= (bad[23:] - bad[:-23]) == 0
        self(np.unique(D.encode(np.ascontiguousarray(w[keep]))))


def genome_freq(genome: np.ndarray, tf: int = 5):
    """(canonical distinct codes, get_freq over them with the one tf)"""
    codes = np.unique(D.canon(D.encode(np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(genome, 23)))))
    return codes, G.dict_freq(codes, np.full(codes.shape[0], tf, np.uint32))


def distinct_freq(plain: np.ndarray):
    """get_freq over the canonical 23-mers of the windows of `plain` that hold upper-case A/C/G/T only, with their counts."""
    w = np.lib.stride_tricks.sliding_window_view(plain, 23)
    ok = np.isin(plain, np.frombuffer(b"ACGT", np.uint8))
    bad = np.concatenate([[0], np.cumsum(~ok)])
    keep = (bad[23:] - bad[:-23]) == 0
    codes, counts = np.unique(D.canon(D.encode(np.ascontiguousarray(w[keep]))), return_counts=True)
    return G.dict_freq(codes, counts.astype(np.uint32))


SPECIAL = (0, 22, 23, 127, 149)


def planted_case(seed=31415, n_reads=2000, n_with_n=200, glen=40_000):
    """(genome uint8[glen], buf uint8[], start, end, truth uint8[] of the size of buf, plants): 150-base reads of either strand, one
    newline behind each. Read r < n_reads - n_with_n carries r % 4 substitutions, pairwise >= 45 bases apart, the first of them at
    SPECIAL[(r // 4) % 5]; the last n_with_n reads carry one 'N'. plants[r] = [(position, byte planted)] in the order in which the rules
    apply the fixes: phase R takes the positions >= 23 from the left, phase L then the one below 23."""
    rng = np.random.default_rng(seed)
    genome = D.LETTERS[rng.integers(0, 4, glen)]
    at = rng.integers(0, glen - 150, n_reads)
    truth = genome[at[:, None] + np.arange(150)[None, :]]
    flip = rng.random(n_reads) < 0.5
    truth[flip] = COMP[truth[flip][:, ::-1]]
    reads = truth.copy()
    plants = []
    for r in range(n_reads):
        if r >= n_reads - n_with_n:
            pos = [int(rng.integers(0, 150))]
            reads[r, pos[0]] = ord("N")
        else:
            pos = [SPECIAL[(r // 4) % 5]] if r % 4 else []
            while len(pos) < r % 4:
                free = [p for p in range(150) if all(abs(p - q) >= 45 for q in pos)]
                if not free:                                       # the draws so far leave no room: keep the special position only
                    pos = pos[:1]
                    continue
                pos.append(free[int(rng.integers(0, len(free)))])
            for p in pos:
                reads[r, p] = b"ACGT"[(b"ACGT".index(truth[r, p]) + int(rng.integers(1, 4))) % 4]
        order = sorted(p for p in pos if p >= 23) + [p for p in pos if p < 23]
        plants.append([(p, int(reads[r, p])) for p in order])
    nl = np.full((n_reads, 1), 10, np.uint8)
    buf = np.concatenate([reads, nl], axis=1).reshape(-1)
    tr = np.concatenate([truth, nl], axis=1).reshape(-1)
    start = np.arange(n_reads, dtype=np.uint64) * np.uint64(151)
    return genome, buf, start, start + np.uint64(150), tr, plants


LENGTHS = (23, 24, 45, 86, 87, 150, 151)


def noisy_case(seed=2718, n_reads=4000, glen=30_000):
    """(plain uint8[], start, end): reads of a genome with a 400 bp repeat planted 4 times, 4 tandem arrays (units of 24 .. 36 bp, 12
    copies) and a 3000 bp segment present twice, the copy differing in one base every 100 bp; lengths drawn from LENGTHS, either
    strand, 1 % substitutions and 0.1 % 'N', one newline behind each read. The last 60 reads are 150 bases without such errors, each
    over one of the 30 differing bases and carrying there one of the two bases that neither copy has: both alleles are solid (nM),
    and no two of these reads share their wrong 23-mers."""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 4, glen).astype(np.uint8)
    rep = rng.integers(0, 4, 400).astype(np.uint8)
    for p in (1000, 5000, 14_000, 26_000):
        g[p:p + 400] = rep
    for a, p in enumerate((2500, 7000, 16_000, 28_000)):
        unit = rng.integers(0, 4, 24 + 4 * a).astype(np.uint8)
        g[p:p + 12 * len(unit)] = np.tile(unit, 12)
    seg_a, seg_b = 9000, 21_000
    loci = 50 + 100 * np.arange(30)
    g[seg_b:seg_b + 3000] = g[seg_a:seg_a + 3000]
    g[seg_b + loci] = (g[seg_a + loci] + 1) % 4
    n_allele_reads = 2 * len(loci)
    out, start, end, at = [], [], [], 0
    for r in range(n_reads):
        L = int(LENGTHS[rng.integers(0, len(LENGTHS))])
        k = r - (n_reads - n_allele_reads)
        if k >= 0:
            L, locus = 150, int(loci[k // 2])
            off = int(rng.integers(30, 121))                       # the differing base lies at 30 .. 120 of the read
            p = (seg_a if k % 3 else seg_b) + locus - off
            s = g[p:p + L].copy()
            s[off] = (g[seg_a + locus] + 2 + k % 2) % 4
        else:
            p = int(rng.integers(0, glen - L))
            s = g[p:p + L].copy()
            sub = rng.random(L) < 0.01
            s = np.where(sub, (s + rng.integers(1, 4, L)) % 4, s).astype(np.uint8)
        s = D.LETTERS[s]
        if k < 0:
            s[rng.random(L) < 0.001] = ord("N")
        if rng.random() < 0.5:
            s = np.where(s[::-1] == ord("N"), ord("N"), COMP[s[::-1]]).astype(np.uint8)
        out += [s, np.array([10], np.uint8)]
        start.append(at)
        end.append(at + L)
        at += L + 1
    return np.concatenate(out), np.array(start, np.uint64), np.array(end, np.uint64)
