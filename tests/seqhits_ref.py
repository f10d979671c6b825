"""Seed hits and diagonal votes of sequences against indexed reads, restated in plain Python for the tests (no GPU).

Per window: PHASH_MAP::get_pfid on the raw bytes (hash.hpp:150-170) with the MPHF of the CPU oracle, the bucket of the positions array
(python_wrapper.cpp:800-831), get_rid / get_start (python_wrapper.cpp:757-789 over IntervalTree::query :66-74), and the strand by
comparing 23 bytes of the reads file. Then the grouping by (rid, strand, diag)."""
import bisect
import os

import numpy as np

import oracle_lib as O

_CODE = {65: 0, 67: 1, 71: 2, 84: 3}
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def encode23(b: bytes) -> int:
    """get_dna23_bitset (kmers.cpp:12-40): two bits per byte, first byte most significant, anything but upper-case ACGT counts as A."""
    code = 0
    for c in b:
        code = (code << 2) | _CODE.get(c, 0)
    return code


def decode23(code: int) -> bytes:
    return bytes(b"ACGT"[(code >> (2 * (22 - i))) & 3] for i in range(23))


def rc_bytes(b: bytes) -> bytes:
    """decode(reverseDNA(sanitised code)): the reverse complement with every byte outside ACGT read as A."""
    return decode23(encode23(b)).translate(_COMP)[::-1]


def revcomp(s: bytes) -> bytes:
    return s.translate(_COMP)[::-1]


class Ref:
    def __init__(self, prefix: str, indices=None, positions=None, reads: bytes = None, ridx=None):
        z = np.load(os.path.join(os.path.dirname(prefix), "aindex.npz")) if indices is None or positions is None else None
        self.orc = O.OracleIndex23.from_prefix(prefix)
        self.checker = self.orc.checker().tolist()
        self.n = len(self.checker)
        self.indices = (z["indices"] if indices is None else np.asarray(indices)).tolist()
        self.positions = (z["index"] if positions is None else np.asarray(positions)).tolist()
        self.reads = open(prefix + ".reads", "rb").read() if reads is None else reads
        t = np.loadtxt(prefix + ".ridx", dtype=np.uint64).reshape(-1, 3) if ridx is None else np.asarray(ridx, dtype=np.uint64).reshape(-1, 3)
        self.rid, self.start, self.end = t[:, 0].tolist(), t[:, 1].tolist(), t[:, 2].tolist()
        self._memo = {}

    def bucket(self, w: bytes):
        """get_pfid: slot of the strand looked up, or None"""
        code = encode23(w)
        rev = rc_bytes(w)
        s, want = (w, code) if w <= rev else (rev, encode23(rev))
        h = self.orc.hash(s)
        return h if h < self.n and self.checker[h] == want else None

    def get_positions(self, w: bytes, max_per_kmer: int = 0):
        if w not in self._memo:                                  # long test sequences repeat their windows
            self._memo[w] = self.bucket(w)
        h = self._memo[w]
        if h is None:
            return []
        lo, hi = self.indices[h], min(self.indices[h + 1], len(self.positions))
        out = [p - 1 for p in self.positions[lo:hi] if p]
        return out[:max_per_kmer] if max_per_kmer else out

    def locate(self, pos: int):
        """(found, rid, start): the first interval with end + 1 >= pos, taken if start <= pos + 1"""
        i = bisect.bisect_left(self.end, pos - 1 if pos else 0)
        if i < len(self.end) and self.start[i] <= pos + 1:
            return True, self.rid[i], self.start[i]
        return False, 0, 0

    def strand(self, w: bytes, pos: int) -> int:
        if pos + 23 > len(self.reads):
            return 2
        t = self.reads[pos:pos + 23]
        return 0 if t == w else (1 if t == rc_bytes(w) else 2)

    def hits(self, seq: bytes, max_per_kmer: int = 0):
        """[(qoff, pos, rid, local, flag)] by window, then slot"""
        out = []
        for q in range(max(0, len(seq) - 22)):
            w = seq[q:q + 23]
            for pos in self.get_positions(w, max_per_kmer):
                found, rid, start = self.locate(pos)
                out.append((q, pos, rid, pos - start, self.strand(w, pos) | (4 if found else 0)))
        return out

    def votes(self, seq: bytes, min_votes: int = 1, max_per_kmer: int = 0):
        """[(rid, strand, diag, votes, q_first, q_last)] ascending"""
        groups = {}
        for q, pos, rid, local, flag in self.hits(seq, max_per_kmer):
            st = flag & 3
            if st == 2 or not flag & 4:
                continue
            groups.setdefault((rid, st, local - q if st == 0 else local + q), []).append(q)
        return [(r, s, d, len(qs), min(qs), max(qs)) for (r, s, d), qs in sorted(groups.items()) if len(qs) >= min_votes]


def hits_csr(ref: Ref, seqs, max_per_kmer: int = 0):
    """the arrays of Index.seq_hits"""
    per = [ref.hits(s, max_per_kmer) for s in seqs]
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(h) for h in per], dtype=np.uint64)
    flat = [h for hs in per for h in hs]
    cols = list(zip(*flat)) if flat else [[]] * 5
    return (off, np.asarray(cols[0], np.uint32), np.asarray(cols[1], np.uint64), np.asarray(cols[2], np.uint64), np.asarray(cols[3], np.int64),
            np.asarray(cols[4], np.uint8))


def votes_csr(ref: Ref, seqs, min_votes: int = 1, max_per_kmer: int = 0):
    """the arrays of Index.seq_votes"""
    per = [ref.votes(s, min_votes, max_per_kmer) for s in seqs]
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(v) for v in per], dtype=np.uint64)
    flat = [v for vs in per for v in vs]
    cols = list(zip(*flat)) if flat else [[]] * 6
    return (off, np.asarray(cols[0], np.uint64), np.asarray(cols[1], np.uint8), np.asarray(cols[2], np.int64), np.asarray(cols[3], np.uint32),
            np.asarray(cols[4], np.uint32), np.asarray(cols[5], np.uint32))


def standard_queries(prefix: str):
    """The query set of the GPU tests: 40 indexed reads as stored, the reverse complements of 20, two slices of the synthetic genome, a
    lower-case read, a read with N ~ newline and bytes >= 0x80 planted, and lengths 0, 22, 23, 24."""
    from aindex_amd import synth
    reads = open(prefix + ".reads", "rb").read()
    ridx = np.loadtxt(prefix + ".ridx", dtype=np.int64).reshape(-1, 3)
    rows = [r for r in ridx if r[2] + 23 < 51612][:120:3]               # the positions array stops at 51 612: indexed reads only
    plain = [reads[int(r[1]):int(r[2])] for r in rows]
    assert len(plain) == 40
    g = synth.genome_ascii(1, 3000).tobytes()
    dirty = bytearray(plain[5])
    dirty[30], dirty[60], dirty[61], dirty[90], dirty[120] = ord("N"), ord("~"), ord("\n"), 0x80, 0xFF
    qs = plain + [revcomp(s) for s in plain[:20]] + [g[100:400], revcomp(g[500:760]), plain[7].lower(), bytes(dirty),
                                                      b"", plain[0][:22], plain[0][:23], plain[1][3:27]]
    return qs
