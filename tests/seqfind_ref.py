"""Sequences with mismatches against the indexed reads, restated in plain Python for the tests (no GPU): the semantics that
include/aindex_hip.h fixes for aix_seq_find / aix_kmer_strands (the reference documents the layer, API_DOCUMENTATION.md:232-255,371-382,
and holds no code for it; hamming_distance is aindex.py:44-46), over the seed hits of seqhits_ref.Ref, and a brute-force Hamming search
over all reads that knows nothing of seeds.

Seeds of a sequence of length L >= 23: its 23-windows at offsets 0, seed_step, 2 seed_step, .. <= L - 23 (seed_step 0 means 23). The hits
of a seed are Ref.get_positions of the window (cap included) whose strand (Ref.strand) is 0 or 1. A hit (q, pos, strand) proposes the
alignment at a = pos - q (strand 0) or pos - (L - 23 - q) (strand 1); dropped when a < 0, a + L > len(reads), or no interval has
start <= a and a + L <= end (plain containment). d = mismatches of reads[a:a + L] against the sequence (strand 0) or its reverse complement
(strand 1; A<->T C<->G a<->t c<->g, other bytes unchanged), positions with an N on either side ignored. Reported when d <= hd, each
(a, strand) once, ascending: (a, rid, a - start, strand, d)."""
import bisect

import numpy as np

import seqhits_ref as R

_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
N = ord("N")


def comp_rev(s: bytes) -> bytes:
    return s.translate(_COMP)[::-1]


def hamming(x: bytes, y: bytes) -> int:
    """hamming_distance (aindex.py:44-46) on raw bytes"""
    return sum(1 for a, b in zip(x, y) if a != b and a != N and b != N)


class FindRef(R.Ref):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        assert all(s > e for s, e in zip(self.start[1:], self.end[:-1])), "intervals sorted and disjoint"

    def interval(self, a: int, L: int):
        """index of the interval with start <= a and a + L <= end, or None"""
        i = bisect.bisect_right(self.start, a) - 1
        return i if i >= 0 and a + L <= self.end[i] else None

    def proposals(self, seq: bytes, seed_step: int = 23, max_per_kmer: int = 0):
        """{(a, strand): number of seeds that proposed it}; a may be negative or reach beyond the reads"""
        L, step, out = len(seq), seed_step or 23, {}
        for q in range(0, L - 22, step):
            w = seq[q:q + 23]
            for pos in self.get_positions(w, max_per_kmer):
                st = self.strand(w, pos)
                if st < 2:
                    key = (pos - q if st == 0 else pos - (L - 23 - q), st)
                    out[key] = out.get(key, 0) + 1
        return out

    def find(self, seq: bytes, hd: int = 0, seed_step: int = 23, max_per_kmer: int = 0, stats: dict = None):
        """[(a, rid, local, strand, dist)] ascending by (a, strand). stats (optional) counts: proposed, multi (proposed by >= 2 seeds),
        bounds (a < 0 or a + L beyond the reads), boundary (no interval contains it), rejected (d > hd)."""
        L, out = len(seq), []
        st_ = stats if stats is not None else {}
        rc = comp_rev(seq)
        for (a, strand), n in sorted(self.proposals(seq, seed_step, max_per_kmer).items()):
            st_["proposed"] = st_.get("proposed", 0) + 1
            if a < 0 or a + L > len(self.reads):
                st_["bounds"] = st_.get("bounds", 0) + 1
                continue
            i = self.interval(a, L)
            if i is None:
                st_["boundary"] = st_.get("boundary", 0) + 1
                continue
            if n >= 2:
                st_["multi"] = st_.get("multi", 0) + 1
            d = hamming(self.reads[a:a + L], rc if strand else seq)
            if d <= hd:
                out.append((a, self.rid[i], a - self.start[i], strand, d))
            else:
                st_["rejected"] = st_.get("rejected", 0) + 1
        return out

    def brute(self, seq: bytes, hd: int):
        """The full Hamming search: every (a, strand) with [a, a + L) inside one interval and d <= hd, in the order and shape of find().
        numpy over all windows of the reads file; no seeds."""
        L = len(seq)
        if L == 0 or L > len(self.reads):
            return []
        buf = np.frombuffer(self.reads, dtype=np.uint8)
        win = np.lib.stride_tricks.sliding_window_view(buf, L)
        inside = np.zeros(win.shape[0], bool)
        owner = np.zeros(win.shape[0], np.int64)
        for i, (s, e) in enumerate(zip(self.start, self.end)):
            if e - s >= L:
                inside[s:e - L + 1] = True
                owner[s:e - L + 1] = i
        idx = np.nonzero(inside)[0]
        out = []
        for strand, pat in ((0, seq), (1, comp_rev(seq))):
            y = np.frombuffer(pat, dtype=np.uint8)
            w = win[idx]
            d = ((w != y) & (w != N) & (y != N)).sum(axis=1)
            for a, dd in zip(idx[d <= hd].tolist(), d[d <= hd].tolist()):
                i = int(owner[a])
                out.append((a, self.rid[i], a - self.start[i], strand, dd))
        return sorted(out, key=lambda r: (r[0], r[3]))

    def strands(self, kmer: bytes, max_per_kmer: int = 0):
        """(plus, minus, total) of the listed hits of a 23-mer"""
        ps = self.get_positions(kmer, max_per_kmer) if len(kmer) == 23 else []
        st = [self.strand(kmer, p) for p in ps]
        return st.count(0), st.count(1), len(st)

    def reads_by_sequence(self, seq: bytes, hd=None):
        """iter_reads_by_sequence: per read, rid ascending, (rid, poses[0], read, poses[, smallest distance])"""
        per = {}
        for a, rid, local, strand, d in self.find(seq, hd or 0):
            e = per.setdefault(rid, [set(), d])
            e[0].add(local)
            e[1] = min(e[1], d)
        out = []
        for rid in sorted(per):
            i = self.rid.index(rid)
            read = self.reads[self.start[i]:self.end[i]].decode("latin-1")
            poses = sorted(per[rid][0])
            out.append((rid, poses[0], read, poses, per[rid][1]) if hd else (rid, poses[0], read, poses))
        return out

    def reads_by_kmer(self, kmer: bytes):
        """iter_reads_by_kmer: get_rid2poses (Ref.locate per occurrence) with rid ascending, poses ascending, pos = poses[0]"""
        per = {}
        for p in self.get_positions(kmer):
            _, rid, start = self.locate(p)
            per.setdefault(rid, []).append(p - start)
        out = []
        for rid in sorted(per):
            i = self.rid.index(rid)
            poses = sorted(per[rid])
            out.append((rid, poses[0], self.reads[self.start[i]:self.end[i]].decode("latin-1"), poses))
        return out


def find_csr(ref: FindRef, seqs, hd: int = 0, seed_step: int = 23, max_per_kmer: int = 0):
    """the arrays of Index.seq_find"""
    per = [ref.find(s, hd, seed_step, max_per_kmer) for s in seqs]
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(p) for p in per], dtype=np.uint64)
    flat = [x for p in per for x in p]
    cols = list(zip(*flat)) if flat else [[]] * 5
    return (off, np.asarray(cols[0], np.uint64), np.asarray(cols[1], np.uint64), np.asarray(cols[2], np.uint64), np.asarray(cols[3], np.uint8),
            np.asarray(cols[4], np.uint32))


LENGTHS = (23, 24, 46, 69, 70, 100, 150)
_SUB = {65: 67, 67: 71, 71: 84, 84: 65}                       # A -> C -> G -> T -> A: a planted byte always differs from the genome's


def plant(seq: bytes, where) -> bytes:
    b = bytearray(seq)
    for j in where:
        b[j] = _SUB[b[j]]
    return bytes(b)


def standard_patterns():
    """The pattern set of the GPU tests: slices of the synthetic genome that the reads of small23 were cut from, of the lengths above, every
    second one reverse-complemented, each with 0 - 3 planted substitutions (the planted count is the expected distance: the reads are
    error-free), among them j = 0 and j = L - 1, and one with an N. [(pattern, planted)]."""
    from aindex_amd import synth
    g = synth.genome_ascii(1, 3000).tobytes()
    out, k = [], 0
    for s in range(0, 2840, 47):
        for L in LENGTHS:
            p = g[s:s + L]
            n = k % 4
            where = [[], [L // 2], [0, L - 1], [0, L // 3, L - 1]][n]
            p = plant(p, where)
            if k % 2:
                p = comp_rev(p)
            out.append((p, n))
            k += 1
    first = bytearray(out[5][0])                               # L = 100, planted 1 at L // 2, reverse-complemented: an N on top
    first[10] = N
    out[5] = (bytes(first), out[5][1])
    return out


def strand_kmers(pats):
    """The k-mers of the strand-count test: the first 23-window of 200 standard patterns, the reverse complement of 40 of them, one of N
    only and one that no read holds."""
    return [p[:23] for p in pats[:200]] + [comp_rev(p[:23]) for p in pats[:40]] + [b"N" * 23, b"ACGT" * 5 + b"ACG"]


def read_search_patterns(pats):
    """The patterns of the iter_reads_by_sequence test: every fifth standard pattern, so all lengths and all planted counts 0 - 3"""
    return pats[7:120:5]
