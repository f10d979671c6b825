"""AIndex — counterpart of the reference's pure-Python `aindex.core.aindex.AIndex`
(aindex/core/aindex.py:48-793) for the tf / coverage path, backed by the MI355X engine.

Same public names and behaviour for every member of the reference class: load_hash / load_13mer_index /
load_from_prefix* / load_aindex / load_reads / load_reads_index, get_tf_value(s), get_hash_value(s), get_kid_by_kmer,
get_kmer_by_kid, get_strand, get_kmer_info, __getitem__/__contains__/get/__len__, iter_sequence_kmers,
get_sequence_coverage (one kernel launch instead of a Python loop), 13-mer array access, positions and reads access
(get_positions / pos / get_rid / get_start / get_read* / get_rid2poses / iter_reads*, pinned against the reference's
compiled module in tests/golden/small23/access.json), get_header, k-mers by frequency. Documented deviations:
load_from_prefix auto-detect tests `.kmers.bin` first (the reference's order always selects 13-mer mode);
kmer_type="auto" follows the loaded mode (the reference's probe always lands on "13mer"); get_reads_by_kmer returns the
reads holding an indexed occurrence (the reference's implementation reads its two arrays crossed: undefined behaviour).
"""
from __future__ import annotations

import logging
import os
from collections import Counter
from enum import IntEnum
from typing import Iterator, List, Optional, Tuple

import numpy as np

from . import _lib
from .wrapper import AindexWrapper

logger = logging.getLogger(__name__)


class Strand(IntEnum):            # aindex.py:29-32
    NOT_FOUND = 0
    FORWARD = 1
    REVERSE = 2


def hamming_distance(s1: str, s2: str) -> int:
    """aindex.py:44-46 — mismatches over the common prefix, positions holding an N on either side ignored."""
    return sum(1 for a, b in zip(s1, s2) if a != b and a != "N" and b != "N")


def edit_distance(s1: str, s2: str) -> int:
    """aindex.py:22 re-exports editdistance.eval under this name: plain Levenshtein distance (unit costs, no N rule), on the host."""
    if len(s1) < len(s2):
        s1, s2 = s2, s1
    row = list(range(len(s2) + 1))
    for i, a in enumerate(s1, 1):
        diag, row[0] = row[0], i
        for j, b in enumerate(s2, 1):
            diag, row[j] = row[j], min(diag + (a != b), row[j] + 1, row[j - 1] + 1)
    return row[-1]


def get_revcomp(sequence: str) -> str:
    c = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N", "a": "t", "c": "g", "g": "c", "t": "a", "n": "n", "~": "~", "[": "]", "]": "["}
    return "".join(c.get(x, x) for x in reversed(sequence))


def unitig_link_pairs(links: dict) -> List[Tuple[int, str, int, str]]:
    """[(a, '+' | '-', b, '+' | '-')] of Index.unitig_links: one tuple per dual pair of links — (e, t) is written iff (e, t) <= (t ^ 1, e ^ 1)
    as tuples, so a self-dual link appears once —, ascending by (e, position among the links of e)."""
    off = np.asarray(links["link_off"]).astype(np.int64)
    to = np.asarray(links["link_to"]).astype(np.int64)
    e = np.repeat(np.arange(off.shape[0] - 1, dtype=np.int64), np.diff(off))
    keep = e <= (to ^ 1)                                            # e == t ^ 1 makes t == e ^ 1: the second components tie
    return [(a >> 1, "+-"[a & 1], b >> 1, "+-"[b & 1]) for a, b in zip(e[keep].tolist(), to[keep].tolist())]


def format_gfa(unitigs: dict, links: dict) -> Iterator[str]:
    """The lines (no line ends) of a GFA 1 file of the unitig graph: the header, one S line per unitig of Index.unitigs (named u{id}, with
    LN = bases, KC = tf_sum, km = tf_sum / k-mers), one L line with overlap 22M per tuple of unitig_link_pairs, and the closing link
    u{c} + -> u{c} + of every circular unitig. Host only."""
    yield "H\tVN:Z:1.0"
    off, text = np.asarray(unitigs["offsets"]).astype(np.int64).tolist(), np.asarray(unitigs["bases"]).tobytes().decode("ascii")
    circular = np.asarray(unitigs["circular"]).tolist()
    for i, s in enumerate(np.asarray(unitigs["tf_sum"]).tolist()):
        ln = off[i + 1] - off[i]
        yield f"S\tu{i}\t{text[off[i]:off[i + 1]]}\tLN:i:{ln}\tKC:i:{s}\tkm:f:{s / (ln - 22):.1f}"
    for a, sa, b, sb in unitig_link_pairs(links):
        yield f"L\tu{a}\t{sa}\tu{b}\t{sb}\t22M"
    for i, c in enumerate(circular):
        if c:
            yield f"L\tu{i}\t+\tu{i}\t+\t22M"


def format_vcf(variants, contig_lengths=None) -> Iterator[str]:
    """The lines (no line ends) of a VCF 4.2 file of the variant sites of AIndex.get_variants, [(contig, pos, ref, alt, ref_count,
    alt_count, depth)]: the header (one ##contig line per entry of contig_lengths, when given), then per site c{id}, the 1-based
    position, '.', REF, ALT, '.', '.', and DP={depth};AD={ref_count},{alt_count}. Host only."""
    yield "##fileformat=VCFv4.2"
    for i, ln in enumerate(contig_lengths if contig_lengths is not None else ()):
        yield f"##contig=<ID=c{i},length={ln}>"
    yield '##INFO=<ID=DP,Number=1,Type=Integer,Description="Reads piled on the base">'
    yield '##INFO=<ID=AD,Number=R,Type=Integer,Description="Reads showing the contig base and the alternative base">'
    yield "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"
    for c, pos, ref, alt, rn, an, dp in variants:
        yield f"c{c}\t{pos + 1}\t.\t{ref}\t{alt}\t.\t.\tDP={dp};AD={rn},{an}"


def format_vcf_phased(variants, contig_lengths=None, sample: str = "sample") -> Iterator[str]:
    """The lines of format_vcf for the rows of AIndex.get_phased_variants, [(contig, pos, ref, alt, ref_count, alt_count, depth, block,
    phase)], plus a FORMAT column GT:PS and one sample: 0|1 (phase 0: the alternative base on haplotype 1) or 1|0 with PS the 1-based
    position of the first site of the block, and 0/1:. for an unphased site. Host only."""
    variants = list(variants)
    tails = iter(["GT:PS\t0/1:." if p is None else f"GT:PS\t{'1|0' if p else '0|1'}:{b + 1}" for *_, b, p in variants])
    for line in format_vcf([v[:7] for v in variants], contig_lengths):
        if line.startswith("#CHROM"):
            yield '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">'
            yield '##FORMAT=<ID=PS,Number=1,Type=Integer,Description="Phase set: the position of the first site of the phase block">'
            yield f"{line}\tFORMAT\t{sample}"
        elif line.startswith("#"):
            yield line
        else:
            yield f"{line}\t{next(tails)}"


def format_gfa_paths(unitigs: dict, links: dict, support, thread: dict, names: List[str]) -> Iterator[str]:
    """format_gfa with the read evidence of Index.seq_thread: every L line carries RC:i:{support of the link} (the closing link of a
    circular unitig: the number of times a step wound round it), and one P line per maximal stretch of linked steps of every sequence —
    named names[i], then names[i].2, .. —, its segments as u{id}+ / u{id}-, with * for the overlaps. A step of one unitig alone is a
    stretch too. unitigs / links / support / thread: numpy arrays (u64 / u32) of one graph. Host only."""
    off = np.asarray(unitigs["offsets"]).astype(np.int64)
    lo = np.asarray(links["link_off"]).astype(np.int64)
    to = np.asarray(links["link_to"]).astype(np.int64)
    e = np.repeat(np.arange(lo.shape[0] - 1, dtype=np.int64), np.diff(lo))
    kept = np.asarray(support)[e <= (to ^ 1)].tolist()              # the links unitig_link_pairs writes, in its order
    su, sp, sf = (np.asarray(thread[k]).astype(np.int64) for k in ("step_unitig", "step_pos", "step_flag"))
    span = np.asarray(thread["q_last"]).astype(np.int64) - np.asarray(thread["q_first"]).astype(np.int64) + 1
    m = (np.diff(off) - 22)[su] if su.shape[0] else su
    ahead = np.where(sf & 1, m - 1 - sp, sp)                        # k-mers between the start of the traversal and the first window
    wraps = np.bincount(su, weights=(ahead + span - 1) // np.maximum(m, 1), minlength=off.shape[0] - 1).astype(np.int64).tolist() if su.shape[0] else []
    n_link = 0
    for line in format_gfa(unitigs, links):
        if line[0] == "L":
            if n_link < len(kept):
                line += f"\tRC:i:{kept[n_link]}"
            else:
                line += f"\tRC:i:{wraps[int(line.split(chr(9))[1][1:])] if wraps else 0}"
            n_link += 1
        yield line
    sso = np.asarray(thread["seq_step_off"]).astype(np.int64).tolist()
    linked = (np.asarray(thread["step_link"]) < np.uint64(_lib.THREAD_BROKEN)).tolist()
    seg = [f"u{u}{'-' if f & 1 else '+'}" for u, f in zip(su.tolist(), sf.tolist())]
    for i, name in enumerate(names):
        part, start = 1, sso[i]
        for j in range(sso[i] + 1, sso[i + 1] + 1):
            if j == sso[i + 1] or not linked[j]:
                if j > start:
                    yield f"P\t{name if part == 1 else f'{name}.{part}'}\t{','.join(seg[start:j])}\t*"
                    part += 1
                start = j


def _records(g: dict, text: Optional[str], min_kmers: int) -> Iterator[Tuple[int, str, int, bool]]:
    """(id, sequence, tf_sum, circular) of the unitigs of `g` (numpy arrays offsets, bases, tf_sum, circular) with at least min_kmers
    k-mers, in order; text: the bases to cut the sequences from when they are not g's own."""
    off, text = g["offsets"].tolist(), g["bases"].tobytes().decode("ascii") if text is None else text
    for i, (s, c) in enumerate(zip(g["tf_sum"].tolist(), g["circular"].tolist())):
        if off[i + 1] - off[i] - 22 >= min_kmers:
            yield i, text[off[i]:off[i + 1]], s, bool(c)


def _contig_rows(g: dict, text: Optional[str] = None, min_kmers: int = 1) -> List[Tuple[str, int, bool]]:
    """[(sequence, tf_sum, circular)] of _records"""
    return [r[1:] for r in _records(g, text, min_kmers)]


def _write_fasta(path: str, prefix: str, g: dict, text: Optional[str] = None, min_kmers: int = 1, suffix=None) -> int:
    """One record >{prefix}{id} LN:i:{len} KC:i:{tf_sum} km:f:{tf_sum/m:.1f}[ circular]{suffix(id)} per entry of _records; returns the number
    of records written."""
    written = 0
    with open(path, "w") as f:
        for i, seq, s, c in _records(g, text, min_kmers):
            ln = len(seq)
            f.write(f">{prefix}{i} LN:i:{ln} KC:i:{s} km:f:{s / (ln - 22):.1f}{' circular' if c else ''}{suffix(i) if suffix else ''}\n{seq}\n")
            written += 1
    return written


def _write_lines(path: str, lines) -> Counter:
    """`lines` written with line ends; returns how many of them begin with each character."""
    first = Counter()
    with open(path, "w") as f:
        for line in lines:
            first[line[0]] += 1
            f.write(line + "\n")
    return first


def iter_reads_by_kmer(kmer: str, aindex: "AIndex", k: int = 23):
    """API_DOCUMENTATION.md:238-243 — yields (rid, pos, read, poses) per read that holds an indexed occurrence of the k-mer, rid ascending;
    poses = the offsets of the k-mer inside the read, ascending, pos = poses[0]. get_rid2poses_batch + get_reads_by_rid_batch: two GPU calls."""
    hits = aindex.get_rid2poses_batch([kmer[:k]])[0]
    rids = sorted(hits)
    for rid, read in zip(rids, aindex.get_reads_by_rid_batch(rids)):
        poses = sorted(hits[rid])
        yield rid, poses[0], read, poses


def iter_reads_by_sequence(sequence: str, aindex: "AIndex", hd: Optional[int] = None, k: int = 23):
    """API_DOCUMENTATION.md:245-246, 371-378 — yields per read that holds the sequence, rid ascending, (rid, pos, read, poses) when hd is
    falsy (exact matches, N positions forgiven) and (rid, pos, read, poses, distance) otherwise (at most hd mismatches): poses = where
    the sequence starts in the read, either strand, ascending and distinct; pos = poses[0]; distance = the smallest of the read's
    alignments. k must be 23, the seed length of AIndex.find_sequences_array."""
    if k != 23:
        raise ValueError("iter_reads_by_sequence seeds with 23-mers: k must be 23")
    _, _, rid, local, _, dist = aindex.find_sequences_array([sequence], hd or 0)
    per = {}
    for r, l, d in zip(rid.tolist(), local.tolist(), dist.tolist()):
        e = per.setdefault(r, [set(), d])
        e[0].add(l)
        e[1] = min(e[1], d)
    rids = sorted(per)
    for r, read in zip(rids, aindex.get_reads_by_rid_batch(rids)):
        poses = sorted(per[r][0])
        yield (r, poses[0], read, poses, per[r][1]) if hd else (r, poses[0], read, poses)


def get_srandness(kmer: str, aindex: "AIndex", k: int = 23) -> Tuple[int, int, int]:
    """API_DOCUMENTATION.md:234-236, 379-381 — (plus, minus, total) of the k-mer's indexed occurrences: the reads hold it as given,
    hold its reverse complement, all listed occurrences. (The reference's spelling of the name.)"""
    return aindex.get_strandness_batch([kmer[:k]])[0]


class AIndex:
    def __init__(self, device: int = 0):
        self._wrapper = AindexWrapper(device)
        self._loaded = False
        self.reads_size = 0
        self.max_tf = 0
        self.loaded_header = False                                # aindex.py:55-61
        self.loaded_intervals = False
        self.loaded_reads = False
        self.rid2start = {}
        self.chrm2start = {}
        self.headers = {}
        self._hdr_start = np.zeros(0, dtype=np.int64)             # header intervals [start, start + length), file order
        self._hdr_end = np.zeros(0, dtype=np.int64)

    # ---- loading -----------------------------------------------------------------------------
    def load_hash(self, hash_file: str, tf_file: str, kmers_bin_file: str, kmers_text_file: str = ""):
        for f in (hash_file, tf_file, kmers_bin_file):           # aindex.py:63-79
            if not os.path.exists(f):
                raise FileNotFoundError(f"File not found: {f}")
        self._wrapper.load(hash_file, tf_file, kmers_bin_file, kmers_text_file)
        self._loaded = True

    load_hash_file = load_hash

    def load_13mer_index(self, hash_file: str, tf_file: str):
        if not os.path.exists(hash_file):
            raise FileNotFoundError(f"13-mer hash file not found: {hash_file}")
        if not os.path.exists(tf_file):
            raise FileNotFoundError(f"13-mer tf file not found: {tf_file}")
        self._wrapper.load_13mer_index(hash_file, tf_file)
        self._loaded = True

    @staticmethod
    def load_13mer_index_static(hash_file: str, tf_file: str, device: int = 0) -> "AIndex":
        ix = AIndex(device)
        ix.load_13mer_index(hash_file, tf_file)
        return ix

    @staticmethod
    def load_23mer_index(hash_file: str, tf_file: str, kmers_bin_file: str, kmers_text_file: str = "", device: int = 0) -> "AIndex":
        ix = AIndex(device)
        ix.load_hash(hash_file, tf_file, kmers_bin_file, kmers_text_file)
        return ix

    @staticmethod
    def load_from_prefix(prefix: str, kmer_size: Optional[int] = None, max_tf: int = 100000, load_aindex: bool = True,
                         load_reads: bool = False, device: int = 0) -> "AIndex":
        ix = AIndex(device)
        if kmer_size is None:
            pf, tf, kb = f"{prefix}.pf", f"{prefix}.tf.bin", f"{prefix}.kmers.bin"
            if os.path.exists(pf) and os.path.exists(tf) and os.path.exists(kb):
                kmer_size = 23                                   # deviation: .kmers.bin is tested first
            elif os.path.exists(pf) and os.path.exists(tf):
                kmer_size = 13
            else:
                raise FileNotFoundError(f"Could not auto-detect k-mer size for prefix '{prefix}'")
        reads_file = ""
        if load_reads:                                           # aindex.py:478-487: <prefix>.reads, else without the .23. / .13. infix
            reads_file = f"{prefix}.reads"
            if not os.path.exists(reads_file):
                reads_file = reads_file.replace(".23.", ".").replace(".13.", ".")
                if not os.path.exists(reads_file):
                    logger.warning(f"Reads file not found: {reads_file}")
                    reads_file = ""
        if kmer_size == 13:
            ix.load_from_prefix_13mer(prefix, load_aindex=load_aindex, reads_file=reads_file)
        elif kmer_size == 23:
            ix.load_from_prefix_23mer(prefix, max_tf=100000 if max_tf is None else max_tf, load_aindex=load_aindex, reads_file=reads_file)
        else:
            raise ValueError(f"Unsupported kmer size: {kmer_size}. Only 13 and 23 are supported.")
        return ix

    def load_from_prefix_23mer(self, prefix: str, max_tf: int = 100, load_aindex: bool = True, reads_file: str = ""):
        """aindex.py:501-521. A missing positions index is a warning here (the reference's C++ loader calls std::terminate())."""
        self._wrapper.load_from_prefix_23mer(prefix, reads_file)
        self._loaded = True
        self._after_reads()
        if load_aindex:
            try:
                self._wrapper.load_aindex_from_prefix_23mer(prefix, max_tf, reads_file)
                self.max_tf = max_tf
            except Exception as e:
                logger.warning(f"Could not load 23-mer AIndex from prefix {prefix}: {e}")

    def load_from_prefix_13mer(self, prefix: str, load_aindex: bool = True, reads_file: str = ""):
        self._wrapper.load_from_prefix_13mer(prefix, reads_file)                       # aindex.py:523-543
        self._loaded = True
        self._after_reads()
        if load_aindex:
            try:
                self._wrapper.load_aindex_from_prefix_13mer(prefix, reads_file)
            except Exception as e:
                logger.warning(f"Could not load 13-mer AIndex from prefix {prefix}: {e}")

    def _after_reads(self):
        self.reads_size = self._wrapper.reads_size
        self.loaded_reads = self.reads_size > 0

    # ---- queries -----------------------------------------------------------------------------
    def get_tf_value(self, kmer: str) -> int:
        return self._wrapper.get_tf_value(kmer) if self._loaded else 0

    def get_tf_values(self, kmers: List[str]) -> List[int]:
        return self._wrapper.get_tf_values(kmers) if self._loaded else [0] * len(kmers)

    def get_tf_values_13mer(self, kmers: List[str]) -> List[int]:
        return self._wrapper.get_tf_values_13mer(kmers) if self._loaded else [0] * len(kmers)

    def get_tf_values_array(self, kmers_u8) -> np.ndarray:
        """(N, k) uint8 ASCII -> uint32 tf, no Python objects on the way."""
        return self._wrapper.get_tf_values_array(kmers_u8)

    def _req(self):
        if not self._loaded:
            raise RuntimeError("Index not loaded")

    def get_hash_value(self, kmer: str) -> int:
        self._req()
        return self._wrapper.get_hash_value(kmer)

    def get_hash_values(self, kmers: List[str]) -> List[int]:
        self._req()
        return self._wrapper.get_hash_values(kmers)

    def get_kid_by_kmer(self, kmer: str) -> int:
        self._req()
        return self._wrapper.get_kid_by_kmer(kmer)

    def get_kmer_by_kid(self, kid: int) -> str:
        self._req()
        return self._wrapper.get_kmer_by_kid(kid)

    def get_strand(self, kmer: str) -> Strand:
        self._req()
        return Strand(self._wrapper.get_strand(kmer))

    def get_kmer_info(self, kid: int) -> Tuple[str, str, int]:
        self._req()                                              # aindex.py:195-207 -> (kmer, rkmer, tf)
        kmer = self.get_kmer_by_kid(kid)
        return kmer, get_revcomp(kmer), self.get_tf_value(kmer)

    def get_kmer_info_by_kid(self, kid: int, k: int = 23):
        return self.get_kmer_info(kid)

    def get_hash_size(self) -> int:
        self._req()
        return self._wrapper.get_hash_size()

    def get_reads_size(self) -> int:
        return self._wrapper.get_reads_size()

    def __len__(self) -> int:
        return self.get_hash_size()

    def __getitem__(self, kmer: str) -> int:
        return self.get_tf_value(kmer)

    def __contains__(self, kmer: str) -> bool:
        return self[kmer] > 0

    def get(self, kmer: str, default: int = 0) -> int:
        tf = self[kmer]
        return tf if tf > 0 else default

    def iter_sequence_kmers(self, sequence: str, k: int = 23):
        kmers = [sequence[i:i + k] for i in range(len(sequence) - k + 1)]     # aindex.py:306-312, one batch call
        kmers = [s for s in kmers if "\n" not in s and "~" not in s]
        for s, tf in zip(kmers, self.get_tf_values(kmers)):
            yield s, tf

    def get_sequence_coverage(self, seq: str, cutoff: int = 0, k: int = 23) -> list:
        """aindex.py:314-322. Every window goes through get_tf_value in the reference, i.e. the mode's
        own k decides what can match; windows are k bytes long."""
        return self.get_sequences_coverage([seq], cutoff, k)[0].tolist()

    def get_sequences_coverage(self, seqs: List[str], cutoff: int = 0, k: int = 23) -> List[np.ndarray]:
        if not self._loaded:
            return [np.zeros(max(0, len(s) - k + 1), dtype=np.uint32) for s in seqs]
        w = self._wrapper
        ix = w._ix13 if w._is_13mer_mode else w._ix23
        if ix is not None and ix.k == k:
            return ix.coverage(seqs, cutoff)
        # window length differs from the index's k: the reference's get_tf_value then sees strings of
        # the wrong length — go through the exact ragged path
        out = []
        for s in seqs:
            wins = [s[i:i + k] for i in range(len(s) - k + 1)]
            tf = np.array(self.get_tf_values(wins), dtype=np.uint32) if wins else np.zeros(0, dtype=np.uint32)
            tf[tf < cutoff] = 0
            out.append(tf)
        return out

    def print_sequence_coverage(self, seq: str, cutoff: int = 0):
        for i, tf in enumerate(self.get_sequence_coverage(seq, cutoff)):
            print(i, seq[i:i + 23], tf)

    # ---- reads + positions index (N2 tier: thin calls into the wrapper, aindex.py:88-133,162-181,271-343) ----------
    def load_reads(self, reads_file: str):
        if not os.path.exists(reads_file):
            raise FileNotFoundError(f"Reads file not found: {reads_file}")
        self._wrapper.load_reads(reads_file)
        self.reads_size = self._wrapper.reads_size
        self.loaded_reads = True

    def load_aindex(self, index_file: str, indices_file: str, max_tf: int):
        for name, path in (("index", index_file), ("indices", indices_file)):
            if not os.path.exists(path):
                raise FileNotFoundError(f"{name} file not found: {path}")
        self._wrapper.load_aindex(index_file, indices_file, max_tf)
        self.max_tf = max_tf

    def load_13mer_aindex(self, index_file: str, indices_file: str):
        for name, path in (("index", index_file), ("indices", indices_file)):
            if not os.path.exists(path):
                raise FileNotFoundError(f"{name} file not found: {path}")
        self._wrapper.load_13mer_aindex(index_file, indices_file)

    def load_reads_index(self, index_file: str, header_file: Optional[str] = None):
        """aindex.py:101-130 — `.ridx` lines "rid<TAB>start<TAB>end" and, optionally, `.header` lines
        "head<TAB>start<TAB>length". The reference keeps both in one IntervalTree; here they are two sorted arrays."""
        self.rid2start, self.chrm2start, self.headers = {}, {}, {}
        with open(index_file) as fh:
            for line in fh:
                rid, start, end = line.rstrip("\n").split("\t")
                self.rid2start[int(rid)] = (int(start), int(end))
        self._wrapper.load_reads_index(index_file)
        self.loaded_intervals = True
        if header_file:
            starts, ends = [], []
            with open(header_file) as fh:
                for rid, line in enumerate(fh):
                    head, start, length = line.rstrip("\n").split("\t")
                    self.headers[rid] = head
                    self.chrm2start[head.split()[0].split(".")[0]] = int(start)
                    starts.append(int(start))
                    ends.append(int(start) + int(length))
            self._hdr_start = np.array(starts, dtype=np.int64)
            self._hdr_end = np.array(ends, dtype=np.int64)
            self.loaded_header = True

    def get_positions(self, kmer: str) -> List[int]:
        return self._wrapper.get_positions(kmer)

    def get_positions_13mer(self, kmer: str) -> List[int]:
        return self._wrapper.get_positions_13mer(kmer)

    def pos(self, kmer: str) -> List[int]:
        return self.get_positions(kmer)

    def get_read_by_rid(self, rid: int) -> str:
        return self._wrapper.get_read_by_rid(rid)

    def get_read(self, start: int, end: int, revcomp: bool = False) -> str:
        return self._wrapper.get_read(start, end, revcomp)

    def get_rid(self, pos: int) -> int:
        return self._wrapper.get_rid(pos)

    def get_start(self, pos: int) -> int:
        return self._wrapper.get_start(pos)

    def get_rid2poses(self, kmer: str) -> dict:
        """aindex.py:333-341 — read id -> offsets of the k-mer inside that read."""
        hits = {}
        for p in self.pos(kmer):
            hits.setdefault(self.get_rid(p), []).append(p - self.get_start(p))
        return hits

    def get_positions_batch(self, kmers) -> List[List[int]]:
        """[get_positions(s) for s in kmers], one GPU call."""
        return self._wrapper.get_positions_batch(kmers)

    def get_positions_array(self, kmers, max_per_kmer: int = 0, locate: bool = False):
        """CSR arrays (offsets, positions[, rid, offset_in_read]); see AindexWrapper.get_positions_array."""
        return self._wrapper.get_positions_array(kmers, max_per_kmer, locate)

    def get_rid2poses_batch(self, kmers) -> List[dict]:
        """[get_rid2poses(s) for s in kmers]: positions and reads resolved in one GPU call."""
        w = self._wrapper
        k = 13 if w._is_13mer_mode else 23
        flat, keep = w._split_fixed(kmers, k)
        out = [{} for _ in range(len(kmers))]
        if keep.shape[0] == 0:
            return out
        off, _, rid, loc = w.get_positions_array(flat, 0, True)
        off, rid, loc = off.tolist(), rid.tolist(), loc.tolist()
        for j, i in enumerate(keep.tolist()):
            hits = out[i]
            for e in range(off[j], off[j + 1]):
                hits.setdefault(rid[e], []).append(loc[e])
        return out

    def get_reads_by_kmer(self, kmer: str, max_reads: int = 100) -> List[str]:
        """aindex.py:162-166 over get_reads_se_by_kmer (see the wrapper for the one documented deviation)."""
        if not self._wrapper.aindex_loaded:
            raise RuntimeError("Aindex not loaded")
        return self._wrapper.get_reads_se_by_kmer(kmer, max_reads)

    def get_reads_batch(self, starts, ends, revcomp=False) -> List[str]:
        """[get_read(s, e, revcomp) ...]: one GPU call over the reads file in HBM (revcomp: one bool or one flag per item)."""
        return self._wrapper.get_reads_batch(starts, ends, revcomp)

    def get_reads_by_rid_batch(self, rids) -> List[str]:
        """[get_read_by_rid(r) for r in rids], one GPU call."""
        return self._wrapper.get_reads_by_rid_batch(rids)

    def get_reads_by_kmer_batch(self, kmers, max_reads: int = 100) -> List[List[str]]:
        """[get_reads_by_kmer(s, max_reads) for s in kmers], one GPU call; wrong-length items give [] in place."""
        if not self._wrapper.aindex_loaded:
            raise RuntimeError("Aindex not loaded")
        return self._wrapper.get_reads_by_kmer_batch(kmers, max_reads)

    def get_sequence_hits_array(self, seqs, max_per_kmer: int = 0):
        """CSR arrays (seq_offsets, qoff, pos, rid, local, flag) of the seed hits of every sequence; see AindexWrapper.get_sequence_hits_array."""
        return self._wrapper.get_sequence_hits_array(seqs, max_per_kmer)

    def map_sequences(self, seqs, min_votes: int = 2, max_per_kmer: int = 0) -> List[List[tuple]]:
        """Per sequence [(rid, strand, diag, votes, q_first, q_last)], one GPU call; see AindexWrapper.map_sequences."""
        return self._wrapper.map_sequences(seqs, min_votes, max_per_kmer)

    def find_sequences_array(self, seqs, hd: int = 0, seed_step: int = 23, max_per_kmer: int = 0):
        """CSR arrays (find_offsets, pos, rid, local, strand, dist) of the alignments of every sequence to the indexed reads with at most
        hd mismatches, either strand, one GPU call; see AindexWrapper.find_sequences_array and include/aindex_hip.h for the rules."""
        return self._wrapper.find_sequences_array(seqs, hd, seed_step, max_per_kmer)

    def find_reads_by_sequence_batch(self, seqs, hd: int = 0) -> List[List[tuple]]:
        """Per sequence [(rid, local, read, strand, dist)] ascending by (position in the reads file, strand): the reads that hold it with
        at most hd mismatches (hamming_distance), local = where it starts in the read, strand 1 = the read holds its reverse complement.
        Two GPU calls: the search, and the reads of every distinct rid."""
        off, _, rid, local, strand, dist = self.find_sequences_array(seqs, hd)
        uniq, inv = np.unique(rid, return_inverse=True)
        reads = self.get_reads_by_rid_batch(uniq)
        recs = [(r, l, reads[j], s, d) for r, l, j, s, d in zip(rid.tolist(), local.tolist(), inv.tolist(), strand.tolist(), dist.tolist())]
        off = off.tolist()
        return [recs[off[i]:off[i + 1]] for i in range(len(off) - 1)]

    def find_sequences_edit_array(self, seqs, ed: int = 1, seed_step: int = 23, max_per_kmer: int = 0):
        """CSR arrays (find_offsets, start, end, rid, local, strand, dist) of the alignments of every sequence to the indexed reads with
        edit distance at most ed (substitutions, inserted and deleted bases), either strand, one GPU call; see
        AindexWrapper.find_sequences_edit_array and include/aindex_hip.h for the rules."""
        return self._wrapper.find_sequences_edit_array(seqs, ed, seed_step, max_per_kmer)

    def find_reads_by_sequence_edit_batch(self, seqs, ed: int = 1) -> List[List[tuple]]:
        """Per sequence, per read that holds it with edit distance at most ed, rid ascending: (rid, starts[0], read, starts, ends, smallest
        dist); starts / ends = where its alignments begin / end in the read, either strand, each ascending and distinct. Seeds on either
        side of an indel report near-duplicate records of one alignment in the arrays; this surface merges them per read.
        Two GPU calls: the search, and the reads of every distinct rid."""
        off, start, end, rid, local, _, dist = self.find_sequences_edit_array(seqs, ed)
        uniq = np.unique(rid)
        reads = dict(zip(uniq.tolist(), self.get_reads_by_rid_batch(uniq)))
        off = off.tolist()
        lend = (end - start + local).tolist()
        rid, local, dist = rid.tolist(), local.tolist(), dist.tolist()
        out = []
        for i in range(len(off) - 1):
            per = {}
            for j in range(off[i], off[i + 1]):
                e = per.setdefault(rid[j], [set(), set(), dist[j]])
                e[0].add(local[j])
                e[1].add(lend[j])
                e[2] = min(e[2], dist[j])
            out.append([(r, min(per[r][0]), reads[r], sorted(per[r][0]), sorted(per[r][1]), per[r][2]) for r in sorted(per)])
        return out

    def get_strandness_batch(self, kmers) -> List[tuple]:
        """[(plus, minus, total)] per 23-mer, one GPU call; see AindexWrapper.get_strandness_batch."""
        return self._wrapper.get_strandness_batch(kmers)

    def get_next_batch(self, kmers, cutoff: int = 0) -> List[dict]:
        """The four successors of every 23-mer with their tf (DEBRUJIN::print_next), one GPU call; see AindexWrapper.get_next_batch."""
        return self._wrapper.get_next_batch(kmers, cutoff)

    def get_prev_batch(self, kmers, cutoff: int = 0) -> List[dict]:
        """The four predecessors of every 23-mer with their tf (DEBRUJIN::print_prev), one GPU call."""
        return self._wrapper.get_prev_batch(kmers, cutoff)

    def extend_batch(self, kmers, max_steps: int = 1000, cutoff: int = 0, mode: str = "greedy", direction: str = "next") -> list:
        """[(extension, stop_name)] along the best continuation of every 23-mer, one GPU call per direction; see AindexWrapper.extend_batch."""
        return self._wrapper.extend_batch(kmers, max_steps, cutoff, mode, direction)

    # ---- De Bruijn compaction (Index.unitigs; aix_unitigs.hip) -----------------------------------------
    def get_unitigs(self, cutoff: int = 0, min_kmers: int = 1) -> List[Tuple[str, int, bool]]:
        """[(sequence, tf_sum, circular)] of every maximal unitig with at least min_kmers k-mers, in unitig order (ascending first k-mer)."""
        self._req()
        return _contig_rows(self._wrapper._need23().unitigs(cutoff), None, min_kmers)

    def get_unitig_of_kmers(self, kmers, cutoff: int = 0) -> List[Optional[Tuple[int, int, int]]]:
        """[(unitig, pos, strand)] per 23-mer through the kid lookup: the k-mer occupies bases [pos, pos + 23) of that unitig, as given
        (strand 0) or as its reverse complement (strand 1). None for an item that is not 23 characters, absent from the index, or dead."""
        self._req()
        import torch
        ix = self._wrapper._need23()
        flat, keep = self._wrapper._split_fixed(kmers, 23)
        out: List[Optional[Tuple[int, int, int]]] = [None] * len(kmers)
        if keep.shape[0] == 0:
            return out
        kid, strand = ix.kid_strand_ascii(flat)
        ku, kp, kf = ix.unitigs_layout_t(cutoff)[:3]
        at = torch.from_numpy(np.where(strand != 0, kid, 0).astype(np.int64)).to(ku.device)
        ku, kp, kf = (t[at].cpu().numpy() for t in (ku, kp, kf))
        for j, i in enumerate(keep.tolist()):
            if strand[j] != 0 and ku[j] != -1:
                out[i] = (int(ku[j]), int(kp[j]), int(kf[j] & 1) ^ int(strand[j] == 2))
        return out

    def write_unitigs(self, path: str, cutoff: int = 0, min_kmers: int = 1) -> int:
        """FASTA of get_unitigs: >u{id} LN:i:{len} KC:i:{tf_sum} km:f:{tf_sum/m:.1f}[ circular]; returns the number of records written."""
        self._req()
        return _write_fasta(path, "u", self._wrapper._need23().unitigs(cutoff), None, min_kmers)

    # ---- the unitig graph (Index.unitig_links; aix_unitigs.hip) ------------------------------------------
    def get_unitig_links(self, cutoff: int = 0) -> List[Tuple[int, str, int, str]]:
        """[(a, '+' | '-', b, '+' | '-')]: unitig a, traversed forwards (+) or backwards (-), is followed by unitig b with an overlap of 22
        bases; one tuple per pair of dual links (unitig_link_pairs). The closing link of a circular unitig is not among them."""
        self._req()
        return unitig_link_pairs(self._wrapper._need23().unitig_links(cutoff))

    def get_bubbles(self, cutoff: int = 0) -> List[Tuple[int, int]]:
        """[(u, w)] with u < w: the two arms of every simple bubble (same source end, same sink end, attached nowhere else)."""
        self._req()
        mate = self._wrapper._need23().unitig_links(cutoff)["bubble_mate"]
        u = np.nonzero(mate != np.uint32(_lib.BUBBLE_NONE))[0]
        return [(a, b) for a, b in zip(u.tolist(), mate[u].tolist()) if a < b]

    def write_gfa(self, path: str, cutoff: int = 0) -> Tuple[int, int]:
        """GFA 1 of the unitig graph (format_gfa); returns (segments, links) written."""
        self._req()
        ix = self._wrapper._need23()
        first = _write_lines(path, format_gfa(ix.unitigs(cutoff), ix.unitig_links(cutoff)))
        return first["S"], first["L"]

    # ---- contigs (Index.graph_clean_t; aix_graphclean.hip) -----------------------------------------------
    def _contig_graph(self, cutoff: int, tip_max_kmers: int, bubble_max_kmers: int, rounds: int) -> dict:
        """the cleaned graph as numpy arrays (u64 / u32): unitigs and links at `cutoff` on the device, up to `rounds` rounds of cleaning"""
        self._req()
        ix = self._wrapper._need23()
        un = ix.unitigs_t(cutoff)
        g, _ = ix.graph_clean_t(un, ix.unitig_links_t(cutoff, unitigs=un), tip_max_kmers, bubble_max_kmers, rounds)
        return ix._graph_to_host({k: g[k] for k in ix.GRAPH_KEYS})

    def get_contigs(self, cutoff: int = 0, tip_max_kmers: int = 46, bubble_max_kmers: int = 46, rounds: int = 3,
                    min_kmers: int = 1) -> List[Tuple[str, int, bool]]:
        """[(sequence, tf_sum, circular)] of every contig with at least min_kmers k-mers, in contig order: the unitigs at `cutoff` after up to
        `rounds` rounds of tip clipping (tips of at most tip_max_kmers k-mers), bubble popping and recompaction."""
        return _contig_rows(self._contig_graph(cutoff, tip_max_kmers, bubble_max_kmers, rounds), None, min_kmers)

    def write_contigs(self, path: str, cutoff: int = 0, tip_max_kmers: int = 46, bubble_max_kmers: int = 46, rounds: int = 3, min_kmers: int = 1) -> int:
        """FASTA of get_contigs: >c{id} LN:i:{len} KC:i:{tf_sum} km:f:{tf_sum/m:.1f}[ circular]; returns the number of records written."""
        return _write_fasta(path, "c", self._contig_graph(cutoff, tip_max_kmers, bubble_max_kmers, rounds), None, min_kmers)

    def write_contigs_gfa(self, path: str, cutoff: int = 0, tip_max_kmers: int = 46, bubble_max_kmers: int = 46, rounds: int = 3) -> Tuple[int, int]:
        """GFA 1 of the cleaned graph through format_gfa (segments are named u{contig id}, as format_gfa names them); returns (segments,
        links) written."""
        g = self._contig_graph(cutoff, tip_max_kmers, bubble_max_kmers, rounds)
        first = _write_lines(path, format_gfa(g, g))
        return first["S"], first["L"]

    # ---- threading (Index.seq_thread_t; aix_seqthread.hip) ------------------------------------------------
    def _thread(self, seqs, graph, cutoff: int, want_support: bool):
        """(graph, the arrays of Index.seq_thread_t as numpy u64 / u32 in a dict, link_support | None)"""
        self._req()
        import torch
        from .engine import _ragged
        ix = self._wrapper._need23()
        if graph is None:
            graph = ix.thread_graph_t(cutoff)
        data, offs = _ragged(seqs)
        dev = graph["node"].device
        st = torch.from_numpy(data.copy() if data.shape[0] else np.zeros(0, np.uint8)).to(dev)
        so = torch.from_numpy(offs.astype(np.int64)).to(dev)
        sup = torch.zeros(int(graph["E"]), dtype=torch.int64, device=dev) if want_support else None
        got = ix.seq_thread_t(graph, st, so, link_support=sup)
        thread = ix._graph_to_host(dict(zip(ix.THREAD_KEYS, got)))
        return graph, thread, (ix._to_host(sup) if want_support else None)

    def thread_sequences(self, seqs, graph=None, cutoff: int = 0) -> List[List[tuple]]:
        """Per sequence its path through the graph: [(unitig, '+' | '-', pos, q_first, q_last, linked)] — windows q_first .. q_last follow
        each other on `unitig` from position pos on, forwards (+) or backwards (-); linked: the step is joined to the one before it by a
        link of the graph. graph: what Index.thread_graph_t returned (unitigs, or contigs after cleaning), so that a caller builds it
        once; None: the unitig graph at `cutoff`."""
        _, t, _ = self._thread(seqs, graph, cutoff, False)
        sso = t["seq_step_off"].tolist()
        linked = (t["step_link"] < np.uint64(_lib.THREAD_BROKEN)).tolist()
        rows = list(zip(t["step_unitig"].tolist(), ["+-"[f & 1] for f in t["step_flag"].tolist()], t["step_pos"].tolist(), t["q_first"].tolist(),
                        t["q_last"].tolist(), linked))
        return [rows[sso[i]:sso[i + 1]] for i in range(len(seqs))]

    def get_link_support(self, seqs, graph=None, cutoff: int = 0) -> np.ndarray:
        """uint64[E]: how many times the sequences traverse every link of the graph (a link and its dual count together)."""
        return self._thread(seqs, graph, cutoff, True)[2]

    def write_gfa_paths(self, path: str, seqs, names=None, graph=None, cutoff: int = 0) -> int:
        """GFA 1 of the graph with the sequences threaded through it (format_gfa_paths): segments, links with RC:i: support, and one P line
        per linked stretch of steps; names default to seq{i}. Returns the number of P lines written."""
        graph, t, sup = self._thread(seqs, graph, cutoff, True)
        ix = self._wrapper._need23()
        g = ix._graph_to_host({k: graph[k] for k in ix.GRAPH_KEYS})
        names = list(names) if names is not None else [f"seq{i}" for i in range(len(seqs))]
        if len(names) != len(seqs):
            raise ValueError("one name per sequence")
        return _write_lines(path, format_gfa_paths(g, g, sup, t, names))["P"]

    # ---- repeat resolution (Index.graph_resolve_t; aix_graphresolve.hip) ---------------------------------
    RESOLVE_BATCH_BYTES = 64 << 20                                 # reads threaded per call

    def _resolved_graph(self, reads, cutoff: int, tip_max_kmers: int, bubble_max_kmers: int, rounds: int, min_link_support: int, min_pair_support: int,
                        max_pair_noise: int) -> dict:
        """the resolved and recompacted graph as numpy arrays: the cleaned graph built once, `reads` threaded through it in batches with
        link support and transitions accumulated, weak links removed and repeats split, then one compaction under a zero mask"""
        self._req()
        import torch
        ix = self._wrapper._need23()
        graph = ix.thread_graph_t(cutoff, tip_max_kmers, bubble_max_kmers, rounds)
        dev = graph["node"].device
        sup = torch.zeros(int(graph["E"]), dtype=torch.int64, device=dev)
        pair = torch.zeros(16 * int(graph["U"]), dtype=torch.int64, device=dev)
        for st, so in self._batches(list(reads), dev, self.RESOLVE_BATCH_BYTES):
            ix.thread_pairs_t(graph, ix.seq_thread_t(graph, st, so, link_support=sup), pair)
        g = ix.graph_resolve_t(graph, sup, pair, min_link_support, min_pair_support, max_pair_noise, compact=True)
        return ix._graph_to_host({k: g[k] for k in ix.GRAPH_KEYS})

    def get_resolved_contigs(self, reads, cutoff: int = 0, tip_max_kmers: int = 46, bubble_max_kmers: int = 46, rounds: int = 3, min_link_support: int = 2,
                             min_pair_support: int = 2, max_pair_noise: int = 0, min_kmers: int = 1) -> List[Tuple[str, int, bool]]:
        """get_contigs with repeats resolved by `reads`: [(sequence, tf_sum, circular)]. The reads are threaded through the cleaned graph; a
        link that fewer than min_link_support reads traverse is removed where its fork has a better one, and a repeat unitig whose entry
        and exit links pair up one to one (every pair seen min_pair_support times or more, every other combination at most
        max_pair_noise times) is split into one copy per pair, which the final compaction merges into its two neighbours."""
        g = self._resolved_graph(reads, cutoff, tip_max_kmers, bubble_max_kmers, rounds, min_link_support, min_pair_support, max_pair_noise)
        return _contig_rows(g, None, min_kmers)

    def write_resolved_contigs(self, path: str, reads, cutoff: int = 0, tip_max_kmers: int = 46, bubble_max_kmers: int = 46, rounds: int = 3,
                               min_link_support: int = 2, min_pair_support: int = 2, max_pair_noise: int = 0, min_kmers: int = 1) -> int:
        """FASTA of get_resolved_contigs in the form of write_contigs; returns the number of records written."""
        g = self._resolved_graph(reads, cutoff, tip_max_kmers, bubble_max_kmers, rounds, min_link_support, min_pair_support, max_pair_noise)
        return _write_fasta(path, "c", g, None, min_kmers)

    # ---- pile-up (Index.pile_place_t .. pile_call_t; aix_pileup.hip) -------------------------------------
    def _pile(self, reads, graph, cutoff: int, tip_max_kmers: int, bubble_max_kmers: int, rounds: int, max_gap: int, extend: int, want_places: bool = False):
        """(graph, counts int32[4 B] on the device, stats, per-read placement rows | None): the cleaned graph built once (or `graph`, what
        Index.thread_graph_t returned), `reads` threaded, placed and piled in batches of RESOLVE_BATCH_BYTES into one counts array"""
        self._req()
        import torch
        ix = self._wrapper._need23()
        if graph is None:
            graph = ix.thread_graph_t(cutoff, tip_max_kmers, bubble_max_kmers, rounds)
        dev = graph["node"].device
        counts = torch.zeros(4 * graph["bases"].numel(), dtype=torch.int32, device=dev)
        stats, rows = [0, 0, 0], []
        for st, so in self._batches(list(reads), dev, self.RESOLVE_BATCH_BYTES):
            places = ix.pile_place_t(graph, so, ix.seq_thread_t(graph, st, so), max_gap, extend)
            got = ix.pileup_t(graph, st, so, places, counts)
            stats = [a + b for a, b in zip(stats, got["stats"])]
            if want_places:
                p = ix._graph_to_host({k: places[k] for k in ix.PLACE_KEYS})
                spo = p["seq_place_off"].tolist()
                flat = list(zip(p["place_unitig"].tolist(), ["+-"[f & 1] for f in p["place_flag"].tolist()], p["place_pos"].tolist(), p["place_q0"].tolist(),
                                p["place_len"].tolist(), ix._to_host(got["place_mism"]).tolist()))
                rows += [flat[spo[j]:spo[j + 1]] for j in range(so.numel() - 1)]
        return graph, counts, stats, rows if want_places else None

    def get_read_placements(self, reads, graph=None, cutoff: int = 0, tip_max_kmers: int = 46, bubble_max_kmers: int = 46, rounds: int = 3, max_gap: int = 46,
                            extend: int = 22) -> List[List[tuple]]:
        """Per read its placements on the contigs of get_contigs (or on `graph`, what Index.thread_graph_t returned):
        [(contig, '+' | '-', contig_pos, read_from, length, mismatches)] — `length` read bases from read_from on lie on the contig from
        contig_pos on, forwards (+) or reverse-complemented (-); steps on one diagonal at most max_gap windows apart are one placement,
        grown by at most `extend` bases at either end."""
        return self._pile(reads, graph, cutoff, tip_max_kmers, bubble_max_kmers, rounds, max_gap, extend, True)[3]

    def get_pileup(self, reads, graph=None, cutoff: int = 0, tip_max_kmers: int = 46, bubble_max_kmers: int = 46, rounds: int = 3, max_gap: int = 46,
                   extend: int = 22) -> dict:
        """The reads piled onto the contigs: offsets uint64[U + 1], bases uint8[B], counts uint32[B, 4] (reads showing A, C, G, T at every
        contig base), depth_sum uint64[U], uncovered uint32[U] (bases no read covers) and stats (bases counted, other bytes, mismatches)."""
        graph, counts, stats, _ = self._pile(reads, graph, cutoff, tip_max_kmers, bubble_max_kmers, rounds, max_gap, extend)
        ix = self._wrapper._need23()
        called = ix.pile_call_t(graph, counts)
        out = ix._graph_to_host({"offsets": graph["offsets"], "bases": graph["bases"], "counts": counts, "depth_sum": called["depth_sum"], "uncovered": called["uncovered"]})
        out["counts"] = out["counts"].reshape(-1, 4)
        out["stats"] = stats
        return out

    def _called(self, reads, graph, cutoff, tip_max_kmers, bubble_max_kmers, rounds, max_gap, extend, min_depth, min_major_permille, min_alt_count, min_alt_permille):
        graph, counts, _, _ = self._pile(reads, graph, cutoff, tip_max_kmers, bubble_max_kmers, rounds, max_gap, extend)
        ix = self._wrapper._need23()
        called = ix.pile_call_t(graph, counts, min_depth, min_major_permille, min_alt_count, min_alt_permille)
        return ix._graph_to_host({k: graph[k] for k in ix.GRAPH_KEYS}), ix._graph_to_host(called)

    def get_variants(self, reads, graph=None, cutoff: int = 0, tip_max_kmers: int = 46, bubble_max_kmers: int = 46, rounds: int = 3, max_gap: int = 46,
                     extend: int = 22, min_depth: int = 8, min_alt_count: int = 3, min_alt_permille: int = 200) -> List[tuple]:
        """[(contig, pos, ref, alt, ref_count, alt_count, depth)] in contig order: the contig bases where at least min_depth reads are piled
        and another base than the contig's is shown by min_alt_count reads or more, min_alt_permille of the depth or more. pos is 0-based."""
        _, c = self._called(reads, graph, cutoff, tip_max_kmers, bubble_max_kmers, rounds, max_gap, extend, min_depth, 700, min_alt_count, min_alt_permille)
        return list(zip(c["var_unitig"].tolist(), c["var_pos"].tolist(), [chr(x) for x in c["var_ref"].tolist()], [chr(x) for x in c["var_alt"].tolist()],
                        c["var_ref_count"].tolist(), c["var_alt_count"].tolist(), c["var_depth"].tolist()))

    def write_variants_vcf(self, path: str, reads, graph=None, cutoff: int = 0, tip_max_kmers: int = 46, bubble_max_kmers: int = 46, rounds: int = 3,
                           max_gap: int = 46, extend: int = 22, min_depth: int = 8, min_alt_count: int = 3, min_alt_permille: int = 200) -> int:
        """VCF of get_variants (format_vcf): c{id}, the 1-based position, REF, ALT, DP= and AD=ref,alt; returns the number of records written."""
        g, c = self._called(reads, graph, cutoff, tip_max_kmers, bubble_max_kmers, rounds, max_gap, extend, min_depth, 700, min_alt_count, min_alt_permille)
        rows = zip(c["var_unitig"].tolist(), c["var_pos"].tolist(), [chr(x) for x in c["var_ref"].tolist()], [chr(x) for x in c["var_alt"].tolist()],
                   c["var_ref_count"].tolist(), c["var_alt_count"].tolist(), c["var_depth"].tolist())
        first = _write_lines(path, format_vcf(rows, np.diff(g["offsets"].astype(np.int64)).tolist()))
        return sum(first.values()) - first["#"]

    def get_polished_contigs(self, reads, graph=None, cutoff: int = 0, tip_max_kmers: int = 46, bubble_max_kmers: int = 46, rounds: int = 3, max_gap: int = 46,
                             extend: int = 22, min_depth: int = 8, min_major_permille: int = 700, min_kmers: int = 1) -> List[Tuple[str, int, bool]]:
        """get_contigs with every base replaced where at least min_depth reads are piled and min_major_permille of them or more show one
        other base: [(sequence, tf_sum, circular)]. An end product: the overlaps between linked contigs are not kept consistent."""
        g, c = self._called(reads, graph, cutoff, tip_max_kmers, bubble_max_kmers, rounds, max_gap, extend, min_depth, min_major_permille, 3, 200)
        return _contig_rows(g, c["polished"].tobytes().decode("ascii"), min_kmers)

    def write_polished_contigs(self, path: str, reads, graph=None, cutoff: int = 0, tip_max_kmers: int = 46, bubble_max_kmers: int = 46, rounds: int = 3,
                               max_gap: int = 46, extend: int = 22, min_depth: int = 8, min_major_permille: int = 700, min_kmers: int = 1) -> int:
        """FASTA of get_polished_contigs: the header of write_contigs plus PC:i:{bases changed}; returns the number of records written."""
        g, c = self._called(reads, graph, cutoff, tip_max_kmers, bubble_max_kmers, rounds, max_gap, extend, min_depth, min_major_permille, 3, 200)
        off, differs = g["offsets"].tolist(), c["polished"] != g["bases"]
        return _write_fasta(path, "c", g, c["polished"].tobytes().decode("ascii"), min_kmers, lambda i: f" PC:i:{int(differs[off[i]:off[i + 1]].sum())}")

    # ---- phasing (Index.phase_observe_t .. phase_tag_t; aix_phase.hip) -----------------------------------
    def _phased(self, reads, graph, cutoff, tip_max_kmers, bubble_max_kmers, rounds, max_gap, extend, min_depth, min_alt_count, min_alt_permille, paired,
                min_link_reads, min_link_permille, want_tags: bool = False):
        """(graph arrays, called sites, edges, solved — numpy — and the per-fragment tag arrays | None). The reads are piled once to fix the
        sites, then threaded and placed a second time, batch by batch, to be read at those sites (and a third time when tags are wanted,
        after the solve): memory stays independent of the number of reads. Only the raw links, 9 bytes each, are kept across batches."""
        import torch
        seqs = [m for pair in self._pairs(reads) for m in pair] if paired else list(reads)
        graph, counts, _, _ = self._pile(seqs, graph, cutoff, tip_max_kmers, bubble_max_kmers, rounds, max_gap, extend)
        ix = self._wrapper._need23()
        dev = graph["node"].device
        called = ix.pile_call_t(graph, counts, min_depth, 700, min_alt_count, min_alt_permille)
        group = 2 if paired else 1

        def observed():
            for st, so in self._batches(seqs, dev, self.RESOLVE_BATCH_BYTES, even=paired):
                places = ix.pile_place_t(graph, so, ix.seq_thread_t(graph, st, so), max_gap, extend)
                yield ix.phase_observe_t(graph, st, so, places, called, group)

        kept = [[o[k] for k in ix.LINK_KEYS] for o in observed()]
        empty = [torch.empty(0, dtype=ty, device=dev) for ty in (torch.int32, torch.int32, torch.uint8)]
        links = {k: torch.cat([b[i] for b in kept] + [empty[i]]) for i, k in enumerate(ix.LINK_KEYS)}
        edges = ix.phase_bundle_t(called["total"], links)
        solved = ix.phase_solve_t(called, edges, min_link_reads, min_link_permille)
        tags = None
        if want_tags:
            got = [ix._graph_to_host(ix.phase_tag_t(o, solved)) for o in observed()]
            tags = {k: np.concatenate([t[k] for t in got] + [np.zeros(0, np.uint32)]) for k in ("tag_block", "tag_h0", "tag_h1", "tag_other")}
        host = ix._graph_to_host
        return host({k: graph[k] for k in ix.GRAPH_KEYS}), host(called), host(edges), host(solved), tags

    @staticmethod
    def _phased_rows(c: dict, s: dict) -> List[tuple]:
        pos, none = c["var_pos"].tolist(), _lib.PHASE_NONE
        tail = [(None, None) if p == none else (pos[b], p) for b, p in zip(s["site_block"].tolist(), s["site_phase"].tolist())]
        rows = zip(c["var_unitig"].tolist(), pos, [chr(x) for x in c["var_ref"].tolist()], [chr(x) for x in c["var_alt"].tolist()],
                   c["var_ref_count"].tolist(), c["var_alt_count"].tolist(), c["var_depth"].tolist())
        return [r + t for r, t in zip(rows, tail)]

    def get_phased_variants(self, reads, graph=None, cutoff: int = 0, tip_max_kmers: int = 46, bubble_max_kmers: int = 46, rounds: int = 3, max_gap: int = 46,
                            extend: int = 22, min_depth: int = 8, min_alt_count: int = 3, min_alt_permille: int = 200, paired: bool = False,
                            min_link_reads: int = 2, min_link_permille: int = 800) -> List[tuple]:
        """get_variants with the sites phased by the reads that cover two of them: [(contig, pos, ref, alt, ref_count, alt_count, depth,
        block, phase)]. block is the 0-based position of the first site of the phase block on the contig, phase 0 when the alternative
        base lies on haplotype 1 of that block and 1 when it lies on haplotype 0; both are None for a site no decided link reaches. Two
        sites are linked by every fragment that shows the contig's or the alternative base at both and at no called site between them; a
        link is decided by min_link_reads fragments or more, min_link_permille of them or more agreeing. paired: `reads` are pairs as
        get_scaffolds takes them, and both mates of a pair are one fragment. The reads are threaded and placed a second time after the
        call has fixed the sites, so memory stays independent of their number: only the raw links, 9 bytes each, are kept across batches."""
        _, c, _, s, _ = self._phased(reads, graph, cutoff, tip_max_kmers, bubble_max_kmers, rounds, max_gap, extend, min_depth, min_alt_count, min_alt_permille,
                                     paired, min_link_reads, min_link_permille)
        return self._phased_rows(c, s)

    def get_phase_blocks(self, reads, graph=None, cutoff: int = 0, tip_max_kmers: int = 46, bubble_max_kmers: int = 46, rounds: int = 3, max_gap: int = 46,
                         extend: int = 22, min_depth: int = 8, min_alt_count: int = 3, min_alt_permille: int = 200, paired: bool = False,
                         min_link_reads: int = 2, min_link_permille: int = 800) -> List[tuple]:
        """The phase blocks of get_phased_variants, in contig order: [(contig, first_pos, last_pos, n_sites, edges_agree,
        edges_conflict)] — the decided links inside the block that agree with its phases and that contradict them."""
        _, c, e, s, _ = self._phased(reads, graph, cutoff, tip_max_kmers, bubble_max_kmers, rounds, max_gap, extend, min_depth, min_alt_count, min_alt_permille,
                                     paired, min_link_reads, min_link_permille)
        rows = {}
        for v, (b, p) in enumerate(zip(s["site_block"].tolist(), s["site_phase"].tolist())):
            if p != _lib.PHASE_NONE:
                r = rows.setdefault(b, [v, v, 0, 0, 0])
                r[1], r[2] = v, r[2] + 1
        for hi, st in zip(e["edge_hi"].tolist(), s["edge_state"].tolist()):
            if st in (1, 2):
                rows[int(s["site_block"][hi])][2 + st] += 1
        pos, unit = c["var_pos"].tolist(), c["var_unitig"].tolist()
        return [(unit[b], pos[first], pos[last], n, agree, conflict) for b, (first, last, n, agree, conflict) in sorted(rows.items())]

    def get_read_haplotags(self, reads, graph=None, cutoff: int = 0, tip_max_kmers: int = 46, bubble_max_kmers: int = 46, rounds: int = 3, max_gap: int = 46,
                           extend: int = 22, min_depth: int = 8, min_alt_count: int = 3, min_alt_permille: int = 200, paired: bool = False,
                           min_link_reads: int = 2, min_link_permille: int = 800) -> List[Optional[tuple]]:
        """Per fragment (a read, or with paired=True a pair) its place in the phase blocks of get_phased_variants: (contig, block_pos, h0,
        h1, other) — the block of its first observation on a phased site, its observations there on haplotype 0 and on haplotype 1, and
        those on phased sites of other blocks — or None for a fragment that observes no phased site. This threads the reads a third time."""
        _, c, _, _, t = self._phased(reads, graph, cutoff, tip_max_kmers, bubble_max_kmers, rounds, max_gap, extend, min_depth, min_alt_count, min_alt_permille,
                                     paired, min_link_reads, min_link_permille, True)
        pos, unit = c["var_pos"].tolist(), c["var_unitig"].tolist()
        return [None if b == _lib.BUBBLE_NONE else (unit[b], pos[b], h0, h1, o)
                for b, h0, h1, o in zip(t["tag_block"].tolist(), t["tag_h0"].tolist(), t["tag_h1"].tolist(), t["tag_other"].tolist())]

    def write_phased_vcf(self, path: str, reads, graph=None, cutoff: int = 0, tip_max_kmers: int = 46, bubble_max_kmers: int = 46, rounds: int = 3,
                         max_gap: int = 46, extend: int = 22, min_depth: int = 8, min_alt_count: int = 3, min_alt_permille: int = 200, paired: bool = False,
                         min_link_reads: int = 2, min_link_permille: int = 800) -> int:
        """VCF of get_phased_variants (format_vcf_phased): the records of write_variants_vcf with GT:PS of one sample; returns the number
        of records written."""
        g, c, _, s, _ = self._phased(reads, graph, cutoff, tip_max_kmers, bubble_max_kmers, rounds, max_gap, extend, min_depth, min_alt_count, min_alt_permille,
                                     paired, min_link_reads, min_link_permille)
        first = _write_lines(path, format_vcf_phased(self._phased_rows(c, s), np.diff(g["offsets"].astype(np.int64)).tolist()))
        return sum(first.values()) - first["#"]

    # ---- scaffolding (Index.mate_links_t .. scaffold_t; aix_scaffold.hip) --------------------------------
    def _pairs(self, pairs) -> list:
        """[(left, right)] as bytes, both mates in fragment orientation: tuples, lines holding '~', or None for the loaded reads file"""
        if pairs is None:
            pairs = [r for _, r in self.iter_reads()]
        out = []
        for p in pairs:
            if isinstance(p, (str, bytes)):
                b = p.encode("latin-1") if isinstance(p, str) else bytes(p)
                if b.count(b"~") != 1:
                    continue                                       # a single-end line carries no pair
                p = b.split(b"~")
            a, b = p
            out.append((a.encode("latin-1") if isinstance(a, str) else bytes(a), b.encode("latin-1") if isinstance(b, str) else bytes(b)))
        return out

    @staticmethod
    def _batches(seqs, dev, limit: int, even: bool = False):
        """(bytes, offsets) tensors on `dev` of `seqs` (a list) in batches: one closes with the sequence that brings it to `limit` bytes
        (callers pass RESOLVE_BATCH_BYTES) — with `even` only on an even number of sequences, so that mates stay together — and with the last"""
        import torch
        from .engine import _ragged
        batch, size = [], 0
        for i, r in enumerate(seqs):
            batch.append(r)
            size += len(r)
            if (size >= limit and not (even and len(batch) % 2)) or i + 1 == len(seqs):
                data, offs = _ragged(batch)
                yield torch.from_numpy(data.copy() if data.shape[0] else np.zeros(0, np.uint8)).to(dev), torch.from_numpy(offs.astype(np.int64)).to(dev)
                batch, size = [], 0

    def scaffold_graph(self, pairs, cutoff: int = 0, tip_max_kmers: int = 46, bubble_max_kmers: int = 46, rounds: int = 3, resolve: bool = False):
        """The graph the mates are threaded through (what Index.thread_graph_t returns): the cleaned graph, or with resolve=True the
        resolved and recompacted one, the k-mers of split unitigs set dead in the map so that mates anchor in unique sequence. pairs
        (read only with resolve=True): as get_scaffolds takes them."""
        self._req()
        import torch
        ix = self._wrapper._need23()
        graph = ix.thread_graph_t(cutoff, tip_max_kmers, bubble_max_kmers, rounds)
        if not resolve:
            return graph
        dev = graph["node"].device
        sup = torch.zeros(int(graph["E"]), dtype=torch.int64, device=dev)
        pair = torch.zeros(16 * int(graph["U"]), dtype=torch.int64, device=dev)
        for st, so in self._batches([m for p in self._pairs(pairs) for m in p], dev, self.RESOLVE_BATCH_BYTES, even=True):
            ix.thread_pairs_t(graph, ix.seq_thread_t(graph, st, so, link_support=sup), pair)
        merged = ix.graph_resolve_t(graph, sup, pair, compact=True)
        ku = graph["kid_unitig"].clone()
        ku[(ku >= 0) & (merged["resolved"]["copies"][ku.clamp(min=0)] > 1)] = -1          # AIX_UNITIG_NONE: a split unitig has no single place
        kid_map = ix.graph_kidmap_t((ku, graph["kid_pos"], graph["kid_flag"]), merged["resolved"]["offsets"], merged)
        g = {k: merged[k] for k in ix.GRAPH_KEYS}
        g.update(kid_unitig=kid_map[0], kid_pos=kid_map[1], kid_flag=kid_map[2], node=ix.thread_nodes_t(kid_map, g["offsets"]), U=g["offsets"].numel() - 1,
                 E=g["link_to"].numel(), rounds=graph["rounds"])
        return g

    def _scaffolds(self, pairs, insert_size, max_insert, min_anchor_windows, min_pairs, dominance, min_contig_bases, min_gap, cutoff, tip_max_kmers,
                   bubble_max_kmers, rounds, resolve, close_gaps=False, gap_tolerance=50, max_fill=16, max_fill_states=1024, drop_absorbed=True) -> dict:
        """numpy arrays: the scaffolds (Index.scaffold_t), the joins, and the contigs' offsets; with close_gaps the closure
        (Index.gap_close_t) and the filled scaffolds (Index.scaffold_fill_t) too"""
        import torch
        ix = self._wrapper._need23()
        pairs = self._pairs(pairs)
        graph = self.scaffold_graph(pairs, cutoff, tip_max_kmers, bubble_max_kmers, rounds, resolve)
        dev = graph["node"].device
        hist, keys, ds = None, [], []
        for st, so in self._batches([m for p in pairs for m in p], dev, self.RESOLVE_BATCH_BYTES, even=True):
            key, d, _, hist = ix.mate_links_t(graph, ix.seq_thread_t(graph, st, so), so, min_anchor_windows, max_insert, hist)
            keys.append(key)
            ds.append(d)
        if insert_size is None:
            if hist is None:
                raise ValueError("no pairs: pass insert_size")
            insert_size = ix.insert_size_t(hist)                   # ValueError when no pair lies within one contig
        key = torch.cat(keys) if keys else torch.zeros(0, dtype=torch.int64, device=dev)
        d = torch.cat(ds) if ds else torch.zeros(0, dtype=torch.int32, device=dev)
        slinks = ix.mate_bundle_t(key, d, int(graph["U"]), cap_hint=2 * key.numel())      # S <= 2 N: one pass, no sizing pass
        joins = ix.scaffold_mark_t(graph, slinks, insert_size, min_pairs, dominance, min_contig_bases)
        sc = ix.scaffold_t(graph, joins, min_gap)
        more = {}
        if close_gaps:
            closure = ix.gap_close_t(graph, joins, gap_tolerance, max_fill, max_fill_states, cap_hint=int(graph["U"]))   # room for a fill per contig: mostly one pass
            more = {**closure, **ix.scaffold_fill_t(graph, joins, sc, closure, min_gap)}
        out = ix._graph_to_host({k: v for k, v in {**joins, **sc, **more, "offsets": graph["offsets"]}.items() if hasattr(v, "cpu")})
        out.update(insert_size=insert_size, n_scaffolds=sc["n_scaffolds"], n_joins=joins["n_joins"], n_cut=sc["n_cut"])
        if close_gaps:
            out["close_counts"] = more["counts"]
        return out

    @staticmethod
    def _kept(s, drop_absorbed: bool) -> list:
        """the filled scaffolds that are written: with drop_absorbed, not a single contig that fills a closed gap elsewhere"""
        fo, fm, uses = s["fmember_off"].tolist(), s["fmember"], s["fill_uses"]
        return [i for i in range(len(fo) - 1) if not (drop_absorbed and fo[i + 1] - fo[i] == 1 and uses[int(fm[fo[i]]) >> 1] >= 1)]

    def get_scaffolds(self, pairs=None, insert_size: Optional[int] = None, max_insert: int = 1000, min_anchor_windows: int = 1, min_pairs: int = 2,
                      dominance: int = 2, min_contig_bases: int = 0, min_gap: int = 1, cutoff: int = 0, tip_max_kmers: int = 46, bubble_max_kmers: int = 46,
                      rounds: int = 3, resolve: bool = False, close_gaps: bool = False, gap_tolerance: int = 50, max_fill: int = 16,
                      max_fill_states: int = 1024, drop_absorbed: bool = True) -> List[Tuple[str, List[tuple]]]:
        """Contigs joined by read pairs: [(sequence, [(contig, '+' | '-', gap)])], the gap in front of the member (0 for the first) as
        estimated, 'N' runs of max(gap, min_gap) in the sequence. pairs: [(left, right)] or lines `left~right`, both mates on the
        fragment's strand as a reads file holds them; None: the loaded reads file. insert_size None: the median of the pairs that lie
        within one contig.
        close_gaps: every join with exactly one path of the estimated length (within gap_tolerance) through at most max_fill unjoined
        contigs of the graph, found within max_fill_states search states, is written with the bases of that path in place of its 'N'
        run. The members are then (contig, strand, gap, kind) with kind "member" or "fill", the gap -22 for a member that overlaps its
        predecessor by 22 bases; with drop_absorbed a single-contig scaffold whose contig fills a gap is left out."""
        s = self._scaffolds(pairs, insert_size, max_insert, min_anchor_windows, min_pairs, dominance, min_contig_bases, min_gap, cutoff, tip_max_kmers,
                            bubble_max_kmers, rounds, resolve, close_gaps, gap_tolerance, max_fill, max_fill_states, drop_absorbed)
        if close_gaps:
            text, so, fo = s["fscaffold_bases"].tobytes().decode("ascii"), s["fscaffold_offsets"].tolist(), s["fmember_off"].tolist()
            mem, flag, gap = s["fmember"].tolist(), s["fmember_flag"].tolist(), s["fmember_gap"].view(np.int64).tolist()
            return [(text[so[i]:so[i + 1]], [(mem[j] >> 1, "+-"[mem[j] & 1], -22 if flag[j] & 1 else gap[j], "fill" if flag[j] & 2 else "member")
                                             for j in range(fo[i], fo[i + 1])]) for i in self._kept(s, drop_absorbed)]
        text, so, mo = s["scaffold_bases"].tobytes().decode("ascii"), s["scaffold_offsets"].tolist(), s["member_off"].tolist()
        mem, gap = s["member"].tolist(), s["member_gap"].view(np.int64).tolist()
        return [(text[so[i]:so[i + 1]], [(w >> 1, "+-"[w & 1], g) for w, g in zip(mem[mo[i]:mo[i + 1]], gap[mo[i]:mo[i + 1]])]) for i in range(len(so) - 1)]

    def write_scaffolds(self, path: str, pairs=None, **kw) -> int:
        """FASTA of get_scaffolds (records s0, s1, ..); returns the number of records written."""
        got = self.get_scaffolds(pairs, **kw)
        with open(path, "w") as f:
            for i, (seq, members) in enumerate(got):
                f.write(f">s{i} LN:i:{len(seq)} members:i:{len(members)}\n{seq}\n")
        return len(got)

    def write_scaffolds_agp(self, path: str, pairs=None, **kw) -> int:
        """AGP 2.0 of the scaffolds: a W line per member (component c<contig>, whole, with its orientation) and an N line per gap
        (scaffold, linkage yes, paired-ends); returns the number of lines written. The arguments and defaults are get_scaffolds's.
        With close_gaps a member that overlaps its predecessor is a W line over its component bases 23 .. L, with no N line."""
        import inspect
        args = inspect.signature(self.get_scaffolds).bind(pairs, **kw)     # a TypeError for a name get_scaffolds does not take
        args.apply_defaults()
        s, min_gap = self._scaffolds(**args.arguments), args.arguments["min_gap"]
        if args.arguments["close_gaps"]:
            off, fo, mem = s["offsets"].tolist(), s["fmember_off"].tolist(), s["fmember"].tolist()
            flag, gap = s["fmember_flag"].tolist(), s["fmember_gap"].view(np.int64).tolist()
            lines = 0
            with open(path, "w") as f:
                f.write("##agp-version 2.0\n")
                for i, sc in enumerate(self._kept(s, args.arguments["drop_absorbed"])):
                    at, part = 1, 1
                    for j in range(fo[sc], fo[sc + 1]):
                        if j > fo[sc] and not flag[j] & 1:
                            n = max(gap[j], min_gap)
                            f.write(f"s{i}\t{at}\t{at + n - 1}\t{part}\tN\t{n}\tscaffold\tyes\tpaired-ends\n")
                            at, part, lines = at + n, part + 1, lines + 1
                        u = mem[j] >> 1
                        ln, skip = off[u + 1] - off[u], 22 * (flag[j] & 1)
                        f.write(f"s{i}\t{at}\t{at + ln - skip - 1}\t{part}\tW\tc{u}\t{skip + 1}\t{ln}\t{'+-'[mem[j] & 1]}\n")
                        at, part, lines = at + ln - skip, part + 1, lines + 1
            return lines
        off, mo, mem, gap = s["offsets"].tolist(), s["member_off"].tolist(), s["member"].tolist(), s["member_gap"].view(np.int64).tolist()
        lines = 0
        with open(path, "w") as f:
            f.write("##agp-version 2.0\n")
            for i in range(len(mo) - 1):
                at, part = 1, 1
                for j in range(mo[i], mo[i + 1]):
                    if j > mo[i]:
                        n = max(gap[j], min_gap)
                        f.write(f"s{i}\t{at}\t{at + n - 1}\t{part}\tN\t{n}\tscaffold\tyes\tpaired-ends\n")
                        at, part, lines = at + n, part + 1, lines + 1
                    u = mem[j] >> 1
                    ln = off[u + 1] - off[u]
                    f.write(f"s{i}\t{at}\t{at + ln - 1}\t{part}\tW\tc{u}\t1\t{ln}\t{'+-'[mem[j] & 1]}\n")
                    at, part, lines = at + ln, part + 1, lines + 1
        return lines

    def get_gap_closures(self, pairs=None, **kw) -> List[tuple]:
        """One record (e, t, gap, status, dist, [path words], states) per join of the scaffolds, e its owner end (e < t ^ 1): the
        estimated gap, "closed" | "no_path" | "ambiguous" | "exhausted", the length of the path (0 unless closed), the intermediates in
        order from e to t, and the search states stored. The arguments and defaults are get_scaffolds's (close_gaps is implied)."""
        import inspect
        from .engine import Index
        args = inspect.signature(self.get_scaffolds).bind(pairs, **kw)
        args.apply_defaults()
        s = self._scaffolds(**dict(args.arguments, close_gaps=True))
        jn, jg, st = s["join"].tolist(), s["join_gap"].view(np.int64).tolist(), s["close_status"].tolist()
        dist, ns, po, path = s["close_dist"].view(np.int64).tolist(), s["close_states"].tolist(), s["path_off"].tolist(), s["path"].tolist()
        return [(e, t, jg[e], Index.CLOSE_STATUS[st[e]], dist[e], path[po[e]:po[e + 1]], ns[e]) for e, t in enumerate(jn) if t != 0xFFFFFFFF and e < t ^ 1]

    # ---- read cleaning (Index.fix_reads; the scaffolding of read.hpp:36-117, :286-343) -----------------
    def correct_reads(self, reads: List[str], true_errors: int = 1, verify: int = 8, max_fixes: int = 4):
        """(corrected reads, records): every read's weak 23-windows (tf <= true_errors, read.hpp:296) are looked for, up to max_fixes
        single-base substitutions are applied where exactly one base makes the next `verify` windows solid, one GPU call. records is a
        structured array (_lib.readfix_dtype()) with status (index into _lib.FIX_NAMES), weak_before, weak_after, fixes, n0, nM and
        the longest solid span trim_start, trim_len (what cut_start_to / cut_end_from would keep, read.hpp:324-343)."""
        bs = [r.encode("latin-1") if isinstance(r, str) else bytes(r) for r in reads]
        if not bs:
            return [], np.zeros(0, dtype=_lib.readfix_dtype())
        lens = np.array([len(b) for b in bs], dtype=np.uint64)
        end = np.cumsum(lens + np.uint64(1), dtype=np.uint64) - np.uint64(1)        # one separator byte behind every read
        start = end - lens
        buf = np.frombuffer(b"\n".join(bs) + b"\n", dtype=np.uint8)
        out, rec, _, _ = self._wrapper._need23().fix_reads(buf, start, end, true_errors, verify, max_fixes)
        raw = out.tobytes()
        return [raw[a:b].decode("latin-1") for a, b in zip(start.tolist(), end.tolist())], rec

    def classify_reads(self, reads: List[str], true_errors: int = 1):
        """The records of correct_reads with max_fixes = 0: profile and trim span only, nothing is changed."""
        return self.correct_reads(reads, true_errors, 1, 0)[1]

    def correct_reads_file(self, reads_file: str, out_file: str, true_errors: int = 1, verify: int = 8, max_fixes: int = 4,
                           chunk_bytes: int = 64 << 20) -> dict:
        """correct_reads over a .reads file (one record per line, mates separated by '~'; every mate is a read of its own), in chunks
        cut at line ends. out_file has the size of reads_file and differs from it in the fixed bytes only. Returns the number of
        mates per status name (_lib.FIX_NAMES), "reads" (their sum) and simple_ok / simple_n0 / simple_nM, the counters of
        CorrectionErrors (read.hpp:36-117): fixes applied, boundaries without a candidate base, boundaries with several."""
        ix = self._wrapper._need23()
        totals = {name: 0 for name in _lib.FIX_NAMES}
        totals.update(reads=0, simple_ok=0, simple_n0=0, simple_nM=0)
        with open(reads_file, "rb") as src, open(out_file, "wb") as dst:
            while True:
                chunk = src.read(chunk_bytes)
                if not chunk:
                    break
                if not chunk.endswith(b"\n"):
                    chunk += src.readline()                                           # up to the line end (or the end of the file)
                a = np.frombuffer(chunk, dtype=np.uint8)
                seps = np.flatnonzero((a == 10) | (a == 126)).astype(np.uint64)
                start = np.concatenate([np.zeros(1, np.uint64), seps + np.uint64(1)])
                end = np.concatenate([seps, np.array([a.shape[0]], np.uint64)])
                if a[-1] == 10:                                                       # nothing follows the last line end
                    start, end = start[:-1], end[:-1]
                out, rec, _, _ = ix.fix_reads(a, start, end, true_errors, verify, max_fixes)
                dst.write(out.tobytes())
                counts = np.bincount(rec["status"], minlength=len(_lib.FIX_NAMES))
                for name, n in zip(_lib.FIX_NAMES, counts.tolist()):
                    totals[name] += n
                totals["reads"] += int(rec.shape[0])
                totals["simple_ok"] += int(rec["fixes"].sum(dtype=np.uint64))
                totals["simple_n0"] += int(rec["n0"].sum(dtype=np.uint64))
                totals["simple_nM"] += int(rec["nM"].sum(dtype=np.uint64))
        return totals

    def get_reads_array(self, starts, ends, revcomp=False):
        """CSR arrays (offsets, bytes uint8); see AindexWrapper.get_reads_array."""
        return self._wrapper.get_reads_array(starts, ends, revcomp)

    def get_reads_by_kmers_array(self, kmers, max_reads: int = 100):
        """CSR arrays (kmer_offsets, rid, read_offsets, bytes uint8); see AindexWrapper.get_reads_by_kmers_array."""
        return self._wrapper.get_reads_by_kmers_array(kmers, max_reads)

    def iter_reads(self):
        if self.reads_size == 0:                                  # aindex.py:271-278
            raise RuntimeError("Reads were not loaded.")
        for rid in range(self.n_reads):
            yield rid, self.get_read_by_rid(rid)

    def iter_reads_se(self):
        if self.reads_size == 0:                                  # aindex.py:280-290
            raise RuntimeError("Reads were not loaded.")
        for rid in range(self.n_reads):
            for idx, sub in enumerate(self.get_read_by_rid(rid).split("~")):
                yield rid, idx, sub

    def get_header(self, pos: int) -> Optional[str]:
        """aindex.py:296-304 — header of the record whose interval [start, start + length) holds pos; None before any
        header file was loaded, '' when no interval holds pos."""
        if not self.loaded_header:
            return None
        hit = np.nonzero((self._hdr_start <= pos) & (pos < self._hdr_end))[0]
        return self.headers.get(int(hit[0]), "") if hit.shape[0] else ""

    # ---- k-mers by frequency (aindex.py:574-793) ---------------------------------------------------------------
    def _index_to_13mer(self, index: int) -> str:
        return "".join("ACGT"[(index >> (2 * (12 - i))) & 3] for i in range(13))

    def _kmer_type(self, kmer_type: str) -> str:
        if kmer_type == "auto":                                   # the reference probes get_13mer_tf_array(), which
            return "13mer" if self._wrapper._is_13mer_mode else "23mer"   # answers [] without raising in 23-mer mode: it always
        if kmer_type not in ("13mer", "23mer"):                   # lands on "13mer"; we pick by the loaded mode (deviation)
            raise ValueError(f"Unsupported kmer_type: {kmer_type}. Use '13mer', '23mer', or 'auto'")
        return kmer_type

    _FREQ_CHUNK = 1 << 16                                          # entries decoded per fetch of iter_kmers_by_frequency

    def _freq_index(self, kmer_type: str):
        """The handle whose entries the reference enumerates: 13-mer mode walks the tf array in FILE order (mphf order) and labels entry i
        with the base-4 spelling of i (aindex.py:633-649 — the label is the 2-bit decoding of the mphf index, not the k-mer counted there;
        kept for drop-in parity); 23-mer mode walks kid = 0..n-1 and asks get_tf_value(get_kmer_by_kid(kid)). None: nothing to enumerate
        ("13mer" without a 13-mer index: the reference's empty tf array)."""
        if kmer_type == "23mer" and self.n_kmers == 0:
            raise RuntimeError("23-mer index not properly loaded")
        return self._wrapper._freq_index(kmer_type)

    def iter_kmers_by_frequency(self, min_tf: int = 1, max_kmers: Optional[int] = None, kmer_type: str = "auto"):
        if not self._loaded:
            raise RuntimeError("Index not loaded")
        ix = self._freq_index(self._kmer_type(kmer_type))
        if ix is None or max_kmers == 0:
            return
        # the selection runs on the device (threshold by radix select, stable cut, sort of the survivors): descending tf, ties in
        # enumeration order. What comes back is 8 bytes per selected entry; the strings are decoded a chunk at a time.
        want = max_kmers if (max_kmers is not None and max_kmers > 0) else 0
        kid, tf, _, _ = ix.top_kmers(want, max(min_tf, 0), want_kmers=False)
        if max_kmers is not None and max_kmers < 0:               # freq_list[:max_kmers] of the reference
            kid, tf = kid[:max_kmers], tf[:max_kmers]
        for lo in range(0, kid.shape[0], self._FREQ_CHUNK):
            rows, _, _ = ix.kmers_by_kid(kid[lo:lo + self._FREQ_CHUNK])
            labels = rows.view(f"S{ix.k}").reshape(-1).tolist()
            for label, t in zip(labels, tf[lo:lo + self._FREQ_CHUNK].tolist()):
                yield label.decode("ascii"), t

    def get_top_kmers(self, n: int = 100, min_tf: int = 1, kmer_type: str = "auto") -> List[Tuple[str, int]]:
        return list(self.iter_kmers_by_frequency(min_tf=min_tf, max_kmers=n, kmer_type=kmer_type))

    def get_kmer_frequency_stats(self, kmer_type: str = "auto") -> dict:
        if not self._loaded:
            raise RuntimeError("Index not loaded")
        kt = self._kmer_type(kmer_type)
        ix = self._freq_index(kt)
        st = ix.tf_stats() if ix is not None else {"n": 0, "non_zero": 0, "max": 0, "min_non_zero": 0, "sum": 0}
        total, nz = st["n"], st["non_zero"]
        return {"kmer_type": kt, "total_kmers": total, "non_zero_kmers": nz, "zero_kmers": total - nz,
                "max_tf": st["max"] if nz else 0, "min_tf": st["min_non_zero"] if nz else 0,
                "avg_tf": (st["sum"] / nz) if nz else 0, "total_tf": st["sum"] if nz else 0,
                "coverage": (nz / total) if total else 0}

    def get_tf_spectrum(self, max_tf: int = 255, kmer_type: str = "auto") -> List[int]:
        """Frequency spectrum: entry j <= max_tf = k-mers with term frequency j, the last entry = k-mers with a higher one."""
        if not self._loaded:
            raise RuntimeError("Index not loaded")
        return self._wrapper.get_tf_spectrum(max_tf, self._kmer_type(kmer_type))

    def get_kmers_by_kid_batch(self, kids) -> List[str]:
        return self._wrapper.get_kmers_by_kid_batch(kids)

    def get_kmer_info_batch(self, kids):
        return self._wrapper.get_kmer_info_batch(kids)

    # ---- 13-mer array access -----------------------------------------------------------------
    def get_13mer_tf_array(self) -> List[int]:
        return self._wrapper.get_13mer_tf_array()

    def get_tf_by_index_13mer(self, index: int) -> int:
        return self._wrapper.get_tf_by_index_13mer(index)

    def get_total_tf_value_13mer(self, kmer: str) -> int:
        return self._wrapper.get_total_tf_value_13mer(kmer)

    def get_total_tf_values_13mer(self, kmers: List[str]) -> List[int]:
        return self._wrapper.get_total_tf_values_13mer(kmers)

    def get_index_info(self) -> str:
        return self._wrapper.get_index_info()

    @property
    def n_kmers(self) -> int:
        return self._wrapper.n_kmers

    @property
    def n_reads(self) -> int:
        return self._wrapper.n_reads

    @property
    def aindex_loaded(self) -> bool:
        return self._wrapper.aindex_loaded
