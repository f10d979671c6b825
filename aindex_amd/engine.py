"""Index — a k-mer index resident in MI355X HBM, driven through the C ABI (include/aindex_hip.h).

Two families of methods:
  * numpy / bytes in host memory  -> staged through HBM by the library (`aix_*`)
  * torch tensors already in HBM  -> zero-copy, asynchronous on torch's current stream (`aix_*_dev`)
All results are bit-exact with the reference's CPU implementation (see tests/).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._calls import _np_ptr, _ragged, _stream_ptr, call, dev_call, dev_grow_retry, dev_size_then_fill, take, tptr, tptr_filled
from ._lib import check, lib, vp
from .engine_graph import GraphMethods


def _as_u8(kmers, k: int) -> np.ndarray:
    """Accept bytes / (N,k) uint8 / flat uint8 and return a flat contiguous uint8 array of N*k bytes."""
    if isinstance(kmers, (bytes, bytearray, memoryview)):
        a = np.frombuffer(kmers, dtype=np.uint8)
    else:
        a = np.ascontiguousarray(kmers, dtype=np.uint8).reshape(-1)
    if a.shape[0] % k:
        raise ValueError(f"k-mer buffer length {a.shape[0]} is not a multiple of k={k}")
    return a


class Index(GraphMethods):
    def __init__(self, handle: vp):
        self._h = handle
        self._info = _lib.Info()
        call("aix_index_info", self._h, C.byref(self._info))

    # ---- lifecycle ---------------------------------------------------------------------------
    @classmethod
    def open_23(cls, pf: str, tf_bin: str, kmers_bin: str, device: int = 0) -> "Index":
        h = vp()
        call("aix_index_open_23", pf.encode(), tf_bin.encode(), kmers_bin.encode(), device, C.byref(h), of=pf)
        return cls(h)

    @classmethod
    def open_13(cls, pf: str, tf_bin: Optional[str], device: int = 0) -> "Index":
        h = vp()
        call("aix_index_open_13", pf.encode(), tf_bin.encode() if tf_bin else None, device, C.byref(h), of=pf)
        return cls(h)

    @classmethod
    def create_23(cls, pf_bytes: bytes, checker: np.ndarray, tf: np.ndarray, device: int = 0) -> "Index":
        checker = np.ascontiguousarray(checker, dtype=np.uint64)
        tf = np.ascontiguousarray(tf, dtype=np.uint32)
        assert checker.shape == tf.shape
        h = vp()
        buf = np.frombuffer(pf_bytes, dtype=np.uint8)
        call("aix_index_create_23", _np_ptr(buf), buf.shape[0], _np_ptr(checker), _np_ptr(tf), checker.shape[0], device, C.byref(h))
        return cls(h)

    @classmethod
    def create_13(cls, pf_bytes: bytes, tf: Optional[np.ndarray] = None, device: int = 0) -> "Index":
        if tf is not None:
            tf = np.ascontiguousarray(tf, dtype=np.uint64)
            assert tf.shape[0] == _lib.TOTAL_13MERS
        h = vp()
        buf = np.frombuffer(pf_bytes, dtype=np.uint8)
        call("aix_index_create_13", _np_ptr(buf), buf.shape[0], _np_ptr(tf), device, C.byref(h))
        return cls(h)

    @classmethod
    def build_23_codes_t(cls, pf_bytes: bytes, keys_t, counts_t=None, device: Optional[int] = None) -> "Index":
        """I1 on the device: scatter (2-bit code, count) pairs that already live in HBM through the MPHF and
        keep the result resident. keys_t: int64/uint64 tensor; counts_t: int32 tensor or None (tf = 0)."""
        import torch
        dev = keys_t.device.index if device is None else device
        h = vp()
        buf = np.frombuffer(pf_bytes, dtype=np.uint8)
        with torch.cuda.device(dev):
            call("aix_index_build_23_codes_dev", _np_ptr(buf), buf.shape[0], tptr(keys_t), tptr(counts_t), keys_t.numel(), dev, _stream_ptr(dev), C.byref(h))
        return cls(h)

    def close(self):
        if self._h is not None and self._h.value:
            lib().aix_index_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- metadata ----------------------------------------------------------------------------
    @property
    def k(self) -> int:
        return self._info.k

    @property
    def n(self) -> int:
        return self._info.n

    @property
    def device(self) -> int:
        return self._info.device

    @property
    def canonical_only(self) -> bool:
        return bool(self._info.canonical_only)

    @property
    def info(self) -> dict:
        i = self._info
        check(lib().aix_index_info(self._h, C.byref(i)))
        return {f: getattr(i, f) for f, _ in i._fields_ if not f.startswith("reserved")}

    def set_canonical_fastpath(self, enabled: bool):
        check(lib().aix_index_set_canonical_fastpath(self._h, int(enabled)))

    def set_fingerprint_filter(self, enabled: bool):
        check(lib().aix_index_set_fingerprint_filter(self._h, int(enabled)))

    def set_early_exit(self, enabled: bool):
        check(lib().aix_index_set_early_exit(self._h, int(enabled)))

    def set_bucket_table(self, enabled: bool, lanes: int = 0):
        """Verification table on / off (answers are identical); lanes = lanes sharing one bucket read (8, 4, 2, 1; 0 = keep)."""
        check(lib().aix_index_set_bucket_table(self._h, int(enabled), lanes))

    def set_absence_filter(self, enabled: bool):
        """Blocked Bloom filter in front of the verification table on / off (answers are identical)."""
        check(lib().aix_index_set_absence_filter(self._h, int(enabled)))

    def set_minimizer_table(self, enabled: bool):
        """Minimizer-keyed copy of the verification table (streaming consumers) on / off (answers are identical)."""
        check(lib().aix_index_set_minimizer_table(self._h, int(enabled)))

    def probe_profile(self) -> dict:
        """What one probe that FINDS its key reads under the current settings (bench.py's roofline accounting)."""
        i = self.info
        if i["bucket_table"] and i["minimizer_lines"]:
            return {"name": "minimizer-keyed verification table: one 128-byte line per super-k-mer (about 7 consecutive windows), re-used from registers / L1",
                    "bytes_per_hit_probe": 128.0, "lines_per_hit_probe": 1.0, "hbm_lines_per_hit_probe": 0.2}
        if i["bucket_table"]:
            return {"name": f"verification table: one 128-byte bucket line per probe ({i['bucket_lanes']} lanes per line)",
                    "bytes_per_hit_probe": 128.0, "lines_per_hit_probe": 1.0}
        return {"name": "three 16-byte MPHF records + one 16-byte key record", "bytes_per_hit_probe": 64.0, "lines_per_hit_probe": 4.0}

    def set_tf_13(self, tf: np.ndarray):
        tf = np.ascontiguousarray(tf, dtype=np.uint64)
        assert tf.shape[0] == _lib.TOTAL_13MERS
        call("aix_index_set_tf_13", self._h, _np_ptr(tf))

    def tf_array(self) -> np.ndarray:
        out = np.empty(self.n, dtype=np.uint64 if self.k == 13 else np.uint32)
        call("aix_index_get_tf", self._h, _np_ptr(out), out.nbytes)
        return out

    def checker_array(self) -> np.ndarray:
        out = np.empty(self.n, dtype=np.uint64)
        call("aix_index_get_checker", self._h, _np_ptr(out), out.shape[0])
        return out

    # ---- host-memory queries -----------------------------------------------------------------
    def tf_ascii(self, kmers) -> np.ndarray:
        a = _as_u8(kmers, self.k)
        n = a.shape[0] // self.k
        out = np.empty(n, dtype=np.uint32)
        call("aix_tf_batch_ascii", self._h, _np_ptr(a), n, _np_ptr(out))
        return out

    def tf_ascii_into(self, a: np.ndarray, out: np.ndarray) -> np.ndarray:
        """tf_ascii on caller-owned buffers (contiguous uint8[n*k] in, uint32[n] out) — e.g. pinned staging kept between calls."""
        assert a.dtype == np.uint8 and out.dtype == np.uint32 and a.flags.c_contiguous and out.flags.c_contiguous and a.shape[0] == out.shape[0] * self.k
        call("aix_tf_batch_ascii", self._h, _np_ptr(a), out.shape[0], _np_ptr(out))
        return out

    def tf_codes(self, codes: np.ndarray) -> np.ndarray:
        c = np.ascontiguousarray(codes, dtype=np.uint64)
        out = np.empty(c.shape[0], dtype=np.uint32)
        call("aix_tf_batch_codes", self._h, _np_ptr(c), c.shape[0], _np_ptr(out))
        return out

    def tf_ragged(self, items: Sequence) -> np.ndarray:
        data, offs = _ragged(items)
        out = np.empty(len(items), dtype=np.uint32)
        call("aix_tf_batch_ragged", self._h, _np_ptr(data), _np_ptr(offs), len(items), _np_ptr(out))
        return out

    def hash_ascii(self, kmers) -> np.ndarray:
        a = _as_u8(kmers, self.k)
        n = a.shape[0] // self.k
        out = np.empty(n, dtype=np.uint64)
        call("aix_hash_batch_ascii", self._h, _np_ptr(a), n, _np_ptr(out))
        return out

    def kid_strand_ascii(self, kmers) -> Tuple[np.ndarray, np.ndarray]:
        a = _as_u8(kmers, self.k)
        n = a.shape[0] // self.k
        kid = np.empty(n, dtype=np.uint64)
        strand = np.empty(n, dtype=np.uint8)
        call("aix_kid_strand_batch_ascii", self._h, _np_ptr(a), n, _np_ptr(kid), _np_ptr(strand))
        return kid, strand

    def both_ascii(self, kmers) -> Tuple[np.ndarray, np.ndarray]:
        a = _as_u8(kmers, self.k)
        n = a.shape[0] // self.k
        f = np.empty(n, dtype=np.uint64)
        r = np.empty(n, dtype=np.uint64)
        call("aix_tf_both_batch_ascii", self._h, _np_ptr(a), n, _np_ptr(f), _np_ptr(r))
        return f, r

    def total_ascii(self, kmers) -> np.ndarray:
        a = _as_u8(kmers, self.k)
        n = a.shape[0] // self.k
        out = np.empty(n, dtype=np.uint64)
        call("aix_tf_total_batch_ascii", self._h, _np_ptr(a), n, _np_ptr(out))
        return out

    def coverage(self, seqs: Sequence, cutoff: int = 0):
        """Per-position tf profile of each sequence (list of np.uint32 arrays, len - k + 1 each)."""
        data, offs = _ragged(seqs)
        lens = np.diff(offs).astype(np.int64)
        outl = np.maximum(lens - self.k + 1, 0).astype(np.uint64)
        ooffs = np.zeros(len(seqs) + 1, dtype=np.uint64)
        ooffs[1:] = np.cumsum(outl, dtype=np.uint64)
        out = np.zeros(int(ooffs[-1]), dtype=np.uint32)
        if len(seqs):
            call("aix_coverage_batch", self._h, _np_ptr(data), _np_ptr(offs), len(seqs), cutoff, _np_ptr(out), _np_ptr(ooffs))
        return [out[int(ooffs[i]):int(ooffs[i + 1])] for i in range(len(seqs))]

    # ---- counting ----------------------------------------------------------------------------
    def count13(self, buf: bytes, fmt: int = _lib.FMT_AUTO) -> np.ndarray:
        a = np.frombuffer(buf, dtype=np.uint8)
        out = np.empty(_lib.TOTAL_13MERS, dtype=np.uint64)
        call("aix_count13", self._h, _np_ptr(a), a.shape[0], fmt, _np_ptr(out))
        return out

    def count23_fixed(self, buf: bytes, fmt: int = _lib.FMT_AUTO, canon_mode: int = _lib.CANON_TRUE_RC) -> np.ndarray:
        a = np.frombuffer(buf, dtype=np.uint8)
        out = np.zeros(self.n, dtype=np.uint32)
        call("aix_count23_fixed", self._h, _np_ptr(a), a.shape[0], fmt, canon_mode, _np_ptr(out))
        return out

    def count13_file(self, path: str, out_path: Optional[str] = None, fmt: int = _lib.FMT_AUTO, want_array: bool = True):
        """count_kmers13 on a FILE, streamed (aix_count13_file: the file is read part by part into pinned staging while the previous part is
        counted; the host never holds it). Returns (u64[4^13] or None, stats dict); out_path receives the reference's output file."""
        out = np.empty(_lib.TOTAL_13MERS, dtype=np.uint64) if want_array else None
        st = _lib.IngestStats()
        call("aix_count13_file", self._h, os.fsencode(path), fmt, os.fsencode(out_path) if out_path else None, _np_ptr(out), C.byref(st), of=path)
        return out, st.as_dict()

    def count23_fixed_file(self, path: str, fmt: int = _lib.FMT_AUTO, canon_mode: int = _lib.CANON_TRUE_RC):
        """aix_count23_fixed on a FILE, streamed. Returns (u32[n], stats dict)."""
        out = np.zeros(self.n, dtype=np.uint32)
        st = _lib.IngestStats()
        call("aix_count23_fixed_file", self._h, os.fsencode(path), fmt, canon_mode, _np_ptr(out), C.byref(st), of=path)
        return out, st.as_dict()

    def positions_fill(self, reads):
        """A1 + A2: (indices uint64[n+1], positions uint64[sum tf]) = the .indices.bin / .index.bin images.
        `reads`: bytes or any buffer (e.g. a numpy memmap of the reads file: nothing is copied on the host)."""
        a = np.frombuffer(reads, dtype=np.uint8)
        indices = np.empty(self.n + 1, dtype=np.uint64)
        total = C.c_uint64()
        call("aix_positions_fill", self._h, _np_ptr(a), a.shape[0], _np_ptr(indices), None, 0, C.byref(total))
        pos = np.zeros(total.value, dtype=np.uint64)
        call("aix_positions_fill", self._h, _np_ptr(a), a.shape[0], _np_ptr(indices), _np_ptr(pos), pos.shape[0], C.byref(total))
        return indices, pos

    def positions_indices(self) -> np.ndarray:
        """A1 alone: uint64[n+1] exclusive prefix sum of tf (the .indices.bin image)."""
        indices = np.empty(self.n + 1, dtype=np.uint64)
        total = C.c_uint64()
        call("aix_positions_fill", self._h, None, 0, _np_ptr(indices), None, 0, C.byref(total))
        return indices

    def positions_bucket_counts(self, reads: bytes, first_shard: bool = True) -> np.ndarray:
        """uint64[n]: windows of `reads` per bucket under A2's rules (the shard-local ppositions counters)."""
        a = np.frombuffer(reads, dtype=np.uint8)
        out = np.zeros(self.n, dtype=np.uint64)
        call("aix_positions_bucket_counts", self._h, _np_ptr(a), a.shape[0], int(first_shard), _np_ptr(out))
        return out

    def positions_fill_shard(self, reads: bytes, total: int, first_shard: bool, base_offset: int, filled_init: Optional[np.ndarray]) -> np.ndarray:
        """uint64[total]: this shard's entries of the positions array (zero elsewhere); see aix_positions_fill_shard."""
        a = np.frombuffer(reads, dtype=np.uint8)
        pos = np.zeros(total, dtype=np.uint64)
        f = None if filled_init is None else np.ascontiguousarray(filled_init, dtype=np.uint32)
        call("aix_positions_fill_shard", self._h, _np_ptr(a), a.shape[0], int(first_shard), base_offset, _np_ptr(f), _np_ptr(pos), pos.shape[0])
        return pos

    # ---- batch position queries over an attached positions index (aix_posquery.hip) -----------
    def attach_aindex(self, indices, positions):
        """Copy the .indices.bin (n + 1) / .index.bin images (numpy arrays or memmaps, uint64) to HBM for positions_batch."""
        ind = np.ascontiguousarray(indices, dtype=np.uint64)
        pos = np.ascontiguousarray(positions, dtype=np.uint64)
        if ind.shape[0] != self.n + 1:
            raise ValueError(f"indices holds {ind.shape[0]} entries, the handle needs n + 1 = {self.n + 1}")
        call("aix_aindex_attach", self._h, _np_ptr(ind), _np_ptr(pos) if pos.shape[0] else None, pos.shape[0])
        self._aindex_keep = None

    def attach_aindex_t(self, indices_t, positions_t):
        """Borrow device tensors (int64 bit patterns, e.g. the outputs of positions_fill_t); they are kept alive by this object."""
        self._chk_dev(indices_t)
        if positions_t.numel():
            self._chk_dev(positions_t)
        if indices_t.numel() != self.n + 1:
            raise ValueError(f"indices holds {indices_t.numel()} entries, the handle needs n + 1 = {self.n + 1}")
        call("aix_aindex_attach_dev", self._h, tptr(indices_t), tptr_filled(positions_t), positions_t.numel(), _stream_ptr(self.device))
        self._aindex_keep = (indices_t, positions_t)

    def detach_aindex(self):
        call("aix_aindex_detach", self._h)
        self._aindex_keep = None

    def attach_ridx(self, triples) -> bool:
        """Read intervals (rid, start, end per read) to HBM. False when they are not sorted and disjoint: nothing is attached then and
        locate=True / locate() are refused."""
        t = np.ascontiguousarray(triples, dtype=np.uint64).reshape(-1, 3)
        what = "aix_ridx_attach"
        st = getattr(lib(), what)(self._h, _np_ptr(t) if t.shape[0] else None, t.shape[0])
        if st == _lib.AIX_ERR_UNSUPPORTED:
            return False
        check(st, what)
        return True

    _take = staticmethod(take)

    def positions_batch(self, kmers, max_per_kmer: int = 0, locate: bool = False):
        """(offsets[N + 1], positions[offsets[N]][, rid, offset_in_read]) as numpy uint64: list i = positions[offsets[i]:offsets[i + 1]] =
        get_positions(kmer i), cut to max_per_kmer entries when that is > 0. `kmers`: what tf_ascii takes."""
        a = _as_u8(kmers, self.k)
        n = a.shape[0] // self.k
        po, pp, pr, pl = vp(), vp(), vp(), vp()
        call("aix_positions_query", self._h, _np_ptr(a) if n else None, n, max_per_kmer, C.byref(po), C.byref(pp), C.byref(pr) if locate else None,
             C.byref(pl) if locate else None)
        offsets = self._take(po, n + 1)
        total = int(offsets[n])
        out = (offsets, self._take(pp, total))
        if locate:
            out += (self._take(pr, total), self._take(pl, total))
        return out

    def positions_batch_t(self, kmers_t, max_per_kmer: int = 0, locate: bool = False):
        """The same on torch tensors of the handle's device (int64 bit patterns out), on torch's current stream: one sizing call,
        then one filling call into tensors of exactly that size."""
        import torch
        self._chk_dev(kmers_t)
        n = kmers_t.numel() // self.k
        q = tptr(kmers_t) if n else None
        offsets, outs = dev_size_then_fill(self.device, "aix_positions_query_dev", n + 1, [torch.int64] * (3 if locate else 1),
                                           lambda off, o, cap, tot: (self._h, q, n, max_per_kmer, off, *(o + [None, None])[:3], cap, tot))
        return (offsets, *outs)

    def locate(self, pos):
        """(rid, start) per position: get_rid / get_start for a batch (numpy uint64 in and out)."""
        p = np.ascontiguousarray(pos, dtype=np.uint64).reshape(-1)
        rid, start = np.empty(p.shape[0], np.uint64), np.empty(p.shape[0], np.uint64)
        call("aix_positions_locate", self._h, _np_ptr(p), p.shape[0], _np_ptr(rid), _np_ptr(start))
        return rid, start

    # ---- batch read retrieval over an attached reads file (aix_readsquery.hip) -----------------
    def attach_reads(self, buf):
        """Copy the .reads image (bytes, numpy uint8 array or memmap) to HBM for fetch_reads* / reads_by_kmers."""
        a = np.frombuffer(buf, dtype=np.uint8) if isinstance(buf, (bytes, bytearray, memoryview)) else np.ascontiguousarray(buf, dtype=np.uint8).reshape(-1)
        call("aix_reads_attach", self._h, _np_ptr(a) if a.shape[0] else None, a.shape[0])
        self._reads_keep = None

    def attach_reads_t(self, t):
        """Borrow a uint8 device tensor (e.g. synth_reads_t output); it is kept alive by this object."""
        if t.numel():
            self._chk_dev(t)
        call("aix_reads_attach_dev", self._h, tptr_filled(t), t.numel(), _stream_ptr(self.device))
        self._reads_keep = t

    def detach_reads(self):
        call("aix_reads_detach", self._h)
        self._reads_keep = None

    def reads_info(self) -> Tuple[int, int]:
        """(0 nothing / 1 copied / 2 borrowed, bytes) of the attached reads."""
        out = (C.c_uint64 * 2)()
        call("aix_reads_info", self._h, C.byref(out))
        return int(out[0]), int(out[1])

    @staticmethod
    def _rc_arg(revcomp, n: int) -> Optional[np.ndarray]:
        if revcomp is None or revcomp is False:
            return None
        if revcomp is True:
            return np.ones(n, dtype=np.uint8)
        r = (np.ascontiguousarray(revcomp).reshape(-1) != 0).astype(np.uint8)
        if r.shape[0] != n:
            raise ValueError(f"revcomp holds {r.shape[0]} flags for {n} spans")
        return r

    def fetch_reads(self, starts, ends, revcomp=None):
        """(offsets uint64[N + 1], bytes uint8[offsets[N]]): item i = get_read(starts[i], ends[i], revcomp[i]). revcomp: None / bool / N flags."""
        s = np.ascontiguousarray(starts, dtype=np.uint64).reshape(-1)
        e = np.ascontiguousarray(ends, dtype=np.uint64).reshape(-1)
        if s.shape != e.shape:
            raise ValueError("starts and ends differ in length")
        n = s.shape[0]
        r = self._rc_arg(revcomp, n)
        po, pb = vp(), vp()
        call("aix_reads_fetch", self._h, _np_ptr(s) if n else None, _np_ptr(e) if n else None, _np_ptr(r) if n else None, n, C.byref(po), C.byref(pb))
        offsets = self._take(po, n + 1)
        return offsets, self._take(pb, int(offsets[n]), np.uint8)

    def fetch_reads_by_rid(self, rids):
        """(offsets, bytes): item i = get_read_by_rid(rids[i]) over the intervals of attach_ridx."""
        r = np.ascontiguousarray(rids, dtype=np.uint64).reshape(-1)
        n = r.shape[0]
        po, pb = vp(), vp()
        call("aix_reads_fetch_rid", self._h, _np_ptr(r) if n else None, n, C.byref(po), C.byref(pb))
        offsets = self._take(po, n + 1)
        return offsets, self._take(pb, int(offsets[n]), np.uint8)

    def reads_by_kmers(self, kmers, max_reads: int = 100):
        """(kmer_offsets uint64[N + 1], rid uint64[R], read_offsets uint64[R + 1], bytes uint8): the reads of k-mer i are
        rid[kmer_offsets[i]:kmer_offsets[i + 1]], read j's bytes are bytes[read_offsets[j]:read_offsets[j + 1]]."""
        a = _as_u8(kmers, self.k)
        n = a.shape[0] // self.k
        pk, pr, po, pb = vp(), vp(), vp(), vp()
        call("aix_reads_by_kmers", self._h, _np_ptr(a) if n else None, n, max_reads, C.byref(pk), C.byref(pr), C.byref(po), C.byref(pb))
        koff = self._take(pk, n + 1)
        nr = int(koff[n])
        rid = self._take(pr, nr)
        roff = self._take(po, nr + 1)
        return koff, rid, roff, self._take(pb, int(roff[nr]), np.uint8)

    def _fetch_t(self, what: str, n: int, *args):
        """The sizing call, then the filling call into a tensor of exactly that size (int64 offsets, uint8 bytes); args: what the entry
        point takes between the handle and the outputs."""
        import torch
        offsets, (out,) = dev_size_then_fill(self.device, what, n + 1, [torch.uint8], lambda off, o, cap, tot: (self._h, *args, off, *o, cap, tot))
        return offsets, out

    def fetch_reads_t(self, starts_t, ends_t, revcomp_t=None):
        """fetch_reads on int64 device tensors (u64 bit patterns); revcomp_t: uint8 / bool tensor of N flags or None."""
        self._chk_dev(starts_t)
        self._chk_dev(ends_t)
        n = starts_t.numel()
        if ends_t.numel() != n or (revcomp_t is not None and revcomp_t.numel() != n):
            raise ValueError("starts, ends and revcomp differ in length")
        if revcomp_t is not None:
            self._chk_dev(revcomp_t)
            if revcomp_t.element_size() != 1:
                raise ValueError("revcomp must be a uint8 or bool tensor")
        return self._fetch_t("aix_reads_fetch_dev", n, tptr_filled(starts_t), tptr_filled(ends_t), tptr_filled(revcomp_t), n)

    def fetch_reads_by_rid_t(self, rids_t):
        """fetch_reads_by_rid on an int64 device tensor, e.g. the rid output of positions_batch_t(..., locate=True)."""
        self._chk_dev(rids_t)
        n = rids_t.numel()
        return self._fetch_t("aix_reads_fetch_rid_dev", n, tptr_filled(rids_t), n)

    def reads_by_kmers_t(self, kmers_t, max_reads: int = 100):
        """reads_by_kmers on a uint8 device tensor of N * k bytes: (kmer_offsets, rid, read_offsets int64; bytes uint8) device tensors."""
        import torch
        self._chk_dev(kmers_t)
        n = kmers_t.numel() // self.k
        dev = kmers_t.device
        koff = torch.empty(n + 1, dtype=torch.int64, device=dev)
        tot = (C.c_uint64 * 2)()
        q = vp(kmers_t.data_ptr()) if n else None
        with torch.cuda.device(dev):
            st = _stream_ptr(self.device)
            call("aix_reads_by_kmers_dev", self._h, q, n, max_reads, vp(koff.data_ptr()), None, None, 0, None, 0, C.byref(tot), st)
            nr, nb = int(tot[0]), int(tot[1])
            rid = torch.empty(max(nr, 1), dtype=torch.int64, device=dev)[:nr]
            roff = torch.zeros(nr + 1, dtype=torch.int64, device=dev)
            by = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)[:nb]
            if nr:
                call("aix_reads_by_kmers_dev", self._h, q, n, max_reads, vp(koff.data_ptr()), vp(rid.data_ptr()), vp(roff.data_ptr()), nr,
                     vp(by.data_ptr()) if nb else None, nb, C.byref(tot), st)
        return koff, rid, roff, by

    # ---- sequences against the indexed reads (aix_seqhits.hip) ---------------------------------
    def _seq_host(self, what: str, seqs: Sequence, dtypes, *args):
        """offsets + one array per dtype through a host form: ragged sequences in, one malloc'd block per output back; the first is the
        offsets[M + 1], every other one holds offsets[M] entries."""
        data, offs = _ragged(seqs)
        m = len(seqs)
        ps = [vp() for _ in range(1 + len(dtypes))]
        call(what, self._h, _np_ptr(data) if data.shape[0] else None, _np_ptr(offs), m, *args, *[C.byref(p) for p in ps])
        offsets = self._take(ps[0], m + 1)
        return (offsets, *[self._take(p, int(offsets[m]), dt) for p, dt in zip(ps[1:], dtypes)])

    def seq_hits(self, seqs: Sequence, max_per_kmer: int = 0):
        """Seed hits of every 23-window of every sequence against the attached positions index, intervals and reads:
        (seq_offsets u64[M + 1], qoff u32, pos u64, rid u64, local i64, flag u8). The hits of sequence i are
        [seq_offsets[i], seq_offsets[i + 1]), by window, then slot; flag = strand (0 as stored, 1 reverse complement, 2 neither) | 4 when
        an interval was found."""
        return self._seq_host("aix_seq_hits", seqs, [np.uint32, np.uint64, np.uint64, np.int64, np.uint8], max_per_kmer)

    def seq_votes(self, seqs: Sequence, min_votes: int = 1, max_per_kmer: int = 0):
        """Votes per (read, strand, diagonal) of every sequence: (vote_offsets u64[M + 1], rid u64, strand u8, diag i64, votes u32,
        q_first u32, q_last u32); the records of sequence i ascend by (rid, strand, diag). diag = local - qoff (strand 0), local + qoff
        (strand 1); only groups of at least min_votes hits are reported."""
        return self._seq_host("aix_seq_votes", seqs, [np.uint64, np.uint8, np.int64, np.uint32, np.uint32, np.uint32], max_per_kmer, min_votes)

    def _seq_t(self, what: str, seqs_t, offs_t, dtypes, cap_hint: int, *args):
        """offsets + one tensor per dtype through a `_dev` twin: filled in one call when cap_hint entries suffice, else sized, then filled.
        args: what the entry point takes between the sequences and the outputs."""
        import torch
        self._chk_dev(seqs_t)
        self._chk_dev(offs_t)
        m = offs_t.numel() - 1
        offsets = torch.empty(m + 1, dtype=torch.int64, device=seqs_t.device)
        outs, _ = dev_grow_retry(self.device, what, dtypes, cap_hint,
                                 lambda o, cap, tot: (self._h, tptr(seqs_t), tptr(offs_t), m, *args, tptr(offsets), *o, cap, tot))
        return (offsets, *outs)

    def seq_hits_t(self, seqs_t, offs_t, max_per_kmer: int = 0, cap_hint: int = 0):
        """seq_hits on device tensors (uint8 bytes, int64 offsets[M + 1] into them), on torch's current stream:
        (seq_offsets int64, qoff int32, pos int64, rid int64, local int64, flag uint8) — bit patterns of the unsigned fields."""
        import torch
        return self._seq_t("aix_seq_hits_dev", seqs_t, offs_t, [torch.int32, torch.int64, torch.int64, torch.int64, torch.uint8], cap_hint, max_per_kmer)

    def seq_votes_t(self, seqs_t, offs_t, min_votes: int = 1, max_per_kmer: int = 0, cap_hint: int = 0):
        """seq_votes on device tensors: (vote_offsets int64, rid int64, strand uint8, diag int64, votes int32, q_first int32, q_last int32)."""
        import torch
        return self._seq_t("aix_seq_votes_dev", seqs_t, offs_t, [torch.int64, torch.uint8, torch.int64, torch.int32, torch.int32, torch.int32], cap_hint,
                           max_per_kmer, min_votes)

    # ---- sequences with mismatches, strand counts (aix_seqfind.hip) ----------------------------
    def seq_find(self, seqs: Sequence, hd: int = 0, seed_step: int = 23, max_per_kmer: int = 0):
        """Alignments of every sequence to the indexed reads with at most hd mismatches (hamming_distance: positions with an N on either
        side are ignored), found from the seed hits of its 23-windows at offsets 0, seed_step, ..: (find_offsets u64[M + 1], pos u64, rid u64,
        local u64, strand u8, dist u32). The records of sequence i are [find_offsets[i], find_offsets[i + 1]), ascending by (pos, strand);
        pos is where the alignment starts in the reads file, local = pos - start of the read that contains it whole. Complete when
        hd < len // 23 and seed_step is 1 or 23 (include/aindex_hip.h)."""
        return self._seq_host("aix_seq_find", seqs, [np.uint64, np.uint64, np.uint64, np.uint8, np.uint32], hd, seed_step, max_per_kmer)

    def seq_find_t(self, seqs_t, offs_t, hd: int = 0, seed_step: int = 23, max_per_kmer: int = 0, cap_hint: int = 0):
        """seq_find on device tensors (uint8 bytes, int64 offsets[M + 1] into them), on torch's current stream:
        (find_offsets int64, pos int64, rid int64, local int64, strand uint8, dist int32) — bit patterns of the unsigned fields."""
        import torch
        return self._seq_t("aix_seq_find_dev", seqs_t, offs_t, [torch.int64, torch.int64, torch.int64, torch.uint8, torch.int32], cap_hint,
                           hd, seed_step, max_per_kmer)

    # ---- sequences with substitutions, insertions and deletions (aix_seqedit.hip) -----------------
    def seq_edit(self, seqs: Sequence, ed: int = 1, seed_step: int = 23, max_per_kmer: int = 0):
        """Alignments of every sequence to the indexed reads with edit distance at most ed (0 .. _lib.SEQEDIT_MAX_ED; substitutions,
        inserted and deleted bases, the N rule of hamming_distance), found by a banded dynamic programme around the diagonal of every seed
        hit: (find_offsets u64[M + 1], start u64, end u64, rid u64, local u64, strand u8, dist u32). The records of sequence i are
        [find_offsets[i], find_offsets[i + 1]), ascending by (start, strand); the alignment is reads[start:end], local = start - start of
        the read that holds the seed. Complete when ed < len // 23 and seed_step is 1 or 23 (include/aindex_hip.h)."""
        return self._seq_host("aix_seq_edit", seqs, [np.uint64, np.uint64, np.uint64, np.uint64, np.uint8, np.uint32], ed, seed_step, max_per_kmer)

    def seq_edit_t(self, seqs_t, offs_t, ed: int = 1, seed_step: int = 23, max_per_kmer: int = 0, cap_hint: int = 0):
        """seq_edit on device tensors (uint8 bytes, int64 offsets[M + 1] into them), on torch's current stream:
        (find_offsets int64, start int64, end int64, rid int64, local int64, strand uint8, dist int32) — bit patterns of the unsigned fields."""
        import torch
        return self._seq_t("aix_seq_edit_dev", seqs_t, offs_t, [torch.int64, torch.int64, torch.int64, torch.int64, torch.uint8, torch.int32], cap_hint,
                           ed, seed_step, max_per_kmer)

    def kmer_strands(self, kmers, max_per_kmer: int = 0):
        """(plus, minus, total) uint64[N]: of the listed hits of every 23-mer (`kmers`: what tf_ascii takes), those where the reads hold it
        as given, those where they hold its reverse complement, and all of them."""
        a = _as_u8(kmers, 23)
        n = a.shape[0] // 23
        out = [np.zeros(n, np.uint64) for _ in range(3)]
        call("aix_kmer_strands", self._h, _np_ptr(a) if n else None, n, max_per_kmer, *[_np_ptr(o) if n else None for o in out])
        return tuple(out)

    def kmer_strands_t(self, kmers_t, max_per_kmer: int = 0):
        """kmer_strands on a uint8 device tensor of N * 23 bytes: three int64 device tensors, on torch's current stream."""
        import torch
        self._chk_dev(kmers_t)
        n = kmers_t.numel() // 23
        out = [torch.zeros(n, dtype=torch.int64, device=kmers_t.device) for _ in range(3)]
        dev_call(self.device, "aix_kmer_strands_dev", self._h, tptr(kmers_t) if n else None, n, max_per_kmer, *[tptr_filled(o) for o in out])
        return tuple(out)

    # ---- De Bruijn neighbours and walks (aix_debruijn.hip) -------------------------------------
    @staticmethod
    def _dir(direction, both_ok: bool) -> int:
        d = {"next": _lib.DIR_NEXT, "prev": _lib.DIR_PREV, "both": _lib.DIR_BOTH}.get(direction, direction)
        if d not in ((_lib.DIR_NEXT, _lib.DIR_PREV, _lib.DIR_BOTH) if both_ok else (_lib.DIR_NEXT, _lib.DIR_PREV)):
            raise ValueError(f"direction {direction!r}: 'next', 'prev'" + (" or 'both'" if both_ok else ""))
        return d

    @staticmethod
    def _walk_mode(mode) -> int:
        m = {"greedy": _lib.WALK_GREEDY, "unitig": _lib.WALK_UNITIG}.get(mode, mode)
        if m not in (_lib.WALK_GREEDY, _lib.WALK_UNITIG):
            raise ValueError(f"mode {mode!r}: 'greedy' or 'unitig'")
        return m

    def _kmers_or_codes(self, x):
        """(codes uint64[N] or None, ascii uint8[N * 23] or None, N): a uint64 array holds 2-bit codes, everything else is what tf_ascii takes."""
        if isinstance(x, np.ndarray) and x.dtype == np.uint64:
            c = np.ascontiguousarray(x).reshape(-1)
            return c, None, c.shape[0]
        a = _as_u8(x, 23)
        return None, a, a.shape[0] // 23

    def neighbours(self, kmers_or_codes, direction="next", cutoff: int = 0) -> np.ndarray:
        """print_next / print_prev for a batch: a structured array (CONT_DTYPE) of N records, or of shape (N, 2) — next, prev — for "both"."""
        d = self._dir(direction, True)
        c, a, n = self._kmers_or_codes(kmers_or_codes)
        out = np.zeros(n * (2 if d == _lib.DIR_BOTH else 1), dtype=_lib.cont_dtype())
        call("aix_neighbours", self._h, _np_ptr(c) if n else None, _np_ptr(a) if n else None, n, d, cutoff, _np_ptr(out) if n else None)
        return out.reshape(n, 2) if d == _lib.DIR_BOTH else out

    def walk(self, seeds, max_steps: int, direction="next", cutoff: int = 0, mode="greedy", want_tf: bool = True):
        """(bases uint8[S, max_steps], length uint32[S], stop uint8[S], tf uint32[S, max_steps] | None, last uint64[S]): row i holds length[i]
        bases ('A', 'C', 'G', 'T') in the order found and 0 beyond; stop[i] indexes _lib.STOP_NAMES; last = the code the walk ended on."""
        d, m = self._dir(direction, False), self._walk_mode(mode)
        c, a, s = self._kmers_or_codes(seeds)
        if not 1 <= max_steps <= _lib.WALK_MAX_STEPS:
            raise ValueError(f"max_steps {max_steps}: 1 .. {_lib.WALK_MAX_STEPS}")
        bases = np.zeros((s, max_steps), dtype=np.uint8)
        tf = np.zeros((s, max_steps), dtype=np.uint32) if want_tf else None
        length, stop, last = np.zeros(s, np.uint32), np.zeros(s, np.uint8), np.zeros(s, np.uint64)
        call("aix_walk", self._h, _np_ptr(c) if s else None, _np_ptr(a) if s else None, s, d, max_steps, cutoff, m, _np_ptr(bases), _np_ptr(length), _np_ptr(stop),
             _np_ptr(tf), _np_ptr(last))
        return bases, length, stop, tf, last

    def _kmers_or_codes_t(self, t):
        import torch
        self._chk_dev(t)                                            # device and contiguity
        if t.dtype == torch.int64:
            return vp(t.data_ptr()), None, t.numel()
        if t.dtype != torch.uint8 or t.numel() % 23:
            raise ValueError("k-mers: an int64 tensor of 2-bit codes or a uint8 tensor of N * 23 bytes")
        return None, vp(t.data_ptr()), t.numel() // 23

    def neighbours_t(self, kmers_or_codes_t, direction="next", cutoff: int = 0, out_t=None):
        """neighbours on a device tensor (int64 codes or uint8 ASCII): int32 tensor [N, 8] ([N, 2, 8] for "both") holding the u32 words of
        the records (tf A C G T, n, sum, best_tf, best_base), asynchronous on torch's current stream."""
        import torch
        d = self._dir(direction, True)
        c, a, n = self._kmers_or_codes_t(kmers_or_codes_t)
        shape = (n, 2, 8) if d == _lib.DIR_BOTH else (n, 8)
        if out_t is None:
            out_t = torch.empty(shape, dtype=torch.int32, device=kmers_or_codes_t.device)
        elif out_t.dtype != torch.int32 or out_t.numel() != 8 * n * (2 if d == _lib.DIR_BOTH else 1) or not out_t.is_contiguous():
            raise ValueError("out_t must be a contiguous int32 tensor of 8 words per record")
        dev_call(self.device, "aix_neighbours_dev", self._h, c if n else None, a if n else None, n, d, cutoff, tptr(out_t) if n else None)
        return out_t

    def walk_t(self, seeds_t, max_steps: int, direction="next", cutoff: int = 0, mode="greedy", want_tf: bool = True, bases_t=None, tf_t=None):
        """walk on a device tensor of seeds: (bases uint8[S, max_steps], length int32[S], stop uint8[S], tf int32[S, max_steps] | None,
        last int64[S]) device tensors, asynchronous on torch's current stream. bases_t / tf_t: caller-owned rows to write into (what lies
        at or beyond a row's length is left as it is); fresh rows are zeroed."""
        import torch
        d, m = self._dir(direction, False), self._walk_mode(mode)
        c, a, s = self._kmers_or_codes_t(seeds_t)
        if not 1 <= max_steps <= _lib.WALK_MAX_STEPS:
            raise ValueError(f"max_steps {max_steps}: 1 .. {_lib.WALK_MAX_STEPS}")
        dev = seeds_t.device
        if bases_t is None:
            bases_t = torch.zeros((s, max_steps), dtype=torch.uint8, device=dev)
        if tf_t is None and want_tf:
            tf_t = torch.zeros((s, max_steps), dtype=torch.int32, device=dev)
        for t, dt in ((bases_t, torch.uint8), (tf_t, torch.int32)):
            if t is not None:
                if t.dtype != dt or t.numel() != s * max_steps:
                    raise ValueError(f"bases_t / tf_t must be uint8 / int32 tensors of S * max_steps = {s * max_steps} elements")
                if t.numel():
                    self._chk_dev(t)
        length = torch.zeros(s, dtype=torch.int32, device=dev)
        stop = torch.zeros(s, dtype=torch.uint8, device=dev)
        last = torch.zeros(s, dtype=torch.int64, device=dev)
        dev_call(self.device, "aix_walk_dev", self._h, c if s else None, a if s else None, s, d, max_steps, cutoff, m,
                 *[tptr(t) if s else None for t in (bases_t, length, stop, tf_t, last)])
        return bases_t, length, stop, tf_t, last

    # ---- read cleaning (aix_readfix.hip) ---------------------------------------------------------
    @staticmethod
    def _fix_args(verify: int, max_fixes: int):
        if not 1 <= verify <= _lib.READFIX_MAX_VERIFY:
            raise ValueError(f"verify {verify}: 1 .. {_lib.READFIX_MAX_VERIFY}")
        if not 0 <= max_fixes <= _lib.READFIX_MAX_FIXES:
            raise ValueError(f"max_fixes {max_fixes}: 0 .. {_lib.READFIX_MAX_FIXES}")

    def fix_reads(self, buf, start, end, true_errors: int = 1, verify: int = 8, max_fixes: int = 4, fix_pos=None, fix_old=None):
        """Weak-window profile, trim span and single-base fixes of the reads buf[start[r] .. end[r]) (ascending, disjoint): (corrected copy
        of buf uint8[], records readfix_dtype[M], fix_pos uint32[M, max_fixes], fix_old uint8[M, max_fixes]). fix_pos / fix_old: caller-owned
        rows to write into (what lies at or beyond a row's `fixes` is left as it is); fresh rows are zeroed."""
        self._fix_args(verify, max_fixes)
        out = np.array(np.frombuffer(buf, dtype=np.uint8) if isinstance(buf, (bytes, bytearray, memoryview)) else buf, dtype=np.uint8, copy=True).reshape(-1)
        st, en = np.ascontiguousarray(start, dtype=np.uint64).reshape(-1), np.ascontiguousarray(end, dtype=np.uint64).reshape(-1)
        m = st.shape[0]
        if en.shape[0] != m:
            raise ValueError("start and end must have the same length")
        rec = np.zeros(m, dtype=_lib.readfix_dtype())
        if fix_pos is None:
            fix_pos = np.zeros((m, max_fixes), dtype=np.uint32)
        if fix_old is None:
            fix_old = np.zeros((m, max_fixes), dtype=np.uint8)
        for a, dt in ((fix_pos, np.uint32), (fix_old, np.uint8)):
            if a.dtype != dt or a.size != m * max_fixes or not a.flags.c_contiguous:
                raise ValueError(f"fix_pos / fix_old must be contiguous uint32 / uint8 arrays of M * max_fixes = {m * max_fixes} elements")
        logs = max_fixes > 0 and m > 0
        call("aix_reads_fix", self._h, _np_ptr(out) if m else None, out.shape[0], _np_ptr(st) if m else None, _np_ptr(en) if m else None, m, true_errors, verify,
             max_fixes, _np_ptr(rec) if m else None, _np_ptr(fix_pos) if logs else None, _np_ptr(fix_old) if logs else None)
        return out, rec, fix_pos, fix_old

    def fix_reads_t(self, buf_t, start_t, end_t, true_errors: int = 1, verify: int = 8, max_fixes: int = 4, fix_pos_t=None, fix_old_t=None):
        """fix_reads on device tensors, asynchronous on torch's current stream: buf_t (uint8) is fixed IN PLACE; start_t / end_t are int64
        tensors of M pairwise disjoint ranges. Returns (rec int32[M, 8] — the u32 words status, weak_before, weak_after, fixes, n0, nM,
        trim_start, trim_len —, fix_pos int32[M, max_fixes], fix_old uint8[M, max_fixes]); fix_pos_t / fix_old_t: caller-owned rows."""
        import torch
        self._fix_args(verify, max_fixes)
        if buf_t.dtype != torch.uint8 or start_t.dtype != torch.int64 or end_t.dtype != torch.int64 or start_t.numel() != end_t.numel():
            raise ValueError("buf_t: a uint8 tensor; start_t / end_t: int64 tensors of equal length")
        m, dev = start_t.numel(), buf_t.device
        for t in (buf_t, start_t, end_t):
            if t.numel():
                self._chk_dev(t)
        rec = torch.zeros((m, 8), dtype=torch.int32, device=dev)
        if fix_pos_t is None:
            fix_pos_t = torch.zeros((m, max_fixes), dtype=torch.int32, device=dev)
        if fix_old_t is None:
            fix_old_t = torch.zeros((m, max_fixes), dtype=torch.uint8, device=dev)
        for t, dt in ((fix_pos_t, torch.int32), (fix_old_t, torch.uint8)):
            if t.dtype != dt or t.numel() != m * max_fixes:
                raise ValueError(f"fix_pos_t / fix_old_t must be int32 / uint8 tensors of M * max_fixes = {m * max_fixes} elements")
            if t.numel():
                self._chk_dev(t)
        logs = max_fixes > 0 and m > 0
        with torch.cuda.device(dev):
            call("aix_reads_fix_dev", self._h, tptr(buf_t) if m else None, buf_t.numel(), tptr_filled(start_t), tptr_filled(end_t), m, true_errors, verify,
                 max_fixes, tptr_filled(rec), tptr(fix_pos_t) if logs else None, tptr(fix_old_t) if logs else None, _stream_ptr(self.device))
        return rec, fix_pos_t, fix_old_t

    # ---- k-mers by frequency (aix_spectrum.hip) ------------------------------------------------
    @staticmethod
    def _stats_dict(stats: np.ndarray) -> dict:
        return {f: int(v) for f, v in zip(_lib.STATS_FIELDS, stats.tolist())}

    def tf_spectrum(self, nbins: int):
        """(hist uint64[nbins], stats dict) of the per-kid values: hist[j] = entries with value j for j < nbins - 1, hist[nbins - 1] = entries
        with value >= nbins - 1; stats: _lib.STATS_FIELDS. The value of entry i is get_tf_value(get_kmer_by_kid(i)) (23-mer handle) or the
        u32 view of tf13[i] (13-mer handle)."""
        if nbins < 2:
            raise ValueError("nbins must be at least 2")
        hist, stats = np.empty(nbins, np.uint64), np.empty(_lib.SPECTRUM_STATS, np.uint64)
        call("aix_tf_spectrum", self._h, nbins, _np_ptr(hist), _np_ptr(stats))
        return hist, self._stats_dict(stats)

    def tf_stats(self) -> dict:
        return self.tf_spectrum(2)[1]

    @staticmethod
    def _cut(n: int, size: int) -> int:
        """max_items for the C ABI (a u64; 0 = all): any Python int, cut to the number of entries — ctypes would mask a larger one silently"""
        n = int(n)
        if n < 0:
            raise ValueError("n must not be negative")
        return min(n, size)

    def top_kmers(self, n: int = 0, min_tf: int = 1, want_kmers: bool = True):
        """(kid uint32[m], tf uint32[m], kmers uint8[m, k] | None, total): the first n (0 = all) entries with value >= min_tf in descending
        value, ties in ascending kid; total = entries with value >= min_tf before the cut."""
        min_tf = max(int(min_tf), 0)
        if min_tf > 0xFFFFFFFF:                                     # no u32 value reaches it
            return np.zeros(0, np.uint32), np.zeros(0, np.uint32), (np.zeros((0, self.k), np.uint8) if want_kmers else None), 0
        n = self._cut(n, self.n)
        pk, pt, ps = vp(), vp(), vp()
        m, total = C.c_uint64(), C.c_uint64()
        call("aix_top_kmers", self._h, min_tf, n, C.byref(pk), C.byref(pt), C.byref(ps) if want_kmers else None, C.byref(m), C.byref(total))
        kid, tf = self._take(pk, m.value, np.uint32), self._take(pt, m.value, np.uint32)
        kmers = self._take(ps, m.value * self.k, np.uint8).reshape(m.value, self.k) if want_kmers else None
        return kid, tf, kmers, total.value

    def kmers_by_kid(self, kids, want_rc: bool = False, want_tf: bool = False):
        """(kmers uint8[N, k], rc uint8[N, k] | None, tf uint32[N] | None): get_kmer_by_kid / get_kmer_info for a batch of kids (uint64);
        a kid >= n gives a row of NUL bytes and tf 0."""
        kd = np.ascontiguousarray(kids, dtype=np.uint64).reshape(-1)
        n = kd.shape[0]
        out = np.zeros((n, self.k), np.uint8)
        rc = np.zeros((n, self.k), np.uint8) if want_rc else None
        tf = np.zeros(n, np.uint32) if want_tf else None
        call("aix_kmers_by_kid", self._h, _np_ptr(kd) if n else None, n, _np_ptr(out) if n else None, _np_ptr(rc) if n else None, _np_ptr(tf) if n else None)
        return out, rc, tf

    def kmer_values_t(self, out_t=None):
        """int32[n] device tensor (u32 bit patterns): the value of every entry in kid order, asynchronous on torch's current stream."""
        import torch
        if out_t is None:
            out_t = torch.empty(self.n, dtype=torch.int32, device=f"cuda:{self.device}")
        elif out_t.dtype != torch.int32 or out_t.numel() != self.n:
            raise ValueError("out_t must be an int32 tensor of n elements")
        self._chk_dev(out_t)
        dev_call(self.device, "aix_kmer_values_dev", self._h, tptr_filled(out_t))
        return out_t

    def tf_spectrum_t(self, nbins: int):
        """(hist int64[nbins], stats int64[8]) device tensors on torch's current stream: complete on return for a 23-mer handle (the values
        pass uses pool scratch), asynchronous for a 13-mer handle."""
        import torch
        if nbins < 2:
            raise ValueError("nbins must be at least 2")
        dev = f"cuda:{self.device}"
        hist, stats = torch.empty(nbins, dtype=torch.int64, device=dev), torch.empty(_lib.SPECTRUM_STATS, dtype=torch.int64, device=dev)
        dev_call(self.device, "aix_tf_spectrum_dev", self._h, nbins, tptr(hist), tptr(stats))
        return hist, stats

    def tf_stats_t(self):
        return self.tf_spectrum_t(2)[1]

    def top_kmers_t(self, n: int = 0, min_tf: int = 1, want_kmers: bool = True):
        """(kid int32[m], tf int32[m], kmers uint8[m, k] | None, total) device tensors (u32 bit patterns); one call into buffers of
        min(n, self.n) entries, returned cut to the m entries selected."""
        import torch
        dev = f"cuda:{self.device}"
        min_tf = min(max(int(min_tf), 0), 1 << 32)
        n = self._cut(n, self.n)
        cap = 0 if min_tf >> 32 else (n if n else self.n)
        kid = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
        tf = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
        kmers = torch.empty((max(cap, 1), self.k), dtype=torch.uint8, device=dev) if want_kmers else None
        m, total = C.c_uint64(), C.c_uint64()
        if not min_tf >> 32:                                        # else: no u32 value reaches it
            dev_call(self.device, "aix_top_kmers_dev", self._h, min_tf, n, tptr(kid), tptr(tf), tptr(kmers), cap, C.byref(m), C.byref(total))
        assert m.value <= cap
        return kid[: m.value], tf[: m.value], (kmers[: m.value] if want_kmers else None), total.value

    def kmers_by_kid_t(self, kids_t, want_rc: bool = False, want_tf: bool = False):
        """kmers_by_kid on an int64 device tensor of kids (u64 bit patterns): (kmers uint8[N, k], rc | None, tf int32[N] | None)."""
        import torch
        self._chk_dev(kids_t)
        if kids_t.dtype != torch.int64:
            raise ValueError("kids: an int64 tensor")
        n, dev = kids_t.numel(), kids_t.device
        out = torch.empty((n, self.k), dtype=torch.uint8, device=dev)
        rc = torch.empty((n, self.k), dtype=torch.uint8, device=dev) if want_rc else None
        tf = torch.empty(n, dtype=torch.int32, device=dev) if want_tf else None
        dev_call(self.device, "aix_kmers_by_kid_dev", self._h, tptr_filled(kids_t), n, tptr_filled(out), tptr_filled(rc), tptr_filled(tf))
        return out, rc, tf

    # ---- HBM-resident (torch) entry points: asynchronous on torch's current stream ------------
    def _chk_dev(self, t):
        if not t.is_cuda or t.device.index != self.device:
            raise ValueError(f"tensor must live on cuda:{self.device}")
        if not t.is_contiguous():
            raise ValueError("tensor must be contiguous")

    def tf_ascii_t(self, kmers_t, out_t=None):
        import torch
        self._chk_dev(kmers_t)
        n = kmers_t.numel() // self.k
        if out_t is None:
            out_t = torch.empty(n, dtype=torch.int32, device=kmers_t.device)   # u32 bit patterns
        check(lib().aix_tf_batch_ascii_dev(self._h, vp(kmers_t.data_ptr()), n, vp(out_t.data_ptr()), _stream_ptr(self.device)),
              "aix_tf_batch_ascii_dev")
        return out_t

    def lines_ascii_t(self, kmers_t):
        """Instrumentation: records (128-byte lines) each tf query reads under the current settings."""
        import torch
        self._chk_dev(kmers_t)
        n = kmers_t.numel() // self.k
        out_t = torch.empty(n, dtype=torch.int32, device=kmers_t.device)
        check(lib().aix_lines_batch_ascii_dev(self._h, vp(kmers_t.data_ptr()), n, vp(out_t.data_ptr()), _stream_ptr(self.device)), "aix_lines_batch_ascii_dev")
        return out_t

    def tf_codes_t(self, codes_t, out_t=None):
        import torch
        self._chk_dev(codes_t)
        n = codes_t.numel()
        if out_t is None:
            out_t = torch.empty(n, dtype=torch.int32, device=codes_t.device)
        check(lib().aix_tf_batch_codes_dev(self._h, vp(codes_t.data_ptr()), n, vp(out_t.data_ptr()), _stream_ptr(self.device)),
              "aix_tf_batch_codes_dev")
        return out_t

    def total_ascii_t(self, kmers_t, out_t=None):
        import torch
        self._chk_dev(kmers_t)
        n = kmers_t.numel() // self.k
        if out_t is None:
            out_t = torch.empty(n, dtype=torch.int64, device=kmers_t.device)
        check(lib().aix_tf_total_batch_ascii_dev(self._h, vp(kmers_t.data_ptr()), n, vp(out_t.data_ptr()), _stream_ptr(self.device)),
              "aix_tf_total_batch_ascii_dev")
        return out_t

    def coverage_t(self, seqs_t, offs_t, out_offs_t, total_out: int, cutoff: int = 0, out_t=None):
        import torch
        self._chk_dev(seqs_t)
        m = offs_t.numel() - 1
        if out_t is None:
            out_t = torch.zeros(total_out, dtype=torch.int32, device=seqs_t.device)
        check(lib().aix_coverage_batch_dev(self._h, vp(seqs_t.data_ptr()), vp(offs_t.data_ptr()), m, seqs_t.numel(), cutoff,
                                           vp(out_t.data_ptr()), vp(out_offs_t.data_ptr()), _stream_ptr(self.device)), "aix_coverage_batch_dev")
        return out_t

    def positions_fill_t(self, reads_t):
        """A1 + A2 with the reads buffer already in HBM: (indices int64[n+1], positions int64[sum tf]) device tensors
        holding the u64 bit patterns of the .indices.bin / .index.bin images."""
        import torch
        self._chk_dev(reads_t)
        total = C.c_uint64()
        check(lib().aix_positions_total(self._h, C.byref(total)), "aix_positions_total")
        # the reference's start adjustment looks at the head of the buffer (hash.cpp:973-986); fetch as much of it as needed
        head_len, start = 1 << 16, C.c_uint64()
        while True:
            head = reads_t[:head_len].cpu().numpy()
            check(lib().aix_positions_start_k(_np_ptr(head), head.shape[0], self.k, C.byref(start)), "aix_positions_start_k")
            if head.shape[0] == reads_t.numel() or start.value + 64 < head.shape[0]:
                break
            head_len *= 16
        dev = reads_t.device
        indices = torch.empty(self.n + 1, dtype=torch.int64, device=dev)
        pos = torch.empty(max(total.value, 1), dtype=torch.int64, device=dev)[: total.value]
        with torch.cuda.device(dev):
            check(lib().aix_positions_fill_dev(self._h, vp(reads_t.data_ptr()), reads_t.numel(), start.value, vp(indices.data_ptr()),
                                               vp(pos.data_ptr()) if total.value else None, total.value, _stream_ptr(self.device)), "aix_positions_fill_dev")
        return indices, pos

    def count13_t(self, plain_t, out_t=None):
        import torch
        self._chk_dev(plain_t)
        if out_t is None:
            out_t = torch.empty(_lib.TOTAL_13MERS, dtype=torch.int64, device=plain_t.device)
        check(lib().aix_count13_dev(self._h, vp(plain_t.data_ptr()), plain_t.numel(), vp(out_t.data_ptr()), _stream_ptr(self.device)),
              "aix_count13_dev")
        return out_t

    def count23_fixed_t(self, plain_t, canon_mode: int = _lib.CANON_TRUE_RC, out_t=None):
        """Accumulates into out_t (int32[n], caller-zeroed when given)."""
        import torch
        self._chk_dev(plain_t)
        if out_t is None:
            out_t = torch.zeros(self.n, dtype=torch.int32, device=plain_t.device)
        check(lib().aix_count23_fixed_dev(self._h, vp(plain_t.data_ptr()), plain_t.numel(), canon_mode, vp(out_t.data_ptr()),
                                          _stream_ptr(self.device)), "aix_count23_fixed_dev")
        return out_t


# ---- synthetic inputs generated in HBM (mirrors aindex_amd/synth.py) ---------------------------
def synth_genome_t(seed: int, length: int, device: int = 0):
    import torch
    t = torch.empty(length, dtype=torch.uint8, device=f"cuda:{device}")
    with torch.cuda.device(device):
        check(lib().aix_synth_genome_dev(seed, length, vp(t.data_ptr()), _stream_ptr()), "aix_synth_genome_dev")
    return t


def synth_kmers_t(seed: int, n: int, k: int, device: int = 0, first: int = 0):
    import torch
    t = torch.empty(n * k + 16, dtype=torch.uint8, device=f"cuda:{device}")[: n * k]
    with torch.cuda.device(device):
        check(lib().aix_synth_kmers_dev(seed, first, n, k, vp(t.data_ptr()), _stream_ptr()), "aix_synth_kmers_dev")
    return t


def synth_reads_t(seed: int, genome_t, n_reads: int, read_len: int, rc_half: bool = False, n_rate_ppm: int = 0,
                  first_read: int = 0):
    import torch
    t = torch.empty(n_reads * (read_len + 1), dtype=torch.uint8, device=genome_t.device)
    with torch.cuda.device(genome_t.device):
        check(lib().aix_synth_reads_dev(seed, vp(genome_t.data_ptr()), genome_t.numel(), first_read, n_reads, read_len,
                                        int(rc_half), n_rate_ppm, vp(t.data_ptr()), _stream_ptr()), "aix_synth_reads_dev")
    return t


def synth_mix23_t(seed: int, genome_t, n: int, first: int = 0):
    """Q_mix: 50 % genome windows on a random strand, 50 % uniform-random 23-mers, generated in HBM."""
    import torch
    t = torch.empty(n * 23 + 16, dtype=torch.uint8, device=genome_t.device)[: n * 23]
    with torch.cuda.device(genome_t.device):
        check(lib().aix_synth_mix23_dev(seed, vp(genome_t.data_ptr()), genome_t.numel(), first, n, vp(t.data_ptr()), _stream_ptr()),
              "aix_synth_mix23_dev")
    return t


# ---- frequency view of any value tensor in HBM (aix_spectrum.hip; e.g. what count23_fixed_t / count13_t leave there) ----
def _values_arg(values_t):
    import torch
    if not values_t.is_cuda or not values_t.is_contiguous() or values_t.dtype not in (torch.int32, torch.int64):
        raise ValueError("values: a contiguous int32 (u32) or int64 (u64) tensor on the GPU")
    return 4 if values_t.dtype == torch.int32 else 8


def spectrum_t(values_t, nbins: int):
    """(hist int64[nbins], stats int64[8]) of a device tensor of u32 (int32) or u64 (int64, binned by their u32 view) values: hist[j] = entries
    equal to j for j < nbins - 1, hist[nbins - 1] = entries >= nbins - 1; stats: _lib.STATS_FIELDS. Asynchronous on torch's current stream."""
    import torch
    eb = _values_arg(values_t)
    if nbins < 2:
        raise ValueError("nbins must be at least 2")
    dev = values_t.device
    hist, stats = torch.empty(nbins, dtype=torch.int64, device=dev), torch.empty(_lib.SPECTRUM_STATS, dtype=torch.int64, device=dev)
    n = values_t.numel()
    with torch.cuda.device(dev):
        check(lib().aix_spectrum_dev(vp(values_t.data_ptr()) if n else None, eb, n, nbins, vp(hist.data_ptr()), vp(stats.data_ptr()), _stream_ptr(dev)),
              "aix_spectrum_dev")
    return hist, stats


def top_values_t(values_t, n: int = 0, min_v: int = 1, idx_t=None, val_t=None):
    """(idx int32[m], val int32[m], total) (u32 bit patterns): the first n (0 = all) entries with value >= min_v in descending value, ties in
    ascending index; total = entries >= min_v before the cut. An int64 tensor is taken by its u32 view. idx_t / val_t: caller-owned int32
    buffers; when the selection does not fit them they are left as they are and (None, None, total) is returned."""
    import torch
    eb = _values_arg(values_t)
    dev, cnt = values_t.device, values_t.numel()
    m, total = C.c_uint64(), C.c_uint64()
    min_v = max(int(min_v), 0)
    n = Index._cut(n, cnt)
    if min_v > 0xFFFFFFFF:                                          # no u32 value reaches it
        cnt, min_v = 0, 0
    with torch.cuda.device(dev):
        if eb == 8:
            narrow = torch.empty(cnt, dtype=torch.int32, device=dev)
            check(lib().aix_values_narrow_dev(vp(values_t.data_ptr()) if cnt else None, cnt, vp(narrow.data_ptr()) if cnt else None, _stream_ptr(dev)),
                  "aix_values_narrow_dev")
            values_t = narrow
        if idx_t is None:
            cap = min(n, cnt) if n else cnt
            idx_t = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)[:cap]
            val_t = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)[:cap]
        cap = idx_t.numel()
        if idx_t.dtype != torch.int32 or (val_t is not None and (val_t.dtype != torch.int32 or val_t.numel() < cap)):
            raise ValueError("idx_t / val_t: int32 tensors of equal length")
        check(lib().aix_select_dev(vp(values_t.data_ptr()) if cnt else None, cnt, min_v, n, vp(idx_t.data_ptr()) if cap else None,
                                   vp(val_t.data_ptr()) if (val_t is not None and cap) else None, cap, C.byref(m), C.byref(total), _stream_ptr(dev)),
              "aix_select_dev")
    if m.value > cap:
        return None, None, total.value
    return idx_t[: m.value], (val_t[: m.value] if val_t is not None else None), total.value
