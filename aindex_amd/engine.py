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
from ._lib import check, lib, vp


def _np_ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(vp)


def _as_u8(kmers, k: int) -> np.ndarray:
    """Accept bytes / (N,k) uint8 / flat uint8 and return a flat contiguous uint8 array of N*k bytes."""
    if isinstance(kmers, (bytes, bytearray, memoryview)):
        a = np.frombuffer(kmers, dtype=np.uint8)
    else:
        a = np.ascontiguousarray(kmers, dtype=np.uint8).reshape(-1)
    if a.shape[0] % k:
        raise ValueError(f"k-mer buffer length {a.shape[0]} is not a multiple of k={k}")
    return a


def _ragged(items: Sequence) -> Tuple[np.ndarray, np.ndarray]:
    bs = [s.encode("latin-1") if isinstance(s, str) else bytes(s) for s in items]
    offs = np.zeros(len(bs) + 1, dtype=np.uint64)
    if bs:
        offs[1:] = np.cumsum([len(b) for b in bs], dtype=np.uint64)
    return np.frombuffer(b"".join(bs), dtype=np.uint8), offs


def _stream_ptr(device=None):
    """torch's current stream ON `device` (the index's device): the library switches to the handle's device for the call,
    so a stream of whichever device happens to be current would be a stream of the wrong device."""
    import torch
    return vp(torch.cuda.current_stream(device).cuda_stream)


class Index:
    def __init__(self, handle: vp):
        self._h = handle
        self._info = _lib.Info()
        check(lib().aix_index_info(self._h, C.byref(self._info)), "aix_index_info")

    # ---- lifecycle ---------------------------------------------------------------------------
    @classmethod
    def open_23(cls, pf: str, tf_bin: str, kmers_bin: str, device: int = 0) -> "Index":
        h = vp()
        check(lib().aix_index_open_23(pf.encode(), tf_bin.encode(), kmers_bin.encode(), device, C.byref(h)),
              f"aix_index_open_23({pf})")
        return cls(h)

    @classmethod
    def open_13(cls, pf: str, tf_bin: Optional[str], device: int = 0) -> "Index":
        h = vp()
        check(lib().aix_index_open_13(pf.encode(), tf_bin.encode() if tf_bin else None, device, C.byref(h)),
              f"aix_index_open_13({pf})")
        return cls(h)

    @classmethod
    def create_23(cls, pf_bytes: bytes, checker: np.ndarray, tf: np.ndarray, device: int = 0) -> "Index":
        checker = np.ascontiguousarray(checker, dtype=np.uint64)
        tf = np.ascontiguousarray(tf, dtype=np.uint32)
        assert checker.shape == tf.shape
        h = vp()
        buf = np.frombuffer(pf_bytes, dtype=np.uint8)
        check(lib().aix_index_create_23(_np_ptr(buf), buf.shape[0], _np_ptr(checker), _np_ptr(tf), checker.shape[0],
                                        device, C.byref(h)), "aix_index_create_23")
        return cls(h)

    @classmethod
    def create_13(cls, pf_bytes: bytes, tf: Optional[np.ndarray] = None, device: int = 0) -> "Index":
        if tf is not None:
            tf = np.ascontiguousarray(tf, dtype=np.uint64)
            assert tf.shape[0] == _lib.TOTAL_13MERS
        h = vp()
        buf = np.frombuffer(pf_bytes, dtype=np.uint8)
        check(lib().aix_index_create_13(_np_ptr(buf), buf.shape[0], _np_ptr(tf), device, C.byref(h)), "aix_index_create_13")
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
            check(lib().aix_index_build_23_codes_dev(_np_ptr(buf), buf.shape[0], vp(keys_t.data_ptr()),
                                                     vp(counts_t.data_ptr()) if counts_t is not None else None,
                                                     keys_t.numel(), dev, _stream_ptr(dev), C.byref(h)), "aix_index_build_23_codes_dev")
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
        check(lib().aix_index_set_tf_13(self._h, _np_ptr(tf)), "aix_index_set_tf_13")

    def tf_array(self) -> np.ndarray:
        out = np.empty(self.n, dtype=np.uint64 if self.k == 13 else np.uint32)
        check(lib().aix_index_get_tf(self._h, _np_ptr(out), out.nbytes), "aix_index_get_tf")
        return out

    def checker_array(self) -> np.ndarray:
        out = np.empty(self.n, dtype=np.uint64)
        check(lib().aix_index_get_checker(self._h, _np_ptr(out), out.shape[0]), "aix_index_get_checker")
        return out

    # ---- host-memory queries -----------------------------------------------------------------
    def tf_ascii(self, kmers) -> np.ndarray:
        a = _as_u8(kmers, self.k)
        n = a.shape[0] // self.k
        out = np.empty(n, dtype=np.uint32)
        check(lib().aix_tf_batch_ascii(self._h, _np_ptr(a), n, _np_ptr(out)), "aix_tf_batch_ascii")
        return out

    def tf_ascii_into(self, a: np.ndarray, out: np.ndarray) -> np.ndarray:
        """tf_ascii on caller-owned buffers (contiguous uint8[n*k] in, uint32[n] out) — e.g. pinned staging kept between calls."""
        assert a.dtype == np.uint8 and out.dtype == np.uint32 and a.flags.c_contiguous and out.flags.c_contiguous and a.shape[0] == out.shape[0] * self.k
        check(lib().aix_tf_batch_ascii(self._h, _np_ptr(a), out.shape[0], _np_ptr(out)), "aix_tf_batch_ascii")
        return out

    def tf_codes(self, codes: np.ndarray) -> np.ndarray:
        c = np.ascontiguousarray(codes, dtype=np.uint64)
        out = np.empty(c.shape[0], dtype=np.uint32)
        check(lib().aix_tf_batch_codes(self._h, _np_ptr(c), c.shape[0], _np_ptr(out)), "aix_tf_batch_codes")
        return out

    def tf_ragged(self, items: Sequence) -> np.ndarray:
        data, offs = _ragged(items)
        out = np.empty(len(items), dtype=np.uint32)
        check(lib().aix_tf_batch_ragged(self._h, _np_ptr(data), _np_ptr(offs), len(items), _np_ptr(out)), "aix_tf_batch_ragged")
        return out

    def hash_ascii(self, kmers) -> np.ndarray:
        a = _as_u8(kmers, self.k)
        n = a.shape[0] // self.k
        out = np.empty(n, dtype=np.uint64)
        check(lib().aix_hash_batch_ascii(self._h, _np_ptr(a), n, _np_ptr(out)), "aix_hash_batch_ascii")
        return out

    def kid_strand_ascii(self, kmers) -> Tuple[np.ndarray, np.ndarray]:
        a = _as_u8(kmers, self.k)
        n = a.shape[0] // self.k
        kid = np.empty(n, dtype=np.uint64)
        strand = np.empty(n, dtype=np.uint8)
        check(lib().aix_kid_strand_batch_ascii(self._h, _np_ptr(a), n, _np_ptr(kid), _np_ptr(strand)), "aix_kid_strand_batch_ascii")
        return kid, strand

    def both_ascii(self, kmers) -> Tuple[np.ndarray, np.ndarray]:
        a = _as_u8(kmers, self.k)
        n = a.shape[0] // self.k
        f = np.empty(n, dtype=np.uint64)
        r = np.empty(n, dtype=np.uint64)
        check(lib().aix_tf_both_batch_ascii(self._h, _np_ptr(a), n, _np_ptr(f), _np_ptr(r)), "aix_tf_both_batch_ascii")
        return f, r

    def total_ascii(self, kmers) -> np.ndarray:
        a = _as_u8(kmers, self.k)
        n = a.shape[0] // self.k
        out = np.empty(n, dtype=np.uint64)
        check(lib().aix_tf_total_batch_ascii(self._h, _np_ptr(a), n, _np_ptr(out)), "aix_tf_total_batch_ascii")
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
            check(lib().aix_coverage_batch(self._h, _np_ptr(data), _np_ptr(offs), len(seqs), cutoff, _np_ptr(out), _np_ptr(ooffs)),
                  "aix_coverage_batch")
        return [out[int(ooffs[i]):int(ooffs[i + 1])] for i in range(len(seqs))]

    # ---- counting ----------------------------------------------------------------------------
    def count13(self, buf: bytes, fmt: int = _lib.FMT_AUTO) -> np.ndarray:
        a = np.frombuffer(buf, dtype=np.uint8)
        out = np.empty(_lib.TOTAL_13MERS, dtype=np.uint64)
        check(lib().aix_count13(self._h, _np_ptr(a), a.shape[0], fmt, _np_ptr(out)), "aix_count13")
        return out

    def count23_fixed(self, buf: bytes, fmt: int = _lib.FMT_AUTO, canon_mode: int = _lib.CANON_TRUE_RC) -> np.ndarray:
        a = np.frombuffer(buf, dtype=np.uint8)
        out = np.zeros(self.n, dtype=np.uint32)
        check(lib().aix_count23_fixed(self._h, _np_ptr(a), a.shape[0], fmt, canon_mode, _np_ptr(out)), "aix_count23_fixed")
        return out

    def count13_file(self, path: str, out_path: Optional[str] = None, fmt: int = _lib.FMT_AUTO, want_array: bool = True):
        """count_kmers13 on a FILE, streamed (aix_count13_file: the file is read part by part into pinned staging while the previous part is
        counted; the host never holds it). Returns (u64[4^13] or None, stats dict); out_path receives the reference's output file."""
        out = np.empty(_lib.TOTAL_13MERS, dtype=np.uint64) if want_array else None
        st = _lib.IngestStats()
        check(lib().aix_count13_file(self._h, os.fsencode(path), fmt, os.fsencode(out_path) if out_path else None, _np_ptr(out), C.byref(st)),
              f"aix_count13_file({path})")
        return out, st.as_dict()

    def count23_fixed_file(self, path: str, fmt: int = _lib.FMT_AUTO, canon_mode: int = _lib.CANON_TRUE_RC):
        """aix_count23_fixed on a FILE, streamed. Returns (u32[n], stats dict)."""
        out = np.zeros(self.n, dtype=np.uint32)
        st = _lib.IngestStats()
        check(lib().aix_count23_fixed_file(self._h, os.fsencode(path), fmt, canon_mode, _np_ptr(out), C.byref(st)), f"aix_count23_fixed_file({path})")
        return out, st.as_dict()

    def positions_fill(self, reads):
        """A1 + A2: (indices uint64[n+1], positions uint64[sum tf]) = the .indices.bin / .index.bin images.
        `reads`: bytes or any buffer (e.g. a numpy memmap of the reads file: nothing is copied on the host)."""
        a = np.frombuffer(reads, dtype=np.uint8)
        indices = np.empty(self.n + 1, dtype=np.uint64)
        total = C.c_uint64()
        check(lib().aix_positions_fill(self._h, _np_ptr(a), a.shape[0], _np_ptr(indices), None, 0, C.byref(total)), "aix_positions_fill")
        pos = np.zeros(total.value, dtype=np.uint64)
        check(lib().aix_positions_fill(self._h, _np_ptr(a), a.shape[0], _np_ptr(indices), _np_ptr(pos), pos.shape[0], C.byref(total)),
              "aix_positions_fill")
        return indices, pos

    def positions_indices(self) -> np.ndarray:
        """A1 alone: uint64[n+1] exclusive prefix sum of tf (the .indices.bin image)."""
        indices = np.empty(self.n + 1, dtype=np.uint64)
        total = C.c_uint64()
        check(lib().aix_positions_fill(self._h, None, 0, _np_ptr(indices), None, 0, C.byref(total)), "aix_positions_fill")
        return indices

    def positions_bucket_counts(self, reads: bytes, first_shard: bool = True) -> np.ndarray:
        """uint64[n]: windows of `reads` per bucket under A2's rules (the shard-local ppositions counters)."""
        a = np.frombuffer(reads, dtype=np.uint8)
        out = np.zeros(self.n, dtype=np.uint64)
        check(lib().aix_positions_bucket_counts(self._h, _np_ptr(a), a.shape[0], int(first_shard), _np_ptr(out)), "aix_positions_bucket_counts")
        return out

    def positions_fill_shard(self, reads: bytes, total: int, first_shard: bool, base_offset: int, filled_init: Optional[np.ndarray]) -> np.ndarray:
        """uint64[total]: this shard's entries of the positions array (zero elsewhere); see aix_positions_fill_shard."""
        a = np.frombuffer(reads, dtype=np.uint8)
        pos = np.zeros(total, dtype=np.uint64)
        f = None if filled_init is None else np.ascontiguousarray(filled_init, dtype=np.uint32)
        check(lib().aix_positions_fill_shard(self._h, _np_ptr(a), a.shape[0], int(first_shard), base_offset, _np_ptr(f), _np_ptr(pos), pos.shape[0]),
              "aix_positions_fill_shard")
        return pos

    # ---- batch position queries over an attached positions index (aix_posquery.hip) -----------
    def attach_aindex(self, indices, positions):
        """Copy the .indices.bin (n + 1) / .index.bin images (numpy arrays or memmaps, uint64) to HBM for positions_batch."""
        ind = np.ascontiguousarray(indices, dtype=np.uint64)
        pos = np.ascontiguousarray(positions, dtype=np.uint64)
        if ind.shape[0] != self.n + 1:
            raise ValueError(f"indices holds {ind.shape[0]} entries, the handle needs n + 1 = {self.n + 1}")
        check(lib().aix_aindex_attach(self._h, _np_ptr(ind), _np_ptr(pos) if pos.shape[0] else None, pos.shape[0]), "aix_aindex_attach")
        self._aindex_keep = None

    def attach_aindex_t(self, indices_t, positions_t):
        """Borrow device tensors (int64 bit patterns, e.g. the outputs of positions_fill_t); they are kept alive by this object."""
        self._chk_dev(indices_t)
        if positions_t.numel():
            self._chk_dev(positions_t)
        if indices_t.numel() != self.n + 1:
            raise ValueError(f"indices holds {indices_t.numel()} entries, the handle needs n + 1 = {self.n + 1}")
        check(lib().aix_aindex_attach_dev(self._h, vp(indices_t.data_ptr()), vp(positions_t.data_ptr()) if positions_t.numel() else None,
                                          positions_t.numel(), _stream_ptr(self.device)), "aix_aindex_attach_dev")
        self._aindex_keep = (indices_t, positions_t)

    def detach_aindex(self):
        check(lib().aix_aindex_detach(self._h), "aix_aindex_detach")
        self._aindex_keep = None

    def attach_ridx(self, triples) -> bool:
        """Read intervals (rid, start, end per read) to HBM. False when they are not sorted and disjoint: nothing is attached then and
        locate=True / locate() are refused."""
        t = np.ascontiguousarray(triples, dtype=np.uint64).reshape(-1, 3)
        st = lib().aix_ridx_attach(self._h, _np_ptr(t) if t.shape[0] else None, t.shape[0])
        if st == _lib.AIX_ERR_UNSUPPORTED:
            return False
        check(st, "aix_ridx_attach")
        return True

    @staticmethod
    def _take(p, n: int, dtype=np.uint64) -> np.ndarray:
        """n entries of a malloc'd output block of the C ABI as a numpy array of its own; the block is freed."""
        dt = np.dtype(dtype)
        try:
            return np.frombuffer(C.string_at(p, dt.itemsize * n), dtype=dt).copy() if n else np.zeros(0, dt)
        finally:
            lib().aix_free(p)

    _take_as = _take                                          # the name with the dtype spelt out, as tests/test_gpu_seqedit.py calls it

    def positions_batch(self, kmers, max_per_kmer: int = 0, locate: bool = False):
        """(offsets[N + 1], positions[offsets[N]][, rid, offset_in_read]) as numpy uint64: list i = positions[offsets[i]:offsets[i + 1]] =
        get_positions(kmer i), cut to max_per_kmer entries when that is > 0. `kmers`: what tf_ascii takes."""
        a = _as_u8(kmers, self.k)
        n = a.shape[0] // self.k
        po, pp, pr, pl = vp(), vp(), vp(), vp()
        check(lib().aix_positions_query(self._h, _np_ptr(a) if n else None, n, max_per_kmer, C.byref(po), C.byref(pp),
                                        C.byref(pr) if locate else None, C.byref(pl) if locate else None), "aix_positions_query")
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
        dev = kmers_t.device
        offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
        total = C.c_uint64()
        with torch.cuda.device(dev):
            q = vp(kmers_t.data_ptr()) if n else None
            check(lib().aix_positions_query_dev(self._h, q, n, max_per_kmer, vp(offsets.data_ptr()), None, None, None, 0, C.byref(total),
                                                _stream_ptr(self.device)), "aix_positions_query_dev")
            t = total.value
            outs = [torch.empty(max(t, 1), dtype=torch.int64, device=dev)[:t] for _ in range(3 if locate else 1)]
            if t:
                check(lib().aix_positions_query_dev(self._h, q, n, max_per_kmer, vp(offsets.data_ptr()), vp(outs[0].data_ptr()),
                                                    vp(outs[1].data_ptr()) if locate else None, vp(outs[2].data_ptr()) if locate else None, t,
                                                    C.byref(total), _stream_ptr(self.device)), "aix_positions_query_dev")
        return (offsets, *outs)

    def locate(self, pos):
        """(rid, start) per position: get_rid / get_start for a batch (numpy uint64 in and out)."""
        p = np.ascontiguousarray(pos, dtype=np.uint64).reshape(-1)
        rid, start = np.empty(p.shape[0], np.uint64), np.empty(p.shape[0], np.uint64)
        check(lib().aix_positions_locate(self._h, _np_ptr(p), p.shape[0], _np_ptr(rid), _np_ptr(start)), "aix_positions_locate")
        return rid, start

    # ---- batch read retrieval over an attached reads file (aix_readsquery.hip) -----------------
    def attach_reads(self, buf):
        """Copy the .reads image (bytes, numpy uint8 array or memmap) to HBM for fetch_reads* / reads_by_kmers."""
        a = np.frombuffer(buf, dtype=np.uint8) if isinstance(buf, (bytes, bytearray, memoryview)) else np.ascontiguousarray(buf, dtype=np.uint8).reshape(-1)
        check(lib().aix_reads_attach(self._h, _np_ptr(a) if a.shape[0] else None, a.shape[0]), "aix_reads_attach")
        self._reads_keep = None

    def attach_reads_t(self, t):
        """Borrow a uint8 device tensor (e.g. synth_reads_t output); it is kept alive by this object."""
        if t.numel():
            self._chk_dev(t)
        check(lib().aix_reads_attach_dev(self._h, vp(t.data_ptr()) if t.numel() else None, t.numel(), _stream_ptr(self.device)), "aix_reads_attach_dev")
        self._reads_keep = t

    def detach_reads(self):
        check(lib().aix_reads_detach(self._h), "aix_reads_detach")
        self._reads_keep = None

    def reads_info(self) -> Tuple[int, int]:
        """(0 nothing / 1 copied / 2 borrowed, bytes) of the attached reads."""
        out = (C.c_uint64 * 2)()
        check(lib().aix_reads_info(self._h, C.byref(out)), "aix_reads_info")
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
        check(lib().aix_reads_fetch(self._h, _np_ptr(s) if n else None, _np_ptr(e) if n else None, _np_ptr(r) if n else None, n, C.byref(po), C.byref(pb)),
              "aix_reads_fetch")
        offsets = self._take(po, n + 1)
        return offsets, self._take(pb, int(offsets[n]), np.uint8)

    def fetch_reads_by_rid(self, rids):
        """(offsets, bytes): item i = get_read_by_rid(rids[i]) over the intervals of attach_ridx."""
        r = np.ascontiguousarray(rids, dtype=np.uint64).reshape(-1)
        n = r.shape[0]
        po, pb = vp(), vp()
        check(lib().aix_reads_fetch_rid(self._h, _np_ptr(r) if n else None, n, C.byref(po), C.byref(pb)), "aix_reads_fetch_rid")
        offsets = self._take(po, n + 1)
        return offsets, self._take(pb, int(offsets[n]), np.uint8)

    def reads_by_kmers(self, kmers, max_reads: int = 100):
        """(kmer_offsets uint64[N + 1], rid uint64[R], read_offsets uint64[R + 1], bytes uint8): the reads of k-mer i are
        rid[kmer_offsets[i]:kmer_offsets[i + 1]], read j's bytes are bytes[read_offsets[j]:read_offsets[j + 1]]."""
        a = _as_u8(kmers, self.k)
        n = a.shape[0] // self.k
        pk, pr, po, pb = vp(), vp(), vp(), vp()
        check(lib().aix_reads_by_kmers(self._h, _np_ptr(a) if n else None, n, max_reads, C.byref(pk), C.byref(pr), C.byref(po), C.byref(pb)), "aix_reads_by_kmers")
        koff = self._take(pk, n + 1)
        nr = int(koff[n])
        rid = self._take(pr, nr)
        roff = self._take(po, nr + 1)
        return koff, rid, roff, self._take(pb, int(roff[nr]), np.uint8)

    def _fetch_t(self, what: str, n: int, dev, call):
        """The sizing call, then the filling call into a tensor of exactly that size (int64 offsets, uint8 bytes)."""
        import torch
        offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
        total = C.c_uint64()
        with torch.cuda.device(dev):
            check(call(vp(offsets.data_ptr()), None, 0, C.byref(total)), what)
            t = total.value
            out = torch.empty(max(t, 1), dtype=torch.uint8, device=dev)[:t]
            if t:
                check(call(vp(offsets.data_ptr()), vp(out.data_ptr()), t, C.byref(total)), what)
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
        s, e, r = vp(starts_t.data_ptr()), vp(ends_t.data_ptr()), vp(revcomp_t.data_ptr()) if revcomp_t is not None else None
        st = _stream_ptr(self.device)
        return self._fetch_t("aix_reads_fetch_dev", n, starts_t.device,
                             lambda off, by, cap, tot: lib().aix_reads_fetch_dev(self._h, s if n else None, e if n else None, r if n else None, n, off, by, cap, tot, st))

    def fetch_reads_by_rid_t(self, rids_t):
        """fetch_reads_by_rid on an int64 device tensor, e.g. the rid output of positions_batch_t(..., locate=True)."""
        self._chk_dev(rids_t)
        n = rids_t.numel()
        r, st = vp(rids_t.data_ptr()), _stream_ptr(self.device)
        return self._fetch_t("aix_reads_fetch_rid_dev", n, rids_t.device,
                             lambda off, by, cap, tot: lib().aix_reads_fetch_rid_dev(self._h, r if n else None, n, off, by, cap, tot, st))

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
            check(lib().aix_reads_by_kmers_dev(self._h, q, n, max_reads, vp(koff.data_ptr()), None, None, 0, None, 0, C.byref(tot), st), "aix_reads_by_kmers_dev")
            nr, nb = int(tot[0]), int(tot[1])
            rid = torch.empty(max(nr, 1), dtype=torch.int64, device=dev)[:nr]
            roff = torch.zeros(nr + 1, dtype=torch.int64, device=dev)
            by = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)[:nb]
            if nr:
                check(lib().aix_reads_by_kmers_dev(self._h, q, n, max_reads, vp(koff.data_ptr()), vp(rid.data_ptr()), vp(roff.data_ptr()), nr,
                                                   vp(by.data_ptr()) if nb else None, nb, C.byref(tot), st), "aix_reads_by_kmers_dev")
        return koff, rid, roff, by

    # ---- sequences against the indexed reads (aix_seqhits.hip) ---------------------------------
    def _seq_host(self, what: str, seqs: Sequence, dtypes, *args):
        """offsets + one array per dtype through a host form: ragged sequences in, one malloc'd block per output back; the first is the
        offsets[M + 1], every other one holds offsets[M] entries."""
        data, offs = _ragged(seqs)
        m = len(seqs)
        ps = [vp() for _ in range(1 + len(dtypes))]
        check(getattr(lib(), what)(self._h, _np_ptr(data) if data.shape[0] else None, _np_ptr(offs), m, *args, *[C.byref(p) for p in ps]), what)
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

    def _seq_t(self, what: str, seqs_t, offs_t, dtypes, cap_hint: int, call):
        """offsets + one tensor per dtype through a `_dev` twin: filled in one call when cap_hint entries suffice, else sized, then filled."""
        import torch
        self._chk_dev(seqs_t)
        self._chk_dev(offs_t)
        m = offs_t.numel() - 1
        dev = seqs_t.device
        offsets = torch.empty(m + 1, dtype=torch.int64, device=dev)
        total = C.c_uint64()
        with torch.cuda.device(dev):
            cap = max(int(cap_hint), 0)
            while True:
                outs = [torch.empty(max(cap, 1), dtype=dt, device=dev) for dt in dtypes]
                check(call(m, vp(offsets.data_ptr()), [vp(o.data_ptr()) if cap else None for o in outs], cap, C.byref(total)), what)
                if total.value <= cap:
                    break
                cap = total.value
        return (offsets, *[o[:total.value] for o in outs])

    def seq_hits_t(self, seqs_t, offs_t, max_per_kmer: int = 0, cap_hint: int = 0):
        """seq_hits on device tensors (uint8 bytes, int64 offsets[M + 1] into them), on torch's current stream:
        (seq_offsets int64, qoff int32, pos int64, rid int64, local int64, flag uint8) — bit patterns of the unsigned fields."""
        import torch
        st = _stream_ptr(self.device)
        return self._seq_t("aix_seq_hits_dev", seqs_t, offs_t, [torch.int32, torch.int64, torch.int64, torch.int64, torch.uint8], cap_hint,
                           lambda m, off, o, cap, tot: lib().aix_seq_hits_dev(self._h, vp(seqs_t.data_ptr()), vp(offs_t.data_ptr()), m, max_per_kmer, off, *o, cap, tot, st))

    def seq_votes_t(self, seqs_t, offs_t, min_votes: int = 1, max_per_kmer: int = 0, cap_hint: int = 0):
        """seq_votes on device tensors: (vote_offsets int64, rid int64, strand uint8, diag int64, votes int32, q_first int32, q_last int32)."""
        import torch
        st = _stream_ptr(self.device)
        return self._seq_t("aix_seq_votes_dev", seqs_t, offs_t, [torch.int64, torch.uint8, torch.int64, torch.int32, torch.int32, torch.int32], cap_hint,
                           lambda m, off, o, cap, tot: lib().aix_seq_votes_dev(self._h, vp(seqs_t.data_ptr()), vp(offs_t.data_ptr()), m, max_per_kmer, min_votes, off,
                                                                               *o, cap, tot, st))

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
        st = _stream_ptr(self.device)
        return self._seq_t("aix_seq_find_dev", seqs_t, offs_t, [torch.int64, torch.int64, torch.int64, torch.uint8, torch.int32], cap_hint,
                           lambda m, off, o, cap, tot: lib().aix_seq_find_dev(self._h, vp(seqs_t.data_ptr()), vp(offs_t.data_ptr()), m, hd, seed_step, max_per_kmer, off,
                                                                              *o, cap, tot, st))

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
        st = _stream_ptr(self.device)
        return self._seq_t("aix_seq_edit_dev", seqs_t, offs_t, [torch.int64, torch.int64, torch.int64, torch.int64, torch.uint8, torch.int32], cap_hint,
                           lambda m, off, o, cap, tot: lib().aix_seq_edit_dev(self._h, vp(seqs_t.data_ptr()), vp(offs_t.data_ptr()), m, ed, seed_step, max_per_kmer, off,
                                                                              *o, cap, tot, st))

    def kmer_strands(self, kmers, max_per_kmer: int = 0):
        """(plus, minus, total) uint64[N]: of the listed hits of every 23-mer (`kmers`: what tf_ascii takes), those where the reads hold it
        as given, those where they hold its reverse complement, and all of them."""
        a = _as_u8(kmers, 23)
        n = a.shape[0] // 23
        out = [np.zeros(n, np.uint64) for _ in range(3)]
        check(lib().aix_kmer_strands(self._h, _np_ptr(a) if n else None, n, max_per_kmer, *[_np_ptr(o) if n else None for o in out]), "aix_kmer_strands")
        return tuple(out)

    def kmer_strands_t(self, kmers_t, max_per_kmer: int = 0):
        """kmer_strands on a uint8 device tensor of N * 23 bytes: three int64 device tensors, on torch's current stream."""
        import torch
        self._chk_dev(kmers_t)
        n = kmers_t.numel() // 23
        out = [torch.zeros(n, dtype=torch.int64, device=kmers_t.device) for _ in range(3)]
        with torch.cuda.device(kmers_t.device):
            check(lib().aix_kmer_strands_dev(self._h, vp(kmers_t.data_ptr()) if n else None, n, max_per_kmer, *[vp(o.data_ptr()) if n else None for o in out],
                                             _stream_ptr(self.device)), "aix_kmer_strands_dev")
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
        check(lib().aix_neighbours(self._h, _np_ptr(c) if n else None, _np_ptr(a) if n else None, n, d, cutoff, _np_ptr(out) if n else None), "aix_neighbours")
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
        check(lib().aix_walk(self._h, _np_ptr(c) if s else None, _np_ptr(a) if s else None, s, d, max_steps, cutoff, m, _np_ptr(bases), _np_ptr(length),
                             _np_ptr(stop), _np_ptr(tf), _np_ptr(last)), "aix_walk")
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
        with torch.cuda.device(kmers_or_codes_t.device):
            check(lib().aix_neighbours_dev(self._h, c if n else None, a if n else None, n, d, cutoff, vp(out_t.data_ptr()) if n else None,
                                           _stream_ptr(self.device)), "aix_neighbours_dev")
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
        with torch.cuda.device(dev):
            check(lib().aix_walk_dev(self._h, c if s else None, a if s else None, s, d, max_steps, cutoff, m, vp(bases_t.data_ptr()) if s else None,
                                     vp(length.data_ptr()) if s else None, vp(stop.data_ptr()) if s else None,
                                     vp(tf_t.data_ptr()) if (tf_t is not None and s) else None, vp(last.data_ptr()) if s else None,
                                     _stream_ptr(self.device)), "aix_walk_dev")
        return bases_t, length, stop, tf_t, last

    # ---- De Bruijn compaction (aix_unitigs.hip) ---------------------------------------------------
    UNITIG_KEYS = ("offsets", "bases", "circular", "tf_sum", "tf_min", "tf_max", "kmer_tf", "kid_unitig", "kid_pos", "kid_flag")

    def unitigs_layout_t(self, cutoff: int = 0):
        """The graph analysed once: (kid_unitig int64[n], kid_pos int32[n], kid_flag uint8[n], U, total_bases, n_live, n_circular) — device
        tensors (u64 / u32 bit patterns; a dead kid holds -1 = AIX_UNITIG_NONE, 0, 0) and ints. Complete on return."""
        import torch
        dev = f"cuda:{self.device}"
        ku = torch.empty(self.n, dtype=torch.int64, device=dev)
        kp = torch.empty(self.n, dtype=torch.int32, device=dev)
        kf = torch.empty(self.n, dtype=torch.uint8, device=dev)
        u, total, live, circ = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        with torch.cuda.device(self.device):
            check(lib().aix_unitigs_layout_dev(self._h, cutoff, vp(ku.data_ptr()), vp(kp.data_ptr()), vp(kf.data_ptr()), C.byref(u), C.byref(total),
                                               C.byref(live), C.byref(circ), _stream_ptr(self.device)), "aix_unitigs_layout_dev")
        return ku, kp, kf, u.value, total.value, live.value, circ.value

    def unitigs_t(self, cutoff: int = 0, want_kmer_tf: bool = False, layout=None) -> dict:
        """All maximal unitigs at `cutoff` as a dict of device tensors (u64 / u32 bit patterns): offsets int64[U + 1], bases uint8[offsets[U]],
        circular uint8[U], tf_sum int64[U], tf_min / tf_max int32[U], kmer_tf int32[n_live] | None (k-mer j of unitig u at
        offsets[u] - 22 u + j), the three per-kid arrays, and the ints U, n_live, n_circular. layout: what unitigs_layout_t(cutoff) returned."""
        import torch
        ku, kp, kf, u, total, live, circ = layout if layout is not None else self.unitigs_layout_t(cutoff)
        for t in (ku, kp, kf):
            self._chk_dev(t)
        dev = ku.device
        out = {"offsets": torch.empty(u + 1, dtype=torch.int64, device=dev), "bases": torch.empty(total, dtype=torch.uint8, device=dev),
               "circular": torch.empty(u, dtype=torch.uint8, device=dev), "tf_sum": torch.empty(u, dtype=torch.int64, device=dev),
               "tf_min": torch.empty(u, dtype=torch.int32, device=dev), "tf_max": torch.empty(u, dtype=torch.int32, device=dev),
               "kmer_tf": torch.empty(live, dtype=torch.int32, device=dev) if want_kmer_tf else None}
        p = lambda t: vp(t.data_ptr()) if t is not None else None
        with torch.cuda.device(self.device):
            check(lib().aix_unitigs_emit_dev(self._h, cutoff, p(ku), p(kp), p(kf), u, p(out["offsets"]), p(out["bases"]), p(out["circular"]), p(out["tf_sum"]),
                                             p(out["tf_min"]), p(out["tf_max"]), p(out["kmer_tf"]), _stream_ptr(self.device)), "aix_unitigs_emit_dev")
        out.update(kid_unitig=ku, kid_pos=kp, kid_flag=kf, U=u, n_live=live, n_circular=circ)
        return out

    def unitigs(self, cutoff: int = 0, want_kmer_tf: bool = False) -> dict:
        """unitigs_t through host memory: the same dict with numpy arrays (offsets / tf_sum / kid_unitig uint64, tf_min / tf_max / kmer_tf /
        kid_pos uint32)."""
        ps = [vp() for _ in range(10)]
        u = C.c_uint64()
        refs = [C.byref(q) for q in ps]
        if not want_kmer_tf:
            refs[6] = None
        check(lib().aix_unitigs(self._h, cutoff, C.byref(u), *refs), "aix_unitigs")
        U = u.value
        off = self._take(ps[0], U + 1, np.uint64)
        total = int(off[U])
        live = total - 22 * U
        sizes = (None, total, U, U, U, U, live, self.n, self.n, self.n)
        types = (None, np.uint8, np.uint8, np.uint64, np.uint32, np.uint32, np.uint32, np.uint64, np.uint32, np.uint8)
        out = {"offsets": off}
        for i in range(1, 10):
            out[self.UNITIG_KEYS[i]] = self._take(ps[i], sizes[i], types[i]) if refs[i] is not None else None
        out.update(U=U, n_live=live, n_circular=int(out["circular"].sum()))
        return out

    def unitig_links_t(self, cutoff: int = 0, unitigs=None) -> dict:
        """The unitig graph at `cutoff` as a dict of device tensors (u64 / u32 bit patterns): link_off int64[2 U + 1], link_to int32[E] — the
        links of end 2 u + side (side 0 leaves unitig u at the right end of its spelling, side 1 at the left) are the words 2 v + r at
        link_to[link_off[e] : link_off[e + 1]] —, bubble_mate int32[U] (-1 = none), and the ints U, E. unitigs: what unitigs_t(cutoff) returned."""
        import torch
        un = unitigs if unitigs is not None else self.unitigs_t(cutoff)
        ku, kp, kf, off, u = un["kid_unitig"], un["kid_pos"], un["kid_flag"], un["offsets"], int(un["U"])
        for t in (ku, kp, kf, off):
            self._chk_dev(t)
        if off.numel() != u + 1:
            raise ValueError("offsets must hold U + 1 entries")
        dev = ku.device
        link_off = torch.empty(2 * u + 1, dtype=torch.int64, device=dev)
        link_to = torch.empty(8 * u, dtype=torch.int32, device=dev)
        mate = torch.empty(u, dtype=torch.int32, device=dev)
        e = C.c_uint64()
        p = lambda t: vp(t.data_ptr())
        with torch.cuda.device(self.device):
            check(lib().aix_unitig_links_dev(self._h, cutoff, p(ku), p(kp), p(kf), u, p(off), p(link_off), p(link_to), 8 * u, C.byref(e),
                                             _stream_ptr(self.device)), "aix_unitig_links_dev")
            link_to = link_to[:e.value].clone()
            check(lib().aix_unitig_bubbles_dev(u, p(link_off), p(link_to), e.value, p(mate), _stream_ptr(self.device)), "aix_unitig_bubbles_dev")
        return {"link_off": link_off, "link_to": link_to, "bubble_mate": mate, "U": u, "E": e.value}

    def unitig_links(self, cutoff: int = 0) -> dict:
        """unitig_links_t through host memory: link_off uint64[2 U + 1], link_to uint32[E], bubble_mate uint32[U] (0xFFFFFFFF = none), U, E."""
        ps = [vp() for _ in range(3)]
        u, e = C.c_uint64(), C.c_uint64()
        check(lib().aix_unitig_links(self._h, cutoff, C.byref(u), C.byref(e), *[C.byref(q) for q in ps]), "aix_unitig_links")
        return {"link_off": self._take(ps[0], 2 * u.value + 1, np.uint64), "link_to": self._take(ps[1], e.value, np.uint32),
                "bubble_mate": self._take(ps[2], u.value, np.uint32), "U": u.value, "E": e.value}

    # ---- graph cleaning (aix_graphclean.hip) ------------------------------------------------------
    GRAPH_KEYS = ("offsets", "bases", "circular", "tf_sum", "tf_min", "tf_max", "link_off", "link_to")
    GRAPH_DTYPES = (np.uint64, np.uint8, np.uint8, np.uint64, np.uint32, np.uint32, np.uint64, np.uint32)

    @classmethod
    def _graph_of(cls, unitigs: dict, links) -> dict:
        """the eight arrays of a unitig set from unitigs_t / unitig_links_t dicts, or from one merged dict (links None)"""
        return {k: (unitigs[k] if k in unitigs else links[k]) for k in cls.GRAPH_KEYS}

    def _graph_ptrs(self, g: dict):
        for k in self.GRAPH_KEYS:
            self._chk_dev(g[k])
        u, e = g["offsets"].numel() - 1, g["link_to"].numel()
        if u < 0 or g["link_off"].numel() != 2 * u + 1 or any(g[k].numel() != u for k in ("circular", "tf_sum", "tf_min", "tf_max")):
            raise ValueError("the arrays of a unitig set must hold U + 1 offsets, U values each and 2 U + 1 link offsets")
        return u, e, {k: vp(g[k].data_ptr()) for k in self.GRAPH_KEYS}

    def graph_mark_t(self, unitigs: dict, links: dict = None, tip_max_kmers: int = 46, bubble_max_kmers: int = 46):
        """Tips and weaker bubble arms of a unitig set in HBM: (remove uint8[U] — 0 keep, 1 tip, 2 arm —, n_tips, n_arms). links None:
        `unitigs` holds the link arrays too. A bubble_mate in either dict is used, else it is computed."""
        import torch
        g = self._graph_of(unitigs, links)
        u, e, q = self._graph_ptrs(g)
        mate = (links or {}).get("bubble_mate", unitigs.get("bubble_mate"))
        if mate is not None:
            self._chk_dev(mate)
        remove = torch.empty(u, dtype=torch.uint8, device=g["offsets"].device)
        tips, arms = C.c_uint64(), C.c_uint64()
        with torch.cuda.device(self.device):
            check(lib().aix_graph_mark_dev(u, q["offsets"], q["circular"], q["tf_sum"], q["link_off"], q["link_to"], e,
                                           vp(mate.data_ptr()) if mate is not None else None, tip_max_kmers, bubble_max_kmers, vp(remove.data_ptr()),
                                           C.byref(tips), C.byref(arms), _stream_ptr(self.device)), "aix_graph_mark_dev")
        return remove, tips.value, arms.value

    def graph_compact_t(self, unitigs: dict, links: dict, remove) -> dict:
        """The survivors of `remove` (uint8[U], non-zero = removed) compacted into contigs: a unitig set in the format of unitigs_t /
        unitig_links_t merged (offsets, bases, circular, tf_sum, tf_min, tf_max, link_off, link_to, bubble_mate, U, E, n_circular), plus the
        map unitig_contig int32[U] (-1 = removed), unitig_pos int64[U], unitig_flag uint8[U]. links None: `unitigs` is a merged dict."""
        import torch
        g = self._graph_of(unitigs, links)
        u, e, q = self._graph_ptrs(g)
        self._chk_dev(remove)
        if remove.numel() != u:
            raise ValueError("remove must hold U entries")
        dev = g["offsets"].device
        uc = torch.empty(u, dtype=torch.int32, device=dev)
        up = torch.empty(u, dtype=torch.int64, device=dev)
        uf = torch.empty(u, dtype=torch.uint8, device=dev)
        c, total, e2, circ = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        p = lambda t: vp(t.data_ptr())
        with torch.cuda.device(self.device):
            check(lib().aix_graph_compact_layout_dev(u, q["offsets"], q["bases"], q["circular"], q["link_off"], q["link_to"], e, p(remove), p(uc), p(up), p(uf),
                                                     C.byref(c), C.byref(total), C.byref(e2), C.byref(circ), _stream_ptr(self.device)),
                  "aix_graph_compact_layout_dev")
            n = c.value
            out = {"offsets": torch.empty(n + 1, dtype=torch.int64, device=dev), "bases": torch.empty(total.value, dtype=torch.uint8, device=dev),
                   "circular": torch.empty(n, dtype=torch.uint8, device=dev), "tf_sum": torch.empty(n, dtype=torch.int64, device=dev),
                   "tf_min": torch.empty(n, dtype=torch.int32, device=dev), "tf_max": torch.empty(n, dtype=torch.int32, device=dev),
                   "link_off": torch.empty(2 * n + 1, dtype=torch.int64, device=dev), "link_to": torch.empty(e2.value, dtype=torch.int32, device=dev)}
            check(lib().aix_graph_compact_emit_dev(u, *[q[k] for k in self.GRAPH_KEYS[:6]], q["link_off"], q["link_to"], e, p(remove), p(uc), p(up), p(uf), n,
                                                   total.value, e2.value, *[p(out[k]) for k in self.GRAPH_KEYS], _stream_ptr(self.device)),
                  "aix_graph_compact_emit_dev")
            mate = torch.empty(n, dtype=torch.int32, device=dev)
            check(lib().aix_unitig_bubbles_dev(n, p(out["link_off"]), p(out["link_to"]), e2.value, p(mate), _stream_ptr(self.device)), "aix_unitig_bubbles_dev")
        out.update(bubble_mate=mate, U=n, E=e2.value, n_circular=circ.value, unitig_contig=uc, unitig_pos=up, unitig_flag=uf)
        return out

    def graph_clean_t(self, unitigs: dict, links: dict = None, tip_max_kmers: int = 46, bubble_max_kmers: int = 46, rounds: int = 1):
        """Mark then compact, repeated until nothing is removed or `rounds` is reached: (graph, rounds done). The graph is a merged dict as
        graph_compact_t returns it; its map arrays are those of the last round (absent when no round removed anything)."""
        g = dict(self._graph_of(unitigs, links))
        g.update(U=g["offsets"].numel() - 1, E=g["link_to"].numel())
        mate = (links or {}).get("bubble_mate", unitigs.get("bubble_mate"))
        if mate is not None:
            g["bubble_mate"] = mate
        done = 0
        while done < rounds:
            remove, tips, arms = self.graph_mark_t(g, None, tip_max_kmers, bubble_max_kmers)
            if tips + arms == 0:
                break
            g = self.graph_compact_t(g, None, remove)
            done += 1
        return g, done

    def graph_clean_round(self, graph: dict, tip_max_kmers: int = 46, bubble_max_kmers: int = 46) -> dict:
        """One round through host memory (aix_graph_clean): numpy arrays in (the eight arrays of a unitig set), numpy arrays out — G', remove
        uint8[U], the map, and the ints U, E, n_tips, n_arms."""
        a = [np.ascontiguousarray(graph[k], dtype=dt) for k, dt in zip(self.GRAPH_KEYS, self.GRAPH_DTYPES)]
        u, e = a[0].shape[0] - 1, a[7].shape[0]
        if u < 0 or a[6].shape[0] != 2 * u + 1 or any(a[i].shape[0] != u for i in (2, 3, 4, 5)) or (u and a[1].shape[0] != int(a[0][u])):
            raise ValueError("the arrays of a unitig set must hold U + 1 offsets, offsets[U] bases, U values each and 2 U + 1 link offsets")
        ps = [vp() for _ in range(12)]
        n = [C.c_uint64() for _ in range(4)]
        with self._device_ctx():
            check(lib().aix_graph_clean(u, *[x.ctypes.data_as(vp) for x in a], e, tip_max_kmers, bubble_max_kmers, *[C.byref(x) for x in n],
                                        *[C.byref(x) for x in ps]), "aix_graph_clean")
        c, e2 = n[0].value, n[1].value
        off = self._take(ps[0], c + 1, np.uint64)
        sizes = (None, int(off[c]), c, c, c, c, 2 * c + 1, e2, u, u, u, u)
        names = self.GRAPH_KEYS + ("remove", "unitig_contig", "unitig_pos", "unitig_flag")
        types = self.GRAPH_DTYPES + (np.uint8, np.uint32, np.uint64, np.uint8)
        out = {"offsets": off}
        for i in range(1, 12):
            out[names[i]] = self._take(ps[i], sizes[i], types[i])
        out.update(U=c, E=e2, n_tips=n[2].value, n_arms=n[3].value)
        return out

    def graph_mark(self, unitigs: dict, links: dict = None, tip_max_kmers: int = 46, bubble_max_kmers: int = 46) -> np.ndarray:
        """graph_mark_t through host memory: numpy arrays in, remove uint8[U] out."""
        return self.graph_mark_t(self._graph_to_device(unitigs, links), None, tip_max_kmers, bubble_max_kmers)[0].cpu().numpy()

    def graph_compact(self, unitigs: dict, links: dict, remove) -> dict:
        """graph_compact_t through host memory: numpy arrays in and out (u64 / u32 as in Index.unitigs and Index.unitig_links)."""
        import torch
        r = torch.from_numpy(np.ascontiguousarray(remove, dtype=np.uint8)).to(f"cuda:{self.device}")
        return self._graph_to_host(self.graph_compact_t(self._graph_to_device(unitigs, links), None, r))

    def graph_clean(self, unitigs: dict, links: dict = None, tip_max_kmers: int = 46, bubble_max_kmers: int = 46, rounds: int = 1):
        """graph_clean_t through host memory: (graph of numpy arrays, rounds done); each round is one aix_graph_clean call."""
        g = {k: np.ascontiguousarray(self._graph_of(unitigs, links)[k], dtype=dt) for k, dt in zip(self.GRAPH_KEYS, self.GRAPH_DTYPES)}
        g.update(U=g["offsets"].shape[0] - 1, E=g["link_to"].shape[0])
        done = 0
        while done < rounds:
            nxt = self.graph_clean_round(g, tip_max_kmers, bubble_max_kmers)
            if nxt["n_tips"] + nxt["n_arms"] == 0:
                break
            g = nxt
            done += 1
        return g, done

    # ---- threading (aix_seqthread.hip) -------------------------------------------------------------
    THREAD_KEYS = ("seq_step_off", "step_unitig", "step_pos", "step_flag", "q_first", "q_last", "step_link")
    THREAD_DTYPES = (np.uint64, np.uint32, np.uint32, np.uint8, np.uint32, np.uint32, np.uint64)

    def graph_kidmap_t(self, kid_map, offsets_t, compacted: dict, out=None):
        """A k-mer map (kid_unitig int64[n], kid_pos int32[n], kid_flag uint8[n]) of a graph with `offsets_t` carried through one
        compaction round: `compacted` is what graph_compact_t returned for that graph. -> the three arrays on the contigs (new tensors,
        or `out`, which may be kid_map itself)."""
        import torch
        ku, kp, kf = kid_map
        uc, up, uf = compacted["unitig_contig"], compacted["unitig_pos"], compacted["unitig_flag"]
        for t in (ku, kp, kf, offsets_t, uc, up, uf):
            self._chk_dev(t)
        n, u = ku.numel(), offsets_t.numel() - 1
        if kp.numel() != n or kf.numel() != n or u < 0 or any(t.numel() != u for t in (uc, up, uf)):
            raise ValueError("a k-mer map holds n entries per array, the compaction map U")
        o = out if out is not None else (torch.empty_like(ku), torch.empty_like(kp), torch.empty_like(kf))
        p = lambda t: vp(t.data_ptr())
        with torch.cuda.device(self.device):
            check(lib().aix_graph_kidmap_dev(n, p(ku), p(kp), p(kf), u, p(offsets_t), p(uc), p(up), p(uf), p(o[0]), p(o[1]), p(o[2]),
                                             _stream_ptr(self.device)), "aix_graph_kidmap_dev")
        return o

    def thread_nodes_t(self, kid_map, offsets_t):
        """One word per kid from a k-mer map and the offsets of its graph: node int64[n] = unitig << 33 | pos << 2 | flag, -1 for a dead kid."""
        import torch
        ku, kp, kf = kid_map
        for t in (ku, kp, kf, offsets_t):
            self._chk_dev(t)
        n, u = ku.numel(), offsets_t.numel() - 1
        if kp.numel() != n or kf.numel() != n or u < 0:
            raise ValueError("a k-mer map holds n entries per array")
        node = torch.empty(n, dtype=torch.int64, device=ku.device)
        p = lambda t: vp(t.data_ptr())
        with torch.cuda.device(self.device):
            check(lib().aix_thread_nodes_dev(n, p(ku), p(kp), p(kf), u, p(offsets_t), p(node), _stream_ptr(self.device)), "aix_thread_nodes_dev")
        return node

    def thread_graph_t(self, cutoff: int = 0, tip_max_kmers: int = 0, bubble_max_kmers: int = 0, rounds: int = 0) -> dict:
        """The graph sequences are threaded through, built once: unitigs and links at `cutoff`, then up to `rounds` cleaning rounds (mark,
        compact, the k-mer map composed after every round). -> the eight arrays of the graph, the k-mer map (kid_unitig, kid_pos,
        kid_flag), node int64[n], and the ints U, E, rounds (done)."""
        un = self.unitigs_t(cutoff)
        g = dict(self._graph_of(un, self.unitig_links_t(cutoff, unitigs=un)))
        kid_map = (un["kid_unitig"], un["kid_pos"], un["kid_flag"])
        done = 0
        while done < rounds:
            remove, tips, arms = self.graph_mark_t(g, None, tip_max_kmers, bubble_max_kmers)
            if tips + arms == 0:
                break
            nxt = self.graph_compact_t(g, None, remove)
            kid_map = self.graph_kidmap_t(kid_map, g["offsets"], nxt)
            g = {k: nxt[k] for k in self.GRAPH_KEYS}
            done += 1
        g.update(kid_unitig=kid_map[0], kid_pos=kid_map[1], kid_flag=kid_map[2], node=self.thread_nodes_t(kid_map, g["offsets"]),
                 U=g["offsets"].numel() - 1, E=g["link_to"].numel(), rounds=done)
        return g

    def seq_thread_t(self, graph: dict, seqs_t, offs_t, link_support=None, cap_hint: int = 0):
        """The paths of M sequences (uint8 bytes, int64 offsets[M + 1]) through `graph` (what thread_graph_t returned), on torch's current
        stream: (seq_step_off int64[M + 1], step_unitig int32, step_pos int32, step_flag uint8, q_first int32, q_last int32, step_link
        int64) — bit patterns of the unsigned fields; step_link -1 = no link, -2 = broken. link_support: int64[E], one is added per
        traversed link and its dual (accumulated across calls)."""
        import torch
        u, e, q = self._graph_ptrs({k: graph[k] for k in self.GRAPH_KEYS})
        node = graph["node"]
        self._chk_dev(node)
        if node.numel() != self.n:
            raise ValueError("node must hold one word per stored k-mer")
        if link_support is not None:
            self._chk_dev(link_support)
            if link_support.numel() != e or link_support.dtype != torch.int64:
                raise ValueError("link_support must be int64[E]")
        sup = vp(link_support.data_ptr()) if link_support is not None else None
        st = _stream_ptr(self.device)
        return self._seq_t("aix_seq_thread_dev", seqs_t, offs_t, [torch.int32, torch.int32, torch.uint8, torch.int32, torch.int32, torch.int64], cap_hint,
                           lambda m, off, o, cap, tot: lib().aix_seq_thread_dev(self._h, vp(seqs_t.data_ptr()), vp(offs_t.data_ptr()), m, vp(node.data_ptr()), u,
                                                                                q["offsets"], q["circular"], q["link_off"], q["link_to"], e, sup, off, *o, cap, tot, st))

    def seq_thread(self, seqs: Sequence, cutoff: int = 0) -> dict:
        """seq_thread_t through host memory, on the unitig graph at `cutoff` (built inside): numpy arrays seq_step_off uint64[M + 1],
        step_unitig / step_pos / q_first / q_last uint32, step_flag uint8, step_link uint64, link_support uint64[E] (counted from zero),
        and the ints U, E."""
        data, offs = _ragged(seqs)
        m = len(seqs)
        ps = [vp() for _ in range(8)]
        u, e = C.c_uint64(), C.c_uint64()
        check(lib().aix_seq_thread(self._h, cutoff, _np_ptr(data) if data.shape[0] else None, _np_ptr(offs), m, *[C.byref(p) for p in ps], C.byref(u), C.byref(e)),
              "aix_seq_thread")
        out = {"seq_step_off": self._take(ps[0], m + 1, np.uint64)}
        t = int(out["seq_step_off"][m])
        for i in range(1, 7):
            out[self.THREAD_KEYS[i]] = self._take(ps[i], t, self.THREAD_DTYPES[i])
        out.update(link_support=self._take(ps[7], e.value, np.uint64), U=u.value, E=e.value)
        return out

    # ---- repeat resolution (aix_graphresolve.hip) -------------------------------------------------
    def thread_pairs_t(self, graph: dict, steps, pair_support=None):
        """The transitions of threaded sequences through every unitig: `steps` is what seq_thread_t returned for `graph` (only step_unitig,
        step_flag and step_link are read). pair_support int64[16 U]: cell 16 u + 4 x + y counts the sequences that pass unitig u between
        link x of end 2 u and link y of end 2 u + 1 (local indices); accumulated across calls, a zeroed one is made when None.
        -> (pair_support, n_pairs)."""
        import torch
        lo, to = graph["link_off"], graph["link_to"]
        su, sf, sl = steps[1], steps[3], steps[6]
        for t in (lo, to, su, sf, sl):
            self._chk_dev(t)
        u, e, n = (lo.numel() - 1) // 2, to.numel(), su.numel()
        if lo.numel() != 2 * u + 1 or sf.numel() != n or sl.numel() != n:
            raise ValueError("link_off must hold 2 U + 1 entries, the step arrays T each")
        if pair_support is None:
            pair_support = torch.zeros(16 * u, dtype=torch.int64, device=lo.device)
        self._chk_dev(pair_support)
        if pair_support.numel() != 16 * u or pair_support.dtype != torch.int64:
            raise ValueError("pair_support must be int64[16 U]")
        got = C.c_uint64()
        p = lambda t: vp(t.data_ptr())
        with torch.cuda.device(self.device):
            check(lib().aix_thread_pairs_dev(u, p(lo), p(to), e, n, p(su), p(sf), p(sl), p(pair_support), C.byref(got), _stream_ptr(self.device)),
                  "aix_thread_pairs_dev")
        return pair_support, got.value

    def _support_ptrs(self, u: int, e: int, link_support, pair_support):
        import torch
        for t, n, what in ((link_support, e, "link_support must be int64[E]"), (pair_support, 16 * u, "pair_support must be int64[16 U]")):
            if t is not None:
                self._chk_dev(t)
                if t.numel() != n or t.dtype != torch.int64:
                    raise ValueError(what)
        return [vp(t.data_ptr()) if t is not None else None for t in (link_support, pair_support)]

    def graph_resolve_mark_t(self, graph: dict, link_support=None, pair_support=None, min_link_support: int = 2, min_pair_support: int = 2,
                             max_pair_noise: int = 0):
        """Weak links and repeat splits of a unitig set in HBM, decided from link_support int64[E] and pair_support int64[16 U] (either may
        be None: its rule is off): (link_remove uint8[E], copies uint8[U], n_links_removed, n_split, n_copies_added)."""
        import torch
        u, e, q = self._graph_ptrs({k: graph[k] for k in self.GRAPH_KEYS})
        sup, pair = self._support_ptrs(u, e, link_support, pair_support)
        dev = graph["offsets"].device
        remove = torch.empty(e, dtype=torch.uint8, device=dev)
        copies = torch.empty(u, dtype=torch.uint8, device=dev)
        n = [C.c_uint64() for _ in range(3)]
        with torch.cuda.device(self.device):
            check(lib().aix_graph_resolve_mark_dev(u, q["offsets"], q["circular"], q["link_off"], q["link_to"], e, sup, pair, min_link_support, min_pair_support,
                                                   max_pair_noise, vp(remove.data_ptr()), vp(copies.data_ptr()), *[C.byref(x) for x in n],
                                                   _stream_ptr(self.device)), "aix_graph_resolve_mark_dev")
        return remove, copies, n[0].value, n[1].value, n[2].value

    def graph_resolve_t(self, graph: dict, link_support=None, pair_support=None, min_link_support: int = 2, min_pair_support: int = 2,
                        max_pair_noise: int = 0, compact: bool = True) -> dict:
        """Mark, layout and emit of the repeat resolution: the resolved unitig set G_r as a merged dict in the format of graph_compact_t
        (the eight arrays, U, E) plus link_remove uint8[E], copies uint8[U], copy_base int32[U] (-1 = unsplit), unitig_origin int32[U']
        and the ints n_links_removed, n_split, n_copies_added. compact: G_r is then compacted under an all-zero mask (graph_compact_t) and
        that merged dict is returned, with "resolved" = the dict described above; unitig_origin still refers to G_r's ids."""
        import torch
        g = {k: graph[k] for k in self.GRAPH_KEYS}
        u, e, q = self._graph_ptrs(g)
        remove, copies, removed, n_split, added = self.graph_resolve_mark_t(graph, link_support, pair_support, min_link_support, min_pair_support, max_pair_noise)
        _, pair = self._support_ptrs(u, e, None, pair_support)
        dev = g["offsets"].device
        base = torch.empty(u, dtype=torch.int32, device=dev)
        u2, total, e2 = C.c_uint64(), C.c_uint64(), C.c_uint64()
        p = lambda t: vp(t.data_ptr())
        with torch.cuda.device(self.device):
            check(lib().aix_graph_resolve_layout_dev(u, q["offsets"], e, p(remove), p(copies), p(base), C.byref(u2), C.byref(total), C.byref(e2),
                                                     _stream_ptr(self.device)), "aix_graph_resolve_layout_dev")
            n = u2.value
            out = {"offsets": torch.empty(n + 1, dtype=torch.int64, device=dev), "bases": torch.empty(total.value, dtype=torch.uint8, device=dev),
                   "circular": torch.empty(n, dtype=torch.uint8, device=dev), "tf_sum": torch.empty(n, dtype=torch.int64, device=dev),
                   "tf_min": torch.empty(n, dtype=torch.int32, device=dev), "tf_max": torch.empty(n, dtype=torch.int32, device=dev),
                   "link_off": torch.empty(2 * n + 1, dtype=torch.int64, device=dev), "link_to": torch.empty(e2.value, dtype=torch.int32, device=dev)}
            origin = torch.empty(n, dtype=torch.int32, device=dev)
            check(lib().aix_graph_resolve_emit_dev(u, *[q[k] for k in self.GRAPH_KEYS], e, p(remove), p(copies), p(base), pair, min_pair_support, n, total.value,
                                                   e2.value, *[p(out[k]) for k in self.GRAPH_KEYS], p(origin), _stream_ptr(self.device)),
                  "aix_graph_resolve_emit_dev")
        out.update(U=n, E=e2.value, link_remove=remove, copies=copies, copy_base=base, unitig_origin=origin, n_links_removed=removed, n_split=n_split,
                   n_copies_added=added)
        if not compact:
            return out
        merged = self.graph_compact_t(out, None, torch.zeros(n, dtype=torch.uint8, device=dev))
        merged.update(resolved=out, unitig_origin=origin)
        return merged

    def graph_resolve(self, graph: dict, link_support=None, pair_support=None, min_link_support: int = 2, min_pair_support: int = 2,
                      max_pair_noise: int = 0) -> dict:
        """The resolution through host memory (aix_graph_resolve): numpy arrays in (the eight arrays of a unitig set, link_support uint64[E]
        and pair_support uint64[16 U], either may be None), numpy arrays out — G_r, link_remove uint8[E], copies uint8[U], unitig_origin
        uint32[U'] and the ints U, E, n_links_removed, n_split."""
        a = [np.ascontiguousarray(graph[k], dtype=dt) for k, dt in zip(self.GRAPH_KEYS, self.GRAPH_DTYPES)]
        u, e = a[0].shape[0] - 1, a[7].shape[0]
        if u < 0 or a[6].shape[0] != 2 * u + 1 or any(a[i].shape[0] != u for i in (2, 3, 4, 5)) or (u and a[1].shape[0] != int(a[0][u])):
            raise ValueError("the arrays of a unitig set must hold U + 1 offsets, offsets[U] bases, U values each and 2 U + 1 link offsets")
        sup = None if link_support is None else np.ascontiguousarray(link_support, dtype=np.uint64)
        pair = None if pair_support is None else np.ascontiguousarray(pair_support, dtype=np.uint64)
        if (sup is not None and sup.shape[0] != e) or (pair is not None and pair.shape[0] != 16 * u):
            raise ValueError("link_support must hold E entries, pair_support 16 U")
        ps = [vp() for _ in range(11)]
        n = [C.c_uint64() for _ in range(4)]
        with self._device_ctx():
            check(lib().aix_graph_resolve(u, *[x.ctypes.data_as(vp) for x in a], e, _np_ptr(sup), _np_ptr(pair), min_link_support, min_pair_support, max_pair_noise,
                                          *[C.byref(x) for x in n], *[C.byref(x) for x in ps]), "aix_graph_resolve")
        u2, e2 = n[0].value, n[1].value
        off = self._take(ps[0], u2 + 1, np.uint64)
        sizes = (None, int(off[u2]), u2, u2, u2, u2, 2 * u2 + 1, e2, e, u, u2)
        names = self.GRAPH_KEYS + ("link_remove", "copies", "unitig_origin")
        types = self.GRAPH_DTYPES + (np.uint8, np.uint8, np.uint32)
        out = {"offsets": off}
        for i in range(1, 11):
            out[names[i]] = self._take(ps[i], sizes[i], types[i])
        out.update(U=u2, E=e2, n_links_removed=n[2].value, n_split=n[3].value)
        return out

    # ---- scaffolding (aix_scaffold.hip) -------------------------------------------------------------
    SLINK_KEYS = ("slink_off", "slink_to", "slink_count", "slink_dsum")

    def mate_links_t(self, graph: dict, steps, offs_t, min_anchor_windows: int = 1, max_insert: int = 1000, insert_hist=None):
        """One observation per pair of a threaded batch: `steps` is what seq_thread_t returned for `graph` and the sequences of `offs_t`
        (int64[2 P + 1]; sequence 2 i the left mate, 2 i + 1 the right mate, both in fragment orientation). insert_hist int64[max_insert + 1]
        is accumulated across calls, a zeroed one is made when None. -> (obs_key int64[P], obs_d int32[P], counts int64[4] = same contig,
        link, discordant, unanchored, insert_hist) — bit patterns of the unsigned fields; obs_key -1 = no observation."""
        import torch
        off, circ = graph["offsets"], graph["circular"]
        sso, su, sp, sf, qf, ql = steps[:6]
        for t in (off, circ, offs_t, sso, su, sp, sf, qf, ql):
            self._chk_dev(t)
        m, n, u = offs_t.numel() - 1, su.numel(), off.numel() - 1
        if m < 0 or m % 2 or sso.numel() != m + 1 or any(t.numel() != n for t in (sp, sf, qf, ql)) or circ.numel() != u:
            raise ValueError("a batch of pairs holds 2 P + 1 offsets and step offsets, the step arrays T entries each")
        dev = off.device
        if insert_hist is None:
            insert_hist = torch.zeros(max_insert + 1, dtype=torch.int64, device=dev)
        self._chk_dev(insert_hist)
        if insert_hist.numel() != max_insert + 1 or insert_hist.dtype != torch.int64:
            raise ValueError("insert_hist must be int64[max_insert + 1]")
        pairs = m // 2
        key = torch.empty(pairs, dtype=torch.int64, device=dev)
        d = torch.empty(pairs, dtype=torch.int32, device=dev)
        counts = torch.empty(4, dtype=torch.int64, device=dev)
        p = lambda t: vp(t.data_ptr())
        with torch.cuda.device(self.device):
            check(lib().aix_mate_links_dev(pairs, p(offs_t), p(sso), n, p(su), p(sp), p(sf), p(qf), p(ql), u, p(off), p(circ), min_anchor_windows, max_insert,
                                           p(insert_hist), p(key), p(d), p(counts), _stream_ptr(self.device)), "aix_mate_links_dev")
        return key, d, counts, insert_hist

    def mate_bundle_t(self, obs_key, obs_d, n_contigs: int, cap_hint: int = 0) -> dict:
        """The observations of any number of batches (concatenated by the caller) as the scaffold graph over the 2 U contig ends:
        slink_off int64[2 U + 1], slink_to int32[S], slink_count int64[S], slink_dsum int64[S] and the int S. cap_hint: the entries to
        make room for at once; below S the call runs twice, a sizing pass and the fill. 2 N is always enough."""
        import torch
        self._chk_dev(obs_key)
        self._chk_dev(obs_d)
        n = obs_key.numel()
        if obs_d.numel() != n or obs_key.dtype != torch.int64 or obs_d.dtype != torch.int32:
            raise ValueError("obs_key must be int64[N], obs_d int32[N]")
        dev = obs_key.device
        off = torch.empty(2 * n_contigs + 1, dtype=torch.int64, device=dev)
        total = C.c_uint64()
        p = lambda t: vp(t.data_ptr())
        with torch.cuda.device(self.device):
            cap = max(int(cap_hint), 0)
            while True:
                outs = [torch.empty(max(cap, 1), dtype=dt, device=dev) for dt in (torch.int32, torch.int64, torch.int64)]
                check(lib().aix_mate_bundle_dev(n, p(obs_key), p(obs_d), n_contigs, p(off), *[p(o) if cap else None for o in outs], cap, C.byref(total),
                                                _stream_ptr(self.device)), "aix_mate_bundle_dev")
                if total.value <= cap:
                    break
                cap = total.value
        s = total.value
        return {"slink_off": off, "slink_to": outs[0][:s], "slink_count": outs[1][:s], "slink_dsum": outs[2][:s], "S": s}

    def scaffold_mark_t(self, graph: dict, slinks: dict, insert_size: int, min_pairs: int = 2, dominance: int = 2, min_contig_bases: int = 0) -> dict:
        """Which contig ends are joined: join int32[2 U] (-1 = none), join_count int64[2 U], join_gap int64[2 U] and the int n_joins."""
        import torch
        off, circ = graph["offsets"], graph["circular"]
        sl = [slinks[k] for k in self.SLINK_KEYS]
        for t in [off, circ] + sl:
            self._chk_dev(t)
        u, s = off.numel() - 1, sl[1].numel()
        if u < 0 or circ.numel() != u or sl[0].numel() != 2 * u + 1 or sl[2].numel() != s or sl[3].numel() != s:
            raise ValueError("a scaffold graph holds 2 U + 1 link offsets and S entries per link array")
        dev = off.device
        join = torch.empty(2 * u, dtype=torch.int32, device=dev)
        count = torch.empty(2 * u, dtype=torch.int64, device=dev)
        gap = torch.empty(2 * u, dtype=torch.int64, device=dev)
        n = C.c_uint64()
        p = lambda t: vp(t.data_ptr())
        with torch.cuda.device(self.device):
            check(lib().aix_scaffold_mark_dev(u, p(off), p(circ), *[p(t) for t in sl], s, insert_size, min_pairs, dominance, min_contig_bases, p(join), p(count), p(gap),
                                              C.byref(n), _stream_ptr(self.device)), "aix_scaffold_mark_dev")
        return {"join": join, "join_count": count, "join_gap": gap, "n_joins": n.value}

    def scaffold_t(self, graph: dict, joins: dict, min_gap: int = 1) -> dict:
        """Layout and emit of the scaffolds of `graph` (offsets, bases) under `joins` (what scaffold_mark_t returned): contig_scaffold and
        contig_rank int32[U], contig_pos int64[U], contig_flag uint8[U], scaffold_offsets int64[Sc + 1], scaffold_bases uint8, member_off
        int64[Sc + 1], member int32[U] (2 u + flag), member_gap int64[U] and the ints n_scaffolds, total_bases, n_cut."""
        import torch
        off, bases = graph["offsets"], graph["bases"]
        jn, jc, jg = joins["join"], joins["join_count"], joins["join_gap"]
        for t in (off, bases, jn, jc, jg):
            self._chk_dev(t)
        u = off.numel() - 1
        if u < 0 or any(t.numel() != 2 * u for t in (jn, jc, jg)):
            raise ValueError("join, join_count and join_gap hold 2 U entries")
        dev = off.device
        cs, cr = torch.empty(u, dtype=torch.int32, device=dev), torch.empty(u, dtype=torch.int32, device=dev)
        cp, cf = torch.empty(u, dtype=torch.int64, device=dev), torch.empty(u, dtype=torch.uint8, device=dev)
        n = [C.c_uint64() for _ in range(3)]
        p = lambda t: vp(t.data_ptr())
        with torch.cuda.device(self.device):
            check(lib().aix_scaffold_layout_dev(u, p(off), p(jn), p(jc), p(jg), min_gap, p(cs), p(cr), p(cp), p(cf), *[C.byref(x) for x in n],
                                                _stream_ptr(self.device)), "aix_scaffold_layout_dev")
            sc, total = n[0].value, n[1].value
            so, mo = torch.empty(sc + 1, dtype=torch.int64, device=dev), torch.empty(sc + 1, dtype=torch.int64, device=dev)
            sb = torch.empty(total, dtype=torch.uint8, device=dev)
            mm, mg = torch.empty(u, dtype=torch.int32, device=dev), torch.empty(u, dtype=torch.int64, device=dev)
            check(lib().aix_scaffold_emit_dev(u, p(off), p(bases), p(jn), p(jg), min_gap, p(cs), p(cr), p(cp), p(cf), sc, total, p(so), p(sb), p(mo), p(mm), p(mg),
                                              _stream_ptr(self.device)), "aix_scaffold_emit_dev")
        return {"contig_scaffold": cs, "contig_rank": cr, "contig_pos": cp, "contig_flag": cf, "scaffold_offsets": so, "scaffold_bases": sb, "member_off": mo,
                "member": mm, "member_gap": mg, "n_scaffolds": sc, "total_bases": total, "n_cut": n[2].value}

    @staticmethod
    def insert_size_t(hist) -> int:
        """The lower median of an insert histogram (what mate_links_t accumulated). ValueError when it is empty: the caller then passes
        insert_size itself."""
        import torch
        acc = torch.cumsum(hist, 0)
        n = int(acc[-1]) if acc.numel() else 0
        if n == 0:
            raise ValueError("the insert histogram is empty")
        return int(torch.searchsorted(acc, torch.tensor([(n + 1) // 2], dtype=acc.dtype, device=acc.device))[0])

    def scaffold(self, offsets, bases, circular, obs_key, obs_d, insert_size: int, min_pairs: int = 2, dominance: int = 2, min_contig_bases: int = 0,
                 min_gap: int = 1) -> dict:
        """Bundle, mark, layout and emit through host memory (aix_scaffold): numpy arrays in (the contigs and N observations), numpy arrays
        out — the five scaffold arrays, join / join_count / join_gap [2 U], the map, and the ints n_scaffolds, n_joins, n_cut, S."""
        a = [np.ascontiguousarray(x, dtype=dt) for x, dt in zip((offsets, bases, circular, obs_key, obs_d), (np.uint64, np.uint8, np.uint8, np.uint64, np.uint32))]
        u, nobs = a[0].shape[0] - 1, a[3].shape[0]
        if u < 0 or a[2].shape[0] != u or a[4].shape[0] != nobs or (u and a[1].shape[0] != int(a[0][u])):
            raise ValueError("contigs hold U + 1 offsets, offsets[U] bases and U flags; observations N keys and N distances")
        ps = [vp() for _ in range(12)]
        n = [C.c_uint64() for _ in range(4)]
        with self._device_ctx():
            check(lib().aix_scaffold(u, _np_ptr(a[0]), _np_ptr(a[1]) if u else None, _np_ptr(a[2]) if u else None, nobs, _np_ptr(a[3]) if nobs else None,
                                     _np_ptr(a[4]) if nobs else None, insert_size, min_pairs, dominance, min_contig_bases, min_gap, *[C.byref(x) for x in n],
                                     *[C.byref(x) for x in ps]), "aix_scaffold")
        sc = n[0].value
        so = self._take(ps[0], sc + 1, np.uint64)
        names = ("scaffold_offsets", "scaffold_bases", "member_off", "member", "member_gap", "join", "join_count", "join_gap", "contig_scaffold", "contig_rank",
                 "contig_pos", "contig_flag")
        sizes = (None, int(so[sc]), sc + 1, u, u, 2 * u, 2 * u, 2 * u, u, u, u, u)
        types = (np.uint64, np.uint8, np.uint64, np.uint32, np.int64, np.uint32, np.uint64, np.int64, np.uint32, np.uint32, np.uint64, np.uint8)
        out = {"scaffold_offsets": so}
        for i in range(1, 12):
            out[names[i]] = self._take(ps[i], sizes[i], types[i])
        out.update(n_scaffolds=sc, n_joins=n[1].value, n_cut=n[2].value, S=n[3].value, total_bases=int(so[sc]))
        return out

    # ---- gap closing (aix_gapclose.hip) --------------------------------------------------------------
    CLOSE_STATUS = ("none", "closed", "no_path", "ambiguous", "exhausted")

    def _gap_graph(self, graph: dict, joins: dict):
        off, lo, lt, jn, jg = graph["offsets"], graph["link_off"], graph["link_to"], joins["join"], joins["join_gap"]
        for t in (off, lo, lt, jn, jg):
            self._chk_dev(t)
        u = off.numel() - 1
        if u < 0 or lo.numel() != 2 * u + 1 or jn.numel() != 2 * u or jg.numel() != 2 * u:
            raise ValueError("a graph holds U + 1 offsets and 2 U + 1 link offsets, the joins 2 U entries per array")
        return off, lo, lt, jn, jg, u

    def gap_close_t(self, graph: dict, joins: dict, tolerance: int = 50, max_fill: int = 16, max_states: int = 1024, cap_hint: int = 0) -> dict:
        """One bounded path search per join of `joins` (what scaffold_mark_t returned) through `graph` (offsets, link_off, link_to):
        close_status uint8[2 U] (see CLOSE_STATUS), close_dist int64[2 U], close_states int32[2 U], path_off int64[2 U + 1], path
        int32[total] (the intermediates of every closed join, at its owner end), fill_uses int32[U], counts (ints: joins of status 1 .. 4
        and the joins) and the int total. cap_hint: the path entries to make room for at once; below the total the call runs twice."""
        import torch
        off, lo, lt, jn, jg, u = self._gap_graph(graph, joins)
        dev = off.device
        st = torch.empty(2 * u, dtype=torch.uint8, device=dev)
        dist = torch.empty(2 * u, dtype=torch.int64, device=dev)
        ns = torch.empty(2 * u, dtype=torch.int32, device=dev)
        po = torch.empty(2 * u + 1, dtype=torch.int64, device=dev)
        uses = torch.empty(u, dtype=torch.int32, device=dev)
        counts = torch.empty(5, dtype=torch.int64, device=dev)
        total = C.c_uint64()
        p = lambda t: vp(t.data_ptr())
        with torch.cuda.device(self.device):
            cap = max(int(cap_hint), 0)
            while True:
                path = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
                check(lib().aix_gap_close_dev(u, p(off), p(lo), p(lt), lt.numel(), p(jn), p(jg), tolerance, max_fill, max_states, p(st), p(dist), p(ns), p(po),
                                              p(path) if cap else None, cap, C.byref(total), p(uses), p(counts), _stream_ptr(self.device)), "aix_gap_close_dev")
                if total.value <= cap:
                    break
                cap = total.value
        return {"close_status": st, "close_dist": dist, "close_states": ns, "path_off": po, "path": path[:total.value], "fill_uses": uses,
                "counts": [int(x) for x in counts.tolist()], "total": total.value}

    def scaffold_fill_t(self, graph: dict, joins: dict, scaffolds: dict, closure: dict, min_gap: int = 1) -> dict:
        """The filled scaffolds of `scaffolds` (what scaffold_t returned for `graph` and `joins`) under `closure` (what gap_close_t
        returned): fmember_off int64[Sc + 1], fmember int32[Mf], fmember_flag uint8[Mf] (bit 0: overlaps its predecessor by 22 bases, bit 1:
        a fill contig), fmember_gap and fmember_pos int64[Mf], fscaffold_offsets int64[Sc + 1], fscaffold_bases uint8 and the ints
        n_fmembers, total_bases."""
        import torch
        off, lo, lt, jn, jg, u = self._gap_graph(graph, joins)
        bases, mo, mm = graph["bases"], scaffolds["member_off"], scaffolds["member"]
        cs, cd, po, pa = closure["close_status"], closure["close_dist"], closure["path_off"], closure["path"]
        for t in (bases, mo, mm, cs, cd, po, pa):
            self._chk_dev(t)
        sc, pt = mo.numel() - 1, pa.numel()
        if sc < 0 or mm.numel() != u or cs.numel() != 2 * u or cd.numel() != 2 * u or po.numel() != 2 * u + 1:
            raise ValueError("the member CSR holds Sc + 1 offsets and U members, the closure 2 U entries per array and 2 U + 1 path offsets")
        dev = off.device
        fo, so = torch.empty(sc + 1, dtype=torch.int64, device=dev), torch.empty(sc + 1, dtype=torch.int64, device=dev)
        fm = torch.empty(u + pt, dtype=torch.int32, device=dev)
        ff = torch.empty(u + pt, dtype=torch.uint8, device=dev)
        fg, fp = torch.empty(u + pt, dtype=torch.int64, device=dev), torch.empty(u + pt, dtype=torch.int64, device=dev)
        n = [C.c_uint64(), C.c_uint64()]
        p = lambda t: vp(t.data_ptr())
        with torch.cuda.device(self.device):
            check(lib().aix_scaffold_fill_layout_dev(u, p(off), p(lo), p(lt), lt.numel(), p(jn), p(jg), min_gap, sc, p(mo), p(mm), p(cs), p(cd), p(po),
                                                     p(pa) if pt else None, pt, p(fo), p(fm), p(ff), p(fg), p(fp), p(so), C.byref(n[0]), C.byref(n[1]),
                                                     _stream_ptr(self.device)), "aix_scaffold_fill_layout_dev")
            mf, total = n[0].value, n[1].value
            sb = torch.empty(total, dtype=torch.uint8, device=dev)
            check(lib().aix_scaffold_fill_emit_dev(u, p(off), p(bases), min_gap, sc, p(fo), mf, p(fm), p(ff), p(fg), p(fp), p(so), total, p(sb),
                                                   _stream_ptr(self.device)), "aix_scaffold_fill_emit_dev")
        return {"fmember_off": fo, "fmember": fm[:mf], "fmember_flag": ff[:mf], "fmember_gap": fg[:mf], "fmember_pos": fp[:mf], "fscaffold_offsets": so,
                "fscaffold_bases": sb, "n_fmembers": mf, "total_bases": total}

    def scaffold_fill(self, offsets, bases, link_off, link_to, join, join_gap, member_off, member, tolerance: int = 50, max_fill: int = 16,
                      max_states: int = 1024, min_gap: int = 1) -> dict:
        """Search, layout and emit through host memory (aix_scaffold_fill): numpy arrays in (the contigs, their links, the joins and the
        member CSR), numpy arrays out — the closure of gap_close_t and the filled arrays of scaffold_fill_t, with the ints n_fmembers,
        total_bases, total (path entries) and counts (a list)."""
        types = (np.uint64, np.uint8, np.uint64, np.uint32, np.uint32, np.int64, np.uint64, np.uint32)
        a = [np.ascontiguousarray(x, dtype=dt) for x, dt in zip((offsets, bases, link_off, link_to, join, join_gap, member_off, member), types)]
        u, e, sc = a[0].shape[0] - 1, a[3].shape[0], a[6].shape[0] - 1
        if u < 0 or sc < 0 or a[2].shape[0] != 2 * u + 1 or a[4].shape[0] != 2 * u or a[5].shape[0] != 2 * u or a[7].shape[0] != u or (u and a[1].shape[0] != int(a[0][u])):
            raise ValueError("contigs hold U + 1 offsets and offsets[U] bases, the links 2 U + 1 offsets, the joins 2 U entries, the members Sc + 1 offsets and U words")
        ps = [vp() for _ in range(14)]
        n = [C.c_uint64() for _ in range(3)]
        ptr = lambda x: _np_ptr(x) if x.shape[0] else None
        with self._device_ctx():
            check(lib().aix_scaffold_fill(u, _np_ptr(a[0]), ptr(a[1]), _np_ptr(a[2]), ptr(a[3]), e, ptr(a[4]), ptr(a[5]), sc, _np_ptr(a[6]), ptr(a[7]), tolerance,
                                          max_fill, max_states, min_gap, *[C.byref(x) for x in n], *[C.byref(x) for x in ps]), "aix_scaffold_fill")
        mf, total, pt = (x.value for x in n)
        names = ("fscaffold_offsets", "fscaffold_bases", "fmember_off", "fmember", "fmember_flag", "fmember_gap", "fmember_pos", "close_status", "close_dist",
                 "close_states", "path_off", "path", "fill_uses", "counts")
        sizes = (sc + 1, total, sc + 1, mf, mf, mf, mf, 2 * u, 2 * u, 2 * u, 2 * u + 1, pt, u, 5)
        types = (np.uint64, np.uint8, np.uint64, np.uint32, np.uint8, np.int64, np.uint64, np.uint8, np.int64, np.uint32, np.uint64, np.uint32, np.uint32, np.uint64)
        out = {k: self._take(q, s, t) for k, q, s, t in zip(names, ps, sizes, types)}
        out.update(n_fmembers=mf, total_bases=total, total=pt, counts=[int(x) for x in out["counts"]])
        return out

    # ---- pile-up (aix_pileup.hip) ----------------------------------------------------------------------
    PLACE_KEYS = ("seq_place_off", "place_unitig", "place_flag", "place_pos", "place_q0", "place_len", "place_steps")
    PLACE_DTYPES = (np.uint64, np.uint32, np.uint8, np.uint32, np.uint32, np.uint32, np.uint32)
    VAR_KEYS = ("var_unitig", "var_pos", "var_ref", "var_alt", "var_ref_count", "var_alt_count", "var_depth")
    VAR_DTYPES = (np.uint32, np.uint32, np.uint8, np.uint8, np.uint32, np.uint32, np.uint32)

    def pile_place_t(self, graph: dict, offs_t, steps, max_gap: int = 46, extend: int = 22) -> dict:
        """The steps of M threaded sequences merged into placements, on torch's current stream: `steps` is what seq_thread_t returned for
        `graph` and the offsets int64[M + 1] of the same batch. -> seq_place_off int64[M + 1], place_unitig int32, place_flag uint8 (bit 0:
        the read lies backwards), place_pos int32 (the leftmost contig base, local), place_q0 int32 (the first read base), place_len int32,
        place_steps int32 — bit patterns of the unsigned fields — and the ints n_place, n_circular_steps."""
        import torch
        off = graph["offsets"]
        sso, su, sp, sf, qf, ql = steps[:6]
        for t in (off, offs_t, sso, su, sp, sf, qf, ql):
            self._chk_dev(t)
        m, n, u = offs_t.numel() - 1, su.numel(), off.numel() - 1
        if m < 0 or u < 0 or sso.numel() != m + 1 or any(t.numel() != n for t in (sp, sf, qf, ql)):
            raise ValueError("the step arrays hold T entries each, seq_step_off M + 1")
        dev = off.device
        spo = torch.empty(m + 1, dtype=torch.int64, device=dev)
        types = (torch.int32, torch.uint8, torch.int32, torch.int32, torch.int32, torch.int32)
        outs = [torch.empty(n, dtype=ty, device=dev) for ty in types]
        got, circ = C.c_uint64(), C.c_uint64()
        p = lambda t: vp(t.data_ptr()) if t.numel() else None
        with torch.cuda.device(self.device):
            check(lib().aix_pile_place_dev(m, p(offs_t), p(sso), n, p(su), p(sp), p(sf), p(qf), p(ql), u, vp(off.data_ptr()), max_gap, extend, vp(spo.data_ptr()),
                                           *[p(o) for o in outs], C.byref(got), C.byref(circ), _stream_ptr(self.device)), "aix_pile_place_dev")
        out = dict(zip(self.PLACE_KEYS, [spo] + [o[:got.value] for o in outs]))
        out.update(n_place=got.value, n_circular_steps=circ.value)
        return out

    def pileup_t(self, graph: dict, seqs_t, offs_t, places: dict, counts=None) -> dict:
        """The read bases of `places` (what pile_place_t returned for this batch) counted at the contig bases of `graph`, on torch's
        current stream. counts: int32[4 B] (or [B, 4], contiguous), cell 4 g + c = the reads showing base c (A, C, G, T) at global base g;
        accumulated across calls, a zeroed one is made when None. -> counts, place_mism int32[R] (the counted bases of a placement that
        differ from the contig) and stats (ints: bases counted, other bytes, mismatches of this call)."""
        import torch
        off, bases = graph["offsets"], graph["bases"]
        arrs = [places[k] for k in self.PLACE_KEYS[:6]]
        for t in (off, bases, seqs_t, offs_t, *arrs):
            self._chk_dev(t)
        m, r, u, b = offs_t.numel() - 1, arrs[1].numel(), off.numel() - 1, bases.numel()
        if m < 0 or u < 0 or arrs[0].numel() != m + 1 or any(t.numel() != r for t in arrs[2:]):
            raise ValueError("the placement arrays hold R entries each, seq_place_off M + 1")
        dev = off.device
        if counts is None:
            counts = torch.zeros(4 * b, dtype=torch.int32, device=dev)
        self._chk_dev(counts)
        if counts.numel() != 4 * b or counts.dtype != torch.int32 or not counts.is_contiguous():
            raise ValueError("counts must be contiguous int32 with four cells per contig base")
        mism = torch.empty(r, dtype=torch.int32, device=dev)
        stats = torch.empty(3, dtype=torch.int64, device=dev)
        p = lambda t: vp(t.data_ptr()) if t.numel() else None
        with torch.cuda.device(self.device):
            check(lib().aix_pileup_dev(p(seqs_t), p(offs_t), m, p(arrs[0]), r, *[p(t) for t in arrs[1:]], u, vp(off.data_ptr()), p(bases), p(counts), p(mism),
                                       vp(stats.data_ptr()), _stream_ptr(self.device)), "aix_pileup_dev")
        return {"counts": counts, "place_mism": mism, "stats": [int(x) for x in stats.tolist()]}

    def pile_call_t(self, graph: dict, counts, min_depth: int = 8, min_major_permille: int = 700, min_alt_count: int = 3, min_alt_permille: int = 200,
                    cap_hint: int = 0) -> dict:
        """The counts of pileup_t read out, on torch's current stream: polished uint8[B] (the contig bases, replaced where a clear majority
        of at least min_depth reads disagrees) and the int n_changed; the variant sites in ascending order — var_unitig, var_pos int32,
        var_ref, var_alt uint8 (ASCII), var_ref_count, var_alt_count, var_depth int32 — and the int total; depth_sum int64[U] and uncovered
        int32[U]. cap_hint: the variants to make room for at once; below the total the call runs twice."""
        import torch
        off, bases = graph["offsets"], graph["bases"]
        for t in (off, bases, counts):
            self._chk_dev(t)
        u, b = off.numel() - 1, bases.numel()
        if u < 0 or counts.numel() != 4 * b or counts.dtype != torch.int32 or not counts.is_contiguous():
            raise ValueError("counts must be contiguous int32 with four cells per contig base")
        dev = off.device
        polished = torch.empty(b, dtype=torch.uint8, device=dev)
        dsum = torch.empty(u, dtype=torch.int64, device=dev)
        unc = torch.empty(u, dtype=torch.int32, device=dev)
        changed, total = C.c_uint64(), C.c_uint64()
        types = (torch.int32, torch.int32, torch.uint8, torch.uint8, torch.int32, torch.int32, torch.int32)
        p = lambda t: vp(t.data_ptr()) if t.numel() else None
        with torch.cuda.device(self.device):
            cap = max(int(cap_hint), 0)
            while True:
                outs = [torch.empty(max(cap, 1), dtype=ty, device=dev) for ty in types]
                check(lib().aix_pile_call_dev(u, vp(off.data_ptr()), p(bases), p(counts), min_depth, min_major_permille, min_alt_count, min_alt_permille, p(polished),
                                              C.byref(changed), *[vp(o.data_ptr()) if cap else None for o in outs], cap, C.byref(total), p(dsum), p(unc),
                                              _stream_ptr(self.device)), "aix_pile_call_dev")
                if total.value <= cap:
                    break
                cap = total.value
        out = dict(zip(self.VAR_KEYS, [o[:total.value] for o in outs]))
        out.update(polished=polished, n_changed=changed.value, total=total.value, depth_sum=dsum, uncovered=unc)
        return out

    def pileup(self, seqs: Sequence, cutoff: int = 0, max_gap: int = 46, extend: int = 22) -> dict:
        """pile_place_t and pileup_t through host memory, on the unitig graph at `cutoff` (built inside, the sequences threaded through
        it): numpy arrays offsets uint64[U + 1], bases uint8[B], counts uint32[4 B] (counted from zero), the seven placement arrays,
        place_mism uint32[R], stats uint64[3], and the ints U, n_place, n_circular_steps."""
        data, offs = _ragged(seqs)
        m = len(seqs)
        ps = [vp() for _ in range(12)]
        n = [C.c_uint64() for _ in range(3)]
        check(lib().aix_pileup(self._h, cutoff, _np_ptr(data) if data.shape[0] else None, _np_ptr(offs), m, max_gap, extend, *[C.byref(x) for x in n],
                               *[C.byref(p) for p in ps]), "aix_pileup")
        u, r, circ = (x.value for x in n)
        out = {"offsets": self._take(ps[0], u + 1, np.uint64)}
        b = int(out["offsets"][u])
        out.update(bases=self._take(ps[1], b, np.uint8), counts=self._take(ps[2], 4 * b, np.uint32), seq_place_off=self._take(ps[3], m + 1, np.uint64))
        for i in range(1, 7):
            out[self.PLACE_KEYS[i]] = self._take(ps[3 + i], r, self.PLACE_DTYPES[i])
        out.update(place_mism=self._take(ps[10], r, np.uint32), stats=self._take(ps[11], 3, np.uint64), U=u, n_place=r, n_circular_steps=circ)
        return out

    def _device_ctx(self):
        """the handle-less calls run on the current device: make it this index's when torch is in the process (it owns the current device then)"""
        import contextlib
        import sys
        torch = sys.modules.get("torch")
        return torch.cuda.device(self.device) if torch is not None and torch.cuda.is_available() else contextlib.nullcontext()

    def _graph_to_device(self, unitigs: dict, links) -> dict:
        import torch
        g = self._graph_of(unitigs, links)
        signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}
        out = {}
        for k, dt in zip(self.GRAPH_KEYS, self.GRAPH_DTYPES):
            a = np.ascontiguousarray(g[k], dtype=dt)
            out[k] = torch.from_numpy(a.view(signed.get(a.dtype, a.dtype))).to(f"cuda:{self.device}")
        return out

    @staticmethod
    def _graph_to_host(g: dict) -> dict:
        unsigned = {np.dtype(np.int64): np.uint64, np.dtype(np.int32): np.uint32}
        out = {}
        for k, v in g.items():
            if hasattr(v, "cpu"):
                a = v.cpu().numpy()
                v = a.view(unsigned.get(a.dtype, a.dtype))
            out[k] = v
        return out

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
        check(lib().aix_reads_fix(self._h, _np_ptr(out) if m else None, out.shape[0], _np_ptr(st) if m else None, _np_ptr(en) if m else None, m, true_errors,
                                  verify, max_fixes, _np_ptr(rec) if m else None, _np_ptr(fix_pos) if logs else None, _np_ptr(fix_old) if logs else None),
              "aix_reads_fix")
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
            check(lib().aix_reads_fix_dev(self._h, vp(buf_t.data_ptr()) if m else None, buf_t.numel(), vp(start_t.data_ptr()) if m else None,
                                          vp(end_t.data_ptr()) if m else None, m, true_errors, verify, max_fixes, vp(rec.data_ptr()) if m else None,
                                          vp(fix_pos_t.data_ptr()) if logs else None, vp(fix_old_t.data_ptr()) if logs else None,
                                          _stream_ptr(self.device)), "aix_reads_fix_dev")
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
        check(lib().aix_tf_spectrum(self._h, nbins, _np_ptr(hist), _np_ptr(stats)), "aix_tf_spectrum")
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
        check(lib().aix_top_kmers(self._h, min_tf, n, C.byref(pk), C.byref(pt), C.byref(ps) if want_kmers else None, C.byref(m), C.byref(total)),
              "aix_top_kmers")
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
        check(lib().aix_kmers_by_kid(self._h, _np_ptr(kd) if n else None, n, _np_ptr(out) if n else None, _np_ptr(rc) if n else None,
                                     _np_ptr(tf) if n else None), "aix_kmers_by_kid")
        return out, rc, tf

    def kmer_values_t(self, out_t=None):
        """int32[n] device tensor (u32 bit patterns): the value of every entry in kid order, asynchronous on torch's current stream."""
        import torch
        if out_t is None:
            out_t = torch.empty(self.n, dtype=torch.int32, device=f"cuda:{self.device}")
        elif out_t.dtype != torch.int32 or out_t.numel() != self.n:
            raise ValueError("out_t must be an int32 tensor of n elements")
        self._chk_dev(out_t)
        with torch.cuda.device(self.device):
            check(lib().aix_kmer_values_dev(self._h, vp(out_t.data_ptr()) if self.n else None, _stream_ptr(self.device)), "aix_kmer_values_dev")
        return out_t

    def tf_spectrum_t(self, nbins: int):
        """(hist int64[nbins], stats int64[8]) device tensors on torch's current stream: complete on return for a 23-mer handle (the values
        pass uses pool scratch), asynchronous for a 13-mer handle."""
        import torch
        if nbins < 2:
            raise ValueError("nbins must be at least 2")
        dev = f"cuda:{self.device}"
        hist, stats = torch.empty(nbins, dtype=torch.int64, device=dev), torch.empty(_lib.SPECTRUM_STATS, dtype=torch.int64, device=dev)
        with torch.cuda.device(self.device):
            check(lib().aix_tf_spectrum_dev(self._h, nbins, vp(hist.data_ptr()), vp(stats.data_ptr()), _stream_ptr(self.device)), "aix_tf_spectrum_dev")
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
        with torch.cuda.device(self.device):
            if not min_tf >> 32:                                    # else: no u32 value reaches it
                check(lib().aix_top_kmers_dev(self._h, min_tf, n, vp(kid.data_ptr()), vp(tf.data_ptr()), vp(kmers.data_ptr()) if want_kmers else None, cap,
                                              C.byref(m), C.byref(total), _stream_ptr(self.device)), "aix_top_kmers_dev")
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
        with torch.cuda.device(dev):
            check(lib().aix_kmers_by_kid_dev(self._h, vp(kids_t.data_ptr()) if n else None, n, vp(out.data_ptr()) if n else None,
                                             vp(rc.data_ptr()) if (want_rc and n) else None, vp(tf.data_ptr()) if (want_tf and n) else None,
                                             _stream_ptr(self.device)), "aix_kmers_by_kid_dev")
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
