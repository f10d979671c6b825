"""Batch read retrieval on the GPU (aix_readsquery.hip): spans / read ids / k-mers -> the reads' bytes as CSR.
Every comparison is exact equality."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from aindex_amd import _lib, synth
from aindex_amd.engine import Index

_COMP = bytes.maketrans(b"ACGT", b"TGCA")
LENS = (0, 1, 15, 16, 17, 63, 64, 65)


def _digest(strings) -> str:
    """tests/golden/make_golden_reads.py: digest()"""
    h = hashlib.sha256()
    for s in strings:
        b = s.encode("latin-1")
        h.update(len(b).to_bytes(8, "little") + b)
    return h.hexdigest()


def _items(off, data):
    off = off.tolist()
    b = data.tobytes()
    return [b[off[i]:off[i + 1]] for i in range(len(off) - 1)]


@pytest.fixture(scope="module")
def acc(small23_prefix, tmp_path_factory):
    """The AIndex mirror over small23 with the positions files built by the GPU and the reads loaded."""
    from aindex_amd.aindex import AIndex
    ai = AIndex.load_from_prefix(small23_prefix)
    prefix = str(tmp_path_factory.mktemp("readsq") / "acc")
    ai._wrapper.build_aindex(small23_prefix + ".reads", prefix)
    ai.load_aindex(prefix + ".index.bin", prefix + ".indices.bin", 100)
    ai.load_reads(small23_prefix + ".reads")
    ai.positions_prefix = prefix
    yield ai
    ai._wrapper.close()


def _with_reads(acc, small23_prefix, reads_path):
    """A second mirror over the small23 index and positions files with another reads file loaded."""
    from aindex_amd.aindex import AIndex
    ai = AIndex.load_from_prefix(small23_prefix)
    ai.load_aindex(acc.positions_prefix + ".index.bin", acc.positions_prefix + ".indices.bin", 100)
    ai.load_reads(reads_path)
    return ai


def test_golden_reads_of_the_compiled_reference(acc, gold, small23_prefix):
    """1. get_read_by_rid for every rid (and n_reads, n_reads + 1, 2^40; lengths and one digest over all answers, a sample in full) and get_read for the seeded triples of the golden files, through
    the list surface and the array surface; aix_reads_info and device_bytes follow attach / detach."""
    docs = [json.load(open(os.path.join(gold, "small23", "reads_access.json"))), json.load(open(os.path.join(gold, "compute_reads", "reads_access.json")))]
    seen = 0
    for doc in docs:
        for f in doc["files"]:
            path = os.path.join(gold, f["reads"])
            if f["reads"].startswith("small23"):
                ai = acc
            else:
                ai = _with_reads(acc, small23_prefix, path)
            w = ai._wrapper
            try:
                ix = w._ix23
                before = ix.info["device_bytes"]
                tr = np.array(f["triples"], dtype=np.uint64).reshape(-1, 3)
                got = ai.get_reads_batch(tr[:, 0], tr[:, 1], tr[:, 2])
                assert sum(1 for t in f["triples"] if t[2]) * 3 >= len(f["triples"]) and sum(1 for s in f["get_read"] if s) * 3 >= len(f["get_read"])
                assert got == f["get_read"]
                assert ix.reads_info() == (1, f["size"]) and ix.info["device_bytes"] == before + f["size"]
                off, data = ai.get_reads_array(tr[:, 0], tr[:, 1], tr[:, 2])
                assert data.dtype == np.uint8 and [b.decode("latin-1") for b in _items(off, data)] == f["get_read"]
                for rc in (False, True):                         # one flag for the whole batch
                    pick = [i for i, t in enumerate(f["triples"]) if bool(t[2]) == rc]
                    assert ai.get_reads_batch(tr[pick, 0], tr[pick, 1], rc) == [f["get_read"][i] for i in pick]
                for got_r in (ai.get_reads_by_rid_batch(f["rids"]), None):        # the list surface, then the array surface
                    if got_r is None:
                        o2, d2 = ix.fetch_reads_by_rid(f["rids"])
                        got_r = [b.decode("latin-1") for b in _items(o2, d2)]
                    # every rid: lengths and the digest over all answers; the stored sample in full
                    assert [len(x) for x in got_r] == f["by_rid_len"] and _digest(got_r) == f["by_rid_sha256"]
                    assert all(got_r[f["rids"].index(int(r))] == x for r, x in f["by_rid_sample"].items())
                assert w._ridx_on_device() and ix.info["ridx_reads"] == f["n_reads"]
                held = ix.info["device_bytes"]                   # the positions index and the intervals were uploaded by the by-rid call
                ix.detach_reads()
                assert ix.reads_info() == (0, 0) and ix.info["device_bytes"] == held - f["size"]
                w._attached_reads = None
                seen += 1
            finally:
                if ai is not acc:
                    w.close()
    assert seen == 3
    # close releases an attachment too (nothing to observe but that it does not fail), and a second attach replaces the first
    with Index.open_23(small23_prefix + ".pf", small23_prefix + ".tf.bin", small23_prefix + ".kmers.bin") as ix:
        base = ix.info["device_bytes"]
        ix.attach_reads(b"ACGT\nTTTT\n")
        ix.attach_reads(b"ACGTACGT\n")
        assert ix.reads_info() == (1, 9) and ix.info["device_bytes"] == base + 9


def _own_reads(tmp_path):
    """A reads file with lower case, '~', bytes >= 0x80, empty lines, one read of more than 4 MiB and a last read without a newline."""
    rng = np.random.default_rng(101)
    alphabet = np.frombuffer(b"ACGTACGTACGTNacgtn~RYKM\x80\xff\xc3\xa9", dtype=np.uint8)
    reads = []
    for i in range(3000):
        ln = int(rng.choice(LENS)) if i % 2 else int(rng.integers(0, 300))
        reads.append(alphabet[rng.integers(0, alphabet.shape[0], ln)].tobytes())
    reads[7] = reads[8] = reads[9] = b""
    big = alphabet[rng.integers(0, alphabet.shape[0], (4 << 20) + 12345)].tobytes()
    reads.insert(1500, big)
    reads.append(b"ACGTNNacgt~TTGA\xfe")                                   # ends at the file size, no newline
    data = b"\n".join(reads)
    starts = np.zeros(len(reads), dtype=np.uint64)
    starts[1:] = np.cumsum([len(r) + 1 for r in reads[:-1]], dtype=np.uint64)
    ends = starts + np.array([len(r) for r in reads], dtype=np.uint64)
    assert int(ends[-1]) == len(data)
    path = str(tmp_path / "own.reads")
    open(path, "wb").write(data)
    with open(str(tmp_path / "own.ridx"), "w") as fh:
        for i in range(len(reads)):
            fh.write(f"{i}\t{int(starts[i])}\t{int(ends[i])}\n")
    return path, data, starts, ends


def _spans(size, starts, ends, n, seed):
    """n seeded (start, end, revcomp): every length of LENS and every source alignment, whole reads, spans across separators, edge cases."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, size, n).astype(np.int64)
    near = np.clip(starts[rng.integers(0, starts.shape[0], n)].astype(np.int64) + rng.integers(-40, 40, n), 0, size - 1)
    a = np.where(np.arange(n) % 2 == 1, near, a)                               # half of the spans begin near a read's start: across '\n'
    ln = np.where(np.arange(n) % 3 == 0, rng.integers(0, 400, n), rng.choice(LENS, n)).astype(np.int64)
    b = a + ln
    whole = np.arange(n) % 7 == 0                                              # a whole read
    r = rng.integers(0, starts.shape[0], n)
    a = np.where(whole, starts[r].astype(np.int64), a)
    b = np.where(whole, ends[r].astype(np.int64), b)
    b[5::97] = a[5::97] - 1                                                    # start > end
    a[11::89] = size + rng.integers(0, 50, a[11::89].shape[0])                 # start >= size
    b[13::83] = size                                                           # end == size
    a[17::79] = size - 1 - rng.integers(0, 200, a[17::79].shape[0])
    b[17::79] = size - 1                                                       # end == size - 1
    rc = rng.integers(0, 2, n).astype(np.uint8)
    return np.maximum(a, 0).astype(np.uint64), np.maximum(b, 0).astype(np.uint64), rc


def _check_alignments(off, starts):
    ln = np.diff(off.astype(np.int64))
    assert set(LENS) <= set(np.unique(ln).tolist())
    nz = ln > 0
    assert set((off[:-1][nz] % np.uint64(16)).tolist()) == set(range(16)), "every destination alignment"
    assert set((starts[nz] % np.uint64(16)).tolist()) == set(range(16)), "every source alignment"


def test_agrees_with_single_item_host_methods(acc, small23_prefix, tmp_path):
    """2. get_reads_batch / get_reads_by_rid_batch == the single-item host methods on 10^5 seeded items per file: small23 and a reads
    buffer written here (lower case, '~', bytes >= 0x80, empty lines, a read of more than 4 MiB, a last read without a newline)."""
    path, data, st_own, en_own = _own_reads(tmp_path)
    own = _with_reads(acc, small23_prefix, path)
    try:
        for ai, name in ((acc, "small23"), (own, "own")):
            w = ai._wrapper
            size = w.reads_size
            s, e, rc = _spans(size, w._ridx_start, w._ridx_end, 100_000, 7 if ai is acc else 8)
            if ai is own:                                                     # the 4 MiB read: whole (both strands), and spans inside it
                big = 1500
                s[:4] = [st_own[big], st_own[big], st_own[big] + np.uint64(3), st_own[big] + np.uint64(1_000_001)]
                e[:4] = [en_own[big], en_own[big], en_own[big] - np.uint64(5), st_own[big] + np.uint64(3_000_000)]
                rc[:4] = [0, 1, 1, 0]
            want = [w.get_read(int(a), int(b), bool(r)) for a, b, r in zip(s.tolist(), e.tolist(), rc.tolist())]
            nonempty = sum(1 for x in want if x)
            print(name, "spans", len(want), "non-empty", nonempty, "bytes", sum(map(len, want)))
            assert 3 * nonempty >= len(want)
            got = ai.get_reads_batch(s, e, rc)
            assert got == want
            off, by = ai.get_reads_array(s, e, rc)
            assert by.tobytes().decode("latin-1") == "".join(want)
            _check_alignments(off, s)
            rng = np.random.default_rng(21)
            rids = rng.integers(0, w.n_reads, 100_000).astype(np.uint64)
            rids[3::1000] = w.n_reads + rng.integers(0, 5, rids[3::1000].shape[0]).astype(np.uint64)
            if ai is own:
                keep = rids != 1500
                rids = np.concatenate([rids[keep], np.array([1500, 7, 8, 9, w.n_reads - 1, 1500], dtype=np.uint64)])
            want_r = [w.get_read_by_rid(int(r)) for r in rids.tolist()]
            assert ai.get_reads_by_rid_batch(rids) == want_r and w._ridx_on_device()
            assert 3 * sum(1 for x in want_r if x) >= len(want_r)
            if ai is own:
                assert want_r[-1].encode("latin-1") == data[int(st_own[1500]):int(en_own[1500])] and len(want_r[-1]) > (4 << 20)
                assert want_r[-2].encode("latin-1") == b"ACGTNNacgt~TTGA\xfe" and want_r[-5:-2] == ["", "", ""]
                o_r, _ = w._ix23.fetch_reads_by_rid(rids)
                _check_alignments(o_r, w._ridx_start[np.minimum(rids, np.uint64(w.n_reads - 1)).astype(np.int64)])
    finally:
        own._wrapper.close()


def _dirty(stored, rng):
    out = []
    for i, s in enumerate(stored):
        b = bytearray(s.encode())
        j = int(rng.integers(0, 23))
        kind = i % 7
        if kind == 0:
            b = bytearray(bytes(b).lower())
        elif kind == 1:
            b[j] = ord("N")
        elif kind == 2:
            b[j] = ord("~")
        elif kind == 3:
            b[j] = ord("\n")
        elif kind == 4:
            b[j] = 0x80 + int(rng.integers(0, 128))
        elif kind == 5:
            b[j] |= 0x20                                      # one lower-case letter
        else:
            b[0] = 0xFF
            b[22] = ord("n")
        out.append(bytes(b).decode("latin-1"))
    return out


class _MemoPositions:
    """get_positions of the wrapper, remembered per k-mer: the host loop runs once per max_reads over the same items."""

    def __init__(self, w):
        self.w, self.memo = w, {}
        self.orig = w.get_positions

    def __enter__(self):
        def memo(kmer):
            if kmer not in self.memo:
                self.memo[kmer] = self.orig(kmer)
            return self.memo[kmer]
        self.w.get_positions = memo
        return self

    def __exit__(self, *a):
        del self.w.get_positions


def _compare_by_kmer(ai, items, ms=(0, 1, 2, 100, 10 ** 6)):
    w = ai._wrapper
    out = {}
    with _MemoPositions(w):
        for m in ms:
            want = [w.get_reads_se_by_kmer(s, m) for s in items]
            got = ai.get_reads_by_kmer_batch(items, m)
            print("max_reads", m, "k-mers with a read", sum(1 for x in want if x), "of", len(items), "reads", sum(map(len, want)))
            assert got == want
            out[m] = want
    return out


def test_reads_by_kmer_equals_the_host_loop(acc, gold):
    """3. get_reads_by_kmer_batch(items, m) == [get_reads_se_by_kmer(s, m) for s in items] for m in 0, 1, 2, 100, 10^6 over all 5 901
    stored k-mers of small23, their reverse complements, 1 000 absent and ~300 dirty ones, verification table on and off."""
    w = acc._wrapper
    rng = np.random.default_rng(11)
    stored = [acc.get_kmer_by_kid(i) for i in range(acc.n_kmers)]
    assert len(stored) == 5901
    rcs = [s.encode().translate(_COMP)[::-1].decode() for s in stored]
    absent = [bytes(r).decode() for r in synth.random_kmers_ascii(77, 1000, 23)]
    dirty = _dirty(stored[:230] + rcs[:64], rng) + ["", stored[0][:22], stored[1] + "A", "", stored[2][:22].lower(), "N" * 24]
    items = stored + rcs + absent + dirty
    assert len(items) == 13102
    # the condition on the inputs, from the committed arrays alone: 2 519 of the 5 901 stored k-mers have occurrences
    z = np.load(os.path.join(gold, "small23", "aindex.npz"))
    ind, pos = z["indices"], z["index"]
    nzc = np.concatenate([[0], np.cumsum(pos != 0)])
    with_occ = int(((nzc[ind[1:].astype(np.int64)] - nzc[ind[:-1].astype(np.int64)]) > 0).sum())
    assert with_occ == 2519 and 3 * 2 * with_occ >= len(items)
    order = rng.permutation(len(items))
    items = [items[i] for i in order]
    ix = w._ix23
    first = None
    for table in (True, False):
        ix.set_bucket_table(table)
        try:
            res = _compare_by_kmer(acc, items)
        finally:
            ix.set_bucket_table(True)
        assert 3 * sum(1 for x in res[100] if x) >= len(items)
        assert all(len(x) <= 1 for x in res[0]) and all(len(x) <= 1 for x in res[1]) and all(len(x) <= 2 for x in res[2])
        assert sum(1 for x in res[0] if x) == sum(1 for x in res[1] if x) > 0          # max_reads = 0 still yields one read
        assert first is None or res == first
        first = res
    # the array surface and the wrapper of AIndex
    sample = [s for s in items if len(s) == 23][:2000]
    koff, rid, roff, by = acc.get_reads_by_kmers_array(sample, 3)
    lists = first[2]
    want3 = [w.get_reads_se_by_kmer(s, 3) for s in sample]
    flat = [b.decode("latin-1") for b in _items(roff, by)]
    assert [flat[int(koff[i]):int(koff[i + 1])] for i in range(len(sample))] == want3 and by.dtype == np.uint8
    assert [w.get_read_by_rid(int(r)) for r in rid.tolist()] == flat
    assert acc.get_reads_by_kmer_batch(sample[:50]) == [acc.get_reads_by_kmer(s) for s in sample[:50]] and lists is not None


def _tandem_index(tmp_path):
    """An index built through the project's own tools from seeded 300 bp reads made of tandem repeats (period 30 - 60), units shared
    between reads: most k-mers meet a read several times and several reads."""
    from aindex_amd import tools
    _lib.lib()                                                 # loaded the usual way (torch's HIP runtime first) before tools.main asks for a torch-free load
    rng = np.random.default_rng(404)
    units = ["".join("ACGT"[c] for c in rng.integers(0, 4, int(rng.integers(30, 61)))) for _ in range(120)]
    reads = []
    for i in range(480):
        u = units[int(rng.integers(0, len(units)))]
        shift = int(rng.integers(0, len(u)))
        reads.append(((u[shift:] + u[:shift]) * 11)[:300])
    out = str(tmp_path)
    open(os.path.join(out, "t.reads"), "w").write("".join(r + "\n" for r in reads))
    open(os.path.join(out, "t.fa"), "w").write("".join(f">r{i}\n{r}\n" for i, r in enumerate(reads)))
    cwd = os.getcwd()
    os.chdir(out)
    try:
        assert tools.main(["kmer_counter", "t.fa", "23", "t.dat"]) == 0
        open("keys.txt", "w").write("".join(r.split("\t")[0] + "\n" for r in open("t.dat").read().split("\n") if r))
        assert tools.main(["compute_mphf_seq", "keys.txt", "t.pf"]) == 0
        assert tools.main(["compute_index", "t.dat", "t.pf", "t", "4", "0"]) == 0
        assert tools.main(["compute_reads", "t.reads", "-", "reads", "t"]) == 0
        assert tools.main(["compute_aindex", "t.reads", "t.pf", "t", "4", "23", "t.tf.bin", "t.kmers.bin", "keys.txt"]) == 0
    finally:
        os.chdir(cwd)
    return os.path.join(out, "t")


def _load(prefix, index_bin=None):
    from aindex_amd.aindex import AIndex
    ai = AIndex.load_from_prefix(prefix)
    ai.load_aindex(index_bin or prefix + ".index.bin", prefix + ".indices.bin", 100)
    ai.load_reads(prefix + ".reads")
    return ai


def test_dedup_and_any_slot_order(tmp_path):
    """4. Tandem repeats: >= 200 k-mers with more occurrences than distinct reads; batch == host loop. Then the slots of every bucket
    permuted: batch == host loop again, and for max_reads = 1 the answer differs from the unpermuted one for some k-mer."""
    prefix = _tandem_index(tmp_path)
    ai = _load(prefix)
    try:
        w = ai._wrapper
        stored = [ai.get_kmer_by_kid(i) for i in range(ai.n_kmers)]
        ind = np.asarray(w._indices).astype(np.int64)
        pos = np.asarray(w._positions).copy()
        assert w._ridx_sorted
        repeated = 0
        for h in range(ai.n_kmers):
            seg = pos[ind[h]:ind[h + 1]]
            seg = seg[seg != 0] - np.uint64(1)
            reads = {w._interval(int(p)) for p in seg.tolist()}
            repeated += int(len(reads) < seg.shape[0])
        print("k-mers", ai.n_kmers, "with more occurrences than distinct reads", repeated)
        assert repeated >= 200
        items = stored + [s.encode().translate(_COMP)[::-1].decode() for s in stored[::3]]
        plain = _compare_by_kmer(ai, items)
        assert 3 * sum(1 for x in plain[100] if x) >= len(items)
        assert max(len(x) for x in plain[100]) >= 3
    finally:
        ai._wrapper.close()
    rng = np.random.default_rng(5)
    perm = pos.copy()
    for h in range(ind.shape[0] - 1):
        lo, hi = int(ind[h]), min(int(ind[h + 1]), perm.shape[0])
        if hi - lo > 1:
            perm[lo:hi] = perm[lo:hi][rng.permutation(hi - lo)]
    assert not np.array_equal(perm, pos)
    perm.tofile(prefix + ".perm.index.bin")
    ai = _load(prefix, prefix + ".perm.index.bin")
    try:
        shuffled = _compare_by_kmer(ai, items)
        assert [sorted(x) for x in shuffled[10 ** 6]] == [sorted(x) for x in plain[10 ** 6]]
        differ = sum(1 for a, b in zip(shuffled[1], plain[1]) if a != b)
        print("k-mers whose first read changed with the slot order", differ)
        assert differ >= 1
    finally:
        ai._wrapper.close()


def test_addressing_beyond_4gib(small23_prefix):
    """5. A device reads buffer of more than 4 GiB (synth_reads_t), spans whose sources straddle 2^31 and 2^32 bytes, and one fetch whose
    OUTPUT exceeds 4 GiB, compared on slabs around each boundary with torch indexing of the same buffer."""
    import torch
    from aindex_amd import engine
    g = engine.synth_genome_t(31, 4_000_000)
    n_reads = 29_000_000
    reads_t = engine.synth_reads_t(47, g, n_reads, 150, rc_half=True, n_rate_ppm=1000)
    size = reads_t.numel()
    assert size == n_reads * 151 and size > (1 << 32) + (1 << 26)
    lut = torch.arange(256, dtype=torch.uint8, device="cuda")
    for a, b in zip(b"ACGT", b"TGCA"):
        lut[a] = b
    with Index.open_23(small23_prefix + ".pf", small23_prefix + ".tf.bin", small23_prefix + ".kmers.bin") as ix:
        before = ix.info["device_bytes"]
        ix.attach_reads_t(reads_t)
        assert ix.reads_info() == (2, size) and ix.info["device_bytes"] == before           # borrowed: not the handle's bytes
        # sources that straddle the boundaries, both strands, odd alignments
        starts, ends, rcs = [], [], []
        for edge in (1 << 31, 1 << 32):
            for d, ln in ((1, 2), (7, 16), (8, 17), (100, 333), (65536 + 3, 200_001), (13, 1 << 20)):
                for rc in (0, 1):
                    starts.append(edge - d); ends.append(edge - d + ln); rcs.append(rc)
        st = torch.tensor(starts, dtype=torch.int64, device="cuda")
        en = torch.tensor(ends, dtype=torch.int64, device="cuda")
        rc_t = torch.tensor(rcs, dtype=torch.uint8, device="cuda")
        off, by = ix.fetch_reads_t(st, en, rc_t)
        torch.cuda.synchronize()
        off = off.cpu().tolist()
        for i, (a, b, r) in enumerate(zip(starts, ends, rcs)):
            want = reads_t[a:b]
            if r:
                want = lut[want.flip(0).long()]
            assert off[i + 1] - off[i] == b - a and torch.equal(by[off[i]:off[i + 1]], want), (a, b, r)
        # one fetch of 4.4 GiB: 69 spans of 64 MiB + 1 at odd starts, every third one reverse-complemented
        n, ln = 69, (64 << 20) + 1
        s_np = (np.arange(n, dtype=np.int64) * 60_000_001 + 12_345) % (size - ln - 1)
        s_np[40] = (1 << 32) - 1_000_003                                                     # source across 2^32
        s_np[41] = (1 << 31) - 77
        r_np = (np.arange(n) % 3 == 1).astype(np.uint8)
        off, by = ix.fetch_reads_t(torch.from_numpy(s_np).cuda(), torch.from_numpy(s_np + ln).cuda(), torch.from_numpy(r_np).cuda())
        torch.cuda.synchronize()
        assert by.numel() == n * ln and by.numel() > (1 << 32) + (1 << 27)
        assert off.cpu().tolist() == [i * ln for i in range(n + 1)]
        slab = 1 << 16
        probes = {0, ln - slab, ln // 2}
        for i in range(n):
            for edge in (1 << 31, 1 << 32):                                                  # the output boundaries and the source boundaries
                if i * ln <= edge < (i + 1) * ln:
                    probes.add(min(max(edge - i * ln - slab // 2, 0), ln - slab))
            local = set(probes)
            for edge in (1 << 31, 1 << 32):
                if int(s_np[i]) <= edge < int(s_np[i]) + ln:
                    t = edge - int(s_np[i])
                    local.add(min(max((ln - t if r_np[i] else t) - slab // 2, 0), ln - slab))
            for p in local:
                got = by[i * ln + p:i * ln + p + slab]
                if r_np[i]:
                    want = lut[reads_t[int(s_np[i]) + ln - p - slab:int(s_np[i]) + ln - p].flip(0).long()]
                else:
                    want = reads_t[int(s_np[i]) + p:int(s_np[i]) + p + slab]
                assert torch.equal(got, want), (i, p)
        crossing = [i for i in range(n) if i * ln <= (1 << 32) < (i + 1) * ln]
        assert len(crossing) == 1
        del by
        # by rid beyond 2^32: every line is one read of 150 bases
        rid_np = np.array([0, 1, (1 << 31) // 151, (1 << 31) // 151 + 1, (1 << 32) // 151 - 1, (1 << 32) // 151, (1 << 32) // 151 + 1, n_reads - 1, n_reads], dtype=np.int64)
        starts64 = np.arange(n_reads, dtype=np.uint64) * np.uint64(151)
        assert ix.attach_ridx(np.stack([np.arange(n_reads, dtype=np.uint64), starts64, starts64 + np.uint64(150)], axis=1)) is True
        o_r, b_r = ix.fetch_reads_by_rid_t(torch.from_numpy(rid_np).cuda())
        torch.cuda.synchronize()
        assert o_r.cpu().tolist() == [150 * i for i in range(9)] + [1200]
        for i, r in enumerate(rid_np[:-1].tolist()):
            assert torch.equal(b_r[150 * i:150 * i + 150], reads_t[151 * r:151 * r + 150])
        ix.detach_reads()
        assert ix.reads_info() == (0, 0)
    del reads_t
    torch.cuda.empty_cache()


def test_errors_and_protocol(small23_prefix, gold):
    """6. Every query with nothing attached, by-rid / by-kmers without intervals -> AIX_ERR_ARG; N = 0 -> offsets = {0}; _dev with cap too
    small writes offsets and the total only; query after detach -> AIX_ERR_ARG."""
    import torch
    z = np.load(os.path.join(gold, "small23", "aindex.npz"))
    reads = open(small23_prefix + ".reads", "rb").read()
    L, vp = _lib.lib(), _lib.vp
    checker = np.fromfile(small23_prefix + ".kmers.bin", dtype=np.uint64)
    q = np.ascontiguousarray(synth.decode_kmers(checker, 23)).reshape(-1)
    n = checker.shape[0]
    ridx = np.loadtxt(small23_prefix + ".ridx", dtype=np.uint64).reshape(-1, 3)

    def refused(fn, *a):
        with pytest.raises(_lib.AixError) as ei:
            fn(*a)
        assert ei.value.status == _lib.AIX_ERR_ARG

    with Index.open_23(small23_prefix + ".pf", small23_prefix + ".tf.bin", small23_prefix + ".kmers.bin") as ix:
        qt = torch.from_numpy(q.copy()).cuda()
        i64 = lambda a: torch.tensor(a, dtype=torch.int64, device="cuda")
        # nothing attached
        refused(ix.fetch_reads, [0], [10])
        refused(ix.fetch_reads_by_rid, [0])
        refused(ix.reads_by_kmers, q)
        refused(ix.fetch_reads_t, i64([0]), i64([10]))
        refused(ix.fetch_reads_by_rid_t, i64([0]))
        refused(ix.reads_by_kmers_t, qt)
        assert ix.reads_info() == (0, 0)
        # reads only: spans work, by-rid and by-kmers need the intervals (and the positions)
        ix.attach_reads(reads)
        off, by = ix.fetch_reads([0, 151], [150, 301])
        assert by.tobytes() == reads[0:150] + reads[151:301] and off.tolist() == [0, 150, 300]
        refused(ix.fetch_reads_by_rid, [0])
        refused(ix.reads_by_kmers, q)
        ix.attach_aindex(z["indices"], z["index"])
        refused(ix.reads_by_kmers, q)
        refused(ix.reads_by_kmers_t, qt)
        assert ix.attach_ridx(ridx) is True
        koff, rid, roff, data = ix.reads_by_kmers(q, 100)
        assert koff.shape[0] == n + 1 and int(koff[-1]) == rid.shape[0] > 1000 and int(roff[-1]) == data.shape[0]
        kt, rt, ot, bt = ix.reads_by_kmers_t(qt, 100)
        torch.cuda.synchronize()
        assert np.array_equal(kt.cpu().numpy().view(np.uint64), koff) and np.array_equal(rt.cpu().numpy().view(np.uint64), rid)
        assert np.array_equal(ot.cpu().numpy().view(np.uint64), roff) and np.array_equal(bt.cpu().numpy(), data)
        # positions_batch_t(locate=True) feeds fetch_reads_by_rid_t without leaving the device
        _, _, rid_t, _ = ix.positions_batch_t(qt, locate=True)
        o_t, b_t = ix.fetch_reads_by_rid_t(rid_t)
        o_h, b_h = ix.fetch_reads_by_rid(rid_t.cpu().numpy().view(np.uint64))
        assert rid_t.numel() > 1000 and np.array_equal(o_t.cpu().numpy().view(np.uint64), o_h) and np.array_equal(b_t.cpu().numpy(), b_h)
        # N = 0
        for o, b in (ix.fetch_reads([], []), ix.fetch_reads_by_rid([])):
            assert o.tolist() == [0] and b.shape == (0,)
        k0, r0, o0, b0 = ix.reads_by_kmers(b"", 5)
        assert k0.tolist() == [0] and r0.shape == (0,) and o0.tolist() == [0] and b0.shape == (0,)
        o, b = ix.fetch_reads_t(i64([]), i64([]))
        assert o.cpu().tolist() == [0] and b.numel() == 0
        k0t = ix.reads_by_kmers_t(qt[:0], 5)
        assert k0t[0].cpu().tolist() == [0] and k0t[1].numel() == 0 and k0t[2].cpu().tolist() == [0] and k0t[3].numel() == 0
        # cap below the total: canary untouched, offsets and the total written
        st_t, en_t = i64(ridx[:, 1].astype(np.int64).tolist()), i64(ridx[:, 2].astype(np.int64).tolist())
        m = ridx.shape[0]
        want_off, want_by = ix.fetch_reads(ridx[:, 1], ridx[:, 2])
        total = int(want_off[-1])
        for cap in (0, 1, total // 2, total - 1, total):
            buf = torch.full((total + 64,), 0x5A, dtype=torch.uint8, device="cuda")
            offs = torch.full((m + 1,), -1, dtype=torch.int64, device="cuda")
            tot = C.c_uint64()
            st = L.aix_reads_fetch_dev(ix._h, vp(st_t.data_ptr()), vp(en_t.data_ptr()), None, m, vp(offs.data_ptr()), vp(buf.data_ptr()), cap, C.byref(tot), None)
            torch.cuda.synchronize()
            assert st == 0 and tot.value == total and np.array_equal(offs.cpu().numpy().view(np.uint64), want_off)
            if cap < total:
                assert bool((buf == 0x5A).all().item())
            else:
                assert np.array_equal(buf[:total].cpu().numpy(), want_by) and bool((buf[total:] == 0x5A).all().item())
        # an output pointer that is not 16-byte aligned
        buf = torch.full((total + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        tot = C.c_uint64()
        offs = torch.empty(m + 1, dtype=torch.int64, device="cuda")
        assert L.aix_reads_fetch_dev(ix._h, vp(st_t.data_ptr()), vp(en_t.data_ptr()), None, m, vp(offs.data_ptr()), vp(buf.data_ptr() + 5), total, C.byref(tot), None) == 0
        torch.cuda.synchronize()
        assert np.array_equal(buf[5:5 + total].cpu().numpy(), want_by) and bool((buf[:5] == 0x5A).all().item()) and bool((buf[5 + total:] == 0x5A).all().item())
        # by-kmers with caps too small: kmer_offsets and the totals only
        R, nbytes = rid.shape[0], data.shape[0]
        for cap_r, cap_b in ((0, 0), (R - 1, nbytes), (R, nbytes - 1), (R, 0)):
            ko = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
            rr = torch.full((R + 8,), -7, dtype=torch.int64, device="cuda")
            ro = torch.full((R + 9,), -7, dtype=torch.int64, device="cuda")
            bb = torch.full((nbytes + 64,), 0x5A, dtype=torch.uint8, device="cuda")
            tots = (C.c_uint64 * 2)()
            st = L.aix_reads_by_kmers_dev(ix._h, vp(qt.data_ptr()), n, 100, vp(ko.data_ptr()), vp(rr.data_ptr()), vp(ro.data_ptr()), cap_r, vp(bb.data_ptr()), cap_b,
                                          C.byref(tots), None)
            torch.cuda.synchronize()
            assert st == 0 and (tots[0], tots[1]) == (R, nbytes) and np.array_equal(ko.cpu().numpy().view(np.uint64), koff)
            assert bool((bb == 0x5A).all().item())
            if cap_r < R:
                assert bool((rr == -7).all().item()) and bool((ro == -7).all().item())
            else:
                assert np.array_equal(rr[:R].cpu().numpy().view(np.uint64), rid) and np.array_equal(ro[:R + 1].cpu().numpy().view(np.uint64), roff)
        # a non-default stream
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            o_s, b_s = ix.fetch_reads_t(st_t, en_t)
        s.synchronize()
        assert np.array_equal(b_s.cpu().numpy(), want_by)
        # aix_aindex_detach keeps the reads; detach_reads drops them
        ix.detach_aindex()
        assert ix.reads_info() == (1, len(reads))
        refused(ix.fetch_reads_by_rid, [0])
        assert ix.fetch_reads([0], [150])[1].tobytes() == reads[:150]
        ix.detach_reads()
        refused(ix.fetch_reads, [0], [10])
        refused(ix.fetch_reads_t, st_t, en_t)
