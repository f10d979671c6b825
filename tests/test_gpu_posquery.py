"""Batch position queries on the GPU (aix_posquery.hip): k-mers -> CSR of positions, read ids and offsets in the read.
Every comparison is exact equality."""
import ctypes as C
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle_lib as O
from aindex_amd import _lib, builder, synth
from aindex_amd.engine import Index

_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _lists(off, vals):
    off, vals = off.tolist(), vals.tolist()
    return [vals[off[i]:off[i + 1]] for i in range(len(off) - 1)]


@pytest.fixture(scope="module")
def acc(gold, small23_prefix, tmp_path_factory):
    """The AIndex mirror over small23 with the positions files built by the GPU, as test_positions_and_reads_access_golden does."""
    from aindex_amd.aindex import AIndex
    ai = AIndex.load_from_prefix(small23_prefix)
    prefix = str(tmp_path_factory.mktemp("posq") / "acc")
    ai._wrapper.build_aindex(small23_prefix + ".reads", prefix)
    ai.load_aindex(prefix + ".index.bin", prefix + ".indices.bin", 100)
    ai.load_reads(small23_prefix + ".reads")
    yield ai
    ai._wrapper.close()


def test_golden_23mers_positions_and_reads(acc, gold):
    """1. The compiled reference's own answers (tests/golden/small23/access.json): 180 k-mers, 75 of them with occurrences, 930 occurrences,
    and the (rid, start) of 300-odd probe positions, the edge probes 0, 1, 149 .. 152 and 10^9 among them."""
    a = json.load(open(os.path.join(gold, "small23", "access.json")))
    got = acc.get_positions_batch(a["kmers"])
    nonempty = sum(1 for p in got if p)
    print("non-empty", nonempty, "of", len(got), "occurrences", sum(map(len, got)))
    assert 3 * sum(1 for p in a["positions"] if p) >= len(a["kmers"])
    assert got == a["positions"]
    assert acc._wrapper._ix23.info["aindex_attached"] == 1 and acc._wrapper._ix23.info["aindex_entries"] == acc._wrapper._positions.shape[0]
    for probes in (a["probes"], [0, 1, 149, 150, 151, 152, 10 ** 9]):
        rid, start = acc._wrapper.get_rid_start_batch(probes)
        want_r = a["rid"] if probes is a["probes"] else [acc.get_rid(p) for p in probes]
        want_s = a["start"] if probes is a["probes"] else [acc.get_start(p) for p in probes]
        assert rid.tolist() == want_r and start.tolist() == want_s
    assert acc._wrapper._ix23.info["ridx_on_device"] == 1 and acc._wrapper._ix23.info["ridx_reads"] == acc.n_reads
    # the array surface: packed bytes, 'S23', joined str give the same CSR; locate=True equals get_rid / get_start per occurrence
    flat = "".join(a["kmers"])
    off, pos, rid, loc = acc.get_positions_array(flat, locate=True)
    assert _lists(off, pos) == a["positions"]
    for form in (flat.encode(), np.frombuffer(flat.encode(), dtype="S23"), list(a["kmers"])):
        o2, p2 = acc.get_positions_array(form)
        assert np.array_equal(o2, off) and np.array_equal(p2, pos)
    assert rid.tolist() == [acc.get_rid(p) for p in pos.tolist()]
    assert loc.tolist() == [p - acc.get_start(p) for p in pos.tolist()]


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


def test_agrees_with_single_kmer_path_on_every_kind_of_input(acc, small23_prefix):
    """2. Batch == [get_positions(s) ...] for all 5 901 stored k-mers and their reverse complements, 2 000 absent random k-mers and a few
    hundred dirty ones (lower case, N, ~, newline, bytes >= 0x80, lengths 0 / 22 / 24), with the verification table on and off and the
    absence filter on and off; get_rid2poses_batch == the per-k-mer get_rid2poses."""
    w = acc._wrapper
    rng = np.random.default_rng(11)
    stored = [acc.get_kmer_by_kid(i) for i in range(acc.n_kmers)]
    assert len(stored) == 5901
    rcs = [s.encode().translate(_COMP)[::-1].decode() for s in stored]
    absent = [bytes(r).decode() for r in synth.random_kmers_ascii(77, 2000, 23)]
    dirty = _dirty(stored[:280] + rcs[:70], rng) + ["", stored[0][:22], stored[1] + "A", "", stored[2][:22].lower(), "N" * 24]
    items = stored + rcs + absent + dirty
    order = rng.permutation(len(items))
    items = [items[i] for i in order]
    ix = w._ix23
    want = None
    for table, filt in ((True, True), (True, False), (False, False), (False, True)):
        ix.set_bucket_table(table)
        ix.set_absence_filter(filt)
        try:
            single = [w.get_positions(s) for s in items]
            got = acc.get_positions_batch(items)
        finally:
            ix.set_bucket_table(True)
            ix.set_absence_filter(True)
        nonempty = sum(1 for p in single if p)
        print("table", table, "filter", filt, "non-empty", nonempty, "of", len(items))
        assert 3 * nonempty >= len(items)
        assert got == single
        assert want is None or single == want
        want = single
    sample = items[:3000]
    assert acc.get_rid2poses_batch(sample) == [acc.get_rid2poses(s) for s in sample]


def test_zeros_anywhere_in_a_bucket(acc):
    """3. Zeros planted at the head and in the middle of buckets of a copy of the small23 positions array: the result is the numpy filter of
    that array (non-zero entries minus one, in slot order)."""
    w = acc._wrapper
    ix = w._ix23
    ind = np.asarray(w._indices).copy()
    pos = np.asarray(w._positions).copy()
    planted = 0
    for h in range(0, ix.n, 3):
        lo, hi = int(ind[h]), int(ind[h + 1])
        nz = np.nonzero(pos[lo:hi])[0]
        if nz.shape[0] >= 3:
            pos[lo + nz[0]] = 0                               # head
            pos[lo + nz[nz.shape[0] // 2]] = 0                # middle
            planted += 1
    assert planted > 200
    stored = [acc.get_kmer_by_kid(i) for i in range(acc.n_kmers)]
    flat = "".join(stored).encode()
    checker = ix.checker_array()
    rc = synth.revcomp_codes(checker, 23)
    canon_ascii = synth.decode_kmers(np.minimum(checker, rc), 23)              # upper-case ACGT: byte order == code order
    h = ix.hash_ascii(canon_ascii)
    ok = (h < ix.n) & (checker[np.minimum(h, ix.n - 1).astype(np.int64)] == np.minimum(checker, rc))
    want = []
    for i in range(ix.n):
        seg = pos[int(ind[int(h[i])]):int(ind[int(h[i]) + 1])] if ok[i] else np.zeros(0, np.uint64)
        want.append((seg[seg != 0] - np.uint64(1)).tolist())
    assert 3 * sum(1 for p in want if p) >= len(want)
    ix.attach_aindex(ind, pos)
    try:
        off, got = ix.positions_batch(flat)
        assert _lists(off, got) == want
        for m in (1, 3):
            off_m, got_m = ix.positions_batch(flat, max_per_kmer=m)
            assert _lists(off_m, got_m) == [p[:m] for p in want]
    finally:
        w._attached_key = None                                 # the mirror uploads its own arrays again on its next batch call
    assert acc.get_positions_batch(stored[:50]) == [acc.get_positions(s) for s in stored[:50]]


def test_13mers_against_oracle_and_single_kmer_path(gold, tmp_path):
    """4. 13-mer positions built with the real u64 table (count13, then positions_fill on a 13-mer handle) == the oracle's arrays; the
    batch over 10^4 random 13-mers == get_positions_13mer one by one == a numpy slice of the oracle's arrays at hash_ascii(kmer);
    lower-case, N and wrong-length items give []."""
    from pf13 import pf13_path
    from aindex_amd.wrapper import AindexWrapper
    reads = open(os.path.join(gold, "count13", "synth.txt"), "rb").read()
    m = O.OracleMphf(pf13_path())
    prefix = str(tmp_path / "a13")
    with Index.open_13(pf13_path(), None) as ix:
        tf = ix.count13(reads, _lib.FMT_PLAIN)
        ix.set_tf_13(tf)
        ind, pos = ix.positions_fill(reads)
        oind, opos = O.positions13(m, tf, reads)
        assert np.array_equal(ind, oind) and np.array_equal(pos, opos) and int((pos != 0).sum()) > 0
    tf.tofile(prefix + ".tf.bin")
    pos.tofile(prefix + ".index.bin")
    ind.tofile(prefix + ".indices.bin")
    os.symlink(pf13_path(), prefix + ".pf")
    w = AindexWrapper()
    try:
        w.load_from_prefix_13mer(prefix)
        assert w.get_positions_batch([reads[:13].decode()]) == [[]]                   # nothing mapped yet
        w.load_aindex_from_prefix_13mer(prefix)
        a = np.frombuffer(reads, dtype=np.uint8)
        rng = np.random.default_rng(13)
        starts = rng.integers(0, a.shape[0] - 13, size=5000)
        from_reads = [bytes(a[s:s + 13]) for s in starts]                             # windows of the reads (some cross a newline)
        rnd = [bytes(r) for r in synth.random_kmers_ascii(5, 5000, 13)]
        kmers = [b.decode("latin-1") for b in from_reads + rnd]
        got = w.get_positions_batch(kmers)
        assert got == [w.get_positions_13mer(s) for s in kmers]
        hs = w._ix13.hash_ascii(np.frombuffer("".join(kmers).encode("latin-1"), dtype=np.uint8))
        want = []
        for s, h in zip(kmers, hs.tolist()):
            clean = all(c in "ACGT" for c in s)
            seg = opos[int(oind[h]):int(oind[h + 1])] if clean and h < 4 ** 13 else np.zeros(0, np.uint64)
            want.append((seg[seg != 0] - np.uint64(1)).tolist())
        assert got == want
        nonempty = sum(1 for p in got if p)
        print("13-mers non-empty", nonempty, "of", len(got))
        assert 3 * nonempty >= len(got)
        good = next(s for s, p in zip(kmers, got) if p)
        odd = [good.lower(), good[:4] + "N" + good[5:], good[:4], "", good, good + "A"]
        assert w.get_positions_batch(odd) == [[], [], [], [], w.get_positions_13mer(good), []]
        assert w.get_positions_batch(odd)[4] != []
        off, p2 = w.get_positions_array("".join(kmers[:100]), max_per_kmer=2)
        assert _lists(off, p2) == [p[:2] for p in got[:100]]
    finally:
        w.close()


HEAVY_COPIES = 100_000


@pytest.fixture(scope="module")
def mid_case():
    """About 10^6 reads of a synthetic genome plus 10^5 copies of one extra read (its 128 23-mers are the heavy ones), the index built on
    the GPU from the reads' own distinct k-mers, positions filled and attached device-resident."""
    import torch
    from aindex_amd import engine, counting
    g = engine.synth_genome_t(29, 2_000_000)
    reads_a = engine.synth_reads_t(43, g, 1_000_000, 150, rc_half=True, n_rate_ppm=0)
    heavy_read = np.concatenate([synth.genome_ascii(1234, 150), np.frombuffer(b"\n", dtype=np.uint8)])
    reads_b = torch.from_numpy(np.tile(heavy_read, HEAVY_COPIES)).cuda()
    reads_t = torch.cat([reads_a, reads_b])
    del reads_a, reads_b
    keys, counts = counting.count_distinct_t(reads_t, 23, _lib.CANON_TRUE_RC)
    pf = builder.build_pf_codes_t(keys, 23)
    ix = Index.build_23_codes_t(pf, keys, counts.to(torch.int32))
    ind_t, pos_t = ix.positions_fill_t(reads_t)
    ix.attach_aindex_t(ind_t, pos_t)
    torch.cuda.synchronize()
    # expectation side, from host copies; this does not go through the probe code
    checker = ix.checker_array()
    ind = ind_t.cpu().numpy().view(np.uint64)
    pos = pos_t.cpu().numpy().view(np.uint64)
    order = np.argsort(checker, kind="stable")
    nzc = np.concatenate([[0], np.cumsum(pos != 0)]).astype(np.int64)
    case = {"ix": ix, "reads_t": reads_t, "keys": keys.cpu().numpy().view(np.uint64), "checker_sorted": checker[order], "order": order,
            "ind": ind.astype(np.int64), "nzc": nzc, "cpos": pos[pos != 0] - np.uint64(1), "heavy": heavy_read[:23].copy(), "keep": (ind_t, pos_t)}
    yield case
    ix.close()


def _expected_csr(case, q_ascii):
    """numpy CSR for clean upper-case queries: canonical code -> searchsorted in the sorted checker -> slice of the positions array."""
    codes = synth.encode_kmers(q_ascii)
    canon = np.minimum(codes, synth.revcomp_codes(codes, 23))
    cs, order, ind, nzc = case["checker_sorted"], case["order"], case["ind"], case["nzc"]
    at = np.minimum(np.searchsorted(cs, canon), cs.shape[0] - 1)
    hit = cs[at] == canon
    h = order[at]
    first = np.where(hit, nzc[ind[h]], 0)
    cnt = np.where(hit, nzc[ind[h + 1]] - nzc[ind[h]], 0)
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    return off, first, cnt


def test_mid_size_device_resident_skewed(mid_case):
    """5. 10^6 queries (half present on a random strand, half random, the heavy k-mer several times) through positions_batch_t against a
    numpy CSR computed from host copies of checker / indices / positions; locate=True against numpy.searchsorted on the .ridx starts."""
    import torch
    ix = mid_case["ix"]
    n = 1_000_000
    keys = mid_case["keys"]
    pick = (synth.sm64(5, np.arange(n // 2, dtype=np.uint64)) % np.uint64(keys.shape[0])).astype(np.int64)
    codes = keys[pick]
    flip = (synth.sm64(6, np.arange(n // 2, dtype=np.uint64)) & np.uint64(1)).astype(bool)
    codes = np.where(flip, synth.revcomp_codes(codes, 23), codes)
    q = np.concatenate([synth.decode_kmers(codes, 23), synth.random_kmers_ascii(7, n - n // 2, 23)])
    q = q[np.random.default_rng(9).permutation(n)].copy()
    heavy_at = [0, 17, 4096, 500_000, 999_999]
    q[heavy_at] = mid_case["heavy"]
    off_w, first, cnt = _expected_csr(mid_case, q)
    assert 3 * int((cnt > 0).sum()) >= n and all(int(cnt[i]) >= HEAVY_COPIES for i in heavy_at)
    print("queries", n, "non-empty", int((cnt > 0).sum()), "entries", int(off_w[-1]), "longest", int(cnt.max()), "median non-empty", float(np.median(cnt[cnt > 0])))
    qt = torch.from_numpy(q.reshape(-1)).cuda()
    off_t, pos_t = ix.positions_batch_t(qt)
    torch.cuda.synchronize()
    off = off_t.cpu().numpy()
    assert np.array_equal(off, off_w)
    src = np.repeat(first - off_w[:-1], cnt) + np.arange(int(off_w[-1]), dtype=np.int64)
    assert np.array_equal(pos_t.cpu().numpy().view(np.uint64), mid_case["cpos"][src])
    # max_per_kmer on the device path
    off3_t, pos3_t = ix.positions_batch_t(qt, max_per_kmer=3)
    c3 = np.minimum(cnt, 3)
    o3 = np.concatenate([[0], np.cumsum(c3)]).astype(np.int64)
    assert np.array_equal(off3_t.cpu().numpy(), o3)
    src3 = np.repeat(first - o3[:-1], c3) + np.arange(int(o3[-1]), dtype=np.int64)
    assert np.array_equal(pos3_t.cpu().numpy().view(np.uint64), mid_case["cpos"][src3])
    # reads: every line of the buffer is one read of 150 bases (rid i at 151 i .. 151 i + 150)
    n_reads = mid_case["reads_t"].numel() // 151
    starts = np.arange(n_reads, dtype=np.uint64) * np.uint64(151)
    triples = np.stack([np.arange(n_reads, dtype=np.uint64), starts, starts + np.uint64(150)], axis=1)
    assert ix.attach_ridx(triples) is True
    sub = qt.view(-1, 23)[:100_000].contiguous().view(-1)
    o_t, p_t, r_t, l_t = ix.positions_batch_t(sub, locate=True)
    p = p_t.cpu().numpy().view(np.uint64)
    assert np.array_equal(o_t.cpu().numpy(), off_w[:100_001]) and p.shape[0] >= 100_000
    # the first interval with end + 1 >= pos (end = start + 150): an occurrence at the very start of read r > 0 belongs to read r - 1,
    # as get_rid answers (the probe 151 of the golden vector)
    key = np.where(p > 0, p - np.uint64(1), np.uint64(0))
    at = np.searchsorted(starts, np.maximum(key, np.uint64(150)) - np.uint64(150), side="left")
    assert int(at.max()) < n_reads and np.all(starts[at] <= p + np.uint64(1)) and int((at != p // np.uint64(151)).sum()) > 0
    assert np.array_equal(r_t.cpu().numpy().view(np.uint64), at.astype(np.uint64))
    assert np.array_equal(l_t.cpu().numpy().view(np.uint64), p - starts[at])
    rid, st = ix.locate(p[:1000])
    assert np.array_equal(rid, at[:1000].astype(np.uint64)) and np.array_equal(st, starts[at[:1000]])
    edge = np.array([0, 1, 150, 151, 152, 151 * n_reads - 1, 151 * n_reads, 151 * n_reads + 1, 10 ** 12], dtype=np.uint64)
    rid, st = ix.locate(edge)
    assert rid.tolist() == [0, 0, 0, 0, 1, n_reads - 1, n_reads - 1, 0, 0] and st.tolist() == [0, 0, 0, 0, 151, 151 * (n_reads - 1), 151 * (n_reads - 1), 0, 0]


def test_output_beyond_4gib(mid_case):
    """6. The heavy k-mer queried 5 400 times: more than 2^29 entries, i.e. byte offsets into the output pass 2^32 (locate=False).
    Allocates on the device: 8 B per entry of output (about 4.4 GB) and about 0.3 B per entry of scratch (a 64-bit mask, a 32-bit count
    and a 64-bit rank per 64 entries), next to the index of the fixture; the comparison of the lists runs on the device in slices."""
    import torch
    ix = mid_case["ix"]
    reps = 5400
    q = np.tile(mid_case["heavy"], (reps, 1))
    q[1::2] = np.frombuffer(bytes(mid_case["heavy"]).translate(_COMP)[::-1], dtype=np.uint8)      # every other one as the reverse complement
    off_w, first, cnt = _expected_csr(mid_case, q)
    L = int(cnt[0])
    assert L >= HEAVY_COPIES and np.all(cnt == L) and reps * L > (1 << 29)
    qt = torch.from_numpy(q.reshape(-1)).cuda()
    off_t, pos_t = ix.positions_batch_t(qt)
    torch.cuda.synchronize()
    assert pos_t.numel() == reps * L and pos_t.numel() * 8 > (1 << 32)
    assert np.array_equal(off_t.cpu().numpy(), off_w)
    lists = pos_t.view(reps, L)
    for r0 in range(0, reps, 600):                                                                 # every list equals the first one
        assert bool((lists[r0:r0 + 600] == lists[0:1]).all().item())
    want = mid_case["cpos"][int(first[0]):int(first[0]) + L]
    assert np.array_equal(pos_t[:10_000].cpu().numpy().view(np.uint64), want[:10_000])
    assert np.array_equal(pos_t[-10_000:].cpu().numpy().view(np.uint64), want[-10_000:])
    del pos_t, lists
    torch.cuda.empty_cache()


def test_protocol_and_hygiene(small23_prefix, gold):
    """7. cap below the total leaves a canary-filled buffer untouched and still reports the total; 0xFF-filled outputs come back fully
    overwritten; N = 0; max_per_kmer = 1 and 3 are prefixes; nothing attached is AIX_ERR_ARG; detach then re-attach; a non-default stream."""
    import torch
    z = np.load(os.path.join(gold, "small23", "aindex.npz"))
    ind, pos = z["indices"], z["index"]
    L, vp = _lib.lib(), _lib.vp
    checker = np.fromfile(small23_prefix + ".kmers.bin", dtype=np.uint64)
    q = np.ascontiguousarray(synth.decode_kmers(checker, 23)).reshape(-1)
    n = checker.shape[0]
    with Index.open_23(small23_prefix + ".pf", small23_prefix + ".tf.bin", small23_prefix + ".kmers.bin") as ix:
        # nothing attached: the documented error from every entry point
        po, pp = vp(), vp()
        assert L.aix_positions_query(ix._h, q.ctypes.data_as(vp), n, 0, C.byref(po), C.byref(pp), None, None) == _lib.AIX_ERR_ARG
        with pytest.raises(_lib.AixError) as ei:
            ix.positions_batch(q)
        assert ei.value.status == _lib.AIX_ERR_ARG
        with pytest.raises(_lib.AixError) as ei:
            ix.locate([1, 2, 3])
        assert ei.value.status == _lib.AIX_ERR_ARG
        qt = torch.from_numpy(q.copy()).cuda()
        with pytest.raises(_lib.AixError) as ei:
            ix.positions_batch_t(qt)
        assert ei.value.status == _lib.AIX_ERR_ARG
        # a malformed image is refused, and nothing stays attached
        bad = ind.copy()
        bad[5], bad[6] = bad[6] + 1, bad[5]
        with pytest.raises(_lib.AixError) as ei:
            ix.attach_aindex(bad, pos)
        assert ei.value.status == _lib.AIX_ERR_FORMAT and ix.info["aindex_attached"] == 0
        with pytest.raises(_lib.AixError) as ei:
            ix.attach_aindex(ind, pos[:-1])                                  # indices[n] > total
        assert ei.value.status == _lib.AIX_ERR_FORMAT
        ix.attach_aindex(ind, pos)
        off, full = ix.positions_batch(q)
        lists = _lists(off, full)
        total = int(off[-1])
        assert 3 * sum(1 for p in lists if p) >= n
        # N = 0
        o0, p0 = ix.positions_batch(b"")
        assert o0.tolist() == [0] and p0.shape == (0,)
        o0t = ix.positions_batch_t(qt[:0])
        assert o0t[0].cpu().tolist() == [0] and o0t[1].numel() == 0
        # max_per_kmer
        for m in (1, 3):
            om, pm = ix.positions_batch(q, max_per_kmer=m)
            assert _lists(om, pm) == [p[:m] for p in lists]
        # cap below the total: canary untouched at and beyond cap (and below it: nothing is written at all), total reported
        canary = 0x5A5A5A5A5A5A5A5A
        for cap in (0, 1, total // 2, total - 1):
            buf = torch.full((total + 8,), canary, dtype=torch.int64, device="cuda")
            offs = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
            tot = C.c_uint64()
            st = L.aix_positions_query_dev(ix._h, vp(qt.data_ptr()), n, 0, vp(offs.data_ptr()), vp(buf.data_ptr()), None, None, cap, C.byref(tot), None)
            torch.cuda.synchronize()
            assert st == 0 and tot.value == total and np.array_equal(offs.cpu().numpy().view(np.uint64), off)
            assert bool((buf[cap:] == canary).all().item()) and bool((buf == canary).all().item())
        # outputs pre-filled with 0xFF come back fully overwritten; cap == total exactly, the slack behind it stays
        assert ix.attach_ridx(np.stack([np.arange(3, dtype=np.uint64), np.array([0, 151, 302], np.uint64), np.array([150, 301, 452], np.uint64)], axis=1))
        bufs = [torch.full((total + 8,), -1, dtype=torch.int64, device="cuda") for _ in range(3)]
        offs = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
        tot = C.c_uint64()
        st = L.aix_positions_query_dev(ix._h, vp(qt.data_ptr()), n, 0, vp(offs.data_ptr()), vp(bufs[0].data_ptr()), vp(bufs[1].data_ptr()), vp(bufs[2].data_ptr()),
                                       total, C.byref(tot), None)
        torch.cuda.synchronize()
        assert st == 0 and tot.value == total
        assert np.array_equal(bufs[0][:total].cpu().numpy().view(np.uint64), full)
        for b in bufs:
            assert bool((b[total:] == -1).all().item())
        p64 = full.astype(np.int64)
        rid_w = np.where(p64 <= 151, 0, np.where(p64 <= 302, 1, np.where(p64 <= 453, 2, 0)))       # first interval with end + 1 >= pos, if start <= pos + 1
        start_w = np.where(p64 <= 151, 0, np.where(p64 <= 302, 151, np.where(p64 <= 453, 302, 0)))
        assert np.array_equal(bufs[1][:total].cpu().numpy(), rid_w) and np.array_equal(bufs[2][:total].cpu().numpy(), p64 - start_w)
        # a query on a non-default torch stream
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            o_s, p_s = ix.positions_batch_t(qt)
        s.synchronize()
        assert np.array_equal(o_s.cpu().numpy().view(np.uint64), off) and np.array_equal(p_s.cpu().numpy().view(np.uint64), full)
        # detach, then re-attach (device tensors this time)
        ix.detach_aindex()
        assert ix.info["aindex_attached"] == 0 and ix.info["ridx_on_device"] == 0
        with pytest.raises(_lib.AixError):
            ix.positions_batch(q)
        ind_t = torch.from_numpy(ind.view(np.int64).copy()).cuda()
        pos_t = torch.from_numpy(pos.view(np.int64).copy()).cuda()
        ix.attach_aindex_t(ind_t, pos_t)
        assert ix.info["aindex_attached"] == 2
        o_r, p_r = ix.positions_batch(q)
        assert np.array_equal(o_r, off) and np.array_equal(p_r, full)
        # read intervals that are not sorted and disjoint are reported, not attached
        assert ix.attach_ridx([[0, 0, 150], [1, 100, 300]]) is False and ix.info["ridx_on_device"] == 0
