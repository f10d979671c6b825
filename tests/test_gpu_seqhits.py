"""Sequences against the indexed reads on the GPU (aix_seqhits.hip): seed hits with strand, votes per (read, strand, diagonal).
Every comparison is exact equality."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import seqhits_ref as R
from aindex_amd import _lib, synth
from aindex_amd.engine import Index


@pytest.fixture(scope="module")
def acc(gold, small23_prefix, tmp_path_factory):
    """The AIndex mirror over small23 with the positions files built by the GPU (the recipe of test_gpu_posquery.py), reads and intervals loaded."""
    from aindex_amd.aindex import AIndex
    ai = AIndex.load_from_prefix(small23_prefix)
    prefix = str(tmp_path_factory.mktemp("seqh") / "acc")
    ai._wrapper.build_aindex(small23_prefix + ".reads", prefix)
    ai.load_aindex(prefix + ".index.bin", prefix + ".indices.bin", 100)
    ai.load_reads(small23_prefix + ".reads")
    yield ai
    ai._wrapper.close()


@pytest.fixture(scope="module")
def ref(small23_prefix):
    return R.Ref(small23_prefix)


@pytest.fixture(scope="module")
def std(small23_prefix, ref):
    """The standard queries with the reference's answers, computed once."""
    qs = R.standard_queries(small23_prefix)
    return {"qs": qs, "hits": R.hits_csr(ref, qs), "votes": R.votes_csr(ref, qs)}


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)


def test_against_the_single_item_path(acc, ref, std, small23_prefix):
    """1. 68 sequences (40 indexed reads, 20 reverse complements, two genome slices, lower case, planted N ~ newline 0x80 0xFF, lengths 0 22
    23 24): hits == per window get_positions / get_rid / get_start of the mirror and the byte rule on the reads file; votes == seqhits_ref."""
    qs = std["qs"]
    reads = open(small23_prefix + ".reads", "rb").read()
    off, qoff, pos, rid, local, flag = acc.get_sequence_hits_array(qs)
    want = []
    for s in qs:
        for q in range(max(0, len(s) - 22)):
            w = s[q:q + 23]
            r = R.rc_bytes(w)
            for p in acc.get_positions(w.decode("latin-1")):
                t = reads[p:p + 23] if p + 23 <= len(reads) else None
                st = 0 if t == w else (1 if t == r else 2)
                found = acc._wrapper._interval(p) is not None
                want.append((q, p, acc.get_rid(p), p - acc.get_start(p), st | (4 if found else 0)))
    assert len(want) == int(off[-1]) and len(want) > 50000
    assert list(zip(qoff.tolist(), pos.tolist(), rid.tolist(), local.tolist(), flag.tolist())) == want
    _same((off, qoff, pos, rid, local, flag), std["hits"])
    got_v = acc._wrapper._ix23.seq_votes(qs)
    _same(got_v, std["votes"])
    # the conditions on the inputs (test_seqhits_cpu.py checks them on the reference alone)
    nh = np.diff(off.astype(np.int64))
    vo, vrid, vstrand, vdiag, votes, qf, ql = got_v
    big = [bool((votes[int(vo[i]):int(vo[i + 1])] >= 10).any()) for i in range(len(qs))]
    print("sequences with hits", int((nh > 0).sum()), "of", len(qs), "with a group >= 10:", sum(big), "strand-2 hits", int(((flag & 3) == 2).sum()))
    assert 3 * int((nh > 0).sum()) >= len(qs) and sum(big) >= 20 and set(vstrand.tolist()) == {0, 1} and int(((flag & 3) == 2).sum()) > 0
    # the list surface
    m = acc.map_sequences(qs, min_votes=2)
    w2 = [ref.votes(s, 2) for s in qs]
    assert m == w2 and sum(map(len, m)) > 100


def _cached(ref, cache, seqs, what, **kw):
    per = []
    for s in seqs:
        key = (what, s, tuple(sorted(kw.items())))
        if key not in cache:
            cache[key] = getattr(ref, what)(s, **kw)
        per.append(cache[key])
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(p) for p in per], dtype=np.uint64)
    return off, [x for p in per for x in p]


def _rows(arrs):
    return arrs[0], list(zip(*[a.tolist() for a in arrs[1:]]))


def test_shapes(acc, ref, std):
    """2. M in {0, 1, 63, 64, 65, 257}; a 23-byte sequence last in the buffer, an empty one between two long ones, one at an odd offset, one
    of 70 000 bytes of repeated genome slices; max_per_kmer in {0, 1, 3}; min_votes in {1, 2, 1000}; the _dev twins with cap = 0,
    total - 1 (canaries intact) and total; host, numpy and torch surfaces agree."""
    import torch
    ix = acc._wrapper._ix23
    acc._wrapper._attach_for_mapping()
    qs, cache = std["qs"], {}
    pool = [q for q in qs if len(q) >= 23]
    for M in (0, 1, 63, 64, 65, 257):
        seqs = [pool[(7 * i) % len(pool)] if i % 9 else pool[i % len(pool)][: 20 + i % 30] for i in range(M)]
        for m in ((0, 1, 3) if M == 65 else (0,)):
            off, rows = _rows(ix.seq_hits(seqs, max_per_kmer=m))
            woff, wrows = _cached(ref, cache, seqs, "hits", max_per_kmer=m)
            assert np.array_equal(off, woff) and rows == wrows and (M < 2 or len(rows) > 100)
            for mv in ((1, 2, 1000) if M == 65 else (1,)):
                voff, vrows = _rows(ix.seq_votes(seqs, min_votes=mv, max_per_kmer=m))
                wvoff, wvrows = _cached(ref, cache, seqs, "votes", min_votes=mv, max_per_kmer=m)
                assert np.array_equal(voff, wvoff) and vrows == wvrows
                assert M < 2 or (len(vrows) > 0) == (mv < 1000)
    g = synth.genome_ascii(1, 3000).tobytes()
    long = (g[100:800] + R.revcomp(g[1500:1801]) + g[300:1001])
    long = (long * (70000 // len(long) + 1))[:70000]
    seqs = [pool[3], b"", long, pool[0][:23], pool[4][1:], pool[2][:23]]
    assert sum(map(len, seqs[:4])) % 2 == 1 and len(seqs[-1]) == 23
    h = ix.seq_hits(seqs)
    off, rows = _rows(h)
    woff, wrows = _cached(ref, cache, seqs, "hits")
    assert np.array_equal(off, woff) and rows == wrows and len(rows) > 200000
    v = ix.seq_votes(seqs, min_votes=2)
    voff, vrows = _rows(v)
    wvoff, wvrows = _cached(ref, cache, seqs, "votes", min_votes=2)
    assert np.array_equal(voff, wvoff) and vrows == wvrows and max(r[3] for r in vrows) > 50
    # torch surface, and the _dev protocol with canaries behind every output
    data = torch.frombuffer(bytearray(b"".join(seqs)), dtype=torch.uint8).cuda()
    offs = torch.tensor(np.concatenate([[0], np.cumsum([len(s) for s in seqs])]), dtype=torch.int64).cuda()
    ht = ix.seq_hits_t(data, offs)
    vt = ix.seq_votes_t(data, offs, min_votes=2, cap_hint=len(vrows))
    for a, b in zip(ht, h):
        assert np.array_equal(a.cpu().numpy().view(b.dtype), b)
    for a, b in zip(vt, v):
        assert np.array_equal(a.cpu().numpy().view(b.dtype), b)
    L, vp, M = _lib.lib(), _lib.vp, len(seqs)
    st = vp(torch.cuda.current_stream().cuda_stream)
    for name, want, dts, extra in (("aix_seq_hits_dev", h, (torch.int32, torch.int64, torch.int64, torch.int64, torch.uint8), (0,)),
                                   ("aix_seq_votes_dev", v, (torch.int64, torch.uint8, torch.int64, torch.int32, torch.int32, torch.int32), (0, 2))):
        total = len(want[1])
        for cap in (0, total - 1, total):
            o = torch.full((M + 1,), -1, dtype=torch.int64).cuda()
            outs = [torch.full((total + 8,), 0x5A, dtype=dt).cuda() for dt in dts]
            tot = C.c_uint64(12345)
            _lib.check(getattr(L, name)(ix._h, vp(data.data_ptr()), vp(offs.data_ptr()), M, *extra, vp(o.data_ptr()),
                                        *[vp(t.data_ptr()) if cap else None for t in outs], cap, C.byref(tot), st), name)
            assert tot.value == total and np.array_equal(o.cpu().numpy().view(np.uint64), want[0])
            for t, w in zip(outs, want[1:]):
                a = t.cpu().numpy()
                if cap == total:
                    assert np.array_equal(a[:total].view(w.dtype), w) and (a[total:] == 0x5A).all()
                else:
                    assert (a == 0x5A).all()


def test_hostile_index(acc, small23_prefix):
    """3. A copy of the positions array with zeros, entries into the last 22 bytes of the reads, entries beyond the reads and entries at a
    newline planted in buckets the queries visit: the result is the reference's on that array; hits beyond the file have strand 2 and no
    interval. Answers only: every read of the reads buffer is bounds-checked in the kernel."""
    w = acc._wrapper
    ix = w._attach_for_mapping()
    reads = open(small23_prefix + ".reads", "rb").read()
    ind = np.asarray(w._indices).copy()
    pos = np.asarray(w._positions).copy()
    qs = R.standard_queries(small23_prefix)[:12]
    base = R.Ref(small23_prefix)
    nl = reads.index(b"\n")
    plant = [0, 0] + [len(reads) - k + 1 for k in (1, 2, 3, 4, 11, 22)] + [len(reads) + 1, len(reads) + 6, 1 << 40, nl + 1, len(reads) - 23 + 1]
    done = 0
    for s in qs:
        for q in range(0, len(s) - 22, 5):
            h = base.bucket(s[q:q + 23])
            if h is None:
                continue
            nz = np.nonzero(pos[int(ind[h]):int(ind[h + 1])])[0]
            if nz.shape[0] >= 2:
                pos[int(ind[h]) + int(nz[done % nz.shape[0]])] = plant[done % len(plant)]
                done += 1
    assert done > 150
    ref = R.Ref(small23_prefix, indices=ind, positions=pos)
    ix.attach_aindex(ind, pos)
    try:
        got = ix.seq_hits(qs)
        want = R.hits_csr(ref, qs)
        for g, x in zip(got, want):
            assert g.dtype == x.dtype and np.array_equal(g, x)
        off, qoff, p, rid, local, flag = got
        beyond = p.astype(np.int64) + 23 > len(reads)
        tail = beyond & (p < len(reads))
        past = p >= np.uint64(len(reads) + 2)
        print("hits", p.shape[0], "ending beyond the reads", int(beyond.sum()), "of them inside the last 22 bytes", int(tail.sum()), "past the end", int(past.sum()))
        assert int(tail.sum()) >= 6 and int(past.sum()) >= 2 and ((flag[beyond] & 3) == 2).all() and ((flag[past] & 4) == 0).all()
        assert int((p == nl).sum()) > 0 and ((flag[p == nl] & 3) == 2).all()
        for mv in (1, 2):
            for g, x in zip(ix.seq_votes(qs, min_votes=mv), R.votes_csr(ref, qs, mv)):
                assert g.dtype == x.dtype and np.array_equal(g, x)
    finally:
        w._attached_key = None                                 # the mirror uploads its own arrays again on its next batch call
    assert acc.map_sequences(qs[:3]) == [base.votes(s, 2) for s in qs[:3]]


def test_switch_independence(acc, ref, std):
    """4. Verification table on / off and absence filter on / off give identical arrays."""
    ix = acc._wrapper._attach_for_mapping()
    qs = std["qs"]
    want_v = R.votes_csr(ref, qs, 2)
    for table, filt in ((True, True), (True, False), (False, False), (False, True)):
        ix.set_bucket_table(table)
        ix.set_absence_filter(filt)
        try:
            h, v = ix.seq_hits(qs), ix.seq_votes(qs, min_votes=2)
        finally:
            ix.set_bucket_table(True)
            ix.set_absence_filter(True)
        _same(h, std["hits"])
        _same(v, want_v)
        assert int(h[0][-1]) > 50000 and v[1].shape[0] > 100


def test_errors(gold, small23_prefix, tmp_path):
    """5. A 13-mer handle: AIX_ERR_MODE. Each missing attachment: AIX_ERR_ARG. The Python surface raises RuntimeError naming the piece."""
    from pf13 import pf13_path
    from aindex_amd.aindex import AIndex
    z = np.load(os.path.join(gold, "small23", "aindex.npz"))
    reads = open(small23_prefix + ".reads", "rb").read()
    ridx = np.loadtxt(small23_prefix + ".ridx", dtype=np.uint64).reshape(-1, 3)
    seqs = [reads[:150]]
    with Index.open_13(pf13_path(), None) as ix13:
        for call in (lambda: ix13.seq_hits(seqs), lambda: ix13.seq_votes(seqs)):
            with pytest.raises(_lib.AixError) as e:
                call()
            assert e.value.status == _lib.AIX_ERR_MODE
    with Index.open_23(small23_prefix + ".pf", small23_prefix + ".tf.bin", small23_prefix + ".kmers.bin") as ix:
        def both_fail():
            for call in (lambda: ix.seq_hits(seqs), lambda: ix.seq_votes(seqs)):
                with pytest.raises(_lib.AixError) as e:
                    call()
                assert e.value.status == _lib.AIX_ERR_ARG
        both_fail()                                            # nothing attached
        ix.attach_aindex(z["indices"], z["index"])
        both_fail()                                            # no intervals, no reads
        assert ix.attach_ridx(ridx)
        both_fail()                                            # no reads
        ix.attach_reads(reads)
        assert int(ix.seq_hits(seqs)[0][-1]) > 100
        ix.detach_reads()
        both_fail()
        ix.attach_reads(reads)
        ix.detach_aindex()                                     # drops the positions index and the intervals
        both_fail()
    ai = AIndex.load_from_prefix(small23_prefix)
    try:
        with pytest.raises(RuntimeError, match="positions index"):
            ai.map_sequences(["ACGT" * 10])
        with pytest.raises(RuntimeError, match="positions index"):
            ai.get_sequence_hits_array(["ACGT" * 10])
        # every other missing piece is named too, in the order positions, intervals, reads
        w = ai._wrapper
        z["index"].tofile(str(tmp_path / "a.index.bin"))
        z["indices"].tofile(str(tmp_path / "a.indices.bin"))
        ai.load_aindex(str(tmp_path / "a.index.bin"), str(tmp_path / "a.indices.bin"), 100)
        with pytest.raises(RuntimeError, match=r"sorted \.ridx"):              # no intervals loaded
            ai.map_sequences(seqs)
        sh = ridx[np.random.default_rng(5).permutation(ridx.shape[0])]
        np.savetxt(str(tmp_path / "shuffled.ridx"), sh, fmt="%d", delimiter="\t")
        w.load_reads_index(str(tmp_path / "shuffled.ridx"))
        assert w._ridx_sorted is False
        with pytest.raises(RuntimeError, match=r"sorted \.ridx"):              # intervals that are not sorted and disjoint
            ai.get_sequence_hits_array(seqs)
        w.load_reads_index(small23_prefix + ".ridx")
        with pytest.raises(RuntimeError, match="needs the reads"):             # intervals on the device, no reads
            ai.map_sequences(seqs)
        w.load_reads(small23_prefix + ".reads")
        assert sum(map(len, ai.map_sequences(seqs))) > 0                       # every piece there: an answer
        w._is_13mer_mode = True
        try:
            with pytest.raises(RuntimeError, match="23-mer index"):
                ai.map_sequences(seqs)
        finally:
            w._is_13mer_mode = False
        # M empty sequences as device tensors (no byte buffer at all): all-zero offsets, as the host twin gives
        import torch
        ix = w._ix23
        e_off = torch.zeros(4, dtype=torch.int64, device="cuda")
        empty = torch.empty(0, dtype=torch.uint8, device="cuda")
        ht, vt = ix.seq_hits_t(empty, e_off), ix.seq_votes_t(empty, e_off)
        assert ht[0].tolist() == [0, 0, 0, 0] and vt[0].tolist() == [0, 0, 0, 0] and ht[1].numel() == 0 and vt[1].numel() == 0
        assert ix.seq_hits([b"", b"", b""])[0].tolist() == [0, 0, 0, 0]
    finally:
        ai._wrapper.close()
