"""Sequences with mismatches against the indexed reads on the GPU (aix_seqfind.hip): Hamming-verified alignments from seed hits, strand
counts, and the analysis functions over them, against the restatement of seqfind_ref.py. Every comparison is exact equality.
test_seqfind_cpu.py checks on the CPU that the inputs used here give results of every kind."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import seqfind_ref as F
from aindex_amd import _lib, synth
from aindex_amd.engine import Index

TRIP = _lib.SEQFIND_TRIP_BYTES                                 # AIX_SEQFIND_TRIP_BYTES: pattern bytes per trip of the verification loop


@pytest.fixture(scope="module")
def acc(gold, small23_prefix, tmp_path_factory):
    """The AIndex mirror over small23 with the positions files built by the GPU (the recipe of test_gpu_seqhits.py), reads and intervals loaded."""
    from aindex_amd.aindex import AIndex
    ai = AIndex.load_from_prefix(small23_prefix)
    prefix = str(tmp_path_factory.mktemp("seqf") / "acc")
    ai._wrapper.build_aindex(small23_prefix + ".reads", prefix)
    ai.load_aindex(prefix + ".index.bin", prefix + ".indices.bin", 100)
    ai.load_reads(small23_prefix + ".reads")
    yield ai
    ai._wrapper.close()


@pytest.fixture(scope="module")
def ref(small23_prefix):
    return F.FindRef(small23_prefix)


@pytest.fixture(scope="module")
def pats():
    return [p for p, _ in F.standard_patterns()]


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)


def test_standard_set(acc, ref, pats):
    """1. The standard patterns through Index.seq_find, AIndex.find_sequences_array and the list surface; hd in {0, 1, 3}, seed_step in
    {1, 7, 23}, max_per_kmer in {0, 1}."""
    ix = acc._wrapper._attach_for_mapping()
    n1 = 0
    for hd in (0, 1, 3):
        for step in (1, 7, 23):
            for m in (0, 1):
                want = F.find_csr(ref, pats, hd, step, m)
                _same(ix.seq_find(pats, hd, step, m), want)
                n1 += int((want[5] >= 1).sum())
    assert n1 > 500
    want = F.find_csr(ref, pats, 3, 23, 0)
    got = acc.find_sequences_array(pats, hd=3)
    _same(got, want)
    assert int((got[5] >= 1).sum()) > 500 and set(got[4].tolist()) == {0, 1}
    _same(acc.find_sequences_array([p.decode() for p in pats[:50]], 1, 7, 1), F.find_csr(ref, pats[:50], 1, 7, 1))
    _same(ix.seq_find(pats[:50], 2, 0), F.find_csr(ref, pats[:50], 2, 23))              # seed_step 0 means 23
    lists = acc.find_reads_by_sequence_batch(pats[:80], hd=3)
    reads = {r: ref.reads[s:e].decode() for r, s, e in zip(ref.rid, ref.start, ref.end)}
    assert lists == [[(r, l, reads[r], s, d) for _, r, l, s, d in ref.find(p, 3)] for p in pats[:80]] and sum(map(len, lists)) > 100


def test_shapes(acc, ref, pats):
    """2. M in {0, 1, 63, 64, 65, 257}; lengths 0, 22 and 23; a sequence at an odd offset; a 23-byte pattern last in the buffer."""
    ix = acc._wrapper._attach_for_mapping()
    memo = {}

    def want_of(seqs, hd, step):
        per = []
        for s in seqs:
            if (s, hd, step) not in memo:
                memo[(s, hd, step)] = ref.find(s, hd, step)
            per.append(memo[(s, hd, step)])
        off = np.zeros(len(seqs) + 1, np.uint64)
        off[1:] = np.cumsum([len(p) for p in per], dtype=np.uint64)
        return off, [x for p in per for x in p]
    for M in (0, 1, 63, 64, 65, 257):
        seqs = [pats[(7 * i) % len(pats)] if i % 9 else pats[i % len(pats)][: 20 + i % 6] for i in range(M)]
        got = ix.seq_find(seqs, 3, 23)
        off, rows = want_of(seqs, 3, 23)
        assert np.array_equal(got[0], off) and list(zip(*[a.tolist() for a in got[1:]])) == rows and (M < 63 or len(rows) > 100)
    long = [p for p in pats if len(p) == 150]
    k23 = [p for p in pats if len(p) == 23 and ref.find(p, 0)]
    odd = next(p[1:] for p in long if ref.find(p[1:], 2, 1))     # chosen by the restatement: a pattern with answers at an odd offset
    seqs = [long[0], b"", long[1][:22], k23[0], odd, long[3], k23[1]]
    assert sum(map(len, seqs[:4])) % 2 == 1 and len(seqs[-1]) == 23
    got = ix.seq_find(seqs, 2, 1)
    off, rows = want_of(seqs, 2, 1)
    assert np.array_equal(got[0], off) and list(zip(*[a.tolist() for a in got[1:]])) == rows
    nres = np.diff(off.astype(np.int64))
    assert nres[1] == 0 and nres[2] == 0 and nres[3] > 0 and nres[6] > 0 and nres[4] > 0
    assert ix.seq_find([b"", b"", b""])[0].tolist() == [0, 0, 0, 0] and ix.seq_find([])[0].tolist() == [0]


def test_long_reads_trip_boundaries(small23_prefix):
    """3. A second index on the device: 40 reads of 700 bytes cut from the same genome, half of them reverse-complemented. Patterns whose
    lengths sit on, just below and just above every boundary of the verification loop that a read of 700 bytes can hold (k TRIP for k = 1 ..
    10, TRIP = 64 bytes per trip; 4 bytes per lane within it), with the only mismatches in the last trip: early exit must not fire before it,
    and the byte-wise tail is exercised."""
    g = synth.genome_ascii(1, 3000).tobytes()
    rng = np.random.default_rng(11)
    starts = rng.integers(0, 2300, 40).tolist()
    rs = [g[s:s + 700] if i % 2 == 0 else F.comp_rev(g[s:s + 700]) for i, s in enumerate(starts)]
    reads = b"\n".join(rs) + b"\n"
    ridx = np.asarray([(i, 701 * i, 701 * i + 700) for i in range(40)], np.uint64)
    with Index.open_23(small23_prefix + ".pf", small23_prefix + ".tf.bin", small23_prefix + ".kmers.bin") as ix:
        ind, pos = ix.positions_fill(reads)
        ix.attach_aindex(ind, pos)
        assert ix.attach_ridx(ridx)
        ix.attach_reads(reads)
        ref = F.FindRef(small23_prefix, indices=ind, positions=pos, reads=reads, ridx=ridx)
        lens = sorted({b + d for b in range(TRIP, 700 + 1, TRIP) for d in (-1, 0, 1, 3, 4, 5)} | {23, 699, 700})
        seqs, planted = [], []
        for k, L in enumerate(lens):
            s = starts[k % 40] + (700 - L) * (k % 3) // 2       # a slice that at least read k % 40 holds whole
            last = ((L - 1) // TRIP) * TRIP                    # first byte of the last trip
            where = sorted({last, L - 1, (last + L - 1) // 2})[: 1 + k % 3]
            p = F.plant(g[s:s + L], where)
            seqs.append(F.comp_rev(p) if k % 2 else p)
            planted.append(len(where))
        for hd in (0, 1, 2, 3):
            want = F.find_csr(ref, seqs, hd, 23)
            _same(ix.seq_find(seqs, hd, 23), want)
            per = np.diff(want[0].astype(np.int64))
            for n, c in zip(planted, per):
                assert c == 0 or n <= hd                       # never found with more planted substitutions than hd
        want = F.find_csr(ref, seqs, 3, 23)
        assert int(want[0][-1]) > 20 and set(want[4].tolist()) == {0, 1} and int((want[5] >= 2).sum()) > 5


def test_dev_twins_and_surfaces(acc, ref, pats):
    """4. aix_seq_find_dev with cap = 0, total - 1 (canaries intact) and total; host, numpy and torch surfaces agree; kmer_strands_t."""
    import torch
    ix = acc._wrapper._attach_for_mapping()
    seqs = pats[:120]
    want = F.find_csr(ref, seqs, 3, 23)
    h = ix.seq_find(seqs, 3, 23)
    _same(h, want)
    data = torch.frombuffer(bytearray(b"".join(seqs)), dtype=torch.uint8).cuda()
    offs = torch.tensor(np.concatenate([[0], np.cumsum([len(s) for s in seqs])]), dtype=torch.int64).cuda()
    for hint in (0, 5, len(want[1]) + 7):
        for a, b in zip(ix.seq_find_t(data, offs, 3, 23, cap_hint=hint), h):
            assert np.array_equal(a.cpu().numpy().view(b.dtype), b)
    L, vp, M = _lib.lib(), _lib.vp, len(seqs)
    st = vp(torch.cuda.current_stream().cuda_stream)
    total = len(want[1])
    assert total > 200
    for cap in (0, total - 1, total):
        o = torch.full((M + 1,), -1, dtype=torch.int64).cuda()
        outs = [torch.full((total + 8,), 0x5A, dtype=dt).cuda() for dt in (torch.int64, torch.int64, torch.int64, torch.uint8, torch.int32)]
        tot = C.c_uint64(12345)
        _lib.check(L.aix_seq_find_dev(ix._h, vp(data.data_ptr()), vp(offs.data_ptr()), M, 3, 23, 0, vp(o.data_ptr()), *[vp(t.data_ptr()) if cap else None for t in outs],
                                      cap, C.byref(tot), st), "aix_seq_find_dev")
        assert tot.value == total and np.array_equal(o.cpu().numpy().view(np.uint64), want[0])
        for t, w in zip(outs, want[1:]):
            a = t.cpu().numpy()
            if cap == total:
                assert np.array_equal(a[:total].view(w.dtype), w) and (a[total:] == 0x5A).all()
            else:
                assert (a == 0x5A).all()
    e_off = torch.zeros(4, dtype=torch.int64, device="cuda")
    et = ix.seq_find_t(torch.empty(0, dtype=torch.uint8, device="cuda"), e_off, 3)
    assert et[0].tolist() == [0, 0, 0, 0] and et[1].numel() == 0
    km = b"".join(p[:23] for p in pats[:100])
    kt = ix.kmer_strands_t(torch.frombuffer(bytearray(km), dtype=torch.uint8).cuda())
    for a, b in zip(kt, ix.kmer_strands(km)):
        assert np.array_equal(a.cpu().numpy().view(np.uint64), b)


def test_hits_at_the_edges_of_the_reads(acc, small23_prefix):
    """5. Hits planted at the first and the last 23 bytes of the reads: patterns that reach before the first byte (a < 0) and beyond the
    last (a + L > the attached length) are dropped, as the restatement drops them. Answers only: the kernel stays in bounds by its own logic."""
    w = acc._wrapper
    ix = w._attach_for_mapping()
    reads = open(small23_prefix + ".reads", "rb").read()
    ind, pos = np.asarray(w._indices).copy(), np.asarray(w._positions).copy()
    base = F.FindRef(small23_prefix)
    end = len(reads) - 1                                       # the file ends with a newline
    first, last = reads[:23], reads[end - 23:end]
    for kmer, at in ((first, 0), (last, end - 23)):
        h = base.bucket(kmer)
        assert h is not None and ind[h + 1] > ind[h]
        pos[int(ind[h])] = at + 1
    junk = b"ACGTTGCAAC"
    seqs = [junk + reads[:60], F.comp_rev(junk + reads[:60]), reads[end - 60:end] + junk, F.comp_rev(reads[end - 60:end] + junk),
            reads[:60], reads[end - 60:end], reads[:23], last, reads[end - 40:end] + b"\n" + junk]
    ref = F.FindRef(small23_prefix, indices=ind, positions=pos)
    st = {}
    for s in seqs:
        ref.find(s, 3, 1, 0, st)
    assert st["bounds"] >= 4
    low = sum(1 for s in seqs for (a, _) in ref.proposals(s, 1) if a < 0)
    high = sum(1 for s in seqs for (a, _) in ref.proposals(s, 1) if a + len(s) > len(reads))
    assert low >= 2 and high >= 2
    ix.attach_aindex(ind, pos)
    try:
        for hd, step in ((0, 1), (3, 1), (3, 23), (60, 1)):
            want = F.find_csr(ref, seqs, hd, step)
            _same(ix.seq_find(seqs, hd, step), want)
        assert int(want[0][-1]) > 10 and 0 in want[1].tolist() and (end - 23) in want[1].tolist()
    finally:
        w._attached_key = None                                 # the mirror uploads its own arrays again on its next batch call


def test_switch_independence(acc, ref, pats):
    """6. Verification table on / off x absence filter on / off give identical arrays."""
    ix = acc._wrapper._attach_for_mapping()
    seqs = pats[:150]
    want = F.find_csr(ref, seqs, 3, 7)
    km = b"".join(p[:23] for p in seqs)
    ks = ix.kmer_strands(km)
    for table, filt in ((True, True), (True, False), (False, False), (False, True)):
        ix.set_bucket_table(table)
        ix.set_absence_filter(filt)
        try:
            got, k2 = ix.seq_find(seqs, 3, 7), ix.kmer_strands(km)
        finally:
            ix.set_bucket_table(True)
            ix.set_absence_filter(True)
        _same(got, want)
        _same(k2, ks)
    assert int(want[0][-1]) > 200


def test_strand_counts_and_analysis_functions(acc, ref, pats):
    """7. kmer_strands == the reduction of get_sequence_hits_array over the same k-mers; get_srandness, iter_reads_by_kmer and
    iter_reads_by_sequence == the restatement."""
    from aindex_amd import get_srandness, iter_reads_by_kmer, iter_reads_by_sequence
    ix = acc._wrapper._attach_for_mapping()
    kmers = F.strand_kmers(pats)
    sums = {}
    for m in (0, 2):
        off, _, _, _, _, flag = acc.get_sequence_hits_array(kmers, m)
        o = off.astype(np.int64)
        red = [[int(((flag[o[i]:o[i + 1]] & 3) == s).sum()) for i in range(len(kmers))] for s in (0, 1)]
        plus, minus, total = ix.kmer_strands(b"".join(kmers), m)
        assert plus.dtype == np.uint64 and plus.tolist() == red[0] and minus.tolist() == red[1] and total.tolist() == np.diff(o).tolist()
        assert [ref.strands(k, m) for k in kmers] == list(zip(plus.tolist(), minus.tolist(), total.tolist()))
        assert (plus + minus <= total).all()
        sums[m] = (int(plus.sum()), int(minus.sum()), int(total.sum()))
    # test_seqfind_cpu.py::test_input_conditions_of_the_gpu_tests pins these for the same k-mers under the restatement: without a cap
    # both strands have more than 100 hits; a cap of 2 lists at most 2 per k-mer, so fewer in all
    assert sums[0][0] > 100 and sums[0][1] > 100 and 0 < sums[2][2] < sums[0][2]
    assert acc.get_strandness_batch([k.decode() for k in kmers[:30]] + ["ACGT"]) == [ref.strands(k) for k in kmers[:30]] + [(0, 0, 0)]
    for k in [k for k in kmers if ref.strands(k)[2] > 0][:6]:      # chosen by the restatement: the first six k-mers with listed hits
        assert get_srandness(k.decode(), acc) == ref.strands(k)
        got = list(iter_reads_by_kmer(k.decode(), acc))
        assert got == ref.reads_by_kmer(k) and len(got) > 0
    n4 = n5 = 0
    for p in F.read_search_patterns(pats):
        got4, got5 = list(iter_reads_by_sequence(p.decode(), acc)), list(iter_reads_by_sequence(p.decode(), acc, hd=3))
        assert got4 == ref.reads_by_sequence(p) and got5 == ref.reads_by_sequence(p, 3)
        assert all(len(t) == 4 for t in got4) and all(len(t) == 5 for t in got5)
        n4, n5 = n4 + len(got4), n5 + len(got5)
    assert n5 > n4 > 0


def test_errors(gold, small23_prefix, tmp_path):
    """8. A 13-mer handle: AIX_ERR_MODE. Each missing attachment: AIX_ERR_ARG. The Python surface raises RuntimeError naming the piece."""
    from pf13 import pf13_path
    from aindex_amd.aindex import AIndex
    z = np.load(os.path.join(gold, "small23", "aindex.npz"))
    reads = open(small23_prefix + ".reads", "rb").read()
    ridx = np.loadtxt(small23_prefix + ".ridx", dtype=np.uint64).reshape(-1, 3)
    seqs = [reads[:150]]
    with Index.open_13(pf13_path(), None) as ix13:
        for call in (lambda: ix13.seq_find(seqs), lambda: ix13.kmer_strands(reads[:23])):
            with pytest.raises(_lib.AixError) as e:
                call()
            assert e.value.status == _lib.AIX_ERR_MODE
    with Index.open_23(small23_prefix + ".pf", small23_prefix + ".tf.bin", small23_prefix + ".kmers.bin") as ix:
        def both_fail():
            for call in (lambda: ix.seq_find(seqs), lambda: ix.kmer_strands(reads[:23])):
                with pytest.raises(_lib.AixError) as e:
                    call()
                assert e.value.status == _lib.AIX_ERR_ARG
        both_fail()                                            # nothing attached
        ix.attach_aindex(z["indices"], z["index"])
        both_fail()                                            # no intervals, no reads
        assert ix.attach_ridx(ridx)
        both_fail()                                            # no reads
        ix.attach_reads(reads)
        assert int(ix.seq_find(seqs)[0][-1]) > 0 and int(ix.kmer_strands(reads[:23])[2][0]) > 0
        ix.detach_reads()
        both_fail()
        ix.attach_reads(reads)
        ix.detach_aindex()                                     # drops the positions index and the intervals
        both_fail()
    ai = AIndex.load_from_prefix(small23_prefix)
    try:
        for call in (lambda: ai.find_sequences_array(["ACGT" * 10]), lambda: ai.find_reads_by_sequence_batch(["ACGT" * 10]),
                     lambda: ai.get_strandness_batch(["ACGT" * 5 + "ACG"])):
            with pytest.raises(RuntimeError, match="positions index"):
                call()
        w = ai._wrapper
        z["index"].tofile(str(tmp_path / "a.index.bin"))
        z["indices"].tofile(str(tmp_path / "a.indices.bin"))
        ai.load_aindex(str(tmp_path / "a.index.bin"), str(tmp_path / "a.indices.bin"), 100)
        with pytest.raises(RuntimeError, match=r"sorted \.ridx"):              # no intervals loaded
            ai.find_sequences_array(seqs)
        w.load_reads_index(small23_prefix + ".ridx")
        with pytest.raises(RuntimeError, match="needs the reads"):             # intervals on the device, no reads
            ai.get_strandness_batch([reads[:23]])
        w.load_reads(small23_prefix + ".reads")
        assert int(ai.find_sequences_array(seqs)[0][-1]) > 0                   # every piece there: an answer
        w._is_13mer_mode = True
        try:
            with pytest.raises(RuntimeError, match="23-mer index"):
                ai.find_sequences_array(seqs)
        finally:
            w._is_13mer_mode = False
    finally:
        ai._wrapper.close()
