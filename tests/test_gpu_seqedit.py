"""Sequences with substitutions, insertions and deletions against the indexed reads on the GPU (aix_seqedit.hip): alignments verified by a
banded edit-distance programme around the diagonal of every seed hit, against the restatement of seqedit_ref.py. Every comparison is exact
equality. test_seqedit_cpu.py checks on the CPU that the inputs used here give results of every kind."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import seqedit_ref as E
import seqfind_ref as F
from aindex_amd import _lib, synth
from aindex_amd.engine import Index


@pytest.fixture(scope="module")
def acc(gold, small23_prefix, tmp_path_factory):
    """The AIndex mirror over small23 with the positions files built by the GPU (the recipe of test_gpu_seqfind.py), reads and intervals loaded."""
    from aindex_amd.aindex import AIndex
    ai = AIndex.load_from_prefix(small23_prefix)
    prefix = str(tmp_path_factory.mktemp("seqe") / "acc")
    ai._wrapper.build_aindex(small23_prefix + ".reads", prefix)
    ai.load_aindex(prefix + ".index.bin", prefix + ".indices.bin", 100)
    ai.load_reads(small23_prefix + ".reads")
    yield ai
    ai._wrapper.close()


@pytest.fixture(scope="module")
def ref(small23_prefix):
    return E.EditRef(small23_prefix)


@pytest.fixture(scope="module")
def pats():
    return [p for p, _ in E.edit_patterns()]


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)


@pytest.mark.parametrize("ed", (0, 1, 2, 3, 7))
def test_standard_set(acc, ref, pats, ed):
    """1. The pattern set through Index.seq_edit: seed_step in {1, 7, 23} x max_per_kmer in {0, 1}; ed = 0 also equals Index.seq_find(hd = 0)."""
    ix = acc._wrapper._attach_for_mapping()
    n = 0
    for step in (1, 7, 23):
        for m in (0, 1):
            want = E.find_ed_csr(ref, pats, ed, step, m)
            got = ix.seq_edit(pats, ed, step, m)
            _same(got, want)
            n += int(want[0][-1])
            if ed == 0:
                f = ix.seq_find(pats, 0, step, m)
                lens = np.repeat(np.asarray([len(p) for p in pats], np.uint64), np.diff(f[0].astype(np.int64)))
                _same(got, (f[0], f[1], f[1] + lens, f[2], f[3], f[4], f[5]))
    assert n > 2000 and (ed == 0 or int((want[6] >= 1).sum()) > 50)


def test_surfaces(acc, ref, pats):
    """1. The array, str-list and list surfaces agree with the restatement; seed_step 0 means 23."""
    ix = acc._wrapper._attach_for_mapping()
    want = E.find_ed_csr(ref, pats, 3, 23, 0)
    got = acc.find_sequences_edit_array(pats, ed=3)
    _same(got, want)
    assert set(got[5].tolist()) == {0, 1} and set(got[6].tolist()) == {0, 1, 2, 3}
    _same(acc.find_sequences_edit_array([p.decode() for p in pats[:50]], 1, 7, 1), E.find_ed_csr(ref, pats[:50], 1, 7, 1))
    _same(ix.seq_edit(pats[:50], 2, 0), E.find_ed_csr(ref, pats[:50], 2, 23))                # seed_step 0 means 23
    _same(ix.seq_edit(pats[:50]), E.find_ed_csr(ref, pats[:50], 1, 23))                      # the defaults
    lists = acc.find_reads_by_sequence_edit_batch(pats[:80], ed=2)
    assert lists == [ref.reads_by_sequence_ed(p, 2) for p in pats[:80]] and sum(map(len, lists)) > 100
    assert all(len(t) == 6 and t[1] == t[3][0] and len(t[3]) >= 1 and len(t[4]) >= 1 for l in lists for t in l)


def test_shapes(acc, ref, pats):
    """2. M in {0, 1, 63, 64, 65, 257}; lengths 0, 22 and 23; a sequence at an odd offset; a 23-byte pattern last in the buffer; hit totals
    that are no multiples of 4 or 64; an all-empty batch."""
    ix = acc._wrapper._attach_for_mapping()
    memo = {}

    def want_of(seqs, ed, step):
        per = []
        for s in seqs:
            if (s, ed, step) not in memo:
                memo[(s, ed, step)] = ref.find_ed(s, ed, step)
            per.append(memo[(s, ed, step)])
        off = np.zeros(len(seqs) + 1, np.uint64)
        off[1:] = np.cumsum([len(p) for p in per], dtype=np.uint64)
        return off, [x for p in per for x in p]
    totals = set()
    for M in (0, 1, 63, 64, 65, 257):
        seqs = [pats[(7 * i) % len(pats)] if i % 9 else pats[i % len(pats)][: 20 + i % 6] for i in range(M)]
        got = ix.seq_edit(seqs, 2, 23)
        off, rows = want_of(seqs, 2, 23)
        assert np.array_equal(got[0], off) and list(zip(*[a.tolist() for a in got[1:]])) == rows and (M < 63 or len(rows) > 100)
        totals.add(sum(len(ref.proposals_ed(s, 23)) for s in seqs))
    assert any(t % 4 for t in totals) and any(t % 64 for t in totals)
    long = [p for p in pats if len(p) == 150]
    k23 = [p for p in pats if len(p) == 23 and ref.find_ed(p, 0)]
    odd = next(p[1:] for p in long if ref.find_ed(p[1:], 2, 1))  # chosen by the restatement: a pattern with answers at an odd offset
    seqs = [long[0], b"", long[1][:22], k23[0], odd, long[3], k23[1]]
    assert sum(map(len, seqs[:4])) % 2 == 1 and len(seqs[-1]) == 23
    got = ix.seq_edit(seqs, 2, 1)
    off, rows = want_of(seqs, 2, 1)
    assert np.array_equal(got[0], off) and list(zip(*[a.tolist() for a in got[1:]])) == rows
    nres = np.diff(off.astype(np.int64))
    assert nres[1] == 0 and nres[2] == 0 and nres[3] > 0 and nres[6] > 0 and nres[4] > 0
    assert ix.seq_edit([b"", b"", b""])[0].tolist() == [0, 0, 0, 0] and ix.seq_edit([])[0].tolist() == [0]
    ps = [_lib.vp() for _ in range(7)]                          # M = 0 without sequences or offsets: find_offsets = {0}
    _lib.check(_lib.lib().aix_seq_edit(ix._h, None, None, 0, 1, 23, 0, *[C.byref(p) for p in ps]), "aix_seq_edit")
    assert ix._take(ps[0], 1, np.uint64).tolist() == [0] and all(ix._take(p, 0, np.uint8).shape == (0,) for p in ps[1:])


BAND_LENGTHS = (23, 24, 63, 64, 65, 127, 128, 129, 255, 256, 257, 699, 700)


def _band_patterns(g, starts, ed):
    """[(pattern, kind)] for one ed: per length of BAND_LENGTHS a slice that read k % 40 holds whole (every second one reverse-complemented)
    with an inserted or deleted base in the last 4 rows; ed deleted bases in a row; ed inserted bases in a row; ed + 1 deleted bases in a
    row. Then, per read of a few, patterns that start at its byte 0 and end at its last byte (the band is clipped by lo and by hi), with
    an indel near the clipped end, and the whole read with ed and with ed + 1 junk bytes around it."""
    out = []
    for k, L in enumerate(BAND_LENGTHS):
        for kind in ("tail", "dels", "inss", "over"):
            if kind == "tail":
                ops = [("ID"[k % 2], L - 1 - k % 4)]
            elif kind == "over":
                ops = [("D", L // 2 + t) for t in range(ed + 1)]
            else:
                ops = [("D" if kind == "dels" else "I", L // 2 + (t if kind == "dels" else 0)) for t in range(ed)]
            src = L - sum(1 for o in ops if o[0] == "I") + sum(1 for o in ops if o[0] == "D")
            if src > 700 or src < 1:
                continue
            ops = [(o, min(j, src - 1)) for o, j in ops]
            s = starts[k % 40] + (700 - src) * (k % 3) // 2
            p = E.plant_edits(g[s:s + src], ops)
            if kind == "inss":                                 # plant_edits puts the bases before one byte in reverse order: any order serves
                assert len(p) == L
            out.append((F.comp_rev(p) if k % 2 else p, kind))
    return out


@pytest.mark.parametrize("ed", (1, 2, 7))
def test_band_edges(small23_prefix, ed):
    """3. A second index on the device: 40 reads of 700 bytes cut from the same genome, half of them reverse-complemented (the recipe of
    test_long_reads_trip_boundaries), every eighth read left out of the intervals so that its hits have none. Pattern lengths on, below
    and above the multiples of the four rows a dword of the pattern feeds, up to the whole read. An indel in the last 4 rows only: the
    early exit must not fire before it. ed deletions / insertions in a row: the path rides the band's edge. ed + 1 edits: never found.
    Alignments from a read's byte 0 and to its last byte, the band clipped by lo / hi; a pattern longer than the read by ed (found with
    dist = ed) and by ed + 1 (not found). ed in {1, 2, 7}."""
    g = synth.genome_ascii(1, 3000).tobytes()
    rng = np.random.default_rng(11)
    starts = rng.integers(0, 2300, 40).tolist()
    rs = [g[s:s + 700] if i % 2 == 0 else F.comp_rev(g[s:s + 700]) for i, s in enumerate(starts)]
    reads = b"\n".join(rs) + b"\n"
    ridx = np.asarray([(i, 701 * i, 701 * i + 700) for i in range(40) if i % 8 != 5], np.uint64)
    with Index.open_23(small23_prefix + ".pf", small23_prefix + ".tf.bin", small23_prefix + ".kmers.bin") as ix:
        ind, pos = ix.positions_fill(reads)
        ix.attach_aindex(ind, pos)
        assert ix.attach_ridx(ridx)
        ix.attach_reads(reads)
        ref = E.EditRef(small23_prefix, indices=ind, positions=pos, reads=reads, ridx=ridx)
        items = _band_patterns(g, starts, ed)
        junk = b"ACGTTGCAAC"
        for i in (0, 3, 6, 39):                            # reads that the intervals hold; 3 and 39 are stored reverse-complemented
            r = rs[i]
            for L in (64, 129, 699):
                items += [(r[:L], "first"), (r[700 - L:], "last"), (E.plant_edits(r[:L], [("D", 2)]), "first-d"),
                          (E.plant_edits(r[700 - L:], [("I", L - 2)]), "last-i"), (junk[:ed] + r[:L], "before"), (r[700 - L:] + junk[:ed], "behind")]
            for e1 in (0, ed // 2, ed):
                items += [(junk[:e1] + r + junk[e1:ed], "whole"), (junk[:e1] + r + junk[e1:ed + 1], "whole-over")]
        seqs = [p for p, _ in items]
        st = {}
        per = [ref.find_ed(p, ed, 7, 0, st) for p in seqs]           # what the assertions below look at: seed_step 7
        _same(ix.seq_edit(seqs, ed, 23), E.find_ed_csr(ref, seqs, ed, 23))
        _same(ix.seq_edit(seqs, ed, 7), E.find_ed_csr(ref, seqs, ed, 7))
        by = {}
        for (p, kind), res in zip(items, per):
            by.setdefault(kind, []).append((len(p), res))
        assert all(not res for _, res in by["over"] + by["whole-over"])                  # ed + 1 edits: never found
    # a pattern longer than the read by exactly ed: found with dist = ed over the whole read, every one of them
    assert all(any(x[5] == ed and x[1] - x[0] == 700 for x in res) for _, res in by["whole"]) and len(by["whole"]) == 12
    # the positions index built here lists a part of the occurrences (its buckets are as long as the golden tf), so a single short
    # pattern may find nothing: each other kind must show its case on more than half of its patterns that kept a seed
    def most(kinds, pred, least=23):
        rows = [(n, res) for kind in kinds for n, res in by[kind] if n - (ed if kind == "inss" else 0) > least + 23]
        return len(rows) > 0 and 2 * sum(1 for n, res in rows if any(pred(n, x) for x in res)) > len(rows)
    assert most(("tail",), lambda n, x: x[5] == 1 and abs(x[1] - x[0] - n) == 1)
    assert most(("dels",), lambda n, x: x[5] == ed and x[1] - x[0] == n + ed)
    assert most(("inss",), lambda n, x: x[5] == ed and x[1] - x[0] == n - ed)
    assert most(("first", "first-d", "before"), lambda n, x: x[3] == 0)
    assert most(("last", "last-i", "behind"), lambda n, x: x[1] % 701 == 700)
    assert most(("before", "behind"), lambda n, x: x[5] == ed and (x[3] == 0 or x[1] % 701 == 700))
    assert st["no_interval"] > 20 and st["rejected"] > 20 and {x[4] for res in per for x in res} == {0, 1}


def test_self_similar_text(small23_prefix):
    """3. Overlapping records of one read and strand with different starts (seqedit_ref.self_similar_case: a read that repeats a 30-mer
    of the genome, patterns of two and more copies): the arrays keep every start. ed in {0, 1, 2}, seed_step 1 and 7."""
    reads, ridx, seqs = E.self_similar_case(E.EditRef(small23_prefix))
    with Index.open_23(small23_prefix + ".pf", small23_prefix + ".tf.bin", small23_prefix + ".kmers.bin") as ix:
        ind, pos = ix.positions_fill(reads)
        ix.attach_aindex(ind, pos)
        assert ix.attach_ridx(ridx)
        ix.attach_reads(reads)
        ref = E.EditRef(small23_prefix, indices=ind, positions=pos, reads=reads, ridx=ridx)
        for ed in (0, 1, 2):
            for step in (1, 7):
                want = E.find_ed_csr(ref, seqs, ed, step)
                _same(ix.seq_edit(seqs, ed, step), want)
            res = [ref.find_ed(p, ed, 1) for p in seqs]
            pairs = [sum(1 for i, x in enumerate(r) for z in r[i + 1:] if z[2] == x[2] and z[4] == x[4] and z[0] != x[0] and z[0] < x[1]) for r in res]
            assert all(pairs[i] > 0 for i in range(4) if i != 1 or ed) and pairs[4] == 0


def test_dev_twin(acc, ref, pats):
    """4. aix_seq_edit_dev with cap = 0, total - 1 (canaries intact) and total; the torch surface with cap_hint in {0, 5, total + 7}; empty input."""
    import torch
    ix = acc._wrapper._attach_for_mapping()
    seqs = pats[:120]
    want = E.find_ed_csr(ref, seqs, 3, 23)
    h = ix.seq_edit(seqs, 3, 23)
    _same(h, want)
    data = torch.frombuffer(bytearray(b"".join(seqs)), dtype=torch.uint8).cuda()
    offs = torch.tensor(np.concatenate([[0], np.cumsum([len(s) for s in seqs])]), dtype=torch.int64).cuda()
    for hint in (0, 5, len(want[1]) + 7):
        for a, b in zip(ix.seq_edit_t(data, offs, 3, 23, cap_hint=hint), h):
            assert np.array_equal(a.cpu().numpy().view(b.dtype), b)
    L, vp, M = _lib.lib(), _lib.vp, len(seqs)
    st = vp(torch.cuda.current_stream().cuda_stream)
    total = len(want[1])
    assert total > 200
    for cap in (0, total - 1, total):
        o = torch.full((M + 1,), -1, dtype=torch.int64).cuda()
        outs = [torch.full((total + 8,), 0x5A, dtype=dt).cuda() for dt in (torch.int64, torch.int64, torch.int64, torch.int64, torch.uint8, torch.int32)]
        tot = C.c_uint64(12345)
        _lib.check(L.aix_seq_edit_dev(ix._h, vp(data.data_ptr()), vp(offs.data_ptr()), M, 3, 23, 0, vp(o.data_ptr()), *[vp(t.data_ptr()) if cap else None for t in outs],
                                      cap, C.byref(tot), st), "aix_seq_edit_dev")
        assert tot.value == total and np.array_equal(o.cpu().numpy().view(np.uint64), want[0])
        for t, w in zip(outs, want[1:]):
            a = t.cpu().numpy()
            if cap == total:
                assert np.array_equal(a[:total].view(w.dtype), w) and (a[total:] == 0x5A).all()
            else:
                assert (a == 0x5A).all()
    e_off = torch.zeros(4, dtype=torch.int64, device="cuda")
    et = ix.seq_edit_t(torch.empty(0, dtype=torch.uint8, device="cuda"), e_off, 3)
    assert et[0].tolist() == [0, 0, 0, 0] and et[1].numel() == 0 and len(et) == 7


def test_hits_at_the_edges_of_the_reads(acc, small23_prefix):
    """5. Hits planted at the first and the last 23 bytes of the reads (the recipe of test_gpu_seqfind.py): patterns that overhang the
    first byte and the last by up to ed + 3 have their bands clipped at lo / hi; the answers are the restatement's. Answers only: the
    kernel stays in bounds by its own logic."""
    w = acc._wrapper
    ix = w._attach_for_mapping()
    reads = open(small23_prefix + ".reads", "rb").read()
    ind, pos = np.asarray(w._indices).copy(), np.asarray(w._positions).copy()
    base = E.EditRef(small23_prefix)
    end = len(reads) - 1                                       # the file ends with a newline
    first, last = reads[:23], reads[end - 23:end]
    for kmer, at in ((first, 0), (last, end - 23)):
        h = base.bucket(kmer)
        assert h is not None and ind[h + 1] > ind[h]
        pos[int(ind[h])] = at + 1
    junk = b"ACGTTGCAAC"
    ref = E.EditRef(small23_prefix, indices=ind, positions=pos)
    ix.attach_aindex(ind, pos)
    try:
        for ed in (1, 3, 7):
            seqs = []
            for n in range(ed + 4):                            # overhangs of 0 .. ed + 3 bytes
                head, tail = junk[:n] + reads[:60], reads[end - 60:end] + junk[:n]
                seqs += [head, F.comp_rev(head), tail, F.comp_rev(tail)]
            seqs += [reads[:23], last, reads[end - 40:end] + b"\n" + junk]
            low = sum(1 for s in seqs for (a, _, _) in ref.proposals_ed(s, 1) if a < 0)
            high = sum(1 for s in seqs for (a, _, _) in ref.proposals_ed(s, 1) if a + len(s) > len(reads))
            assert low >= 2 and high >= 2
            for step in (23, 1):
                want = E.find_ed_csr(ref, seqs, ed, step)
                _same(ix.seq_edit(seqs, ed, step), want)
            off = want[0].astype(np.int64).tolist()
            for n in range(ed + 4):                            # at the file's ends (seed_step 1): found while ed pays for the overhang, never beyond
                for j in range(4):
                    lo, hi = off[4 * n + j], off[4 * n + j + 1]
                    at_edge = (want[1][lo:hi] == 0) if j < 2 else (want[2][lo:hi] == end)
                    assert bool((at_edge & (want[5][lo:hi] == j % 2)).any()) == (n <= ed)
            assert 0 in want[1].tolist() and end in want[2].tolist()
    finally:
        w._attached_key = None                                 # the mirror uploads its own arrays again on its next batch call


def test_switch_independence(acc, ref, pats):
    """6. Verification table on / off x absence filter on / off give identical arrays."""
    ix = acc._wrapper._attach_for_mapping()
    seqs = pats[:150]
    want = E.find_ed_csr(ref, seqs, 3, 7)
    for table, filt in ((True, True), (True, False), (False, False), (False, True)):
        ix.set_bucket_table(table)
        ix.set_absence_filter(filt)
        try:
            got = ix.seq_edit(seqs, 3, 7)
        finally:
            ix.set_bucket_table(True)
            ix.set_absence_filter(True)
        _same(got, want)
    assert int(want[0][-1]) > 200


def test_errors(gold, small23_prefix, tmp_path):
    """7. ed = 8: AIX_ERR_ARG. A 13-mer handle: AIX_ERR_MODE. Each missing attachment: AIX_ERR_ARG. The Python surface raises RuntimeError
    naming the piece."""
    from pf13 import pf13_path
    from aindex_amd.aindex import AIndex
    z = np.load(os.path.join(gold, "small23", "aindex.npz"))
    reads = open(small23_prefix + ".reads", "rb").read()
    ridx = np.loadtxt(small23_prefix + ".ridx", dtype=np.uint64).reshape(-1, 3)
    seqs = [reads[:150]]
    with Index.open_13(pf13_path(), None) as ix13:
        with pytest.raises(_lib.AixError) as e:
            ix13.seq_edit(seqs)
        assert e.value.status == _lib.AIX_ERR_MODE
    with Index.open_23(small23_prefix + ".pf", small23_prefix + ".tf.bin", small23_prefix + ".kmers.bin") as ix:
        def fails():
            with pytest.raises(_lib.AixError) as e:
                ix.seq_edit(seqs)
            assert e.value.status == _lib.AIX_ERR_ARG
        fails()                                                # nothing attached
        ix.attach_aindex(z["indices"], z["index"])
        fails()                                                # no intervals, no reads
        assert ix.attach_ridx(ridx)
        fails()                                                # no reads
        ix.attach_reads(reads)
        assert int(ix.seq_edit(seqs)[0][-1]) > 0 and int(ix.seq_edit(seqs, _lib.SEQEDIT_MAX_ED)[0][-1]) > 0
        for bad in (_lib.SEQEDIT_MAX_ED + 1, 100):
            with pytest.raises(_lib.AixError) as e:
                ix.seq_edit(seqs, bad)
            assert e.value.status == _lib.AIX_ERR_ARG
        ix.detach_reads()
        fails()
        ix.attach_reads(reads)
        ix.detach_aindex()                                     # drops the positions index and the intervals
        fails()
    ai = AIndex.load_from_prefix(small23_prefix)
    try:
        for call in (lambda: ai.find_sequences_edit_array(["ACGT" * 10]), lambda: ai.find_reads_by_sequence_edit_batch(["ACGT" * 10])):
            with pytest.raises(RuntimeError, match="positions index"):
                call()
        w = ai._wrapper
        z["index"].tofile(str(tmp_path / "a.index.bin"))
        z["indices"].tofile(str(tmp_path / "a.indices.bin"))
        ai.load_aindex(str(tmp_path / "a.index.bin"), str(tmp_path / "a.indices.bin"), 100)
        with pytest.raises(RuntimeError, match=r"sorted \.ridx"):              # no intervals loaded
            ai.find_sequences_edit_array(seqs)
        w.load_reads_index(small23_prefix + ".ridx")
        with pytest.raises(RuntimeError, match="needs the reads"):             # intervals on the device, no reads
            ai.find_sequences_edit_array(seqs)
        w.load_reads(small23_prefix + ".reads")
        assert int(ai.find_sequences_edit_array(seqs)[0][-1]) > 0              # every piece there: an answer
        w._is_13mer_mode = True
        try:
            with pytest.raises(RuntimeError, match="23-mer index"):
                ai.find_sequences_edit_array(seqs)
        finally:
            w._is_13mer_mode = False
    finally:
        ai._wrapper.close()
