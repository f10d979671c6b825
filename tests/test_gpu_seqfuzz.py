"""Differential fuzzing of the sequence-search chain (aix_seqhits.hip, aix_seqfind.hip, aix_seqedit.hip): random small indexes with dirty
bytes in reads and patterns, every seed_step of seqfuzz_cases.steps(), hostile positions and intervals behind k_sh_hits<false>, and a reads
buffer beyond 4 GiB, against the restatements (seqhits_ref / seqfind_ref / seqedit_ref) and the brute-force searches that know nothing of
seeds, bands or DPP. Every comparison is exact equality of dtype and content. test_seqfuzz_cpu.py shows on the CPU that the cases give
answers of every kind, so nothing here passes on empty arrays."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import seqedit_ref as E
import seqfind_ref as F
import seqfuzz_cases as S
import seqhits_ref as R
from aindex_amd.engine import Index
from test_gpu_fuzz import _seeds


def _same(got, want, tag=None):
    assert len(got) == len(want), tag
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and np.array_equal(g, w), (tag, "column", i)


def _open(case):
    return Index.open_23(case[0] + ".pf", case[0] + ".tf.bin", case[0] + ".kmers.bin")


def _attach(ix, indices, positions, ridx, reads=None):
    ix.attach_aindex(indices, positions)
    assert ix.attach_ridx(ridx)
    if reads is not None:
        ix.attach_reads(reads)


def _rows(arrs, i):
    """the records of sequence i of a CSR answer as tuples"""
    lo, hi = int(arrs[0][i]), int(arrs[0][i + 1])
    return list(zip(*[a[lo:hi].tolist() for a in arrs[1:]]))


def _windows(pats):
    return [p[q:q + 23] for p in pats for q in range(len(p) - 22)]


def _strands(ref, kmers, m):
    cols = list(zip(*[ref.strands(k, m) for k in kmers]))
    return tuple(np.asarray(c, np.uint64) for c in cols)


@pytest.mark.parametrize("seed", _seeds(S.N_SEEDS))
def test_fuzz_chain(seed, tmp_path):
    """One random case per seed (seqfuzz_cases.make_case: canonical / both strands stored / as-met index; reads with N n a c g t ~ CR 0x00
    0x80 0xFF planted, overlapping, a third reverse-complemented, every seventh without an interval; clean, dirty and short patterns).
    seq_hits / seq_votes (max_per_kmer 0, 2, 3; min_votes 1, 2), seq_find (hd 0, 1, 3) and seq_edit (ed 0, 1, 2, 7) at the seed's seed_step
    (1, 2, 5, 22, 23, 24, 47, Lmax - 23, Lmax - 22, 10^6, 2^32, 2^63 + 1 over the twelve seeds) and max_per_kmer 0, 2, 7, and kmer_strands of
    every window of ten patterns == the restatements. On the clean patterns, max_per_kmer 0, seed_step 1 and 23: seq_find(hd) == F.brute
    record for record and seq_edit(ed) reduced to {(rid, strand): min dist} == E.brute_ed, for hd / ed < len // 23 - dead seeds
    (seqfuzz_cases.dead_seeds: windows whose occurrences an as-met index does not list; none in the canonical cases), on the reads
    without an N — the header's completeness guarantees. Seeds 1 and 7 (mod 6 == 1): one seq_find and one seq_edit call again under
    verification table on / off x absence filter on / off.
    First to run on the device: k_sh_windows / k_sh_resolve / k_sh_hits with a window stride other than 1, 7, 23 (the division and the two
    multiplications by step, up to 2^63 + 1); sf_comp and the bswap / >> 24 of both verification kernels on bytes outside ACGTN; the N
    rule with the N on the read side; max_per_kmer 2, 3, 7 behind the searches; all of it on indexes other than small23."""
    case = S.make_case(seed, str(tmp_path))
    ref = S.make_ref(case)
    pats = [p for p, _ in case[5]]
    step = S.step_of(seed, case[5])
    with _open(case) as ix:
        _attach(ix, case[3], case[4], case[2], case[1])
        for m in (0, 2, 3):
            _same(ix.seq_hits(pats, m), R.hits_csr(ref, pats, m), ("hits", seed, m))
            for mv in (1, 2):
                _same(ix.seq_votes(pats, mv, m), R.votes_csr(ref, pats, mv, m), ("votes", seed, mv, m))
        n = 0
        for m in (0, 2, 7):
            for hd in (0, 1, 3):
                want = F.find_csr(ref, pats, hd, step, m)
                _same(ix.seq_find(pats, hd, step, m), want, ("find", seed, hd, step, m))
                n += int(want[0][-1])
            for ed in (0, 1, 2, 7):
                want = E.find_ed_csr(ref, pats, ed, step, m)
                _same(ix.seq_edit(pats, ed, step, m), want, ("edit", seed, ed, step, m))
                n += int(want[0][-1])
        assert n > 300
        kmers = _windows(pats[3::6])
        for m in (0, 3):
            _same(ix.kmer_strands(b"".join(kmers), m), _strands(ref, kmers, m), ("strands", seed, m))
        # the independent references
        skip = S.n_reads_of(ref)
        clean = [p for p, kind in case[5] if kind == "clean"]
        top = {p: len(p) // 23 - S.dead_seeds(ref, p) for p in clean}
        table = {p: ref.brute_ed(p, 2) for p in clean if top[p] > 0}
        brute = {}
        checked = 0
        for d in (0, 1, 3):
            some = [p for p in clean if d < top[p]]
            for p in some:
                brute[(p, d)] = [r for r in ref.brute(p, d) if r[1] not in skip]
            for st in (1, 23):
                got = ix.seq_find(some, d, st, 0)
                for i, p in enumerate(some):
                    assert [r for r in _rows(got, i) if r[1] not in skip] == brute[(p, d)], ("find against the full Hamming search", seed, len(p), d, st)
                    checked += 1
        for d in (0, 1, 2):
            some = [p for p in clean if d < top[p]]
            for st in (1, 23):
                got = ix.seq_edit(some, d, st, 0)
                for i, p in enumerate(some):
                    have = {}
                    for s, e, rid, local, strand, dist in _rows(got, i):
                        if rid not in skip:
                            have[(rid, strand)] = min(have.get((rid, strand), 99), dist)
                    assert have == {k: v for k, v in table[p].items() if v <= d and k[0] not in skip}, ("edit against the unbanded search", seed, len(p), d, st)
                    checked += 1
        assert checked > 150
        if seed % 6 == 1:
            wf, we = F.find_csr(ref, pats, 3, step, 0), E.find_ed_csr(ref, pats, 2, step, 0)
            try:
                for table_on, filt in ((True, False), (False, False), (False, True), (True, True)):
                    ix.set_bucket_table(table_on)
                    ix.set_absence_filter(filt)
                    _same(ix.seq_find(pats, 3, step, 0), wf, ("find", seed, "table", table_on, "filter", filt))
                    _same(ix.seq_edit(pats, 2, step, 0), we, ("edit", seed, "table", table_on, "filter", filt))
            finally:
                ix.set_bucket_table(True)
                ix.set_absence_filter(True)


def test_hostile_attachments(tmp_path):
    """seq_find, seq_edit and kmer_strands on seed 1's case with a hostile positions copy and a hostile interval table
    (seqfuzz_cases.hostile_case; test_seqfuzz_cpu.test_hostile_case shows that every planted kind is read and every odd interval decides a
    proposal). The answers are the restatements' on the same arrays. Answers only: each planted kind stays in bounds by these guards.
      zeros                                    aix_posquery.hip:160-163, k_pq_flat keeps entries with v != 0 only: a zero never becomes a hit
      entries into the last 1, 2, 11, 22       aix_seqhits.hip:112, sh_read23 `p > size || size - p < 23`: the reads are not touched and the
      bytes, len + 1, len + 6, 2^40            flag is 2 (:136-140); k_sf_verify (aix_seqfind.hip:64) and k_se_verify (aix_seqedit.hip:80)
                                               take up hits with strand < 2 only, so every hit they see has pos + 23 <= reads_len
      an entry at a newline                    inside the buffer: sh_read23 reads its 23 bytes (aix_seqhits.hip:113-119), they equal no
                                               pattern window, flag 2
      an interval that ends beyond the reads   k_sf_verify: aix_seqfind.hip:75 tests a + L against reads_len before any interval;
                                               k_se_verify: aix_seqedit.hip:104 clips hi with min(en, reads_len)
      an empty interval, a 23-byte interval,   k_sf_verify: aix_seqfind.hip:85 `en >= a && en - a >= L`; k_se_verify: aix_seqedit.hip:99
      a read split inside a seed window        `en >= p && en - p >= 23`, then lo / hi (:103-104) bound the columns
    Behind all of them every load of the reads in both verification kernels goes through sf_load4 (aix_seqhits.hpp:94-108), which touches
    no byte outside [0, size): aix_seqfind.hip:106, aix_seqedit.hip:134.
    First to run on the device: k_sh_hits<false> on positions in the last 22 bytes, past the end, at 2^40 and at a newline; the guards of
    k_sf_verify and k_se_verify named above on intervals that end beyond the reads, are empty, hold 23 bytes or cut a seed."""
    case = S.make_case(1, str(tmp_path))
    ind, pos, ridx, items, info = S.hostile_case(case)
    pats = [p for p, _ in items]
    ref = S.make_ref(case, indices=ind, positions=pos, ridx=ridx)
    with _open(case) as ix:
        _attach(ix, ind, pos, ridx, case[1])
        n = 0
        for step in (1, 23):
            for hd in (0, 3):
                want = F.find_csr(ref, pats, hd, step)
                _same(ix.seq_find(pats, hd, step), want, ("find", hd, step))
                n += int(want[0][-1])
            for ed in (1, 2) + ((7,) if step == 23 else ()):
                want = E.find_ed_csr(ref, pats, ed, step)
                _same(ix.seq_edit(pats, ed, step), want, ("edit", ed, step))
                n += int(want[0][-1])
        print("records compared", n)
        assert n > 100
        kmers = _windows(pats[3::4])
        for m in (0, 3):
            want = _strands(ref, kmers, m)
            _same(ix.kmer_strands(b"".join(kmers), m), want, ("strands", m))
            assert int(want[2].sum()) > int(want[0].sum() + want[1].sum())     # hits that are neither strand: the planted ones among them


def test_search_beyond_4gib(tmp_path):
    """Seed 2's case in a borrowed device buffer of 2^32 + 2^20 newlines, its reads image copied in at D = 2^31 - h - r (r = 0, 1) and
    2^32 - h - r (r = 2, 3), h the middle of a read near the image's middle: both boundaries fall inside a read and the four dword
    alignments of sf_load4 occur. Positions (the non-zero entries) and interval starts / ends are raised by D. The answers are those of
    the unshifted case (the restatement == the GPU at shift 0) with pos / start / end raised by D and rid, local, strand, dist, votes and
    offsets unchanged (seq_hits reports a hit without an interval with start 0, so the local of such a hit is its position and rises too): seq_hits, seq_votes, seq_find (hd 2, step 7), seq_edit (ed 2 at step 1 and ed 7 at step 23 against the restatement;
    ed 2 at step 23 and ed 7 at step 1 against the GPU at shift 0). The filler cannot matter: every byte the kernels may read lies inside
    an interval or within the 23 bytes at a listed position, and every listed position is an occurrence inside a read.
    First to run on the device: every kernel of the chain with positions, starts and flat read offsets above 2^31 and 2^32; the sort
    widths sv_bits((rd_len << 1) | 1) of sf_run and sv_bits((rd_len << 9) | 0x1FF) of se_run with keys of 34 and 42 bits that differ
    in their top bits only."""
    import torch
    case = S.make_case(2, str(tmp_path))
    prefix, reads, ridx, indices, positions, items = case
    pats = [p for p, _ in items]
    ref = S.make_ref(case)
    h = S.beyond_offset(case)
    n = len(reads)
    want = {"hits": R.hits_csr(ref, pats, 0), "votes": R.votes_csr(ref, pats, 1, 0), "find": F.find_csr(ref, pats, 2, 7),
            "edit21": E.find_ed_csr(ref, pats, 2, 1), "edit723": E.find_ed_csr(ref, pats, 7, 23)}

    def run(ix):
        return {"hits": ix.seq_hits(pats, 0), "votes": ix.seq_votes(pats, 1, 0), "find": ix.seq_find(pats, 2, 7), "edit21": ix.seq_edit(pats, 2, 1),
                "edit723": ix.seq_edit(pats, 7, 23), "edit223": ix.seq_edit(pats, 2, 23), "edit71": ix.seq_edit(pats, 7, 1)}
    raised = {"hits": (2,), "votes": (), "find": (1,), "edit21": (1, 2), "edit723": (1, 2), "edit223": (1, 2), "edit71": (1, 2)}
    size = (1 << 32) + (1 << 20)
    buf = torch.full((size,), 10, dtype=torch.uint8, device="cuda")
    image = torch.frombuffer(bytearray(reads), dtype=torch.uint8).cuda()
    try:
        with _open(case) as ix:
            _attach(ix, indices, positions, ridx, reads)
            base = run(ix)
            for k, w in want.items():
                _same(base[k], w, ("shift 0", k))
            assert all(int(v[0][-1]) > 100 for v in base.values())
            ix.attach_reads_t(buf)
            assert ix.reads_info() == (2, size)
            for edge, r in ((1 << 31, 0), (1 << 31, 1), (1 << 32, 2), (1 << 32, 3)):
                D = edge - h - r
                assert D % 4 == (-h - r) % 4 and D + n < size
                buf[D:D + n] = image
                pos2, ridx2 = np.asarray(positions).copy(), np.asarray(ridx).copy()
                pos2[pos2 != 0] += np.uint64(D)
                ridx2[:, 1:] += np.uint64(D)
                _attach(ix, indices, pos2, ridx2)
                got = run(ix)
                for k, b in base.items():
                    moved = tuple(c + np.uint64(D) if i in raised[k] else c for i, c in enumerate(b))
                    if k == "hits":                            # a hit without an interval has start 0: its local is its position
                        moved = moved[:4] + (np.where(b[5] & 4, b[4], b[4] + np.int64(D)),) + moved[5:]
                    _same(got[k], moved, ("shift", D, k))
                f, e = got["find"], got["edit21"]
                lens = np.repeat(np.asarray([len(p) for p in pats], np.uint64), np.diff(f[0].astype(np.int64)))
                across = (int(((f[1] < edge) & (f[1] + lens > edge)).sum()), int(((e[1] < edge) & (e[2] > edge)).sum()),
                          int(((got["edit723"][1] < edge) & (got["edit723"][2] > edge)).sum()))
                print("shift", D, "alignment", D % 4, "records across the boundary: find, edit", across)
                assert all(a >= 1 for a in across)
                buf[D:D + n] = 10
            ix.detach_reads()
    finally:
        del buf
        torch.cuda.empty_cache()
