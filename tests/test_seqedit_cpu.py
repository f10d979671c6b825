"""The restatement of the edit-distance search (seqedit_ref.py) on the CPU: ed = 0 against the Hamming restatement, the seeded and banded
search against an unbanded semi-global Levenshtein search over all reads, the conditions on the inputs of the GPU tests
(test_gpu_seqedit.py), so that those cannot pass on empty answers, and the host-side edit_distance. Every comparison is exact equality."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import seqedit_ref as E
import seqfind_ref as F


@pytest.fixture(scope="module")
def ref(small23_prefix):
    return E.EditRef(small23_prefix)


@pytest.fixture(scope="module")
def pats():
    return E.edit_patterns()


def test_surface_exists():
    """The public names of the feature: AIndex and Index methods, library symbols declared and exported, the constant mirrored."""
    from aindex_amd import _lib
    from aindex_amd.aindex import AIndex, edit_distance
    from aindex_amd.engine import Index
    assert callable(edit_distance)
    for name in ("find_sequences_edit_array", "find_reads_by_sequence_edit_batch"):
        assert callable(getattr(AIndex, name))
    for name in ("seq_edit", "seq_edit_t"):
        assert callable(getattr(Index, name))
    L = _lib.lib()
    for name in ("aix_seq_edit", "aix_seq_edit_dev"):
        assert hasattr(L, name) and name in _lib.SIGNATURES and name in _lib.header_symbols()
    assert _lib.SEQEDIT_MAX_ED == E.MAX_ED == 7
    assert "#define AIX_SEQEDIT_MAX_ED 7u" in open(os.path.join(_lib.CSRC, "aix_seqhits.hpp")).read()


def test_ed0_is_the_hamming_search_at_hd0(ref):
    """1. With ed = 0 the band is one diagonal: the records are those of FindRef.find(hd = 0) with start = a and end = a + L."""
    n = 0
    for p, _ in F.standard_patterns():
        for step, m in ((23, 0), (1, 0), (7, 1)):
            want = [(a, a + len(p), rid, local, strand, d) for a, rid, local, strand, d in ref.find(p, 0, step, m)]
            assert ref.find_ed(p, 0, step, m) == want
            n += len(want)
    assert n > 1000


def test_hand_written_cases(ref):
    """The rules one by one on a read of the golden set: an inserted and a deleted base, the ends of the read, the tie-breaks."""
    i = next(k for k, (s, e) in enumerate(zip(ref.start, ref.end)) if e + 23 < 51612 and e - s >= 150 and b"N" not in ref.reads[s:e])
    s0, rid, r = ref.start[i], ref.rid[i], ref.reads[ref.start[i]:ref.end[i]]
    me = lambda res: [x for x in res if x[2] == rid and x[4] == 0]
    pat = r[10:110]
    assert me(ref.find_ed(pat, 1)) == [(s0 + 10, s0 + 110, rid, 10, 0, 0)]
    # a base deleted from the pattern at 50: the text is one longer than the pattern. Seeds 0 and 23 sit on the diagonal of the start;
    # seeds 46 and 69 (pattern offsets) on the next one, whose band sees the same alignment: one record, not two, when the starts agree
    dele = E.plant_edits(pat, [("D", 50)])
    got = me(ref.find_ed(dele, 1))
    assert (s0 + 10, s0 + 110, rid, 10, 0, 1) in got and all(x[5] == 1 for x in got) and me(ref.find_ed(dele, 0)) == []
    assert me(ref.find(dele, 3)) == []                         # the Hamming search misses it at any hd the pattern could bear
    # a base inserted into the pattern: the text is one shorter
    ins = E.plant_edits(pat, [("I", 50)])
    got = me(ref.find_ed(ins, 1))
    assert (s0 + 10, s0 + 110, rid, 10, 0, 1) in got and len(ins) == 101
    # the pattern overhangs the read's first byte by one: the band is clipped at lo = start, one deletion pays for the byte
    over = b"T" + r[:60] if r[0:1] != b"T" else b"G" + r[:60]
    assert (s0, s0 + 60, rid, 0, 0, 1) in me(ref.find_ed(over, 1)) and me(ref.find_ed(over, 0)) == []
    # and its last byte
    tail = r[90:150] + (b"T" if r[149:150] != b"T" else b"G")
    assert (s0 + 90, s0 + 150, rid, 90, 0, 1) in me(ref.find_ed(tail, 1))
    # reverse strand
    rc = F.comp_rev(dele)
    assert (s0 + 10, s0 + 110, rid, 10, 1, 1) in [x for x in ref.find_ed(rc, 1) if x[2] == rid]
    # shorter than 23: no seeds; the bound on ed
    assert ref.find_ed(pat[:22], 3) == []
    with pytest.raises(AssertionError):
        ref.find_ed(pat, 8)
    assert E.lev(b"kitten", b"sitting") == 3 and E.lev(b"ANGT", b"ACGA", True) == 1 and E.lev(b"ANGT", b"ACGA") == 2


def test_complete_against_the_unbanded_search(ref, pats, small23_prefix):
    """2. On an index that lists every occurrence (seqedit_ref.full_index; the golden positions array lists a part of them), for every
    pattern of edit_patterns(), seed_step 1 and 23, max_per_kmer 0, and every ed < L // 23 - u: the smallest distance per (rid, strand) of
    find_ed equals brute_ed, on the reads without an N. u counts the 23-windows at offsets 0, 23, .. of the pattern that no edit touched
    (the window, or its reverse complement, is a piece of the genome) and that the index still does not hold (a k-mer outside the golden
    k-mer set), and the window with the N: the header asks for ed + 1 disjoint seed windows listed in full, at most ed of the L // 23 can
    be touched by edits (they are charged to ed, not to u), and u more are dead for other reasons. Then, on the golden index: no
    record's dist is below the Levenshtein distance of the oriented pattern to reads[start:end], and every seq_find(hd = d <= ed)
    record's (rid, strand) appears with dist <= d."""
    from aindex_amd import synth
    g = synth.genome_ascii(1, 3000).tobytes()
    ind, pos = E.full_index(ref)
    full = E.EditRef(small23_prefix, indices=ind, positions=pos)
    clean = np.asarray([b"N" not in full.reads[s:e] for s, e in zip(full.start, full.end)])
    assert int(clean.sum()) > 250
    by_len = {L: [p for p, _ in pats if len(p) == L] for L in E.LENGTHS}
    with ThreadPoolExecutor(4) as ex:                          # numpy releases the interpreter lock in the row operations
        tables = list(ex.map(lambda ps: full.brute_all(ps + [F.comp_rev(p) for p in ps]), by_len.values()))
    dist = {}
    for ps, d in zip(by_len.values(), tables):
        for n, p in enumerate(ps):
            dist[p] = (d[n], d[n + len(ps)])
    assert full.brute_ed(pats[9][0], 2) == {(full.rid[r], st): int(dist[pats[9][0]][st][r]) for st in (0, 1) for r in range(len(full.rid))
                                            if dist[pats[9][0]][st][r] <= 2}
    checked = found = 0
    tried, reached = set(), {}
    for p, ops in pats:
        L = len(p)
        wins = [p[q:q + 23] for q in range(0, L - 22, 23)]
        u = sum(1 for w in wins if b"N" in w or ((w in g or F.comp_rev(w) in g) and full.bucket(w) is None))
        for ed in range(0, L // 23 - u):
            want = {(full.rid[r], st): int(dist[p][st][r]) for st in (0, 1) for r in np.nonzero(clean & (dist[p][st] <= ed))[0].tolist()}
            for step in (1, 23):
                got = {}
                for s, e, rid, local, strand, d in full.find_ed(p, ed, step):
                    if clean[full.rid.index(rid)]:
                        got[(rid, strand)] = min(got.get((rid, strand), 99), d)
                assert got == want
                checked += 1
                found += len(got)
            tried.add((L, ed))
            if ops and ed >= len(ops) and want:
                reached[(L, len(ops))] = reached.get((L, len(ops)), 0) + 1
    print("tried", sorted(tried), checked, found, "patterns with n edits compared, with answers, at an ed >= n", sorted(reached.items()))
    assert checked > 1000 and found > 4000 and {(150, 5), (100, 3), (70, 2), (69, 2), (47, 1), (46, 1), (24, 0), (23, 0)} <= tried
    # every (length, planted edits) pair that ed < L // 23 allows is compared where ed reaches the edits, on answers that are not empty
    assert set(reached) == {(L, n) for L in E.LENGTHS for n in (1, 2, 3) if n < L // 23}
    n = low = 0
    for p, _ in pats[::3]:
        res = ref.find_ed(p, 3, 23)
        for s, e, rid, local, strand, d in res:
            y = F.comp_rev(p) if strand else p
            assert d >= E.lev(y, ref.reads[s:e], True)
            if b"N" not in p and b"N" not in ref.reads[s:e]:
                from aindex_amd.aindex import edit_distance
                assert d >= edit_distance(y.decode(), ref.reads[s:e].decode())
            n += 1
        have = {}
        for s, e, rid, local, strand, d in res:
            have[(rid, strand)] = min(have.get((rid, strand), 99), d)
        for a, rid, local, strand, d in ref.find(p, 3, 23):
            assert have[(rid, strand)] <= d
            low += 1
    assert n > 500 and low > 200


def test_input_conditions(ref, pats, small23_prefix):
    """3. What the GPU tests rely on, under the restatement alone: the pattern set gives results of every kind they compare."""
    assert {len(p) for p, _ in pats} == set(E.LENGTHS) and {len(o) for _, o in pats} == {0, 1, 2, 3} and sum(1 for p, _ in pats if b"N" in p) == 1
    assert {k for _, o in pats for k, _ in o} == set("SID")
    st = {}
    res = [ref.find_ed(p, 3, 23, 0, st) for p, _ in pats]
    flat = [(len(p),) + x for (p, _), r in zip(pats, res) for x in r]
    by_dist = [sum(1 for x in flat if x[6] == d) for d in range(4)]
    by_len = [sum(1 for x in flat if x[2] - x[1] - x[0] == d) for d in (-1, 0, 1)]
    iv = {rid: (s, e) for rid, s, e in zip(ref.rid, ref.start, ref.end)}
    first = sum(1 for x in flat if x[4] == 0)
    last = sum(1 for x in flat if x[2] == iv[x[3]][1])
    strands = [sum(1 for x in flat if x[5] == s) for s in (0, 1)]
    dup = 0                                                    # sequences with two records of one (rid, strand) that overlap and start apart
    for r in res:
        dup += any(z[2] == x[2] and z[4] == x[4] and z[0] != x[0] and z[0] < x[1] for i, x in enumerate(r) for z in r[i + 1:])
    only = sum(1 for p, _ in pats if ref.find_ed(p, 1) and not ref.find(p, 3))     # found at ed = 1, missed by the Hamming search at hd = 3
    # proposals without an interval: the reads hold no seed outside an interval, so every fifth interval is taken away
    ridx = np.asarray([r for i, r in enumerate(zip(ref.rid, ref.start, ref.end)) if i % 5], np.uint64)
    gaps, sg = E.EditRef(small23_prefix, ridx=ridx), {}
    ng = sum(len(gaps.find_ed(p, 3, 23, 0, sg)) for p, _ in pats)
    print("results", len(flat), "by dist", by_dist, "by end - start - L", by_len, "first / last byte", first, last, "strands", strands, "stats", st,
          "near-duplicates", dup, "ed 1 only", only, "without every fifth interval", ng, sg)
    assert all(n > 0 for n in by_dist + by_len + strands) and first > 0 and last > 0 and only > 0
    assert st["shared"] > 0 and st["rejected"] > 0 and sg["no_interval"] > 0 and 0 < ng < len(flat)
    assert by_dist == [736, 476, 333, 270] and by_len == [325, 1192, 240] and (first, last) == (58, 60) and strands == [878, 937] and only == 53
    assert (st["proposed"], st.get("no_interval", 0), st["shared"], st["rejected"]) == (5852, 0, 757, 3280)
    assert (sg["proposed"], sg["no_interval"], ng) == (5852, 1181, 1439)
    # Near-duplicates (two overlapping records of one read and strand with different starts) need a pattern that aligns within ed at two
    # starts: both alignments hold an exact seed, so a 23-mer of the pattern must match the reads again at a shift of at most 2 ed with
    # at most ed edits. The synthetic genome has no such self-similar stretch, and an alignment with at most ed indels stays inside the
    # band of each of its own seeds, so all its seeds report the same (dist, start): none here. test_self_similar_text shows them.
    assert dup == 0


def test_self_similar_text(small23_prefix):
    """Overlapping records of one read and strand with different starts, on text made for them (seqedit_ref.self_similar_case: a read
    that repeats a 30-mer of the genome): the array surface keeps every start, the list surface merges them per read. The merge of
    AIndex.find_reads_by_sequence_edit_batch runs here over the restatement's arrays."""
    from aindex_amd.aindex import AIndex
    reads, ridx, seqs = E.self_similar_case(E.EditRef(small23_prefix))
    ind, pos = E.full_index(E.EditRef(small23_prefix, reads=reads, ridx=ridx))
    ss = E.EditRef(small23_prefix, indices=ind, positions=pos, reads=reads, ridx=ridx)
    for ed in (0, 1, 2):
        res = [ss.find_ed(p, ed, 1) for p in seqs]
        dup = [sum(1 for i, x in enumerate(r) for z in r[i + 1:] if z[2] == x[2] and z[4] == x[4] and z[0] != x[0] and z[0] < x[1]) for r in res]
        print("ed", ed, "records", [len(r) for r in res], "overlapping pairs", dup)
        live = [i for i in range(4) if i != 1 or ed]           # the pattern with a deleted base needs ed >= 1
        assert all(dup[i] > 0 for i in live) and dup[4] == 0   # the last pattern is a plain piece of the genome
        assert ed == 0 or any(x[5] == 1 for x in res[1])       # the repeat with a deleted base

        class Stub:
            def find_sequences_edit_array(self, s, e):
                return E.find_ed_csr(ss, s, e)

            def get_reads_by_rid_batch(self, rids):
                return [reads[701 * int(r):701 * int(r) + 700].decode() for r in rids]
        lists = AIndex.find_reads_by_sequence_edit_batch(Stub(), seqs, ed)
        assert lists == [ss.reads_by_sequence_ed(p, ed) for p in seqs]
        assert all(len(lists[i][0][3]) > 5 and len(lists[i][0][4]) > 5 and lists[i][0][1] == lists[i][0][3][0] for i in live)


def _dp(a: str, b: str) -> int:
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j - 1] + (a[i - 1] != b[j - 1]), prev[j] + 1, cur[j - 1] + 1)
        prev = cur
    return prev[-1]


def test_edit_distance():
    """4. aindex_amd.aindex.edit_distance (the reference re-exports editdistance.eval under this name): plain Levenshtein on str."""
    from aindex_amd.aindex import edit_distance
    assert edit_distance("", "") == 0 and edit_distance("kitten", "sitting") == 3 and edit_distance("", "ACGT") == 4
    assert edit_distance("ACGTACGT", "ACG") == 5 and edit_distance("ACG", "ACGTACGT") == 5 and edit_distance("ANGT", "ACGT") == 1
    rng = np.random.default_rng(5)
    for _ in range(200):
        a, b = ("".join(rng.choice(list("ACGTN"), int(n))) for n in rng.integers(0, 40, 2))
        assert edit_distance(a, b) == _dp(a, b) == edit_distance(b, a)
