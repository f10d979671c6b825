"""Differential fuzzing: many small random indexes / query sets / read buffers, HIP path vs the oracle."""
import os
import shutil

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import debruijn_ref as D
import graph_cases as G
import oracle_lib as O
from aindex_amd import _lib, builder, synth
from aindex_amd.engine import Index

ALPH = np.frombuffer(b"ACGTACGTACGTNacgtn~\n?U", dtype=np.uint8)


def _seeds(n):
    """The suite runs seeds 0..n-1; AIX_FUZZ_SEEDS="lo:hi" swaps in another range for one-off soak runs on a GPU box."""
    r = os.environ.get("AIX_FUZZ_SEEDS")
    if r:
        lo, hi = r.split(":")
        return range(int(lo), int(hi))
    return range(n)


def make_case(seed, tmp):
    rng = np.random.default_rng(seed)
    n = int(rng.choice([1, 3, 4, 7, 50, 333, 2000, 6000]))
    codes = np.unique(rng.integers(0, 4 ** 23, size=n, dtype=np.uint64))
    mode = seed % 3
    if mode == 0:                                  # all true-canonical -> fast path
        codes = np.unique(np.minimum(codes, synth.revcomp_codes(codes, 23)))
    elif mode == 1:                                # both strands of some keys stored
        codes = np.unique(np.concatenate([codes, synth.revcomp_codes(codes[: max(1, len(codes) // 3)], 23)]))
    if codes.shape[0] == 2:                        # hash domain 1 is never peelable (also in the reference)
        codes = codes[:1]
    tfs = rng.integers(0, 1000, size=codes.shape[0]).astype(np.uint32)
    tfs[rng.integers(0, codes.shape[0])] = 0xFFFFFFFF
    pf = builder.build_pf_codes(codes, 23)
    prefix = os.path.join(tmp, f"f{seed}")
    open(prefix + ".pf", "wb").write(pf)
    m = O.OracleMphf(prefix + ".pf")
    keys = synth.decode_kmers(codes, 23)
    rc, checker, tf = O.index_scatter(m, np.ascontiguousarray(keys).reshape(-1), tfs)
    assert rc == 0
    checker.tofile(prefix + ".kmers.bin")
    tf.tofile(prefix + ".tf.bin")
    return rng, codes, keys, prefix


def positions_reference(orc, q, oind, opos):
    """get_positions_23mer (python_wrapper.cpp:800-831) over get_pfid (hash.hpp:150-170), one k-mer at a time: the strand looked up is
    the raw 23 bytes if they compare bytewise <= the decode of the reverse complement of their sanitised code, else that decode; its
    bucket is answered when the hash of those bytes is a slot whose stored code is the strand's sanitised code."""
    q = np.ascontiguousarray(q, dtype=np.uint8).reshape(-1, 23)
    rev = D.decode(D.revcomp(D.encode(q)))
    checker, n = orc.checker(), orc.n
    out = []
    for i in range(q.shape[0]):
        raw, rv = bytes(q[i]), bytes(rev[i])
        strand = raw if raw <= rv else rv
        h = orc.hash(strand)
        if h < n and int(checker[h]) == int(D.encode(strand)[0]):
            seg = opos[int(oind[h]):min(int(oind[h + 1]), opos.shape[0])]
            out.append((seg[seg != 0] - np.uint64(1)).tolist())
        else:
            out.append([])
    return out


def check_positions_batch(ix, orc, q, tag):
    """positions_batch over the ORACLE's positions arrays of a buffer that holds the queries themselves, against positions_reference;
    ix / orc: the same index files with tf small enough for the arrays to be attached. get_pfid only ever looks up the bytewise
    smaller strand, so a key stored as the larger strand alone has no list: 500 queries for smaller strands stored in their own slot
    with tf > 0 are added, so that a quarter of the lists are non-empty whatever the strands of the case are. An index that stores no such key (one
    key, stored as its larger strand) cannot give a non-empty list: there the guard is that every list is empty."""
    checker, tf = orc.checker(), orc.tf_array()
    clean = np.unique(checker[checker < np.uint64(4 ** 23)])
    clean = clean[clean <= D.revcomp(clean)]
    h = np.minimum(orc.hash_batch(D.decode(clean)), np.uint64(orc.n - 1)).astype(np.int64)     # (a corrupt checker may hold a code in a slot that is not its own)
    reach = clean[(checker[h] == clean) & (tf[h] > 0)]
    if reach.shape[0]:
        q = np.concatenate([q, D.decode(np.resize(reach, 500))])
    # where the bytewise rule and the numeric one (code <= reverse complement) part: a smaller strand A...T, whose larger strand starts
    # with A too. The larger strand with '\n' for its first A is numerically the larger and bytewise the smaller: looked up as its raw
    # bytes, no list. The smaller strand with 'a' for its first A is the other way round: the list of the larger strand, if stored.
    a = D.decode(reach)
    edge = reach[(a[:, 0] == ord("A")) & (a[:, 22] == ord("T"))][:100]
    assert edge.shape[0] or reach.shape[0] < 200, tag
    if edge.shape[0]:
        large, small = D.decode(D.revcomp(edge)).copy(), D.decode(edge).copy()
        large[:, 0], small[:, 0] = ord("\n"), ord("a")
        q = np.concatenate([q, D.decode(edge), large, small])
    q = np.ascontiguousarray(q)
    buf = b"\n".join(bytes(x) for x in q) + b"\n"
    oind, opos = orc.positions(buf)
    want = positions_reference(orc, q, oind, opos)
    nonempty = sum(1 for p in want if p)
    print(tag, "position lists", len(want), "non-empty", nonempty, "entries", sum(map(len, want)), "keys with a list", reach.shape[0],
          "of them A...T", edge.shape[0])
    if reach.shape[0]:
        assert 4 * nonempty >= len(want), tag
    else:                                                          # only the smallest indexes of make_case (1 .. 7 keys, 3 trailing entries at most)
        assert nonempty == 0 and orc.n <= 10, tag
    ix.attach_aindex(oind, opos)
    try:
        for table in (True, False):
            for filt in (True, False):
                ix.set_bucket_table(table, 8); ix.set_absence_filter(filt)
                for m in (0, 1, 3):
                    off, pos = ix.positions_batch(q, max_per_kmer=m)
                    off, pos = off.tolist(), pos.tolist()
                    got = [pos[off[i]:off[i + 1]] for i in range(len(off) - 1)]
                    assert got == [p[:m] if m else p for p in want], (tag, table, filt, m)
    finally:
        ix.set_bucket_table(True, 8); ix.set_absence_filter(True)
        ix.detach_aindex()


@pytest.mark.parametrize("seed", _seeds(24))
def test_fuzz_queries_counts_positions(seed, tmp_path):
    rng, codes, keys, prefix = make_case(seed, str(tmp_path))
    orc = O.OracleIndex23.from_prefix(prefix)
    with Index.open_23(prefix + ".pf", prefix + ".tf.bin", prefix + ".kmers.bin") as ix:
        assert ix.canonical_only == bool(np.all(codes <= synth.revcomp_codes(codes, 23)))
        nq = 3000
        q = ALPH[rng.integers(0, ALPH.shape[0], size=(nq, 23))].copy()
        pick = rng.integers(0, keys.shape[0], size=nq // 3)
        q[: nq // 3] = keys[pick]
        q[nq // 3: nq // 2] = synth.decode_kmers(synth.revcomp_codes(codes[pick[: nq // 2 - nq // 3]], 23), 23)
        mut = rng.integers(0, nq // 2, size=200)
        q[mut, rng.integers(0, 23, size=200)] = ALPH[rng.integers(0, ALPH.shape[0], size=200)]
        want_tf = orc.tf_batch(q)
        qb = [bytes(x) for x in q[:400]]
        for fast in (True, False):
            for ee in (True, False):
                for bk, lanes in ((True, 8), (True, 1 << (seed % 3)), (False, 0)):     # verification table on (two lane widths) / off
                    ix.set_canonical_fastpath(fast); ix.set_early_exit(ee); ix.set_bucket_table(bk, lanes)
                    assert np.array_equal(ix.tf_ascii(q), want_tf), (seed, fast, ee, bk, lanes)
        ix.set_canonical_fastpath(True); ix.set_early_exit(True); ix.set_bucket_table(seed % 2 == 0, 8)
        assert ix.total_ascii(q[:400]).tolist() == [orc.total(b) for b in qb]
        f, r = ix.both_ascii(q[:400])
        assert [(int(a), int(b)) for a, b in zip(f, r)] == [orc.both(b) for b in qb]
        kid, strand = ix.kid_strand_ascii(q[:400])
        assert strand.tolist() == [orc.strand(b) for b in qb] and kid.tolist() == [orc.kid(b) for b in qb]
        assert np.array_equal(ix.hash_ascii(q[:400]), orc.hash_batch(q[:400]))
        # ragged lengths
        items = [bytes(x)[: int(rng.integers(0, 24))] + bytes(ALPH[rng.integers(0, 8, size=int(rng.integers(0, 30)))]) for x in q[:300]]
        assert ix.tf_ragged(items).tolist() == [orc.tf(b) for b in items]
        # a reads-like buffer built from keys, their reverse complements and noise, with separators
        parts = []
        for i in range(60):
            k1 = bytes(keys[int(rng.integers(0, keys.shape[0]))])
            noise = bytes(ALPH[rng.integers(0, ALPH.shape[0], size=int(rng.integers(0, 40)))])
            parts.append(k1 + noise + bytes(q[int(rng.integers(0, nq))]) + (b"\n" if i % 3 else b"~"))
        buf = b"".join(parts)
        for mode in (0, 1, 2):
            assert np.array_equal(ix.count23_fixed(buf, _lib.FMT_PLAIN, mode), orc.count23_fixed(buf, False, mode)), (seed, mode)
        ind, pos = ix.positions_fill(buf)
        oind, opos = orc.positions(buf)
        assert np.array_equal(ind, oind) and np.array_equal(pos, opos)
        # the multi-GPU shard protocols, replayed rank by rank: positions (tallies + carried slot numbering) and index scatter
        from shard_helpers import positions_by_shards, scatter_by_shards
        world = 2 + seed % 3
        pfa = np.fromfile(prefix + ".pf", dtype=np.uint8)
        ck, tfv = np.fromfile(prefix + ".kmers.bin", dtype=np.uint64), np.fromfile(prefix + ".tf.bin", dtype=np.uint32)
        # (one tf of the case is 2^32-1, i.e. a 34 GB positions array per call: the shard replay runs on the same keys with tf <= 3)
        with Index.create_23(pfa.tobytes(), ck, np.minimum(tfv, 3).astype(np.uint32)) as ix_small:
            wind, wpos = ix_small.positions_fill(buf)
            sind, spos, _ = positions_by_shards(ix_small, buf, world)
            assert np.array_equal(sind, wind) and np.array_equal(spos, wpos), (seed, world)
            # batch position queries (the strand rule of get_pfid) on the same small-tf index, over the oracle's arrays
            np.minimum(tfv, 3).astype(np.uint32).tofile(prefix + ".tf3.bin")
            orc_small = O.OracleIndex23(prefix + ".pf", prefix + ".tf3.bin", prefix + ".kmers.bin")
            check_positions_batch(ix_small, orc_small, q[:1500], ("positions", seed, seed % 3))
        n = ck.shape[0]
        perm = rng.permutation(n)                                         # the .dat order is not the slot order
        cuts = [0] + sorted(int(x) for x in rng.integers(0, n + 1, size=world - 1)) + [n]
        sc, stf, socc, sts, clash = scatter_by_shards(pfa, synth.decode_kmers(ck, 23)[perm], tfv[perm], n, cuts)
        assert all(x == 0 for x in sts) and not clash, (seed, sts)
        assert np.array_equal(sc, ck) and np.array_equal(stf, tfv)
        seqs = [buf[:200], buf[200:460], b"", buf[-30:]]
        for cutoff in (0, 5):
            for s, got in zip(seqs, ix.coverage(seqs, cutoff)):
                assert np.array_equal(got, orc.coverage(s, cutoff))


# ------------------------------------------------------------------------------------------------
# 13-mer mode: random buffers in the three input formats, then noisy queries against the counted table
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ix13():
    from pf13 import pf13_path
    ix = Index.open_13(pf13_path(), None)
    yield ix
    ix.close()


def _rand_seq(rng, lo, hi):
    return bytes(ALPH[rng.integers(0, ALPH.shape[0] - 3, size=int(rng.integers(lo, hi)))])     # no '~', '\n', '?' inside


@pytest.mark.parametrize("seed", _seeds(8))
def test_fuzz_13mer(seed, ix13):
    from pf13 import pf13_path
    rng = np.random.default_rng(1_000_000 + seed)
    m = O.OracleMphf(pf13_path())
    kind = seed % 4
    recs = [_rand_seq(rng, 0, 120) for _ in range(int(rng.integers(1, 60)))]
    if kind == 0:
        buf = b"".join(r + (b"\n" if rng.random() < 0.9 else b"~" + _rand_seq(rng, 0, 50) + b"\n") for r in recs)
    elif kind == 1:
        buf = b"".join(b">h%d %s\n" % (i, _rand_seq(rng, 0, 10)) + b"".join(r[j:j + 37] + (b"\r\n" if i % 7 == 0 else b"\n") for j in range(0, len(r), 37)) +
                       (b"\n" if i % 5 == 0 else b"") for i, r in enumerate(recs))
    elif kind == 2:
        buf = b"".join(b"@r%d\n" % i + r + b"\n+\n" + b"I" * len(r) + b"\n" for i, r in enumerate(recs))
    else:
        buf = b"\n" + b"".join(r + b"\n" for r in recs)                    # empty first line -> PLAIN
    if seed >= 4:
        buf = buf.rstrip(b"\n")                                            # no trailing newline
    want = O.count13(m, buf, -1)
    got = ix13.count13(buf)
    assert np.array_equal(got, want), (seed, kind)
    tf = want.copy()
    tf[np.nonzero(tf)[0][::3]] += np.uint64(1 << 33)                       # > 32-bit values
    ix13.set_tf_13(tf)
    orc = O.OracleIndex13(pf13_path(), tf)
    plain = [r for r in recs if len(r) >= 13]
    q = []
    for r in plain[:40]:
        p = int(rng.integers(0, len(r) - 12))
        q.append(r[p:p + 13])
    q += [bytes(ALPH[rng.integers(0, ALPH.shape[0], size=13)]) for _ in range(200)]
    q += [bytes(ALPH[rng.integers(0, 12, size=13)]) for _ in range(200)]   # mostly valid upper-case
    qa = np.frombuffer(b"".join(q), dtype=np.uint8)
    assert np.array_equal(ix13.tf_ascii(qa), orc.tf_batch(qa))
    assert ix13.total_ascii(qa).tolist() == [orc.total(s) for s in q]
    f, r2 = ix13.both_ascii(qa)
    assert [(int(a), int(b)) for a, b in zip(f, r2)] == [orc.both(s) for s in q]
    items = [s[: int(rng.integers(0, 14))] + bytes(ALPH[rng.integers(0, 8, size=int(rng.integers(0, 5)))]) for s in q[:100]]
    assert ix13.tf_ragged(items).tolist() == [orc.tf(s) for s in items]
    for s, got_cov in zip(plain[:5], ix13.coverage(plain[:5], 1)):
        assert np.array_equal(got_cov, orc.coverage(s, 1))


@pytest.mark.parametrize("seed", _seeds(6))
def test_fuzz_normalise_and_distinct(seed):
    """Random FASTA/FASTQ-like byte soup: device normalisation == host normalisation; distinct k-mer sets == oracle."""
    import torch
    from aindex_amd import counting
    rng = np.random.default_rng(2_000_000 + seed)
    soup = np.frombuffer(b"ACGTACGTACGTNacgtu>@+\n\n\r ~U", dtype=np.uint8)
    buf = bytes(soup[rng.integers(0, soup.shape[0], size=int(rng.integers(1, 40000)))])
    if seed % 2 == 0:
        buf = b">" + buf
    t = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
    for fmt, mode in ((1, 0), (1, 1), (2, 0)):
        want = counting.normalize(buf, fmt, mode)
        got = counting.normalize_t(t, fmt, mode).cpu().numpy().tobytes()
        assert got == want, (seed, fmt, mode)
    for k in (5, 13, 17, 23, 31):
        for canon in (0, 1, 2):
            keys, counts = counting.count_distinct(buf, k, canon, 1 + seed % 2)
            okeys, ocnt = O.count_distinct(buf, k, canon, 1 + seed % 2)
            assert np.array_equal(keys, okeys) and np.array_equal(counts, ocnt), (seed, k, canon)
    # counted piece by piece (what buffers beyond 2^31 windows go through): every cut position gives the same set
    for piece in (1, 97, 4096):
        os.environ["AIX_DISTINCT_PIECE"] = str(piece)
        try:
            small = buf[: 3000 if piece == 1 else len(buf)]
            for k, canon, mc in ((13, 2, 1), (23, 1, 2), (31, 0, 1)):
                keys, counts = counting.count_distinct(small, k, canon, mc)
                okeys, ocnt = O.count_distinct(small, k, canon, mc)
                assert np.array_equal(keys, okeys) and np.array_equal(counts, ocnt), (seed, piece, k, canon)
        finally:
            del os.environ["AIX_DISTINCT_PIECE"]


def corrupt_index_files(rng, prefix, p2):
    """Copy the index files of `prefix` to `p2` with a checker that disagrees with the MPHF (swapped / foreign / duplicated / out-of-range
    codes, the reverse complement of another key), maybe extra trailing entries and a short tf file. Returns the corrupt checker."""
    checker = np.fromfile(prefix + ".kmers.bin", dtype=np.uint64)
    tf = np.fromfile(prefix + ".tf.bin", dtype=np.uint32)
    n = checker.shape[0]
    for _ in range(max(1, n // 10)):
        i, j = rng.integers(0, n, size=2)
        op = int(rng.integers(0, 5))
        if op == 0:
            checker[[i, j]] = checker[[j, i]]
        elif op == 1:
            checker[i] = rng.integers(0, 4 ** 23, dtype=np.uint64)
        elif op == 2:
            checker[i] = checker[j]
        elif op == 3:
            checker[i] |= np.uint64(1) << np.uint64(int(rng.integers(46, 64)))
        else:
            checker[i] = synth.revcomp_codes(checker[j:j + 1] & np.uint64(4 ** 23 - 1), 23)[0]
    extra = int(rng.integers(0, 4))
    if extra:
        checker = np.concatenate([checker, rng.integers(0, 4 ** 23, size=extra, dtype=np.uint64)])
        tf = np.concatenate([tf, rng.integers(1, 9, size=extra).astype(np.uint32)])
    checker.tofile(p2 + ".kmers.bin")
    tf[: max(0, tf.shape[0] - int(rng.integers(0, 3)))].tofile(p2 + ".tf.bin")          # tf file may be short (hash.cpp:431-444)
    shutil.copy(prefix + ".pf", p2 + ".pf")
    return checker


@pytest.mark.parametrize("seed", _seeds(10))
def test_fuzz_corrupt_index_files(seed, tmp_path):
    """Index files that disagree with the MPHF (swapped / foreign / duplicated / out-of-range codes, short tf file,
    extra trailing entries): the HIP path must answer exactly like the reference's evaluator on the same files."""
    rng, codes, keys, prefix = make_case(3_000_000 + seed, str(tmp_path))
    p2 = os.path.join(str(tmp_path), "c")
    checker = corrupt_index_files(rng, prefix, p2)
    orc = O.OracleIndex23.from_prefix(p2)
    allc = np.unique(np.concatenate([codes, checker & np.uint64(4 ** 23 - 1)]))
    q = np.concatenate([synth.decode_kmers(allc, 23), synth.decode_kmers(synth.revcomp_codes(allc, 23), 23),
                        ALPH[rng.integers(0, ALPH.shape[0], size=(500, 23))]])
    if q.shape[0] > 6000:
        q = q[rng.permutation(q.shape[0])[:6000]]
    q = q.copy()
    mut = rng.integers(0, q.shape[0], size=300)
    q[mut, rng.integers(0, 23, size=300)] = ALPH[rng.integers(0, ALPH.shape[0], size=300)]
    want = orc.tf_batch(q)
    qb = [bytes(x) for x in q[:300]]
    with Index.open_23(p2 + ".pf", p2 + ".tf.bin", p2 + ".kmers.bin") as ix:
        for fast in (True, False):
            for fp in (True, False):
                for ee in (True, False):
                    for bk in (True, False):
                        ix.set_canonical_fastpath(fast); ix.set_fingerprint_filter(fp); ix.set_early_exit(ee); ix.set_bucket_table(bk, 8 >> (seed % 4))
                        assert np.array_equal(ix.tf_ascii(q), want), (seed, fast, fp, ee, bk)
        ix.set_canonical_fastpath(True); ix.set_fingerprint_filter(True); ix.set_early_exit(True); ix.set_bucket_table(seed % 2 == 1, 8)
        kid, strand = ix.kid_strand_ascii(q[:300])
        assert strand.tolist() == [orc.strand(b) for b in qb] and kid.tolist() == [orc.kid(b) for b in qb]
        assert ix.total_ascii(q[:300]).tolist() == [orc.total(b) for b in qb]
        buf = b"\n".join(bytes(x) for x in q[:200]) + b"\n"
        for mode in (0, 1, 2):
            assert np.array_equal(ix.count23_fixed(buf, _lib.FMT_PLAIN, mode), orc.count23_fixed(buf, False, mode))
        ind, pos = ix.positions_fill(buf)
        oind, opos = orc.positions(buf)
        assert np.array_equal(ind, oind) and np.array_equal(pos, opos)
    # batch position queries on the corrupt files (one tf of the case is 2^32-1: the same files with tf <= 3, so that the arrays can be
    # attached). Queries: the codes of the original and of the corrupt checker and their reverse complements, repeated where the index
    # is tiny (many lists then read one bucket), and the noisy tail of q.
    p3 = os.path.join(str(tmp_path), "c3")
    checker.tofile(p3 + ".kmers.bin")
    np.minimum(orc.tf_array(), 3).astype(np.uint32).tofile(p3 + ".tf.bin")
    shutil.copy(p2 + ".pf", p3 + ".pf")
    both = np.stack([allc, synth.revcomp_codes(allc, 23)], axis=1).reshape(-1)
    pq = np.concatenate([synth.decode_kmers(np.resize(both, 1100), 23), q[-400:]])
    with Index.open_23(p3 + ".pf", p3 + ".tf.bin", p3 + ".kmers.bin") as ix3:
        check_positions_batch(ix3, O.OracleIndex23.from_prefix(p3), pq, ("positions, corrupt files", seed))


# ------------------------------------------------------------------------------------------------
# De Bruijn neighbours and walks (aix_debruijn.hip) on graph cases: keys with neighbours, both strands stored with different tf, stored
# tf of 0 and of 2^32-1, ties, sums that wrap (tests/graph_cases.py; tests/test_debruijn_cpu.py shows that the cases hold all that)
# ------------------------------------------------------------------------------------------------
CANARY8, CANARY32 = 0xEE, 0xEEEEEEEE
DIRTY = np.frombuffer(b"acgtnN~\n\x00" + bytes(range(0x80, 0x100)), dtype=np.uint8)
DBJ_WALKS = [(d, m, c) for d in (D.NEXT, D.PREV) for m in (D.GREEDY, D.UNITIG) for c in (0, 3)]
DBJ_TAILS = (1, 3, 15, 16, 17, 63, 64, 65, 255, 257)


def _rows(recs):
    """CONT records -> int array [..., 8]: tf A C G T, n, sum, best_tf, best_base"""
    return np.concatenate([recs["tf"], np.stack([recs["n"], recs["sum"], recs["best_tf"], recs["best_base"]], axis=-1)], axis=-1).astype(np.int64)


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64).copy() if a.dtype == np.uint64 else a.reshape(-1).copy()).cuda()


def _dirty_ascii(rng, codes):
    """The k-mers as ASCII with bytes outside upper-case ACGT (lower case, N, ~, newline, 0x00, 0x80 .. 0xFF) planted in about a tenth of them"""
    a = D.decode(codes & D.MASK46).copy()
    hit = np.nonzero(rng.random(a.shape[0]) < 0.1)[0]
    for _ in range(3):                                             # one to three bytes per dirty item
        a[hit, rng.integers(0, 23, hit.shape[0])] = DIRTY[rng.integers(0, DIRTY.shape[0], hit.shape[0])]
        hit = hit[rng.random(hit.shape[0]) < 0.5]
    return a


class DbjCase:
    """One index and one seed set: debruijn_ref's answers over `freq` (computed once per leg and kept) against the device entry points,
    which write into canary-filled tensors 64 records / rows longer than the batch."""

    def __init__(self, ix, freq, seeds, rng):
        self.ix, self.freq = ix, freq
        self.codes = np.ascontiguousarray(seeds)
        self.ascii = _dirty_ascii(rng, seeds)
        self.src = {"codes": self.codes, "ascii": D.encode(self.ascii)}     # what the reference walks from
        self.t = {"codes": _dev(self.codes), "ascii": _dev(self.ascii)}
        assert (self.src["ascii"] != (self.codes & D.MASK46)).mean() > 0.03
        self._nb, self._walk = {}, {}

    def nb_ref(self, form, cutoff):
        """int64 [S, 2, 8]: next, prev"""
        if (form, cutoff) not in self._nb:
            self._nb[(form, cutoff)] = _rows(D.neighbours(self.freq, self.src[form], D.BOTH, cutoff))
        return self._nb[(form, cutoff)]

    def walk_ref(self, form, d, m, L, cutoff):
        key = (form, d, m, L, cutoff)
        if key not in self._walk:
            self._walk[key] = D.walk(self.freq, self.src[form], d, L, cutoff, m)
        return self._walk[key]

    def neighbours(self, form, direction, cutoff, tag, count=None):
        import torch
        n = self.codes.shape[0] if count is None else count
        t = self.t[form][: n * (23 if form == "ascii" else 1)]
        recs = n * (2 if direction == D.BOTH else 1)
        big = torch.full((recs + 64, 8), CANARY32 - (1 << 32), dtype=torch.int32, device="cuda")
        self.ix.neighbours_t(t, direction, cutoff, out_t=big[:recs])
        got = big.cpu().numpy().view(np.uint32)
        assert (got[recs:] == CANARY32).all(), (tag, "records beyond the batch were written")
        ref = self.nb_ref(form, cutoff)[:n]
        want = ref.reshape(-1, 8) if direction == D.BOTH else ref[:, direction]
        bad = np.nonzero((got[:recs].astype(np.int64) != want).any(axis=1))[0]
        assert bad.shape[0] == 0, (tag, "first differing record", int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist(), "of", bad.shape[0])

    def walk(self, form, d, m, L, cutoff, want_tf, tag, count=None):
        import torch
        s = self.codes.shape[0] if count is None else count
        t = self.t[form][: s * (23 if form == "ascii" else 1)]
        bases = torch.full((s + 64, L), CANARY8, dtype=torch.uint8, device="cuda")
        tfs = torch.full((s + 64, L), CANARY32 - (1 << 32), dtype=torch.int32, device="cuda") if want_tf else None
        b, ln, st, tf, last = self.ix.walk_t(t, L, d, cutoff, m, want_tf=want_tf, bases_t=bases[:s], tf_t=tfs[:s] if want_tf else None)
        assert (tf is None) == (not want_tf)
        wb, wl, ws, wt, wlast = (x[:s] for x in self.walk_ref(form, d, m, L, cutoff))
        inside = np.arange(L)[None, :] < wl[:, None]
        assert np.array_equal(ln.cpu().numpy().view(np.uint32), wl), (tag, "length")
        assert np.array_equal(st.cpu().numpy(), ws), (tag, "stop")
        assert np.array_equal(last.cpu().numpy().view(np.uint64), wlast), (tag, "last")
        got_b = bases.cpu().numpy()
        assert np.array_equal(got_b[:s], np.where(inside, wb, CANARY8)), (tag, "bases up to the length, the canary from there on")
        assert (got_b[s:] == CANARY8).all(), (tag, "rows beyond the batch were written")
        if want_tf:
            got_t = tfs.cpu().numpy().view(np.uint32)
            assert np.array_equal(got_t[:s], np.where(inside, wt, CANARY32)), (tag, "tf")
            assert (got_t[s:] == CANARY32).all(), (tag, "tf rows beyond the batch were written")
        return ws

    def every_leg(self, tag, steps=(1, 7, 64)):
        """neighbours: NEXT / PREV / BOTH x cutoff 0, 3 x codes, dirty ASCII; walks: direction x mode x max_steps x cutoff x want_tf"""
        for cutoff in (0, 3):
            for form in ("codes", "ascii"):
                for direction in (D.NEXT, D.PREV, D.BOTH):
                    self.neighbours(form, direction, cutoff, tag + ("neighbours", form, direction, cutoff))
        hist = np.zeros(5, np.int64)
        for d, m, cutoff in DBJ_WALKS:
            for L in steps:
                for want_tf in (True, False):
                    ws = self.walk("codes", d, m, L, cutoff, want_tf, tag + ("walk", d, m, L, cutoff, want_tf))
                hist += np.bincount(ws, minlength=5)
        self.walk("ascii", D.NEXT, D.UNITIG, 7, 0, True, tag + ("walk from dirty ASCII",))
        self.walk("ascii", D.PREV, D.GREEDY, 7, 3, False, tag + ("walk from dirty ASCII",))
        return hist


@pytest.mark.parametrize("seed", _seeds(12))
def test_fuzz_debruijn(seed, tmp_path, monkeypatch):
    """De Bruijn neighbours and walks on a graph case (canonical / strand met first / mixed, a third of the keys with both strands stored
    and different tf) == debruijn_ref over the oracle on the same files: every direction, cutoff, input form, walk mode and max_steps;
    every absence-filter policy, verification-table shape and the canonical fast path on and off; batches of 1 .. 257 seeds."""
    prefix, codes, tfs, seeds = G.write_graph_case(seed, str(tmp_path))
    rng = np.random.default_rng(5_000_000 + seed)
    freq = D.oracle_freq(O.OracleIndex23.from_prefix(prefix))
    with Index.open_23(prefix + ".pf", prefix + ".tf.bin", prefix + ".kmers.bin") as ix:
        assert ix.canonical_only == bool(np.all(codes <= D.revcomp(codes))) == (seed % 3 == 0)
        case = DbjCase(ix, freq, seeds, rng)
        tag = ("debruijn", seed, "mode", seed % 3, "keys", codes.shape[0], "seeds", seeds.shape[0])
        hist = case.every_leg(tag)
        print(*tag, "stop histogram of the reference", dict(zip(D.STOP_NAMES, hist.tolist())))
        assert (hist > 0).all()
        # the switches: one neighbours leg and one walk leg per combination
        k = 0
        for policy in ("0", "1", "2"):
            monkeypatch.setenv("AIX_DBJ_FILTER", policy)
            for table, lanes in ((True, 8), (True, 1 << (seed % 3)), (False, 0)):
                for fast in (True, False):
                    ix.set_bucket_table(table, lanes); ix.set_canonical_fastpath(fast)
                    sw = tag + ("filter policy", policy, "table", table, lanes, "fast path", fast)
                    case.neighbours("codes", D.BOTH, 3 * (k % 2), sw)
                    d, m, cutoff = DBJ_WALKS[(k + seed) % len(DBJ_WALKS)]
                    case.walk("codes", d, m, 64, cutoff, k % 2 == 0, sw + ("walk", d, m, cutoff))
                    k += 1
        assert k == 18
        monkeypatch.delenv("AIX_DBJ_FILTER")
        ix.set_bucket_table(True, 8); ix.set_canonical_fastpath(True)
        # batch tails: a partial last quad group, a partial wave, a partial workgroup
        for j, n in enumerate(DBJ_TAILS):
            case.neighbours("codes", D.BOTH, 0, tag + ("first", n), count=n)
            d, m, cutoff = DBJ_WALKS[(j + seed) % len(DBJ_WALKS)]
            case.walk("codes", d, m, 7, cutoff, True, tag + ("first", n, "walk", d, m, cutoff), count=n)


@pytest.mark.parametrize("seed", _seeds(6))
def test_fuzz_debruijn_corrupt_index(seed, tmp_path):
    """The corruption of test_fuzz_corrupt_index_files applied to a graph case: overflowed buckets, unfiled keys, codes with bits
    46 .. 63 set, foreign and duplicate codes reach the quad-layout probes of the De Bruijn kernels; == debruijn_ref over the oracle on
    the corrupt files, with the fingerprint filter and the early exit on and off."""
    prefix, codes, tfs, seeds = G.write_graph_case(1000 + seed, str(tmp_path))
    rng = np.random.default_rng(6_000_000 + seed)
    p2 = os.path.join(str(tmp_path), "c")
    checker = corrupt_index_files(rng, prefix, p2)
    assert (checker[: codes.shape[0]] != np.fromfile(prefix + ".kmers.bin", dtype=np.uint64)).mean() > 0.03
    # the codes the corruption brought in and their reverse complements are seeds too
    foreign = np.setdiff1d(checker, codes)
    seeds = np.concatenate([seeds, foreign, D.revcomp(foreign & D.MASK46)])
    freq = D.oracle_freq(O.OracleIndex23.from_prefix(p2))
    with Index.open_23(p2 + ".pf", p2 + ".tf.bin", p2 + ".kmers.bin") as ix:
        case = DbjCase(ix, freq, seeds, rng)
        for fp in (True, False):
            for ee in (True, False):
                ix.set_fingerprint_filter(fp); ix.set_early_exit(ee); ix.set_bucket_table(seed % 2 == 0 or fp, 8 >> (seed % 4))
                tag = ("debruijn, corrupt files", seed, "mode", (1000 + seed) % 3, "fingerprints", fp, "early exit", ee)
                hist = case.every_leg(tag)
                print(*tag, "stop histogram of the reference", dict(zip(D.STOP_NAMES, hist.tolist())))
                assert (hist > 0).all()


def test_neighbours_second_trip_of_the_grid_stride_loop(gold, monkeypatch):
    """k_db_neighbours runs on at most 65 536 workgroups of 64 records: from 4 194 304 records on a workgroup makes a second trip of
    its loop, with the absence-filter state of the first. 2^21 + 37 seeds in both directions and 2^22 + 53 seeds in one: every record of
    the second trip and 20 000 sampled ones of the first equal the helper's, and the whole output equals the same call made in chunks
    of 2^20 seeds (HIP against HIP; batches of that size are what the other tests compare with the oracle), under the gauge policy and
    the always-on policy of the filter.
    k_db_walk is capped at 2^22 workgroups of 64 seeds: its loop makes a second trip from 2^28 seeds on, which no test of a few seconds
    can reach; its trip is the body of this kernel's trip around the same probe."""
    import torch
    FIRST_TRIP = 65536 * 64
    p = os.path.join(gold, "small23", "small23")
    freq = D.oracle_freq(O.OracleIndex23.from_prefix(p), threads=8)
    with Index.open_23(p + ".pf", p + ".tf.bin", p + ".kmers.bin") as ix:
        checker = ix.checker_array()
        rng = np.random.default_rng(9)
        for n, direction, cutoff in (((1 << 21) + 37, D.BOTH, 0), (FIRST_TRIP + 53, D.NEXT, 2)):
            per = 2 if direction == D.BOTH else 1
            recs = n * per
            assert recs > FIRST_TRIP
            seeds = rng.integers(0, 1 << 46, n, dtype=np.uint64)
            stored_at = np.concatenate([rng.choice(n - 200, n // 50, replace=False), np.arange(n - 200, n, 2)])   # about 2 %, and half of the last 200
            keys = checker[rng.integers(0, checker.shape[0], stored_at.shape[0])]
            seeds[stored_at] = np.where(rng.random(stored_at.shape[0]) < 0.5, keys, D.revcomp(keys))
            t = torch.from_numpy(seeds.view(np.int64)).cuda()
            sample = np.unique(np.concatenate([rng.integers(0, n, 20_000 // per), np.arange((FIRST_TRIP // per) - 100, n)]))
            assert (sample * per >= FIRST_TRIP).sum() >= (37 if per == 2 else 53)
            want = _rows(D.neighbours(freq, seeds[sample], direction, cutoff)).reshape(sample.shape[0], per * 8)
            assert (want.reshape(-1, 8)[:, 4] > 0).mean() > 0.01
            sample_t = torch.from_numpy(sample).cuda()
            for policy in ("0", "1"):
                monkeypatch.setenv("AIX_DBJ_FILTER", policy)
                whole = ix.neighbours_t(t, direction, cutoff)
                pieces = torch.full_like(whole, -1)
                for lo in range(0, n, 1 << 20):
                    ix.neighbours_t(t[lo:lo + (1 << 20)], direction, cutoff, out_t=pieces[lo:lo + (1 << 20)])
                torch.cuda.synchronize()
                got = whole.reshape(n, per * 8)[sample_t].cpu().numpy().view(np.uint32).astype(np.int64)
                bad = np.nonzero((got != want).any(axis=1))[0]
                assert bad.shape[0] == 0, (n, policy, "first differing seed", int(sample[bad[0]]), "of", bad.shape[0])
                assert torch.equal(whole, pieces), (n, policy)
                print("seeds", n, "records", recs, "policy", policy, "sampled seeds", sample.shape[0], "records with a neighbour",
                      int((want.reshape(-1, 8)[:, 4] > 0).sum()))
