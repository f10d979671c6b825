"""Read cleaning on the GPU (aix_readfix.hip): planted substitutions that must be undone completely, and noisy reads, odd shapes, the
golden index and every switch against the test-side restatement (tests/readfix_ref.py). Every comparison is exact equality."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import debruijn_ref as D
import oracle_lib as O
import readfix_cases as K
import readfix_ref as R
from aindex_amd import _lib, builder
from aindex_amd.aindex import AIndex
from aindex_amd.engine import Index

vp = _lib.vp
PARAMS = [(1, 8, 4), (2, 1, 16), (1, 16, 1), (1, 8, 0)]


def _i64(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def _dev(ix, buf, start, end, t, V, F, canary=True):
    """the device form on fresh tensors with canary-filled log rows: (bytes, records, fix_pos, fix_old) as numpy arrays"""
    import torch
    b = torch.from_numpy(np.array(buf, dtype=np.uint8, copy=True)).cuda()
    m = len(start)
    fp = torch.full((m, F), -0x11111112 if canary else 0, dtype=torch.int32, device="cuda")
    fo = torch.full((m, F), 0xEE if canary else 0, dtype=torch.uint8, device="cuda")
    rec, fp, fo = ix.fix_reads_t(b, _i64(start), _i64(end), t, V, F, fp, fo)
    torch.cuda.synchronize()
    return b.cpu().numpy(), rec.cpu().numpy().view(np.uint32).reshape(m, 8), fp.cpu().numpy().view(np.uint32), fo.cpu().numpy()


def _rows(rec):
    return np.stack([rec[f] for f in R.REC_FIELDS], axis=1).astype(np.uint32)


def _want(freq, buf, start, end, t, V, F):
    m = len(start)
    return R.fix_reads(freq, buf, start, end, t, V, F, np.full((m, F), 0xEEEEEEEE, np.uint32), np.full((m, F), 0xEE, np.uint8))


def _same(got, want, tag=""):
    out, rec, fp, fo = want
    assert np.array_equal(got[1], _rows(rec)), tag
    assert np.array_equal(got[2], fp) and np.array_equal(got[3], fo), tag
    assert np.array_equal(got[0], out), tag


def _build_from_codes(codes, tf):
    import torch
    keys = _i64(codes)
    pf = builder.build_pf_codes_t(keys, 23)
    return pf, Index.build_23_codes_t(pf, keys, torch.full((len(codes),), tf, dtype=torch.int32, device="cuda"))


@pytest.fixture(scope="module")
def planted():
    genome, buf, start, end, truth, plants = K.planted_case()
    codes, _ = K.genome_freq(genome)
    pf, ix = _build_from_codes(codes, 5)
    yield {"ix": ix, "buf": buf, "start": start, "end": end, "truth": truth, "plants": plants}
    ix.close()


def _check_planted(c, out, rec, fp, fo):
    """Every read equals its truth, fixes = the number planted, the log = the plants, CLEAN or FIXED, and the buffer differs from the
    input exactly at the logged positions. Holds for these inputs because the plants lie >= 45 > V + 22 bases apart in a random genome
    whose 23-mers all have tf 5: a try sees one error at a time and only the true base makes its windows solid (confirmed with the
    helper over dict_freq for this seed)."""
    assert np.array_equal(out, c["truth"])
    n = np.array([len(p) for p in c["plants"]])
    assert np.array_equal(rec[:, 3], n) and np.isin(rec[:, 0], (R.CLEAN, R.FIXED)).all()
    assert np.array_equal(rec[:, 0] == R.CLEAN, n == 0) and not rec[:, 2].any() and (rec[:, 6] == 0).all() and (rec[:, 7] == 150).all()
    logged = []
    for r, pl in enumerate(c["plants"]):
        assert [(int(fp[r, j]), int(fo[r, j])) for j in range(len(pl))] == pl, r
        logged += [151 * r + p for p, _ in pl]
    assert sorted(logged) == np.flatnonzero(out != c["buf"]).tolist()
    assert {0, 22, 23, 127, 149} <= {p for pl in c["plants"] for p, _ in pl} and n.max() == 3


def test_planted_substitutions_are_undone_device_form(planted):
    c = planted
    out, rec, fp, fo = _dev(c["ix"], c["buf"], c["start"], c["end"], 1, 8, 4)
    _check_planted(c, out, rec, fp, fo)
    for r, pl in enumerate(c["plants"]):                          # nothing at or beyond `fixes`
        assert (fp[r, len(pl):] == 0xEEEEEEEE).all() and (fo[r, len(pl):] == 0xEE).all()


def test_planted_substitutions_are_undone_host_form(planted):
    c = planted
    out, rec, fp, fo = c["ix"].fix_reads(c["buf"], c["start"], c["end"], 1, 8, 4)
    _check_planted(c, out, _rows(rec), fp, fo)


def test_planted_substitutions_are_undone_list_form(planted):
    c = planted
    ai = AIndex()
    ai._wrapper._ix23 = c["ix"]
    try:
        raw, tr = c["buf"].tobytes(), c["truth"].tobytes()
        reads = [raw[a:b].decode() for a, b in zip(c["start"].tolist(), c["end"].tolist())]
        fixed, rec = ai.correct_reads(reads, 1, 8, 4)
        assert fixed == [tr[a:b].decode() for a, b in zip(c["start"].tolist(), c["end"].tolist())]
        assert rec["fixes"].tolist() == [len(p) for p in c["plants"]]
        cls = ai.classify_reads(reads, 1)
        assert np.array_equal(cls["weak_before"], rec["weak_before"]) and not cls["fixes"].any()
        assert np.array_equal(cls["status"] == R.CLEAN, rec["status"] == R.CLEAN) and (cls["status"][rec["status"] == R.FIXED] == R.UNFIXED).all()
        assert ai.correct_reads([]) [0] == []
    finally:
        ai._wrapper._ix23 = None


@pytest.fixture(scope="module")
def noisy(tmp_path_factory):
    """The index of the reads' own distinct 23-mers built on the device, and the helper's freq over the oracle on the same files."""
    import torch
    from aindex_amd import counting
    plain, start, end = K.noisy_case()
    keys, counts = counting.count_distinct_t(torch.from_numpy(plain).cuda(), 23, _lib.CANON_TRUE_RC)
    pf = builder.build_pf_codes_t(keys, 23)
    ix = Index.build_23_codes_t(pf, keys, counts.to(torch.int32))
    torch.cuda.synchronize()
    d = tmp_path_factory.mktemp("readfix")
    paths = [str(d / n) for n in ("s.pf", "s.tf.bin", "s.kmers.bin")]
    open(paths[0], "wb").write(pf)
    ix.tf_array().tofile(paths[1])
    ix.checker_array().tofile(paths[2])
    freq = K.MemoFreq(D.oracle_freq(O.OracleIndex23(*paths), threads=8))
    freq.prime(plain, start, end)
    yield {"ix": ix, "freq": freq, "plain": plain, "start": start, "end": end}
    ix.close()


@pytest.mark.parametrize("t,V,F", PARAMS)
def test_noisy_reads_against_the_helper_over_the_oracle(noisy, t, V, F):
    c = noisy
    want = _want(c["freq"], c["plain"], c["start"], c["end"], t, V, F)
    rec = want[1]
    hist = np.bincount(rec["status"], minlength=7)
    print((t, V, F), "status", hist.tolist(), "fixes", int(rec["fixes"].sum()), "n0", int(rec["n0"].sum()), "nM", int(rec["nM"].sum()))
    if F:
        assert (hist[:4] >= 50).all() and rec["n0"].sum() >= 50 and rec["nM"].sum() >= 50, hist
    else:
        assert hist[R.CLEAN] >= 50 and hist[R.UNFIXED] >= 50 and not rec["fixes"].any()
    _same(_dev(c["ix"], c["plain"], c["start"], c["end"], t, V, F), want, (t, V, F))
    assert len(c["start"]) == 4000 and set((c["end"] - c["start"]).tolist()) == set(K.LENGTHS)


def _small23(gold):
    p = os.path.join(gold, "small23", "small23")
    return Index.open_23(p + ".pf", p + ".tf.bin", p + ".kmers.bin"), K.MemoFreq(D.oracle_freq(O.OracleIndex23.from_prefix(p)))


def _small23_reads(gold, n, seed=4):
    """n reads of the golden reads file with 0 .. 3 substitutions each and a few 'N', lower-case bases and '~', one newline behind each"""
    rng = np.random.default_rng(seed)
    lines = open(os.path.join(gold, "small23", "small23.reads"), "rb").read().split(b"\n")[:n]
    a = np.frombuffer(b"\n".join(lines) + b"\n", np.uint8).copy().reshape(n, 151)
    for r in range(n):
        for p in rng.integers(0, 150, r % 4):
            a[r, p] = b"ACGT"[(b"ACGT".index(a[r, p]) + 1) % 4] if a[r, p] in b"ACGT" else a[r, p]
        if r % 9 == 0:
            a[r, rng.integers(0, 150)] = (ord("N"), ord("a"), ord("~"))[(r // 9) % 3]
    start = np.arange(n, dtype=np.uint64) * np.uint64(151)
    return a.reshape(-1), start, start + np.uint64(150)


def test_shapes_and_ranges(gold):
    import torch
    ix, freq = _small23(gold)
    with ix:
        big, _, _ = _small23_reads(gold, 60)
        long_read = big[big != 10][:4097]                          # 4097 bases of the golden reads, with their planted errors
        for m in (1, 3, 4, 5, 257):
            buf, start, end = _small23_reads(gold, m, seed=m)
            buf = np.concatenate([np.full(3, 0xEE, np.uint8), buf, np.full(7, 0xEE, np.uint8)])          # odd offsets, canaries around
            start, end = start + np.uint64(3), end + np.uint64(3)
            buf[end.astype(np.int64)] = 0xEE                       # and between the reads
            want = _want(freq, buf, start, end, 1, 8, 4)
            _same(_dev(ix, buf, start, end, 1, 8, 4), want, m)
            assert (want[0][end.astype(np.int64)] == 0xEE).all()
        # 4096 and 4097 bases, short reads, bad ranges among good ones
        buf = np.concatenate([long_read[:4096], [0xEE], long_read, [0xEE], long_read[:22], [0xEE], long_read[100:123], [0xEE], long_read[:10]]).astype(np.uint8)
        n = buf.shape[0]
        o = [0, 4097, 8195, 8218, 8242]
        start = np.array([o[0], o[1], o[2], o[3], o[4], 50, n - 30, 0, 1 << 63, o[4]], np.uint64)
        end = np.array([4096, o[1] + 4097, o[2] + 22, o[3] + 23, n, 40, n + 1, (1 << 64) - 1, (1 << 63) + 150, o[4]], np.uint64)
        want = _want(freq, buf, start, end, 1, 8, 4)
        assert want[1]["status"][1:].tolist() == [R.TOO_LONG, R.SHORT, want[1]["status"][3], R.SHORT, R.BAD_RANGE, R.BAD_RANGE, R.BAD_RANGE, R.BAD_RANGE, R.SHORT]
        assert want[1]["status"][0] in (R.FIXED, R.PARTIAL, R.UNFIXED) and want[1]["weak_before"][0] > 0
        got = _dev(ix, buf, start, end, 1, 8, 4)
        _same(got, want, "ranges")
        assert np.array_equal(got[0][4097:], buf[4097:])          # TOO_LONG, SHORT and BAD_RANGE reads and every canary untouched
        # the host form: the same answers, overlapping or descending ranges refused
        good = np.array([0, 2, 3], np.intp)
        h = ix.fix_reads(buf, start[good], end[good], 1, 8, 4)
        assert np.array_equal(_rows(h[1]), _rows(want[1])[good]) and np.array_equal(h[0], want[0])
        for s2, e2 in (([0, 100], [150, 250]), ([200, 0], [350, 150]), ([0, 200, 149], [150, 100, 300])):
            with pytest.raises(_lib.AixError) as err:
                ix.fix_reads(buf, np.array(s2, np.uint64), np.array(e2, np.uint64))
            assert err.value.status == _lib.AIX_ERR_ARG
        # empty batch, bad V / F, missing pointers
        e64 = torch.zeros(0, dtype=torch.int64, device="cuda")
        rec, fp, fo = ix.fix_reads_t(torch.zeros(10, dtype=torch.uint8, device="cuda"), e64, e64)
        assert rec.shape == (0, 8) and fp.shape == (0, 4) and fo.shape == (0, 4)
        assert ix.fix_reads(b"", [], [])[1].shape == (0,)
        L_ = _lib.lib()
        assert L_.aix_reads_fix(ix._h, None, 0, None, None, 0, 1, 8, 4, None, None, None) == 0
        assert L_.aix_reads_fix_dev(ix._h, None, 0, None, None, 0, 1, 8, 4, None, None, None, None) == 0
        z = np.zeros(64, np.uint64)
        p = z.ctypes.data_as(vp)
        ARG = _lib.AIX_ERR_ARG
        for V, F in ((0, 4), (17, 4), (8, 17)):
            assert L_.aix_reads_fix(ix._h, p, 8, p, p, 1, 1, V, F, p, p, p) == ARG
            assert L_.aix_reads_fix_dev(ix._h, p, 8, p, p, 1, 1, V, F, p, p, p, None) == ARG
        assert L_.aix_reads_fix(ix._h, None, 8, p, p, 1, 1, 8, 4, p, p, p) == ARG and L_.aix_reads_fix(ix._h, p, 8, p, p, 1, 1, 8, 4, None, p, p) == ARG
        assert L_.aix_reads_fix(ix._h, p, 8, p, p, 1, 1, 8, 4, p, None, p) == ARG and L_.aix_reads_fix_dev(ix._h, p, 8, p, p, 1, 1, 8, 4, p, p, None, None) == ARG
        assert L_.aix_reads_fix(ix._h, p, 8, p, p, 1, 1, 8, 0, p, None, None) == 0          # one empty read: SHORT
        assert L_.aix_reads_fix(None, p, 8, p, p, 1, 1, 8, 4, p, p, p) == ARG
        # a buffer of no bytes: every range is empty, the host form answers SHORT as the device form does
        z3, r3 = np.zeros(3, np.uint64), np.zeros(3, dtype=_lib.readfix_dtype())
        assert L_.aix_reads_fix(ix._h, p, 0, z3.ctypes.data_as(vp), z3.ctypes.data_as(vp), 3, 1, 8, 0, r3.ctypes.data_as(vp), None, None) == 0
        assert r3["status"].tolist() == [R.SHORT] * 3
    from pf13 import pf13_path
    with Index.open_13(pf13_path(), None) as ix13:
        assert L_.aix_reads_fix(ix13._h, p, 8, p, p, 1, 1, 8, 4, p, p, p) == _lib.AIX_ERR_MODE
        assert L_.aix_reads_fix_dev(ix13._h, p, 8, p, p, 1, 1, 8, 4, p, p, p, None) == _lib.AIX_ERR_MODE


def test_the_golden_index_and_every_switch(gold, monkeypatch):
    """small23 stores keys of either strand; the answers do not depend on the verification table and its lane width, the absence
    filter and its three policies, fingerprints, early exit or the canonical fast path."""
    ix, freq = _small23(gold)
    with ix:
        assert not ix.canonical_only
        buf, start, end = _small23_reads(gold, 300)
        wants = {prm: _want(freq, buf, start, end, *prm) for prm in ((1, 8, 4), (3, 4, 16))}
        # the golden index holds a part of these reads' 23-mers only: no read is clean, most boundaries have no candidate
        assert all(w[1]["fixes"].sum() > 50 and w[1]["n0"].sum() > 50 and len(set(w[1]["status"].tolist())) >= 2 for w in wants.values())
        n = 0
        for policy in ("0", "1", "2"):
            monkeypatch.setenv("AIX_DBJ_FILTER", policy)
            for table, lanes in ((True, 8), (True, 1), (False, 0)):
                for filt in (True, False):
                    for fp, ee, canon in ((True, True, True), (False, False, False), (True, False, True)):
                        ix.set_bucket_table(table, lanes)
                        ix.set_absence_filter(filt)
                        ix.set_fingerprint_filter(fp)
                        ix.set_early_exit(ee)
                        ix.set_canonical_fastpath(canon)
                        prm = (1, 8, 4) if n % 2 else (3, 4, 16)
                        _same(_dev(ix, buf, start, end, *prm), wants[prm], (policy, table, lanes, filt, fp, ee, canon))
                        n += 1
        for lanes in (4, 2):
            ix.set_bucket_table(True, lanes)
            _same(_dev(ix, buf, start, end, 1, 8, 4), wants[(1, 8, 4)], lanes)
        assert n == 54


def test_correct_reads_file(gold, small23_prefix, tmp_path):
    ai = AIndex.load_from_prefix(small23_prefix)
    try:
        buf, start, end = _small23_reads(gold, 40)
        lines = buf.tobytes().split(b"\n")[:40]
        text = b"\n".join([lines[0] + b"~" + lines[1], b"", lines[2], lines[3][:22] + b"~" + lines[4] + b"~", lines[5]] + lines[6:])   # no final newline
        src, dst = str(tmp_path / "in.reads"), str(tmp_path / "out.reads")
        open(src, "wb").write(text)
        for chunk in (64 << 20, 100):
            totals = ai.correct_reads_file(src, dst, 1, 8, 4, chunk_bytes=chunk)
            got = open(dst, "rb").read()
            assert len(got) == len(text)
            a, b = np.frombuffer(text, np.uint8), np.frombuffer(got, np.uint8)
            sep = (a == 10) | (a == 126)
            assert np.array_equal(a[sep], b[sep]) and np.array_equal(sep, (b == 10) | (b == 126))
            mates = [m for line in text.decode().split("\n") for m in line.split("~")]
            fixed, rec = ai.correct_reads(mates, 1, 8, 4)
            assert [m for line in got.decode().split("\n") for m in line.split("~")] == fixed
            assert totals["reads"] == len(mates) == sum(totals[k] for k in _lib.FIX_NAMES)
            assert [totals[k] for k in _lib.FIX_NAMES] == np.bincount(rec["status"], minlength=7).tolist()
            assert (totals["simple_ok"], totals["simple_n0"], totals["simple_nM"]) == (int(rec["fixes"].sum()), int(rec["n0"].sum()), int(rec["nM"].sum()))
            assert totals["simple_ok"] > 10 and totals["short"] >= 3 and (a != b).sum() == totals["simple_ok"]
    finally:
        ai._wrapper.close()
