"""The absence filter keyed by the k-mer code (aix_device.hpp: filter_key) on the device: the filter's words against the numpy
restatement (filterkey_ref.py), answers of the direct and the binned path against the CPU oracle, pass B of the binned path letting
through exactly the filter's positives, and the probe with the filter on and off. Small synthetic canonical indexes: 4092 keys (1024
filter words), ~300 000 keys at 64 filter bits per key (more than 2^18 words, partial last slice), and 1, 3 and 5 keys (1, 1 and 2
words). Every output buffer starts as 0xFFFFFFFF. Bit-exact."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import filterkey_ref as F
import oracle_lib as O
from aindex_amd import _lib, builder, synth
from aindex_amd.engine import Index

NS = (1, 63, 64, 65, 4097, 70001)
NMAX = max(NS)
BINS = (2, 8, 64)
N_KEYS = 4092                                  # 16 filter bits per key: floor(4092 / 4) + 1 = 1024 filter words
TINY_KEYS = (1, 3, 5)
KINDS = ("absent", "present", "half", "dirty", "neighbour")


def build_index(d, name, keys, counts, env=None):
    """MPHF (builder.build_pf_codes, the CPU construction), product-side scatter, files, handle and oracle of a true-canonical key
    set. `env` is set around Index.open_23 only."""
    n = keys.shape[0]
    pf = builder.build_pf_codes(keys, 23)
    prefix = str(d / name)
    open(prefix + ".pf", "wb").write(pf)
    flatk = np.ascontiguousarray(synth.decode_kmers(keys, 23)).reshape(-1)
    checker = np.empty(n, dtype=np.uint64)
    tf = np.empty(n, dtype=np.uint32)
    vp = _lib.vp
    pfa = np.frombuffer(pf, dtype=np.uint8)
    _lib.check(_lib.lib().aix_index_scatter(pfa.ctypes.data_as(vp), pfa.shape[0], flatk.ctypes.data_as(vp), counts.ctypes.data_as(vp), n, 0,
                                            checker.ctypes.data_as(vp), tf.ctypes.data_as(vp)))
    checker.tofile(prefix + ".kmers.bin")
    tf.tofile(prefix + ".tf.bin")
    saved = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        ix = Index.open_23(prefix + ".pf", prefix + ".tf.bin", prefix + ".kmers.bin")
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    return ix, O.OracleIndex23.from_prefix(prefix)


def distinct_counts(seed, n):
    """a tf of its own for (nearly) every key, so that an answer written to another query's slot shows"""
    return (synth.sm64(seed, np.arange(n, dtype=np.uint64)) % np.uint64(1 << 20) + np.uint64(1)).astype(np.uint32)


def make_batches(keys, nmax):
    """(nmax, 23) ASCII queries: uniform random k-mers, keys on both strands, the two interleaved, the interleaving with other bytes,
    and one-substitution neighbours of keys (what reads with sequencing errors ask for)"""
    ar = np.arange(nmax, dtype=np.uint64)
    codes = keys[(synth.sm64(3, ar) % np.uint64(keys.shape[0])).astype(np.int64)]
    flip = (synth.sm64(4, ar) & np.uint64(1)).astype(bool)
    present = synth.decode_kmers(np.where(flip, synth.revcomp_codes(codes, 23), codes), 23)
    absent = synth.random_kmers_ascii(5, nmax, 23)
    half = np.where((ar & np.uint64(1)).astype(bool)[:, None], present, absent)
    dirty = half.copy()
    for start, step, byte in ((0, 97, ord("N")), (3, 131, ord("U")), (7, 211, ord("*")), (11, 389, 0)):
        idx = np.arange(start, nmax, step)
        dirty[idx, (idx * 7) % 23] = byte
    dirty[np.arange(5, nmax, 149)] |= 0x20                                                        # lower-case letters
    nb = F.neighbours(keys, nmax)
    neighbour = synth.decode_kmers(np.where(flip, synth.revcomp_codes(nb, 23), nb), 23)           # either strand of the neighbour
    return {"absent": absent, "present": present, "half": half, "dirty": dirty, "neighbour": neighbour}


def finish_case(ix, orc, keys, bits, batches):
    flat = {k: np.ascontiguousarray(v).reshape(-1) for k, v in batches.items()}
    want = {k: orc.tf_batch(v) for k, v in flat.items()}                                          # computed once; a batch of N = its first N queries
    dev = {k: torch.from_numpy(v.copy()).cuda() for k, v in flat.items()}
    nwords = ix.info["absence_filter_words"]
    assert nwords == F.filter_words(keys.shape[0], bits)
    found = orc.tf_batch(np.ascontiguousarray(synth.decode_kmers(keys, 23)).reshape(-1)) > 0     # every tf is >= 1: the keys the oracle finds
    w, m = F.new_key(keys[found], nwords)
    return {"ix": ix, "keys": keys, "rows": batches, "flat": flat, "want": want, "dev": dev, "nwords": nwords, "filter": F.build_filter(w, m, nwords)}


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("fk")
    keys, counts = synth.canonical_distinct(synth.genome_codes(29, 6000), 23)
    keys, counts = np.ascontiguousarray(keys[:N_KEYS]), np.ascontiguousarray(counts[:N_KEYS])
    ix, orc = build_index(d, "fk", keys, counts)
    c = finish_case(ix, orc, keys, 16, make_batches(keys, NMAX))
    assert ix.canonical_only and c["nwords"] == 1024 and c["want"]["present"].min() > 0
    yield c
    ix.close()


@pytest.fixture(scope="module")
def case_wide(tmp_path_factory):
    """~300 000 keys at 64 filter bits per key: n + 1 > 2^18 filter words"""
    d = tmp_path_factory.mktemp("fk_wide")
    keys, _ = synth.canonical_distinct(synth.genome_codes(37, 300_000), 23)
    keys = np.ascontiguousarray(keys)
    ix, orc = build_index(d, "wide", keys, distinct_counts(41, keys.shape[0]), env={"AIX_BLOOM_BITS": "64"})
    c = finish_case(ix, orc, keys, 64, make_batches(keys, NMAX))
    assert ix.canonical_only and c["nwords"] == keys.shape[0] + 1 and c["nwords"] > 2 ** 18 and c["want"]["present"].min() > 0
    yield c
    ix.close()


@pytest.fixture(scope="module")
def case_tiny(tmp_path_factory):
    d = tmp_path_factory.mktemp("fk_tiny")
    all_keys, _ = synth.canonical_distinct(synth.genome_codes(31, 200), 23)
    out = {}
    for nk in TINY_KEYS:
        keys = np.ascontiguousarray(all_keys[:nk])
        ix, orc = build_index(d, f"tiny{nk}", keys, distinct_counts(43, nk))
        out[nk] = finish_case(ix, orc, keys, 16, make_batches(keys, NMAX))
        assert ix.canonical_only and out[nk]["nwords"] == nk // 4 + 1
    yield out
    for c in out.values():
        c["ix"].close()


def every_case(request):
    return [("small", request.getfixturevalue("case")), ("wide", request.getfixturevalue("case_wide"))] + [
        (f"tiny{nk}", c) for nk, c in request.getfixturevalue("case_tiny").items()]


def lookup(ix, dq, n):
    out = torch.full((n,), -1, dtype=torch.int32, device=dq.device)                               # 0xFFFFFFFF everywhere
    ix.tf_ascii_t(dq[: 23 * n], out)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32)


def stats(ix):
    out = (C.c_uint64 * 4)()
    _lib.check(_lib.lib().aix_lookup_binned_stats(ix._h, C.cast(out, _lib.vp)))
    return dict(zip(("binned", "direct", "overflow", "survivors"), (int(x) for x in out)))


def slice_bytes_for(nwords, bins):
    """slices of ceil(nwords / bins) words: `bins` slices, or as many one-word slices as the filter has words"""
    return 8 * max(-(-nwords // bins), 1)


def filter_words_of(ix, nwords):
    out = np.full(nwords, 0xDEADBEEFDEADBEEF, dtype=np.uint64)
    st = _lib.lib().aix_debug_filter_words(ix._h, out.ctypes.data_as(_lib.vp), nwords)
    return st, out


def test_filter_bits(request):
    """the filter in HBM = the restatement's filter over the keys the oracle finds, bit for bit"""
    for name, c in every_case(request):
        st, got = filter_words_of(c["ix"], c["nwords"])
        assert st == 0, name
        assert np.array_equal(got, c["filter"]), (name, int((got != c["filter"]).sum()))
        assert got.any(), name
        for wrong in (c["nwords"] - 1, c["nwords"] + 1):                                           # a size that is not the filter's: refused, nothing written
            out = np.full(c["nwords"] + 1, 0xDEADBEEFDEADBEEF, dtype=np.uint64)
            assert _lib.lib().aix_debug_filter_words(c["ix"]._h, out.ctypes.data_as(_lib.vp), wrong) != 0, (name, wrong)
            assert (out == np.uint64(0xDEADBEEFDEADBEEF)).all(), (name, wrong)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("which", ["small", "wide"])
def test_answers(request, monkeypatch, which, kind):
    c = request.getfixturevalue("case" if which == "small" else "case_wide")
    ix, dq, want = c["ix"], c["dev"][kind], c["want"][kind]
    monkeypatch.setenv("AIX_LOOKUP_BINNED", "0")
    for n in NS:
        before = stats(ix)
        assert np.array_equal(lookup(ix, dq, n), want[:n]), (which, kind, "direct", n)
        assert stats(ix) == before
    monkeypatch.setenv("AIX_LOOKUP_BINNED", "2")
    for bins in BINS:
        monkeypatch.setenv("AIX_LOOKUP_SLICE_BYTES", str(slice_bytes_for(c["nwords"], bins)))
        for n in NS:
            before = stats(ix)
            got = lookup(ix, dq, n)
            after = stats(ix)
            assert after["binned"] == before["binned"] + 1 and after["direct"] == before["direct"], (which, kind, bins, n)
            assert np.array_equal(got, want[:n]), (which, kind, bins, n)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nk", TINY_KEYS)
def test_answers_tiny(case_tiny, monkeypatch, nk, kind):
    """filters of one and two words: one slice as wide as the filter, or one-word slices"""
    c = case_tiny[nk]
    ix, dq, want = c["ix"], c["dev"][kind], c["want"][kind]
    for mode, slice_bytes in (("0", None), ("2", None), ("2", 8)):
        monkeypatch.setenv("AIX_LOOKUP_BINNED", mode)
        if slice_bytes is None:
            monkeypatch.delenv("AIX_LOOKUP_SLICE_BYTES", raising=False)
        else:
            monkeypatch.setenv("AIX_LOOKUP_SLICE_BYTES", str(slice_bytes))
        for n in NS:
            assert np.array_equal(lookup(ix, dq, n), want[:n]), (nk, kind, mode, slice_bytes, n)


def expected_survivors(c, kind):
    """clean queries (23 bytes of ACGT) whose canonical code passes the restated filter, plus the queries with other bytes"""
    rows = c["rows"][kind]
    clean = np.isin(rows, np.frombuffer(b"ACGT", dtype=np.uint8)).all(axis=1)
    codes = F.canonical(synth.encode_kmers(rows[clean]))
    w, m = F.new_key(codes, c["nwords"])
    return int(F.passes(c["filter"], w, m).sum()) + int((~clean).sum())


# small: 8 slices of 128 words. wide: the default slice (2^17 words, 3 slices, the last one partial), 2^18-word slices (every bit of the
# record's word field) and 100 003-word slices (no power of two, slice-relative words above 2^16)
@pytest.mark.parametrize("kind", ["absent", "half", "neighbour", "dirty"])
@pytest.mark.parametrize("which,slice_bytes", [("small", 8 * 128), ("wide", None), ("wide", 2097152), ("wide", 8 * 100003)])
def test_pass_b_is_exact(request, monkeypatch, which, slice_bytes, kind):
    c = request.getfixturevalue("case" if which == "small" else "case_wide")
    ix = c["ix"]
    monkeypatch.setenv("AIX_LOOKUP_BINNED", "2")
    if slice_bytes is None:
        monkeypatch.delenv("AIX_LOOKUP_SLICE_BYTES", raising=False)
    else:
        monkeypatch.setenv("AIX_LOOKUP_SLICE_BYTES", str(slice_bytes))
    if which == "wide":
        # the premise is that no record overflows. A slice region is sized for an even share of the piece plus a quarter, and a batch this
        # small pays a partly filled chunk per slice and workgroup on top: the two full slices of three take 44 % each, the first of two
        # 87 %. The test switch lifts the regions to the size of the piece.
        monkeypatch.setenv("AIX_LOOKUP_TEST_BIN_CAP", str(1 << 20))
    before = stats(ix)
    got = lookup(ix, c["dev"][kind], NMAX)
    after = stats(ix)
    want = expected_survivors(c, kind)
    print(which, slice_bytes, kind, "survivors", after["survivors"] - before["survivors"], "expected", want)
    assert np.array_equal(got, c["want"][kind])
    assert after["binned"] == before["binned"] + 1 and after["overflow"] == before["overflow"]
    assert after["survivors"] - before["survivors"] == want


@pytest.mark.parametrize("kind", ["half", "dirty"])
def test_through_the_probe(case, monkeypatch, kind):
    """every kernel that reaches the filter through probe23_wave: the same results with the filter on and off, and the oracle's tf"""
    ix, flat = case["ix"], case["flat"][kind]
    monkeypatch.setenv("AIX_LOOKUP_BINNED", "0")
    seqs = [flat[: 23 * 1000].tobytes(), flat[23 * 1000: 23 * 1003].tobytes(), flat[23 * 2000: 23 * 2000 + 22].tobytes(), flat[23 * 3000: 23 * 4097].tobytes()]
    res = {}
    for on in (True, False):
        ix.set_absence_filter(on)
        try:
            assert (ix.info["absence_filter_words"] > 0) == on
            kid, strand = ix.kid_strand_ascii(flat)
            res[on] = {"tf": ix.tf_ascii(flat), "kid": kid, "strand": strand, "total": ix.total_ascii(flat), "coverage": np.concatenate(ix.coverage(seqs))}
        finally:
            ix.set_absence_filter(True)
    assert np.array_equal(res[True]["tf"], case["want"][kind])
    for what in res[True]:
        assert np.array_equal(res[True][what], res[False][what]), (kind, what)
