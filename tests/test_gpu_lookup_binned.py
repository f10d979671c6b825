"""The binned tf lookup (aix_lookup_binned.hip: bin by filter slice, filter from L2, survivors through the probe) against the direct
kernel and the CPU oracle, on a small synthetic canonical index whose absence filter has exactly 1024 words: slices of 512, 128 and
16 words give 2, 8 and 64 bins. Every output buffer starts as 0xFFFFFFFF. Bit-exact."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle_lib as O
from aindex_amd import _lib, builder, synth
from aindex_amd.engine import Index

NS = (1, 63, 64, 65, 4097, 70001)
NMAX = max(NS)
BINS = (2, 8, 64)
N_KEYS = 4092                                  # 16 filter bits per key: floor(4092 / 4) + 1 = 1024 filter words


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("binned")
    g = synth.genome_codes(29, 6000)
    keys, counts = synth.canonical_distinct(g, 23)
    assert keys.shape[0] >= N_KEYS
    keys, counts = np.ascontiguousarray(keys[:N_KEYS]), np.ascontiguousarray(counts[:N_KEYS])
    pf = builder.build_pf_codes(keys, 23)
    prefix = str(d / "binned")
    open(prefix + ".pf", "wb").write(pf)
    flatk = np.ascontiguousarray(synth.decode_kmers(keys, 23)).reshape(-1)
    checker = np.empty(N_KEYS, dtype=np.uint64)
    tf = np.empty(N_KEYS, dtype=np.uint32)
    vp = _lib.vp
    pfa = np.frombuffer(pf, dtype=np.uint8)
    _lib.check(_lib.lib().aix_index_scatter(pfa.ctypes.data_as(vp), pfa.shape[0], flatk.ctypes.data_as(vp), counts.ctypes.data_as(vp), N_KEYS, 0,
                                            checker.ctypes.data_as(vp), tf.ctypes.data_as(vp)))
    checker.tofile(prefix + ".kmers.bin")
    tf.tofile(prefix + ".tf.bin")
    ix = Index.open_23(prefix + ".pf", prefix + ".tf.bin", prefix + ".kmers.bin")
    assert ix.canonical_only and ix.info["absence_filter_words"] == 1024
    orc = O.OracleIndex23.from_prefix(prefix)

    ar = np.arange(NMAX, dtype=np.uint64)
    codes = keys[(synth.sm64(3, ar) % np.uint64(N_KEYS)).astype(np.int64)]
    flip = (synth.sm64(4, ar) & np.uint64(1)).astype(bool)
    present = synth.decode_kmers(np.where(flip, synth.revcomp_codes(codes, 23), codes), 23)      # both strands
    absent = synth.random_kmers_ascii(5, NMAX, 23)
    half = np.where((ar & np.uint64(1)).astype(bool)[:, None], present, absent)
    dirty = half.copy()
    for start, step, byte in ((0, 97, ord("N")), (3, 131, ord("U")), (7, 211, ord("*")), (11, 389, 0)):
        idx = np.arange(start, NMAX, step)
        dirty[idx, (idx * 7) % 23] = byte
    dirty[np.arange(5, NMAX, 149)] |= 0x20                                                        # lower-case letters
    batches = {"absent": absent, "present": present, "half": half, "same_present": np.repeat(present[:1], NMAX, axis=0),
               "same_absent": np.repeat(absent[:1], NMAX, axis=0), "dirty": dirty}
    batches = {k: np.ascontiguousarray(v).reshape(-1) for k, v in batches.items()}
    want = {k: orc.tf_batch(v) for k, v in batches.items()}                                       # computed once; a batch of N = its first N queries
    assert want["present"].min() > 0 and int((want["absent"] != 0).sum()) < NMAX // 100
    dev = {k: torch.from_numpy(v.copy()).cuda() for k, v in batches.items()}
    yield {"ix": ix, "want": want, "dev": dev}
    ix.close()


def lookup(ix, dq, n):
    out = torch.full((n,), -1, dtype=torch.int32, device=dq.device)                               # 0xFFFFFFFF everywhere
    ix.tf_ascii_t(dq[: 23 * n], out)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32)


def stats(ix):
    out = (C.c_uint64 * 4)()
    _lib.check(_lib.lib().aix_lookup_binned_stats(ix._h, C.cast(out, _lib.vp)))
    return dict(zip(("binned", "direct", "overflow", "survivors"), (int(x) for x in out)))


def set_bins(monkeypatch, bins):
    monkeypatch.setenv("AIX_LOOKUP_SLICE_BYTES", str(8 * (1024 // bins)))


@pytest.mark.parametrize("bins", BINS)
@pytest.mark.parametrize("kind", ["absent", "present", "half", "same_present", "same_absent", "dirty"])
def test_paths_agree(case, monkeypatch, kind, bins):
    ix, dq, want = case["ix"], case["dev"][kind], case["want"][kind]
    set_bins(monkeypatch, bins)
    for n in NS:
        before = stats(ix)
        monkeypatch.setenv("AIX_LOOKUP_BINNED", "2")
        binned = lookup(ix, dq, n)
        after = stats(ix)
        assert after["binned"] == before["binned"] + 1 and after["direct"] == before["direct"]
        monkeypatch.setenv("AIX_LOOKUP_BINNED", "0")
        direct = lookup(ix, dq, n)
        assert stats(ix) == after                                                                 # switched off: the binned path is not entered
        assert np.array_equal(direct, want[:n]), (kind, bins, n)
        assert np.array_equal(binned, want[:n]), (kind, bins, n)


@pytest.mark.parametrize("kind", ["absent", "half", "same_absent", "dirty"])
def test_overflow_goes_to_the_probe(case, monkeypatch, kind):
    ix, dq, want = case["ix"], case["dev"][kind], case["want"][kind]
    set_bins(monkeypatch, 8)
    monkeypatch.setenv("AIX_LOOKUP_BINNED", "2")
    for cap in (0, 256, 2048):                                                                    # expected load of a bin: 70 001 / 8 = 8 750 records
        monkeypatch.setenv("AIX_LOOKUP_TEST_BIN_CAP", str(cap))
        before = stats(ix)
        got = lookup(ix, dq, NMAX)
        after = stats(ix)
        assert np.array_equal(got, want), (kind, cap)
        assert after["overflow"] > before["overflow"]
        assert after["survivors"] - before["survivors"] >= after["overflow"] - before["overflow"]


@pytest.mark.parametrize("piece", [1000, 4096])
def test_piece_cuts(case, monkeypatch, piece):
    ix = case["ix"]
    set_bins(monkeypatch, 8)
    monkeypatch.setenv("AIX_LOOKUP_BINNED", "2")
    monkeypatch.setenv("AIX_LOOKUP_PIECE", str(piece))
    for kind in ("absent", "dirty"):
        for n in (4097, NMAX):
            before = stats(ix)
            got = lookup(ix, case["dev"][kind], n)
            assert np.array_equal(got, case["want"][kind][:n]), (kind, piece, n)
            assert stats(ix)["binned"] - before["binned"] == -(-n // piece)


def test_gate_picks_the_path(case, monkeypatch):
    ix = case["ix"]
    set_bins(monkeypatch, 8)
    monkeypatch.setenv("AIX_LOOKUP_BINNED", "1")
    monkeypatch.setenv("AIX_LOOKUP_BINNED_MIN", "0")
    for kind, field in (("absent", "binned"), ("half", "direct"), ("present", "direct"), ("same_absent", "binned")):
        for n in (65, NMAX):
            before = stats(ix)
            got = lookup(ix, case["dev"][kind], n)
            after = stats(ix)
            assert np.array_equal(got, case["want"][kind][:n]), (kind, n)
            other = "direct" if field == "binned" else "binned"
            assert after[field] == before[field] + 1 and after[other] == before[other], (kind, n)
    monkeypatch.delenv("AIX_LOOKUP_BINNED_MIN")                                                   # below the default minimum: not a candidate at all
    before = stats(ix)
    assert np.array_equal(lookup(ix, case["dev"]["absent"], NMAX), case["want"]["absent"])
    assert stats(ix) == before


def test_fall_back_to_the_direct_path(case, monkeypatch, small23_prefix):
    monkeypatch.setenv("AIX_LOOKUP_BINNED", "2")
    ix, dq, want = case["ix"], case["dev"]["dirty"], case["want"]["dirty"]
    for off, on in ((lambda: ix.set_bucket_table(False), lambda: ix.set_bucket_table(True)),
                    (lambda: ix.set_absence_filter(False), lambda: ix.set_absence_filter(True)),
                    (lambda: ix.set_canonical_fastpath(False), lambda: ix.set_canonical_fastpath(True))):
        before = stats(ix)
        off()
        try:
            assert np.array_equal(lookup(ix, dq, NMAX), want)
            assert stats(ix) == before
        finally:
            on()
    # an index built with the reference's tools: the stored set is not all-canonical
    orc = O.OracleIndex23.from_prefix(small23_prefix)
    rng = np.random.default_rng(7)
    keys = np.fromfile(small23_prefix + ".kmers.bin", dtype=np.uint64)
    q = np.concatenate([synth.decode_kmers(keys[rng.integers(0, keys.shape[0], 2000)], 23), synth.random_kmers_ascii(9, 2097, 23)]).reshape(-1)
    with Index.open_23(small23_prefix + ".pf", small23_prefix + ".tf.bin", small23_prefix + ".kmers.bin") as gx:
        assert not gx.canonical_only
        got = lookup(gx, torch.from_numpy(q.copy()).cuda(), 4097)
        assert np.array_equal(got, orc.tf_batch(q))
        assert stats(gx) == {"binned": 0, "direct": 0, "overflow": 0, "survivors": 0}


def test_two_streams_share_the_workspace(case, monkeypatch):
    ix = case["ix"]
    set_bins(monkeypatch, 8)
    monkeypatch.setenv("AIX_LOOKUP_BINNED", "2")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    outs = []
    for s, kind in ((s1, "absent"), (s2, "dirty"), (s1, "half"), (s2, "same_absent")):           # issued back to back, no synchronisation between them
        with torch.cuda.stream(s):
            out = torch.full((NMAX,), -1, dtype=torch.int32, device="cuda")
            ix.tf_ascii_t(case["dev"][kind], out)
            outs.append((kind, out))
    torch.cuda.synchronize()
    for kind, out in outs:
        assert np.array_equal(out.cpu().numpy().view(np.uint32), case["want"][kind]), kind
