"""The binned tf lookup (aix_lookup_binned.hip: bin by filter slice, filter from L2, survivors through the probe) against the direct
kernel and the CPU oracle, on a small synthetic canonical index whose absence filter has exactly 1024 words: slices of 512, 128 and
16 words give 2, 8 and 64 bins. Every output buffer starts as 0xFFFFFFFF. Bit-exact.

Below the first group of tests: batches of 2^23 + 1000 queries gathered on the device from the 70 001 oracle-checked rows (pass-A
workgroups that run several tiles, pass-B workgroups that flush inside their loop, a slice region that overflows at its real
capacity), slice widths that are no power of two, 256 and 257 slices, a filter of more than 2^18 words (all 18 bits of the record's
word field), filters of one and two words, and a piece of 2^27 queries (all 27 bits of the record's index field)."""
import ctypes as C
import os

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


def build_index(d, name, keys, counts, env=None):
    """MPHF (builder.build_pf_codes, the CPU construction: 2 s for 300 000 keys, and its bytes do not depend on the device),
    product-side scatter, files, handle and oracle of a true-canonical key set. `env` is set around Index.open_23 only."""
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


def base_batches(keys, nmax):
    """(nmax, 23) ASCII queries: keys on both strands, uniform random k-mers, the two interleaved, and the interleaving with other bytes"""
    ar = np.arange(nmax, dtype=np.uint64)
    codes = keys[(synth.sm64(3, ar) % np.uint64(keys.shape[0])).astype(np.int64)]
    flip = (synth.sm64(4, ar) & np.uint64(1)).astype(bool)
    present = synth.decode_kmers(np.where(flip, synth.revcomp_codes(codes, 23), codes), 23)      # both strands
    absent = synth.random_kmers_ascii(5, nmax, 23)
    half = np.where((ar & np.uint64(1)).astype(bool)[:, None], present, absent)
    dirty = half.copy()
    for start, step, byte in ((0, 97, ord("N")), (3, 131, ord("U")), (7, 211, ord("*")), (11, 389, 0)):
        idx = np.arange(start, nmax, step)
        dirty[idx, (idx * 7) % 23] = byte
    dirty[np.arange(5, nmax, 149)] |= 0x20                                                        # lower-case letters
    return {"absent": absent, "present": present, "half": half, "dirty": dirty}


def finish_case(ix, orc, batches):
    batches = {k: np.ascontiguousarray(v).reshape(-1) for k, v in batches.items()}
    want = {k: orc.tf_batch(v) for k, v in batches.items()}                                       # computed once; a batch of N = its first N queries
    dev = {k: torch.from_numpy(v.copy()).cuda() for k, v in batches.items()}
    want_dev = {k: torch.from_numpy(v.view(np.int32).copy()).cuda() for k, v in want.items()}
    return {"ix": ix, "want": want, "dev": dev, "want_dev": want_dev}


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("binned")
    g = synth.genome_codes(29, 6000)
    keys, counts = synth.canonical_distinct(g, 23)
    assert keys.shape[0] >= N_KEYS
    keys, counts = np.ascontiguousarray(keys[:N_KEYS]), np.ascontiguousarray(counts[:N_KEYS])
    ix, orc = build_index(d, "binned", keys, counts)
    assert ix.canonical_only and ix.info["absence_filter_words"] == 1024
    b = base_batches(keys, NMAX)
    batches = {"absent": b["absent"], "present": b["present"], "half": b["half"], "same_present": np.repeat(b["present"][:1], NMAX, axis=0),
               "same_absent": np.repeat(b["absent"][:1], NMAX, axis=0), "dirty": b["dirty"]}
    c = finish_case(ix, orc, batches)
    assert c["want"]["present"].min() > 0 and int((c["want"]["absent"] != 0).sum()) < NMAX // 100
    yield c
    ix.close()


def distinct_counts(seed, n):
    """a tf of its own for (nearly) every key, so that an answer written to another query's slot shows"""
    return (synth.sm64(seed, np.arange(n, dtype=np.uint64)) % np.uint64(1 << 20) + np.uint64(1)).astype(np.uint32)


@pytest.fixture(scope="module")
def case_wide(tmp_path_factory):
    """~300 000 keys at 64 filter bits per key: a filter of n + 1 > 2^18 words. The default slice (2^17 words) gives 3 bins, the last
    one partial; 2^18-word slices use every bit of the record's word field."""
    d = tmp_path_factory.mktemp("binned_wide")
    keys, _ = synth.canonical_distinct(synth.genome_codes(37, 300_000), 23)
    keys = np.ascontiguousarray(keys)
    ix, orc = build_index(d, "wide", keys, distinct_counts(41, keys.shape[0]), env={"AIX_BLOOM_BITS": "64"})
    assert ix.canonical_only and ix.info["absence_filter_words"] == keys.shape[0] + 1 and ix.info["absence_filter_words"] > 2 ** 18
    c = finish_case(ix, orc, base_batches(keys, NMAX))
    assert c["want"]["present"].min() > 0 and int((c["want"]["absent"] != 0).sum()) < NMAX // 100
    yield c
    ix.close()


TINY_KEYS = (1, 3, 5)


@pytest.fixture(scope="module")
def case_tiny(tmp_path_factory):
    """indexes of 1, 3 and 5 keys: filters of 1, 1 and 2 words (16 bits per key), so a slice is 1 or 2 words wide"""
    d = tmp_path_factory.mktemp("binned_tiny")
    all_keys, _ = synth.canonical_distinct(synth.genome_codes(31, 200), 23)
    out = {}
    for nk in TINY_KEYS:
        keys = np.ascontiguousarray(all_keys[:nk])
        ix, orc = build_index(d, f"tiny{nk}", keys, distinct_counts(43, nk))
        assert ix.canonical_only and ix.info["absence_filter_words"] == nk // 4 + 1
        q = np.concatenate([synth.decode_kmers(keys, 23), synth.decode_kmers(synth.revcomp_codes(keys, 23), 23), synth.random_kmers_ascii(47, 200, 23)])
        stained = np.repeat(q[:1], 4, axis=0)                                                      # a key with one other byte, and in lower case
        for j, byte in enumerate((ord("N"), ord("*"), 0)):
            stained[j, 5 * j + 1] = byte
        stained[3] |= 0x20
        q = np.ascontiguousarray(np.concatenate([q[:1], stained, q[1:]])).reshape(-1)
        want = orc.tf_batch(q)
        assert np.count_nonzero(want) >= 2 * nk
        out[nk] = {"ix": ix, "want": want, "dq": torch.from_numpy(q.copy()).cuda()}
    yield out
    for c in out.values():
        c["ix"].close()


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


# ------------------------------------------------------------------------------------------------
# Batches gathered on the device from the NMAX oracle-checked rows: the answer to row idx[i] of a base batch is want[idx[i]]
# ------------------------------------------------------------------------------------------------
N_BIG = 2 ** 23 + 1000              # 2049 tiles of 4096 on the 768 workgroups of pass A: two or three tiles each, the last one ragged
PASS_A_GRID, TILE = 768, 4096       # LB_GRID_A, LB_TILE
PASS_B_GRID, FLUSH_AT = 2048, 3584  # LB_GRID_B, LB_SURV - LB_U * LB_FB: a pass-B workgroup that holds more survivors flushes inside its loop
assert N_BIG > PASS_A_GRID * TILE and N_BIG > PASS_B_GRID * FLUSH_AT and N_BIG % TILE


def lookup_dev(ix, dq, n):
    out = torch.full((n,), -1, dtype=torch.int32, device=dq.device)                               # 0xFFFFFFFF everywhere
    ix.tf_ascii_t(dq[: 23 * n], out)
    torch.cuda.synchronize()
    return out


def assert_same_dev(got, want, what):
    """compared on the device; only the first differing positions come back"""
    if torch.equal(got, want):
        return
    bad = torch.nonzero(got != want).reshape(-1)
    first = bad[:8]
    raise AssertionError(f"{what}: {bad.numel()} of {got.numel()} answers differ, first at {first.tolist()}: got "
                         f"{(got[first].cpu().numpy().view(np.uint32)).tolist()}, want {(want[first].cpu().numpy().view(np.uint32)).tolist()}")


def uniform_idx(seed, n):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    return torch.randint(0, NMAX, (n,), generator=gen, device="cuda")


def big_batch(c, kind, n=N_BIG):
    """(queries, expected answers) of n rows, both on the device"""
    rows = {k: v.view(NMAX, 23) for k, v in c["dev"].items()}
    want = c["want_dev"]
    if kind.startswith("same_"):                                                                   # every row the same k-mer
        base = kind[len("same_"):-len("_big")]
        return rows[base][:1].repeat(n, 1).reshape(-1), want[base][:1].repeat(n)
    if kind == "skew_big":                                                                         # 90 % one absent k-mer, 10 % uniform rows of `half`
        idx = uniform_idx(101, n)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(102)
        one = torch.rand(n, generator=gen, device="cuda") < 0.9
        q = rows["half"].index_select(0, idx)
        q[one] = rows["absent"][0]
        return q.reshape(-1), torch.where(one, want["absent"][0], want["half"][idx])
    base = kind[:-len("_big")]
    idx = uniform_idx(100 + sorted(rows).index(base), n)
    return rows[base].index_select(0, idx).reshape(-1), want[base][idx]


def delta(after, before):
    return {k: after[k] - before[k] for k in after}


@pytest.mark.parametrize("kind", ["present_big", "absent_big", "same_present_big", "skew_big", "dirty_big"])
def test_big_batches(case, monkeypatch, kind):
    """Pass A carries a slice's chunk, its fill and the fresh chunks from tile to tile (no workgroup of the tests above runs a second
    tile). present_big: nothing overflows, so all N_BIG records go through pass B and all of them pass; its grid has at most
    PASS_B_GRID workgroups and one that never flushes inside its loop hands over at most FLUSH_AT survivors at its end, so with
    N_BIG > PASS_B_GRID * FLUSH_AT at least one workgroup flushes inside the loop. same_present_big and skew_big: one slice region
    (about 1.5 M records under the real capacity formula) fills part-way through a tile and the rest goes to the survivor list."""
    ix = case["ix"]
    set_bins(monkeypatch, 8)
    monkeypatch.setenv("AIX_LOOKUP_BINNED", "2")
    dq, want = big_batch(case, kind)
    before = stats(ix)
    got = lookup_dev(ix, dq, N_BIG)
    d = delta(stats(ix), before)
    print(kind, d)
    assert d["binned"] == 1 and d["direct"] == 0
    assert_same_dev(got, want, kind)
    if kind == "present_big":
        assert d["overflow"] == 0 and d["survivors"] == N_BIG and N_BIG > PASS_B_GRID * FLUSH_AT  # the premises of the argument above
    if kind == "absent_big":
        assert d["overflow"] == 0
    if kind == "same_present_big":
        assert d["overflow"] > 0 and d["survivors"] == N_BIG
    if kind == "skew_big":
        assert d["overflow"] > 0


def test_big_piece_cuts(case, monkeypatch):
    """two pieces of several tiles per workgroup each; header, cursors and tickets are zeroed again between them"""
    ix = case["ix"]
    set_bins(monkeypatch, 8)
    monkeypatch.setenv("AIX_LOOKUP_BINNED", "2")
    monkeypatch.setenv("AIX_LOOKUP_PIECE", "5000000")
    assert 5000000 > PASS_A_GRID * TILE and N_BIG - 5000000 > PASS_A_GRID * TILE
    for kind in ("dirty_big", "same_present_big"):
        dq, want = big_batch(case, kind)
        before = stats(ix)
        got = lookup_dev(ix, dq, N_BIG)
        d = delta(stats(ix), before)
        assert d["binned"] == 2 and d["direct"] == 0, kind
        assert_same_dev(got, want, kind)


def test_big_gate(case, monkeypatch):
    """auto mode: the gated direct kernel and the binned kernels are both in the queue, and one of them returns at once"""
    ix = case["ix"]
    set_bins(monkeypatch, 8)
    monkeypatch.setenv("AIX_LOOKUP_BINNED", "1")
    monkeypatch.setenv("AIX_LOOKUP_BINNED_MIN", "0")
    for kind, field in (("absent_big", "binned"), ("present_big", "direct")):
        dq, want = big_batch(case, kind)
        before = stats(ix)
        got = lookup_dev(ix, dq, N_BIG)
        d = delta(stats(ix), before)
        assert d[field] == 1 and d["binned"] + d["direct"] == 1, (kind, d)
        assert_same_dev(got, want, kind)


# ------------------------------------------------------------------------------------------------
# slice geometry
# ------------------------------------------------------------------------------------------------
def set_slice(monkeypatch, slice_bytes):
    if slice_bytes is None:
        monkeypatch.delenv("AIX_LOOKUP_SLICE_BYTES", raising=False)                                # the default: 1 MiB
    else:
        monkeypatch.setenv("AIX_LOOKUP_SLICE_BYTES", str(slice_bytes))


# 341 words: 4 bins, the last of one word, and floor(2^32 / 341) * 341 < 2^32, so the quotient is one short at every multiple of 341;
# 1000 words: bins of 1000 and 24; 4 words: LB_MAXBINS = 256 bins exactly; 3 words: 342 bins, not taken; 1024 words and the default:
# one bin as wide as the filter
@pytest.mark.parametrize("slice_bytes,taken", [(8 * 341, 1), (8 * 1000, 1), (8 * 4, 1), (8 * 3, 0), (8 * 1024, 1), (None, 1)])
def test_slice_widths(case, monkeypatch, slice_bytes, taken):
    ix = case["ix"]
    set_slice(monkeypatch, slice_bytes)
    monkeypatch.setenv("AIX_LOOKUP_BINNED", "2")
    for kind in ("half", "dirty"):
        for n in (NMAX, 4097):
            before = stats(ix)
            got = lookup(ix, case["dev"][kind], n)
            d = delta(stats(ix), before)
            assert np.array_equal(got, case["want"][kind][:n]), (kind, slice_bytes, n)
            if taken:
                assert d["binned"] == 1 and d["direct"] == 0, (kind, slice_bytes, n)
            else:
                assert d == {"binned": 0, "direct": 0, "overflow": 0, "survivors": 0}, (kind, slice_bytes, n)


# the default slice: 2^17 words, 3 bins, the last one partial; 2 MiB: 2^18 words, 2 bins, slice-relative words up to 2^18 - 1;
# 100 003 words: no power of two, and slice-relative words above 2^16
@pytest.mark.parametrize("slice_bytes,bins", [(None, 3), (2097152, 2), (8 * 100003, 3)])
def test_wide_filter(case_wide, monkeypatch, slice_bytes, bins):
    ix = case_wide["ix"]
    nbloom = ix.info["absence_filter_words"]
    wps = (1 << 17) if slice_bytes is None else slice_bytes // 8
    assert -(-nbloom // wps) == bins and nbloom % wps                                              # the last slice is partial
    set_slice(monkeypatch, slice_bytes)
    monkeypatch.setenv("AIX_LOOKUP_BINNED", "2")
    for kind in ("present", "absent", "half", "dirty"):
        before = stats(ix)
        got = lookup(ix, case_wide["dev"][kind], NMAX)
        d = delta(stats(ix), before)
        assert d["binned"] == 1 and d["direct"] == 0, (kind, slice_bytes)
        assert np.array_equal(got, case_wide["want"][kind]), (kind, slice_bytes)


@pytest.mark.parametrize("kind", ["present_big", "absent_big"])
def test_wide_filter_big(case_wide, monkeypatch, kind):
    """the shipped geometry (1 MiB slices of a filter larger than one slice) with several tiles per pass-A workgroup"""
    ix = case_wide["ix"]
    set_slice(monkeypatch, None)
    monkeypatch.setenv("AIX_LOOKUP_BINNED", "2")
    dq, want = big_batch(case_wide, kind)
    before = stats(ix)
    got = lookup_dev(ix, dq, N_BIG)
    d = delta(stats(ix), before)
    print(kind, d)
    assert d["binned"] == 1 and d["direct"] == 0
    assert_same_dev(got, want, kind)


@pytest.mark.parametrize("slice_bytes", [None, 8])
@pytest.mark.parametrize("nk", TINY_KEYS)
def test_tiny_filters(case_tiny, monkeypatch, nk, slice_bytes):
    """filters of one and two words: one slice as wide as the filter, or one-word slices, for which the reciprocal is 0xFFFFFFFF"""
    c = case_tiny[nk]
    ix, total = c["ix"], c["want"].shape[0]
    set_slice(monkeypatch, slice_bytes)
    monkeypatch.setenv("AIX_LOOKUP_BINNED", "2")
    for n in (1, 65, total):
        before = stats(ix)
        got = lookup(ix, c["dq"], n)
        d = delta(stats(ix), before)
        assert d["binned"] == 1 and d["direct"] == 0, (nk, slice_bytes, n)
        assert np.array_equal(got, c["want"][:n]), (nk, slice_bytes, n)


@pytest.mark.slow
def test_full_piece(case_wide, monkeypatch):
    """2^27 + 4097 queries, alternately from `absent` and `present`: a piece of exactly 1 << LB_IDX_BITS queries, whose records use
    all 27 bits of the index field, then a second piece of 4097. The 3.1 GB of queries are built and compared on the device."""
    ix = case_wide["ix"]
    n, step = 2 ** 27 + 4097, 2 ** 24
    set_slice(monkeypatch, None)
    monkeypatch.setenv("AIX_LOOKUP_BINNED", "2")
    rows = torch.cat([case_wide["dev"]["absent"].view(NMAX, 23), case_wide["dev"]["present"].view(NMAX, 23)])
    answers = torch.cat([case_wide["want_dev"]["absent"], case_wide["want_dev"]["present"]])
    dq = torch.empty(23 * n, dtype=torch.uint8, device="cuda")
    want = torch.empty(n, dtype=torch.int32, device="cuda")
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        idx = uniform_idx(200 + lo // step, hi - lo) + NMAX * (torch.arange(lo, hi, device="cuda") & 1)
        dq[23 * lo: 23 * hi] = rows.index_select(0, idx).reshape(-1)
        want[lo:hi] = answers[idx]
    del idx
    before = stats(ix)
    got = lookup_dev(ix, dq, n)
    d = delta(stats(ix), before)
    assert d["binned"] == 2 and d["direct"] == 0
    assert_same_dev(got, want, "full piece")
