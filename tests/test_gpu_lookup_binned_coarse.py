"""Pass B of the binned tf lookup with the coarse image of a filter slice in LDS (aix_lookup_binned.hip: k_lb_fold,
k_lb_filter_coarse; aix_device.hpp: bloom_fold) on the 4092-key index of test_gpu_lookup_binned.py, whose filter has 1024 words.
Every answer is compared bit-exact with the CPU oracle and with the direct kernel (run once per batch), every output buffer starts as
0xFFFFFFFF, and the two coarse counters (records tested against the image, records sent on to the filter word) are compared with a
numpy restatement over the host copy of the filter: they are the only sign that the coarse kernel ran at all. No tolerance anywhere.

A ticket of the coarse kernel is 16 chunks (4096 records). With 8 slices a batch of 70 001 leaves ~8750 records per slice in the
partly filled chunks of 18 pass-A workgroups and a batch of 4097 leaves ~512 in those of two: no slice's chunk count is a multiple of
the ticket, and every slice ends in a ticket that is cut short."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import filterkey_ref as F
from aindex_amd import _lib, synth
from test_gpu_lookup_binned import NMAX, TINY_KEYS, case, case_tiny, delta, lookup, set_bins, set_slice, stats  # noqa: F401  (fixtures)

NS = (1, 65, 4097, NMAX)
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
FLUSH_AT = 2048                                  # LBC_FLUSH_AT: a coarse pass-B workgroup that holds more survivors appends them inside its loop


def cstats(ix):
    out = (C.c_uint64 * 2)()
    _lib.check(_lib.lib().aix_lookup_binned_coarse_stats(ix._h, C.cast(out, _lib.vp)))
    return np.array([int(out[0]), int(out[1])], dtype=np.int64)


def filter_of(ix):
    n = ix.info["absence_filter_words"]
    out = np.zeros(n, dtype=np.uint64)
    _lib.check(_lib.lib().aix_debug_filter_words(ix._h, out.ctypes.data_as(_lib.vp), n))
    return out


def fold(words):
    """bloom_fold: quarter 0 of the word folded onto 8 bits"""
    return ((words & np.uint64(0xFF)) | ((words >> np.uint64(8)) & np.uint64(0xFF))).astype(np.uint8)


def restate(filt, flat):
    """per query of the flat ASCII batch: has a record (23 bytes of ACGT), its slice-free filter word, and whether the coarse test sends
    it on; as prefix sums (tested, sent on) over the first n queries, n = 0 .. N"""
    rows = flat.reshape(-1, 23)
    clean = np.isin(rows, ACGT).all(axis=1)
    hw, hb = F.filter_key(F.canonical(synth.encode_kmers(rows[clean])))
    word = F.word_index(hw, filt.shape[0])
    on = np.zeros(rows.shape[0], dtype=bool)
    on[clean] = ((fold(filt)[word] >> (hb & np.uint32(7)).astype(np.uint8)) & np.uint8(1)).astype(bool)
    words = np.full(rows.shape[0], -1, dtype=np.int64)
    words[clean] = word
    z = np.zeros(1, dtype=np.int64)
    return {"tested": np.concatenate([z, np.cumsum(clean)]), "on": np.concatenate([z, np.cumsum(on)]), "word": words}


@pytest.fixture(scope="module")
def world(case):
    """the shared case with more batches (subsets of its oracle-checked rows), the direct kernel's answers and the restated counts"""
    ix = case["ix"]
    filt = filter_of(ix)
    assert filt.shape[0] == 1024 and filt.any()
    flat = {k: v.cpu().numpy() for k, v in case["dev"].items()}
    want = dict(case["want"])
    half = restate(filt, flat["half"])
    dirty_rows = flat["dirty"].reshape(-1, 23)
    # gappy: the rows of `half` whose filter word lies outside slices 1, 3 and 4 of 8 (128 words each): slices with no chunk at all
    # between slices that have some; foreign: the rows of `dirty` with other bytes, none of which gets a record
    keep = np.flatnonzero(~np.isin(half["word"] // 128, (1, 3, 4)))
    other = np.flatnonzero(~np.isin(dirty_rows, ACGT).all(axis=1))
    assert keep.shape[0] > NMAX // 2 and other.shape[0] > 1000
    for name, src, idx in (("gappy", "half", keep), ("foreign", "dirty", other)):
        flat[name] = np.ascontiguousarray(flat[src].reshape(-1, 23)[idx]).reshape(-1)
        want[name] = want[src][idx]
    dev = {k: torch.from_numpy(v.copy()).cuda() for k, v in flat.items()}
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("AIX_LOOKUP_BINNED", "0")                                                        # the direct kernel, once per batch
        direct = {k: lookup(ix, dev[k], want[k].shape[0]) for k in dev}
    for k in dev:
        assert np.array_equal(direct[k], want[k]), k
    return {"ix": ix, "filt": filt, "dev": dev, "want": want, "direct": direct, "re": {k: restate(filt, v) for k, v in flat.items()}}


def run(w, kind, n, pieces=1):
    """one forced binned call through the coarse kernel: answers, the four counters and the two coarse counters"""
    ix = w["ix"]
    before, cbefore = stats(ix), cstats(ix)
    got = lookup(ix, w["dev"][kind], n)
    d, cd = delta(stats(ix), before), cstats(ix) - cbefore
    assert np.array_equal(got, w["want"][kind][:n]), (kind, n)
    assert np.array_equal(got, w["direct"][kind][:n]), (kind, n)
    assert d["binned"] == pieces and d["direct"] == 0 and d["overflow"] == 0, (kind, n, d)
    re = w["re"][kind]
    assert cd.tolist() == [int(re["tested"][n]), int(re["on"][n])], (kind, n, cd.tolist())
    return d, cd


@pytest.mark.parametrize("kind", ["absent", "half", "present"])
def test_exact_coarse_counts(world, monkeypatch, kind):
    set_bins(monkeypatch, 8)
    monkeypatch.setenv("AIX_LOOKUP_BINNED", "2")
    re = world["re"][kind]
    assert re["tested"][NMAX] == NMAX                                                             # no other bytes in these batches
    if kind == "present":
        assert re["on"][NMAX] == NMAX                                                             # a key's own bit is set in the image
    if kind == "absent":
        share = re["on"][NMAX] / NMAX
        print("absent: share sent on to the filter word %.4f" % share)
        assert 0.0 < share < 1.0                                                                  # 0.3897 when restated on the CPU alone; 1 - (7/8)^4 = 0.41
    for n in NS:
        d, cd = run(world, kind, n)
        if kind == "present":
            assert cd[1] == cd[0] == n and d["survivors"] == n


@pytest.mark.parametrize("grid", [1, 3, 8, 9])
def test_slice_changes_inside_a_workgroup(world, monkeypatch, grid):
    """8 slices on 1 workgroup (it owns and reloads all of them), on 3 (counters own 3 / 3 / 2 slices), on 8 (one each) and on 9 (eight
    counters in use, two workgroups on the first). same_absent: one slice has chunks, so every other counter's first ticket is
    already past the end. gappy: slices without chunks between slices that have some. foreign: no chunk anywhere."""
    set_bins(monkeypatch, 8)
    monkeypatch.setenv("AIX_LOOKUP_BINNED", "2")
    monkeypatch.setenv("AIX_LOOKUP_TEST_GRID_B", str(grid))
    monkeypatch.setenv("AIX_LOOKUP_TEST_BIN_CAP", str(1 << 20))                                   # same_absent: 70 001 records in one slice, none overflows
    for kind in ("absent", "half", "dirty", "same_absent", "gappy", "foreign"):
        for n in NS:
            if n <= world["want"][kind].shape[0]:
                run(world, kind, n)


@pytest.mark.parametrize("slice_bytes,bins", [(8 * 341, 4), (8 * 1000, 2), (8 * 4, 256), (8 * 1024, 1), (None, 1)])
def test_odd_slice_geometry(world, monkeypatch, slice_bytes, bins):
    """341 words: an image of 341 bytes in a stride of 352, and a last slice of one word; 1000 words: slices of 1000 and 24; 4 words:
    256 slices, 32 owned by each counter; one slice as wide as the filter"""
    assert slice_bytes is None or -(-1024 // (slice_bytes // 8)) == bins
    set_slice(monkeypatch, slice_bytes)
    monkeypatch.setenv("AIX_LOOKUP_BINNED", "2")
    monkeypatch.setenv("AIX_LOOKUP_TEST_BIN_CAP", str(1 << 20))                                   # no overflow whatever the slice count
    for grid in (3, None):
        if grid:
            monkeypatch.setenv("AIX_LOOKUP_TEST_GRID_B", str(grid))
        else:
            monkeypatch.delenv("AIX_LOOKUP_TEST_GRID_B")
        for kind in ("half", "dirty"):
            for n in (4097, NMAX):
                run(world, kind, n)


@pytest.mark.parametrize("slice_bytes", [None, 8])
@pytest.mark.parametrize("nk", TINY_KEYS)
def test_tiny_filters(case_tiny, monkeypatch, nk, slice_bytes):
    """filters of one and two words: an image of one or two bytes in a stride of 16"""
    c = case_tiny[nk]
    ix, total = c["ix"], c["want"].shape[0]
    re = restate(filter_of(ix), c["dq"].cpu().numpy())
    set_slice(monkeypatch, slice_bytes)
    for n in (1, 65, total):
        monkeypatch.setenv("AIX_LOOKUP_BINNED", "0")
        direct = lookup(ix, c["dq"], n)
        monkeypatch.setenv("AIX_LOOKUP_BINNED", "2")
        before, cbefore = stats(ix), cstats(ix)
        got = lookup(ix, c["dq"], n)
        d, cd = delta(stats(ix), before), cstats(ix) - cbefore
        assert d["binned"] == 1 and d["direct"] == 0 and d["overflow"] == 0, (nk, slice_bytes, n)
        assert np.array_equal(got, c["want"][:n]) and np.array_equal(got, direct), (nk, slice_bytes, n)
        assert cd.tolist() == [int(re["tested"][n]), int(re["on"][n])], (nk, slice_bytes, n)


@pytest.mark.parametrize("switch,value", [("AIX_LOOKUP_TEST_COARSE_MAX", "127"), ("AIX_LOOKUP_TEST_COARSE_MAX", "0"), ("AIX_LOOKUP_COARSE", "0")])
def test_fallback_to_pass_b_without_the_image(world, monkeypatch, switch, value):
    """slices of 128 words: a limit of 127 words, or the switch, sends the batch through k_lb_filter; a limit of 128 does not"""
    ix = world["ix"]
    set_bins(monkeypatch, 8)
    monkeypatch.setenv("AIX_LOOKUP_BINNED", "2")
    monkeypatch.setenv("AIX_LOOKUP_TEST_GRID_B", "3")
    for kind in ("absent", "dirty"):
        for n in (4097, NMAX):
            monkeypatch.setenv("AIX_LOOKUP_TEST_COARSE_MAX", "128")
            monkeypatch.delenv("AIX_LOOKUP_COARSE", raising=False)
            with_image, _ = run(world, kind, n)
            monkeypatch.delenv("AIX_LOOKUP_TEST_COARSE_MAX")
            monkeypatch.setenv(switch, value)
            before, cbefore = stats(ix), cstats(ix)
            got = lookup(ix, world["dev"][kind], n)
            assert np.array_equal(cstats(ix), cbefore), (kind, n)
            assert delta(stats(ix), before) == with_image, (kind, n)                              # the same pieces, overflow and survivors
            assert np.array_equal(got, world["want"][kind][:n]) and np.array_equal(got, world["direct"][kind][:n]), (kind, n)
            monkeypatch.delenv(switch)


def test_image_follows_the_filter(world, case_tiny, monkeypatch):
    """the filter switched off (the binned path declines) and on again; two indexes with filters of 1024 and 2 words open at once, and
    the same index at two slice widths: each call tests the image of its own filter and geometry"""
    ix = world["ix"]
    monkeypatch.setenv("AIX_LOOKUP_BINNED", "2")
    set_bins(monkeypatch, 8)
    run(world, "half", NMAX)
    before, cbefore = stats(ix), cstats(ix)
    ix.set_absence_filter(False)
    try:
        assert np.array_equal(lookup(ix, world["dev"]["half"], NMAX), world["want"]["half"])
        assert stats(ix) == before and np.array_equal(cstats(ix), cbefore)
    finally:
        ix.set_absence_filter(True)
    run(world, "half", NMAX)
    tiny = case_tiny[5]
    tix, total = tiny["ix"], tiny["want"].shape[0]
    re = restate(filter_of(tix), tiny["dq"].cpu().numpy())
    for bins in (8, 2, 8):
        set_slice(monkeypatch, 8)
        cbefore = cstats(tix)
        assert np.array_equal(lookup(tix, tiny["dq"], total), tiny["want"])
        assert (cstats(tix) - cbefore).tolist() == [int(re["tested"][total]), int(re["on"][total])]
        set_bins(monkeypatch, bins)
        run(world, "absent", NMAX)
        run(world, "dirty", 4097)


def test_pieces(world, monkeypatch):
    """pieces of 1000 on three workgroups: the ticket counters start at zero and no workgroup holds a slice at the start of a piece"""
    set_bins(monkeypatch, 8)
    monkeypatch.setenv("AIX_LOOKUP_BINNED", "2")
    monkeypatch.setenv("AIX_LOOKUP_PIECE", "1000")
    monkeypatch.setenv("AIX_LOOKUP_TEST_GRID_B", "3")
    for kind in ("absent", "dirty"):
        for n in (4097, NMAX):
            run(world, kind, n, pieces=-(-n // 1000))


def test_survivor_flush_inside_the_loop(world, monkeypatch):
    """one workgroup, every record survives: 70 001 survivors against room for FLUSH_AT between two tickets"""
    set_bins(monkeypatch, 8)
    monkeypatch.setenv("AIX_LOOKUP_BINNED", "2")
    monkeypatch.setenv("AIX_LOOKUP_TEST_GRID_B", "1")
    d, cd = run(world, "present", NMAX)
    assert d["survivors"] == NMAX and cd[1] == NMAX and NMAX > 2 * FLUSH_AT
