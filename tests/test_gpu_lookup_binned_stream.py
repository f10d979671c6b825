"""Pass A of the binned tf lookup (k_lb_bin of aix_lookup_binned.hip) writes a slice's records in whole 128-byte lines (LINE records) and
keeps what does not fill a line in an LDS carry from tile to tile; a workgroup writes its carries with its last tile. One wave flushes
a slice. AIX_LOOKUP_TEST_GRID_A caps pass A's grid, so that the small batches of tests/test_gpu_lookup_binned.py (the same 4092-key
index with 1024 filter words, built the same way) drive one workgroup through many tiles. Every answer is compared bit-exact with the
CPU oracle and with the direct kernel (AIX_LOOKUP_BINNED=0); every output buffer starts as 0xFFFFFFFF. For batches of keys every record
is filed once and passes the filter once, so `survivors` shows a lost or doubled carry."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import filterkey_ref as F
from test_gpu_lookup_binned import (N_BIG, N_KEYS, NMAX, assert_same_dev, base_batches, big_batch, build_index, case_wide,  # noqa: F401
                                    delta, finish_case, lookup, lookup_dev, set_bins, set_slice, stats)
from aindex_amd import synth

# the constants of aix_lookup_binned.hip
T, LINE, CHUNK = 4096, 16, 256                               # LB_TILE, LB_LINE, LB_CH
FILTER_WORDS = 1024
CARRY_BINS = 8
CARRY_R = (0, 1, 15, 16, 17, 31, 255, 256, 257)
CARRY_TILES = 3


def slice_of(codes, bins):
    """the filter slice pass A files a k-mer under: that of the canonical code's filter word"""
    word, _ = F.new_key(F.canonical(codes), FILTER_WORDS)
    return word // (FILTER_WORDS // bins)


def carry_batch(keys):
    """For every r of CARRY_R, CARRY_TILES tiles in which the slice with the most keys receives exactly r records, each a key of its
    own within the tile; of the other rows every eighth is a key of one other slice (more would fill that slice's region, which is
    sized for uniformly hashed queries) and the rest carry a foreign byte. Returns the
    rows (len(CARRY_R) * CARRY_TILES * T, 23), the target slice and the number of (r, tile) cells that could not be filled."""
    sl = slice_of(keys, CARRY_BINS)
    per = np.bincount(sl, minlength=CARRY_BINS)
    target = int(np.argmax(per))
    other = int(np.argsort(per)[-2])
    tk, ok = keys[sl == target], keys[sl == other]
    rows, missing = [], 0
    for ri, r in enumerate(CARRY_R):
        for tile in range(CARRY_TILES):
            have = min(r, tk.shape[0])
            missing += have < r
            start = (97 * (ri * CARRY_TILES + tile)) % tk.shape[0]                                 # other keys from tile to tile
            mine = tk[(start + np.arange(have)) % tk.shape[0]]
            rest = T - have
            codes = np.concatenate([mine, ok[(np.arange(rest) * 7 + tile) % ok.shape[0]]])
            flip = (synth.sm64(61 + tile, np.arange(T, dtype=np.uint64)) & np.uint64(1)).astype(bool)
            asc = synth.decode_kmers(np.where(flip, synth.revcomp_codes(codes, 23), codes), 23)  # both strands
            foreign = have + np.flatnonzero(np.arange(rest) % 8 != 0)
            asc[foreign, (foreign * 5) % 23] = np.where(foreign & 8, ord("N"), 0).astype(np.uint8)
            order = np.argsort(synth.sm64(71 + ri, np.arange(T, dtype=np.uint64) + np.uint64(T * tile)), kind="stable")
            rows.append(asc[order])
    return np.concatenate(rows), target, missing


@pytest.fixture(scope="module")
def scase(tmp_path_factory):
    d = tmp_path_factory.mktemp("binned_stream")
    g = synth.genome_codes(29, 6000)
    keys, counts = synth.canonical_distinct(g, 23)
    assert keys.shape[0] >= N_KEYS
    keys, counts = np.ascontiguousarray(keys[:N_KEYS]), np.ascontiguousarray(counts[:N_KEYS])
    ix, orc = build_index(d, "stream", keys, counts)
    assert ix.canonical_only and ix.info["absence_filter_words"] == FILTER_WORDS
    b = base_batches(keys, NMAX)
    carry, target, missing = carry_batch(keys)
    c = finish_case(ix, orc, {"absent": b["absent"], "present": b["present"], "half": b["half"], "dirty": b["dirty"], "carry": carry})
    c["keys"], c["carry_target"], c["carry_missing"] = keys, target, missing
    assert c["want"]["present"].min() > 0 and int((c["want"]["absent"] != 0).sum()) < NMAX // 100
    with pytest.MonkeyPatch.context() as mp:                  # the direct kernel's answers, once per batch
        mp.setenv("AIX_LOOKUP_BINNED", "0")
        before = stats(ix)
        c["direct"] = {k: lookup(ix, v, v.numel() // 23) for k, v in c["dev"].items()}
        assert stats(ix) == before
    for k, v in c["direct"].items():
        assert np.array_equal(v, c["want"][k]), k
    yield c
    ix.close()


def binned(monkeypatch, grid=None, bins=8):
    if bins is not None:
        set_bins(monkeypatch, bins)
    monkeypatch.setenv("AIX_LOOKUP_BINNED", "2")
    if grid is None:
        monkeypatch.delenv("AIX_LOOKUP_TEST_GRID_A", raising=False)
    else:
        monkeypatch.setenv("AIX_LOOKUP_TEST_GRID_A", str(grid))


def check(c, kind, n, first=0):
    """rows first .. first + n of a batch"""
    ix = c["ix"]
    before = stats(ix)
    got = lookup(ix, c["dev"][kind][23 * first:], n)
    d = delta(stats(ix), before)
    assert np.array_equal(got, c["want"][kind][first:first + n]), (kind, n)
    assert np.array_equal(got, c["direct"][kind][first:first + n]), (kind, n)
    return d


@pytest.mark.parametrize("kind", ["absent", "present", "half", "dirty"])
@pytest.mark.parametrize("grid", [1, 2, 3])
def test_tile_edges(scase, monkeypatch, grid, kind):
    """One, two and three workgroups on up to six tiles: a workgroup's carries go from tile to tile and leave with its last one, which
    is ragged at 5 T + 1; N < LINE: nothing but the last tile's partial lines."""
    for bins in (2, 8, 64):
        binned(monkeypatch, grid, bins)
        for n in (1, 15, 16, 17, T - 1, T, T + 1, 2 * T, 5 * T + 1):
            d = check(scase, kind, n)
            assert d["binned"] == 1 and d["direct"] == 0, (grid, kind, bins, n)
            if kind == "present":
                assert d["survivors"] == n and d["overflow"] == 0, (grid, bins, n, d)


def test_keys_give_every_carry_length(scase):
    """no GPU work: at 8 bins the fullest slice of the 4092 keys has at least max(CARRY_R) keys, so every (r, tile) cell is filled"""
    per = np.bincount(slice_of(scase["keys"], CARRY_BINS), minlength=CARRY_BINS)
    print("keys per slice at 8 bins:", per.tolist(), "cells not filled:", scase["carry_missing"], "of", len(CARRY_R) * CARRY_TILES)
    assert per.max() >= max(CARRY_R)
    assert 4 * scase["carry_missing"] <= len(CARRY_R) * CARRY_TILES
    rows = scase["dev"]["carry"].cpu().numpy().reshape(-1, 23)
    clean = np.isin(rows, np.frombuffer(b"ACGT", dtype=np.uint8)).all(axis=1)
    sl = np.full(rows.shape[0], -1)
    sl[clean] = slice_of(synth.encode_kmers(rows[clean]), CARRY_BINS)
    got = (sl.reshape(len(CARRY_R), CARRY_TILES, T) == scase["carry_target"]).sum(axis=2)
    want = np.minimum(np.array(CARRY_R)[:, None], per.max()).repeat(CARRY_TILES, axis=1)
    assert np.array_equal(got, want), got.tolist()


@pytest.mark.parametrize("r", CARRY_R)
def test_carry_lengths(scase, monkeypatch, r):
    """One workgroup, three tiles, one slice that receives exactly r records in each of them: its carry goes 0 -> r % LINE ->
    2 r % LINE and is written with the third tile. All rows are keys or carry a foreign byte, so every row is a survivor."""
    binned(monkeypatch, 1, CARRY_BINS)
    n = CARRY_TILES * T
    d = check(scase, "carry", n, first=CARRY_R.index(r) * n)
    assert d == {"binned": 1, "direct": 0, "overflow": 0, "survivors": n}, (r, d)


@pytest.mark.parametrize("kind", ["absent", "present"])
@pytest.mark.parametrize("grid", [1, None])
def test_full_regions_with_a_carry(scase, monkeypatch, grid, kind):
    """Regions of 0, 1, 1 and 2 chunks: carried records find their region full when they leave, and are survivors exactly once"""
    binned(monkeypatch, grid)
    n = 5 * T + 1
    for cap in (0, 16, 256, 272):
        monkeypatch.setenv("AIX_LOOKUP_TEST_BIN_CAP", str(cap))
        d = check(scase, kind, n)
        assert d["binned"] == 1 and d["overflow"] > 0 and d["survivors"] - d["overflow"] >= 0, (grid, kind, cap, d)
        if kind == "present":
            assert d["survivors"] == n, (grid, cap, d)


@pytest.mark.parametrize("grid", [1, None])
def test_alignment_of_the_queries(scase, monkeypatch, grid):
    """the same batch at eight byte offsets inside a larger buffer whose other bytes are 'A' or 0xFF"""
    binned(monkeypatch, grid)
    ix, src, want = scase["ix"], scase["dev"]["dirty"], scase["want"]["dirty"]
    for n in (1, T + 1, 3 * T + 5):
        for fill in (ord("A"), 0xFF):
            buf = torch.full((23 * n + 64,), fill, dtype=torch.uint8, device="cuda")
            for off in (0, 1, 2, 3, 4, 7, 8, 15):
                buf[:] = fill
                buf[off:off + 23 * n] = src[:23 * n]
                out = torch.full((n,), -1, dtype=torch.int32, device="cuda")
                ix.tf_ascii_t(buf[off:off + 23 * n], out)
                torch.cuda.synchronize()
                assert np.array_equal(out.cpu().numpy().view(np.uint32), want[:n]), (grid, n, fill, off)


@pytest.mark.parametrize("piece", [1000, T + 3])
def test_pieces(scase, monkeypatch, piece):
    """pieces that start at changing offsets inside a dword; the header is zeroed between them and every piece flushes its own carries"""
    n = 4 * T + 1
    for grid in (1, None):
        binned(monkeypatch, grid)
        monkeypatch.setenv("AIX_LOOKUP_PIECE", str(piece))
        for kind in ("dirty", "present"):
            d = check(scase, kind, n)
            assert d["binned"] == -(-n // piece) and d["direct"] == 0, (piece, kind)
            if kind == "present":
                assert d["survivors"] == n and d["overflow"] == 0, (piece, d)


def test_one_slice(scase, monkeypatch):
    """nbins = 1: one wave flushes every record of a tile"""
    for grid in (1, None):
        binned(monkeypatch, grid, 1)
        for n in (4097, NMAX):
            d = check(scase, "present", n)
            assert d == {"binned": 1, "direct": 0, "overflow": 0, "survivors": n}
            check(scase, "dirty", n)


@pytest.mark.parametrize("bins", [255, 256])
def test_wide_geometry(case_wide, monkeypatch, bins):
    """255 and LB_MAXBINS slices of a filter of ~300 000 words: the carry of 256 slices takes 32 KiB of LDS beside the tile's"""
    ix = case_wide["ix"]
    nbloom = ix.info["absence_filter_words"]
    wps = next(w for w in range(nbloom // bins + 2, 0, -1) if -(-nbloom // w) == bins)
    set_slice(monkeypatch, 8 * wps)
    monkeypatch.setenv("AIX_LOOKUP_BINNED", "2")
    for grid in ("1", None):
        if grid:
            monkeypatch.setenv("AIX_LOOKUP_TEST_GRID_A", grid)
        else:
            monkeypatch.delenv("AIX_LOOKUP_TEST_GRID_A", raising=False)
        for kind in ("present", "dirty"):
            for n in (4097, NMAX):
                before = stats(ix)
                got = lookup(ix, case_wide["dev"][kind], n)
                d = delta(stats(ix), before)
                assert d["binned"] == 1 and d["direct"] == 0, (bins, kind, n)
                assert np.array_equal(got, case_wide["want"][kind][:n]), (bins, kind, n)
                if kind == "present":
                    assert d["survivors"] == n and d["overflow"] == 0, (bins, n, d)


@pytest.mark.parametrize("kind", ["absent_big", "dirty_big"])
def test_one_large_batch(scase, monkeypatch, kind):
    """2^23 + 1000 queries on the whole grid: two or three tiles per workgroup, the last one ragged"""
    binned(monkeypatch)
    ix = scase["ix"]
    base = ("absent", "present", "half", "dirty")               # big_batch takes every batch to have NMAX rows
    dq, want = big_batch({"dev": {k: scase["dev"][k] for k in base}, "want_dev": {k: scase["want_dev"][k] for k in base}}, kind)
    before = stats(ix)
    got = lookup_dev(ix, dq, N_BIG)
    d = delta(stats(ix), before)
    assert d["binned"] == 1 and d["direct"] == 0 and d["overflow"] == 0, d
    assert_same_dev(got, want, kind)
