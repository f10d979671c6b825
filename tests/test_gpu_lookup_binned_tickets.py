"""Pass B of the binned tf lookup (k_lb_filter of aix_lookup_binned.hip) hands its chunks out in tickets of PER_TICKET chunks through
eight counters. AIX_LOOKUP_TEST_GRID_B caps its grid, so that the small batches of tests/test_gpu_lookup_binned.py (the same 4092-key
index with 1024 filter words, built the same way) drive one workgroup through many tickets: a first ticket that is already past the
end, the guarded loads of a last ticket that is only partly inside, more counters than workgroups, and flushes of the survivor buffer
inside the loop. Every answer is compared bit-exact with the CPU oracle and with the direct kernel (AIX_LOOKUP_BINNED=0); every
output buffer starts as 0xFFFFFFFF."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_gpu_lookup_binned import (N_BIG, N_KEYS, NMAX, TINY_KEYS, assert_same_dev, base_batches, big_batch, build_index, case_tiny,  # noqa: F401
                                    delta, finish_case, lookup, lookup_dev, set_bins, set_slice, stats)
from aindex_amd import synth

# the constants of aix_lookup_binned.hip
PASS_B_THREADS, CHUNK, GROUPS = 512, 256, 2                  # LB_FB, LB_CH, LB_U
PER_TICKET = GROUPS * PASS_B_THREADS // CHUNK                # LB_CPT: 4 chunks = 1024 records
COUNTERS = 8                                                 # LB_TICKETS
PASS_B_GRID = 1024                                           # LB_GRID_B
FLUSH_AT = 4096 - GROUPS * PASS_B_THREADS                    # LB_FLUSH_AT = LB_SURV - LB_U * LB_FB: a workgroup that holds more survivors appends them
NS = (1, 65, 4097, NMAX)


@pytest.fixture(scope="module")
def tcase(tmp_path_factory):
    d = tmp_path_factory.mktemp("binned_tickets")
    g = synth.genome_codes(29, 6000)
    keys, counts = synth.canonical_distinct(g, 23)
    assert keys.shape[0] >= N_KEYS
    keys, counts = np.ascontiguousarray(keys[:N_KEYS]), np.ascontiguousarray(counts[:N_KEYS])
    ix, orc = build_index(d, "tickets", keys, counts)
    assert ix.canonical_only and ix.info["absence_filter_words"] == 1024
    b = base_batches(keys, NMAX)
    foreign = b["half"].copy()                                # a byte that is no base in every query: nothing reaches a chunk
    rows = np.arange(NMAX)
    foreign[rows, (rows * 7) % 23] = np.where(rows & 1, ord("N"), ord("*")).astype(np.uint8)
    c = finish_case(ix, orc, {"absent": b["absent"], "present": b["present"], "half": b["half"], "dirty": b["dirty"], "foreign": foreign})
    assert c["want"]["present"].min() > 0 and int((c["want"]["absent"] != 0).sum()) < NMAX // 100
    with pytest.MonkeyPatch.context() as mp:                  # the direct kernel's answers, once per batch
        mp.setenv("AIX_LOOKUP_BINNED", "0")
        before = stats(ix)
        c["direct"] = {k: lookup(ix, v, NMAX) for k, v in c["dev"].items()}
        assert stats(ix) == before
    for k, v in c["direct"].items():
        assert np.array_equal(v, c["want"][k]), k
    yield c
    ix.close()


def binned(monkeypatch, grid=None, bins=8):
    if bins is not None:
        set_bins(monkeypatch, bins)
    monkeypatch.setenv("AIX_LOOKUP_BINNED", "2")
    if grid is not None:
        monkeypatch.setenv("AIX_LOOKUP_TEST_GRID_B", str(grid))


def check(c, kind, n):
    ix = c["ix"]
    before = stats(ix)
    got = lookup(ix, c["dev"][kind], n)
    d = delta(stats(ix), before)
    assert np.array_equal(got, c["want"][kind][:n]), (kind, n)
    assert np.array_equal(got, c["direct"][kind][:n]), (kind, n)
    return d


@pytest.mark.parametrize("kind", ["absent", "present", "half", "dirty"])
@pytest.mark.parametrize("grid", [1, 3, 8, 9])
def test_grid_caps(tcase, monkeypatch, grid, kind):
    """One workgroup that takes every ticket; fewer workgroups than the COUNTERS counters (only as many counters as workgroups own
    tickets then, or the chunks of the others would never be filtered); as many; one more. N = 1: one chunk, so ticket 0 of counter
    0 is partly past the end and the first ticket of every other workgroup is past the end altogether. At N = NMAX the 18
    workgroups of pass A leave 8 * 18 partly filled chunks beside the full ones; whether their number is a multiple of PER_TICKET
    differs from batch to batch."""
    binned(monkeypatch, grid)
    for n in NS:
        d = check(tcase, kind, n)
        assert d["binned"] == 1 and d["direct"] == 0, (grid, kind, n)
        if kind == "present":
            assert d["survivors"] == n, (grid, n)                # every record passes the filter, and exactly once


@pytest.mark.parametrize("n", [1, 4097])
def test_zero_chunks(tcase, monkeypatch, n):
    """every query goes straight onto the survivor list in pass A: no chunk, and the first pull of every workgroup is past the end"""
    for grid in (None, 1):
        binned(monkeypatch, grid)
        d = check(tcase, "foreign", n)
        assert d == {"binned": 1, "direct": 0, "overflow": 0, "survivors": n}


def test_flush_inside_the_loop(tcase, monkeypatch):
    """one workgroup collects all NMAX survivors of `present`: more than two flush thresholds plus a trip, so it appends them at
    least twice inside its loop, and what is left at its end"""
    assert NMAX > 2 * FLUSH_AT + GROUPS * PASS_B_THREADS
    binned(monkeypatch, 1)
    d = check(tcase, "present", NMAX)
    assert d == {"binned": 1, "direct": 0, "overflow": 0, "survivors": NMAX}


def test_shipped_constants(tcase, monkeypatch):
    """The whole grid, no cap: all N_BIG records pass. A workgroup that never appends inside its loop hands over at most FLUSH_AT
    survivors at its end, so with N_BIG > PASS_B_GRID * FLUSH_AT at least one of them appends inside the loop."""
    assert N_BIG > PASS_B_GRID * FLUSH_AT
    binned(monkeypatch)
    ix = tcase["ix"]
    dq, want = big_batch(tcase, "present_big")
    before = stats(ix)
    got = lookup_dev(ix, dq, N_BIG)
    d = delta(stats(ix), before)
    assert_same_dev(got, want, "present_big")
    assert d == {"binned": 1, "direct": 0, "overflow": 0, "survivors": N_BIG}


@pytest.mark.parametrize("slice_bytes", [None, 8])
@pytest.mark.parametrize("nk", TINY_KEYS)
def test_tiny_filters(case_tiny, monkeypatch, nk, slice_bytes):
    """filters of one and two words, one workgroup"""
    c = case_tiny[nk]
    ix, total = c["ix"], c["want"].shape[0]
    set_slice(monkeypatch, slice_bytes)
    binned(monkeypatch, 1, bins=None)
    for n in (1, 65, total):
        before = stats(ix)
        got = lookup(ix, c["dq"], n)
        d = delta(stats(ix), before)
        assert d["binned"] == 1 and d["direct"] == 0, (nk, slice_bytes, n)
        assert np.array_equal(got, c["want"][:n]), (nk, slice_bytes, n)
        monkeypatch.setenv("AIX_LOOKUP_BINNED", "0")
        assert np.array_equal(lookup(ix, c["dq"], n), c["want"][:n]), (nk, slice_bytes, n)
        monkeypatch.setenv("AIX_LOOKUP_BINNED", "2")


def test_piece_cuts(tcase, monkeypatch):
    """71 pieces on three workgroups: the header and the ticket counters are zeroed for each, and each starts at ticket 0 again"""
    binned(monkeypatch, 3)
    monkeypatch.setenv("AIX_LOOKUP_PIECE", "1000")
    for kind in ("absent", "dirty", "present"):
        d = check(tcase, kind, NMAX)
        assert d["binned"] == -(-NMAX // 1000) and d["direct"] == 0, kind
        if kind == "present":
            assert d["survivors"] == NMAX and d["overflow"] == 0
