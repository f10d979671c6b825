"""Pass A of the binned tf lookup (k_lb_bin of aix_lookup_binned.hip): it fetches a query one query ahead of the one it encodes, through
a clamped, branch-free fetch; encodes with encode23_clean; finds the filter slice with a shift where the slice width is a power of two;
and zeroes a tile's answers with 16-byte stores behind the query loop. On the 4092-key index with 1024 filter words of
tests/test_gpu_lookup_binned.py (built the same way), forced binned (AIX_LOOKUP_BINNED=2), 8 bins unless a test says otherwise. Every
answer is compared bit for bit with the direct kernel (AIX_LOOKUP_BINNED=0) and the CPU oracle; every output buffer starts as 0xFFFFFFFF."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_lookup_binned import N_KEYS, base_batches, build_index, delta, finish_case, lookup, set_bins, set_slice, stats
from aindex_amd import synth

# one query; the edges of a round of LB_TB = 512 queries (a lane's second query) and of a tile of LB_TILE = 4096; a third tile of one query
NS = (1, 511, 512, 513, 4095, 4096, 4097, 8193)
NROWS = max(NS)
FOREIGN = (ord("N"), ord("g"), 0x00, 0xFF, ord("@"))


@pytest.fixture(scope="module")
def acase(tmp_path_factory):
    d = tmp_path_factory.mktemp("binned_pass_a")
    keys, counts = synth.canonical_distinct(synth.genome_codes(29, 6000), 23)
    assert keys.shape[0] >= N_KEYS
    keys, counts = np.ascontiguousarray(keys[:N_KEYS]), np.ascontiguousarray(counts[:N_KEYS])
    ix, orc = build_index(d, "pass_a", keys, counts)
    assert ix.canonical_only and ix.info["absence_filter_words"] == 1024
    b = base_batches(keys, NROWS)
    # present keys on both strands, one foreign byte at each of the 23 positions in turn, for each of the foreign bytes; clean rows between them
    stained = b["present"][: 2 * 23 * len(FOREIGN)].copy()
    stained_rows = np.arange(0, stained.shape[0], 2)
    for r in stained_rows:
        stained[r, (r // 2) % 23] = FOREIGN[(r // 2) // 23]
    c = finish_case(ix, orc, {"dirty": b["dirty"], "half": b["half"], "absent": b["absent"], "stained": stained})
    c["stained_rows"] = stained_rows
    with pytest.MonkeyPatch.context() as mp:     # the direct kernel's answers, once per batch
        mp.setenv("AIX_LOOKUP_BINNED", "0")
        before = stats(ix)
        c["direct"] = {k: lookup(ix, v, v.numel() // 23) for k, v in c["dev"].items()}
        assert stats(ix) == before
    for k, v in c["direct"].items():
        assert np.array_equal(v, c["want"][k]), k
    assert int((c["want"]["absent"] != 0).sum()) < NROWS // 100 and np.count_nonzero(c["want"]["half"]) > NROWS // 3
    yield c
    ix.close()


def binned(monkeypatch, bins=8):
    set_bins(monkeypatch, bins)
    monkeypatch.setenv("AIX_LOOKUP_BINNED", "2")


@pytest.mark.parametrize("kind", ["dirty", "half", "absent"])
def test_lane_round_and_tile_edges(acase, monkeypatch, kind):
    ix = acase["ix"]
    binned(monkeypatch)
    for n in NS:
        before = stats(ix)
        got = lookup(ix, acase["dev"][kind], n)
        d = delta(stats(ix), before)
        assert d["binned"] == 1 and d["direct"] == 0 and d["overflow"] == 0, (kind, n, d)
        assert np.array_equal(got, acase["want"][kind][:n]), (kind, n)
        assert np.array_equal(got, acase["direct"][kind][:n]), (kind, n)


@pytest.mark.parametrize("q_off", [0, 1, 2, 3])
@pytest.mark.parametrize("out_off", [0, 1, 2, 3])
def test_every_alignment_of_queries_and_answers(acase, monkeypatch, q_off, out_off):
    """the queries start at byte q_off of a larger tensor (every alignment of a lane's dword window, of the batch's first and of its last
    query), the answers at element out_off of a larger one (every split of a tile's zeroing into single dwords and 16-byte stores);
    what lies around the answers keeps its 0xFFFFFFFF"""
    ix = acase["ix"]
    binned(monkeypatch)
    pad = 8
    for n in (1, 2, 3, 5, 513, 4097, 8193):
        src = acase["dev"]["dirty"][: 23 * n]
        q = torch.full((23 * n + 2 * pad,), ord("A"), dtype=torch.uint8, device="cuda")
        q[q_off: q_off + 23 * n] = src
        out = torch.full((n + 2 * pad,), -1, dtype=torch.int32, device="cuda")
        before = stats(ix)
        ix.tf_ascii_t(q[q_off: q_off + 23 * n], out[out_off: out_off + n])
        torch.cuda.synchronize()
        d = delta(stats(ix), before)
        assert d["binned"] == 1 and d["direct"] == 0, (n, d)
        got = out.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[out_off: out_off + n], acase["want"]["dirty"][:n]), (q_off, out_off, n)
        assert (got[:out_off] == 0xFFFFFFFF).all() and (got[out_off + n:] == 0xFFFFFFFF).all(), (q_off, out_off, n)


def test_foreign_bytes_go_through_the_survivor_list(acase, monkeypatch):
    ix, want = acase["ix"], acase["want"]["stained"]
    n, rows = want.shape[0], acase["stained_rows"]
    assert rows.shape[0] == 23 * len(FOREIGN) and n == 2 * rows.shape[0]
    binned(monkeypatch)
    before = stats(ix)
    got = lookup(ix, acase["dev"]["stained"], n)
    d = delta(stats(ix), before)
    assert np.array_equal(got, want) and np.array_equal(got, acase["direct"]["stained"])
    clean = np.setdiff1d(np.arange(n), rows)
    assert want[clean].min() > 0                                     # the clean rows are keys: pass B lets them through as well
    assert d["binned"] == 1 and d["overflow"] == 0 and d["survivors"] >= rows.shape[0], d
    # the stained rows alone, so that nothing else can account for the survivors
    only = torch.from_numpy(np.ascontiguousarray(acase["dev"]["stained"].cpu().numpy().reshape(n, 23)[rows]).reshape(-1)).cuda()
    before = stats(ix)
    got = lookup(ix, only, rows.shape[0])
    d = delta(stats(ix), before)
    assert np.array_equal(got, want[rows])
    assert d["overflow"] == 0 and d["survivors"] == rows.shape[0], d  # a query with another byte never reaches a chunk: every one is a survivor


@pytest.mark.parametrize("kind", ["dirty", "half"])
def test_shift_and_reciprocal_slices_agree(acase, monkeypatch, kind):
    """128-word slices (a power of two: shift and mask) and 100-word slices (the reciprocal) on the same batch: the same answers and the
    same number of survivors, which is the filter's positives plus the queries with other bytes whatever the slicing"""
    ix = acase["ix"]
    monkeypatch.setenv("AIX_LOOKUP_BINNED", "2")
    for n in (NROWS, 4097):
        seen = []
        for words in (128, 100):
            set_slice(monkeypatch, 8 * words)
            before = stats(ix)
            got = lookup(ix, acase["dev"][kind], n)
            d = delta(stats(ix), before)
            assert d["binned"] == 1 and d["direct"] == 0 and d["overflow"] == 0, (kind, words, d)
            assert np.array_equal(got, acase["want"][kind][:n]), (kind, words, n)
            assert np.array_equal(got, acase["direct"][kind][:n]), (kind, words, n)
            seen.append(d["survivors"])
        assert seen[0] == seen[1] and seen[0] >= np.count_nonzero(acase["want"][kind][:n]), (kind, n, seen)
