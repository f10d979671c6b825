"""The pile-up on the GPU (k_pl_* of aix_pileup.hip) on inputs no threading and no pile-up wrote (tests/pileup_fuzz_cases.py): random valid
step arrays under five (max_gap, extend) sets, placements of one base and up (thousands on one contig base, bytes of all 256 values,
counts that wrap), cells over an enumerated palette and thresholds from 0 to 2^32 - 1, every presence pattern of the call's nullable
outputs, U = 0. Every array equals the restatement (tests/pileup_ref.py), which test_pileup_fuzz_cpu.py pins to a second opinion and
whose inputs it shows to reach these situations. Exact equality throughout; 64 poisoned elements stand behind every output of a raw call."""
import ctypes as C
import hashlib
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import graph_cases as G
import pileup_fuzz_cases as FC
import pileup_ref as PR
import test_gpu_pileup as TP
from aindex_amd import _lib

vp, _t, _np = _lib.vp, TP._t, TP._np
P8, P32, P64 = 0x6B, 0x6B6B6B6B, 0x6B6B6B6B6B6B6B6B
GRIDS = (None, "1", "3")
THRESHOLDS = dict(min_depth=8, min_major_permille=700, min_alt_count=3, min_alt_permille=200)
PER_BASE = ("polished", "n_changed", "depth_sum", "uncovered")
ORDER = ("seq_place_off", "place_unitig", "place_flag", "place_pos", "place_q0", "place_len")


def _set_grid(monkeypatch, grid):
    if grid is None:
        monkeypatch.delenv("AIX_UG_TEST_GRID", raising=False)
    else:
        monkeypatch.setenv("AIX_UG_TEST_GRID", grid)


def _poison(n, ty):
    import torch
    return torch.full((n + 64,), {torch.uint8: P8, torch.int32: P32, torch.int64: P64}[ty], dtype=ty, device="cuda")


def _clean(t, k=0):
    import torch
    return bool((t[k:] == {torch.uint8: P8, torch.int32: P32, torch.int64: P64}[t.dtype]).all())


def _q(t):
    return vp(t.data_ptr()) if t is not None and t.numel() else None


@pytest.fixture(scope="module")
def index(tmp_path_factory):
    """an index to hang the engine methods on: they take arrays, but live on a handle"""
    with TP._open(G.write_graph_case(0, str(tmp_path_factory.mktemp("plf")))[0]) as ix:
        yield ix


@pytest.fixture(scope="module")
def step_wants():
    """a steps case and the restatement of place, pile and the call at two threshold sets per parameter set: made once, left unchanged"""
    made = {}

    def get(seed):
        if seed not in made:
            c = FC.steps_case(seed)
            wants = []
            for max_gap, extend in FC.PLACE_PARAMS:
                wp = PR.place(c["offs"], c["steps"], c["offsets"], max_gap, extend)
                wc = PR.pile(c["seqs"], wp, c["offsets"], c["bases"])
                wants.append((wp, wc, [PR.call(c["offsets"], c["bases"], wc["counts"], **th) for th in ({}, FC.LOOSE)]))
            made[seed] = (c, wants)
        return made[seed]
    return get


@pytest.fixture(scope="module")
def place_wants():
    """a placements case piled by the restatement onto its prefilled counts, and once more on top"""
    made = {}

    def get(seed):
        if seed not in made:
            c = FC.placements_case(seed)
            once = PR.pile(c["seqs"], c["places"], c["offsets"], c["bases"], c["counts"])
            made[seed] = (c, once, PR.pile(c["seqs"], c["places"], c["offsets"], c["bases"], once["counts"]))
        return made[seed]
    return get


@pytest.fixture(scope="module")
def cell_wants():
    c = FC.cells_case()
    return c, [PR.call(c["offsets"], c["bases"], c["counts"], **th) for th in FC.CALL_PARAMS]


def _dev_graph(c):
    return {"offsets": _t(c["offsets"]), "bases": _t(c["bases"])}


def _dev_seqs(c):
    return _t(np.frombuffer(b"".join(c["seqs"]), dtype=np.uint8)), _t(c["offs"])


def _steps_chain(ix, c, wants, graph, st, so, dev_steps, tag):
    """pile_place_t, pileup_t and pile_call_t under every parameter set, each on the device arrays of the one before -> a digest"""
    h = hashlib.sha256()
    for (max_gap, extend), (wp, wc, calls) in zip(FC.PLACE_PARAMS, wants):
        places = ix.pile_place_t(graph, so, dev_steps, max_gap=max_gap, extend=extend)
        TP._same(places, wp, PR.PLACE_KEYS, PR.PLACE_DTYPES, (tag, max_gap, extend))
        assert (places["n_place"], places["n_circular_steps"]) == (wp["n_place"], wp["n_circular_steps"]), (tag, max_gap, extend)
        piled = ix.pileup_t(graph, st, so, places)
        TP._same(piled, wc, ("counts", "place_mism"), (np.uint32, np.uint32), (tag, max_gap, extend))
        assert piled["stats"] == wc["stats"].tolist(), (tag, max_gap, extend)
        for t in [places[k] for k in PR.PLACE_KEYS] + [piled["counts"], piled["place_mism"]]:
            h.update(_np(t).tobytes())
        for th, want in zip(({}, FC.LOOSE), calls):
            got = ix.pile_call_t(graph, piled["counts"], **th)
            TP._same_call(got, want, (tag, max_gap, extend, sorted(th)))
            for k in PR.VAR_KEYS + ("polished", "depth_sum", "uncovered"):
                h.update(_np(got[k]).tobytes())
    return h.hexdigest()


def _dev_steps(c):
    return tuple(_t(c["steps"][k]) for k in ("seq_step_off",) + FC._STEP_KEYS)


@pytest.mark.parametrize("seed", FC.SEEDS)
def test_random_steps(index, step_wants, monkeypatch, seed):
    """1. steps_case x PLACE_PARAMS through pile_place_t, pileup_t and pile_call_t (defaults and LOOSE), under the default grid and 1 and 3
    workgroups: every array and scalar equals the restatement."""
    c, wants = step_wants(seed)
    graph, (st, so), dev_steps = _dev_graph(c), _dev_seqs(c), _dev_steps(c)
    digests = set()
    for grid in GRIDS:
        _set_grid(monkeypatch, grid)
        digests.add(_steps_chain(index, c, wants, graph, st, so, dev_steps, (seed, grid)))
    assert len(digests) == 1


def _dev_pile_input(c):
    d = dict(_dev_graph(c), M=len(c["seqs"]), R=int(c["places"]["place_unitig"].shape[0]), U=int(c["offsets"].shape[0]) - 1)
    d["seqs"], d["offs"] = _dev_seqs(c)
    d.update({k: _t(c["places"][k]) for k in ORDER})
    return d


def _raw_pile(d, counts, mism=True, stats=True, stream=None):
    """aix_pileup_dev itself onto `counts` (in place), 64 poisoned elements behind place_mism and stats -> status, place_mism, stats"""
    import torch as T
    m = _poison(d["R"], T.int32) if mism else None
    s = _poison(3, T.int64) if stats else None
    status = _lib.lib().aix_pileup_dev(_q(d["seqs"]), _q(d["offs"]), d["M"], _q(d[ORDER[0]]), d["R"], *[_q(d[k]) for k in ORDER[1:]], d["U"], vp(d["offsets"].data_ptr()),
                                       _q(d["bases"]), _q(counts), _q(m), _q(s), stream)
    T.cuda.synchronize()
    assert (m is None or _clean(m, d["R"] if status == 0 else 0)) and (s is None or _clean(s, 3 if status == 0 else 0))
    return status, None if m is None else _np(m[:d["R"]]), None if s is None else _np(s[:3])


def _same_pile(counts, mism, stats, want, tag):
    assert np.array_equal(_np(counts), want["counts"]), (tag, "counts")
    assert mism is None or (mism.dtype == np.uint32 and np.array_equal(mism, want["place_mism"])), (tag, "place_mism")
    assert stats is None or (stats.dtype == np.uint64 and np.array_equal(stats, want["stats"])), (tag, "stats")


@pytest.mark.parametrize("seed", FC.PLACEMENT_SEEDS)
def test_array_level_placements(place_wants, monkeypatch, seed):
    """2. placements_case through aix_pileup_dev itself onto the prefilled counts: counts, place_mism and stats equal the restatement, with
    place_mism and stats present, one of them, and neither; a second call on top equals the restatement applied twice; the reverse
    complement of the input gives equal counts, place_mism and stats."""
    c, once, twice = place_wants(seed)
    d, twin = _dev_pile_input(c), _dev_pile_input(FC.rc_twin(c))
    for grid in GRIDS:
        _set_grid(monkeypatch, grid)
        for mism, stats in itertools.product((True, False), repeat=2):
            counts = _t(c["counts"])
            status, m, s = _raw_pile(d, counts, mism, stats)
            assert status == 0
            _same_pile(counts, m, s, once, (seed, grid, mism, stats))
        status, m, s = _raw_pile(d, counts)                          # (counts: what the call without outputs left)
        assert status == 0
        _same_pile(counts, m, s, twice, (seed, grid, "twice"))
        counts = _t(c["counts"])
        status, m, s = _raw_pile(twin, counts)
        assert status == 0
        _same_pile(counts, m, s, once, (seed, grid, "reverse complement"))


def _raw_call(d, counts, cap, present=PER_BASE, variants=True, stream=None, **th):
    """aix_pile_call_dev itself with 64 poisoned elements behind every output it is given; `present`: which of the four nullable
    outputs it is given -> dict: status, total, n_changed and the arrays as numpy (a variant array only up to cap)"""
    import torch as T
    th = dict(THRESHOLDS, **th)
    U, B = d["offsets"].numel() - 1, d["bases"].numel()
    outs = {"polished": _poison(B, T.uint8), "depth_sum": _poison(U, T.int64), "uncovered": _poison(U, T.int32)}
    outs = {k: (t if k in present else None) for k, t in outs.items()}
    var = [_poison(cap, ty) for ty in (T.int32, T.int32, T.uint8, T.uint8, T.int32, T.int32, T.int32)]
    changed, total = C.c_uint64(77), C.c_uint64(77)
    status = _lib.lib().aix_pile_call_dev(U, vp(d["offsets"].data_ptr()), _q(d["bases"]), _q(counts), th["min_depth"], th["min_major_permille"], th["min_alt_count"],
                                          th["min_alt_permille"], None if outs["polished"] is None else vp(outs["polished"].data_ptr()),
                                          C.byref(changed) if "n_changed" in present else None, *[vp(t.data_ptr()) if variants else None for t in var],
                                          cap if variants else 0, C.byref(total) if variants else None,
                                          None if outs["depth_sum"] is None else vp(outs["depth_sum"].data_ptr()),
                                          None if outs["uncovered"] is None else vp(outs["uncovered"].data_ptr()), stream)
    T.cuda.synchronize()
    res = dict(status=status, total=total.value, n_changed=changed.value)
    fits = status == 0 and variants and total.value <= cap
    assert all(_clean(t, total.value if fits else 0) for t in var), "a variant array written beyond the total, or at all without room"
    for k, n in (("polished", B), ("depth_sum", U), ("uncovered", U)):
        if outs[k] is not None:
            assert _clean(outs[k], n if status == 0 else 0), k
            res[k] = _np(outs[k][:n])
    if fits:
        res.update({k: _np(t[:total.value]) for k, t in zip(PR.VAR_KEYS, var)})
    return res


def _same_raw_call(got, want, present, variants, tag):
    assert got["status"] == 0, tag
    for k, dt in (("polished", np.uint8), ("depth_sum", np.uint64), ("uncovered", np.uint32)):
        if k in present:
            assert got[k].dtype == dt and np.array_equal(got[k], want[k]), (tag, k)
    assert got["n_changed"] == (want["n_changed"] if "n_changed" in present else 77), (tag, "n_changed")
    assert got["total"] == (want["total"] if variants else 77), (tag, "total")
    if variants:
        for k, dt in zip(PR.VAR_KEYS, PR.VAR_DTYPES):
            assert got[k].dtype == dt and np.array_equal(got[k], want[k]), (tag, k)


@pytest.mark.parametrize("pi", range(len(FC.CALL_PARAMS)))
def test_raw_cells(index, cell_wants, monkeypatch, pi):
    """3. cells_case under one threshold set of CALL_PARAMS through aix_pile_call_dev (room for exactly the total) and pile_call_t, under
    the default grid and 1 and 3 workgroups: everything equals the restatement. Sets 6 and 7 hold the permille thresholds of 2^31 under
    which a product that wraps at 2^64 turns OVERFLOW_CELLS into a variant site and a polished base."""
    c, wants = cell_wants
    th, want = FC.CALL_PARAMS[pi], wants[pi]
    d = _dev_graph(c)
    counts = _t(c["counts"])
    for grid in GRIDS:
        _set_grid(monkeypatch, grid)
        _same_raw_call(_raw_call(d, counts, want["total"], **th), want, PER_BASE, True, (pi, grid))
        TP._same_call(index.pile_call_t(d, counts, **th), want, (pi, grid, "pile_call_t"))


def test_every_base_a_variant_site_and_the_sizing_rule(cell_wants):
    """3b. All thresholds 0: total == B at cap 0, B - 1 (nothing written: the raw caller asserts the poison) and B."""
    c, wants = cell_wants
    want = wants[FC.CALL_PARAMS.index(FC.ZERO)]
    d, counts, B = _dev_graph(c), _t(c["counts"]), int(c["offsets"][-1])
    assert want["total"] == B
    for cap in (0, B - 1):
        got = _raw_call(d, counts, cap, **FC.ZERO)
        assert got["status"] == 0 and got["total"] == B and "var_pos" not in got and got["n_changed"] == want["n_changed"], cap
    _same_raw_call(_raw_call(d, counts, B, **FC.ZERO), want, PER_BASE, True, "cap == B")


def test_every_presence_pattern_of_the_nullable_outputs(cell_wants):
    """3c. The 2^4 presence patterns of polished, n_changed, depth_sum and uncovered, with and without variants: each present output
    equals the full call's (the restatement's), nothing else is written."""
    c, wants = cell_wants
    want = wants[FC.CALL_PARAMS.index(FC.LOOSE)]
    d, counts = _dev_graph(c), _t(c["counts"])
    for n in range(5):
        for present in itertools.combinations(PER_BASE, n):
            for variants in (True, False):
                got = _raw_call(d, counts, want["total"], present, variants, **FC.LOOSE)
                _same_raw_call(got, want, present, variants, (present, variants))


def test_empty_shapes():
    """4. U = 0 (offsets = [0], B = 0) for all three calls with M = 0 and with M > 0, R = T = 0: AIX_OK, a zeroed CSR, zeroed stats and
    counters, nothing else written. R > 0 with U = 0: AIX_ERR_ARG, nothing touched."""
    import torch as T
    L = _lib.lib()
    off0 = _t(np.zeros(1, np.uint64))
    for seqs in ([], [b"", b"ACGTTGCAAC" * 3, b""]):
        M = len(seqs)
        so = _t(FC._csr([len(s) for s in seqs]))
        st = _t(np.frombuffer(b"".join(seqs), np.uint8))
        csr = _t(np.zeros(M + 1, np.uint64))
        spo = _poison(M + 1, T.int64)
        n, circ = C.c_uint64(77), C.c_uint64(77)
        assert L.aix_pile_place_dev(M, _q(so) if M else None, _q(csr) if M else None, 0, *[None] * 5, 0, _q(off0), 46, 22, _q(spo), *[None] * 6, C.byref(n), C.byref(circ),
                                    None) == 0
        T.cuda.synchronize()
        assert (n.value, circ.value) == (0, 0) and not spo[:M + 1].any() and _clean(spo, M + 1), M
        d = dict(M=M, R=0, U=0, offsets=off0, bases=None, seqs=st, offs=so if M else None, **{k: None for k in ORDER})
        d["seq_place_off"] = csr if M else None
        status, m, s = _raw_pile(d, None)
        assert status == 0 and s.tolist() == [0, 0, 0], M
        assert _raw_pile(d, None, False, False)[0] == 0
        for present, variants in ((PER_BASE, True), ((), True), (PER_BASE, False), ((), False)):
            got = _raw_call({"offsets": off0, "bases": T.zeros(0, dtype=T.uint8, device="cuda")}, None, 0, present, variants)
            assert got["status"] == 0 and got["total"] == (0 if variants else 77) and got["n_changed"] == (0 if present else 77), (M, present, variants)
            assert all(got[k].shape[0] == 0 for k in present if k != "n_changed")
    c = FC.placements_case(0)
    d = dict(_dev_pile_input(c), U=0, offsets=off0)
    counts = _t(c["counts"])
    status, m, s = _raw_pile(d, counts)                              # (the raw caller asserts that place_mism and stats kept their poison)
    assert status == _lib.AIX_ERR_ARG and np.array_equal(_np(counts), c["counts"])
    T.cuda.synchronize()


def test_twice_and_on_a_side_stream(index, step_wants, place_wants):
    """5. One steps case and one placements case twice on the null stream and once on a stream of their own with the null stream busy:
    one digest. counts and place_mism come from atomics and are part of it."""
    import torch
    c, wants = step_wants(FC.SEEDS[1])
    graph, (st, so), dev_steps = _dev_graph(c), _dev_seqs(c), _dev_steps(c)
    pc, once, twice = place_wants(FC.PLACEMENT_SEEDS[2])
    d = _dev_pile_input(pc)

    def run(tag, stream=None):
        counts = _t(pc["counts"])
        status, m, s = _raw_pile(d, counts, stream=stream)
        assert status == 0
        _same_pile(counts, m, s, once, tag)
        return _steps_chain(index, c, wants, graph, st, so, dev_steps, tag) + hashlib.sha256(_np(counts).tobytes() + m.tobytes() + s.tobytes()).hexdigest()

    digests = [run("first"), run("again")]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    busy = torch.empty(1 << 24, dtype=torch.float32, device="cuda")
    busy.normal_()
    with torch.cuda.stream(side):
        digests.append(run("side", vp(side.cuda_stream)))
    torch.cuda.synchronize()
    assert len(set(digests)) == 1
