"""Gap closing on the GPU on tangled graphs (tests/gap_close_fuzz_cases.py): the searches of different joins meet, paths share contigs,
the path total exceeds U, joins cut from a cycle close, lengths pass 2^32. Every array equals the restatement (tests/gap_close_ref.py),
which test_gap_close_fuzz_cpu.py pins to a second opinion and whose inputs it shows to reach these situations; the property checks of
tests/gap_close_walks.py then run on the GPU's own arrays. Exact equality throughout; the raw callers are those of test_gpu_gap_close.py
and test_gpu_scaffold.py, with their poisoned tails and untouched-on-refusal asserts."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import gap_close_fuzz_cases as FC
import gap_close_ref as GF
import gap_close_walks as W
import scaffold_cases as SC
import scaffold_ref as SF
import test_gpu_gap_close as TG
import test_gpu_scaffold as TS
from aindex_amd.engine import Index

GRAPH, CLOSE, FILL = TG.GRAPH, TG.CLOSE, TG.FILL
_t, _np = TG._t, TG._np
GRIDS = (None, "1", "3")


def _set_grid(monkeypatch, grid):
    if grid is None:
        monkeypatch.delenv("AIX_UG_TEST_GRID", raising=False)
    else:
        monkeypatch.setenv("AIX_UG_TEST_GRID", grid)


def _signed(res, *keys):
    """a raw result with its signed arrays read as signed (the raw callers hand every 64-bit array out unsigned)"""
    return dict(res, **{k: res[k].view(np.int64) for k in keys})


def _search(g, **p):
    return GF.search(*[g[k] for k in GRAPH], **p)


@pytest.fixture(scope="module")
def tangled():
    """a tangled graph with the restatement's members, and its filled arrays per parameter set: made once, shared, left unchanged"""
    made = {}

    def get(seed, U=128, params=None):
        if (seed, U) not in made:
            g = FC.tangled(seed, U)
            made[seed, U] = (g, TG._members(g), {})
        g, em, wants = made[seed, U]
        if params is None:
            return g, em
        key = tuple(sorted(params.items()))
        if key not in wants:
            wants[key] = TG._want(g, em, params)
        return g, em, wants[key]
    return get


@pytest.fixture(scope="module")
def index(tmp_path_factory):
    """an index to hang the engine methods on: they take arrays, but live on a handle"""
    p = SC.planted("two_copy")
    prefix = TG._write_index(str(tmp_path_factory.mktemp("gcf") / "two_copy"), p.codes, p.tfs)
    with Index.open_23(prefix + ".pf", prefix + ".tf.bin", prefix + ".kmers.bin") as ix:
        yield ix


def _gpu_scaffolds(gt, g):
    """bundle, mark, layout and emit from the observations, each fed the arrays of the one before"""
    st, S, sl = TS._raw_bundle(_t(g["obs_key"]), _t(g["obs_d"]), g["U"])
    assert st == 0
    mk = TS._raw_mark(gt, {k: _t(sl[k]) for k in TS.SLINK}, g["params"])
    lay = TS._raw_layout(gt["offsets"], mk["tensors"])
    em = TS._raw_emit(gt, mk["tensors"], lay["tensors"], lay["n_scaffolds"], lay["total_bases"])
    assert mk["status"] == 0 and lay["status"] == 0 and em["status"] == 0
    return mk, em


@pytest.mark.parametrize("pi", range(len(FC.PARAM_SETS)))
@pytest.mark.parametrize("seed", FC.SEEDS)
def test_tangled(tangled, monkeypatch, seed, pi):
    """1. From the observations to the filled bases, every stage on the GPU arrays of the stage before and equal to its restatement, with
    the default grid and with 1 and 3 workgroups (one workgroup takes a search of thousands of states and then a tiny one from the same
    LDS); then the property checks on what the GPU wrote."""
    p = FC.PARAM_SETS[pi]
    g, em_w, want = tangled(seed, params=p)
    gt = TG._dev(g, GRAPH[:3] + ("bases", "circular"))
    key_t, d_t = _t(g["obs_key"]), _t(g["obs_d"])
    for grid in GRIDS:
        _set_grid(monkeypatch, grid)
        tag = (seed, pi, grid)
        _, mk, _, em = TS._scaffold_all(gt, g, key_t, d_t, g["obs_key"], g["obs_d"], g["params"], tag)
        assert np.array_equal(mk["join"], g["join"]) and np.array_equal(mk["join_gap"], g["join_gap"]) and np.array_equal(em["member"], em_w["member"])
        gj = dict(gt, join=mk["tensors"]["join"], join_gap=mk["tensors"]["join_gap"])
        _, cl, fl = TG._fill_all(gj, g, em, p, tag, want=want)
        if grid is None:
            eb = TG._raw_fill_emit(gj, fl["tensors"], fl["n_fmembers"], fl["total_bases"])
            assert eb["status"] == 0
            cl = _signed(cl, "close_dist")
            W.check_closure(g, p, cl)
            W.check_fill(g, em, cl, dict(_signed(fl, "fmember_gap"), fscaffold_bases=eb["fscaffold_bases"]))


@pytest.mark.parametrize("seed", FC.SEEDS)
def test_nothing_closed_is_the_plain_scaffold(tangled, seed):
    """2. Without links, and with max_fill = 0 once the direct links e -> t are gone, no join closes: the filled arrays are the arrays of
    aix_scaffold_emit_dev. GPU against GPU: the two instantiations of the base emitter agree."""
    g, _ = tangled(seed)
    U = g["U"]
    bare = dict(g, link_off=np.zeros(2 * U + 1, np.uint64), link_to=np.zeros(0, np.uint32), E=0)
    for h, p, tag in ((bare, FC.PARAM_SETS[1], "E = 0"), (FC.without_direct_links(g), dict(FC.PARAM_SETS[1], max_fill=0), "max_fill = 0")):
        gt = TG._dev(h, GRAPH[:3] + ("bases", "circular"))
        mk, em = _gpu_scaffolds(gt, h)
        gj = dict(gt, join=mk["tensors"]["join"], join_gap=mk["tensors"]["join_gap"])
        cl = TG._raw_close(gj, p)
        assert cl["status"] == 0 and cl["total"] == 0 and cl["counts"][0] == 0 and cl["counts"][4] == mk["n_joins"] > 0 and not cl["fill_uses"].any(), tag
        fl = TG._raw_fill_layout(gj, {k: _t(em[k]) for k in ("member_off", "member")}, cl["tensors"])
        assert fl["status"] == 0 and fl["n_fmembers"] == U and not fl["fmember_flag"].any(), tag
        eb = TG._raw_fill_emit(gj, fl["tensors"], fl["n_fmembers"], fl["total_bases"])
        assert eb["status"] == 0
        for a, b in (("fscaffold_offsets", "scaffold_offsets"), ("fmember_off", "member_off"), ("fmember", "member")):
            assert np.array_equal(fl[a], em[b]), (tag, a)
        assert np.array_equal(fl["fmember_gap"].view(np.int64), em["member_gap"]) and np.array_equal(eb["fscaffold_bases"], em["scaffold_bases"]), tag
        assert fl["total_bases"] == em["scaffold_bases"].shape[0] and (em["scaffold_bases"] == ord("N")).any()


def test_shared_corridor(index):
    """3. k joins through one chain of m contigs: the path total k m exceeds U, so a caller that made room for U entries is told the
    total and handed no entry, and the engine method and the host form take their second pass."""
    g, p = FC.corridor(), FC.CORRIDOR_PARAMS
    U, k = g["U"], 8
    em = TG._members(g)
    want = TG._want(g, em, p)
    T = want["total"]
    assert T == k * len(g["corridor"]) > U and all(want["fill_uses"][u] == k for u in g["corridor"])
    gt = TG._dev(g)
    cl = TG._raw_close(gt, p, cap=U)                                       # (the raw caller asserts that no path entry was touched)
    assert cl["status"] == 0 and cl["total"] == T and "path" not in cl
    TG._same(cl, want, [x for x in CLOSE if x != "path"], "cap = U")
    cl = TG._raw_close(gt, p, cap=T)
    assert cl["status"] == 0 and cl["total"] == T
    TG._same(cl, want, CLOSE, "cap = total")
    _, cl, fl = TG._fill_all(gt, g, em, p, "corridor", want=want)
    W.check_closure(g, p, _signed(cl, "close_dist"))
    W.check_fill(g, em, _signed(cl, "close_dist"), dict(_signed(fl, "fmember_gap"), fscaffold_bases=want["fscaffold_bases"]))
    fo, fm = fl["fmember_off"].tolist(), fl["fmember"].tolist()
    multi = [s for s in range(len(fo) - 1) if em["member_off"][s + 1] - em["member_off"][s] > 1]
    assert len(multi) == k and all({w >> 1 for w in fm[fo[s]:fo[s + 1]]} >= set(g["corridor"]) for s in multi)
    joins = {"join": gt["join"], "join_gap": gt["join_gap"]}
    for hint in (0, U, T):
        ec = index.gap_close_t(gt, joins, cap_hint=hint, **p)
        TG._same({x: _np(v) for x, v in ec.items() if hasattr(v, "cpu")}, want, CLOSE[:6], ("engine search", hint))
        assert ec["counts"] == want["counts"].tolist() and ec["total"] == T and ec["path"].numel() == T
    ef = index.scaffold_fill_t(gt, joins, {x: _t(em[x]) for x in ("member_off", "member")}, ec, 1)
    TG._same({x: _np(v) for x, v in ef.items() if hasattr(v, "cpu")}, want, FILL, "engine fill")
    host = index.scaffold_fill(*[g[x] for x in ("offsets", "bases", "link_off", "link_to", "join", "join_gap")], em["member_off"], em["member"], **p, min_gap=1)
    TG._same(host, want, CLOSE[:6] + FILL, "host")
    assert (host["counts"], host["total"], host["n_fmembers"], host["total_bases"]) == (want["counts"].tolist(), T, want["n_fmembers"], want["total_bases"])


def test_budget_and_fill_edges(tangled):
    """4. max_states at exactly the states of a join's complete search and one below, for the smallest and largest such counts and those
    nearest the round of 64 and twice it; max_fill at 0, 1, 2 and 64; tolerance at 0 and 2^20."""
    g, _ = tangled(*FC.SMALL)
    full = _search(g, **FC.FULL)
    ns, sets = FC.edge_param_sets(full)
    assert len(ns) >= 10 and min(ns) <= 2 and max(ns) > 256 and min(abs(n - 64) for n in ns) <= 1 and min(abs(n - 128) for n in ns) <= 9
    gt = TG._dev(g)
    owners = [e for e, t in enumerate(g["join"].tolist()) if t != SF.NONE32 and e < t ^ 1]
    for p in sets:
        cl = TG._raw_close(gt, p)
        assert cl["status"] == 0
        TG._same(cl, _search(g, **p), CLOSE, p)
        m = p["max_states"]
        for e in owners:                                                   # (tolerance and max_fill as in the complete search: its counts apply)
            if p["tolerance"] == FC.FULL["tolerance"] and p["max_fill"] == FC.FULL["max_fill"] and full["close_status"][e] != 4:
                n = int(full["close_states"][e])
                assert (cl["close_status"][e], cl["close_states"][e]) == ((full["close_status"][e], n) if n <= m else (4, m)), (p, e)


def test_giant_lengths():
    """5. A distance of 2^30 + 2^20 stored and reported, contigs of 2^33 and 2^40 bases dropped and not wrapped, a gap of -2^30, filled
    positions beyond 2^32. No bases: the search and the layout read none."""
    g, p = FC.giant(), FC.GIANT_PARAMS
    gt = TG._dev(g, GRAPH)
    want = _search(g, **p)
    assert want["close_dist"][2] == (1 << 30) + (1 << 20) == int(g["join_gap"][2]) + p["tolerance"] and want["counts"].tolist() == [1, 2, 0, 0, 3]
    cl = TG._raw_close(gt, p)
    assert cl["status"] == 0
    TG._same(cl, want, CLOSE, "giant")
    less = dict(p, tolerance=p["tolerance"] - 1)
    c2 = TG._raw_close(gt, less)
    TG._same(c2, _search(g, **less), CLOSE, "giant, one base of tolerance fewer")
    assert c2["close_status"][2] == 2 and c2["total"] == 0
    wl = GF.fill_layout(*[g[x] for x in GRAPH], g["member_off"], g["member"], want)
    fl = TG._raw_fill_layout(gt, {x: _t(g[x]) for x in ("member_off", "member")}, cl["tensors"])
    assert fl["status"] == 0 and (fl["n_fmembers"], fl["total_bases"]) == (wl["n_fmembers"], wl["total_bases"])
    TG._same(fl, wl, FILL[:6], "giant layout")
    assert fl["fmember_pos"][4] > 1 << 33 and fl["total_bases"] > 1 << 40
    W.check_closure(g, p, _signed(cl, "close_dist"))
    W.check_fill(g, g, _signed(cl, "close_dist"), _signed(fl, "fmember_gap"))


def test_twice_and_on_a_side_stream(tangled):
    """6. The same case twice on the null stream and once on a stream of its own with the null stream busy: one digest. fill_uses comes
    from atomics and is part of it."""
    import torch
    p = FC.PARAM_SETS[1]
    g, em, want = tangled(FC.SEEDS[0], params=p)
    gt = TG._dev(g)
    digests = []
    for _ in range(2):
        _, cl, fl = TG._fill_all(gt, g, em, p, "again", want=want)
        digests.append(TG._digest(cl, CLOSE) + TG._digest(fl, FILL[:6]))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    busy = torch.empty(1 << 24, dtype=torch.float32, device="cuda")
    busy.normal_()
    with torch.cuda.stream(side):
        _, cl, fl = TG._fill_all(gt, g, em, p, "side", stream=TG.vp(side.cuda_stream), want=want)
    torch.cuda.synchronize()
    digests.append(TG._digest(cl, CLOSE) + TG._digest(fl, FILL[:6]))
    assert len(set(digests)) == 1 and want["fill_uses"].max() > 1
