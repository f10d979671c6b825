"""Pins the test-side restatement of the repeat resolution (tests/graph_resolve_ref.py) and the inputs of tests/graph_resolve_cases.py,
without a GPU: literals, the planted genomes recovered as contigs, the properties of the contract, and the refusals of the handle-less
entry points that are decided before any device call."""
import ctypes as C

import numpy as np
import pytest

import graph_clean_ref as GR
import graph_resolve_cases as RC
import graph_resolve_ref as RR
import seqthread_cases as SC
import seqthread_ref as SR
import unitig_links_ref as RL
import unitigs_ref as R
from aindex_amd import _lib

NONE32 = RR.NONE32


def restated(p, reads=None):
    """(g, steps, pair_support, n_pairs) of a planted case: the restated graph, its reads threaded, the transitions counted"""
    un = R.unitigs(p.codes, p.tfs, 0)
    lk = RL.links(p.codes, p.tfs, 0, un)
    g = GR.graph(un, lk)
    node = SR.nodes(un["kid_unitig"], un["kid_pos"], un["kid_flag"], un["offsets"])
    kid_of = {int(c): i for i, c in enumerate(p.codes.tolist())}
    if reads is None:
        reads = p.reads if p.reads is not None else SC.batch(un, lk, 1).seqs
    steps = SR.thread(kid_of, node, g, reads, support=np.zeros(g["E"], np.uint64))
    pair, n = RR.pairs(g, steps)
    return dict(g, strings=un["strings"]), steps, pair, n, reads, (kid_of, node)


@pytest.fixture(scope="module")
def every():
    return {name: (RC.planted(name),) + restated(RC.planted(name)) for name in RC.PLANTED}


def as_graph(res):
    g = {k: res[k] for k in GR.GRAPH_KEYS}
    g["U"], g["E"] = res["U"], res["E"]
    return g


def test_literals_of_the_two_copy_repeat(every):
    """A R B and C R D: R is unitig 0 of 18 k-mers with two links at either end; every array of the resolution, written out."""
    p, g, steps, pair, n, reads, _ = every["two_copy"]
    assert len(reads) == 122 and g["offsets"].tolist() == [0, 40, 182, 324, 466, 608]
    assert g["link_off"].tolist() == [0, 2, 4, 5, 5, 6, 6, 7, 7, 7, 8] and g["link_to"].tolist() == [8, 3, 7, 5, 1, 0, 0, 1]
    assert g["tf_sum"].tolist() == [936, 2145, 2145, 2145, 2145]
    assert steps["support"].tolist() == [25] * 8 and n == 38
    assert pair.dtype == np.uint64 and pair.shape == (80,) and {int(i): int(pair[i]) for i in np.nonzero(pair)[0]} == {0: 19, 5: 19}
    res = RR.resolve(g, steps["support"], pair)
    want = {"offsets": [0, 40, 182, 324, 466, 608, 648], "circular": [0] * 6, "tf_sum": [468, 2145, 2145, 2145, 2145, 468],
            "tf_min": [52, 1, 1, 1, 1, 52], "tf_max": [52, 26, 26, 26, 26, 52], "link_off": [0, 1, 2, 3, 3, 4, 4, 5, 5, 5, 6, 7, 8],
            "link_to": [8, 7, 11, 10, 0, 1, 3, 5], "link_remove": [0] * 8, "copies": [2, 1, 1, 1, 1], "copy_base": [5, NONE32, NONE32, NONE32, NONE32],
            "unitig_origin": [0, 1, 2, 3, 4, 0]}
    for k, v in want.items():
        assert res[k].tolist() == v, k
    for k, dt in zip(GR.GRAPH_KEYS, (np.uint64, np.uint8, np.uint8, np.uint64, np.uint32, np.uint32, np.uint64, np.uint32)):
        assert res[k].dtype == dt, k
    assert res["bases"].tobytes().decode() == "".join(g["strings"]) + g["strings"][0]
    assert (res["U"], res["E"], res["n_links_removed"], res["n_split"], res["n_copies_added"]) == (6, 8, 0, 1, 1)
    lay = RR.layout(g, res["link_remove"], res["copies"])
    assert (lay["U"], lay["total_bases"], lay["E"]) == (6, 648, 8)


@pytest.mark.parametrize("name", [n for n in RC.PLANTED if n != "hairpin_ends"])
def test_planted_genomes_come_back_as_contigs(every, name):
    p, g, steps, pair, n, reads, _ = every[name]
    res = RR.resolve(g, steps["support"], pair)
    assert (res["n_split"], res["n_links_removed"]) == (p.n_split, p.n_removed)
    c = GR.compact(as_graph(res), np.zeros(res["U"], np.uint8))              # property (b): the compaction accepts G_r
    got = sorted(RC.canon_str(s) for s in c["strings"])
    if p.contigs is None:                                                 # nothing can be decided: the unitigs stay as they are
        assert res["U"] == g["U"] and got == sorted(RC.canon_str(s) for s in GR.compact(g, np.zeros(g["U"], np.uint8))["strings"])
    else:
        assert got == p.contigs and c["E"] == 0


def test_shapes_of_the_planted_repeats(every):
    d = {"two_copy": [2], "inverted": [2], "adjacent": [2, 2], "three_copy": [3], "four_copy": [4], "twice": [2], "ambiguous": [], "tandem": [],
         "weak_fork": []}
    for name, want in d.items():
        p, g, steps, pair, n, reads, _ = every[name]
        copies = RR.mark(g, steps["support"], pair)["copies"]
        assert sorted(copies[copies > 1].tolist()) == want, name
    p, g, steps, pair, n, reads, _ = every["ambiguous"]                   # three strong cells at the repeat: no matching
    u = int(np.argmax(np.diff(g["link_off"].astype(np.int64)).reshape(-1, 2).sum(1)))
    assert sorted(pair[16 * u:16 * u + 16][pair[16 * u:16 * u + 16] > 0].tolist()) == [19, 19, 19]
    p, g, steps, pair, n, reads, _ = every["tandem"]                      # the self-link, traversed
    src = np.repeat(np.arange(2 * g["U"]), np.diff(g["link_off"].astype(np.int64)))
    own = np.nonzero(g["link_to"] == src)[0]
    assert own.shape[0] == 2 and (steps["support"][own] >= 2).all()
    p, g, steps, pair, n, reads, _ = every["hairpin_ends"]
    hair = np.nonzero(g["link_to"] == (np.repeat(np.arange(2 * g["U"]), np.diff(g["link_off"].astype(np.int64))) ^ 1))[0]
    assert hair.shape[0] and n > 0


@pytest.mark.parametrize("name", RC.PLANTED)
def test_properties(every, name):
    p, g, steps, pair, n, reads, _ = every[name]
    # (a) nothing removed, nothing split: G_r == G and the origin is the identity
    same = RR.resolve(g, None, None)
    for k in GR.GRAPH_KEYS:
        assert same[k].dtype == g[k].dtype and np.array_equal(same[k], g[k]), k
    assert same["unitig_origin"].tolist() == list(range(g["U"])) and not same["link_remove"].any() and (same["copies"] == 1).all()
    same = RR.resolve(g, steps["support"], pair, 0, 0, 0)                 # thresholds of 0 switch the rules off
    assert same["U"] == g["U"] and same["E"] == g["E"]
    # (c) and duality
    res = RR.resolve(g, steps["support"], pair)
    assert res["E"] == g["E"] - res["n_links_removed"] and res["U"] - g["U"] == int((res["copies"].astype(np.int64) - 1).sum()) == res["n_copies_added"]
    assert sum(res["tf_sum"].tolist()) == sum(g["tf_sum"].tolist())
    RR.validate(as_graph(res))
    # sum over y of pair[u][x][.] <= the support of link x. A hairpin u+ -> u- is its own dual: the threading counts one traversal once,
    # but the sequence passes u twice there, forwards into the hairpin and backwards out of it, and both passes hit the cell of that link
    lo, to = g["link_off"].tolist(), g["link_to"].tolist()
    room = lambda e, j: int(steps["support"][j]) * (2 if to[j] == e ^ 1 else 1)
    for u in range(g["U"]):
        cell = pair[16 * u:16 * u + 16].reshape(4, 4)
        for x in range(lo[2 * u + 1] - lo[2 * u]):
            assert int(cell[x].sum()) <= room(2 * u, lo[2 * u] + x)
        for y in range(lo[2 * u + 2] - lo[2 * u + 1]):
            assert int(cell[:, y].sum()) <= room(2 * u + 1, lo[2 * u + 1] + y)
        assert not cell[lo[2 * u + 1] - lo[2 * u]:].any() and not cell[:, lo[2 * u + 2] - lo[2 * u + 1]:].any()


@pytest.mark.parametrize("name", ("two_copy", "inverted", "twice", "hairpin_ends"))
def test_a_batch_and_its_reverse_complement_give_the_same_pairs(every, name):
    p, g, steps, pair, n, reads, (kid_of, node) = every[name]
    back = [SC.rc(r.decode()).encode() if set(r) <= set(b"ACGT") else r for r in reads]
    pair2, n2 = RR.pairs(g, SR.thread(kid_of, node, g, back))
    assert n2 == n > 0 and np.array_equal(pair2, pair)
    twice, n3 = RR.pairs(g, steps, pair_support=pair)                     # accumulated, never zeroed
    assert n3 == n and np.array_equal(twice, pair * np.uint64(2))


@pytest.mark.parametrize("seed", (0, 1))
def test_link_structures(seed):
    g = RC.make_resolve_graph(seed)
    ml, mp, mn = g["thresholds"]
    res = RR.resolve(g, g["link_support"], g["pair_support"], ml, mp, mn)
    assert {c: int(res["copies"][c]) for c in g["want"]} == g["want"]
    assert sorted(set(g["want"].values())) == [1, 2, 3, 4] and res["n_links_removed"] > 0
    assert sum(res["tf_sum"].tolist()) == sum(g["tf_sum"].tolist()) and res["E"] == g["E"] - res["n_links_removed"]
    RR.validate(as_graph(res))
    assert (np.diff(res["link_off"].astype(np.int64))[2 * g["U"]:] == 1).all()          # every end of a copy has exactly one link
    src = np.repeat(np.arange(2 * g["U"]), np.diff(g["link_off"].astype(np.int64)))
    both = (res["copies"][src >> 1] > 1) & (res["copies"][g["link_to"] >> 1] > 1)         # links that join two split unitigs ...
    assert {(int(e) & 1, int(t) & 1) for e, t in zip(src[both], g["link_to"][both])} == {(0, 0), (0, 1), (1, 0), (1, 1)}   # ... in all four orientations
    # a product not taken in 128 bits gives other abundances
    big = [c for c in g["want"] if g["want"][c] == 4 and int(g["tf_sum"][c]) >= 1 << 33]
    assert big
    wrapped = 0
    for c in big:
        ids = [c] + [int(res["copy_base"][c]) + r for r in range(3)]
        parts = [int(res["tf_sum"][i]) for i in ids]
        assert sum(parts) == int(g["tf_sum"][c])
        cells = [int(v) for v in g["pair_support"][16 * c:16 * c + 16] if int(v) >= mp]
        tf, S = int(g["tf_sum"][c]), sum(cells)
        exact = sorted(tf * p // S for p in cells)
        assert len(cells) == 4 and all(part in exact for part in parts[1:])
        wrapped += exact != sorted(((tf * p) & RR.M64) // ((S & RR.M64) or 1) for p in cells)
    assert wrapped
    with pytest.raises(ValueError):
        RR.mark(RC.asymmetric(g), RC.asymmetric(g)["link_support"], g["pair_support"], ml, mp, mn)
    with pytest.raises(ValueError):
        RR.mark(g, g["link_support"], g["pair_support"], ml, mp, mp)                  # noise must lie below min_pair_support
    assert (RR.mark(g, None, g["pair_support"], ml, mp, mn)["link_remove"] == 0).all()
    assert (RR.mark(g, g["link_support"], None, ml, mp, mn)["copies"] == 1).all()


def test_refusals_of_the_restatement(every):
    p, g, steps, pair, n, reads, _ = every["two_copy"]
    bad = dict(steps, step_link=steps["step_link"].copy())
    bad["step_link"][0] = 0
    with pytest.raises(ValueError):
        RR.pairs(g, bad)
    linked = steps["step_link"] < g["E"]
    i = int(np.nonzero(linked[:-1] & linked[1:])[0][0])                   # a transition
    bad = dict(steps, step_link=steps["step_link"].copy())
    bad["step_link"][i] = g["E"]
    with pytest.raises(ValueError):
        RR.pairs(g, bad)
    bad = dict(steps, step_unitig=steps["step_unitig"].copy())
    bad["step_unitig"][i] = (int(steps["step_unitig"][i]) + 1) % g["U"]       # the link does not enter that unitig
    with pytest.raises(ValueError):
        RR.pairs(g, bad)
    copies = np.array([2, 1, 1, 1, 1], np.uint8)
    with pytest.raises(ValueError):
        RR.emit(g, np.zeros(8, np.uint8), copies, None)
    with pytest.raises(ValueError):
        RR.emit(g, np.zeros(8, np.uint8), np.array([1, 2, 1, 1, 1], np.uint8), pair)
    with pytest.raises(ValueError):
        RR.emit(g, np.array([1, 0, 0, 0, 0, 0, 0, 0], np.uint8), np.ones(5, np.uint8), pair)   # removed without its dual
    with pytest.raises(ValueError):
        RR.layout(g, np.zeros(8, np.uint8), np.array([5, 1, 1, 1, 1], np.uint8))


def test_null_pointers_are_refused_before_any_device_call():
    """Runs without a GPU: the handle-less entry points decide a NULL pointer and an impossible size before anything is allocated or
    launched."""
    L = _lib.lib()
    a = np.zeros(64, np.uint64)
    p = a.ctypes.data_as(C.c_void_p)
    n = [C.c_uint64(77) for _ in range(4)]
    r = [C.byref(x) for x in n]
    ARG, UNS = _lib.AIX_ERR_ARG, _lib.AIX_ERR_UNSUPPORTED
    assert L.aix_thread_pairs_dev(1, None, p, 1, 3, p, p, p, p, r[0], None) == ARG
    assert L.aix_thread_pairs_dev(1, p, None, 1, 3, p, p, p, p, r[0], None) == ARG
    assert L.aix_thread_pairs_dev(1, p, p, 1, 3, p, None, p, p, r[0], None) == ARG
    assert L.aix_thread_pairs_dev(1, p, p, 1, 3, p, p, p, None, r[0], None) == ARG
    assert L.aix_thread_pairs_dev(1, p, p, 1, 3, p, p, p, p, None, None) == ARG
    assert L.aix_thread_pairs_dev(1, p, p, 9, 3, p, p, p, p, r[0], None) == ARG
    assert L.aix_thread_pairs_dev((1 << 31) - 3, p, p, 1, 3, p, p, p, p, r[0], None) == UNS
    assert L.aix_thread_pairs_dev(1, p, p, 1, 0, None, None, None, p, r[0], None) == 0 and n[0].value == 0
    n[0].value = 77
    mark = lambda **o: L.aix_graph_resolve_mark_dev(*[o.get(k, v) for k, v in (("U", 1), ("off", p), ("circ", p), ("lo", p), ("to", p), ("E", 1), ("sup", p), ("pair", p),
                                                                                 ("ml", 2), ("mp", 2), ("mn", 0), ("rm", p), ("cp", p), ("n0", r[0]), ("n1", r[1]), ("n2", r[2]),
                                                                                 ("st", None))])
    for k in ("off", "circ", "lo", "to", "rm", "cp", "n0", "n1", "n2"):
        assert mark(**{k: None}) == ARG, k
    assert mark(E=9) == ARG and mark(mn=2) == ARG and mark(U=(1 << 31) - 3) == UNS
    assert L.aix_graph_resolve_layout_dev(1, None, 1, p, p, p, r[0], r[1], r[2], None) == ARG
    assert L.aix_graph_resolve_layout_dev(1, p, 1, p, None, p, r[0], r[1], r[2], None) == ARG
    assert L.aix_graph_resolve_layout_dev(1, p, 1, p, p, p, r[0], None, r[2], None) == ARG
    assert L.aix_graph_resolve_layout_dev((1 << 31) - 3, p, 1, p, p, p, r[0], r[1], r[2], None) == UNS
    emit = lambda **o: L.aix_graph_resolve_emit_dev(*[o.get(k, v) for k, v in (("U", 1), ("a0", p), ("a1", p), ("a2", p), ("a3", p), ("a4", p), ("a5", p), ("a6", p), ("a7", p),
                                                                                 ("E", 1), ("rm", p), ("cp", p), ("cb", p), ("pair", p), ("mp", 2), ("U2", 1), ("tot", 23),
                                                                                 ("E2", 1), ("o0", p), ("o1", p), ("o2", p), ("o3", p), ("o4", p), ("o5", p), ("o6", p),
                                                                                 ("o7", p), ("og", p), ("st", None))])
    for k in ["a%d" % i for i in range(8)] + ["rm", "cp", "cb"] + ["o%d" % i for i in range(8)] + ["og"]:
        assert emit(**{k: None}) == ARG, k
    assert emit(U2=0) == ARG and emit(U2=5) == ARG and emit(E2=2) == ARG and emit(o1=C.c_void_p(p.value + 1)) == ARG and emit(U=(1 << 31) - 3) == UNS
    assert all(x.value == 77 for x in n)
    host = lambda **o: L.aix_graph_resolve(*[o.get(k, v) for k, v in (("U", 1), ("a0", p), ("a1", p), ("a2", p), ("a3", p), ("a4", p), ("a5", p), ("a6", p), ("a7", p),
                                                                        ("E", 1), ("sup", None), ("pair", None), ("ml", 2), ("mp", 2), ("mn", 0))], *r,
                                           *[C.byref(C.c_void_p()) for _ in range(11)])
    for k in ["a%d" % i for i in range(8)]:
        assert host(**{k: None}) == ARG, k
    assert host(E=9) == ARG and host(U=(1 << 31) - 3) == UNS
    assert host() == ARG                                                  # offsets[1] == 0: no unitig of 23 bases
