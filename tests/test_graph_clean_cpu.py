"""Graph cleaning without a GPU: the four entry points are declared, exported and typed; the test-side restatement
(tests/graph_clean_ref.py) is pinned with literal answers and held to the two properties of the contract; the array checker
(tests/graph_clean_check.py) accepts it and rejects wrong answers. test_gpu_graph_clean.py holds the kernels to this restatement."""
import itertools

import numpy as np
import pytest

import graph_cases as G
import graph_clean_check as GK
import graph_clean_ref as GR
import unitig_links_cases as LC
import unitig_links_ref as RL
import unitigs_cases as UC
import unitigs_ref as R

NONE32 = GR.NONE32
SEEDS = (0, 3, 6, 9)


def _both(codes, tfs, cutoff):
    un = R.unitigs(codes, tfs, cutoff)
    return un, RL.links(codes, tfs, cutoff, un)


def _graph(codes, tfs, cutoff=0):
    un, lk = _both(codes, tfs, cutoff)
    return un, GR.graph(un, lk)


def _same_graph(a, b, tag=""):
    for k in GR.GRAPH_KEYS:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (tag, k)


def _reduced(codes, tfs, cutoff, un, remove):
    """the graph of the index that holds only the k-mers of the surviving unitigs"""
    ku = un["kid_unitig"].tolist()
    keep = np.array([t > cutoff and remove[u] == 0 for u, t in zip(ku, tfs.tolist())], dtype=bool)
    return _graph(codes[keep], tfs[keep], cutoff)[1]


def _property_b(codes, tfs, cutoff, remove, tag):
    un, g = _graph(codes, tfs, cutoff)
    got = GR.compact(g, remove)
    GK.check(g, remove, got)
    a, b = GR.canonical_form(got), GR.canonical_form(_reduced(codes, tfs, cutoff, un, remove))
    assert a["strings"] == b["strings"], tag
    for k in ("offsets", "circular", "tf_sum", "tf_min", "tf_max", "link_off", "link_to"):
        assert np.array_equal(a[k], b[k]), (tag, k)
    return got


def test_entry_points_are_declared_exported_and_typed():
    import ctypes as C
    import os
    from aindex_amd import _lib
    names = {"aix_graph_mark_dev": 14, "aix_graph_compact_layout_dev": 16, "aix_graph_compact_emit_dev": 26, "aix_graph_clean": 28}
    declared = _lib.header_symbols()
    header = open(os.path.join(_lib.ROOT, "include", "aindex_hip.h")).read()
    L = _lib.lib()
    for name, n_args in names.items():
        assert name in declared and name in _lib.SIGNATURES and hasattr(L, name), name
        assert _lib.SIGNATURES[name][0] is C.c_int32 and len(_lib.SIGNATURES[name][1]) == n_args, name
    assert "#define AIX_GRAPH_MAX_THRESHOLD 32767u" in header and _lib.GRAPH_MAX_THRESHOLD == GR.MAX_THRESHOLD == 32767
    # the refusals that need no device: NULL arrays, thresholds, sizes
    ARG, UNS = _lib.AIX_ERR_ARG, _lib.AIX_ERR_UNSUPPORTED
    n = [C.c_uint64(77) for _ in range(4)]
    r = [C.byref(x) for x in n]
    one = C.c_void_p(0x1000)
    assert L.aix_graph_mark_dev(1, None, None, None, None, None, 0, None, 46, 46, None, r[0], r[1], None) == ARG
    assert L.aix_graph_mark_dev(1, one, one, one, one, one, 0, None, 32768, 46, one, r[0], r[1], None) == ARG
    assert L.aix_graph_mark_dev(1, one, one, one, one, one, 0, None, 46, 32768, one, r[0], r[1], None) == ARG
    assert L.aix_graph_mark_dev(1, one, one, one, one, one, 9, one, 46, 46, one, r[0], r[1], None) == ARG      # E > 8 U
    assert L.aix_graph_mark_dev(2 ** 31 - 3, one, one, one, one, one, 0, None, 46, 46, one, r[0], r[1], None) == UNS
    assert L.aix_graph_compact_layout_dev(1, None, None, None, None, None, 0, None, None, None, None, *r, None) == ARG
    assert L.aix_graph_compact_layout_dev(2 ** 31 - 3, one, one, one, one, one, 0, one, one, one, one, *r, None) == UNS
    assert L.aix_graph_compact_emit_dev(1, *[None] * 8, 0, *[None] * 4, 0, 0, 0, *[None] * 8, None) == ARG
    assert L.aix_graph_compact_emit_dev(1, *[one] * 8, 0, *[one] * 4, 2, 23, 0, *[one] * 8, None) == ARG        # C > U
    assert L.aix_graph_clean(1, *[None] * 8, 0, 46, 46, *r, *[None] * 12) == ARG
    assert [x.value for x in n] == [77] * 4


def test_pinned_bubble_snp_equals_the_next_cutoff():
    case = LC.link_cases()["bubble_snp"]
    un, g = _graph(case.codes, case.tfs, 0)
    remove = GR.mark(g, 46, 46)
    (arm,) = np.nonzero(remove)[0].tolist()
    assert remove.tolist().count(2) == 1 and g["tf_sum"][arm] == 2 * 23 and g["tf_min"][arm] == 2     # the weak arm (tf 2)
    got = GR.compact(g, remove)
    _same_graph(got, _graph(case.codes, case.tfs, 3)[1], "bubble_snp")
    assert got["C"] == 1 and got["E"] == 0 and got["offsets"].tolist() == [0, 18 + 18 + 23 + 22] and got["tf_sum"].tolist() == [5 * 59]
    assert got["unitig_contig"].tolist().count(NONE32) == 1 and sorted(got["unitig_pos"].tolist()) == [0, 0, 18, 41]
    GK.check(g, remove, got)
    assert GR.mark(g, 0, 0).tolist() == [0] * 4 and GR.mark(g, 46, 22).tolist() == [0] * 4             # switched off; an arm longer than the threshold
    assert GR.mark(g, 0, 23).tolist() == remove.tolist()


def test_pinned_tip_cases_equal_the_next_cutoff():
    topo, link = UC.topology_cases(), LC.link_cases()
    for name, case, removed, pinned in (("tip_of_one", link["tip_of_one"], [1], [0, 38 + 22]),
                                        ("bubble_tip_cutoff", topo["bubble_tip_cutoff"], [1, 2], [0, 79 + 22])):
        un, g = _graph(case.codes, case.tfs, 0)
        remove = GR.mark(g, 46, 46)
        assert sorted(remove[remove != 0].tolist()) == removed, name
        got = GR.compact(g, remove)
        _same_graph(got, _graph(case.codes, case.tfs, 3)[1], name)
        assert got["offsets"].tolist() == pinned and got["E"] == 0, name
        GK.check(g, remove, got)
    case = link["tip_of_one"]                                       # a tip of one k-mer survives a threshold of 0 and is clipped at 1
    _, g = _graph(case.codes, case.tfs, 0)
    assert not GR.mark(g, 0, 46).any() and GR.mark(g, 1, 0).tolist().count(1) == 1


def _fork(tf_a, tf_b, seed=401):
    """a stem of 18 k-mers that forks into two tips of 11 k-mers with abundance tf_a and tf_b"""
    for s in itertools.count(seed):
        ks = UC._Keys(s)
        stem = ks.base(40)
        a = ks.add(stem + [0] + ks.base(10), tf=[5] * 18 + [tf_a] * 11)
        b = ks.add(stem[-22:] + [1] + ks.base(10), tf=tf_b)
        if a is not None and b is not None:
            codes, tfs = ks.arrays()
            return codes, tfs, a[18:], b


def test_forks_of_two_candidate_tips():
    for tf_a, tf_b in ((9, 5), (5, 9), (5, 5)):
        codes, tfs, ka, kb = _fork(tf_a, tf_b)
        un, g = _graph(codes, tfs, 0)
        assert g["U"] == 3 and sorted(LC.members(un).tolist()) == [11, 11, 18]
        ua, ub = (int(UC._unitig_of(codes, un, k)[0]) for k in (ka, kb))
        remove = GR.mark(g, 46, 0)
        loser = (ub if tf_a > tf_b else ua) if tf_a != tf_b else max(ua, ub)     # the stronger one stays; equal means: the smaller id
        assert np.nonzero(remove)[0].tolist() == [loser] and remove[loser] == 1, (tf_a, tf_b)
        got = GR.compact(g, remove)
        assert got["C"] == 1 and got["offsets"].tolist() == [0, 18 + 11 + 22] and got["E"] == 0
        assert got["tf_sum"].tolist() == [5 * 18 + 11 * (max(tf_a, tf_b))] and got["tf_min"].tolist() == [5] and got["tf_max"].tolist() == [max(tf_a, tf_b, 5)]
        _property_b(codes, tfs, 0, remove, (tf_a, tf_b))
        assert GR.mark(g, 10, 0).tolist() == [0, 0, 0]               # both tips are longer than the threshold


def _lollipop_two_stems(seed=411, m=64):
    """a ring of m k-mers entered by two stems of 30 k-mers, in front of its k-mers 0 and 20: the ring is two linear unitigs"""
    for s in itertools.count(seed):
        ks = UC._Keys(s)
        ring = (lambda unit: (unit * (R.K // m + 2))[: m + R.K - 1])(ks.base(m))
        if ks.add(ks.base(30) + ring) is not None and ks.add(ks.base(30) + ring[20:42]) is not None:
            return ks.arrays()


def test_lollipops_close_into_circular_contigs():
    codes, tfs = _lollipop_two_stems()
    un, g = _graph(codes, tfs, 0)
    assert sorted(LC.members(un).tolist()) == [20, 30, 30, 44] and un["n_circular"] == 0
    remove = GR.mark(g, 46, 46)
    ring = np.nonzero(remove == 0)[0].tolist()
    assert remove.tolist().count(1) == 2 and sorted(LC.members(un)[ring].tolist()) == [20, 44]
    got = _property_b(codes, tfs, 0, remove, "two stems")
    assert got["C"] == 1 and got["circular"].tolist() == [1] and got["E"] == 0 and got["offsets"].tolist() == [0, 64 + 22]
    first = min(ring)                                               # it starts at its smallest member, forwards
    assert got["chains"][0][0] == (first, 0) and got["unitig_pos"][first] == 0 and got["unitig_flag"][first] == 2
    assert got["strings"][0][: 22 + LC.members(un)[first]] == un["strings"][first]
    assert got["unitig_flag"][max(ring)] & 2 and got["unitig_pos"][max(ring)] == LC.members(un)[first]
    # the ring of the topology case is ONE unitig with the link u+ -> u+: clipping the stem closes it on itself
    case = UC.topology_cases()["lollipop"]
    un, g = _graph(case.codes, case.tfs, 0)
    remove = GR.mark(g, 46, 46)
    assert remove.tolist().count(1) == len(UC.LOLLIPOPS)
    got = _property_b(case.codes, case.tfs, 0, remove, "lollipop")
    assert got["C"] == len(UC.LOLLIPOPS) and got["circular"].tolist() == [1] * got["C"] and got["E"] == 0
    assert sorted(LC.members(got).tolist()) == sorted(UC.LOLLIPOPS) and (got["unitig_flag"][remove == 0] == 2).all()


def test_hairpins_and_homopolymers_are_never_merged():
    codes = np.array([0], dtype=np.uint64)                          # A * 23: u+ -> u+ and u- -> u-, one k-mer
    un, g = _graph(codes, np.ones(1, np.uint32))
    got = GR.compact(g, np.zeros(1, np.uint8))
    _same_graph(got, g)
    assert got["circular"].tolist() == [0] and got["link_to"].tolist() == [0, 1] and got["unitig_flag"].tolist() == [0]
    for name in ("hairpin_ends", "selfloop"):
        case = UC.topology_cases()[name]
        un, g = _graph(case.codes, case.tfs, 0)
        got = GR.compact(g, np.zeros(g["U"], np.uint8))
        _same_graph(got, g, name)
        assert not got["circular"].any() and got["unitig_contig"].tolist() == list(range(g["U"]))
    case = LC.link_cases()["near_hairpin_arm"]                      # the tip goes; the arm that ends in a hairpin keeps its link u+ -> u-
    un, g = _graph(case.codes, case.tfs, 0)
    got = _property_b(case.codes, case.tfs, 0, GR.mark(g), "near_hairpin_arm")
    assert got["C"] == 1 and got["E"] == 1 and got["circular"].tolist() == [0] and int(got["link_to"][0]) in (0, 1)


@pytest.mark.parametrize("seed", SEEDS)
def test_property_a_the_identity(seed):
    codes, tfs = G.make_graph_case(seed)[:2]
    for cutoff in (0, 3):
        un, g = _graph(codes, tfs, cutoff)
        got = GR.compact(g, np.zeros(g["U"], np.uint8))
        _same_graph(got, g, (seed, cutoff))
        assert got["unitig_contig"].tolist() == list(range(g["U"])) and not got["unitig_pos"].any() and not got["unitig_flag"].any()
        assert got["n_circular"] == un["n_circular"]
        GK.check(g, np.zeros(g["U"], np.uint8), got)


@pytest.mark.parametrize("seed", SEEDS)
def test_property_b_random_masks(seed):
    codes, tfs = G.make_graph_case(seed)[:2]
    un, g = _graph(codes, tfs, 0)
    U = g["U"]
    rng = np.random.default_rng(1000 + seed)
    but_one = np.ones(U, np.uint8)
    but_one[int(rng.integers(0, U))] = 0
    for tag, remove in (("10 %", (rng.random(U) < 0.1).astype(np.uint8)), ("50 %", (rng.random(U) < 0.5).astype(np.uint8)), ("all", np.ones(U, np.uint8)),
                        ("all but one", but_one), ("mark", GR.mark(g))):
        got = _property_b(codes, tfs, 0, remove, (seed, tag))
        if tag == "all":
            assert got["C"] == 0 and got["offsets"].tolist() == [0] and got["link_off"].tolist() == [0]
        if tag == "all but one":
            assert got["C"] == 1


def test_pinned_graph_case_and_rounds():
    codes, tfs = G.make_graph_case(0)[:2]
    un, g = _graph(codes, tfs, 0)
    remove = GR.mark(g)
    got = GR.compact(g, remove)
    assert (g["U"], int((remove == 1).sum()), int((remove == 2).sum()), got["C"], got["n_circular"]) == (585, 39, 0, 522, 4)
    final, rounds = GR.clean(g, 46, 46, 8)
    assert 1 <= rounds < 8 and not GR.mark(final).any()              # a fixed point
    GK.check_graph(final)
    assert GR.clean(g, 0, 0, 3)[1] == 0


def test_checker_rejects_wrong_answers():
    case = UC.topology_cases()["bubble_tip_cutoff"]
    un, g = _graph(case.codes, case.tfs, 0)
    remove = np.zeros(g["U"], np.uint8)
    remove[int(np.argmin(LC.members(un)))] = 1                      # the tip alone: the bubble stays, the sink and the tail merge
    good = GR.compact(g, remove)
    GK.check(g, remove, good)
    assert good["C"] == 4 and good["E"] == 8
    merged = int(np.argmax(LC.members(good)))
    second = next(v for v, _ in good["chains"][merged][1:])

    def broken(change):
        bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in good.items()}
        change(bad)
        with pytest.raises(AssertionError):
            GK.check(g, remove, bad)

    def drop(b):
        b["unitig_contig"][second] = NONE32

    def flip(b):
        b["unitig_flag"][second] ^= 1

    def overlap(b):
        b["bases"][int(b["offsets"][merged]) + int(b["unitig_pos"][second]) + 3] ^= 0x02

    def undual(b):
        b["link_to"][0] ^= 1

    def tf_sum(b):
        b["tf_sum"][merged] += 1

    def swap(b):
        order = [1, 0] + list(range(2, b["C"]))
        un2 = {"U": b["C"], "strings": [b["strings"][i] for i in order]}
        off = [0]
        for s in un2["strings"]:
            off.append(off[-1] + len(s))
        b["offsets"] = np.array(off, np.uint64)
        b["bases"] = np.frombuffer("".join(un2["strings"]).encode(), np.uint8).copy()
        for k in ("circular", "tf_sum", "tf_min", "tf_max"):
            b[k] = b[k][order]
        ren = {old: new for new, old in enumerate(order)}
        b["unitig_contig"] = np.array([ren.get(c, c) for c in b["unitig_contig"].tolist()], np.uint32)
        lo, to = b["link_off"].tolist(), b["link_to"].tolist()
        nlo, nto = [0], []
        for c in order:
            for side in (0, 1):
                nto += [2 * ren[t >> 1] + (t & 1) for t in to[lo[2 * c + side]:lo[2 * c + side + 1]]]
                nlo.append(len(nto))
        b["link_off"], b["link_to"] = np.array(nlo, np.uint64), np.array(nto, np.uint32)

    def map_entry(b):
        b["unitig_pos"][second] += 1

    for change in (drop, flip, overlap, undual, tf_sum, swap, map_entry):
        broken(change)
