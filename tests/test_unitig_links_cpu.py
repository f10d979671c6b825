"""The unitig graph without a GPU: the three entry points are declared, exported and have ctypes signatures; the test-side restatement
(tests/unitig_links_ref.py) is pinned with literal answers; the array checker (tests/unitig_links_check.py) accepts it on every case and
rejects wrong answers; format_gfa on the restatement's arrays. test_gpu_unitig_links.py holds the kernels to this restatement."""
import numpy as np
import pytest

import graph_cases as G
import unitig_links_cases as LC
import unitig_links_check as LK
import unitig_links_ref as RL
import unitigs_cases as UC
import unitigs_ref as R

NONE32 = RL.NONE32


@pytest.fixture(scope="module")
def topo():
    return UC.topology_cases()


@pytest.fixture(scope="module")
def planted():
    return LC.link_cases()


def _both(codes, tfs, cutoff):
    un = R.unitigs(codes, tfs, cutoff)
    return un, RL.links(codes, tfs, cutoff, un)


def _self_dual(lk) -> int:
    e = np.repeat(np.arange(2 * lk["U"]), np.diff(lk["link_off"].astype(np.int64)))
    return int((lk["link_to"].astype(np.int64) == (e ^ 1)).sum())


def test_entry_points_are_declared_exported_and_typed():
    import ctypes as C
    import os
    from aindex_amd import _lib
    names = ("aix_unitig_links_dev", "aix_unitig_bubbles_dev", "aix_unitig_links")
    declared = _lib.header_symbols()
    header = open(os.path.join(_lib.ROOT, "include", "aindex_hip.h")).read()
    L = _lib.lib()
    for name in names:
        assert name in declared and name in _lib.SIGNATURES and hasattr(L, name), name
    u64, u32, vp = C.c_uint64, C.c_uint32, C.c_void_p
    assert _lib.SIGNATURES["aix_unitig_links_dev"] == (C.c_int32, [vp, u32, vp, vp, vp, u64, vp, vp, vp, u64, C.POINTER(u64), vp])
    assert _lib.SIGNATURES["aix_unitig_bubbles_dev"] == (C.c_int32, [u64, vp, vp, u64, vp, vp])
    assert _lib.SIGNATURES["aix_unitig_links"] == (C.c_int32, [vp, u32, C.POINTER(u64), C.POINTER(u64)] + [C.POINTER(vp)] * 3)
    assert "#define AIX_BUBBLE_NONE 0xFFFFFFFFu" in header and _lib.BUBBLE_NONE == NONE32
    # the refusals that need no device: NULL handle, NULL arrays
    assert L.aix_unitig_links_dev(None, 0, None, None, None, 0, None, None, None, 0, None, None) == _lib.AIX_ERR_ARG
    assert L.aix_unitig_links(None, 0, None, None, None, None, None) == _lib.AIX_ERR_ARG
    assert L.aix_unitig_bubbles_dev(1, None, None, 0, None, None) == _lib.AIX_ERR_ARG


def test_pinned_bubble_with_tip(topo):
    case = topo["bubble_tip_cutoff"]
    un, lk = _both(case.codes, case.tfs, 0)
    assert (lk["U"], lk["E"]) == (6, 12) and LC.histogram(lk) == [3, 6, 3, 0, 0]
    m = LC.members(un)
    (u, w), = LC.mate_pairs(lk)
    assert m[u] == 23 and m[w] == 23 and lk["bubble_mate"].tolist().count(NONE32) == 4
    assert lk["bubble_mate"][u] == w and lk["bubble_mate"][w] == u
    un3, lk3 = _both(case.codes, case.tfs, 3)
    assert (lk3["U"], lk3["E"]) == (1, 0) and lk3["link_off"].tolist() == [0, 0, 0] and lk3["bubble_mate"].tolist() == [NONE32]
    assert lk["link_off"].dtype == np.uint64 and lk["link_to"].dtype == np.uint32 and lk["bubble_mate"].dtype == np.uint32


def test_pinned_graph_case_and_topologies(topo):
    codes, tfs = G.make_graph_case(0)[:2]
    _, lk = _both(codes, tfs, 0)
    assert lk["E"] == 128 and LC.histogram(lk) == [1081, 65, 14, 5, 5]
    assert _both(codes, tfs, 3)[1]["E"] == 60
    none = _both(codes, tfs, 2 ** 32 - 1)[1]
    assert none["U"] == 0 and none["link_off"].tolist() == [0] and none["E"] == 0
    _, lk = _both(topo["hairpin_ends"].codes, topo["hairpin_ends"].tfs, 0)
    assert lk["E"] == 16 and _self_dual(lk) == 14
    _, lk = _both(topo["selfloop"].codes, topo["selfloop"].tfs, 0)
    assert lk["E"] == 16 and LC.histogram(lk)[2] == 8
    _, lk = _both(topo["many_circles"].codes, topo["many_circles"].tfs, 0)
    assert lk["E"] == 0


def test_hand_made_hairpin_and_homopolymer():
    """u+ -> u- at a hairpin end; u+ -> u+ and u- -> u- at a homopolymer"""
    codes = np.array([0], dtype=np.uint64)                          # A * 23: its own successor on both strands
    _, lk = _both(codes, np.ones(1, np.uint32), 0)
    assert lk["link_off"].tolist() == [0, 1, 2] and lk["link_to"].tolist() == [0, 1] and lk["bubble_mate"].tolist() == [NONE32]
    half = "GATTACAGGCT"
    x = RL.encode("C" + half + half[::-1].translate(str.maketrans("ACGT", "TGCA")))
    assert R.nxt(x, 2) == R.rc(x)
    codes = np.array([R.canon(x)], dtype=np.uint64)
    _, lk = _both(codes, np.ones(1, np.uint32), 0)
    f = 0 if R.canon(x) == x else 1                                 # the end through which x leaves
    assert lk["E"] == 1 and lk["link_to"].tolist() == [f ^ 1] and np.diff(lk["link_off"].astype(np.int64)).tolist()[f] == 1


def test_planted_cases_hold_their_structures(planted):
    for name, case in planted.items():
        ans = {c: _both(case.codes, case.tfs, c) for c in case.cutoffs}
        case.pred(ans)
        for c, (un, lk) in ans.items():
            LK.check(case.codes, case.tfs, c, un, lk)


def test_checker_accepts_the_restatement_everywhere(topo):
    for seed in (0, 3, 6, 9):
        codes, tfs = G.make_graph_case(seed)[:2]
        for c in (0, 3, 2 ** 32 - 1):
            un, lk = _both(codes, tfs, c)
            LK.check(codes, tfs, c, un, lk)
    for name, case in topo.items():
        if name == "isolated":                                      # 5000 unitigs without a link: the restatement's time, nothing to check
            continue
        for c in UC.topology_cutoffs(name):
            un, lk = _both(case.codes, case.tfs, c)
            LK.check(case.codes, case.tfs, c, un, lk)


def _drop(lk, i):
    """the answer without link i"""
    off = lk["link_off"].astype(np.int64)
    e = int(np.searchsorted(off, i, side="right")) - 1
    off = off.copy()
    off[e + 1:] -= 1
    return dict(lk, link_off=off.astype(np.uint64), link_to=np.delete(lk["link_to"], i), E=lk["E"] - 1)


def test_checker_rejects_wrong_answers(topo, planted):
    case = topo["bubble_tip_cutoff"]
    un, lk = _both(case.codes, case.tfs, 0)
    LK.check(case.codes, case.tfs, 0, un, lk)
    off, to = lk["link_off"].astype(np.int64), lk["link_to"]

    def rejected(bad, case=case, un=un):
        with pytest.raises(AssertionError):
            LK.check(case.codes, case.tfs, 0, un, bad)

    rejected(_drop(lk, 0))                                          # a dropped link
    e = int(np.nonzero(np.diff(off) == 2)[0][0])                    # a swapped pair within an end
    swapped = to.copy()
    swapped[off[e]], swapped[off[e] + 1] = to[off[e] + 1], to[off[e]]
    rejected(dict(lk, link_to=swapped))
    flipped = to.copy()                                             # a flipped r bit
    flipped[3] ^= 1
    rejected(dict(lk, link_to=flipped))
    t = int(to[off[e]])                                             # a missing dual: (t ^ 1 -> e ^ 1) is gone, (e -> t) is still there
    src = t ^ 1
    dual = next(i for i in range(off[src], off[src + 1]) if int(to[i]) == e ^ 1)
    rejected(_drop(lk, dual))
    (u, w), = LC.mate_pairs(lk)                                     # an asymmetric mate
    mate = lk["bubble_mate"].copy()
    mate[w] = NONE32
    rejected(dict(lk, bubble_mate=mate))
    mate = lk["bubble_mate"].copy()                                 # a mate on a unitig that is no arm
    other = next(i for i in range(lk["U"]) if i not in (u, w))
    mate[other] = u
    rejected(dict(lk, bubble_mate=mate))
    three = planted["near_three_arms"]                              # a mate set on a three-armed structure
    un3, lk3 = _both(three.codes, three.tfs, 0)
    LK.check(three.codes, three.tfs, 0, un3, lk3)
    arms = np.nonzero(LC.members(un3) == 23)[0]
    mate = lk3["bubble_mate"].copy()
    mate[arms[0]], mate[arms[1]] = arms[1], arms[0]
    rejected(dict(lk3, bubble_mate=mate), three, un3)


def test_mates_vectorised_equals_the_sequential_rule(planted, topo):
    sets = [(c.codes, c.tfs) for c in planted.values()] + [G.make_graph_case(seed)[:2] for seed in (0, 3)] + [(topo["selfloop"].codes, topo["selfloop"].tfs)]
    for codes, tfs in sets:
        _, lk = _both(codes, tfs, 0)
        assert np.array_equal(LK.mates(lk["U"], lk["link_off"], lk["link_to"]), lk["bubble_mate"])


def test_format_gfa_literal_lines(topo):
    from aindex_amd.aindex import format_gfa, unitig_link_pairs
    case = topo["bubble_tip_cutoff"]
    un, lk = _both(case.codes, case.tfs, 0)
    lines = list(format_gfa(un, lk))
    assert lines[0] == "H\tVN:Z:1.0" and len(lines) == 1 + 6 + 6
    for i, s in enumerate(un["strings"]):
        t = int(un["tf_sum"][i])
        assert lines[1 + i] == f"S\tu{i}\t{s}\tLN:i:{len(s)}\tKC:i:{t}\tkm:f:{t / (len(s) - 22):.1f}"
    assert lines[7:] == GFA_LINKS
    assert unitig_link_pairs(lk) == [tuple(int(f[1:]) if f[0] == "u" else f for f in ln.split("\t")[1:5]) for ln in GFA_LINKS]
    # each L line joins two oriented segments that overlap by 22 bases
    rc = lambda s: s[::-1].translate(str.maketrans("ACGT", "TGCA"))
    for ln in lines[7:]:
        _, a, sa, b, sb, ov = ln.split("\t")
        sa_, sb_ = un["strings"][int(a[1:])], un["strings"][int(b[1:])]
        assert ov == "22M" and (sa_ if sa == "+" else rc(sa_))[-22:] == (sb_ if sb == "+" else rc(sb_))[:22]
    # a self-dual link once, both links of a homopolymer, the closing link of a circle
    codes = np.array([0], dtype=np.uint64)
    un1, lk1 = _both(codes, np.ones(1, np.uint32), 0)
    assert list(format_gfa(un1, lk1))[2:] == ["L\tu0\t+\tu0\t+\t22M"]  # u- -> u- is the dual of u+ -> u+
    hp = topo["hairpin_ends"]
    unh, lkh = _both(hp.codes, hp.tfs, 0)
    assert sum(ln[0] == "L" for ln in format_gfa(unh, lkh)) == 14 + (16 - 14) // 2
    ring = topo["opened_circle"]
    unr, lkr = _both(ring.codes, ring.tfs, 0)
    got = list(format_gfa(unr, lkr))
    assert got[-2:] == ["L\tu0\t+\tu0\t+\t22M", "L\tu1\t+\tu1\t+\t22M"] and len(got) == 5
    assert all("\n" not in ln and " " not in ln for ln in got + lines)


# u0 and u1 are the arms (spelled from the right flank to the left one), u2 the 20 k-mers between the bubble and the tip, u3 the left flank,
# u4 the tip (entered at its last k-mer), u5 what follows the tip's branch
GFA_LINKS = ["L\tu0\t+\tu3\t+\t22M", "L\tu0\t-\tu2\t+\t22M", "L\tu1\t+\tu3\t+\t22M", "L\tu1\t-\tu2\t+\t22M", "L\tu2\t+\tu4\t-\t22M", "L\tu2\t+\tu5\t+\t22M"]
