"""Pins the test-side restatement of the threading (tests/seqthread_ref.py) and the batches of tests/seqthread_cases.py, without a GPU:
literals, the properties of the contract, the composed k-mer map held against the contig bases, what the batches reach, and the
refusals of the two handle-less entry points that are decided before any device call."""
import ctypes as C

import numpy as np
import pytest

import graph_cases as G
import graph_clean_ref as GR
import seqthread_cases as SC
import seqthread_ref as SR
import unitig_links_ref as RL
import unitigs_cases as UC
import unitigs_ref as R
from aindex_amd import _lib

NO, BROKEN = SR.NO_LINK, SR.BROKEN


def _graph(codes, tfs, cutoff):
    """(un, lk, g, kid_of, node) of the restated unitig graph; kids in the order of `codes`"""
    un = R.unitigs(codes, tfs, cutoff)
    lk = RL.links(codes, tfs, cutoff, un)
    node = SR.nodes(un["kid_unitig"], un["kid_pos"], un["kid_flag"], un["offsets"])
    return un, lk, GR.graph(un, lk), {int(c): i for i, c in enumerate(np.asarray(codes).tolist())}, node


@pytest.fixture(scope="module")
def case0():
    codes, tfs, _ = G.make_graph_case(0)
    un, lk, g, kid_of, node = _graph(codes, tfs, 0)
    b = SC.batch(un, lk, 0)
    out = SR.thread(kid_of, node, g, b.seqs, support=np.zeros(g["E"], np.uint64))
    return dict(codes=codes, tfs=tfs, un=un, lk=lk, g=g, kid_of=kid_of, node=node, batch=b, out=out)


def _steps(out, i):
    a, z = int(out["seq_step_off"][i]), int(out["seq_step_off"][i + 1])
    return [tuple(int(out[k][j]) for k in SR.KEYS[1:]) for j in range(a, z)]


def test_literals_of_a_hand_made_fork():
    """A stem of two k-mers whose last k-mer has two successors, one stored as given (unitig 2) and one stored reverse-complemented
    (unitig 1): every array, written out."""
    stem = "ACGGTCATTGCAGATCCGTAAGCT"
    keys = sorted({R.canon(RL.encode(s)) for s in (stem[:23], stem[1:24], stem[2:] + "A", stem[2:] + "G")})
    assert keys == [7374343723785, 10933434387990, 20325544641413, 47620755402908]
    un, lk, g, kid_of, node = _graph(np.array(keys, np.uint64), np.full(4, 5, np.uint32), 0)
    assert un["strings"] == ["ACGGTCATTGCAGATCCGTAAGCT", "CAGCTTACGGATCTGCAATGACC", "GGTCATTGCAGATCCGTAAGCTA"]
    assert lk["link_off"].tolist() == [0, 2, 2, 3, 3, 3, 4] and lk["link_to"].tolist() == [4, 3, 1, 1]
    assert node.dtype == np.uint64 and node.tolist() == [0x0, 0x5, 0x200000000, 0x400000000]
    seqs = [(stem + "A").encode(), SC.rc(stem + "G").encode(), stem[:23].encode(), (stem[:10] + "N" + stem[11:] + "A").encode(), b"ACGT",
            (stem + "AC").encode()]
    out = SR.thread(kid_of, node, g, seqs, support=np.zeros(4, np.uint64))
    want = {"seq_step_off": [0, 2, 4, 5, 5, 5, 7], "step_unitig": [0, 2, 1, 0, 0, 0, 2], "step_pos": [0, 0, 0, 1, 0, 0, 0],
            "step_flag": [0, 0, 0, 1, 0, 0, 0], "q_first": [0, 2, 0, 1, 0, 0, 2], "q_last": [1, 2, 0, 2, 0, 1, 2],
            "step_link": [NO, 0, NO, 2, NO, NO, 0], "support": [2, 1, 1, 2]}
    for k, dt in zip(SR.KEYS + ("support",), SR.DTYPES + (np.uint64,)):
        assert out[k].dtype == dt and out[k].tolist() == want[k], k
    assert SR.thread(kid_of, node, g, seqs)["support"] is None
    # a dead node is no node: the arm stored reverse-complemented disappears from the second sequence
    dead = node.copy()
    dead[int(np.nonzero(un["kid_unitig"] == 1)[0][0])] = SR.DEAD
    assert _steps(SR.thread(kid_of, dead, g, seqs), 1) == [(0, 1, 1, 1, 2, NO)]


def test_a_walk_threads_to_its_own_path(case0):
    out, b = case0["out"], case0["batch"]
    assert len(b.walks) > 150
    for w in b.walks:
        steps = _steps(out, w.index)
        assert [(s[0], s[2] & 1) for s in steps] == w.visits, w
        if w.links is not None:
            assert [s[5] for s in steps] == [NO] + w.links, w
        assert all(a[4] + 1 == b_[3] for a, b_ in zip(steps, steps[1:]))


def test_reverse_complement_gives_the_reversed_path(case0):
    g, b = case0["g"], case0["batch"]
    dual = SR.dual_of(g)
    assert None not in dual
    rcs = [SC.rc(s.decode()).encode() if set(s) <= set(b"ACGT") else s for s in b.seqs]
    back = SR.thread(case0["kid_of"], case0["node"], g, rcs, support=np.zeros(g["E"], np.uint64))
    out = case0["out"]
    for i, s in enumerate(b.seqs):
        if not set(s) <= set(b"ACGT"):
            continue
        fw, bw = _steps(out, i), _steps(back, i)
        nw = len(s) - 22
        assert [(u, f ^ 1, nw - 1 - ql, nw - 1 - qf) for u, _, f, qf, ql, _ in reversed(fw)] == [(u, f, qf, ql) for u, _, f, qf, ql, _ in bw], i
        # the link into step j of the reversed path is the dual of the link out of it in the forward path
        assert ([NO] if fw else []) + [dual[l] if l < BROKEN else l for l in [s_[5] for s_ in reversed(fw)][:-1]] == [s_[5] for s_ in bw], i
    assert np.array_equal(out["support"], back["support"])
    sup = out["support"].tolist()
    assert all(sup[j] == sup[dual[j]] for j in range(g["E"])) and sum(sup) > 0


def test_an_n_gives_a_gap_of_23_windows(case0):
    un = case0["un"]
    u = int(np.argmax(np.diff(un["offsets"].astype(np.int64)) * (1 - un["circular"].astype(np.int64))))
    text = un["strings"][u]
    assert len(text) >= 56                                             # room for a mutation with 23 clean bases on either side
    clean = _steps(SR.thread(case0["kid_of"], case0["node"], case0["g"], [text.encode()]), 0)
    assert clean == [(u, 0, 0, 0, len(text) - 23, NO)]
    for i in (23, 30, len(text) - 24):
        got = _steps(SR.thread(case0["kid_of"], case0["node"], case0["g"], [(text[:i] + "N" + text[i + 1:]).encode()]), 0)
        assert got == [(u, 0, 0, 0, i - 23, NO), (u, i + 1, 0, i + 1, len(text) - 23, NO)], i
    for i, how in ((30, "a"), (31, "c")):                             # lower case is no base
        got = _steps(SR.thread(case0["kid_of"], case0["node"], case0["g"], [(text[:i] + how + text[i + 1:]).encode()]), 0)
        assert [(s[3], s[4]) for s in got] == [(0, i - 23), (i + 1, len(text) - 23)]


def test_broken_only_on_a_foreign_graph(case0):
    out = case0["out"]
    assert not (out["step_link"] == BROKEN).any()
    # the links of another cutoff belong to other unitig ids
    lk3 = RL.links(case0["codes"], case0["tfs"], 3)
    foreign = dict(case0["g"], link_off=lk3["link_off"], link_to=lk3["link_to"])
    got = SR.thread(case0["kid_of"], case0["node"], foreign, case0["batch"].seqs)
    assert (got["step_link"] == BROKEN).any()
    for k in SR.KEYS[:-1]:                                             # only the links differ
        assert np.array_equal(got[k], out[k]), k
    assert np.array_equal(got["step_link"] == NO, out["step_link"] == NO)


@pytest.mark.parametrize("seed", (0, 3))
@pytest.mark.parametrize("cutoff", (0, 3))
def test_composed_map_against_the_contig_bases(seed, cutoff):
    """For every live kid after 1, 2 and 3 cleaning rounds the 23 bases at its place in its contig decode to the stored code (flag bit 0
    clear) or to its reverse complement (set); the dead kids are exactly the k-mers of removed unitigs."""
    codes, tfs, _ = G.make_graph_case(seed)
    un, lk, g, kid_of, node = _graph(codes, tfs, cutoff)
    km = (un["kid_unitig"], un["kid_pos"], un["kid_flag"])
    gone = km[0] == SR.NONE64
    removed_any = 0
    for rnd in (1, 2, 3):
        remove = GR.mark(g, 46, 46)
        nxt = GR.compact(g, remove)
        live = km[0] != SR.NONE64
        gone = gone | (live & (remove[np.where(live, km[0], 0).astype(np.int64)] != 0))
        removed_any += int(remove.any())
        km = SR.kidmap(*km, g["offsets"], nxt["unitig_contig"], nxt["unitig_pos"], nxt["unitig_flag"])
        g = nxt
        assert np.array_equal(km[0] == SR.NONE64, gone), rnd
        text, off = g["bases"].tobytes(), g["offsets"].tolist()
        for kid in np.nonzero(~gone)[0].tolist():
            c, p, f = int(km[0][kid]), int(km[1][kid]), int(km[2][kid])
            assert p < off[c + 1] - off[c] - 22
            w = text[off[c] + p:off[c] + p + 23]
            want = int(codes[kid])
            assert GR.code23(w) == (R.rc(want) if f & 1 else want), (rnd, kid)
            assert bool(f & 2) == bool(g["circular"][c])
        # the node words of the composed map thread a contig to one step
        nd = SR.nodes(*km, g["offsets"])
        c = int(np.argmax(np.diff(g["offsets"].astype(np.int64))))
        got = _steps(SR.thread(kid_of, nd, g, [text[off[c]:off[c + 1]]]), 0)
        assert got == [(c, 0, 2 if g["circular"][c] else 0, 0, off[c + 1] - off[c] - 23, NO)]
    assert removed_any >= 1 and gone.sum() > (un["kid_unitig"] == SR.NONE64).sum()


def test_kidmap_and_nodes_refuse_what_the_contract_refuses():
    off = np.array([0, 25], np.uint64)
    one = lambda v, dt: np.array([v], dt)
    ok = (one(0, np.uint64), one(1, np.uint32), one(0, np.uint8))
    assert SR.nodes(*ok, off).tolist() == [1 << 2]
    for bad in ((one(1, np.uint64), ok[1], ok[2]), (ok[0], one(3, np.uint32), ok[2])):
        with pytest.raises(ValueError):
            SR.nodes(*bad, off)
        with pytest.raises(ValueError):
            SR.kidmap(*bad, off, one(0, np.uint32), one(0, np.uint64), one(0, np.uint8))
    with pytest.raises(ValueError):
        SR.kidmap(*ok, off, one((1 << 31) - 4, np.uint32), one(0, np.uint64), one(0, np.uint8))
    with pytest.raises(ValueError):
        SR.kidmap(*ok, off, one(0, np.uint32), one(0xFFFFFFFF, np.uint64), one(0, np.uint8))
    got = SR.kidmap(*ok, off, one(7, np.uint32), one(10, np.uint64), one(3, np.uint8))          # reversed member of a merged cycle: 3 k-mers, p = 1
    assert [a.tolist() for a in got] == [[7], [11], [3]]
    got = SR.kidmap(*ok, off, one(SR.NONE32, np.uint32), one(0, np.uint64), one(0, np.uint8))
    assert [a.tolist() for a in got] == [[SR.NONE64], [0], [0]]


def test_what_the_batches_reach(case0):
    """No GPU comparison on these batches passes vacuously."""
    g, out, b = case0["g"], case0["out"], case0["batch"]
    m = np.diff(g["offsets"].astype(np.int64)) - 22
    assert np.bincount(out["step_flag"] & 1).min() > 50                                      # both strands
    per_seq = np.diff(out["seq_step_off"].astype(np.int64))
    gaps = sum(1 for i in range(len(b.seqs)) for s in _steps(out, i)[1:] if s[5] == NO)
    assert gaps >= 3                                                                          # steps parted by windows without a node
    wound = (out["q_last"].astype(np.int64) - out["q_first"] + 1) > m[out["step_unitig"]]
    assert wound.any() and (out["step_flag"][wound] & 2).all()                               # a circular wrap
    lo, to = g["link_off"].tolist(), g["link_to"].tolist()
    src = np.repeat(np.arange(2 * g["U"]), np.diff(g["link_off"].astype(np.int64)))
    selfl = [j for j in range(g["E"]) if to[j] == src[j] and m[src[j] >> 1] == 1]
    followed = set(out["step_link"][out["step_link"] < BROKEN].tolist())
    assert selfl and set(selfl) & followed                                                    # the self-link of a one-k-mer unitig
    assert len(followed) * 2 >= g["E"] and g["E"] > 100                                      # links followed cover at least half of E
    assert per_seq.max() >= 4 and (per_seq == 0).sum() >= 5
    # graph case 0 has no hairpin: the planted case provides the link that is its own dual, and it is counted once
    case = UC.topology_cases()["hairpin_ends"]
    un, lk, gh, kid_of, node = _graph(case.codes, case.tfs, 0)
    bh = SC.batch(un, lk, 1)
    oh = SR.thread(kid_of, node, gh, bh.seqs, support=np.zeros(gh["E"], np.uint64))
    srch = np.repeat(np.arange(2 * gh["U"]), np.diff(gh["link_off"].astype(np.int64)))
    hair = [j for j in range(gh["E"]) if int(gh["link_to"][j]) == int(srch[j]) ^ 1]
    assert hair and SR.dual_of(gh)[hair[0]] == hair[0]
    for j in hair:
        assert int(oh["support"][j]) == int((oh["step_link"] == j).sum()) > 0


def test_null_pointers_are_refused_before_any_device_call():
    """Runs without a GPU: the two handle-less entry points decide a NULL pointer before anything is allocated or launched."""
    L = _lib.lib()
    a = np.zeros(4, np.uint64)
    p = a.ctypes.data_as(C.c_void_p)
    assert L.aix_graph_kidmap_dev(1, None, p, p, 1, p, p, p, p, p, p, p, None) == _lib.AIX_ERR_ARG
    assert L.aix_graph_kidmap_dev(1, p, p, p, 1, None, p, p, p, p, p, p, None) == _lib.AIX_ERR_ARG
    assert L.aix_graph_kidmap_dev(1, p, p, p, 1, p, p, None, p, p, p, p, None) == _lib.AIX_ERR_ARG
    assert L.aix_graph_kidmap_dev(1, p, p, p, 1, p, p, p, p, p, p, None, None) == _lib.AIX_ERR_ARG
    assert L.aix_thread_nodes_dev(1, p, p, None, 1, p, p, None) == _lib.AIX_ERR_ARG
    assert L.aix_thread_nodes_dev(1, p, p, p, 1, p, None, None) == _lib.AIX_ERR_ARG
    assert L.aix_thread_nodes_dev(1, p, p, p, 1, None, p, None) == _lib.AIX_ERR_ARG
    assert L.aix_thread_nodes_dev(1, p, p, p, (1 << 31) - 3, p, p, None) == _lib.AIX_ERR_UNSUPPORTED
    assert _lib.THREAD_NO_LINK == NO and _lib.THREAD_BROKEN == BROKEN
