"""Threading on the GPU (k_st_* of aix_seqthread.hip) against the test-side restatement (tests/seqthread_ref.py, pinned by
test_seqthread_cpu.py) on the batches of tests/seqthread_cases.py. Every comparison is exact equality."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import debruijn_ref as D
import graph_cases as G
import graph_clean_ref as GR
import oracle_lib as O
import seqthread_cases as SC
import seqthread_ref as SR
import unitig_links_cases as LC
import unitig_links_ref as RL
import unitigs_cases as UC
import unitigs_ref as R
from aindex_amd import _lib, builder
from aindex_amd.engine import Index

vp = _lib.vp
SEEDS = (0, 3, 6, 9)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO, BROKEN = SR.NO_LINK, SR.BROKEN
P64, P32, P8 = 0x6B6B6B6B6B6B6B6B, 0x6B6B6B6B, 0x6B
GRAPH_KEYS = GR.GRAPH_KEYS
_UNSIGNED = {np.dtype(np.int64): np.uint64, np.dtype(np.int32): np.uint32}


def _open(prefix):
    return Index.open_23(prefix + ".pf", prefix + ".tf.bin", prefix + ".kmers.bin")


def _np(t):
    a = t.cpu().numpy()
    return a.view(_UNSIGNED.get(a.dtype, a.dtype))


def _ref(ix, cutoff):
    """(un, lk, g, kid_of, node) of the restated unitig graph, kids in the order of the handle"""
    codes, tfs = ix.checker_array() & np.uint64(R.MASK), ix.tf_array()
    un = R.unitigs(codes, tfs, cutoff)
    lk = RL.links(codes, tfs, cutoff, un)
    node = SR.nodes(un["kid_unitig"], un["kid_pos"], un["kid_flag"], un["offsets"])
    return un, lk, GR.graph(un, lk), {int(c): i for i, c in enumerate(codes.tolist())}, node


def _dev_seqs(seqs):
    import torch
    data = np.frombuffer(b"".join(seqs), dtype=np.uint8)
    offs = np.zeros(len(seqs) + 1, np.int64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    return torch.from_numpy(data.copy()).cuda(), torch.from_numpy(offs).cuda()


def _same(got, want, tag):
    """got: the tuple of seq_thread_t (or the dict of seq_thread); want: the dict of SR.thread"""
    if not isinstance(got, dict):
        got = {k: _np(t) for k, t in zip(SR.KEYS, got)}
    for k, dt in zip(SR.KEYS, SR.DTYPES):
        assert got[k].dtype == dt and np.array_equal(got[k], want[k]), (tag, k)


def _zeros(n):
    import torch
    return torch.zeros(n, dtype=torch.int64, device="cuda")


def _write_index(prefix, codes, tfs):
    open(prefix + ".pf", "wb").write(builder.build_pf_codes(codes, 23))
    rc, checker, tf = O.index_scatter(O.OracleMphf(prefix + ".pf"), np.ascontiguousarray(D.decode(codes)).reshape(-1), tfs)
    assert rc == 0
    checker.tofile(prefix + ".kmers.bin")
    tf.tofile(prefix + ".tf.bin")
    return prefix


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("st"))
    return {seed: G.write_graph_case(seed, d)[0] for seed in SEEDS + (1,)}


_EVERY = dict(UC.topology_cases())
_EVERY.update(LC.link_cases())
NAMES = sorted(nm for nm, c in _EVERY.items() if c.codes.shape[0] + 22 <= 40_000 and nm != "isolated")   # at most 40 000 bases


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("stp"))
    made = {}

    def get(name):
        if name not in made:
            made[name] = _write_index(os.path.join(d, name), _EVERY[name].codes, _EVERY[name].tfs)
        return made[name]
    return get


def _every_form(ix, cutoff, seed, tag):
    """device form with and without support, host form, two calls accumulated, against the restatement; -> (graph, ref tuple, batch, want)"""
    un, lk, g, kid_of, node = _ref(ix, cutoff)
    graph = ix.thread_graph_t(cutoff)
    assert (graph["U"], graph["E"], graph["rounds"]) == (g["U"], g["E"], 0), tag
    assert np.array_equal(_np(graph["node"]), node), tag
    b = SC.batch(un, lk, seed)
    want = SR.thread(kid_of, node, g, b.seqs, support=np.zeros(g["E"], np.uint64))
    st, so = _dev_seqs(b.seqs)
    sup = _zeros(g["E"])
    _same(ix.seq_thread_t(graph, st, so, link_support=sup), want, (tag, "device"))
    assert np.array_equal(_np(sup), want["support"]), tag
    _same(ix.seq_thread_t(graph, st, so, cap_hint=len(want["step_link"])), want, (tag, "device, no support"))
    host = ix.seq_thread(b.seqs, cutoff)
    _same(host, want, (tag, "host"))
    assert np.array_equal(host["link_support"], want["support"]) and (host["U"], host["E"]) == (g["U"], g["E"]), tag
    half = len(b.seqs) // 2                                            # batch after batch into one array
    sup2 = _zeros(g["E"])
    for part in (b.seqs[:half], b.seqs[half:]):
        ix.seq_thread_t(graph, *_dev_seqs(part), link_support=sup2)
    assert np.array_equal(_np(sup2), want["support"]), tag
    return graph, (un, lk, g, kid_of, node), b, want


def _raw(ix, graph, st, so, cap, sup=None, total=None, stream=None, **over):
    """aix_seq_thread_dev itself: 64 poisoned elements behind every output, the outputs dirty before the call. over: arguments replaced."""
    import torch
    L = _lib.lib()
    m = so.numel() - 1
    n_out = total if total is not None else cap
    types = (torch.int64, torch.int32, torch.int32, torch.uint8, torch.int32, torch.int32, torch.int64)
    poison = {torch.int64: P64, torch.int32: P32, torch.uint8: P8}
    outs = [torch.full(((m + 1 if i == 0 else n_out) + 64,), poison[ty], dtype=ty, device="cuda") for i, ty in enumerate(types)]
    q = lambda t: vp(t.data_ptr()) if t is not None else None
    a = dict(h=ix._h if ix is not None else None, seqs=q(st), offs=q(so), M=m, node=q(graph["node"]), U=graph["offsets"].numel() - 1, offsets=q(graph["offsets"]),
             circular=q(graph["circular"]), link_off=q(graph["link_off"]), link_to=q(graph["link_to"]), E=graph["link_to"].numel(), sup=q(sup),
             outs=[q(t) for t in outs], cap=cap)
    for k, v in over.items():
        if k.startswith("out"):
            a["outs"][int(k[3:])] = v
        else:
            a[k] = q(v) if hasattr(v, "data_ptr") else v
    tot = C.c_uint64(77)
    status = L.aix_seq_thread_dev(a["h"], a["seqs"], a["offs"], a["M"], a["node"], a["U"], a["offsets"], a["circular"], a["link_off"], a["link_to"], a["E"], a["sup"],
                                  *a["outs"], a["cap"], C.byref(tot), stream)
    torch.cuda.synchronize()
    clean = lambda t, n=0: bool((t[n:] == poison[t.dtype]).all())
    return status, tot.value, outs, clean


@pytest.mark.parametrize("seed", SEEDS)
def test_graph_cases_every_form(cases, seed):
    """1. Graph cases at cutoffs 0 and 3: seq_thread_t and seq_thread on the walk batch, with and without link_support; support over two
    calls; the cap protocol."""
    import torch
    with _open(cases[seed]) as ix:
        for cutoff in (0, 3):
            graph, ref, b, want = _every_form(ix, cutoff, seed, (seed, cutoff))
            for w in b.walks:                                      # the batch is what it says it is
                a, z = int(want["seq_step_off"][w.index]), int(want["seq_step_off"][w.index + 1])
                assert list(zip(want["step_unitig"][a:z].tolist(), (want["step_flag"][a:z] & 1).tolist())) == w.visits
            assert not (want["step_link"] == BROKEN).any() and int(want["support"].sum()) > 0
            # cap 0, total - 1 and total: the same offsets and total; entries and support only in the call that fits, exactly once
            total = len(want["step_link"])
            st, so = _dev_seqs(b.seqs)
            sup = torch.arange(ref[2]["E"], dtype=torch.int64, device="cuda") * 3 + 1
            pattern = _np(sup).copy()
            for cap in (0, total - 1):
                status, tot, outs, clean = _raw(ix, graph, st, so, cap, sup=sup)
                assert status == 0 and tot == total and np.array_equal(_np(outs[0][:len(b.seqs) + 1]), want["seq_step_off"]), cap
                assert clean(outs[0], len(b.seqs) + 1) and all(clean(t) for t in outs[1:]) and np.array_equal(_np(sup), pattern), cap
            status, tot, outs, clean = _raw(ix, graph, st, so, total, sup=sup)
            assert status == 0 and tot == total
            _same({k: _np(t[:len(b.seqs) + 1 if i == 0 else total]) for i, (k, t) in enumerate(zip(SR.KEYS, outs))}, want, (seed, cutoff, "cap == total"))
            assert clean(outs[0], len(b.seqs) + 1) and all(clean(t, total) for t in outs[1:])
            assert np.array_equal(_np(sup), pattern + want["support"])      # the pattern plus the counts


@pytest.mark.parametrize("seed", (0, 3))
def test_contigs(cases, seed):
    """2. thread_graph_t(rounds = 1, 3): the composed k-mer map and the node words equal the restatement's, threads through the contig
    graph equal the restatement's, nothing is BROKEN, and a walk spelled from a contig threads to one step."""
    with _open(cases[seed]) as ix:
        un, lk, g0, kid_of, _ = _ref(ix, 0)
        b = SC.batch(un, lk, seed)
        st, so = _dev_seqs(b.seqs)
        for rounds in (1, 3):
            g, km, done = g0, (un["kid_unitig"], un["kid_pos"], un["kid_flag"]), 0
            while done < rounds:
                remove = GR.mark(g, 46, 46)
                if not remove.any():
                    break
                nxt = GR.compact(g, remove)
                km = SR.kidmap(*km, g["offsets"], nxt["unitig_contig"], nxt["unitig_pos"], nxt["unitig_flag"])
                g = nxt
                done += 1
            graph = ix.thread_graph_t(0, 46, 46, rounds)
            assert graph["rounds"] == done >= 1 and graph["U"] == g["C"] and graph["E"] == g["E"]
            for k, a in zip(("kid_unitig", "kid_pos", "kid_flag"), km):
                assert np.array_equal(_np(graph[k]), a), (rounds, k)
            for k in GRAPH_KEYS:
                assert np.array_equal(_np(graph[k]), g[k]), (rounds, k)
            node = SR.nodes(*km, g["offsets"])
            assert np.array_equal(_np(graph["node"]), node)
            want = SR.thread(kid_of, node, g, b.seqs, support=np.zeros(g["E"], np.uint64))
            sup = _zeros(g["E"])
            _same(ix.seq_thread_t(graph, st, so, link_support=sup), want, (seed, rounds))
            assert np.array_equal(_np(sup), want["support"]) and not (want["step_link"] == BROKEN).any()
            assert len(want["step_link"]) < len(SR.thread(kid_of, _ref(ix, 0)[4], g0, b.seqs)["step_link"])      # merged unitigs: fewer steps
            text, off = g["bases"].tobytes(), g["offsets"].tolist()
            contigs = [text[off[c]:off[c + 1]] for c in np.argsort(-np.diff(g["offsets"].astype(np.int64)))[:8].tolist()]
            got = ix.seq_thread_t(graph, *_dev_seqs(contigs))
            _same(got, SR.thread(kid_of, node, g, contigs), (seed, rounds, "contigs"))
            assert _np(got[0]).tolist() == list(range(len(contigs) + 1))
            assert np.array_equal(_np(got[5]).astype(np.int64), np.array([len(c) - 23 for c in contigs]))


@pytest.mark.parametrize("name", NAMES)
def test_planted_cases(planted, name):
    """3. Every planted topology and link case of at most 40 000 bases."""
    with _open(planted(name)) as ix:
        graph, ref, b, want = _every_form(ix, 0, 7, name)
        if name in ("hairpin_ends", "near_hairpin_arm"):                  # the link that is its own dual is counted once
            g = ref[2]
            src = np.repeat(np.arange(2 * g["U"]), np.diff(g["link_off"].astype(np.int64)))
            hair = np.nonzero(g["link_to"] == (src ^ 1))[0]
            assert hair.shape[0] and all(int(want["support"][j]) == int((want["step_link"] == j).sum()) > 0 for j in hair.tolist())
        if name == "many_circles":                                   # one step of 5000 windows
            assert (want["q_last"].astype(np.int64) - want["q_first"] + 1).max() == UC.LONG_PATH


@pytest.fixture(scope="module")
def depth():
    """the paths and circles of unitigs_cases.depth_case as an index built on the device, its restated graph and a batch: every unitig
    spelled whole in both orientations (one step each, the path of 20 001 k-mers among them), the circles 2.5 times round, walks of
    exactly 64 / 65 / 256 / 257 windows"""
    import torch
    codes, tfs, paths, circles = UC.depth_case()
    keys = torch.from_numpy(codes.astype(np.int64)).cuda()
    ix = Index.build_23_codes_t(builder.build_pf_codes_t(keys, 23), keys, torch.from_numpy(tfs.astype(np.int32)).cuda())
    torch.cuda.synchronize()
    un, lk, g, kid_of, node = _ref(ix, 0)
    b = SC.batch(un, lk, 11)
    seqs = list(b.seqs)
    for s in un["strings"]:
        seqs += [s.encode(), SC.rc(s).encode()]
    for u in np.nonzero(un["circular"])[0].tolist():                 # every circle, not only the first six of the batch
        s = un["strings"][u]
        m = len(s) - 22
        seqs.append((s[:m] * 4)[:(5 * m + 1) // 2 + 22].encode() if m >= 22 else (s[:m] * (60 // m + 4))[:(5 * m + 1) // 2 + 22].encode())
    want = SR.thread(kid_of, node, g, seqs, support=np.zeros(g["E"], np.uint64))
    yield ix, (un, lk, g, kid_of, node), seqs, want
    ix.close()


def test_depth_case_long_steps_and_circles(depth):
    """3b. Runs that cross wave, workgroup and trip boundaries: one step of 20 001 windows, circles of 2 .. 4097 k-mers wound 2.5 times,
    walks of exactly 64, 65, 256 and 257 windows."""
    ix, (un, lk, g, kid_of, node), seqs, want = depth
    windows = [len(s) - 22 for s in seqs]
    assert all(n in windows for n in SC.EXACT_WINDOWS) and max(UC.PATHS) in windows
    span = want["q_last"].astype(np.int64) - want["q_first"] + 1
    assert span.max() == max(UC.PATHS) and (want["step_flag"] & 2).any()
    graph = ix.thread_graph_t(0)
    sup = _zeros(g["E"])
    _same(ix.seq_thread_t(graph, *_dev_seqs(seqs), link_support=sup), want, "depth")
    assert np.array_equal(_np(sup), want["support"])
    _same(ix.seq_thread(seqs, 0), want, "depth, host")


_CHILD = """
import hashlib, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from aindex_amd.engine import Index
h = hashlib.sha256()
for p in sys.argv[2:]:
    seqs = [l.rstrip(b"\\n") for l in open(p + ".seqs", "rb")]
    with Index.open_23(p + ".pf", p + ".tf.bin", p + ".kmers.bin") as ix:
        for cutoff in (0, 3):
            out = ix.seq_thread(seqs, cutoff)
            for k in %r:
                h.update(np.ascontiguousarray(out[k]).tobytes())
print("digest", h.hexdigest())
""" % (SR.KEYS + ("link_support",),)


def test_many_trips_of_every_loop(cases, planted, depth, monkeypatch):
    """4. AIX_UG_TEST_GRID = 1, 2, 3 workgroups for every launch: in this process (the switch is read per call) for the device forms, in
    fresh child processes for the host form; the same bytes as the restatement."""
    import torch
    prefixes = [cases[3], planted("many_circles"), planted("lollipop")]
    h = hashlib.sha256()
    opened, sets = [], []
    try:
        for prefix in prefixes:
            ix = _open(prefix)
            opened.append(ix)
            for cutoff in (0, 3):
                un, lk, g, kid_of, node = _ref(ix, cutoff)
                if cutoff == 0:
                    seqs = SC.batch(un, lk, 5).seqs
                    assert not any(b"\n" in s for s in seqs)
                    open(prefix + ".seqs", "wb").write(b"".join(s + b"\n" for s in seqs))
                want = SR.thread(kid_of, node, g, seqs, support=np.zeros(g["E"], np.uint64))
                sets.append((ix, cutoff, seqs, want))
                for k in SR.KEYS + ("support",):
                    h.update(np.ascontiguousarray(want[k]).tobytes())
        dix, _, dseqs, dwant = depth
        sets.append((dix, 0, dseqs, dwant))
        for grid in ("1", "2", "3"):
            monkeypatch.setenv("AIX_UG_TEST_GRID", grid)
            for ix, cutoff, seqs, want in sets:
                if ix is dix and grid != "1":
                    continue
                graph = ix.thread_graph_t(cutoff)
                sup = _zeros(graph["E"])
                _same(ix.seq_thread_t(graph, *_dev_seqs(seqs), link_support=sup), want, (grid, cutoff))
                assert np.array_equal(_np(sup), want["support"]), (grid, cutoff)
            ix, cutoff, seqs, want = sets[0]                         # the composed map and the contig threads, many trips
            graph = ix.thread_graph_t(cutoff, 46, 46, 3)
            got = ix.seq_thread_t(graph, *_dev_seqs(seqs))
            monkeypatch.delenv("AIX_UG_TEST_GRID")
            graph1 = ix.thread_graph_t(cutoff, 46, 46, 3)
            assert all(torch.equal(graph[k], graph1[k]) for k in GRAPH_KEYS + ("node", "kid_unitig", "kid_pos", "kid_flag"))
            assert all(torch.equal(a, b) for a, b in zip(got, ix.seq_thread_t(graph1, *_dev_seqs(seqs))))
    finally:
        for ix in opened:
            ix.close()
    torch.cuda.synchronize()
    kids = []
    for grid in ("1", "2", "3"):
        env = dict(os.environ, AIX_UG_TEST_GRID=grid, AIX_NO_TORCH="1")
        kids.append(subprocess.Popen([sys.executable, "-c", _CHILD, ROOT] + prefixes, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE))
    for grid, k in zip("123", kids):
        out, err = k.communicate(timeout=300)
        assert k.returncode == 0, (grid, err.decode()[-2000:])
        assert out.decode().split()[-2:] == ["digest", h.hexdigest()], grid


def test_side_stream(cases):
    """5. The graph built and the sequences threaded on a side stream."""
    import torch
    with _open(cases[6]) as ix:
        un, lk, g, kid_of, node = _ref(ix, 0)
        b = SC.batch(un, lk, 6)
        want = SR.thread(kid_of, node, g, b.seqs, support=np.zeros(g["E"], np.uint64))
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            st, so = _dev_seqs(b.seqs)
            graph = ix.thread_graph_t(0)
            sup = _zeros(g["E"])
            got = ix.seq_thread_t(graph, st, so, link_support=sup)
            status, tot, outs, clean = _raw(ix, graph, st, so, len(want["step_link"]), stream=vp(side.cuda_stream))
        side.synchronize()
        _same(got, want, "side stream")
        assert np.array_equal(_np(sup), want["support"])
        assert status == 0 and np.array_equal(_np(outs[6][:tot]), want["step_link"])
    torch.cuda.synchronize()


def test_refusals_corrupt_arrays_and_poison(cases, planted):
    """6. Every refusal leaves every output and link_support untouched; corrupt arrays return, and the poison behind the outputs is intact."""
    import torch
    from pf13 import pf13_path
    L = _lib.lib()
    ARG, UNS, MODE = _lib.AIX_ERR_ARG, _lib.AIX_ERR_UNSUPPORTED, _lib.AIX_ERR_MODE
    with _open(cases[0]) as ix:
        un, lk, g, kid_of, node = _ref(ix, 0)
        graph = ix.thread_graph_t(0)
        b = SC.batch(un, lk, 0)
        st, so = _dev_seqs(b.seqs)
        want = SR.thread(kid_of, node, g, b.seqs, support=np.zeros(g["E"], np.uint64))
        total, U, E, M = len(want["step_link"]), g["U"], g["E"], len(b.seqs)
        pattern = torch.arange(E, dtype=torch.int64, device="cuda") + 5

        def refused(status, ix_=ix, graph_=graph, so_=so, **over):
            sup = pattern.clone()
            r = _raw(ix_, graph_, st, so_, total, sup=sup, **over)
            assert r[0] == status and r[1] == 77 and all(r[3](t) for t in r[2]) and torch.equal(sup, pattern), (status, sorted(over))

        def changed(key, i, v):
            g_ = dict(graph)
            g_[key] = graph[key].clone()
            g_[key][i] = v
            return g_

        with _open(cases[1]) as other:                              # both strands stored: not strand-symmetric
            assert not other.canonical_only
            refused(UNS, ix_=other)
        with Index.open_13(pf13_path(), None) as ix13:
            refused(MODE, ix_=ix13)
        refused(ARG, ix_=None)
        for key in ("node", "offsets", "link_off", "circular", "link_to", "offs", "out0"):
            refused(ARG, **{key: None})
        for i in range(1, 7):                                         # cap > 0 needs every entry array
            refused(ARG, **{"out%d" % i: None})
        status, tot, outs, clean = _raw(ix, graph, st, so, 0, out1=None, out2=None, out3=None, out4=None, out5=None, out6=None)
        assert status == 0 and tot == total                           # ... cap == 0 does not
        live = int(np.nonzero(node != SR.DEAD)[0][0])
        refused(ARG, graph_=changed("node", live, U << 33))                                     # a node of unitig U
        refused(ARG, graph_=changed("node", live, (int(node[live]) >> 33 << 33) | (0x7FFFFFFF << 2)))   # a position beyond its unitig
        refused(ARG, graph_=changed("link_off", 2 * U, E - 1))                                  # link_off does not end at E
        refused(ARG, graph_=changed("link_off", 1, E + 1))
        refused(ARG, graph_=changed("offsets", 2, int(g["offsets"][1])))                        # offsets do not ascend by 23
        refused(ARG, E=8 * U + 1)
        refused(UNS, U=2 ** 31 - 3)
        bad_so = so.clone()
        bad_so[1] = so[2] + 1                                                                   # sequence offsets that descend
        refused(ARG, so_=bad_so)
        # the two handle-less calls: refusals leave the outputs untouched
        ku, kp, kf = graph["kid_unitig"], graph["kid_pos"], graph["kid_flag"]
        nd = torch.full((ix.n + 64,), P64, dtype=torch.int64, device="cuda")
        bad_ku = ku.clone()
        bad_ku[live] = U
        q = lambda t: vp(t.data_ptr())
        assert L.aix_thread_nodes_dev(ix.n, q(bad_ku), q(kp), q(kf), U, q(graph["offsets"]), q(nd), None) == ARG and bool((nd == P64).all())
        assert L.aix_thread_nodes_dev(ix.n, q(ku), q(kp), q(kf), U, q(graph["offsets"]), q(nd), None) == 0
        assert torch.equal(nd[:ix.n], graph["node"]) and bool((nd[ix.n:] == P64).all())
        rm, tips, arms = ix.graph_mark_t(graph, None, 46, 46)
        nxt = ix.graph_compact_t(graph, None, rm)
        outs = [torch.full((ix.n + 64,), p_, dtype=ty, device="cuda") for p_, ty in ((P64, torch.int64), (P32, torch.int32), (P8, torch.uint8))]
        call = lambda ku_, uc_: L.aix_graph_kidmap_dev(ix.n, q(ku_), q(kp), q(kf), U, q(graph["offsets"]), q(uc_), q(nxt["unitig_pos"]), q(nxt["unitig_flag"]),
                                                       *[q(t) for t in outs], None)
        big = nxt["unitig_contig"].clone()
        big[int(un["kid_unitig"][live])] = 2 ** 31 - 4
        for args in ((bad_ku, nxt["unitig_contig"]), (ku, big)):
            assert call(*args) == ARG
            torch.cuda.synchronize()
            assert all(bool((t == p_).all()) for t, p_ in zip(outs, (P64, P32, P8)))
        assert call(ku, nxt["unitig_contig"]) == 0
        torch.cuda.synchronize()
        km = SR.kidmap(un["kid_unitig"], un["kid_pos"], un["kid_flag"], g["offsets"], _np(nxt["unitig_contig"]), _np(nxt["unitig_pos"]), _np(nxt["unitig_flag"]))
        for t, a, p_ in zip(outs, km, (P64, P32, P8)):
            assert np.array_equal(_np(t[:ix.n]), a) and bool((t[ix.n:] == p_).all())
        inplace = [ku.clone(), kp.clone(), kf.clone()]                                           # the outputs may be the inputs
        assert L.aix_graph_kidmap_dev(ix.n, *[q(t) for t in inplace], U, q(graph["offsets"]), q(nxt["unitig_contig"]), q(nxt["unitig_pos"]), q(nxt["unitig_flag"]),
                                      *[q(t) for t in inplace], None) == 0
        torch.cuda.synchronize()
        assert all(np.array_equal(_np(t), a) for t, a in zip(inplace, km))
        # corrupt arrays: random link words, and the node words dealt out to other kids. No error: BROKEN where the graph says so
        rng = np.random.default_rng(99)
        foreign = dict(graph)
        words = rng.integers(0, 1 << 32, E, dtype=np.uint64).astype(np.uint32)
        words[::3] = g["link_to"][rng.permutation(E)][::3]                                      # a third of them are link words of this graph
        foreign["link_to"] = torch.from_numpy(words.view(np.int32)).cuda()
        perm = rng.permutation(ix.n)
        foreign["node"] = graph["node"][torch.from_numpy(perm).cuda()]
        gf = dict(g, link_to=words)
        want_f = SR.thread(kid_of, node[perm], gf, b.seqs, support=np.zeros(E, np.uint64))
        assert (want_f["step_link"] == BROKEN).any()
        tf_ = len(want_f["step_link"])
        sup = _zeros(E)
        status, tot, outs, clean = _raw(ix, foreign, st, so, tf_, sup=sup)
        assert status == 0 and tot == tf_
        _same({k: _np(t[:M + 1 if i == 0 else tf_]) for i, (k, t) in enumerate(zip(SR.KEYS, outs))}, want_f, "foreign")
        assert clean(outs[0], M + 1) and all(clean(t, tf_) for t in outs[1:]) and np.array_equal(_np(sup), want_f["support"])
        junk = dict(graph, node=torch.from_numpy(rng.integers(0, 1 << 63, ix.n, dtype=np.int64)).cuda())   # random node words: refused
        refused(ARG, graph_=junk)
        # empty inputs
        e = torch.zeros(0, dtype=torch.uint8, device="cuda")
        got = ix.seq_thread_t(graph, e, torch.zeros(1, dtype=torch.int64, device="cuda"))
        assert _np(got[0]).tolist() == [0] and got[1].numel() == 0
        got = ix.seq_thread_t(graph, e, torch.zeros(4, dtype=torch.int64, device="cuda"))
        assert _np(got[0]).tolist() == [0, 0, 0, 0]
        assert ix.seq_thread([], 0)["seq_step_off"].tolist() == [0] and ix.seq_thread([b"", b"ACGT"], 0)["seq_step_off"].tolist() == [0, 0, 0]
    torch.cuda.synchronize()


def test_list_surface(planted, tmp_path):
    """7. thread_sequences, get_link_support and write_gfa_paths."""
    from aindex_amd.aindex import AIndex, format_gfa, format_gfa_paths, unitig_link_pairs
    prefix = planted("bubble_tip_cutoff")
    with _open(prefix) as ix:
        un, lk, g, kid_of, node = _ref(ix, 0)
    b = SC.batch(un, lk, 3)
    seqs = [s.decode() for s in b.seqs]
    want = SR.thread(kid_of, node, g, b.seqs, support=np.zeros(g["E"], np.uint64))
    a = AIndex.load_23mer_index(prefix + ".pf", prefix + ".tf.bin", prefix + ".kmers.bin")
    try:
        graph = a._wrapper._need23().thread_graph_t(0)
        paths = a.thread_sequences(seqs, graph=graph)
        assert len(paths) == len(seqs)
        for i, p in enumerate(paths):
            lo, hi = int(want["seq_step_off"][i]), int(want["seq_step_off"][i + 1])
            exp = [(int(want["step_unitig"][j]), "-" if want["step_flag"][j] & 1 else "+", int(want["step_pos"][j]), int(want["q_first"][j]),
                    int(want["q_last"][j]), bool(want["step_link"][j] < BROKEN)) for j in range(lo, hi)]
            assert p == exp, i
        assert a.thread_sequences(seqs[:5]) == paths[:5]               # the graph built inside
        sup = a.get_link_support(seqs, graph=graph)
        assert sup.dtype == np.uint64 and np.array_equal(sup, want["support"])
        out = str(tmp_path / "paths.gfa")
        n_paths = a.write_gfa_paths(out, seqs, graph=graph)
        lines = open(out).read().splitlines()
        ls = [l.split("\t") for l in lines if l.startswith("L")]
        dual = SR.dual_of(g)
        src = np.repeat(np.arange(2 * g["U"]), np.diff(g["link_off"].astype(np.int64))).tolist()
        kept = [j for j in range(g["E"]) if (src[j], int(g["link_to"][j])) <= (int(g["link_to"][j]) ^ 1, src[j] ^ 1)]
        assert len(kept) == len(unitig_link_pairs(lk)) == len(ls) and int(want["support"].sum()) > 0
        for f, j in zip(ls, kept):
            assert f[1:6] == ["u%d" % (src[j] >> 1), "+-"[src[j] & 1], "u%d" % (int(g["link_to"][j]) >> 1), "+-"[int(g["link_to"][j]) & 1], "22M"]
            assert f[6] == "RC:i:%d" % int(want["support"][j]) and want["support"][j] == want["support"][dual[j]]
        assert [l for l in lines if l[0] in "HS"] == [l for l in format_gfa(g, g) if l[0] in "HS"]
        ps = [l.split("\t") for l in lines if l.startswith("P")]
        assert len(ps) == n_paths == sum(1 for j in range(len(want["step_link"])) if want["step_link"][j] >= BROKEN)
        assert all(f[3] == "*" for f in ps)
        exp = []                                                      # the P lines, restated
        for i in range(len(seqs)):
            part = 0
            for j in range(int(want["seq_step_off"][i]), int(want["seq_step_off"][i + 1])):
                seg = "u%d%s" % (want["step_unitig"][j], "-" if want["step_flag"][j] & 1 else "+")
                if want["step_link"][j] >= BROKEN:
                    part += 1
                    exp.append(["seq%d" % i if part == 1 else "seq%d.%d" % (i, part), seg])
                else:
                    exp[-1][1] += "," + seg
        assert [f[1:3] for f in ps] == exp and any("," in e[1] for e in exp) and any("." in e[0] for e in exp)
        named = list(format_gfa_paths(g, g, want["support"], want, ["r%d" % i for i in range(len(seqs))]))
        assert [l.replace("\tr", "\tseq", 1) if l[0] == "P" else l for l in named] == lines
    finally:
        a._wrapper.close()
