"""Repeat resolution on the GPU (k_gr_* of aix_graphresolve.hip) against the test-side restatement (tests/graph_resolve_ref.py, pinned by
test_graph_resolve_cpu.py) on the inputs of tests/graph_resolve_cases.py and the batches of tests/seqthread_cases.py. Every comparison
is exact equality; every raw call has 64 poisoned elements behind every output."""
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
import graph_resolve_cases as RC
import graph_resolve_ref as RR
import oracle_lib as O
import seqthread_cases as SC
import seqthread_ref as SR
import unitig_links_ref as RL
import unitigs_ref as R
from aindex_amd import _lib, builder
from aindex_amd.engine import Index

vp = _lib.vp
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (0, 3, 6, 9)
KEYS = GR.GRAPH_KEYS
OUT_KEYS = KEYS + ("unitig_origin", "link_remove", "copies", "copy_base")
P64, P32, P8 = 0x6B6B6B6B6B6B6B6B, 0x6B6B6B6B, 0x6B
_UNSIGNED = {np.dtype(np.int64): np.uint64, np.dtype(np.int32): np.uint32}
_SIGNED = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}
ARG, UNS = _lib.AIX_ERR_ARG, _lib.AIX_ERR_UNSUPPORTED


def _open(prefix):
    return Index.open_23(prefix + ".pf", prefix + ".tf.bin", prefix + ".kmers.bin")


def _np(t):
    a = t.cpu().numpy()
    return a.view(_UNSIGNED.get(a.dtype, a.dtype))


def _t(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(_SIGNED.get(a.dtype, a.dtype)).copy()).cuda()


def _dev_seqs(seqs):
    import torch
    data = np.frombuffer(b"".join(seqs), dtype=np.uint8)
    offs = np.zeros(len(seqs) + 1, np.int64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    return torch.from_numpy(data.copy()).cuda(), torch.from_numpy(offs).cuda()


def _write_index(prefix, codes, tfs):
    open(prefix + ".pf", "wb").write(builder.build_pf_codes(codes, 23))
    rc, checker, tf = O.index_scatter(O.OracleMphf(prefix + ".pf"), np.ascontiguousarray(D.decode(codes)).reshape(-1), tfs)
    assert rc == 0
    checker.tofile(prefix + ".kmers.bin")
    tf.tofile(prefix + ".tf.bin")
    return prefix


def _ref(ix, cutoff):
    """(un, lk, g, kid_of, node) of the restated unitig graph, kids in the order of the handle"""
    codes, tfs = ix.checker_array() & np.uint64(R.MASK), ix.tf_array()
    un = R.unitigs(codes, tfs, cutoff)
    lk = RL.links(codes, tfs, cutoff, un)
    node = SR.nodes(un["kid_unitig"], un["kid_pos"], un["kid_flag"], un["offsets"])
    return un, lk, GR.graph(un, lk), {int(c): i for i, c in enumerate(codes.tolist())}, node


def _poisoned(n, dtype):
    import torch
    return torch.full((n + 64,), {torch.int64: P64, torch.int32: P32, torch.uint8: P8}[dtype], dtype=dtype, device="cuda")


def _intact(t, n=0):
    import torch
    return bool((t[n:] == {torch.int64: P64, torch.int32: P32, torch.uint8: P8}[t.dtype]).all())


def _q(t):
    return vp(t.data_ptr()) if t is not None else None


def _raw_pairs(gt, steps, acc, stream=None, **over):
    """aix_thread_pairs_dev itself on a pair array with 64 poisoned elements behind it -> (status, n_pairs)"""
    import torch
    a = dict(U=(gt["link_off"].numel() - 1) // 2, lo=_q(gt["link_off"]), to=_q(gt["link_to"]), E=gt["link_to"].numel(), T=steps[1].numel(), su=_q(steps[1]),
             sf=_q(steps[3]), sl=_q(steps[6]), pair=_q(acc))
    a.update({k: (_q(v) if hasattr(v, "data_ptr") else v) for k, v in over.items()})
    n = C.c_uint64(77)
    st = _lib.lib().aix_thread_pairs_dev(a["U"], a["lo"], a["to"], a["E"], a["T"], a["su"], a["sf"], a["sl"], a["pair"], C.byref(n), stream)
    torch.cuda.synchronize()
    return st, n.value


def _raw_resolve(gt, sup, pair, thresholds=(2, 2, 0), stream=None):
    """mark, layout and emit themselves, every output dirty before the call and followed by 64 poisoned elements -> dict of numpy arrays"""
    import torch
    L = _lib.lib()
    ml, mp, mn = thresholds
    U, E = gt["offsets"].numel() - 1, gt["link_to"].numel()
    rm, cp, cb = _poisoned(E, torch.uint8), _poisoned(U, torch.uint8), _poisoned(U, torch.int32)
    n = [C.c_uint64(77) for _ in range(6)]
    st = L.aix_graph_resolve_mark_dev(U, _q(gt["offsets"]), _q(gt["circular"]), _q(gt["link_off"]), _q(gt["link_to"]), E, _q(sup), _q(pair), ml, mp, mn, _q(rm), _q(cp),
                                      C.byref(n[0]), C.byref(n[1]), C.byref(n[2]), stream)
    torch.cuda.synchronize()
    if st:
        assert _intact(rm) and _intact(cp) and all(x.value == 77 for x in n)
        return {"status": st}
    assert _intact(rm, E) and _intact(cp, U)
    assert L.aix_graph_resolve_layout_dev(U, _q(gt["offsets"]), E, _q(rm), _q(cp), _q(cb), C.byref(n[3]), C.byref(n[4]), C.byref(n[5]), stream) == 0
    torch.cuda.synchronize()
    assert _intact(cb, U)
    U2, total, E2 = n[3].value, n[4].value, n[5].value
    sizes = (U2 + 1, total, U2, U2, U2, U2, 2 * U2 + 1, E2, U2)
    types = (torch.int64, torch.uint8, torch.uint8, torch.int64, torch.int32, torch.int32, torch.int64, torch.int32, torch.int32)
    outs = [_poisoned(s, ty) for s, ty in zip(sizes, types)]
    st = L.aix_graph_resolve_emit_dev(U, *[_q(gt[k]) for k in KEYS], E, _q(rm), _q(cp), _q(cb), _q(pair), mp, U2, total, E2, *[_q(t) for t in outs], stream)
    torch.cuda.synchronize()
    assert st == 0 and all(_intact(t, s) for t, s in zip(outs, sizes))
    res = {k: _np(t[:s]) for k, t, s in zip(KEYS + ("unitig_origin",), outs, sizes)}
    res.update(link_remove=_np(rm[:E]), copies=_np(cp[:U]), copy_base=_np(cb[:U]), U=U2, E=E2, n_links_removed=n[0].value, n_split=n[1].value,
               n_copies_added=n[2].value, status=0, tensors=dict(zip(KEYS, [t[:s] for t, s in zip(outs, sizes)]), rm=rm, cp=cp, cb=cb))
    return res


def _same(got, want, tag, keys=OUT_KEYS):
    for k in keys:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (tag, k)
    for k in ("U", "E", "n_links_removed", "n_split"):
        assert got[k] == want[k], (tag, k)


def _pipeline(ix, cutoff, seqs, tag, thresholds=(2, 2, 0)):
    """thread, pairs (two calls onto a prefilled pattern), raw resolve, engine resolve and host form against the restatement"""
    import torch
    un, lk, g, kid_of, node = _ref(ix, cutoff)
    graph = ix.thread_graph_t(cutoff)
    want_steps = SR.thread(kid_of, node, g, seqs, support=np.zeros(g["E"], np.uint64))
    want_pair, want_n = RR.pairs(g, want_steps)
    sup = torch.zeros(g["E"], dtype=torch.int64, device="cuda")
    steps = ix.seq_thread_t(graph, *_dev_seqs(seqs), link_support=sup)
    assert np.array_equal(_np(sup), want_steps["support"]), tag
    pair, n = ix.thread_pairs_t(graph, steps)
    assert n == want_n and np.array_equal(_np(pair), want_pair), tag
    # two batches onto a prefilled pattern, the array followed by poison
    half = len(seqs) // 2
    acc = _poisoned(16 * g["U"], torch.int64)
    pattern = torch.arange(16 * g["U"], dtype=torch.int64, device="cuda") * 5 + 3
    acc[:16 * g["U"]] = pattern
    total = 0
    for part in (seqs[:half], seqs[half:]):
        st, k = _raw_pairs(graph, ix.seq_thread_t(graph, *_dev_seqs(part)), acc)
        assert st == 0
        total += k
    assert total == want_n and _intact(acc, 16 * g["U"]) and np.array_equal(_np(acc[:16 * g["U"]]), _np(pattern) + want_pair), tag
    want = RR.resolve(g, want_steps["support"], want_pair, *thresholds)
    got = _raw_resolve(graph, sup, pair, thresholds)
    _same(got, want, (tag, "raw"))
    assert got["n_copies_added"] == want["n_copies_added"]
    eng = ix.graph_resolve_t(graph, sup, pair, *thresholds, compact=False)
    _same({k: (_np(v) if hasattr(v, "cpu") else v) for k, v in eng.items()}, want, (tag, "engine"))
    host = ix.graph_resolve(g, want_steps["support"], want_pair, *thresholds)
    _same(host, want, (tag, "host"), KEYS + ("unitig_origin", "link_remove", "copies"))
    return g, graph, sup, pair, want, got


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("gr"))
    return {seed: G.write_graph_case(seed, d)[0] for seed in SEEDS}


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("grp"))
    made = {}

    def get(name):
        if name not in made:
            p = RC.planted(name)
            made[name] = (_write_index(os.path.join(d, name), p.codes, p.tfs), p)
        return made[name]
    return get


@pytest.mark.parametrize("seed", SEEDS)
def test_graph_cases(cases, seed):
    """1. Graph cases at cutoffs 0 and 3 with the walk batches of seqthread_cases: every form, two threshold sets."""
    with _open(cases[seed]) as ix:
        for cutoff in (0, 3):
            un, lk, g, kid_of, node = _ref(ix, cutoff)
            seqs = SC.batch(un, lk, seed).seqs
            g, graph, sup, pair, want, got = _pipeline(ix, cutoff, seqs, (seed, cutoff))
            # the walks of these sparse graphs seldom pass a whole unitig between two links: 14 to 26 transitions, none in three of the cases
            assert (int(_np(pair).sum()) > 0) == ((seed, cutoff) not in ((0, 3), (3, 0), (3, 3)))
            want1 = RR.resolve(g, _np(sup), _np(pair), 1, 1, 0)
            _same(_raw_resolve(graph, sup, pair, (1, 1, 0)), want1, (seed, cutoff, "1, 1, 0"))
            RR.validate({k: want1[k] for k in KEYS})


@pytest.mark.parametrize("name", RC.PLANTED)
def test_planted_cases(planted, name):
    """2. Every planted case: the resolution equals the restatement's; resolve followed by the existing compaction on the GPU equals the
    restatement's compaction and gives the planted genomes."""
    import torch
    prefix, p = planted(name)
    with _open(prefix) as ix:
        un, lk, g, kid_of, node = _ref(ix, 0)
        seqs = p.reads if p.reads is not None else SC.batch(un, lk, 1).seqs
        g, graph, sup, pair, want, got = _pipeline(ix, 0, seqs, name)
        if p.n_split is not None:
            assert (got["n_split"], got["n_links_removed"]) == (p.n_split, p.n_removed)
        gr = {k: want[k] for k in KEYS}
        gr["U"], gr["E"] = want["U"], want["E"]
        cw = GR.compact(gr, np.zeros(want["U"], np.uint8))
        merged = ix.graph_resolve_t(graph, sup, pair, compact=True)
        for k in KEYS:
            assert np.array_equal(_np(merged[k]), cw[k]), (name, k)
        assert np.array_equal(_np(merged["unitig_origin"]), want["unitig_origin"]) and merged["U"] == cw["C"]
        rm, tips, arms = ix.graph_mark_t(got["tensors"], None, 46, 46)    # the existing mark accepts G_r
        assert np.array_equal(_np(rm), GR.mark(gr, 46, 46))
        if p.contigs is not None:
            text, off = _np(merged["bases"]).tobytes().decode(), _np(merged["offsets"]).tolist()
            assert sorted(RC.canon_str(text[off[i]:off[i + 1]]) for i in range(merged["U"])) == p.contigs and merged["E"] == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("seed", (0, 1))
def test_link_structures(planted, seed):
    """3. The hand-made link structures: cells at the thresholds, d = 2 .. 4, lattices of split unitigs, 128-bit abundances; the
    asymmetric support is refused with nothing written."""
    import torch
    g = RC.make_resolve_graph(seed)
    th = g["thresholds"]
    want = RR.resolve(g, g["link_support"], g["pair_support"], *th)
    assert {c: int(want["copies"][c]) for c in g["want"]} == g["want"]
    gt = {k: _t(g[k]) for k in KEYS}
    sup, pair = _t(g["link_support"]), _t(g["pair_support"])
    got = _raw_resolve(gt, sup, pair, th)
    _same(got, want, seed)
    for a, b in ((sup, None), (None, pair), (None, None)):                 # a rule without its array is off
        _same(_raw_resolve(gt, a, b, th), RR.resolve(g, None if a is None else g["link_support"], None if b is None else g["pair_support"], *th), (seed, "off"))
    same = _raw_resolve(gt, None, None, th)                                # property (a)
    assert all(np.array_equal(same[k], g[k]) for k in KEYS) and same["unitig_origin"].tolist() == list(range(g["U"]))
    with _open(planted("two_copy")[0]) as ix:                              # the host form takes no handle; the method lives on one
        host = ix.graph_resolve(g, g["link_support"], g["pair_support"], *th)
    _same(host, want, (seed, "host"), KEYS + ("unitig_origin", "link_remove", "copies"))
    assert _raw_resolve(gt, _t(RC.asymmetric(g)["link_support"]), pair, th)["status"] == ARG
    assert _raw_resolve(gt, sup, pair, (th[0], th[1], th[1]))["status"] == ARG


_CHILD = """
import hashlib, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import torch
import graph_resolve_cases as RC
from aindex_amd.engine import Index
h = hashlib.sha256()
p = sys.argv[2]
seqs = [l.rstrip(b"\\n") for l in open(p + ".seqs", "rb")]
data = np.frombuffer(b"".join(seqs), dtype=np.uint8)
offs = np.zeros(len(seqs) + 1, np.int64); offs[1:] = np.cumsum([len(s) for s in seqs])
with Index.open_23(p + ".pf", p + ".tf.bin", p + ".kmers.bin") as ix:
    graph = ix.thread_graph_t(0)
    sup = torch.zeros(graph["E"], dtype=torch.int64, device="cuda")
    steps = ix.seq_thread_t(graph, torch.from_numpy(data.copy()).cuda(), torch.from_numpy(offs).cuda(), link_support=sup)
    pair, n = ix.thread_pairs_t(graph, steps)
    res = ix.graph_resolve_t(graph, sup, pair, compact=False)
    for k in %r:
        h.update(np.ascontiguousarray(res[k].cpu().numpy()).tobytes())
    h.update(pair.cpu().numpy().tobytes())
    g = RC.make_resolve_graph(0)
    host = ix.graph_resolve(g, g["link_support"], g["pair_support"], *g["thresholds"])
    for k in %r:
        h.update(np.ascontiguousarray(host[k]).tobytes())
print("digest", h.hexdigest())
""" % (OUT_KEYS, KEYS + ("unitig_origin", "link_remove", "copies"))


def test_many_trips_of_every_loop(planted, monkeypatch):
    """4. AIX_UG_TEST_GRID = 1, 2, 3 workgroups for every launch: in this process (the switch is read per call) and in fresh child
    processes; the same bytes as the restatement."""
    import torch
    prefix, p = planted("four_copy")
    open(prefix + ".seqs", "wb").write(b"".join(s + b"\n" for s in p.reads))
    h = hashlib.sha256()
    with _open(prefix) as ix:
        un, lk, g, kid_of, node = _ref(ix, 0)
        steps = SR.thread(kid_of, node, g, p.reads, support=np.zeros(g["E"], np.uint64))
        pair, n = RR.pairs(g, steps)
        want = RR.resolve(g, steps["support"], pair)
        for k in OUT_KEYS:
            h.update(np.ascontiguousarray(want[k]).tobytes())
        h.update(pair.tobytes())
        lg = RC.make_resolve_graph(0)
        lwant = RR.resolve(lg, lg["link_support"], lg["pair_support"], *lg["thresholds"])
        for k in KEYS + ("unitig_origin", "link_remove", "copies"):
            h.update(np.ascontiguousarray(lwant[k]).tobytes())
        lt = {k: _t(lg[k]) for k in KEYS}
        for grid in ("1", "2", "3"):
            monkeypatch.setenv("AIX_UG_TEST_GRID", grid)
            _pipeline(ix, 0, p.reads, ("grid", grid))
            _same(_raw_resolve(lt, _t(lg["link_support"]), _t(lg["pair_support"]), lg["thresholds"]), lwant, ("grid", grid, "links"))
        monkeypatch.delenv("AIX_UG_TEST_GRID")
    torch.cuda.synchronize()
    kids = []
    for grid in ("1", "2", "3"):
        env = dict(os.environ, AIX_UG_TEST_GRID=grid)
        kids.append(subprocess.Popen([sys.executable, "-c", _CHILD, ROOT, prefix], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE))
    for grid, k in zip("123", kids):
        out, err = k.communicate(timeout=300)
        assert k.returncode == 0, (grid, err.decode()[-2000:])
        assert out.decode().split()[-2:] == ["digest", h.hexdigest()], grid


def test_side_stream(planted):
    """5. Threading, pairs and the resolution on a side stream."""
    import torch
    prefix, p = planted("adjacent")
    with _open(prefix) as ix:
        un, lk, g, kid_of, node = _ref(ix, 0)
        steps = SR.thread(kid_of, node, g, p.reads, support=np.zeros(g["E"], np.uint64))
        want_pair, n = RR.pairs(g, steps)
        want = RR.resolve(g, steps["support"], want_pair)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            graph = ix.thread_graph_t(0)
            sup = torch.zeros(g["E"], dtype=torch.int64, device="cuda")
            st = ix.seq_thread_t(graph, *_dev_seqs(p.reads), link_support=sup)
            pair = torch.zeros(16 * g["U"], dtype=torch.int64, device="cuda")
            status, k = _raw_pairs(graph, st, pair, stream=vp(side.cuda_stream))
            got = _raw_resolve(graph, sup, pair, stream=vp(side.cuda_stream))
            eng = ix.graph_resolve_t(graph, sup, pair, compact=True)
        side.synchronize()
        assert status == 0 and k == n and np.array_equal(_np(pair), want_pair)
        _same(got, want, "side stream")
        assert eng["U"] == 3 and eng["E"] == 0
    torch.cuda.synchronize()


def test_refusals_leave_everything_untouched(planted):
    """6. Every refusal leaves the outputs and pair_support untouched."""
    import torch
    L = _lib.lib()
    prefix, p = planted("two_copy")
    with _open(prefix) as ix:
        un, lk, g, kid_of, node = _ref(ix, 0)
        graph = ix.thread_graph_t(0)
        sup = torch.zeros(g["E"], dtype=torch.int64, device="cuda")
        steps = ix.seq_thread_t(graph, *_dev_seqs(p.reads), link_support=sup)
        U, E, T = g["U"], g["E"], steps[1].numel()
        pattern = torch.arange(16 * U, dtype=torch.int64, device="cuda") + 9

        def refused(status, steps_=steps, graph_=graph, **over):
            acc = _poisoned(16 * U, torch.int64)
            acc[:16 * U] = pattern
            st, n = _raw_pairs(graph_, steps_, acc, **over)
            assert st == status and n == 77 and torch.equal(acc[:16 * U], pattern) and _intact(acc, 16 * U), (status, sorted(over))

        def changed(i, idx, v):
            s = list(steps)
            s[i] = steps[i].clone()
            s[i][idx] = v
            return s

        linked = (steps[6] >= 0) & (steps[6] < E)
        tr = int(torch.nonzero(linked[:-1] & linked[1:])[0][0])          # a transition
        for k in ("lo", "to", "su", "sf", "sl", "pair"):
            refused(ARG, **{k: None})
        refused(ARG, E=8 * U + 1)
        refused(UNS, U=2 ** 31 - 3)
        refused(ARG, steps_=changed(1, tr, U))                          # a unitig beyond U
        refused(ARG, steps_=changed(6, tr, E))                          # neither a link nor a sentinel
        refused(ARG, steps_=changed(6, 0, 0))                           # the first step has a link
        refused(ARG, steps_=changed(1, tr, (int(steps[1][tr]) + 1) % U))   # the link does not enter that unitig
        refused(ARG, steps_=changed(3, tr, int(steps[3][tr]) ^ 1))      # ... nor in that direction
        refused(ARG, steps_=changed(6, tr + 1, (int(steps[6][tr + 1]) + 4) % E))   # an exit link of another end
        bad_lo = dict(graph, link_off=graph["link_off"].clone())
        bad_lo["link_off"][2 * U] = E - 1
        refused(ARG, graph_=bad_lo)
        bad_to = dict(graph, link_to=graph["link_to"].clone())        # the dual of the entry link is gone
        a = int(steps[6][tr])
        e_prev = 2 * int(steps[1][tr - 1]) + (int(steps[3][tr - 1]) & 1)
        t = int(graph["link_to"][a])
        lo = _np(graph["link_off"]).tolist()
        d = next(j for j in range(lo[t ^ 1], lo[(t ^ 1) + 1]) if int(graph["link_to"][j]) == e_prev ^ 1)
        bad_to["link_to"][d] = 2 * U - 1 - (e_prev ^ 1)
        refused(ARG, graph_=bad_to)
        acc = pattern.clone()
        assert _raw_pairs(graph, steps, acc, T=0, su=None, sf=None, sl=None) == (0, 0) and torch.equal(acc, pattern)
        # the resolution: arrays that are no unitig set, splits the arrays do not support, wrong sizes
        pair, n = ix.thread_pairs_t(graph, steps)
        ok = _raw_resolve(graph, sup, pair)
        assert ok["status"] == 0 and ok["n_split"] == 1
        assert _raw_resolve(bad_lo, sup, pair)["status"] == ARG
        assert _raw_resolve(bad_to, sup, pair)["status"] == ARG           # a link without its dual
        bad_sup = sup.clone()
        bad_sup[0] += 1
        assert _raw_resolve(graph, bad_sup, pair)["status"] == ARG
        t_ = ok["tensors"]
        n3 = [C.c_uint64(77) for _ in range(3)]
        cb = _poisoned(U, torch.int32)
        five = t_["cp"].clone()
        five[0] = 5
        assert L.aix_graph_resolve_layout_dev(U, _q(graph["offsets"]), E, _q(t_["rm"]), _q(five), _q(cb), *[C.byref(x) for x in n3], None) == ARG
        torch.cuda.synchronize()
        assert _intact(cb) and all(x.value == 77 for x in n3)

        def emit(status, **over):
            sizes = (ok["U"] + 1, int(ok["offsets"][-1]), ok["U"], ok["U"], ok["U"], ok["U"], 2 * ok["U"] + 1, ok["E"], ok["U"])
            types = (torch.int64, torch.uint8, torch.uint8, torch.int64, torch.int32, torch.int32, torch.int64, torch.int32, torch.int32)
            outs = [_poisoned(s, ty) for s, ty in zip(sizes, types)]
            a = dict(g=graph, rm=t_["rm"], cp=t_["cp"], cb=t_["cb"], pair=pair, mp=2, U2=ok["U"], total=sizes[1], E2=ok["E"])
            a.update(over)
            st = L.aix_graph_resolve_emit_dev(U, *[_q(a["g"][k]) for k in KEYS], E, _q(a["rm"]), _q(a["cp"]), _q(a["cb"]), _q(a["pair"]), a["mp"], a["U2"], a["total"],
                                              a["E2"], *[_q(t) for t in outs], None)
            torch.cuda.synchronize()
            assert st == status and (status == 0 or all(_intact(t) for t in outs)), (status, sorted(over))

        emit(0)
        emit(ARG, pair=None)                                              # a split without the cells that justify it
        emit(ARG, mp=0)
        emit(ARG, mp=20)                                                  # no cell is strong
        emit(ARG, U2=ok["U"] + 1)
        emit(ARG, total=int(ok["offsets"][-1]) + 1)
        emit(ARG, E2=ok["E"] - 1)
        other = t_["cp"].clone()
        other[0], other[1] = 1, 2                                         # a split of a unitig with one link per end
        emit(ARG, cp=other)
        moved = t_["cb"].clone()
        moved[0] += 1
        emit(ARG, cb=moved)
        one = t_["rm"].clone()
        one[0] = 1                                                        # removed without its dual
        emit(ARG, rm=one, E2=ok["E"] - 1)
        emit(ARG, g=bad_to)
    torch.cuda.synchronize()


def test_list_surface(planted, tmp_path):
    """7. get_resolved_contigs and write_resolved_contigs next to get_contigs."""
    from aindex_amd.aindex import AIndex
    prefix, p = planted("two_copy")
    a = AIndex.load_23mer_index(prefix + ".pf", prefix + ".tf.bin", prefix + ".kmers.bin")
    try:
        reads = [r.decode() for r in p.reads]
        before = a.get_contigs(0, 0, 0, 0)
        got = a.get_resolved_contigs(reads, rounds=0)
        assert len(before) == 5 and sorted(RC.canon_str(s) for s, _, _ in got) == p.contigs
        assert sum(tf for _, tf, _ in got) == sum(tf for _, tf, _ in before) and not any(c for _, _, c in got)
        assert a.get_resolved_contigs(reads, rounds=0, min_pair_support=0) == before           # nothing to decide with
        a.RESOLVE_BATCH_BYTES = 2000                                                           # several batches, accumulated
        assert a.get_resolved_contigs(reads, rounds=0) == got
        out = str(tmp_path / "resolved.fa")
        assert a.write_resolved_contigs(out, reads, rounds=0) == 2
        lines = open(out).read().splitlines()
        assert [l for l in lines if not l.startswith(">")] == [s for s, _, _ in got]
        assert lines[0].split()[:2] == [">c0", "LN:i:280"]
    finally:
        a._wrapper.close()
