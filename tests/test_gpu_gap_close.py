"""Gap closing on the GPU (k_gp_* and k_gf_* of aix_gapclose.hip) against the test-side restatement (tests/gap_close_ref.py, pinned by
test_gap_close_cpu.py) on the inputs of tests/gap_close_cases.py and the planted genomes of tests/scaffold_cases.py. Every comparison
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
import gap_close_cases as GC
import gap_close_ref as GF
import oracle_lib as O
import scaffold_cases as SC
import scaffold_ref as SF
from aindex_amd import _lib, builder
from aindex_amd.engine import Index

vp = _lib.vp
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P64, P32, P8 = 0x6B6B6B6B6B6B6B6B, 0x6B6B6B6B, 0x6B
_UNSIGNED = {np.dtype(np.int64): np.uint64, np.dtype(np.int32): np.uint32}
_SIGNED = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}
ARG = _lib.AIX_ERR_ARG
GRAPH = ("offsets", "link_off", "link_to", "join", "join_gap")
CLOSE = ("close_status", "close_dist", "close_states", "path_off", "path", "fill_uses", "counts")
FILL = ("fmember_off", "fmember", "fmember_flag", "fmember_gap", "fmember_pos", "fscaffold_offsets", "fscaffold_bases")
NONE32 = SF.NONE32


def _np(t):
    a = t.cpu().numpy()
    return a.view(_UNSIGNED.get(a.dtype, a.dtype))


def _t(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(_SIGNED.get(a.dtype, a.dtype)).copy()).cuda()


def _poison_of(dtype):
    import torch
    return {torch.int64: P64, torch.int32: P32, torch.uint8: P8}[dtype]


def _poisoned(n, dtype):
    import torch
    return torch.full((n + 64,), _poison_of(dtype), dtype=dtype, device="cuda")


def _intact(t, n=0):
    return bool((t[n:] == _poison_of(t.dtype)).all())


def _q(t):
    return vp(t.data_ptr()) if t is not None else None


def _sync():
    import torch
    torch.cuda.synchronize()


def _dev(g, keys=GRAPH + ("bases",)):
    return {k: _t(g[k]) for k in keys}


def _same(got, want, keys, tag):
    for k in keys:
        g = got[k]
        g = g.view(want[k].dtype) if g.dtype != want[k].dtype and g.dtype.itemsize == want[k].dtype.itemsize else g
        assert g.dtype == want[k].dtype and np.array_equal(g, want[k]), (tag, k)


# ---- the raw calls, every output dirty and followed by poison ---------------------------------------------
def _raw_close(gt, params, cap=None, stream=None):
    """aix_gap_close_dev -> dict (status alone on a refusal); cap None: sized first (cap 0, path NULL), then filled at exactly the total"""
    import torch
    L = _lib.lib()
    U, E = gt["offsets"].numel() - 1, gt["link_to"].numel()
    total = C.c_uint64(77)
    sizes = (2 * U, 2 * U, 2 * U, 2 * U + 1, U, 5)
    types = (torch.uint8, torch.int64, torch.int32, torch.int64, torch.int32, torch.int64)

    def run(cap):
        outs = [_poisoned(n, dt) for n, dt in zip(sizes, types)]
        path = _poisoned(cap, torch.int32)
        st = L.aix_gap_close_dev(U, *[_q(gt[k]) for k in GRAPH[:3]], E, _q(gt["join"]), _q(gt["join_gap"]), params["tolerance"], params["max_fill"], params["max_states"],
                                 *[_q(o) for o in outs[:4]], _q(path) if cap else None, cap, C.byref(total), _q(outs[4]), _q(outs[5]), stream)
        _sync()
        if st:
            assert all(_intact(o) for o in outs) and _intact(path) and total.value == 77
            return st, None, None
        assert all(_intact(o, n) for o, n in zip(outs, sizes)) and _intact(path, total.value if total.value <= cap else 0)
        return 0, outs, path

    if cap is None:
        st, outs, path = run(0)
        if st:
            return {"status": st}
        cap = total.value
    st, outs, path = run(cap)
    if st:
        return {"status": st}
    T = total.value
    res = {k: _np(o[:n]) for k, o, n in zip(CLOSE[:4] + CLOSE[5:], outs, sizes)}
    res.update(status=0, total=T, tensors={k: o[:n] for k, o, n in zip(CLOSE[:4] + CLOSE[5:], outs, sizes)})
    if T <= cap:
        res["path"] = _np(path[:T])
        res["tensors"]["path"] = path[:T]
    return res


def _raw_fill_layout(gt, mt, ct, min_gap=1, stream=None):
    """aix_scaffold_fill_layout_dev -> dict; mt: member_off, member; ct: the closure tensors"""
    import torch
    U, E, Sc, pt = gt["offsets"].numel() - 1, gt["link_to"].numel(), mt["member_off"].numel() - 1, ct["path"].numel()
    sizes = (Sc + 1, U + pt, U + pt, U + pt, U + pt, Sc + 1)
    outs = [_poisoned(n, dt) for n, dt in zip(sizes, (torch.int64, torch.int32, torch.uint8, torch.int64, torch.int64, torch.int64))]
    n = [C.c_uint64(77), C.c_uint64(77)]
    st = _lib.lib().aix_scaffold_fill_layout_dev(U, *[_q(gt[k]) for k in GRAPH[:3]], E, _q(gt["join"]), _q(gt["join_gap"]), min_gap, Sc, _q(mt["member_off"]), _q(mt["member"]),
                                                 _q(ct["close_status"]), _q(ct["close_dist"]), _q(ct["path_off"]), _q(ct["path"]) if pt else None, pt, *[_q(o) for o in outs],
                                                 C.byref(n[0]), C.byref(n[1]), stream)
    _sync()
    if st:
        assert all(_intact(o) for o in outs) and all(x.value == 77 for x in n)
        return {"status": st}
    Mf = n[0].value
    used = (Sc + 1, Mf, Mf, Mf, Mf, Sc + 1)
    assert Mf <= U + pt and all(_intact(o, k) for o, k in zip(outs, used))
    res = {k: _np(o[:m]) for k, o, m in zip(FILL[:6], outs, used)}
    res.update(status=0, n_fmembers=Mf, total_bases=n[1].value, tensors={k: o[:m] for k, o, m in zip(FILL[:6], outs, used)})
    return res


def _raw_fill_emit(gt, ft, Mf, total, min_gap=1, stream=None):
    import torch
    U, Sc = gt["offsets"].numel() - 1, ft["fmember_off"].numel() - 1
    out = _poisoned(total, torch.uint8)
    st = _lib.lib().aix_scaffold_fill_emit_dev(U, _q(gt["offsets"]), _q(gt["bases"]), min_gap, Sc, _q(ft["fmember_off"]), Mf, _q(ft["fmember"]), _q(ft["fmember_flag"]),
                                               _q(ft["fmember_gap"]), _q(ft["fmember_pos"]), _q(ft["fscaffold_offsets"]), total, _q(out), stream)
    _sync()
    if st:
        assert _intact(out)
        return {"status": st}
    assert _intact(out, total)
    return {"status": 0, "fscaffold_bases": _np(out[:total])}


def _members(g, min_gap=1):
    lay = SF.layout(g["offsets"], g["join"], g["join_count"], g["join_gap"], min_gap)
    return SF.emit(g["offsets"], g["bases"], g["join"], g["join_gap"], lay, min_gap)


def _want(g, em, params, min_gap=1):
    return GF.fill(*[g[k] for k in ("offsets", "bases", "link_off", "link_to", "join", "join_gap")], em["member_off"], em["member"], **params, min_gap=min_gap)


def _fill_all(gt, g, em, params, tag, min_gap=1, stream=None, want=None):
    """search, layout and emit, raw, against the restatement -> (want, closure, layout)"""
    want = _want(g, em, params, min_gap) if want is None else want
    cl = _raw_close(gt, params, stream=stream)
    assert cl["status"] == 0 and cl["total"] == want["total"], tag
    _same(cl, want, CLOSE, (tag, "search"))
    lay = _raw_fill_layout(gt, {k: _t(em[k]) for k in ("member_off", "member")}, cl["tensors"], min_gap, stream)
    assert lay["status"] == 0 and (lay["n_fmembers"], lay["total_bases"]) == (want["n_fmembers"], want["total_bases"]), tag
    _same(lay, want, FILL[:6], (tag, "layout"))
    eb = _raw_fill_emit(gt, lay["tensors"], lay["n_fmembers"], lay["total_bases"], min_gap, stream)
    assert eb["status"] == 0
    _same(eb, want, FILL[6:], (tag, "emit"))
    return want, cl, lay


def _digest(res, keys):
    h = hashlib.sha256()
    for k in keys:
        h.update(np.ascontiguousarray(res[k]).tobytes())
    return h.hexdigest()


@pytest.fixture(scope="module")
def batches():
    made = {}

    def get(J):
        if J not in made:
            g = GC.make_batch(J, J)
            em = _members(g)
            made[J] = (g, em, _want(g, em, GC.PARAMS))                     # the reference once, shared and left unchanged
        return made[J]
    return get


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("gc"))
    made = {}

    def get(name):
        if name not in made:
            p = SC.planted(name)
            made[name] = (_write_index(os.path.join(d, name), p.codes, p.tfs), p)
        return made[name]
    return get


# ---- 1. the planted genomes, end to end -----------------------------------------------------------------
def _write_index(prefix, codes, tfs):
    open(prefix + ".pf", "wb").write(builder.build_pf_codes(codes, 23))
    rc, checker, tf = O.index_scatter(O.OracleMphf(prefix + ".pf"), np.ascontiguousarray(D.decode(codes)).reshape(-1), tfs)
    assert rc == 0
    checker.tofile(prefix + ".kmers.bin")
    tf.tofile(prefix + ".tf.bin")
    return prefix


def _dev_seqs(seqs):
    import torch
    data = np.frombuffer(b"".join(seqs), dtype=np.uint8)
    offs = np.zeros(len(seqs) + 1, np.int64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    return torch.from_numpy(data.copy()).cuda(), torch.from_numpy(offs).cuda()


FILLED_LENGTHS = {"two_copy": [1150, 1150], "jitter": [1150, 1150], "inverted": [1800], "chain3": [1800, 1800], "cycle": [1844]}


@pytest.mark.parametrize("name", SC.PLANTED)
def test_planted_cases(planted, tmp_path, name):
    """Every planted case through thread_graph_t, seq_thread_t, the scaffold calls and the new ones, raw, by the engine methods, by the
    host form and on the AIndex surface: the restatement's arrays, every join closed, the planted genomes back whole."""
    from aindex_amd.aindex import AIndex
    prefix, p = planted(name)
    par = dict(insert_size=p.insert, min_pairs=2, dominance=2, min_contig_bases=SC.MIN_BASES)
    params = dict(tolerance=10, max_fill=16, max_states=1024)
    a = AIndex.load_23mer_index(prefix + ".pf", prefix + ".tf.bin", prefix + ".kmers.bin")
    try:
        ix = a._wrapper._need23()
        graph = ix.thread_graph_t(0)
        data_t, offs_t = _dev_seqs(SC.mates(p.pairs))
        key, d, _, hist = ix.mate_links_t(graph, ix.seq_thread_t(graph, data_t, offs_t), offs_t, 1, 1000)
        joins = ix.scaffold_mark_t(graph, ix.mate_bundle_t(key, d, int(graph["U"])), **par)
        sc = ix.scaffold_t(graph, joins, 1)
        g = {k: _np(graph[k]) for k in ("offsets", "bases", "link_off", "link_to")}
        g.update(join=_np(joins["join"]), join_gap=_np(joins["join_gap"]).view(np.int64))
        em = {k: _np(sc[k]) for k in ("member_off", "member")}
        gt = dict(graph, join=joins["join"], join_gap=joins["join_gap"])
        want, cl, lay = _fill_all(gt, g, em, params, name)
        n_joins = joins["n_joins"]
        assert want["counts"].tolist() == [n_joins, 0, 0, 0, n_joins] and n_joins > 0
        mo = em["member_off"].tolist()
        lens = np.diff(want["fscaffold_offsets"].astype(np.int64)).tolist()
        assert [lens[s] for s in range(len(lens)) if mo[s + 1] - mo[s] > 1] == FILLED_LENGTHS[name]
        # the engine methods and the host form
        ec = ix.gap_close_t(graph, joins, **params)
        _same({k: _np(v) for k, v in ec.items() if hasattr(v, "cpu")}, want, CLOSE[:6], (name, "engine search"))
        assert ec["counts"] == want["counts"].tolist() and ec["total"] == want["total"]
        ef = ix.scaffold_fill_t(graph, joins, sc, ec, 1)
        _same({k: _np(v) for k, v in ef.items() if hasattr(v, "cpu")}, want, FILL, (name, "engine fill"))
        assert (ef["n_fmembers"], ef["total_bases"]) == (want["n_fmembers"], want["total_bases"])
        host = ix.scaffold_fill(g["offsets"], g["bases"], g["link_off"], g["link_to"], g["join"], g["join_gap"], em["member_off"], em["member"], **params, min_gap=1)
        _same(host, want, CLOSE[:6] + FILL, (name, "host"))
        assert (host["counts"], host["total"], host["n_fmembers"], host["total_bases"]) == (want["counts"].tolist(), want["total"], want["n_fmembers"], want["total_bases"])
        # the list surface: without close_gaps what get_scaffolds gives today; with it the filled scaffolds
        kw = dict(min_contig_bases=SC.MIN_BASES, rounds=0)
        text, so, mo2 = _np(sc["scaffold_bases"]).tobytes().decode(), _np(sc["scaffold_offsets"]).tolist(), mo
        mem, mg = em["member"].tolist(), _np(sc["member_gap"]).view(np.int64).tolist()
        today = [(text[so[i]:so[i + 1]], [(w >> 1, "+-"[w & 1], x) for w, x in zip(mem[mo2[i]:mo2[i + 1]], mg[mo2[i]:mo2[i + 1]])]) for i in range(len(so) - 1)]
        assert a.get_scaffolds(p.pairs, **kw) == today == a.get_scaffolds(p.pairs, close_gaps=False, gap_tolerance=3, drop_absorbed=False, **kw)
        ftext, fso, fo = want["fscaffold_bases"].tobytes().decode(), want["fscaffold_offsets"].tolist(), want["fmember_off"].tolist()
        fm, ff, fg = want["fmember"].tolist(), want["fmember_flag"].tolist(), want["fmember_gap"].tolist()
        filled = [(ftext[fso[i]:fso[i + 1]], [(fm[j] >> 1, "+-"[fm[j] & 1], -22 if ff[j] & 1 else fg[j], "fill" if ff[j] & 2 else "member") for j in range(fo[i], fo[i + 1])])
                  for i in range(len(fso) - 1)]
        assert a.get_scaffolds(p.pairs, close_gaps=True, gap_tolerance=10, drop_absorbed=False, **kw) == filled
        kept = [x for x in filled if len(x[1]) > 1]
        got = a.get_scaffolds(p.pairs, close_gaps=True, gap_tolerance=10, **kw)
        assert got == kept and [len(s) for s, _ in got] == FILLED_LENGTHS[name] and all(SC.located(p, s) is not None for s, _ in got)
        out = str(tmp_path / "f.fa")
        assert a.write_scaffolds(out, p.pairs, close_gaps=True, gap_tolerance=10, **kw) == len(kept)
        assert open(out).read().splitlines()[1::2] == [s for s, _ in kept]
        out = str(tmp_path / "f.agp")
        n = a.write_scaffolds_agp(out, p.pairs, close_gaps=True, gap_tolerance=10, **kw)
        agp = [l.split("\t") for l in open(out).read().splitlines() if not l.startswith("#")]
        off = g["offsets"].tolist()
        assert n == len(agp) == sum(len(m) for _, m in kept) and all(r[4] == "W" for r in agp)
        for i, (s, members) in enumerate(kept):
            rows = [r for r in agp if r[0] == "s%d" % i]
            assert int(rows[-1][2]) == len(s) and int(rows[0][1]) == 1 and all(int(x[2]) + 1 == int(y[1]) for x, y in zip(rows, rows[1:]))
            assert [(int(r[5][1:]), r[8], int(r[6]), int(r[7])) for r in rows] == [(u, o, 23 if gap == -22 else 1, off[u + 1] - off[u]) for u, o, gap, _ in members]
        recs = a.get_gap_closures(p.pairs, gap_tolerance=10, **kw)
        po, path = want["path_off"].tolist(), want["path"].tolist()
        assert recs == [(e, int(t), int(g["join_gap"][e]), "closed", int(want["close_dist"][e]), path[po[e]:po[e + 1]], int(want["close_states"][e]))
                        for e, t in enumerate(g["join"].tolist()) if t != NONE32 and e < t ^ 1] and len(recs) == n_joins
    finally:
        a._wrapper.close()
    _sync()


# ---- 2. the hand-made cases -------------------------------------------------------------------------------
@pytest.mark.parametrize("dual", (True, False))
def test_hand_made_cases(dual):
    """The literals of every case, then the budget at exactly the states of the complete search and one below: 4, 12, 252 and 4 092
    states cross one and many rounds of 64; the fans put 63, 64 and 65 states at a round boundary."""
    for name in GC.NAMES:
        g, params, want = GC.case(name, dual)
        gt, em = _dev(g), _members(g)
        w, cl, _ = _fill_all(gt, g, em, params, name)
        e = g["probe"]
        got = (int(cl["close_status"][e]), int(cl["close_states"][e]), int(cl["close_dist"].view(np.int64)[e]), cl["path"][int(cl["path_off"][e]):int(cl["path_off"][e + 1])].tolist())
        assert got == want, name
        if want[0] == 3:
            n = want[1]
            for budget, status in ((n, 3), (n - 1, 4)):
                if budget:
                    p2 = dict(params, max_states=budget)
                    c2 = _raw_close(gt, p2)
                    _same(c2, GF.search(*[g[k] for k in GRAPH], **p2), CLOSE, (name, budget))
                    assert (c2["close_status"][e], c2["close_states"][e]) == (status, budget), (name, budget)


def test_non_owner_traversal_and_small_gaps():
    for g, params, min_gap in ((GC.non_owner_case()[0], dict(tolerance=0, max_fill=16, max_states=1024), 1),
                               (GC.non_owner_case(400)[0], dict(tolerance=0, max_fill=16, max_states=1024), 1),
                               (GC.below_min_gap_case(), dict(tolerance=5, max_fill=0, max_states=1), 3)):
        want, cl, lay = _fill_all(_dev(g), g, _members(g, min_gap), params, "small", min_gap)
        assert want["counts"][0] >= 1
    assert want["close_dist"].tolist() == [-22, 0, 0, -22, 0, 0] and want["fmember_pos"].tolist() == [0, 60, 101]


# ---- 3. launch geometry, processes, streams ---------------------------------------------------------------
@pytest.mark.parametrize("grid", ("1", "2", "3"))
def test_launch_geometry(batches, grid, monkeypatch):
    """65, 257 and 769 joins over mixed motifs under 1, 2 and 3 workgroups per launch: a workgroup of the search takes many joins in turn"""
    monkeypatch.setenv("AIX_UG_TEST_GRID", grid)
    for J in (65, 257, 769):
        g, em, want = batches(J)
        _fill_all(_dev(g), g, em, GC.PARAMS, (grid, J), want=want)
        assert want["counts"][4] == J and (J < 257 or (want["counts"][:4] > 0).all())


_CHILD = """
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import gap_close_cases as GC
import test_gpu_gap_close as T
g = GC.make_batch(257, 257)
want, cl, lay = T._fill_all(T._dev(g), g, T._members(g), GC.PARAMS, "child")
print("DIGEST", T._digest(cl, T.CLOSE) + T._digest(lay, T.FILL[:6]))
"""


def test_a_fresh_process_agrees(batches, tmp_path):
    g, em, want = batches(257)
    script = tmp_path / "child.py"
    script.write_text(_CHILD)
    child = subprocess.run([sys.executable, str(script), ROOT], env=dict(os.environ, AIX_UG_TEST_GRID="2"), capture_output=True, text=True, timeout=300)
    assert child.returncode == 0, child.stderr[-2000:]
    assert [l.split()[1] for l in child.stdout.splitlines() if l.startswith("DIGEST")] == [_digest(want, CLOSE) + _digest(want, FILL[:6])]


def test_side_stream(batches):
    """Everything on a stream of its own, the null stream busy."""
    import torch
    g, em, want = batches(257)
    gt = _dev(g)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    busy = torch.empty(1 << 24, dtype=torch.float32, device="cuda")
    busy.normal_()
    with torch.cuda.stream(side):
        _fill_all(gt, g, em, GC.PARAMS, "side", stream=vp(side.cuda_stream), want=want)
    torch.cuda.synchronize()


# ---- 4. sizing and refusals -------------------------------------------------------------------------------
def test_path_sizing(batches):
    g, em, want = batches(65)
    gt = _dev(g)
    T = want["total"]
    assert T > 1
    for cap in (0, T - 1, T):
        cl = _raw_close(gt, GC.PARAMS, cap=cap)
        assert cl["status"] == 0 and cl["total"] == T and ("path" in cl) == (cap == T)
        _same(cl, want, [k for k in CLOSE if k != "path" or cap == T], cap)
    # no joins, and no contigs
    none = dict(g, join=np.full(2 * g["U"], NONE32, np.uint32), join_gap=np.zeros(2 * g["U"], np.int64))
    cl = _raw_close(_dev(none), GC.PARAMS)
    assert cl["status"] == 0 and cl["total"] == 0 and cl["counts"].tolist() == [0] * 5 and not cl["path_off"].any() and not cl["close_status"].any()
    empty = {"offsets": np.zeros(1, np.uint64), "link_off": np.zeros(1, np.uint64), "link_to": np.zeros(0, np.uint32), "join": np.zeros(0, np.uint32),
             "join_gap": np.zeros(0, np.int64), "bases": np.zeros(0, np.uint8)}
    cl = _raw_close(_dev(empty), GC.PARAMS)
    assert cl["status"] == 0 and cl["total"] == 0 and cl["counts"].tolist() == [0] * 5 and cl["path_off"].tolist() == [0]


def test_refusals_leave_the_outputs_untouched(batches):
    """Every malformed input comes back as AIX_ERR_ARG (the raw helpers assert that no output was touched)."""
    g, em, _ = batches(65)
    gt, U = _dev(g), g["U"]
    mt = {k: _t(em[k]) for k in ("member_off", "member")}
    cl = _raw_close(gt, GC.PARAMS)
    ct = cl["tensors"]
    lay = _raw_fill_layout(gt, mt, ct)
    assert cl["status"] == 0 and lay["status"] == 0
    both = lambda **o: (_raw_close(dict(gt, **o), GC.PARAMS)["status"], _raw_fill_layout(dict(gt, **o), mt, ct)["status"])
    rng = np.random.default_rng(5)
    for _ in range(3):                                                    # a random join
        assert both(join=_t(rng.integers(0, 2 * U, 2 * U).astype(np.uint32))) == (ARG, ARG)
    e = int(np.nonzero(g["join"] != NONE32)[0][0])
    t = int(g["join"][e])

    def poked(a, i, v):
        a = a.copy()
        a[i] = v
        return _t(a)
    assert both(join=poked(g["join"], e, NONE32)) == (ARG, ARG)           # a join without its dual
    assert both(join=poked(g["join"], e, e ^ 1)) == (ARG, ARG)            # within one contig
    assert both(join=poked(g["join"], e, 2 * U)) == (ARG, ARG)
    assert both(join_gap=poked(g["join_gap"], e, int(g["join_gap"][e]) + 1)) == (ARG, ARG)
    big = g["join_gap"].copy()
    big[[e, t ^ 1]] = (1 << 30) + 1
    assert both(join_gap=_t(big)) == (ARG, ARG)
    assert both(link_to=poked(g["link_to"], 3, 2 * U)) == (ARG, ARG)
    assert both(link_off=poked(g["link_off"], 5, g["E"] + 1)) == (ARG, ARG) and both(link_off=poked(g["link_off"], 0, 1)) == (ARG, ARG)
    assert both(link_off=poked(g["link_off"], 2 * U, g["E"] - 1)) == (ARG, ARG)
    short = g["offsets"].copy()
    short[3:] -= np.uint64(int(short[3] - short[2]) - 22)                  # a contig of 22 bases
    assert both(offsets=_t(short)) == (ARG, ARG)
    for o in (dict(tolerance=(1 << 20) + 1), dict(max_fill=65), dict(max_states=0), dict(max_states=4097)):
        assert _raw_close(gt, dict(GC.PARAMS, **o))["status"] == ARG
    # the closure handed to the layout
    owner = int(np.nonzero(np.diff(cl["path_off"].astype(np.int64)) > 0)[0][0])          # a closed join with a path
    q = int(cl["path_off"][owner])
    free = [x for x in range(2 * U) if g["join"][x] == NONE32]
    joined_contig = next(x for x in range(2 * U) if g["join"][x] != NONE32 and x >> 1 not in (owner >> 1, int(g["join"][owner]) >> 1))
    refused = lambda **o: _raw_fill_layout(gt, {k: o.pop(k, v) for k, v in mt.items()}, dict(ct, **o))["status"] == ARG
    dist = cl["close_dist"].view(np.int64)
    assert refused(path=poked(cl["path"], q, int(cl["path"][q]) ^ 1))     # a step that is no link
    assert refused(path=poked(cl["path"], q, 2 * U))
    assert refused(path=poked(cl["path"], q, joined_contig))              # a joined intermediate (and no link either)
    assert refused(close_dist=poked(dist, owner, int(dist[owner]) + 1)) and refused(close_dist=poked(dist, int(g["join"][owner]) ^ 1, int(dist[owner]) - 1))
    assert refused(close_status=poked(cl["close_status"], free[0], 2))    # a status on an unjoined end
    assert refused(close_status=poked(cl["close_status"], owner, 5)) and refused(close_status=poked(cl["close_status"], owner, 2))
    assert refused(path_off=poked(cl["path_off"], 2 * U, cl["total"] + 1)) and refused(path_off=poked(cl["path_off"], 0, 1))
    assert refused(member=poked(em["member"], 0, int(em["member"][1]))) and refused(member=poked(em["member"], 4, 2 * U))
    assert refused(member_off=poked(em["member_off"], 1, 0)) and refused(member=_t(em["member"][::-1]))
    # a joined intermediate that the links do allow: the case made for it, its status forged to closed
    g2, p2, _ = GC.case("joined_intermediate")
    gt2, em2 = _dev(g2), _members(g2)
    e2 = g2["probe"]
    t2 = int(g2["join"][e2])
    mid = int(g2["link_to"][int(g2["link_off"][e2])])
    st2, d2 = np.zeros(2 * g2["U"], np.uint8), np.zeros(2 * g2["U"], np.int64)
    other = [x for x in range(2 * g2["U"]) if g2["join"][x] != NONE32 and x not in (e2, t2 ^ 1)]
    st2[[e2, t2 ^ 1]], d2[[e2, t2 ^ 1]], st2[other] = 1, 16, 2
    po2 = np.zeros(2 * g2["U"] + 1, np.uint64)
    po2[e2 + 1:] = 1
    forged = {"close_status": _t(st2), "close_dist": _t(d2), "path_off": _t(po2), "path": _t(np.array([mid], np.uint32))}
    assert _raw_fill_layout(gt2, {k: _t(em2[k]) for k in ("member_off", "member")}, forged)["status"] == ARG
    # the filled arrays handed to the emit
    ft, Mf, total = lay["tensors"], lay["n_fmembers"], lay["total_bases"]
    assert _raw_fill_emit(gt, ft, Mf, total)["status"] == 0
    j = int(np.nonzero(lay["fmember_flag"] == 3)[0][0])
    for k, v in (("fmember_pos", int(lay["fmember_pos"][j]) + 1), ("fmember_flag", 2), ("fmember_flag", 0), ("fmember", 2 * U), ("fmember_off", 0)):
        assert _raw_fill_emit(gt, dict(ft, **{k: poked(lay[k], j if k != "fmember_off" else 1, v)}), Mf, total)["status"] == ARG, k
    assert _raw_fill_emit(gt, dict(ft, fscaffold_offsets=poked(lay["fscaffold_offsets"], 1, int(lay["fscaffold_offsets"][1]) + 1)), Mf, total)["status"] == ARG
    assert _raw_fill_emit(gt, ft, Mf, total + 1)["status"] == ARG and _raw_fill_emit(dict(gt, offsets=_t(short)), ft, Mf, total)["status"] == ARG


def test_host_form(batches, planted):
    g, em, _ = batches(65)
    want = _want(g, em, GC.PARAMS, min_gap=2)
    args = [g[k] for k in ("offsets", "bases", "link_off", "link_to", "join", "join_gap")] + [em["member_off"], em["member"]]
    prefix = planted("two_copy")[0]
    with Index.open_23(prefix + ".pf", prefix + ".tf.bin", prefix + ".kmers.bin") as ix:   # the host form takes no handle; the method lives on one
        host = ix.scaffold_fill(*args, **GC.PARAMS, min_gap=2)
        _same(host, want, CLOSE[:6] + FILL, "host")
        assert (host["counts"], host["total"], host["n_fmembers"], host["total_bases"]) == (want["counts"].tolist(), want["total"], want["n_fmembers"], want["total_bases"])
        args[3] = g["link_to"] + np.uint32(2 * g["U"])
        with pytest.raises(_lib.AixError):
            ix.scaffold_fill(*args)
