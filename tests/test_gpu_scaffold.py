"""Scaffolding on the GPU (k_sc_* of aix_scaffold.hip) against the test-side restatement (tests/scaffold_ref.py, pinned by
test_scaffold_cpu.py) on the inputs of tests/scaffold_cases.py. Every comparison is exact equality; every raw call has 64 poisoned
elements behind every output."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import debruijn_ref as D
import graph_clean_ref as GR
import oracle_lib as O
import scaffold_cases as SC
import scaffold_ref as SF
import seqthread_ref as SR
import unitig_links_ref as RL
import unitigs_ref as R
from aindex_amd import _lib, builder
from aindex_amd.engine import Index

vp = _lib.vp
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P64, P32, P8 = 0x6B6B6B6B6B6B6B6B, 0x6B6B6B6B, 0x6B
_UNSIGNED = {np.dtype(np.int64): np.uint64, np.dtype(np.int32): np.uint32}
_SIGNED = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}
ARG = _lib.AIX_ERR_ARG
SLINK = ("slink_off", "slink_to", "slink_count", "slink_dsum")
JOIN = ("join", "join_count", "join_gap")
MAP = ("contig_scaffold", "contig_rank", "contig_pos", "contig_flag")
EMIT = ("scaffold_offsets", "scaffold_bases", "member_off", "member", "member_gap")
STEP = ("seq_step_off", "step_unitig", "step_pos", "step_flag", "q_first", "q_last")
MAX_INSERT = 1000


def _np(t, signed=False):
    a = t.cpu().numpy()
    return a if signed else a.view(_UNSIGNED.get(a.dtype, a.dtype))


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


def _open(prefix):
    return Index.open_23(prefix + ".pf", prefix + ".tf.bin", prefix + ".kmers.bin")


def _sync():
    import torch
    torch.cuda.synchronize()


# ---- the raw calls, every output dirty and followed by poison ---------------------------------------------
def _raw_links(offsets, circular, steps, offs, hist, maw=1, mi=MAX_INSERT, stream=None, **over):
    """aix_mate_links_dev -> (status, obs_key, obs_d, counts); hist is accumulated in place. steps / offs: device tensors"""
    import torch
    P = (offs.numel() - 1) // 2
    key, d, counts = _poisoned(P, torch.int64), _poisoned(P, torch.int32), _poisoned(4, torch.int64)
    a = dict(P=P, offs=offs, sso=steps[0], T=steps[1].numel(), su=steps[1], sp=steps[2], sf=steps[3], qf=steps[4], ql=steps[5], U=offsets.numel() - 1, off=offsets,
             circ=circular, maw=maw, mi=mi, hist=hist, key=key, d=d, counts=counts)
    a.update(over)
    st = _lib.lib().aix_mate_links_dev(*[(_q(v) if hasattr(v, "data_ptr") else v) for v in a.values()], stream)
    _sync()
    if st:
        assert _intact(key) and _intact(d) and _intact(counts)
        return st, None, None, None
    assert _intact(key, P) and _intact(d, P) and _intact(counts, 4)
    return 0, _np(key[:P]), _np(d[:P]), _np(counts[:4])


def _raw_bundle(key, d, U, cap=None, stream=None):
    """aix_mate_bundle_dev -> (status, S, dict); cap None: sized first, then filled at exactly S"""
    import torch
    L = _lib.lib()
    N = key.numel()
    total = C.c_uint64(77)
    if cap is None:
        off = _poisoned(2 * U + 1, torch.int64)
        st = L.aix_mate_bundle_dev(N, _q(key), _q(d), U, _q(off), None, None, None, 0, C.byref(total), stream)
        _sync()
        if st:
            assert _intact(off) and total.value == 77
            return st, None, None
        cap = total.value
    off = _poisoned(2 * U + 1, torch.int64)
    outs = [_poisoned(cap, dt) for dt in (torch.int32, torch.int64, torch.int64)]
    st = L.aix_mate_bundle_dev(N, _q(key), _q(d), U, _q(off), *[_q(o) for o in outs], cap, C.byref(total), stream)
    _sync()
    if st:
        assert _intact(off) and all(_intact(o) for o in outs)
        return st, None, None
    S = total.value
    assert _intact(off, 2 * U + 1) and all(_intact(o, cap if S <= cap else 0) for o in outs)
    res = {"slink_off": _np(off[:2 * U + 1]), "S": S}
    if S <= cap:
        res.update({k: _np(o[:S]) for k, o in zip(SLINK[1:], outs)})
    return 0, S, res


def _raw_mark(gt, sl, par, stream=None):
    """aix_scaffold_mark_dev -> dict (status alone on a refusal)"""
    import torch
    U, S = gt["offsets"].numel() - 1, sl["slink_to"].numel()
    outs = [_poisoned(2 * U, dt) for dt in (torch.int32, torch.int64, torch.int64)]
    n = C.c_uint64(77)
    st = _lib.lib().aix_scaffold_mark_dev(U, _q(gt["offsets"]), _q(gt["circular"]), *[_q(sl[k]) for k in SLINK], S, par["insert_size"], par["min_pairs"], par["dominance"],
                                          par["min_contig_bases"], *[_q(o) for o in outs], C.byref(n), stream)
    _sync()
    if st:
        assert all(_intact(o) for o in outs) and n.value == 77
        return {"status": st}
    assert all(_intact(o, 2 * U) for o in outs)
    return {"status": 0, "join": _np(outs[0][:2 * U]), "join_count": _np(outs[1][:2 * U]), "join_gap": _np(outs[2][:2 * U], signed=True), "n_joins": n.value,
            "tensors": {k: o[:2 * U] for k, o in zip(JOIN, outs)}}


def _raw_layout(offsets, jt, min_gap=1, stream=None):
    import torch
    U = offsets.numel() - 1
    outs = [_poisoned(U, dt) for dt in (torch.int32, torch.int32, torch.int64, torch.uint8)]
    n = [C.c_uint64(77) for _ in range(3)]
    st = _lib.lib().aix_scaffold_layout_dev(U, _q(offsets), *[_q(jt[k]) for k in JOIN], min_gap, *[_q(o) for o in outs], *[C.byref(x) for x in n], stream)
    _sync()
    if st:
        assert all(_intact(o) for o in outs) and all(x.value == 77 for x in n)
        return {"status": st}
    assert all(_intact(o, U) for o in outs)
    res = {k: _np(o[:U]) for k, o in zip(MAP, outs)}
    res.update(status=0, n_scaffolds=n[0].value, total_bases=n[1].value, n_cut=n[2].value, tensors={k: o[:U] for k, o in zip(MAP, outs)})
    return res


def _raw_emit(gt, jt, mt, Sc, total, min_gap=1, stream=None):
    import torch
    U = gt["offsets"].numel() - 1
    sizes = (Sc + 1, total, Sc + 1, U, U)
    outs = [_poisoned(s, dt) for s, dt in zip(sizes, (torch.int64, torch.uint8, torch.int64, torch.int32, torch.int64))]
    st = _lib.lib().aix_scaffold_emit_dev(U, _q(gt["offsets"]), _q(gt["bases"]), _q(jt["join"]), _q(jt["join_gap"]), min_gap, *[_q(mt[k]) for k in MAP], Sc, total,
                                          *[_q(o) for o in outs], stream)
    _sync()
    if st:
        assert all(_intact(o) for o in outs)
        return {"status": st}
    assert all(_intact(o, s) for o, s in zip(outs, sizes))
    res = {k: _np(o[:s], signed=(k == "member_gap")) for k, o, s in zip(EMIT, outs, sizes)}
    res["status"] = 0
    return res


def _same(got, want, keys, tag):
    for k in keys:
        g = got[k].cpu().numpy() if hasattr(got[k], "cpu") else got[k]
        g = g.view(want[k].dtype) if g.dtype != want[k].dtype and g.dtype.itemsize == want[k].dtype.itemsize else g
        assert g.dtype == want[k].dtype and np.array_equal(g, want[k]), (tag, k)


def _scaffold_all(gt, g, key_t, d_t, key, d, par, tag, min_gap=1, stream=None):
    """bundle, mark, layout and emit, raw, against the restatement -> (want, raw results)"""
    U = g["U"] if "U" in g else len(g["circular"])
    want = SF.scaffold(g["offsets"], g["bases"], g["circular"], key, d, par["insert_size"], par["min_pairs"], par["dominance"], par["min_contig_bases"], min_gap)
    st, S, sl = _raw_bundle(key_t, d_t, U, stream=stream)
    assert st == 0 and S == want["S"]
    _same(sl, want, SLINK, (tag, "bundle"))
    mk = _raw_mark(gt, {k: _t(want[k]) for k in SLINK}, par, stream)
    assert mk["status"] == 0 and mk["n_joins"] == want["n_joins"]
    _same(mk, want, JOIN, (tag, "mark"))
    lay = _raw_layout(gt["offsets"], mk["tensors"], min_gap, stream)
    assert lay["status"] == 0 and (lay["n_scaffolds"], lay["total_bases"], lay["n_cut"]) == (want["n_scaffolds"], want["total_bases"], want["n_cut"]), tag
    _same(lay, want, MAP, (tag, "layout"))
    em = _raw_emit(gt, mk["tensors"], lay["tensors"], lay["n_scaffolds"], lay["total_bases"], min_gap, stream)
    assert em["status"] == 0
    _same(em, want, EMIT, (tag, "emit"))
    return want, mk, lay, em


def _digest(res, keys):
    h = hashlib.sha256()
    for k in keys:
        h.update(np.ascontiguousarray(res[k]).tobytes())
    return h.hexdigest()


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("sc"))
    made = {}

    def get(name):
        if name not in made:
            p = SC.planted(name)
            made[name] = (_write_index(os.path.join(d, name), p.codes, p.tfs), p)
        return made[name]
    return get


def _ref_graph(ix):
    codes, tfs = ix.checker_array() & np.uint64(R.MASK), ix.tf_array()
    un = R.unitigs(codes, tfs, 0)
    lk = RL.links(codes, tfs, 0, un)
    node = SR.nodes(un["kid_unitig"], un["kid_pos"], un["kid_flag"], un["offsets"])
    return GR.graph(un, lk), {int(c): i for i, c in enumerate(codes.tolist())}, node


@pytest.mark.parametrize("name", SC.PLANTED)
def test_planted_cases(planted, name):
    """1. Every planted case end to end through thread_graph_t and seq_thread_t: observations (two batches onto a prefilled histogram),
    the four raw calls, the engine methods and the host form, all equal to the restatement; the scaffolds are the planted genomes."""
    import torch
    prefix, p = planted(name)
    par = dict(insert_size=p.insert, min_pairs=2, dominance=2, min_contig_bases=SC.MIN_BASES)
    with _open(prefix) as ix:
        g, kid_of, node = _ref_graph(ix)
        seqs = SC.mates(p.pairs)
        steps_w = SR.thread(kid_of, node, g, seqs)
        offs_w = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
        key_w, d_w, counts_w, hist_w = SF.mate_links(offs_w, steps_w, g["offsets"], g["circular"], 1, MAX_INSERT)
        graph = ix.thread_graph_t(0)
        data_t, offs_t = _dev_seqs(seqs)
        steps = ix.seq_thread_t(graph, data_t, offs_t)
        _same(dict(zip(STEP, steps)), steps_w, STEP, (name, "steps"))
        key, d, counts, hist = ix.mate_links_t(graph, steps, offs_t, 1, MAX_INSERT)
        assert np.array_equal(_np(key), key_w) and np.array_equal(_np(d), d_w) and np.array_equal(_np(counts), counts_w) and np.array_equal(_np(hist), hist_w), name
        assert ix.insert_size_t(hist) == p.insert == SF.insert_size(hist_w)
        # two batches onto a prefilled pattern, raw
        half = 2 * (len(p.pairs) // 2)
        acc = _poisoned(MAX_INSERT + 1, torch.int64)
        pattern = torch.arange(MAX_INSERT + 1, dtype=torch.int64, device="cuda") * 3 + 1
        acc[:MAX_INSERT + 1] = pattern
        parts = []
        for part in (seqs[:half], seqs[half:]):
            dt, ot = _dev_seqs(part)
            st, k, x, c = _raw_links(graph["offsets"], graph["circular"], ix.seq_thread_t(graph, dt, ot), ot, acc)
            assert st == 0
            parts.append((k, x, c))
        assert _intact(acc, MAX_INSERT + 1) and np.array_equal(_np(acc[:MAX_INSERT + 1]), _np(pattern) + hist_w)
        assert np.array_equal(np.concatenate([parts[0][0], parts[1][0]]), key_w) and np.array_equal(np.concatenate([parts[0][1], parts[1][1]]), d_w)
        assert np.array_equal(parts[0][2] + parts[1][2], counts_w)
        want, mk, lay, em = _scaffold_all(graph, g, key, d, key_w, d_w, par, name)
        assert sorted(np.diff(want["member_off"].astype(np.int64)).tolist()) == p.sizes and want["n_cut"] == p.n_cut
        # the engine methods and the host form
        sl = ix.mate_bundle_t(key, d, g["U"])
        _same(sl, want, SLINK, (name, "engine bundle"))
        jn = ix.scaffold_mark_t(graph, sl, **par)
        _same(jn, want, JOIN, (name, "engine mark"))
        sc = ix.scaffold_t(graph, jn, 1)
        _same(sc, want, MAP + EMIT, (name, "engine scaffold"))
        assert (sc["n_scaffolds"], sc["total_bases"], sc["n_cut"], jn["n_joins"], sl["S"]) == tuple(want[k] for k in ("n_scaffolds", "total_bases", "n_cut", "n_joins", "S"))
        host = ix.scaffold(g["offsets"], g["bases"], g["circular"], key_w, d_w, **par, min_gap=1)
        _same(host, want, JOIN + MAP + EMIT, (name, "host"))
        assert (host["n_scaffolds"], host["n_joins"], host["n_cut"], host["S"]) == (want["n_scaffolds"], want["n_joins"], want["n_cut"], want["S"])
    _sync()


@pytest.fixture(scope="module")
def structures():
    return {seed: SC.make_scaffold_graph(seed) for seed in (0, 1)}


@pytest.mark.parametrize("seed", (0, 1))
def test_scaffold_graph_structures(planted, structures, seed):
    """2. The hand-set structures: thresholds, 128-bit dominance, long lists, chains and cycles, every gap kind; bundle caps; refusals
    that leave every output untouched."""
    import torch
    g = structures[seed]
    U, par = g["U"], g["params"]
    gt = {k: _t(g[k]) for k in ("offsets", "bases", "circular")}
    key_t, d_t = _t(g["obs_key"]), _t(g["obs_d"])
    _scaffold_all(gt, g, key_t, d_t, g["obs_key"], g["obs_d"], par, (seed, "obs"))
    S = g["obs_slinks"]["S"]
    for cap in (0, S - 1, S):                                             # sizing: the entries only when they fit
        st, total, res = _raw_bundle(key_t, d_t, U, cap=cap)
        assert st == 0 and total == S and np.array_equal(res["slink_off"], g["obs_slinks"]["slink_off"]) and ("slink_to" in res) == (cap == S)
    st, total, res = _raw_bundle(key_t[:0], d_t[:0], U, cap=4)
    assert st == 0 and total == 0 and not res["slink_off"].any()
    # the full link set (counts no observation list could hold), two settings
    slt = {k: _t(g[k]) for k in SLINK}
    for p2 in (par, dict(par, min_contig_bases=0), dict(par, dominance=1, min_pairs=1)):
        want = SF.mark(g["offsets"], g["circular"], g, **p2)
        mk = _raw_mark(gt, slt, p2)
        assert mk["status"] == 0 and mk["n_joins"] == want["n_joins"]
        _same(mk, want, JOIN, (seed, "mark", p2["min_contig_bases"]))
        for min_gap in (1, 9):
            wl = SF.layout(g["offsets"], want["join"], want["join_count"], want["join_gap"], min_gap)
            lay = _raw_layout(gt["offsets"], mk["tensors"], min_gap)
            assert lay["status"] == 0 and (lay["n_scaffolds"], lay["total_bases"], lay["n_cut"]) == (wl["n_scaffolds"], wl["total_bases"], wl["n_cut"])
            _same(lay, wl, MAP, (seed, "layout", min_gap))
            we = SF.emit(g["offsets"], g["bases"], want["join"], want["join_gap"], wl, min_gap)
            em = _raw_emit(gt, mk["tensors"], lay["tensors"], lay["n_scaffolds"], lay["total_bases"], min_gap)
            assert em["status"] == 0
            _same(em, we, EMIT, (seed, "emit", min_gap))
    mk = _raw_mark(gt, slt, par)
    lay = _raw_layout(gt["offsets"], mk["tensors"])
    assert lay["n_cut"] == 5
    with _open(planted("two_copy")[0]) as ix:                              # the host form takes no handle; the method lives on one
        host = ix.scaffold(g["offsets"], g["bases"], g["circular"], g["obs_key"], g["obs_d"], **par, min_gap=1)
    _same(host, SF.scaffold(g["offsets"], g["bases"], g["circular"], g["obs_key"], g["obs_d"], **par, min_gap=1), JOIN + MAP + EMIT, (seed, "host"))
    # refusals
    bad = g["slink_count"].copy()
    bad[0] += np.uint64(1)
    assert _raw_mark(gt, dict(slt, slink_count=_t(bad)), par)["status"] == ARG            # a link without an equal dual
    bad = g["slink_to"].copy()
    bad[3] = 2 * U
    assert _raw_mark(gt, dict(slt, slink_to=_t(bad)), par)["status"] == ARG
    bad = g["slink_off"].copy()
    bad[5] = g["S"] + 1
    assert _raw_mark(gt, dict(slt, slink_off=_t(bad)), par)["status"] == ARG
    keys = g["obs_key"].copy()
    live = int(np.nonzero(keys != SF.NOKEY)[0][0])
    keys[live] = ((int(keys[live]) & SF.M32) ^ 1) << 32 | ((int(keys[live]) >> 32) ^ 1)   # the dual of a canonical key
    assert _raw_bundle(_t(keys), d_t, U)[0] == ARG
    dd = g["obs_d"].copy()
    dd[live] = 0
    assert _raw_bundle(key_t, _t(dd), U)[0] == ARG
    jt = dict(mk["tensors"])
    e = g["want_join"][0][0]
    cut = mk["join"].copy()
    cut[e] = SF.NONE32
    assert _raw_layout(gt["offsets"], dict(jt, join=_t(cut)))["status"] == ARG             # a join without its dual
    assert _raw_emit(gt, dict(jt, join=_t(cut)), lay["tensors"], lay["n_scaffolds"], lay["total_bases"])["status"] == ARG
    rng = np.random.default_rng(seed)
    for _ in range(3):                                                    # random join arrays handed to emit
        rj = rng.integers(0, 2 * U, 2 * U).astype(np.uint32)
        assert _raw_emit(gt, dict(jt, join=_t(rj)), lay["tensors"], lay["n_scaffolds"], lay["total_bases"])["status"] == ARG
    none = _t(np.full(2 * U, SF.NONE32, np.uint32))                          # a map that claims joins the join array does not hold
    assert _raw_emit(gt, dict(jt, join=none, join_gap=_t(np.zeros(2 * U, np.int64))), lay["tensors"], lay["n_scaffolds"], lay["total_bases"])["status"] == ARG
    for k in MAP:                                                         # one entry of the map off by one
        a = lay[k].copy()
        a[g["chains"]["chain65"][3]] ^= 1
        assert _raw_emit(gt, jt, dict(lay["tensors"], **{k: _t(a)}), lay["n_scaffolds"], lay["total_bases"])["status"] == ARG, k
    assert _raw_emit(gt, jt, lay["tensors"], lay["n_scaffolds"], lay["total_bases"] + 1)["status"] == ARG
    assert _raw_emit(gt, jt, lay["tensors"], lay["n_scaffolds"] - 1, lay["total_bases"])["status"] == ARG


def _batch_case(g, P, seed=0):
    offs, steps = SC.make_pair_batch(seed, P, g["offsets"])
    return offs, steps, SF.mate_links(offs, steps, g["offsets"], g["circular"], 2, 150)


@pytest.mark.parametrize("grid", ("1", "2", "3"))
def test_launch_geometry(structures, grid, monkeypatch):
    """3. 1, 2 and 3 workgroups per launch: P of 65, 257 and 3 * 256 + 1 hand-set pairs, and the structures (2 U ends make several trips)."""
    monkeypatch.setenv("AIX_UG_TEST_GRID", grid)
    g = structures[0]
    gt = {k: _t(g[k]) for k in ("offsets", "bases", "circular")}
    for P in (65, 257, 3 * 256 + 1):
        import torch
        offs, steps, (key_w, d_w, counts_w, hist_w) = _batch_case(g, P)
        hist = torch.zeros(151, dtype=torch.int64, device="cuda")
        st, key, d, counts = _raw_links(gt["offsets"], gt["circular"], [_t(steps[k]) for k in STEP], _t(offs), hist, maw=2, mi=150)
        assert st == 0 and np.array_equal(key, key_w) and np.array_equal(d, d_w) and np.array_equal(counts, counts_w) and np.array_equal(_np(hist), hist_w), P
        assert counts_w.min() > 0                                         # every kind of pair occurs
        st, S, sl = _raw_bundle(_t(key_w), _t(d_w), g["U"])
        assert st == 0
        _same(sl, SF.bundle(key_w, d_w, g["U"]), SLINK, (grid, P))
    for U in (65, 257, 3 * 256 + 1):                                      # the same sizes as contigs: chains and cycles in random id order
        c = SC.make_chains(U, U)
        ct = {k: _t(c[k]) for k in ("offsets", "bases", "circular")}
        wm = SF.mark(c["offsets"], c["circular"], c, **c["params"])
        mk = _raw_mark(ct, {k: _t(c[k]) for k in SLINK}, c["params"])
        assert mk["status"] == 0 and mk["n_joins"] == wm["n_joins"] > 0
        _same(mk, wm, JOIN, (grid, U))
        wl = SF.layout(c["offsets"], wm["join"], wm["join_count"], wm["join_gap"])
        lay = _raw_layout(ct["offsets"], mk["tensors"])
        assert lay["status"] == 0 and (lay["n_scaffolds"], lay["total_bases"], lay["n_cut"]) == (wl["n_scaffolds"], wl["total_bases"], wl["n_cut"]) and wl["n_cut"] > 0
        _same(lay, wl, MAP, (grid, U))
        em = _raw_emit(ct, mk["tensors"], lay["tensors"], lay["n_scaffolds"], lay["total_bases"])
        assert em["status"] == 0
        _same(em, SF.emit(c["offsets"], c["bases"], wm["join"], wm["join_gap"], wl), EMIT, (grid, U))
    _scaffold_all(gt, g, _t(g["obs_key"]), _t(g["obs_d"]), g["obs_key"], g["obs_d"], g["params"], ("grid", grid))
    want = SF.mark(g["offsets"], g["circular"], g, **g["params"])
    mk = _raw_mark(gt, {k: _t(g[k]) for k in SLINK}, g["params"])
    _same(mk, want, JOIN, ("grid", grid))
    lay = _raw_layout(gt["offsets"], mk["tensors"])
    _same(lay, SF.layout(g["offsets"], want["join"], want["join_count"], want["join_gap"]), MAP, ("grid", grid))


def test_refusals_of_mate_links(structures):
    """4. Every violation of the step arrays is refused with the outputs and the histogram untouched; P == 0."""
    import torch
    g = structures[0]
    off_t, circ_t = _t(g["offsets"]), _t(g["circular"])
    offs, steps, _ = _batch_case(g, 65)
    st_t = {k: _t(steps[k]) for k in STEP}
    hist = _poisoned(151, torch.int64)

    def refused(**change):
        s = dict(st_t)
        o = change.pop("offs", offs)
        for k, v in change.items():
            s[k] = _t(v)
        st = _raw_links(off_t, circ_t, [s[k] for k in STEP], _t(o), hist, maw=2, mi=150)[0]
        return st == ARG and _intact(hist)

    def bumped(k, i, v):
        a = steps[k].copy()
        a[i] = v
        return {k: a}

    T = steps["step_unitig"].shape[0]
    u0 = int(steps["step_unitig"][0])
    assert refused(**bumped("step_unitig", T - 1, g["U"]))
    assert refused(**bumped("step_pos", 0, int(g["offsets"][u0 + 1] - g["offsets"][u0]) - 22))
    assert refused(**bumped("q_first", 1, int(steps["q_last"][1]) + 1))
    assert refused(**bumped("seq_step_off", 130, T + 1)) and refused(**bumped("seq_step_off", 0, 1)) and refused(**bumped("seq_step_off", 7, int(steps["seq_step_off"][9]) + 1))
    o = offs.copy()
    o[5] = o[7]
    assert refused(offs=o)
    short = g["offsets"].copy()
    short[3:] -= np.uint64(int(short[3] - short[2]) - 22)                  # a contig of 22 bases
    assert _raw_links(_t(short), circ_t, [st_t[k] for k in STEP], _t(offs), hist, maw=2, mi=150)[0] == ARG and _intact(hist)
    empty = [_t(np.zeros(1, np.uint64))] + [_t(steps[k][:0]) for k in STEP[1:]]
    st, key, d, counts = _raw_links(off_t, circ_t, empty, _t(np.zeros(1, np.uint64)), hist, maw=2, mi=150)
    assert st == 0 and counts.tolist() == [0, 0, 0, 0] and _intact(hist)
    with pytest.raises(ValueError):                                       # no pair within one contig: the caller passes insert_size itself
        Index.insert_size_t(torch.zeros(151, dtype=torch.int64, device="cuda"))
    one = torch.zeros(151, dtype=torch.int64, device="cuda")
    one[[7, 9, 140]] = torch.tensor([2, 1, 1], device="cuda")
    assert Index.insert_size_t(one) == 7 == SF.insert_size(_np(one))       # the lower median of {7, 7, 9, 140}


def test_a_mate_that_ends_before_its_contig_is_discordant(structures):
    """4b. Hand-set steps whose q_first lies beyond the mate: d far below 0 and d == 0 are discordant, d == 1 is an observation."""
    import torch
    g = structures[0]
    offs, steps, (u, v) = SC.make_pairs_before_contig(g["offsets"], g["circular"])
    key_w, d_w, counts_w, hist_w = SF.mate_links(offs, steps, g["offsets"], g["circular"], 1, 150)
    assert counts_w.tolist() == [0, 1, 2, 0] and d_w.tolist() == [0, 0, 1]
    hist = torch.zeros(151, dtype=torch.int64, device="cuda")
    st, key, d, counts = _raw_links(_t(g["offsets"]), _t(g["circular"]), [_t(steps[k]) for k in STEP], _t(offs), hist, maw=1, mi=150)
    assert st == 0 and np.array_equal(key, key_w) and np.array_equal(d, d_w) and np.array_equal(counts, counts_w) and np.array_equal(_np(hist), hist_w)


def test_side_stream(structures):
    """5. Everything on a stream of its own, the null stream busy."""
    import torch
    g = structures[1]
    gt = {k: _t(g[k]) for k in ("offsets", "bases", "circular")}
    key_t, d_t = _t(g["obs_key"]), _t(g["obs_d"])
    offs, steps, (key_w, d_w, counts_w, hist_w) = _batch_case(g, 257, seed=1)
    st_t, offs_t = [_t(steps[k]) for k in STEP], _t(offs)
    hist = torch.zeros(151, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    busy = torch.empty(1 << 24, dtype=torch.float32, device="cuda")
    busy.normal_()
    with torch.cuda.stream(side):
        ptr = vp(side.cuda_stream)
        st, key, d, counts = _raw_links(gt["offsets"], gt["circular"], st_t, offs_t, hist, maw=2, mi=150, stream=ptr)
        assert st == 0 and np.array_equal(key, key_w) and np.array_equal(d, d_w) and np.array_equal(counts, counts_w) and np.array_equal(_np(hist), hist_w)
        _scaffold_all(gt, g, key_t, d_t, g["obs_key"], g["obs_d"], g["params"], "side", stream=ptr)
    torch.cuda.synchronize()


def test_list_surface(planted, tmp_path):
    """7. get_scaffolds, write_scaffolds and write_scaffolds_agp: the restatement's scaffolds, in one batch and in several."""
    from aindex_amd.aindex import AIndex
    prefix, p = planted("chain3")
    a = AIndex.load_23mer_index(prefix + ".pf", prefix + ".tf.bin", prefix + ".kmers.bin")
    try:
        with _open(prefix) as ix:
            g, kid_of, node = _ref_graph(ix)
        seqs = SC.mates(p.pairs)
        offs_w = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
        key_w, d_w, _, hist_w = SF.mate_links(offs_w, SR.thread(kid_of, node, g, seqs), g["offsets"], g["circular"], 1, MAX_INSERT)
        want = SF.scaffold(g["offsets"], g["bases"], g["circular"], key_w, d_w, p.insert, 2, 2, SC.MIN_BASES, 1)
        text, so, mo = want["scaffold_bases"].tobytes().decode(), want["scaffold_offsets"].tolist(), want["member_off"].tolist()
        expect = [(text[so[i]:so[i + 1]], [(int(w) >> 1, "+-"[int(w) & 1], int(x)) for w, x in zip(want["member"][mo[i]:mo[i + 1]], want["member_gap"][mo[i]:mo[i + 1]])])
                  for i in range(want["n_scaffolds"])]
        kw = dict(min_contig_bases=SC.MIN_BASES, rounds=0)
        got = a.get_scaffolds(p.pairs, **kw)                                # insert_size: the median of the histogram
        assert got == expect and sorted(len(m) for _, m in got) == p.sizes
        lines = [x + b"~" + y for x, y in p.pairs]
        a.RESOLVE_BATCH_BYTES = 3000                                        # several batches, the observations concatenated
        assert a.get_scaffolds(lines, insert_size=p.insert, **kw) == expect
        out = str(tmp_path / "s.fa")
        assert a.write_scaffolds(out, p.pairs, **kw) == len(expect)
        fa = open(out).read().splitlines()
        assert fa[1::2] == [s for s, _ in expect] and fa[0].split()[:2] == [">s0", "LN:i:%d" % len(expect[0][0])]
        out = str(tmp_path / "s.agp")
        n = a.write_scaffolds_agp(out, p.pairs, **kw)
        with pytest.raises(TypeError):
            a.write_scaffolds_agp(out, p.pairs, min_contigs=3)              # the arguments are get_scaffolds's, no others
        agp = [l.split("\t") for l in open(out).read().splitlines() if not l.startswith("#")]
        assert n == len(agp) == sum(2 * len(m) - 1 for _, m in expect)
        for i, (s, members) in enumerate(expect):
            rows = [r for r in agp if r[0] == "s%d" % i]
            assert int(rows[-1][2]) == len(s) and [r[3] for r in rows] == [str(j + 1) for j in range(len(rows))]
            assert [(int(r[5][1:]), r[8]) for r in rows if r[4] == "W"] == [(u, o) for u, o, _ in members]
            assert [int(r[5]) for r in rows if r[4] == "N"] == [max(x, 1) for _, _, x in members[1:]]
            assert all(s[int(r[1]) - 1:int(r[2])] == "N" * int(r[5]) for r in rows if r[4] == "N")
    finally:
        a._wrapper.close()


def test_mates_thread_through_resolved_contigs(tmp_path):
    """8. resolve=True on the planted two-copy repeat of graph_resolve_cases: the k-mers of the split unitig are dead in the map, so
    every step of every read lies where the resolved contig's bases say, and no step is broken."""
    import graph_resolve_cases as RC
    from aindex_amd.aindex import AIndex
    p = RC.planted("two_copy")
    prefix = _write_index(str(tmp_path / "two_copy"), p.codes, p.tfs)
    a = AIndex.load_23mer_index(prefix + ".pf", prefix + ".tf.bin", prefix + ".kmers.bin")
    try:
        pairs = [(p.reads[i], p.reads[i + 1]) for i in range(0, len(p.reads) - 1, 2)]
        graph = a.scaffold_graph(pairs, rounds=0, resolve=True)
        assert graph["U"] == 2 and graph["E"] == 0
        lines = a.scaffold_graph([x + b"~" + y for x, y in pairs] + [b"single"], rounds=0, resolve=True)   # pairs as get_scaffolds takes them
        assert all(np.array_equal(_np(lines[k]), _np(graph[k])) for k in ("offsets", "bases", "node"))
        ix = a._wrapper._need23()
        steps = [_np(t) for t in ix.seq_thread_t(graph, *_dev_seqs(p.reads))]
        sso, su, sp, sf, qf, ql, link = steps
        off, text = _np(graph["offsets"]).tolist(), _np(graph["bases"]).tobytes()
        assert int(sso[-1]) >= len(p.reads) and not (link == np.uint64(SR.BROKEN)).any()
        gaps = 0
        for i, r in enumerate(p.reads):
            lo, hi = int(sso[i]), int(sso[i + 1])
            gaps += hi - lo > 1                                             # the split repeat: a gap in the read's path, no link
            for j in range(lo, hi):
                u, pos, s, q0, q1 = int(su[j]), int(sp[j]), int(sf[j]) & 1, int(qf[j]), int(ql[j])
                n = q1 - q0 + 23
                piece = text[off[u] + pos:off[u] + pos + n] if not s else SF.rc_bytes(text[off[u] + pos - (q1 - q0):off[u] + pos + 23])
                assert piece == r[q0:q0 + n], (i, j)
        assert gaps > 0
        got = a.get_scaffolds(pairs, insert_size=150, rounds=0, resolve=True)   # nothing to join: the two resolved contigs
        assert sorted(RC.canon_str(s) for s, _ in got) == p.contigs
    finally:
        a._wrapper.close()


_CHILD = """
import hashlib, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import torch
import scaffold_cases as SC
import test_gpu_scaffold as T
g = SC.make_scaffold_graph(0)
gt = {k: T._t(g[k]) for k in ("offsets", "bases", "circular")}
st, S, sl = T._raw_bundle(T._t(g["obs_key"]), T._t(g["obs_d"]), g["U"])
mk = T._raw_mark(gt, {k: T._t(g[k]) for k in T.SLINK}, g["params"])
lay = T._raw_layout(gt["offsets"], mk["tensors"])
em = T._raw_emit(gt, mk["tensors"], lay["tensors"], lay["n_scaffolds"], lay["total_bases"])
offs, steps = SC.make_pair_batch(0, 769, g["offsets"])
hist = torch.zeros(151, dtype=torch.int64, device="cuda")
ml = T._raw_links(gt["offsets"], gt["circular"], [T._t(steps[k]) for k in T.STEP], T._t(offs), hist, maw=2, mi=150)
assert st == 0 and mk["status"] == 0 and lay["status"] == 0 and em["status"] == 0 and ml[0] == 0
print("DIGEST", T._digest(sl, T.SLINK) + T._digest(mk, T.JOIN) + T._digest(lay, T.MAP) + T._digest(em, T.EMIT) +
      T._digest({"k": ml[1], "d": ml[2], "c": ml[3], "h": T._np(hist)}, ("k", "d", "c", "h")))
"""


def test_fresh_processes_agree(structures, tmp_path):
    """6. The same calls in fresh child processes under 1, 2 and 3 workgroups: one digest, the restatement's."""
    g = structures[0]
    want = SF.scaffold(g["offsets"], g["bases"], g["circular"], g["obs_key"], g["obs_d"], **g["params"], min_gap=1)
    wm = SF.mark(g["offsets"], g["circular"], g, **g["params"])
    wl = SF.layout(g["offsets"], wm["join"], wm["join_count"], wm["join_gap"])
    we = SF.emit(g["offsets"], g["bases"], wm["join"], wm["join_gap"], wl)
    offs, steps, (key_w, d_w, counts_w, hist_w) = _batch_case(g, 769)
    expect = _digest(want, SLINK) + _digest(wm, JOIN) + _digest(wl, MAP) + _digest(we, EMIT) + _digest({"k": key_w, "d": d_w, "c": counts_w, "h": hist_w}, ("k", "d", "c", "h"))
    script = tmp_path / "child.py"
    script.write_text(_CHILD)
    children = []
    for grid in ("1", "2", "3"):                                          # side by side: the start of a process is most of its time
        env = dict(os.environ, AIX_UG_TEST_GRID=grid)
        children.append((grid, subprocess.Popen([sys.executable, str(script), ROOT], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)))
    for grid, child in children:
        out, err = child.communicate(timeout=300)
        assert child.returncode == 0, err[-2000:]
        assert [l.split()[1] for l in out.splitlines() if l.startswith("DIGEST")] == [expect], grid
