"""The phasing on the GPU (k_ph_* of aix_phase.hip) against the test-side restatement (tests/phase_ref.py, pinned by test_phase_cpu.py) on
the planted case, graph cases with their own reads, and hand-made arrays. Every comparison is exact equality."""
import ctypes as C
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import debruijn_ref as D
import graph_cases as G
import oracle_lib as O
import phase_cases as HC
import phase_ref as HR
import pileup_cases as PC
import pileup_fuzz_cases as FC
import pileup_ref as PR
import seqthread_cases as SC
import unitigs_ref as R
from aindex_amd import _lib, builder
from aindex_amd.engine import Index

vp = _lib.vp
ARG = _lib.AIX_ERR_ARG
P8, P32, P64 = 0x6B, 0x6B6B6B6B, 0x6B6B6B6B6B6B6B6B
LOOSE = dict(min_depth=1, min_major_permille=500, min_alt_count=1, min_alt_permille=50)       # thresholds the small batches reach
EVERY = dict(LOOSE, min_alt_count=0, min_alt_permille=0)                                       # every covered base is a site
_UNSIGNED = {np.dtype(np.int64): np.uint64, np.dtype(np.int32): np.uint32}
OBS_KEYS = ("frag_obs_off", "obs_site", "obs_allele") + HR.LINK_KEYS
OBS_DTYPES = (np.uint64, np.uint32, np.uint8) + HR.LINK_DTYPES
EDGE_KEYS = HR.EDGE_KEYS + ("edge_off",)
EDGE_DTYPES = (np.uint32,) * 4 + (np.uint64,)
SOLVED_KEYS = ("site_block", "site_phase", "site_parent", "edge_state")
SOLVED_DTYPES = (np.uint32, np.uint8, np.uint32, np.uint8)
THRESHOLDS = ({}, dict(min_link_reads=1, min_link_permille=501))


def _open(prefix):
    return Index.open_23(prefix + ".pf", prefix + ".tf.bin", prefix + ".kmers.bin")


def _np(t):
    a = t.cpu().numpy()
    return a.view(_UNSIGNED.get(a.dtype, a.dtype))


def _t(a):
    import torch
    a = np.ascontiguousarray(a)
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}
    return torch.from_numpy(a.view(signed.get(a.dtype, a.dtype)).copy()).cuda()


def _dev_seqs(seqs):
    seqs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
    return _t(np.frombuffer(b"".join(seqs), dtype=np.uint8)), _t(PC.seq_offs(seqs))


def _write_index(prefix, codes, tfs):
    open(prefix + ".pf", "wb").write(builder.build_pf_codes(codes, 23))
    rc, checker, tf = O.index_scatter(O.OracleMphf(prefix + ".pf"), np.ascontiguousarray(D.decode(codes)).reshape(-1), tfs)
    assert rc == 0
    checker.tofile(prefix + ".kmers.bin")
    tf.tofile(prefix + ".tf.bin")
    return prefix


@pytest.fixture(scope="module")
def ix(tmp_path_factory):
    with _open(G.write_graph_case(0, str(tmp_path_factory.mktemp("ph")))[0]) as index:
        yield index


def _same(got, want, keys, dtypes, tag):
    for k, dt in zip(keys, dtypes):
        a = _np(got[k]) if hasattr(got[k], "cpu") else got[k]
        assert a.dtype == dt and np.array_equal(a, want[k]), (tag, k)


def _dev(d, keys):
    return {k: _t(d[k]) for k in keys}


def _solve_every_form(ix, sites, links, tag, obs=None, dev_obs=None, h=None):
    """bundle, solve at THRESHOLDS, the host form and (with observations) tag against the restatement"""
    h = hashlib.sha256() if h is None else h
    V = len(sites["var_unitig"])
    want_edges = HR.bundle(V, links)
    dev_sites = {"var_unitig": _t(sites["var_unitig"])}
    edges = ix.phase_bundle_t(V, links if hasattr(links["link_lo"], "cpu") else _dev(links, HR.LINK_KEYS))
    _same(edges, want_edges, EDGE_KEYS, EDGE_DTYPES, tag)
    assert edges["n_edges"] == want_edges["n_edges"], tag
    for th in THRESHOLDS:
        want = HR.solve(sites["var_unitig"], want_edges, **th)
        solved = ix.phase_solve_t(dev_sites, edges, **th)
        _same(solved, want, SOLVED_KEYS, SOLVED_DTYPES, (tag, sorted(th)))
        assert solved["counts"] == want["counts"].tolist(), tag
        for k in SOLVED_KEYS:
            h.update(_np(solved[k]).tobytes())
        if obs is not None:
            _same(ix.phase_tag_t(dev_obs, solved), HR.tag(obs, want), HR.TAG_KEYS, (np.uint32,) * 4, (tag, "tag"))
    for k in EDGE_KEYS:
        h.update(_np(edges[k]).tobytes())
    return h, want_edges


def _every_form(ix, offsets, seqs, places, sites, tag, groups=(1,), want=None):
    """observe per group, then bundle, solve and tag, against the restatement (computed once per case: `want` is a dict the first call
    fills) -> the digest of every device output"""
    want = {} if want is None else want
    st, so = _dev_seqs(seqs)
    graph = {"offsets": _t(offsets)}
    dev_places = places if hasattr(places["seq_place_off"], "cpu") else _dev(places, PR.PLACE_KEYS[:6])
    dev_sites = sites if hasattr(sites["var_unitig"], "cpu") else _dev(sites, PR.VAR_KEYS[:4])
    host_sites = {k: _np(v) if hasattr(v, "cpu") else v for k, v in sites.items() if k in PR.VAR_KEYS[:4]}
    h = hashlib.sha256()
    for group in groups:
        if group not in want:
            host_places = {k: _np(v) if hasattr(v, "cpu") else v for k, v in places.items() if k in PR.PLACE_KEYS[:6]}
            want[group] = HR.observe([s.encode() if isinstance(s, str) else bytes(s) for s in seqs], host_places, offsets, host_sites, group)
        w = want[group]
        for hint in (0, int(w["stats"][4]) + 3):
            obs = ix.phase_observe_t(graph, st, so, dev_places, dev_sites, group, hint)
            _same(obs, w, OBS_KEYS, OBS_DTYPES, (tag, group, hint))
            assert obs["stats"] == w["stats"].tolist() and (obs["n_obs"], obs["n_links"]) == (w["stats"][4], w["stats"][5]), (tag, group)
        for k in OBS_KEYS:
            h.update(_np(obs[k]).tobytes())
        _solve_every_form(ix, host_sites, w, (tag, group), w, obs, h)
    return h.hexdigest()


# ---- 1. the planted case ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    p = HC.planted()
    ref = PC.ref_graph(p["codes"], p["tfs"], 1, 3)
    out = dict(p=p, ref=ref, prefix=_write_index(str(tmp_path_factory.mktemp("php") / "planted"), p["codes"], p["tfs"]))
    for name, seqs, group in (("reads", p["reads"], 1), ("mates", p["mates"], 2)):
        _, places, piled = PC.chain(ref, seqs)
        called = PR.call(ref["g"]["offsets"], ref["g"]["bases"], piled["counts"])
        out[name] = (places, called) + HC.phase(seqs, places, ref["g"]["offsets"], called, group)
    return out


@pytest.mark.parametrize("name", ("reads", "mates"))
def test_planted_case_through_the_t_methods(planted, name):
    p, ref = planted["p"], planted["ref"]
    places, called, obs, edges, solved, tags = planted[name]
    seqs, group = (p["reads"], 1) if name == "reads" else (p["mates"], 2)
    with _open(planted["prefix"]) as ix:
        graph = ix.thread_graph_t(1, 46, 46, 3)
        assert np.array_equal(_np(graph["bases"]), ref["g"]["bases"])
        st, so = _dev_seqs(seqs)
        dev_places = ix.pile_place_t(graph, so, ix.seq_thread_t(graph, st, so))
        dev_called = ix.pile_call_t(graph, ix.pileup_t(graph, st, so, dev_places)["counts"])
        _same(dev_called, called, PR.VAR_KEYS, PR.VAR_DTYPES, name)
        got = ix.phase_observe_t(graph, st, so, dev_places, dev_called, group)
        _same(got, obs, OBS_KEYS, OBS_DTYPES, name)
        assert got["stats"] == obs["stats"].tolist()
        dev_edges = ix.phase_bundle_t(dev_called["total"], got)
        _same(dev_edges, edges, EDGE_KEYS, EDGE_DTYPES, name)
        dev_solved = ix.phase_solve_t(dev_called, dev_edges)
        _same(dev_solved, solved, SOLVED_KEYS, SOLVED_DTYPES, name)
        assert dev_solved["counts"] == solved["counts"].tolist() and dev_solved["counts"][0] == (3 if name == "reads" else 2) and dev_solved["counts"][4] == 0
        _same(ix.phase_tag_t(got, dev_solved), tags, HR.TAG_KEYS, (np.uint32,) * 4, name)


@pytest.mark.parametrize("paired", (False, True))
def test_planted_case_through_aindex(planted, paired, tmp_path):
    from aindex_amd.aindex import AIndex, format_vcf_phased
    p = planted["p"]
    places, called, obs, edges, solved, tags = planted["mates" if paired else "reads"]
    reads = list(zip(p["mates"][::2], p["mates"][1::2])) if paired else p["reads"]
    pos, none = called["var_pos"].tolist(), HR.NONE
    want_tail = [(None, None) if ph == none else (pos[b], ph) for b, ph in zip(solved["site_block"].tolist(), solved["site_phase"].tolist())]
    prefix = planted["prefix"]
    a = AIndex.load_23mer_index(prefix + ".pf", prefix + ".tf.bin", prefix + ".kmers.bin")
    try:
        got = a.get_phased_variants(reads, cutoff=1, paired=paired)
        assert [r[:4] for r in got] == [(0, x, chr(r), chr(alt)) for x, r, alt in zip(pos, called["var_ref"].tolist(), called["var_alt"].tolist())]
        assert [r[4:7] for r in got] == list(zip(called["var_ref_count"].tolist(), called["var_alt_count"].tolist(), called["var_depth"].tolist()))
        assert [r[7:] for r in got] == want_tail
        blocks = a.get_phase_blocks(reads, cutoff=1, paired=paired)
        members = {}
        for v, (b, ph) in enumerate(zip(solved["site_block"].tolist(), solved["site_phase"].tolist())):
            if ph != none:
                members.setdefault(b, []).append(v)
        state_of = lambda b, s: sum(1 for hi, st in zip(edges["edge_hi"].tolist(), solved["edge_state"].tolist()) if st == s and solved["site_block"][hi] == b)
        assert blocks == [(0, pos[m[0]], pos[m[-1]], len(m), state_of(b, 1), state_of(b, 2)) for b, m in sorted(members.items())]
        assert len(blocks) == (2 if paired else 3) and sum(r[4] for r in blocks) == solved["counts"][3]
        want_tags = [None if b == HR.NO_SITE else (0, pos[b], h0, h1, o) for b, h0, h1, o in zip(*(tags[k].tolist() for k in HR.TAG_KEYS))]
        assert a.get_read_haplotags(reads, cutoff=1, paired=paired) == want_tags and len(want_tags) == len(reads)
        out = str(tmp_path / "phased.vcf")
        assert a.write_phased_vcf(out, reads, cutoff=1, paired=paired) == len(pos)
        lines = open(out).read().splitlines()
        assert lines == list(format_vcf_phased(got, [HC.GENOME]))
        assert lines[-len(pos) - 1] == "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tsample" and sum(l.startswith("##FORMAT=<ID=") for l in lines) == 2
        body = [l.split("\t") for l in lines if l[0] != "#"]
        assert all(f[8] == "GT:PS" and f[9] == "%s:%d" % ("1|0" if ph else "0|1", b + 1) for f, (b, ph) in zip(body, want_tail))
        assert list(format_vcf_phased([(0, 4, "A", "C", 5, 4, 9, None, None)]))[-1] == "c0\t5\t.\tA\tC\t.\t.\tDP=9;AD=5,4\tGT:PS\t0/1:."
    finally:
        a._wrapper.close()


# ---- 2. graph cases with their own reads --------------------------------------------------------------------
@pytest.mark.parametrize("seed", (0, 3))
def test_graph_cases(seed, tmp_path):
    with _open(G.write_graph_case(seed, str(tmp_path))[0]) as ix:
        ref = PC.ref_graph(ix.checker_array() & np.uint64(R.MASK), ix.tf_array(), 0)
        seqs = SC.batch(ref["un"], ref["lk"], seed).seqs
        seqs = seqs + seqs[:len(seqs) % 2]                           # an even number, for fragments of two
        _, places, piled = PC.chain(ref, seqs)
        for th in (LOOSE, EVERY):
            called = PR.call(ref["g"]["offsets"], ref["g"]["bases"], piled["counts"], **th)
            assert called["total"] > (1000 if th is EVERY else 2)
            _every_form(ix, ref["g"]["offsets"], seqs, places, called, (seed, sorted(th.items())), groups=(1, 2))


# ---- 3. hand-made arrays ------------------------------------------------------------------------------------
def _hot_sites(case, seed, n):
    """random sites plus the base under the 3000 placements of the case: one fragment with far more than 64 raw observations of one site"""
    s = HC.random_sites(case, seed, n)
    off = case["offsets"].astype(np.int64)
    g = np.unique(np.concatenate((off[s["var_unitig"]] + s["var_pos"], [case["hot"]])))
    u = np.searchsorted(off, g, side="right") - 1
    ref = case["bases"][g]
    alt = np.frombuffer(b"CATG", np.uint8)[np.searchsorted(np.frombuffer(b"ACGT", np.uint8), ref)]
    return {"var_unitig": u.astype(np.uint32), "var_pos": (g - off[u]).astype(np.uint32), "var_ref": ref.astype(np.uint8), "var_alt": alt.astype(np.uint8)}


@pytest.mark.parametrize("seed", FC.PLACEMENT_SEEDS[:3])
def test_placements_no_threading_writes(ix, seed):
    """U = 1, 2 and 40 contigs of 23 to 300 bases (waves straddle contig boundaries), placements of one base, every byte value, empty
    sequences and empty mates, a site at base 0 of contig 0 and at the last base of the last contig, a run of raws that crosses waves."""
    case = FC.placements_case(seed)
    sites = _hot_sites(case, 900 + seed, 500)
    assert len(case["seqs"]) % 2 == 0 and any(len(s) == 0 for s in case["seqs"]) and sites["var_pos"][0] == 0
    want = {}
    _every_form(ix, case["offsets"], case["seqs"], case["places"], sites, seed, groups=(1, 2), want=want)
    assert want[1]["stats"][0] > 3000 and want[1]["stats"][2] >= 1 and want[2]["stats"][1] <= want[1]["stats"][1]


def test_shapes_where_the_kernels_can_go_wrong(ix):
    import torch
    rng = np.random.default_rng(5)
    a = PC.random_text(rng, 400)
    off = PC.seq_offs([a])
    one = lambda rows: {"seq_place_off": np.array([0, len(rows)], np.uint64), **{k: np.array(c, dtype=dt) for k, dt, c in
                                                                                     zip(PR.PLACE_KEYS[1:6], PR.PLACE_DTYPES[1:6], zip(*rows))}}
    every = HC.sites_dict([(x, a[x], PC.substitute(a, x)[x]) for x in range(50, 350)])
    read = "".join(PC.substitute(a, x)[x] if x % 3 == 0 else a[x] for x in range(50, 350))
    w = {}
    _every_form(ix, off, [read], one([(0, 0, 50, 0, 300)]), every, "every base a site", want=w)
    assert w[1]["stats"].tolist() == [300, 300, 0, 0, 300, 299]
    _every_form(ix, off, [PC.rc(read)], one([(0, 1, 50, 0, 300)]), every, "every base a site, backwards", want={})
    few = HC.sites_dict([(0, a[0], PC.substitute(a, 0)[0]), (399, a[399], PC.substitute(a, 399)[399])])
    w = {}
    _every_form(ix, off, [a[1:399], a], one([(0, 0, 1, 0, 398)]) | {"seq_place_off": np.array([0, 1, 1], np.uint64)}, few, "placements holding 0 sites", want=w)
    assert w[1]["stats"].tolist() == [0] * 6
    empty = {"seq_place_off": np.zeros(3, np.uint64), **{k: np.zeros(0, dt) for k, dt in zip(PR.PLACE_KEYS[1:6], PR.PLACE_DTYPES[1:6])}}
    _every_form(ix, off, [a, ""], empty, few, "R = 0", groups=(1, 2))
    _every_form(ix, off, [], dict(empty, seq_place_off=np.zeros(1, np.uint64)), few, "F = 0", groups=(1, 2))
    _every_form(ix, off, [a], one([(0, 0, 0, 0, 400)]), HC.sites_dict([]), "V = 0")
    unit = lambda V: {"var_unitig": np.zeros(V, np.uint32)}
    for V in (0, 1, 2, 63, 64, 65):
        _solve_every_form(ix, unit(V), HC.chain_links(V, (0, 1, 1)), ("V", V))
    # 4097 sites on one contig: 13 jumping rounds, more than one workgroup; alternating signs; the chain cut every 64 sites
    for signs, cut in (((0,), 0), ((0, 1), 0), ((1, 0, 0), 64)):
        links = HC.chain_links(4097, signs, 2, cut)
        h, edges = _solve_every_form(ix, unit(4097), links, ("chain", signs, cut))
        s = HR.solve(unit(4097)["var_unitig"], edges)
        assert (s["counts"][0], s["counts"][1]) == ((64, 4096) if cut else (1, 4097)) and (len(signs) == 1 or 1000 < int(s["site_phase"].sum()) < 3000)
    two = {"var_unitig": np.repeat(np.array([0, 1, 4], np.uint32), (40, 1, 30))}
    links = HC.chain_links(71, (0, 1), 3)
    keep = (links["link_hi"] != 40) & (links["link_hi"] != 41)                                 # no link crosses a contig boundary
    _solve_every_form(ix, two, {k: v[keep] for k, v in links.items()}, "three contigs")
    torch.cuda.synchronize()


def test_links_of_two_batches_in_either_order(ix):
    case = FC.placements_case(1)
    sites = _hot_sites(case, 77, 500)
    obs = HR.observe(case["seqs"], case["places"], case["offsets"], sites)
    n = len(obs["link_lo"]) // 2
    assert n > 5
    halves = [{k: obs[k][:n] for k in HR.LINK_KEYS}, {k: obs[k][n:] for k in HR.LINK_KEYS}]
    V = len(sites["var_unitig"])
    got = [ix.phase_bundle_t(V, _dev({k: np.concatenate((x[k], y[k])) for k in HR.LINK_KEYS}, HR.LINK_KEYS)) for x, y in (halves, halves[::-1])]
    want = HR.bundle(V, obs)
    for g in got:
        _same(g, want, EDGE_KEYS, EDGE_DTYPES, "either order")
    host = ix.phase_solve(sites["var_unitig"], obs["link_lo"], obs["link_hi"], obs["link_rel"], 1, 600)
    _same(host, dict(want, **HR.solve(sites["var_unitig"], want, 1, 600)), EDGE_KEYS + SOLVED_KEYS + ("counts",), EDGE_DTYPES + SOLVED_DTYPES + (np.uint64,), "host form")
    assert host["n_edges"] == want["n_edges"]
    none = ix.phase_solve(np.zeros(0, np.uint32), *[np.zeros(0, np.uint32)] * 3)
    assert none["n_edges"] == 0 and none["edge_off"].tolist() == [0] and none["counts"].tolist() == [0] * 6


def test_many_trips_of_every_loop_and_a_side_stream(ix, monkeypatch):
    import torch
    case = FC.placements_case(2)
    sites = _hot_sites(case, 31, 500)
    shared = {}
    run = lambda tag: _every_form(ix, case["offsets"], case["seqs"], case["places"], sites, tag, groups=(1, 2), want=shared)
    want = run("default")
    assert run("again") == want
    for grid in ("1", "2", "3"):
        monkeypatch.setenv("AIX_UG_TEST_GRID", grid)
        assert run(("grid", grid)) == want, grid
    monkeypatch.delenv("AIX_UG_TEST_GRID")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        got = run("side stream")
    side.synchronize()
    assert got == want
    torch.cuda.synchronize()


# ---- 4. the raw calls: caps, nullable outputs, violations ---------------------------------------------------
def _poison(n, ty):
    import torch
    return torch.full((n + 64,), P8 if ty == torch.uint8 else (P32 if ty == torch.int32 else P64), dtype=ty, device="cuda")


def _clean(t, k=0):
    import torch
    return bool((t[k:] == (P8 if t.dtype == torch.uint8 else (P32 if t.dtype == torch.int32 else P64))).all())


def _q(t):
    return None if t is None else vp(t.data_ptr())


class _Observe:
    """aix_phase_observe_dev itself on a small case, 64 poisoned elements behind every output"""

    def __init__(self):
        rng = np.random.default_rng(9)
        self.a, self.b = PC.random_text(rng, 200), PC.random_text(rng, 100)
        self.off = PC.seq_offs([self.a, self.b])
        self.seqs = [PC.substitute(self.a[10:110], 50).encode(), PC.rc(self.b[20:90]).encode(), (self.a[100:150] + "N" + self.a[151:200]).encode(), b""]
        rows = [(0, 0, 10, 0, 100), (1, 1, 20, 0, 70), (0, 0, 100, 0, 100)]
        self.places = {"seq_place_off": np.array([0, 1, 2, 3, 3], np.uint64), **{k: np.array(c, dtype=dt) for k, dt, c in
                                                                                zip(PR.PLACE_KEYS[1:6], PR.PLACE_DTYPES[1:6], zip(*rows))}}
        self.sites = {k: np.concatenate((x, y)) for (k, x), y in zip(
            HC.sites_dict([(x, self.a[x], PC.substitute(self.a, x)[x]) for x in (10, 60, 105, 109, 150, 199)]).items(),
            HC.sites_dict([(x, self.b[x], PC.substitute(self.b, x)[x]) for x in (0, 25, 50, 89)], 1).values())}
        self.want = HR.observe(self.seqs, self.places, self.off, self.sites)
        self.st, self.so = _dev_seqs(self.seqs)
        self.dev_off = _t(self.off)

    def __call__(self, obs_cap, link_cap, group=1, stats=True, places=None, sites=None, off=None, so=None, null_obs=False, null_links=False):
        import torch
        p = _dev(self.places if places is None else places, PR.PLACE_KEYS[:6])
        s = _dev(self.sites if sites is None else sites, PR.VAR_KEYS[:4])
        off, so = self.dev_off if off is None else off, self.so if so is None else so
        n_obs, n_links = int(self.want["stats"][4]), int(self.want["stats"][5])
        M = so.numel() - 1
        outs = [_poison(M // max(group, 1) + 1, torch.int64), _poison(n_obs, torch.int32), _poison(n_obs, torch.uint8), _poison(n_links, torch.int32),
                _poison(n_links, torch.int32), _poison(n_links, torch.uint8), _poison(6, torch.int64)]
        to, tl = C.c_uint64(77), C.c_uint64(77)
        obs_ptrs = [None, None] if null_obs else [_q(t) for t in outs[1:3]]
        link_ptrs = [None] * 3 if null_links else [_q(t) for t in outs[3:6]]
        status = _lib.lib().aix_phase_observe_dev(_q(self.st), _q(so), M, group, *[_q(p[k]) for k in PR.PLACE_KEYS[:1]], p["place_unitig"].numel(),
                                                  *[_q(p[k]) for k in PR.PLACE_KEYS[1:6]], off.numel() - 1, _q(off), s["var_unitig"].numel(),
                                                  *[_q(s[k]) for k in PR.VAR_KEYS[:4]], _q(outs[0]), *obs_ptrs, obs_cap, C.byref(to), *link_ptrs, link_cap, C.byref(tl),
                                                  _q(outs[6]) if stats else None, None)
        torch.cuda.synchronize()
        return status, to.value, tl.value, outs


def test_sizing_of_both_kinds_and_the_nullable_stats():
    ob = _Observe()
    w = ob.want
    n_obs, n_links = int(w["stats"][4]), int(w["stats"][5])
    assert n_obs > 4 and n_links > 2 and w["stats"][2] >= 1
    for obs_cap in (0, n_obs - 1, n_obs, n_obs + 5):
        for link_cap in (0, n_links - 1, n_links, n_links + 5):
            status, to, tl, outs = ob(obs_cap, link_cap, stats=(obs_cap + link_cap) % 2 == 0, null_obs=obs_cap == 0, null_links=link_cap == 0)
            tag = (obs_cap, link_cap)
            assert status == 0 and (to, tl) == (n_obs, n_links), tag
            assert np.array_equal(_np(outs[0][:5]), w["frag_obs_off"]) and _clean(outs[0], 5), tag
            if obs_cap >= n_obs:
                assert np.array_equal(_np(outs[1][:n_obs]), w["obs_site"]) and np.array_equal(_np(outs[2][:n_obs]), w["obs_allele"]), tag
            assert all(_clean(t, n_obs if obs_cap >= n_obs else 0) for t in outs[1:3]), tag
            if link_cap >= n_links:
                assert all(np.array_equal(_np(t[:n_links]), w[k]) for t, k in zip(outs[3:6], HR.LINK_KEYS)), tag
            assert all(_clean(t, n_links if link_cap >= n_links else 0) for t in outs[3:6]), tag
            if (obs_cap + link_cap) % 2 == 0:
                assert np.array_equal(_np(outs[6][:6]), w["stats"]) and _clean(outs[6], 6), tag
            else:
                assert _clean(outs[6]), tag


def test_observe_violations_leave_everything_untouched():
    ob = _Observe()
    n_obs, n_links = int(ob.want["stats"][4]), int(ob.want["stats"][5])
    over = lambda d, k, j, v: dict(d, **{k: np.concatenate((d[k][:j], [v], d[k][j + 1:])).astype(d[k].dtype)})
    bad_off = _t(np.array([0, 200, 210], np.uint64))
    bad_so = _t(np.array([0, 100, 170, 270, 1 << 33], np.uint64))
    cases = [("u = U", dict(sites=over(ob.sites, "var_unitig", 9, 2))), ("pos = L", dict(sites=over(ob.sites, "var_pos", 9, 100))),
             ("g equal", dict(sites=over(ob.sites, "var_pos", 1, 10))), ("g descending", dict(sites=over(ob.sites, "var_pos", 2, 59))),
             ("contigs descending", dict(sites=over(ob.sites, "var_unitig", 3, 1))), ("ref lower case", dict(sites=over(ob.sites, "var_ref", 0, ord("a")))),
             ("alt N", dict(sites=over(ob.sites, "var_alt", 4, ord("N")))), ("ref == alt", dict(sites=over(ob.sites, "var_alt", 4, int(ob.sites["var_ref"][4])))),
             ("broken CSR", dict(places=over(ob.places, "seq_place_off", 1, 3))), ("CSR does not end at R", dict(places=over(ob.places, "seq_place_off", 4, 2))),
             ("placement on U", dict(places=over(ob.places, "place_unitig", 1, 2))), ("beyond the contig", dict(places=over(ob.places, "place_pos", 1, 31))),
             ("q0 + len beyond the read", dict(places=over(ob.places, "place_q0", 0, 1))), ("len = 0", dict(places=over(ob.places, "place_len", 2, 0))),
             ("offsets", dict(off=bad_off)), ("sequence offsets", dict(so=bad_so)), ("group 3", dict(group=3)), ("group 0", dict(group=0))]
    for what, kw in cases:
        status, to, tl, outs = ob(n_obs, n_links, **kw)
        assert status == ARG and (to, tl) == (77, 77) and all(_clean(t) for t in outs), what
    odd = dict(ob.places, seq_place_off=ob.places["seq_place_off"][:4])
    status, to, tl, outs = ob(n_obs, n_links, group=2, places=odd, so=_t(PC.seq_offs(ob.seqs[:3])))
    assert status == ARG and all(_clean(t) for t in outs), "M odd"
    status, to, tl, outs = ob(n_obs, n_links, null_obs=True)
    assert status == ARG and (to, tl) == (77, 77) and all(_clean(t) for t in outs), "NULL at a cap above 0"


def _raw_bundle(V, links, N=None):
    import torch
    L = _dev(links, HR.LINK_KEYS)
    n = len(links["link_lo"]) if N is None else N
    outs = [_poison(len(links["link_lo"]), torch.int32) for _ in range(4)] + [_poison(min(V + 1, 1 << 10), torch.int64)]      # (a V beyond the limit is refused at once)
    e = C.c_uint64(77)
    status = _lib.lib().aix_phase_bundle_dev(V, n, *[_q(L[k]) for k in HR.LINK_KEYS], *[_q(t) for t in outs], C.byref(e), None)
    torch.cuda.synchronize()
    return status, e.value, outs


def _raw_solve(unit, edges, parent=True, state=True, counts=True, E=None):
    import torch
    V, E = len(unit), (len(edges["edge_lo"]) if E is None else E)
    d = _dev(edges, ("edge_off", "edge_lo", "edge_cis", "edge_trans"))
    outs = [_poison(V, torch.int32), _poison(V, torch.uint8), _poison(V, torch.int32), _poison(E, torch.uint8), _poison(6, torch.int64)]
    ptrs = [_q(outs[0]), _q(outs[1]), _q(outs[2]) if parent else None, _q(outs[3]) if state else None, _q(outs[4]) if counts else None]
    status = _lib.lib().aix_phase_solve_dev(V, _q(_t(unit)), _q(d["edge_off"]), E, _q(d["edge_lo"]), _q(d["edge_cis"]), _q(d["edge_trans"]), 2, 800, *ptrs, None)
    torch.cuda.synchronize()
    return status, outs


def _raw_tag(obs, solved):
    import torch
    F, n, V = len(obs["frag_obs_off"]) - 1, len(obs["obs_site"]), len(solved["site_block"])
    o, s = _dev(obs, ("frag_obs_off", "obs_site", "obs_allele")), _dev(solved, ("site_block", "site_phase"))
    outs = [_poison(F, torch.int32) for _ in range(4)]
    status = _lib.lib().aix_phase_tag_dev(F, _q(o["frag_obs_off"]), n, _q(o["obs_site"]), _q(o["obs_allele"]), V, _q(s["site_block"]), _q(s["site_phase"]),
                                          *[_q(t) for t in outs], None)
    torch.cuda.synchronize()
    return status, outs


def test_bundle_solve_and_tag_violations_and_nullable_outputs():
    over = lambda d, k, j, v: dict(d, **{k: np.concatenate((d[k][:j], [v], d[k][j + 1:])).astype(d[k].dtype)})
    links = HC.chain_links(6, (0, 1), 3)
    status, e, outs = _raw_bundle(6, links)
    want = HR.bundle(6, links)
    assert status == 0 and e == 5 and all(np.array_equal(_np(t[:5]), want[k]) and _clean(t, 15) for t, k in zip(outs, HR.EDGE_KEYS))
    assert np.array_equal(_np(outs[4][:7]), want["edge_off"]) and _clean(outs[4], 7)
    for what, bad in (("lo == hi", over(links, "link_lo", 4, 2)), ("lo > hi", over(links, "link_lo", 4, 5)), ("hi == V", over(links, "link_hi", 14, 6)),
                      ("rel 2", over(links, "link_rel", 7, 2))):
        status, e, outs = _raw_bundle(6, bad)
        assert status == ARG and e == 77 and all(_clean(t) for t in outs), what
    assert _raw_bundle(6, links, N=1 << 32)[0] == _lib.AIX_ERR_UNSUPPORTED and _raw_bundle((1 << 31) - 3, links)[0] == _lib.AIX_ERR_UNSUPPORTED
    unit = np.zeros(6, np.uint32)
    w = HR.solve(unit, want)
    for parent in (True, False):
        for state in (True, False):
            for counts in (True, False):
                status, outs = _raw_solve(unit, want, parent, state, counts)
                tag = (parent, state, counts)
                assert status == 0 and np.array_equal(_np(outs[0][:6]), w["site_block"]) and np.array_equal(_np(outs[1][:6]), w["site_phase"]), tag
                assert all(_clean(t, 6) for t in outs[:2]), tag
                assert (np.array_equal(_np(outs[2][:6]), w["site_parent"]) and _clean(outs[2], 6)) if parent else _clean(outs[2]), tag
                assert (np.array_equal(_np(outs[3][:5]), w["edge_state"]) and _clean(outs[3], 5)) if state else _clean(outs[3]), tag
                assert (np.array_equal(_np(outs[4][:6]), w["counts"]) and _clean(outs[4], 6)) if counts else _clean(outs[4]), tag
    tri = HR.bundle(6, {k: np.concatenate((links[k], [v] * 3)).astype(links[k].dtype) for k, v in zip(HR.LINK_KEYS, (1, 3, 0))})      # row 3: lo 1 and 2
    assert tri["edge_lo"].tolist() == [0, 1, 1, 2, 3, 4]
    bad_cases = [("edge_off does not start at 0", unit, over(want, "edge_off", 0, 1)), ("edge_off descends", unit, over(want, "edge_off", 3, 0)),
                 ("edge_off does not end at E", unit, over(want, "edge_off", 6, 4)), ("lo == w", unit, over(want, "edge_lo", 2, 3)),
                 ("lo beyond V", unit, over(want, "edge_lo", 2, 1 << 31)), ("lo equal in a row", unit, over(tri, "edge_lo", 3, 1)),
                 ("lo descending in a row", unit, over(over(tri, "edge_lo", 2, 2), "edge_lo", 3, 1)),
                 ("an edge across contigs", np.array([0, 0, 0, 1, 1, 1], np.uint32), want), ("var_unitig descends", np.array([1, 1, 1, 1, 1, 0], np.uint32), want)]
    for what, u, edges in bad_cases:
        status, outs = _raw_solve(u, edges)
        assert status == ARG and all(_clean(t) for t in outs), what
    obs = {"frag_obs_off": np.array([0, 3, 3, 5], np.uint64), "obs_site": np.array([0, 2, 5, 1, 4], np.uint32), "obs_allele": np.array([0, 1, 1, 0, 0], np.uint8)}
    status, outs = _raw_tag(obs, w)
    wt = HR.tag(obs, w)
    assert status == 0 and all(np.array_equal(_np(t[:3]), wt[k]) and _clean(t, 3) for t, k in zip(outs, HR.TAG_KEYS))
    for what, o, s in (("CSR does not start at 0", over(obs, "frag_obs_off", 0, 1), w), ("CSR descends", over(obs, "frag_obs_off", 1, 4), w),
                       ("CSR does not end at n_obs", over(obs, "frag_obs_off", 3, 4), w), ("site == V", over(obs, "obs_site", 2, 6), w),
                       ("allele 2", over(obs, "obs_allele", 0, 2), w), ("block beyond its site", obs, over(w, "site_block", 2, 3)),
                       ("phase 2", obs, over(w, "site_phase", 5, 2))):
        status, outs = _raw_tag(o, s)
        assert status == ARG and all(_clean(t) for t in outs), what
