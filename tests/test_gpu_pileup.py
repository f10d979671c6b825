"""The pile-up on the GPU (k_pl_* of aix_pileup.hip) against the test-side restatement (tests/pileup_ref.py, pinned by
test_pileup_cpu.py) on the batches of tests/seqthread_cases.py and the cases of tests/pileup_cases.py. Every comparison is exact equality."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import debruijn_ref as D
import graph_cases as G
import oracle_lib as O
import pileup_cases as PC
import pileup_ref as PR
import seqthread_cases as SC
import seqthread_ref as SR
import unitig_links_cases as LC
import unitigs_cases as UC
import unitigs_ref as R
from aindex_amd import _lib, builder
from aindex_amd.engine import Index

vp = _lib.vp
SEEDS = (0, 3, 6, 9)
P32, P8 = 0x6B6B6B6B, 0x6B
_UNSIGNED = {np.dtype(np.int64): np.uint64, np.dtype(np.int32): np.uint32}
LOOSE = dict(min_depth=1, min_major_permille=500, min_alt_count=1, min_alt_permille=50)       # thresholds the small batches reach


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


def _ref(ix, cutoff, rounds=0):
    return PC.ref_graph(ix.checker_array() & np.uint64(R.MASK), ix.tf_array(), cutoff, rounds)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("pl"))
    return {seed: G.write_graph_case(seed, d)[0] for seed in SEEDS}


_EVERY = dict(UC.topology_cases())
_EVERY.update(LC.link_cases())
NAMES = sorted(nm for nm, c in _EVERY.items() if c.codes.shape[0] + 22 <= 40_000 and nm != "isolated")      # those of test_gpu_seqthread.py


@pytest.fixture(scope="module")
def planted_topologies(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("plp"))
    made = {}

    def get(name):
        if name not in made:
            made[name] = _write_index(os.path.join(d, name), _EVERY[name].codes, _EVERY[name].tfs)
        return made[name]
    return get


def _same(got: dict, want: dict, keys, dtypes, tag):
    for k, dt in zip(keys, dtypes):
        a = _np(got[k]) if hasattr(got[k], "cpu") else got[k]
        assert a.dtype == dt and np.array_equal(a, want[k]), (tag, k)


def _same_call(got, want, tag):
    _same(got, want, PR.VAR_KEYS + ("polished", "depth_sum", "uncovered"), PR.VAR_DTYPES + (np.uint8, np.uint64, np.uint32), tag)
    assert (got["n_changed"], got["total"]) == (want["n_changed"], want["total"]), tag


def _device_chain(ix, graph, seqs, counts=None, **kw):
    st, so = _dev_seqs(seqs)
    places = ix.pile_place_t(graph, so, ix.seq_thread_t(graph, st, so), **kw)
    return places, ix.pileup_t(graph, st, so, places, counts)


def _every_form(ix, graph, ref, seqs, tag, host_cutoff=None, want=None):
    """pile_place_t, pileup_t (one call, two calls into one array, two halves), pile_call_t at two threshold sets and the host form
    against the restatement (computed once per case: `want` is a dict the first call fills); -> the digest of every device output"""
    g = ref["g"]
    want = {} if want is None else want
    if not want:
        steps, wp, wc = PC.chain(ref, seqs)
        want.update(wp=wp, wc=wc, calls=[PR.call(g["offsets"], g["bases"], wc["counts"], **th) for th in ({}, LOOSE)],
                    twice=PR.pile([s.encode() if isinstance(s, str) else bytes(s) for s in seqs], wp, g["offsets"], g["bases"], wc["counts"]))
    wp, wc = want["wp"], want["wc"]
    places, piled = _device_chain(ix, graph, seqs)
    _same(places, wp, PR.PLACE_KEYS, PR.PLACE_DTYPES, tag)
    assert (places["n_place"], places["n_circular_steps"]) == (wp["n_place"], wp["n_circular_steps"]), tag
    _same(piled, wc, ("counts", "place_mism"), (np.uint32, np.uint32), tag)
    assert piled["stats"] == wc["stats"].tolist(), tag
    h = hashlib.sha256()
    for t in [places[k] for k in PR.PLACE_KEYS] + [piled["counts"], piled["place_mism"]]:
        h.update(_np(t).tobytes())
    for th, called in zip(({}, LOOSE), want["calls"]):
        got = ix.pile_call_t(graph, piled["counts"], **th)
        _same_call(got, called, (tag, sorted(th)))
        for k in PR.VAR_KEYS + ("polished", "depth_sum", "uncovered"):
            h.update(_np(got[k]).tobytes())
    again = _device_chain(ix, graph, seqs, piled["counts"].clone())[1]
    assert np.array_equal(_np(again["counts"]), want["twice"]["counts"]), (tag, "two calls")
    half = len(seqs) // 2
    acc = _device_chain(ix, graph, seqs[:half])[1]["counts"]
    assert np.array_equal(_np(_device_chain(ix, graph, seqs[half:], acc)[1]["counts"]), wc["counts"]), (tag, "two halves")
    if host_cutoff is not None:
        host = ix.pileup(seqs, host_cutoff)
        _same(host, wp, PR.PLACE_KEYS, PR.PLACE_DTYPES, (tag, "host"))
        _same(host, dict(wc, offsets=g["offsets"], bases=g["bases"]), ("offsets", "bases", "counts", "place_mism", "stats"),
              (np.uint64, np.uint8, np.uint32, np.uint32, np.uint64), (tag, "host"))
        assert (host["U"], host["n_place"], host["n_circular_steps"]) == (g["U"], wp["n_place"], wp["n_circular_steps"]), tag
    return h.hexdigest()


@pytest.mark.parametrize("seed", SEEDS)
def test_graph_cases_every_form(cases, seed):
    """1. SC.batch on the graph cases at cutoffs 0 and 3: every form against the restatement."""
    with _open(cases[seed]) as ix:
        for cutoff in (0, 3):
            ref = _ref(ix, cutoff)
            b = SC.batch(ref["un"], ref["lk"], seed)
            _every_form(ix, ix.thread_graph_t(cutoff), ref, b.seqs, (seed, cutoff), host_cutoff=cutoff)


@pytest.mark.parametrize("seed", (0, 3))
def test_contigs_after_three_cleaning_rounds(cases, seed):
    """1b. The graph after three cleaning rounds: the batch of the unitig graph piled onto the contigs."""
    with _open(cases[seed]) as ix:
        ref0, ref = _ref(ix, 0), _ref(ix, 0, 3)
        graph = ix.thread_graph_t(0, 46, 46, 3)
        assert graph["rounds"] == ref["rounds"] >= 1 and np.array_equal(_np(graph["bases"]), ref["g"]["bases"])
        _every_form(ix, graph, ref, SC.batch(ref0["un"], ref0["lk"], seed).seqs, (seed, "contigs"))


@pytest.mark.parametrize("name", NAMES)
def test_planted_topologies(planted_topologies, name):
    """1c. Every planted topology and link case that test_gpu_seqthread.py threads."""
    with _open(planted_topologies(name)) as ix:
        ref = _ref(ix, 0)
        _every_form(ix, ix.thread_graph_t(0), ref, SC.batch(ref["un"], ref["lk"], 7).seqs, name, host_cutoff=0)


def test_many_trips_of_every_loop_and_a_side_stream(cases, monkeypatch):
    """2. AIX_UG_TEST_GRID = 1, 2, 3 workgroups for every launch (read per call): the results of the default grid; the same case twice and
    on a side stream: one digest."""
    import torch
    with _open(cases[3]) as ix:
        ref = _ref(ix, 0)
        seqs = SC.batch(ref["un"], ref["lk"], 5).seqs
        graph = ix.thread_graph_t(0)
        shared = {}
        want = _every_form(ix, graph, ref, seqs, "default", want=shared)
        assert _every_form(ix, graph, ref, seqs, "again", want=shared) == want
        for grid in ("1", "2", "3"):
            monkeypatch.setenv("AIX_UG_TEST_GRID", grid)
            assert _every_form(ix, graph, ref, seqs, ("grid", grid), want=shared) == want, grid
        monkeypatch.delenv("AIX_UG_TEST_GRID")
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            got = _every_form(ix, ix.thread_graph_t(0), ref, seqs, "side stream", want=shared)
        side.synchronize()
        assert got == want
    torch.cuda.synchronize()


def _hand_graph(texts):
    """a graph dict of device tensors (offsets, bases) from contig texts, and the matching restated arrays"""
    off = np.zeros(len(texts) + 1, np.uint64)
    off[1:] = np.cumsum([len(t) for t in texts])
    bases = np.frombuffer("".join(texts).encode(), np.uint8)
    return {"offsets": _t(off), "bases": _t(bases)}, off, bases


def _hand_steps(rows, m):
    """rows: (sequence, unitig, pos, flag, q_first, q_last), in order -> the dict of seqthread_ref.thread and the tuple of seq_thread_t"""
    sso = np.zeros(m + 1, np.uint64)
    for r in rows:
        sso[r[0] + 1:] += 1
    cols = list(zip(*rows)) if rows else [[]] * 6
    d = {"seq_step_off": sso}
    for k, dt, col in zip(SR.KEYS[1:6], SR.DTYPES[1:6], cols[1:]):
        d[k] = np.array(col, dtype=dt)
    return d, tuple(_t(d[k]) for k in SR.KEYS[:6])


def _hand_case(ix, texts, reads, rows, tag, **kw):
    """place, pile and call on hand-made steps against the restatement"""
    graph, off, bases = _hand_graph(texts)
    seqs = [r.encode() for r in reads]
    steps, dev_steps = _hand_steps(rows, len(seqs))
    st, so = _dev_seqs(seqs)
    wp = PR.place(PC.seq_offs(seqs), steps, off, **kw)
    places = ix.pile_place_t(graph, so, dev_steps, **kw)
    _same(places, wp, PR.PLACE_KEYS, PR.PLACE_DTYPES, tag)
    assert (places["n_place"], places["n_circular_steps"]) == (wp["n_place"], wp["n_circular_steps"]), tag
    wc = PR.pile(seqs, wp, off, bases)
    piled = ix.pileup_t(graph, st, so, places)
    _same(piled, wc, ("counts", "place_mism"), (np.uint32, np.uint32), tag)
    assert piled["stats"] == wc["stats"].tolist(), tag
    for th in ({}, LOOSE):
        _same_call(ix.pile_call_t(graph, piled["counts"], **th), PR.call(off, bases, wc["counts"], **th), tag)
    return wp, wc


def test_shapes_where_the_kernels_can_go_wrong(cases):
    """3. Placement lengths around the wave and the workgroup, the first base of the first and the last base of the last contig, U = 1,
    M = 0, T = 0, R = 0, a batch of circular steps only, a contig set beyond one block of the depth scan."""
    import torch
    rng = np.random.default_rng(21)
    with _open(cases[0]) as ix:
        a, b = PC.random_text(rng, 400), PC.random_text(rng, 300)
        reads, rows = [], []
        for n in (23, 63, 64, 65, 256, 257):
            x = int(rng.integers(1, 300 - n if n < 256 else 400 - n))
            for u, text in ((0, a), (1, b)) if n < 256 else ((0, a),):
                r = text[x:x + n]
                r = PC.substitute(r, n // 2) if n > 23 else r
                reads += [r, PC.rc(r)]
                rows += [(len(reads) - 2, u, x, 0, 0, n - 23), (len(reads) - 1, u, x + n - 23, 1, 0, n - 23)]
        reads += [a[:40], PC.rc(b[-40:]), b[-23:], a[:5].lower() + a[5:60] + "N" * 8]          # base 0 of contig 0, the last base of the last contig
        k = len(reads)
        rows += [(k - 4, 0, 0, 0, 0, 17), (k - 3, 1, 300 - 23, 1, 0, 17), (k - 2, 1, 300 - 23, 0, 0, 0), (k - 1, 0, 5, 0, 5, 37)]
        wp, wc = _hand_case(ix, [a, b], reads, rows, "lengths")
        assert sorted(set(wp["place_len"].tolist())) == [23, 40, 63, 64, 65, 68, 256, 257]
        assert wc["stats"][1] == 5 + 8 and wc["stats"][2] > 10
        assert wc["counts"].reshape(-1, 4)[0].sum() == 1 and wc["counts"].reshape(-1, 4)[-1].sum() == 2
        _hand_case(ix, [a], [a[10:70], PC.rc(a)], [(0, 0, 10, 0, 0, 37), (1, 0, 400 - 23, 1, 0, 400 - 23)], "U = 1")
        _hand_case(ix, [a, b], [], [], "M = 0")
        _hand_case(ix, [a, b], ["", a[:22], "ACGT"], [], "T = 0")
        wp, wc = _hand_case(ix, [a, b], [a[:60], b[:50]], [(0, 0, 3, 2, 0, 37), (1, 1, 9, 3, 0, 27)], "circular only")
        assert wp["n_place"] == 0 and wp["n_circular_steps"] == 2 and not wc["counts"].any()
        # a merge of three steps, a circular step between two linear ones (it parts them and is no neighbour), and max_gap / extend at 0
        mixed = [(0, 0, 5, 0, 0, 10), (0, 0, 40, 0, 35, 40), (0, 0, 90, 0, 85, 100), (1, 1, 100, 0, 0, 20), (1, 1, 7, 2, 30, 40), (1, 1, 160, 0, 60, 70)]
        for kw in ({}, {"max_gap": 0}, {"extend": 0}, {"max_gap": 24, "extend": 3}, {"max_gap": 0xFFFFFFFF, "extend": 0xFFFFFFFF}):
            _hand_case(ix, [a, b], [a[5:150], b[100:250]], mixed, ("mixed", sorted(kw.items())), **kw)
        # 70 000 bases in 90 contigs (the first holds what the others leave): the scan of the difference array and the select of the
        # variant flags run over many blocks
        texts = [PC.random_text(rng, int(n)) for n in rng.integers(23, 1000, 90)]
        texts[0] = PC.random_text(rng, 70_000 - sum(len(t) for t in texts[1:]))
        reads, rows = [], []
        for i in range(400):
            u = int(rng.integers(0, len(texts)))
            n = int(rng.integers(23, min(len(texts[u]), 300) + 1))
            x = int(rng.integers(0, len(texts[u]) - n + 1))
            r = texts[u][x:x + n]
            for _ in range(int(rng.integers(0, 3))):
                r = PC.substitute(r, int(rng.integers(0, n)))
            back = i % 2
            reads.append(PC.rc(r) if back else r)
            rows.append((i, u, x + n - 23 if back else x, back, 0, n - 23))
        wp, wc = _hand_case(ix, texts, reads, rows, "70 000 bases")
        assert PR.call(*_hand_graph(texts)[1:], wc["counts"], **LOOSE)["total"] > 20
    torch.cuda.synchronize()


def _raw_call(graph, counts, cap, total=None, **th):
    """aix_pile_call_dev itself with 64 poisoned elements behind every variant array"""
    import torch
    th = dict(dict(min_depth=8, min_major_permille=700, min_alt_count=3, min_alt_permille=200), **th)
    n = total if total is not None else cap
    types = (torch.int32, torch.int32, torch.uint8, torch.uint8, torch.int32, torch.int32, torch.int32)
    outs = [torch.full((n + 64,), P8 if ty == torch.uint8 else P32, dtype=ty, device="cuda") for ty in types]
    tot = C.c_uint64(77)
    q = lambda t: vp(t.data_ptr())
    status = _lib.lib().aix_pile_call_dev(graph["offsets"].numel() - 1, q(graph["offsets"]), q(graph["bases"]), q(counts), th["min_depth"], th["min_major_permille"],
                                          th["min_alt_count"], th["min_alt_permille"], None, None, *[q(t) for t in outs], cap, C.byref(tot), None, None, None)
    torch.cuda.synchronize()
    clean = lambda t, k=0: bool((t[k:] == (P8 if t.dtype == torch.uint8 else P32)).all())
    return status, tot.value, outs, clean


def test_variant_sizing(cases):
    """3b. cap = 0, total - 1 and total: the total always, the entries only when they fit, nothing at or beyond cap."""
    with _open(cases[3]) as ix:
        ref = _ref(ix, 0)
        seqs = SC.batch(ref["un"], ref["lk"], 3).seqs
        graph = ix.thread_graph_t(0)
        counts = _device_chain(ix, graph, seqs)[1]["counts"]
        want = PR.call(ref["g"]["offsets"], ref["g"]["bases"], _np(counts), **LOOSE)
        total = want["total"]
        assert total > 3
        for cap in (0, total - 1):
            status, tot, outs, clean = _raw_call(graph, counts, cap, total=total, **LOOSE)
            assert status == 0 and tot == total and all(clean(t) for t in outs), cap
        status, tot, outs, clean = _raw_call(graph, counts, total, **LOOSE)
        assert status == 0 and tot == total and all(clean(t, total) for t in outs)
        _same({k: t[:total] for k, t in zip(PR.VAR_KEYS, outs)}, want, PR.VAR_KEYS, PR.VAR_DTYPES, "cap == total")
        status, tot, outs, clean = _raw_call(graph, counts, total + 5, **LOOSE)
        assert status == 0 and tot == total and all(clean(t, total) for t in outs)
        assert ix.pile_call_t(graph, counts, cap_hint=total + 9, **LOOSE)["var_pos"].numel() == total


def test_array_level_violations_leave_everything_untouched(cases):
    """4. Inputs no index produces: every violation of the three validations is AIX_ERR_ARG with the poisoned outputs and counts untouched."""
    import torch
    L = _lib.lib()
    ARG = _lib.AIX_ERR_ARG
    rng = np.random.default_rng(33)
    a, b = PC.random_text(rng, 200), PC.random_text(rng, 100)
    graph, off, bases = _hand_graph([a, b])
    reads = [PC.substitute(a[10:110], 50), PC.rc(b[20:90])]
    seqs = [r.encode() for r in reads]
    steps, dev_steps = _hand_steps([(0, 0, 10, 0, 0, 27), (0, 0, 61, 0, 51, 77), (1, 1, 67, 1, 0, 47)], 2)
    st, so = _dev_seqs(seqs)
    wp = PR.place(PC.seq_offs(seqs), steps, off)
    U, T, R, B = 2, 3, wp["n_place"], 300
    q = lambda t: vp(t.data_ptr())
    poison = lambda n, ty: torch.full((n + 64,), P8 if ty == torch.uint8 else (P32 if ty == torch.int32 else 0x6B6B6B6B6B6B6B6B), dtype=ty, device="cuda")
    clean = lambda t: bool((t == (P8 if t.dtype == torch.uint8 else (P32 if t.dtype == torch.int32 else 0x6B6B6B6B6B6B6B6B))).all())

    def place(steps_=dev_steps, so_=so, off_=graph["offsets"], U_=U):
        outs = [poison(3, torch.int64)] + [poison(T, ty) for ty in (torch.int32, torch.uint8, torch.int32, torch.int32, torch.int32, torch.int32)]
        n, c = C.c_uint64(77), C.c_uint64(77)
        status = L.aix_pile_place_dev(2, q(so_), *[q(t) for t in steps_[:1]], T, *[q(t) for t in steps_[1:]], U_, q(off_), 46, 22, *[q(t) for t in outs], C.byref(n),
                                      C.byref(c), None)
        torch.cuda.synchronize()
        return status, n.value, c.value, outs

    def swapped(tensors, i, j, v):
        out = list(tensors)
        out[i] = tensors[i].clone()
        out[i][j] = v
        return tuple(out)

    status, n, c, outs = place()
    assert status == 0 and n == R == 2 and c == 0 and np.array_equal(_np(outs[0][:3]), wp["seq_place_off"]) and all(clean(t[T:]) for t in outs[1:])
    bad_off = graph["offsets"].clone()
    bad_off[1] = 290                                                # the second contig: 10 bases
    for what, kw in (("broken CSR", dict(steps_=swapped(dev_steps, 0, 1, 4))), ("CSR does not end at T", dict(steps_=swapped(dev_steps, 0, 2, 2))),
                     ("u = U", dict(steps_=swapped(dev_steps, 1, 0, U))), ("beyond the contig", dict(steps_=swapped(dev_steps, 2, 1, 160))),
                     ("backwards below its span", dict(steps_=swapped(dev_steps, 2, 2, 40))), ("q_last + 23 beyond the read", dict(steps_=swapped(dev_steps, 5, 1, 78))),
                     ("q_first > q_last", dict(steps_=swapped(dev_steps, 4, 0, 28))), ("descending steps", dict(steps_=swapped(dev_steps, 4, 1, 27))),
                     ("offsets", dict(off_=bad_off)), ("sequence offsets", dict(so_=swapped((so,), 0, 1, 400)[0]))):
        status, n, c, outs = place(**kw)
        assert status == ARG and n == 77 and c == 77 and all(clean(t) for t in outs), what
    places = {k: _t(wp[k]) for k in PR.PLACE_KEYS}
    order = ("seq_place_off", "place_unitig", "place_flag", "place_pos", "place_q0", "place_len")
    pattern = torch.arange(4 * B, dtype=torch.int32, device="cuda") * 7 + 3

    def pile(bases_=graph["bases"], off_=graph["offsets"], **over):
        p = dict(places)
        for k, (j, v) in over.items():
            p[k] = places[k].clone()
            p[k][j] = v
        counts, mism, stats = pattern.clone(), poison(R, torch.int32), poison(3, torch.int64)
        status = L.aix_pileup_dev(q(st), q(so), 2, q(p[order[0]]), R, *[q(p[k]) for k in order[1:]], U, q(off_), q(bases_), q(counts), q(mism), q(stats), None)
        torch.cuda.synchronize()
        return status, counts, mism, stats

    status, counts, mism, stats = pile()
    wc = PR.pile(seqs, wp, off, bases, _np(pattern))
    assert status == 0 and np.array_equal(_np(counts), wc["counts"]) and np.array_equal(_np(mism[:R]), wc["place_mism"]) and clean(mism[R:]) and clean(stats[3:])
    lower = graph["bases"].clone()
    lower[299] |= 0x20
    for what, kw in (("broken CSR", dict(seq_place_off=(1, 3))), ("u = U", dict(place_unitig=(1, U))), ("beyond the contig", dict(place_pos=(1, 31))),
                     ("q0 + len beyond the read", dict(place_q0=(0, 1))), ("len = 0", dict(place_len=(1, 0))), ("a lower-case contig byte", dict(bases_=lower)),
                     ("offsets", dict(off_=bad_off))):
        status, counts, mism, stats = pile(**kw)
        assert status == ARG and torch.equal(counts, pattern) and clean(mism) and clean(stats), what
    for bases_, off_ in ((lower, graph["offsets"]), (graph["bases"], bad_off)):
        outs = [poison(B, torch.uint8), poison(U, torch.int64), poison(U, torch.int32)]
        n = C.c_uint64(77)
        g_ = {"offsets": off_, "bases": bases_}
        assert L.aix_pile_call_dev(U, q(off_), q(bases_), q(counts), 8, 700, 3, 200, q(outs[0]), C.byref(n), *[None] * 7, 0, None, q(outs[1]), q(outs[2]), None) == ARG
        torch.cuda.synchronize()
        assert n.value == 77 and all(clean(t) for t in outs)
        status, tot, vouts, vclean = _raw_call(g_, counts, 8)
        assert status == ARG and tot == 77 and all(vclean(t) for t in vouts)
    torch.cuda.synchronize()


def test_planted_case_end_to_end(tmp_path):
    """5. The planted heterozygous genome through AIndex on a written index: the 39 sites and no other, nothing polished, the VCF."""
    from aindex_amd.aindex import AIndex, format_vcf
    p = PC.planted()
    prefix = _write_index(str(tmp_path / "planted"), p["codes"], p["tfs"])
    a = AIndex.load_23mer_index(prefix + ".pf", prefix + ".tf.bin", prefix + ".kmers.bin")
    try:
        contigs = a.get_contigs(cutoff=1)
        assert [len(s) for s, _, _ in contigs] == [PC.GENOME]
        sites = PC.expected_sites(p, contigs[0][0])
        got = a.get_variants(p["reads"], cutoff=1)
        assert [(c, x, r, alt) for c, x, r, alt, _, _, _ in got] == [(0, x, r, alt) for x, r, alt in sites]
        assert all(d == 30 and rn >= 19 and an >= 9 for _, _, _, _, rn, an, d in got)
        assert a.get_polished_contigs(p["reads"], cutoff=1) == contigs
        out = str(tmp_path / "planted.vcf")
        assert a.write_variants_vcf(out, p["reads"], cutoff=1) == 39
        lines = open(out).read().splitlines()
        assert lines == list(format_vcf(got, [PC.GENOME])) and lines[1] == "##contig=<ID=c0,length=4000>"
        body = [l.split("\t") for l in lines if l[0] != "#"]
        assert [(f[0], int(f[1]), f[3], f[4]) for f in body] == [("c0", x + 1, r, alt) for x, r, alt in sites]
        assert all(f[7] == "DP=%d;AD=%d,%d" % (d, rn, an) for f, (_, _, _, _, rn, an, d) in zip(body, got))
        pile = a.get_pileup(p["reads"], cutoff=1)
        assert pile["counts"].shape == (PC.GENOME, 4) and pile["counts"].dtype == np.uint32 and pile["depth_sum"].tolist() == [int(pile["counts"].sum())]
        assert pile["stats"][0] == int(pile["counts"].sum()) and pile["uncovered"].tolist() == [0]
        rows = a.get_read_placements(p["reads"][:50], cutoff=1)
        assert len(rows) == 50 and all(len(r) == 1 and r[0][0] == 0 and r[0][4] == PC.READ for r in rows) and {r[0][1] for r in rows} == {"+", "-"}
        fa = str(tmp_path / "polished.fa")
        assert a.write_polished_contigs(fa, p["reads"], cutoff=1) == 1
        head, seq = open(fa).read().splitlines()
        assert head.startswith(">c0 LN:i:4000 ") and head.endswith(" PC:i:0") and seq == contigs[0][0]
    finally:
        a._wrapper.close()
