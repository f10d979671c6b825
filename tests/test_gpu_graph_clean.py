"""Graph cleaning on the GPU (k_gc_* of aix_graphclean.hip) against the test-side restatement (tests/graph_clean_ref.py, pinned by
test_graph_clean_cpu.py) and the array checker (tests/graph_clean_check.py). Every comparison is exact equality."""
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
import graph_clean_check as GK
import graph_clean_ref as GR
import oracle_lib as O
import test_graph_clean_cpu as TC
import unitig_links_cases as LC
import unitig_links_ref as RL
import unitigs_cases as UC
import unitigs_ref as R
from aindex_amd import _lib, builder
from aindex_amd.engine import Index

vp = _lib.vp
SEEDS = (0, 3, 6, 9)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE32 = GR.NONE32
ALL_KEYS = GR.GRAPH_KEYS + GR.MAP_KEYS
CHAINS = (1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 5000)
RINGS = (2, 3, 64, 4096, 4097)
P64, P32, P8 = 0x6B6B6B6B6B6B6B6B, 0x6B6B6B6B, 0x6B


def _open(prefix):
    return Index.open_23(prefix + ".pf", prefix + ".tf.bin", prefix + ".kmers.bin")


def _numpy(d):
    return Index._graph_to_host(d)


def _ref_graph(ix, cutoff):
    codes, tfs = ix.checker_array() & np.uint64(R.MASK), ix.tf_array()
    un = R.unitigs(codes, tfs, cutoff)
    return un, GR.graph(un, RL.links(codes, tfs, cutoff, un))


def _device_graph(ix, cutoff):
    un = ix.unitigs_t(cutoff)
    return un, ix.unitig_links_t(cutoff, unitigs=un)


def _same(got, want, tag, keys=ALL_KEYS):
    got = _numpy(got)
    assert got["U"] == want["C"] and got["E"] == want["E"], tag
    for k in keys:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (tag, k)
    if "n_circular" in got:
        assert got["n_circular"] == want["n_circular"] and np.array_equal(got["bubble_mate"], want["bubble_mate"]), tag


def _masks(U, seed):
    rng = np.random.default_rng(seed)
    but_one = np.ones(U, np.uint8)
    if U:
        but_one[int(rng.integers(0, U))] = 0
    return (("zero", np.zeros(U, np.uint8)), ("10 %", (rng.random(U) < 0.1).astype(np.uint8)), ("50 %", (rng.random(U) < 0.5).astype(np.uint8)),
            ("all", np.ones(U, np.uint8)), ("all but one", but_one))


def _all_forms(ix, cutoff, tag, masks=True):
    """mark, compact and one whole round, device and host forms, against the restatement; property (a); random masks"""
    import torch
    un, g = _ref_graph(ix, cutoff)
    ud, ld = _device_graph(ix, cutoff)
    want_rm = GR.mark(g, 46, 46)
    rm, tips, arms = ix.graph_mark_t(ud, ld, 46, 46)
    assert np.array_equal(rm.cpu().numpy(), want_rm) and (tips, arms) == (int((want_rm == 1).sum()), int((want_rm == 2).sum())), tag
    assert np.array_equal(ix.graph_mark(g, None, 46, 46), want_rm), tag
    todo = (("mark", want_rm),) + (_masks(g["U"], 77) if masks else (("zero", np.zeros(g["U"], np.uint8)),))
    for name, mask in todo:
        want = GR.compact(g, mask)
        got = ix.graph_compact_t(ud, ld, torch.from_numpy(mask).cuda())
        _same(got, want, (tag, name, "device"))
        if name == "zero":                                          # property (a): G' == G and the map is the identity
            for k in GR.GRAPH_KEYS:
                assert np.array_equal(_numpy(got)[k], g[k]), (tag, k)
            assert _numpy(got)["unitig_contig"].tolist() == list(range(g["U"])) and not bool(got["unitig_pos"].any()) and not bool(got["unitig_flag"].any())
        if name in ("mark", "50 %"):
            _same(ix.graph_compact(g, None, mask), want, (tag, name, "host"))
    want = GR.compact(g, want_rm)
    h = ix.graph_clean_round(g, 46, 46)
    _same(h, want, (tag, "aix_graph_clean"))
    assert np.array_equal(h["remove"], want_rm) and (h["n_tips"], h["n_arms"]) == (tips, arms)
    return g, want_rm, want


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("gc"))
    return {seed: G.write_graph_case(seed, d)[0] for seed in SEEDS}


def _extra_cases():
    codes, tfs = TC._lollipop_two_stems()
    fork = TC._fork(5, 5)
    return {"two_stems": UC.Case(codes, tfs, None), "fork_equal_means": UC.Case(fork[0], fork[1], None)}


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    """name -> prefix of the index files of a topology case, a planted link case or one of the two cases of this file, built when first asked for"""
    d = str(tmp_path_factory.mktemp("gct"))
    every, made = dict(UC.topology_cases()), {}
    every.update(LC.link_cases())
    every.update(_extra_cases())

    def get(name):
        if name not in made:
            case = every[name]
            prefix = os.path.join(d, name)
            open(prefix + ".pf", "wb").write(builder.build_pf_codes(case.codes, 23))
            rc, checker, tf = O.index_scatter(O.OracleMphf(prefix + ".pf"), np.ascontiguousarray(D.decode(case.codes)).reshape(-1), case.tfs)
            assert rc == 0
            checker.tofile(prefix + ".kmers.bin")
            tf.tofile(prefix + ".tf.bin")
            made[name] = prefix
        return made[name]
    return get


NAMES = sorted(set(UC.topology_cases()) | set(LC.link_cases()) | {"two_stems", "fork_equal_means"})


@pytest.mark.parametrize("seed", SEEDS)
def test_graph_cases_every_form(cases, seed):
    """1. Graph cases at cutoffs 0 and 3: mark, compact (the mark, property (a), random masks of 10 %, 50 %, all, all but one), one whole
    round; device and host forms."""
    with _open(cases[seed]) as ix:
        for cutoff in (0, 3):
            g, rm, want = _all_forms(ix, cutoff, (seed, cutoff))
            if cutoff == 0:                                         # the case cannot pass vacuously
                assert (rm == 1).sum() > 5 and want["n_circular"] > 0 and (want["unitig_flag"] & 1).any() and want["C"] < g["U"] - 5


@pytest.mark.parametrize("name", NAMES)
def test_planted_cases_every_form(planted, name):
    """2. Every topology case, every planted link case, the ring with two stems and the fork with equal means, at cutoff 0 (and 3 where the
    case has structure there)."""
    with _open(planted(name)) as ix:
        for cutoff in (0, 3) if name in ("bubble_tip_cutoff", "opened_circle", "many_circles", "hairpin_ends") else (0,):
            g, rm, want = _all_forms(ix, cutoff, (name, cutoff), masks=name != "isolated")
            GK.check(g, rm, want)
        if name == "two_stems":
            assert want["C"] == 1 and want["circular"].tolist() == [1] and (want["unitig_flag"][rm == 0] & 2).all()
        if name == "lollipop":
            assert want["circular"].tolist() == [1] * len(UC.LOLLIPOPS)


# ---- planted chains and rings ------------------------------------------------------------------------------------------------------
def _window_codes(seq: np.ndarray) -> np.ndarray:
    """the 46-bit codes of every 23-window of a sequence of values 0 .. 3, and of their reverse complements"""
    n = seq.shape[0] - 22
    f, r = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    s = seq.astype(np.uint64)
    for j in range(23):
        f = (f << np.uint64(2)) | s[j:j + n]
        r = r | ((np.uint64(3) - s[j:j + n]) << np.uint64(2 * j))
    return f, r


def _planted_chains(seed=20260):
    """paths cut into CHAINS unitigs and circles cut into RINGS unitigs by one-k-mer tips (tf 1 against tf 5) about every 30 k-mers; one
    member of the chain of three is the path of 20 001 k-mers. -> (codes ascending, tfs, path strings, [(ring k-mers, pieces)])"""
    rng = np.random.default_rng(seed)
    while True:
        seqs, tips, paths, rings = [], [], [], []
        for j in CHAINS:
            pieces = [int(v) for v in rng.integers(28, 33, j)]
            if j == 3:
                pieces[1] = max(UC.PATHS)
            if j > 1:
                pieces[0] += 20
                pieces[-1] += 20                                    # the end pieces are longer than any threshold of the tests
            seq = rng.integers(0, 4, sum(pieces) + 22)
            cuts = np.cumsum(pieces)[:-1]
            seqs.append(seq)
            paths.append(seq)
            for p in cuts.tolist():                                 # the tip leaves behind k-mer p - 1, beside k-mer p
                tips.append(np.concatenate([seq[p:p + 22], [(seq[p + 22] + 1 + rng.integers(0, 3)) % 4]]))
        for j in RINGS:
            pieces = [int(v) for v in rng.integers(28, 33, j)]
            m = sum(pieces)
            unit = rng.integers(0, 4, m)
            seq = np.tile(unit, 23 // m + 2)[:m + 22]
            seqs.append(seq)
            rings.append((m, j))
            for p in np.concatenate([[0], np.cumsum(pieces)[:-1]]).tolist():
                tips.append(np.concatenate([seq[p:p + 22], [(seq[p + 22] + 1 + rng.integers(0, 3)) % 4]]))
        codes, tfs = [], []
        for s, tf in [(s, 5) for s in seqs] + [(s, 1) for s in tips]:
            f, r = _window_codes(np.asarray(s))
            codes.append(np.minimum(f, r))
            tfs.append(np.full(f.shape[0], tf, np.uint32))
        codes, tfs = np.concatenate(codes), np.concatenate(tfs)
        uniq, first = np.unique(codes, return_index=True)
        if uniq.shape[0] == codes.shape[0]:                         # else a k-mer was met twice: draw again
            return uniq, tfs[first], ["".join("ACGT"[b] for b in p.tolist()) for p in paths], rings


def _index_of(codes, tfs):
    """an index over (codes ascending, tfs), built on the device: the helper of the unitig GPU tests"""
    import torch
    keys = torch.from_numpy(codes.astype(np.int64)).cuda()
    ix = Index.build_23_codes_t(builder.build_pf_codes_t(keys, 23), keys, torch.from_numpy(tfs.astype(np.int32)).cuda())
    torch.cuda.synchronize()
    return ix


def test_planted_chains_and_rings():
    """3. Clipping merges chains of exactly CHAINS unitigs (some members reversed, one member the path of 20 001 k-mers: the emission is
    balanced per output byte) and rings of exactly RINGS unitigs (the cycle phase, rounds that are no power of two). The contigs must be
    the planted paths, byte for byte; the rings and every array are held to the checker."""
    rc = lambda s: s[::-1].translate(str.maketrans("ACGT", "TGCA"))
    codes, tfs, paths, rings = _planted_chains()
    ix = _index_of(codes, tfs)
    try:
        ud, ld = _device_graph(ix, 0)
        n_tips = sum(j - 1 for j in CHAINS) + sum(RINGS)
        assert ud["U"] == sum(CHAINS) + sum(RINGS) + n_tips and ud["n_circular"] == 0
        rm, tips, arms = ix.graph_mark_t(ud, ld, 46, 46)
        assert (tips, arms) == (n_tips, 0)
        got = ix.graph_compact_t(ud, ld, rm)
        g, out, remove = _numpy({k: (ud[k] if k in ud else ld[k]) for k in GR.GRAPH_KEYS}), _numpy(got), rm.cpu().numpy()
        GK.check(g, remove, out)
        assert out["U"] == len(CHAINS) + len(RINGS) and out["E"] == 0 and out["n_circular"] == len(RINGS)
        members = np.bincount(out["unitig_contig"][remove == 0], minlength=out["U"])
        lin = out["circular"] == 0
        assert sorted(members[lin].tolist()) == sorted(CHAINS) and sorted(members[~lin].tolist()) == sorted(RINGS)
        flags = out["unitig_flag"][remove == 0]
        assert (flags & 1).any() and not (flags & 1).all() and ((flags & 2) != 0).sum() == sum(RINGS)
        off, text = out["offsets"].tolist(), out["bases"].tobytes().decode("ascii")
        strings = [text[off[c]:off[c + 1]] for c in range(out["U"])]
        want = sorted((min(p, rc(p), key=lambda s: GR.code23(s.encode())) for p in paths), key=lambda s: GR.code23(s.encode()))
        assert [s for s, l in zip(strings, lin.tolist()) if l] == want
        assert sorted(len(s) - 22 for s, l in zip(strings, lin.tolist()) if not l) == sorted(m for m, _ in rings)
        assert out["tf_sum"].tolist() == [5 * (len(s) - 22) for s in strings] and (out["tf_min"] == 5).all() and (out["tf_max"] == 5).all()
        m_in = np.diff(g["offsets"].astype(np.int64)) - 22
        assert m_in.max() == max(UC.PATHS) and remove[int(np.argmax(m_in))] == 0
        h = ix.graph_clean_round(g, 46, 46)                          # the host form on the same arrays
        for k in ALL_KEYS:
            assert np.array_equal(h[k], out[k]), k
        again, rounds = ix.graph_clean_t(got, None, 46, 46, 3)      # nothing is left to clean
        assert rounds == 0 and again["U"] == out["U"]
    finally:
        ix.close()


# ---- launch geometry ----------------------------------------------------------------------------------------------------------------
_CHILD = """
import hashlib, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from aindex_amd.engine import Index
h = hashlib.sha256()
for p in sys.argv[2:]:
    with Index.open_23(p + ".pf", p + ".tf.bin", p + ".kmers.bin") as ix:
        for cutoff in (0, 3):
            g = dict(ix.unitigs(cutoff))
            g.update(ix.unitig_links(cutoff))
            out = ix.graph_clean_round(g, 46, 46)
            for k in %r:
                h.update(np.ascontiguousarray(out[k]).tobytes())
print("digest", h.hexdigest())
""" % (ALL_KEYS + ("remove",),)


def test_many_trips_of_every_loop(cases, planted, monkeypatch):
    """4. AIX_UG_TEST_GRID = 1, 2, 3 workgroups for every launch: in this process (the switch is read per call) for the device forms, and in
    fresh child processes for the host form; the same bytes as the restatement."""
    import torch
    names = ("two_stems", "lollipop", "bubble_tip_cutoff", "tip_of_one", "many_circles", "fork_equal_means")
    prefixes = [cases[3]] + [planted(nm) for nm in names]
    h = hashlib.sha256()
    opened = []
    try:
        sets = []
        for prefix in prefixes:
            ix = _open(prefix)
            opened.append(ix)
            for cutoff in (0, 3):
                un, g = _ref_graph(ix, cutoff)
                rm = GR.mark(g, 46, 46)
                want = GR.compact(g, rm)
                sets.append((ix, cutoff, rm, want))
                for k in ALL_KEYS:
                    h.update(np.ascontiguousarray(want[k]).tobytes())
                h.update(rm.tobytes())
        for grid in ("1", "2", "3"):
            monkeypatch.setenv("AIX_UG_TEST_GRID", grid)
            for ix, cutoff, rm, want in sets:
                ud, ld = _device_graph(ix, cutoff)
                got_rm = ix.graph_mark_t(ud, ld, 46, 46)[0]
                assert np.array_equal(got_rm.cpu().numpy(), rm), (grid, cutoff)
                _same(ix.graph_compact_t(ud, ld, got_rm), want, (grid, cutoff))
        monkeypatch.delenv("AIX_UG_TEST_GRID")
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


# ---- refusals and canaries ------------------------------------------------------------------------------------------------------------
def test_poison_behind_every_output_and_refusals(planted):
    """5. 64 poisoned elements behind every output stay as they are; every refusal of the contract leaves every output untouched."""
    import torch
    L = _lib.lib()
    ARG, UNS = _lib.AIX_ERR_ARG, _lib.AIX_ERR_UNSUPPORTED
    q = lambda t: vp(t.data_ptr()) if t is not None else None
    poison = {torch.int64: P64, torch.int32: P32, torch.uint8: P8}

    def buf(n, dtype):
        return torch.full((n + 64,), poison[dtype], dtype=dtype, device="cuda")

    def clean(t, n=0):
        return bool((t[n:] == poison[t.dtype]).all())

    with _open(planted("bubble_tip_cutoff")) as ix:
        un, g = _ref_graph(ix, 0)
        ud, ld = _device_graph(ix, 0)
        G0 = {k: (ud[k] if k in ud else ld[k]) for k in GR.GRAPH_KEYS}
        U, E = g["U"], g["E"]
        want_rm = GR.mark(g, 46, 46)
        want = GR.compact(g, want_rm)
        Cn, total, E2 = want["C"], int(want["offsets"][-1]), want["E"]

        def mark(G_, U_=U, E_=E, tip=46, bub=46, mate=None):
            rm = buf(U, torch.uint8)
            n = [C.c_uint64(77), C.c_uint64(77)]
            st = L.aix_graph_mark_dev(U_, q(G_["offsets"]), q(G_["circular"]), q(G_["tf_sum"]), q(G_["link_off"]), q(G_["link_to"]), E_, q(mate), tip, bub, q(rm),
                                      C.byref(n[0]), C.byref(n[1]), None)
            torch.cuda.synchronize()
            return st, rm, [x.value for x in n]

        def layout(G_, rm, U_=U, E_=E):
            outs = [buf(U, torch.int32), buf(U, torch.int64), buf(U, torch.uint8)]
            n = [C.c_uint64(77) for _ in range(4)]
            st = L.aix_graph_compact_layout_dev(U_, q(G_["offsets"]), q(G_["bases"]), q(G_["circular"]), q(G_["link_off"]), q(G_["link_to"]), E_, q(rm),
                                                *[q(t) for t in outs], *[C.byref(x) for x in n], None)
            torch.cuda.synchronize()
            return st, outs, [x.value for x in n]

        def emit(G_, rm, m, sizes=(Cn, total, E2), U_=U, E_=E, shift=0):
            c, t, e = sizes
            types = (torch.int64, torch.uint8, torch.uint8, torch.int64, torch.int32, torch.int32, torch.int64, torch.int32)
            outs = [buf(n + (16 if i == 1 else 0), ty) for i, (n, ty) in enumerate(zip((Cn + 1, total, Cn, Cn, Cn, Cn, 2 * Cn + 1, E2), types))]
            ptrs = [q(t) for t in outs]
            if shift:
                ptrs[1] = vp(outs[1].data_ptr() + shift)
            st = L.aix_graph_compact_emit_dev(U_, *[q(G_[k]) for k in GR.GRAPH_KEYS], E_, q(rm), *[q(t) for t in m], c, t, e, *ptrs, None)
            torch.cuda.synchronize()
            return st, outs

        # the calls as they should be: exact outputs, poison intact behind them
        st, rm, n = mark(G0)
        assert st == 0 and np.array_equal(rm[:U].cpu().numpy(), want_rm) and clean(rm, U) and n == [1, 1]
        st, rm2, n = mark(G0, mate=ld["bubble_mate"])
        assert st == 0 and torch.equal(rm, rm2)
        rm_t = rm[:U].clone()
        st, m, n = layout(G0, rm_t)
        assert st == 0 and n == [Cn, total, E2, want["n_circular"]] and all(clean(t, U) for t in m)
        for t, k in zip(m, GR.MAP_KEYS):
            assert np.array_equal(_numpy({k: t[:U]})[k], want[k]), k
        m = [t[:U].clone() for t in m]
        st, outs = emit(G0, rm_t, m)
        assert st == 0
        for t, k, n_ in zip(outs, GR.GRAPH_KEYS, (Cn + 1, total, Cn, Cn, Cn, Cn, 2 * Cn + 1, E2)):
            assert np.array_equal(_numpy({k: t[:n_]})[k], want[k]) and clean(t, n_), k

        untouched_mark = lambda r: r[0] in (ARG, UNS) and clean(r[1]) and r[2] == [77, 77]
        untouched_layout = lambda r: r[0] in (ARG, UNS) and all(clean(t) for t in r[1]) and r[2] == [77] * 4
        untouched_emit = lambda r: r[0] in (ARG, UNS) and all(clean(t) for t in r[1])

        def every(G_, rm=rm_t, status=ARG, **kw):
            r = mark(G_, **kw)
            assert untouched_mark(r) and r[0] == status
            r = layout(G_, rm, **kw)
            assert untouched_layout(r) and r[0] == status
            r = emit(G_, rm, m, **kw)
            assert untouched_emit(r) and r[0] == status

        def changed(key, fn):
            G_ = dict(G0)
            G_[key] = G0[key].clone()
            fn(G_[key])
            return G_

        def set_(i, v):
            def fn(t):
                t[i] = v
            return fn

        every(changed("offsets", set_(1, int(g["offsets"][0]) + 22)))                                                         # unitig 0 keeps 22 bases
        every(changed("offsets", set_(2, int(g["offsets"][1]))))                                                               # not ascending
        every(changed("link_to", set_(0, 2 * U)))                                                                              # a link word >= 2 U
        every(changed("link_to", set_(0, -1)))
        every(changed("link_off", set_(1, E + 1)))                                                                             # an offset beyond E
        every(changed("link_off", set_(2 * U, E - 1)))
        linked = int(g["link_to"][0]) >> 1
        every(changed("circular", set_(linked, 1)))                                                                            # a link of a circular unitig
        src = np.repeat(np.arange(2 * U), np.diff(g["link_off"].astype(np.int64)))
        i = int(np.nonzero((want_rm[src >> 1] == 0) & (want_rm[g["link_to"] >> 1] == 0))[0][0])
        every(changed("link_to", set_(i, int(g["link_to"][i]) ^ 1)))                                                           # a surviving link without its dual
        every(G0, status=UNS, U_=2 ** 31 - 3)
        every(G0, U_=U, E_=8 * U + 1)
        assert untouched_mark(mark(G0, tip=32768)) and untouched_mark(mark(G0, bub=32768))
        bad_mate = ld["bubble_mate"].clone()
        bad_mate[int(np.nonzero(want_rm == 2)[0][0])] = -1                                                                    # not symmetric
        assert untouched_mark(mark(G0, mate=bad_mate))
        # a removed unitig takes its links with it: the dual of a link that does not survive is not asked for
        lone = changed("link_to", set_(i, int(g["link_to"][i]) ^ 1))
        gone = torch.ones(U, dtype=torch.uint8, device="cuda")
        assert layout(lone, gone)[0] == 0 and untouched_mark(mark(lone))
        # the emit holds the map against the graph and the sizes
        for key, i, v in (("contig", 0, Cn), ("pos", int(np.argmax(want["unitig_pos"])), 1), ("flag", int(np.argmax(want["unitig_pos"])), 1)):
            mm = [t.clone() for t in m]
            j = ("contig", "pos", "flag").index(key)
            mm[j][i] = (mm[j][i] ^ v) if key == "flag" else (v if key == "contig" else mm[j][i] + v)
            assert untouched_emit(emit(G0, rm_t, mm)), key
        assert untouched_emit(emit(G0, rm_t, m, sizes=(Cn + 1, total + 22, E2)))
        assert untouched_emit(emit(G0, rm_t, m, sizes=(Cn, total + 1, E2)))
        assert untouched_emit(emit(G0, rm_t, m, sizes=(Cn, total, E2 + 1)))
        assert untouched_emit(emit(G0, torch.zeros(U, dtype=torch.uint8, device="cuda"), m))                                  # another mask
        assert untouched_emit(emit(G0, rm_t, m, shift=8))                                                                      # d_out_bases not aligned to 16
        # U == 0
        z = {k: torch.zeros(1 if k in ("offsets", "link_off") else 0, dtype=G0[k].dtype, device="cuda") for k in GR.GRAPH_KEYS}
        e = torch.zeros(0, dtype=torch.uint8, device="cuda")
        got = ix.graph_compact_t(z, None, e)
        assert got["U"] == 0 and got["E"] == 0 and got["offsets"].tolist() == [0] and got["link_off"].tolist() == [0]
        assert ix.graph_mark_t(z)[1:] == (0, 0) and ix.graph_clean_t(z, None, 46, 46, 3)[1] == 0
    torch.cuda.synchronize()


def test_side_stream(cases):
    """6. Mark, layout and emit on a side stream; the graph made on one stream and cleaned on another."""
    import torch
    with _open(cases[6]) as ix:
        un, g = _ref_graph(ix, 0)
        rm = GR.mark(g, 46, 46)
        want = GR.compact(g, rm)
        a, b = torch.cuda.Stream(), torch.cuda.Stream()
        with torch.cuda.stream(a):
            ud, ld = _device_graph(ix, 0)
            got, rounds = ix.graph_clean_t(ud, ld, 46, 46, 1)
        a.synchronize()
        _same(got, want, "side stream")
        assert rounds == 1
        with torch.cuda.stream(b):
            got = ix.graph_compact_t(ud, ld, ix.graph_mark_t(ud, ld)[0])
        b.synchronize()
        _same(got, want, "graph on one stream, cleaning on another")


# ---- a natural index -------------------------------------------------------------------------------------------------------------------
def _midsize_text(rng, planted_codes):
    """plain text (records end with a newline): a 200 kbp genome, 150-bp reads of either strand at 8 x over its first 30 kbp with 0.5 %
    substitutions, and the keys of the planted bubble cases as 23-base records (the text of test_gpu_unitig_links.py)"""
    nl = np.array([10], np.uint8)
    g = rng.integers(0, 4, 200_000).astype(np.uint8)
    parts = [D.LETTERS[g], nl]
    n_reads = 8 * 30_000 // 150
    reads = g[rng.integers(0, 30_000 - 150, n_reads)[:, None] + np.arange(150)[None, :]]
    reads = np.where(rng.random(reads.shape) < 0.005, (reads + rng.integers(1, 4, reads.shape)) % 4, reads).astype(np.uint8)
    flip = rng.random(n_reads) < 0.5
    reads[flip] = (3 - reads[flip])[:, ::-1]
    parts.append(np.concatenate([D.LETTERS[reads], np.full((n_reads, 1), 10, np.uint8)], axis=1).reshape(-1))
    parts.append(np.concatenate([D.decode(planted_codes), np.full((planted_codes.shape[0], 1), 10, np.uint8)], axis=1).reshape(-1))
    return np.concatenate(parts)


def test_natural_midsize_index_reaches_a_fixed_point():
    """7. The index of about 2.2 x 10^5 keys of test_gpu_unitig_links.py: every round of graph_clean_t(rounds = 3) is held to the array
    checker, the result is a fixed point, aix_unitig_bubbles_dev and format_gfa work on it; property (b) once on a real second index,
    opened over the surviving k-mers of the first round."""
    import torch
    from aindex_amd import counting
    from aindex_amd.aindex import format_gfa
    rc = lambda s: s[::-1].translate(str.maketrans("ACGT", "TGCA"))
    link = LC.link_cases()
    extra = np.concatenate([link[nm].codes for nm in ("bubble_snp", "bubble_indel", "degrees_0_to_4")])
    plain = _midsize_text(np.random.default_rng(20252), extra)
    keys, counts = counting.count_distinct_t(torch.from_numpy(plain).cuda(), 23, _lib.CANON_TRUE_RC)
    ix = Index.build_23_codes_t(builder.build_pf_codes_t(keys, 23), keys, counts.to(torch.int32))
    torch.cuda.synchronize()
    second = None
    try:
        assert 10 ** 5 <= ix.n <= 3 * 10 ** 5 and ix.canonical_only
        ud, ld = _device_graph(ix, 0)
        g = {k: (ud[k] if k in ud else ld[k]) for k in GR.GRAPH_KEYS}
        first = None
        for rnd in range(3):
            rm, tips, arms = ix.graph_mark_t(g, None, 46, 46)
            print("round", rnd, "U", g["offsets"].numel() - 1, "E", g["link_to"].numel(), "tips", tips, "arms", arms)
            if tips + arms == 0:
                break
            out = ix.graph_compact_t(g, None, rm)
            GK.check(_numpy(g), rm.cpu().numpy(), _numpy(out))
            if first is None:
                first = (rm, out)
                assert tips > 100 and arms > 2 and out["U"] < ud["U"] - tips - arms
            g = out
        final, rounds = ix.graph_clean_t(ud, ld, 46, 46, 3)
        for k in GR.GRAPH_KEYS:
            assert torch.equal(final[k], g[k]), k
        rm, tips, arms = ix.graph_mark_t(final, None, 46, 46)
        print("after", rounds, "rounds: U", final["U"], "E", final["E"], "tips", tips, "arms", arms)
        assert tips + arms == 0 and 1 <= rounds <= 3                 # a fixed point
        fh = _numpy(final)
        GK.check_graph(fh)
        assert np.array_equal(fh["bubble_mate"], np.array(GR.bubbles(fh["U"], fh["link_off"], fh["link_to"]), np.uint32))
        seg, n_links = {}, 0
        for ln in format_gfa(fh, fh):
            f = ln.split("\t")
            if f[0] == "S":
                seg[f[1]] = f[2]
            elif f[0] == "L":
                n_links += 1
                a, b = seg[f[1]], seg[f[3]]
                assert f[5] == "22M" and (a if f[2] == "+" else rc(a))[-22:] == (b if f[4] == "+" else rc(b))[:22]
        assert len(seg) == fh["U"] and n_links > 0
        # property (b): a second index over the k-mers of the unitigs that survive the first round
        rm1, out1 = first
        codes, tfs = ix.checker_array() & np.uint64(R.MASK), ix.tf_array()
        ku = ud["kid_unitig"].cpu().numpy()
        keep = (tfs > 0) & (rm1.cpu().numpy()[np.where(tfs > 0, ku, 0)] == 0)
        order = np.argsort(codes[keep])
        second = _index_of(codes[keep][order], tfs[keep][order])
        u2, l2 = _device_graph(second, 0)
        a = GR.canonical_form(GR.graph(_numpy(out1), _numpy(out1)))
        b = GR.canonical_form(GR.graph(_numpy(u2), _numpy(l2)))
        assert a["strings"] == b["strings"]
        for k in ("offsets", "circular", "tf_sum", "tf_min", "tf_max", "link_off", "link_to"):
            assert np.array_equal(a[k], b[k]), k
    finally:
        ix.close()
        if second is not None:
            second.close()


def test_list_surface(planted, tmp_path):
    """8. get_contigs, write_contigs and write_contigs_gfa."""
    from aindex_amd.aindex import AIndex
    prefix = planted("bubble_tip_cutoff")
    ai = AIndex.load_23mer_index(prefix + ".pf", prefix + ".tf.bin", prefix + ".kmers.bin")
    try:
        ix = ai._wrapper._need23()
        un, g = _ref_graph(ix, 0)
        want, _ = GR.clean(g, 46, 46, 3)
        assert want["C"] == 1
        assert ai.get_contigs() == [(want["strings"][0], int(want["tf_sum"][0]), False)] and ai.get_contigs(min_kmers=80) == []
        assert ai.get_contigs(tip_max_kmers=0, bubble_max_kmers=0) == ai.get_unitigs()
        path = str(tmp_path / "c.fa")
        assert ai.write_contigs(path) == 1
        s = want["strings"][0]
        assert open(path).read() == f">c0 LN:i:{len(s)} KC:i:{int(want['tf_sum'][0])} km:f:{int(want['tf_sum'][0]) / (len(s) - 22):.1f}\n{s}\n"
        assert ai.write_contigs_gfa(str(tmp_path / "c.gfa")) == (1, 0)
        assert open(str(tmp_path / "c.gfa")).read().split("\n")[1].split("\t")[:3] == ["S", "u0", s]
    finally:
        ai._wrapper.close()
