"""The unitig graph on the GPU (k_ul_* of aix_unitigs.hip) against the test-side restatement (tests/unitig_links_ref.py, pinned by
test_unitig_links_cpu.py) and the array checker (tests/unitig_links_check.py). Every comparison is exact equality."""
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
import oracle_lib as O
import unitig_links_cases as LC
import unitig_links_check as LK
import unitig_links_ref as RL
import unitigs_cases as UC
import unitigs_ref as R
from aindex_amd import _lib, builder
from aindex_amd.engine import Index

vp = _lib.vp
SEEDS = (0, 3, 6, 9)
CUTOFFS = (0, 3, 2 ** 32 - 1)
ARRAYS = ("link_off", "link_to", "bubble_mate")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE32 = RL.NONE32


def _open(prefix):
    return Index.open_23(prefix + ".pf", prefix + ".tf.bin", prefix + ".kmers.bin")


def _host(t):
    a = t.cpu().numpy()
    return a.view({np.dtype(np.int64): np.uint64, np.dtype(np.int32): np.uint32}.get(a.dtype, a.dtype))


def _numpy(d):
    return {k: (_host(v) if hasattr(v, "cpu") else v) for k, v in d.items()}


def _ref(ix, cutoff):
    codes, tfs = ix.checker_array() & np.uint64(R.MASK), ix.tf_array()
    un = R.unitigs(codes, tfs, cutoff)
    return un, RL.links(codes, tfs, cutoff, un)


def _same(got, want, tag):
    got = _numpy(got)
    assert got["U"] == want["U"] and got["E"] == want["E"], tag
    for k in ARRAYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (tag, k)


def _digest(lk):
    h = hashlib.sha256()
    for k in ARRAYS:
        h.update(np.ascontiguousarray(lk[k]).tobytes())
    return h.hexdigest()


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("ul"))
    return {seed: G.write_graph_case(seed, d)[0] for seed in SEEDS + (1,)}


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    """name -> {"prefix", "case", "codes", "tfs", "cutoffs", "want": cutoff -> (un, lk)}: the topology cases of the compaction and the planted
    link cases as index files, each built and answered once, when a test first asks for it"""
    d = str(tmp_path_factory.mktemp("ult"))
    topo, link, made = UC.topology_cases(), LC.link_cases(), {}

    def get(name):
        if name not in made:
            case = link[name] if name in link else topo[name]
            cutoffs = case.cutoffs if name in link else UC.topology_cutoffs(name)
            prefix = os.path.join(d, name)
            open(prefix + ".pf", "wb").write(builder.build_pf_codes(case.codes, 23))
            rc, checker, tf = O.index_scatter(O.OracleMphf(prefix + ".pf"), np.ascontiguousarray(D.decode(case.codes)).reshape(-1), case.tfs)
            assert rc == 0
            checker.tofile(prefix + ".kmers.bin")
            tf.tofile(prefix + ".tf.bin")
            codes = checker & np.uint64(R.MASK)
            want = {}
            for c in cutoffs:
                un = R.unitigs(codes, tf, c)
                want[c] = (un, RL.links(codes, tf, c, un))
            made[name] = {"prefix": prefix, "case": case, "codes": codes, "tfs": tf, "cutoffs": cutoffs, "want": want}
        return made[name]
    return get


NAMES = sorted(set(UC.topology_cases()) | set(LC.link_cases()))


@pytest.mark.parametrize("seed", SEEDS)
def test_graph_cases_host_and_device_forms(cases, seed):
    """1. Index.unitig_links and unitigs_t + unitig_links_t at three cutoffs."""
    with _open(cases[seed]) as ix:
        for cutoff in CUTOFFS:
            un, want = _ref(ix, cutoff)
            if cutoff == 0:                                         # the case cannot pass vacuously
                assert all(LC.histogram(want)) and want["E"] > 0
            if cutoff == CUTOFFS[-1]:
                assert want["U"] == 0 and want["link_off"].tolist() == [0]
            _same(ix.unitig_links(cutoff), want, (seed, cutoff, "host"))
            _same(ix.unitig_links_t(cutoff), want, (seed, cutoff, "device"))
            _same(ix.unitig_links_t(cutoff, unitigs=ix.unitigs_t(cutoff)), want, (seed, cutoff, "device, given unitigs"))


@pytest.mark.parametrize("name", NAMES)
def test_planted_cases_host_and_device_forms(planted, name):
    """2. Every topology case of the compaction and every planted link case at its cutoffs: both forms equal the restatement, the
    checker accepts them; bubble_mate is exact, every near-bubble included (test_unitig_links_cpu.py asserts the structures)."""
    t = planted(name)
    with _open(t["prefix"]) as ix:
        for cutoff in t["cutoffs"]:
            un, want = t["want"][cutoff]
            _same(ix.unitig_links(cutoff), want, (name, cutoff, "host"))
            u = ix.unitigs_t(cutoff)
            got = ix.unitig_links_t(cutoff, unitigs=u)
            _same(got, want, (name, cutoff, "device"))
            LK.check(t["codes"], t["tfs"], cutoff, _numpy(u), _numpy(got))


_CHILD = """
import hashlib, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from aindex_amd.engine import Index
h = hashlib.sha256()
for p in sys.argv[2:]:
    with Index.open_23(p + ".pf", p + ".tf.bin", p + ".kmers.bin") as ix:
        for cutoff in (0, 3):
            u = ix.unitig_links(cutoff)
            for k in %r:
                h.update(np.ascontiguousarray(u[k]).tobytes())
print("digest", h.hexdigest())
""" % (ARRAYS,)


def test_many_trips_of_every_loop(cases, planted, monkeypatch):
    """3. AIX_UG_TEST_GRID = 1, 2, 3 workgroups for every launch on seed 3, the bubble cases and tip_of_one (6 ends: no multiple of 16):
    many trips per wave, the tail of the last trip inside a live wave, the filter gauge carried from trip to trip. With 2 workgroups,
    AIX_DBJ_FILTER 0, 1, 2 each in a fresh child: the same digest."""
    names = ("bubble_snp", "bubble_indel", "bubble_same_source_and_sink", "bubble_tip_cutoff", "tip_of_one")
    assert (2 * planted("tip_of_one")["want"][0][1]["U"]) % 16 != 0
    opened = []
    try:
        sets = []
        for prefix, want in [(cases[3], None)] + [(planted(nm)["prefix"], planted(nm)["want"]) for nm in names]:
            ix = _open(prefix)
            opened.append(ix)
            sets.append((ix, {c: (want[c][1] if want and c in want else _ref(ix, c)[1]) for c in (0, 3)}))
        for grid in ("1", "2", "3"):
            monkeypatch.setenv("AIX_UG_TEST_GRID", grid)
            for i, (ix, want) in enumerate(sets):
                for c in (0, 3):
                    _same(ix.unitig_links(c), want[c], (grid, i, c, "host"))
                    _same(ix.unitig_links_t(c), want[c], (grid, i, c, "device"))
        monkeypatch.delenv("AIX_UG_TEST_GRID")
        h = hashlib.sha256()
        for ix, want in sets[:3]:
            for c in (0, 3):
                for k in ARRAYS:
                    h.update(np.ascontiguousarray(want[c][k]).tobytes())
    finally:
        for ix in opened:
            ix.close()
    kids = []
    for policy in ("0", "1", "2"):
        env = dict(os.environ, AIX_DBJ_FILTER=policy, AIX_UG_TEST_GRID="2", AIX_NO_TORCH="1")
        kids.append(subprocess.Popen([sys.executable, "-c", _CHILD, ROOT, cases[3], planted(names[0])["prefix"], planted(names[1])["prefix"]], env=env,
                                     stdout=subprocess.PIPE, stderr=subprocess.PIPE))
    for policy, k in zip("012", kids):
        out, err = k.communicate(timeout=300)
        assert k.returncode == 0, (policy, err.decode()[-2000:])
        assert out.decode().split()[-2:] == ["digest", h.hexdigest()], policy


def _midsize_text(rng, planted_codes):
    """plain text (records end with a newline): a 200 kbp genome, 150-bp reads of either strand at 8 x over its first 30 kbp with 0.5 %
    substitutions, and the keys of the planted bubble cases as 23-base records"""
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


def test_natural_midsize_index_with_the_array_checker():
    """4. An index of about 2.2 x 10^5 keys built on the device from a genome, reads with substitution errors and the planted bubble
    cases; the device form is held to unitig_links_check.check (numpy over the arrays, no dict restatement) at cutoffs 0 and 1. From the
    code: k_ug_check (512 kids per workgroup) and k_ul_ends (1024 per workgroup, so every lane makes four trips) run below their cap of
    4096 workgroups; k_ul_probe gets one workgroup per 128 ends, so each of its waves makes two trips of 16 ends and carries its filter
    gauge into the second; k_ul_fill and k_ul_bubbles make four trips per lane."""
    import torch
    from aindex_amd import counting
    link = LC.link_cases()
    extra = np.concatenate([link[nm].codes for nm in ("bubble_snp", "bubble_indel", "degrees_0_to_4")])
    plain = _midsize_text(np.random.default_rng(20252), extra)
    keys, counts = counting.count_distinct_t(torch.from_numpy(plain).cuda(), 23, _lib.CANON_TRUE_RC)
    ix = Index.build_23_codes_t(builder.build_pf_codes_t(keys, 23), keys, counts.to(torch.int32))
    torch.cuda.synchronize()
    try:
        assert 10 ** 5 <= ix.n <= 3 * 10 ** 5 and ix.canonical_only
        codes, tfs = ix.checker_array() & np.uint64(R.MASK), ix.tf_array()
        for cutoff in (0, 1):
            u = ix.unitigs_t(cutoff)
            got = _numpy(ix.unitig_links_t(cutoff, unitigs=u))
            LK.check(codes, tfs, cutoff, _numpy(u), got)
            if cutoff == 0:
                hist, arms = LC.histogram(got), int((got["bubble_mate"] != NONE32).sum())
                print("n", ix.n, "U", got["U"], "E", got["E"], "degrees", hist, "bubble arms", arms)
                assert all(hist) and arms > 4 and got["U"] > 1000
                _same(ix.unitig_links(0), got, "host form")
    finally:
        ix.close()


def test_refusals_touch_nothing(cases, planted):
    """5. Statuses, 64 poisoned elements behind every output, canaries intact."""
    import torch
    from pf13 import pf13_path
    L = _lib.lib()
    ARG = _lib.AIX_ERR_ARG
    buf = torch.full((1 << 16,), 0xEE, dtype=torch.uint8, device="cuda")
    p = vp(buf.data_ptr())
    e77 = C.c_uint64(77)
    hp = [vp(0x5A5A) for _ in range(3)]
    n2 = [C.c_uint64(77), C.c_uint64(77)]

    def every_call(h, status):
        assert L.aix_unitig_links_dev(h, 0, p, p, p, 1, p, p, p, 8, C.byref(e77), None) == status
        assert L.aix_unitig_links(h, 0, C.byref(n2[0]), C.byref(n2[1]), *[C.byref(x) for x in hp]) == status

    with _open(cases[1]) as ix:
        assert not ix.canonical_only
        every_call(ix._h, _lib.AIX_ERR_UNSUPPORTED)
        with pytest.raises(_lib.AixError):
            ix.unitig_links()
    with Index.open_13(pf13_path(), None) as ix13:
        every_call(ix13._h, _lib.AIX_ERR_MODE)
    every_call(None, ARG)
    assert L.aix_unitig_bubbles_dev(1, None, p, 1, p, None) == ARG and L.aix_unitig_bubbles_dev(1, p, p, 9, p, None) == ARG
    poison = {torch.int64: 0x6B6B6B6B6B6B6B6B, torch.int32: 0x6B6B6B6B}
    t = planted("bubble_tip_cutoff")
    with _open(t["prefix"]) as ix:
        h = ix._h
        for i in (0, 1, 2, 4, 5, 8):                                # every pointer that is needed
            a = [p, p, p, 1, p, p, p, 8, C.byref(e77)]
            a[i] = None
            assert L.aix_unitig_links_dev(h, 0, *a, None) == ARG
        for i in range(4):
            a = [C.byref(n2[0]), C.byref(n2[1]), C.byref(hp[0]), C.byref(hp[1])]
            a[i] = None
            assert L.aix_unitig_links(h, 0, *a, C.byref(hp[2])) == ARG
        u0, u3 = ix.unitigs_t(0), ix.unitigs_t(3)
        want = t["want"][0][1]
        U, E = want["U"], want["E"]
        assert U == 6 and E == 12 and u3["U"] == 1

        def call(cutoff, ku, kp, kf, U_, off, cap):
            lo = torch.full((2 * U_ + 1 + 64,), poison[torch.int64], dtype=torch.int64, device="cuda")
            lt = torch.full((max(cap, 0) + 64,), poison[torch.int32], dtype=torch.int32, device="cuda")
            e = C.c_uint64(77)
            q = lambda x: vp(x.data_ptr())
            st = L.aix_unitig_links_dev(h, cutoff, q(ku), q(kp), q(kf), U_, q(off), q(lo), q(lt), cap, C.byref(e), None)
            torch.cuda.synchronize()
            return st, _host(lo), _host(lt), e.value

        st, lo, lt, e = call(0, u0["kid_unitig"], u0["kid_pos"], u0["kid_flag"], U, u0["offsets"], E)     # exactly enough room
        assert st == 0 and e == E and np.array_equal(lo[:2 * U + 1], want["link_off"]) and np.array_equal(lt[:E], want["link_to"])
        assert (lo[2 * U + 1:] == 0x6B6B6B6B6B6B6B6B).all() and (lt[E:] == 0x6B6B6B6B).all()
        st, lo, lt, e = call(0, u0["kid_unitig"], u0["kid_pos"], u0["kid_flag"], U, u0["offsets"], E - 1)  # one too few
        assert st == ARG and e == E and np.array_equal(lo[:2 * U + 1], want["link_off"]) and (lo[2 * U + 1:] == 0x6B6B6B6B6B6B6B6B).all()
        assert (lt == 0x6B6B6B6B).all()
        untouched = lambda r: r[0] == ARG and r[3] == 77 and (r[1] == 0x6B6B6B6B6B6B6B6B).all() and (r[2] == 0x6B6B6B6B).all()
        assert untouched(call(3, u0["kid_unitig"], u0["kid_pos"], u0["kid_flag"], U, u0["offsets"], E))    # a layout of another cutoff
        wrong = torch.zeros(U + 1, dtype=torch.int64, device="cuda")                                        # offsets of another cutoff
        wrong[1:] = u3["offsets"][1]
        assert untouched(call(0, u0["kid_unitig"], u0["kid_pos"], u0["kid_flag"], U, wrong, E))
        shifted = u0["offsets"].clone()                                                                     # one member moved to its neighbour
        shifted[1] += 1
        assert untouched(call(0, u0["kid_unitig"], u0["kid_pos"], u0["kid_flag"], U, shifted, E))
        ku = u0["kid_unitig"].clone()                                                                       # kid_unitig entries >= U
        ku[::7] = U + 5
        assert untouched(call(0, ku, u0["kid_pos"], u0["kid_flag"], U, u0["offsets"], E))
        ku = u0["kid_unitig"].clone()
        ku[3] = 1 << 40
        assert untouched(call(0, ku, u0["kid_pos"], u0["kid_flag"], U, u0["offsets"], E))
        mate = torch.full((U + 64,), poison[torch.int32], dtype=torch.int32, device="cuda")
        got = ix.unitig_links_t(0, unitigs=u0)
        _lib.check(L.aix_unitig_bubbles_dev(U, vp(got["link_off"].data_ptr()), vp(got["link_to"].data_ptr()), E, vp(mate.data_ptr()), None))
        assert np.array_equal(_host(mate[:U]), want["bubble_mate"]) and bool((mate[U:] == poison[torch.int32]).all())
    torch.cuda.synchronize()
    assert bool((buf == 0xEE).all()) and e77.value == 77 and [x.value for x in hp] == [0x5A5A] * 3 and [x.value for x in n2] == [77, 77]


def test_determinism_options_and_streams(cases):
    """6. Two calls give identical bytes; the verification table and the absence filter on / off; a side stream; unitigs made on one
    stream and links on another."""
    import torch
    with _open(cases[6]) as ix:
        want = {c: _ref(ix, c)[1] for c in (0, 3)}
        digest = {c: _digest(want[c]) for c in (0, 3)}
        assert digest[0] != digest[3]
        for c in (0, 3):
            assert _digest(ix.unitig_links(c)) == _digest(ix.unitig_links(c)) == digest[c]
        for table, lanes in ((False, 0), (True, 8)):
            ix.set_bucket_table(table, lanes)
            for filt in (True, False):
                ix.set_absence_filter(filt)
                for c in (0, 3):
                    assert _digest(ix.unitig_links(c)) == digest[c], (table, lanes, filt, c)
                    assert _digest(_numpy(ix.unitig_links_t(c))) == digest[c], (table, lanes, filt, c)
        a, b = torch.cuda.Stream(), torch.cuda.Stream()
        for c in (0, 3):
            with torch.cuda.stream(a):
                got = ix.unitig_links_t(c)
            a.synchronize()
            _same(got, want[c], (c, "side stream"))
            with torch.cuda.stream(a):
                u = ix.unitigs_t(c)
            with torch.cuda.stream(b):
                got = ix.unitig_links_t(c, unitigs=u)
            b.synchronize()
            _same(got, want[c], (c, "unitigs on one stream, links on another"))


def test_list_surface(cases, planted, small23_prefix, tmp_path):
    """7. get_unitig_links, get_bubbles and write_gfa; the file re-parsed, every L line verified by the overlap of its segments."""
    from aindex_amd.aindex import AIndex
    rc = lambda s: s[::-1].translate(str.maketrans("ACGT", "TGCA"))
    with _open(small23_prefix) as probe:
        canonical = probe.canonical_only
    second = small23_prefix if canonical else cases[0]             # kmer_counter's keys are not all canonical: then a graph case
    for prefix in (planted("bubble_tip_cutoff")["prefix"], second):
        ai = AIndex.load_23mer_index(prefix + ".pf", prefix + ".tf.bin", prefix + ".kmers.bin")
        try:
            ix = ai._wrapper._need23()
            for cutoff in (0, 3):
                un, want = _ref(ix, cutoff)
                off, to = want["link_off"].tolist(), want["link_to"].tolist()
                pairs = [(e, t) for e in range(2 * want["U"]) for t in to[off[e]:off[e + 1]] if (e, t) <= (t ^ 1, e ^ 1)]
                assert ai.get_unitig_links(cutoff) == [(e >> 1, "+-"[e & 1], t >> 1, "+-"[t & 1]) for e, t in pairs]
                assert ai.get_bubbles(cutoff) == LC.mate_pairs(want)
                path = str(tmp_path / f"g{cutoff}.gfa")
                n_circ = int(un["n_circular"])
                assert ai.write_gfa(path, cutoff) == (want["U"], len(pairs) + n_circ)
                lines = open(path).read().split("\n")
                assert lines[-1] == "" and lines[0] == "H\tVN:Z:1.0"
                seg = {}
                for ln in lines[1:-1]:
                    f = ln.split("\t")
                    if f[0] == "S":
                        seg[f[1]] = f[2]
                        assert f[3] == f"LN:i:{len(f[2])}"
                assert len(seg) == want["U"] and [seg[f"u{i}"] for i in range(want["U"])] == un["strings"]
                n_links = 0
                for ln in lines[1:-1]:
                    f = ln.split("\t")
                    if f[0] == "L":
                        n_links += 1
                        a, b = seg[f[1]], seg[f[3]]
                        assert f[5] == "22M" and (a if f[2] == "+" else rc(a))[-22:] == (b if f[4] == "+" else rc(b))[:22]
                assert n_links == len(pairs) + n_circ
        finally:
            ai._wrapper.close()
