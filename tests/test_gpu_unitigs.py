"""De Bruijn compaction on the GPU (aix_unitigs.hip) against the test-side restatement (tests/unitigs_ref.py, pinned by
test_unitigs_cpu.py). Every comparison is exact equality."""
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
import unitigs_cases as UC
import unitigs_check as KC
import unitigs_ref as R
from aindex_amd import _lib, builder
from aindex_amd.engine import Index

vp = _lib.vp
SEEDS = (0, 3, 6, 9)
CUTOFFS = (0, 3, 2 ** 32 - 1)
ARRAYS = ("offsets", "bases", "circular", "tf_sum", "tf_min", "tf_max", "kid_unitig", "kid_pos", "kid_flag")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _open(prefix):
    return Index.open_23(prefix + ".pf", prefix + ".tf.bin", prefix + ".kmers.bin")


def _ref(ix, cutoff):
    return R.unitigs(ix.checker_array() & np.uint64(R.MASK), ix.tf_array(), cutoff)


def _host(t):
    """a device tensor of u64 / u32 bit patterns as the unsigned numpy array"""
    a = t.cpu().numpy()
    return a.view({np.dtype(np.int64): np.uint64, np.dtype(np.int32): np.uint32}.get(a.dtype, a.dtype))


def _same(got, want, kmer_tf, tag):
    for k in ("U", "n_live", "n_circular"):
        assert got[k] == want[k], (tag, k)
    for k in ARRAYS:
        a = got[k] if isinstance(got[k], np.ndarray) else _host(got[k])
        assert a.dtype == want[k].dtype and np.array_equal(a, want[k]), (tag, k)
    if kmer_tf:
        a = got["kmer_tf"] if isinstance(got["kmer_tf"], np.ndarray) else _host(got["kmer_tf"])
        assert a.dtype == np.uint32 and np.array_equal(a, want["kmer_tf"]), (tag, "kmer_tf")
    else:
        assert got["kmer_tf"] is None, tag


def _digest(u):
    h = hashlib.sha256()
    for k in ARRAYS + ("kmer_tf",):
        h.update(np.ascontiguousarray(u[k]).tobytes())
    return h.hexdigest()


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """seed -> prefix of the graph case as index files; the both-strand seeds 1 and 2 for the refusals"""
    d = str(tmp_path_factory.mktemp("ug"))
    return {seed: G.write_graph_case(seed, d)[0] for seed in SEEDS + (1, 2)}


@pytest.fixture(scope="module")
def depth(tmp_path_factory):
    """~33 000 keys with tf 1: linear paths and circles of prescribed lengths; the restatement's answer, computed once"""
    codes, tfs, paths, circles = UC.depth_case()
    pf = builder.build_pf_codes(codes, 23)
    path = str(tmp_path_factory.mktemp("ugd") / "depth.pf")
    open(path, "wb").write(pf)
    rc, checker, tf = O.index_scatter(O.OracleMphf(path), np.ascontiguousarray(D.decode(codes)).reshape(-1), tfs)
    assert rc == 0
    ix = Index.create_23(pf, checker, tf)
    want = R.unitigs(checker & np.uint64(R.MASK), tf, 0)
    yield {"ix": ix, "want": want, "paths": paths, "circles": circles}
    ix.close()


@pytest.mark.parametrize("seed", SEEDS)
def test_graph_cases_host_and_device_forms(cases, seed):
    """1. Every output array of Index.unitigs and of unitigs_layout_t + unitigs_t, kmer_tf on and off, at three cutoffs."""
    with _open(cases[seed]) as ix:
        assert ix.canonical_only
        for cutoff in CUTOFFS:
            want = _ref(ix, cutoff)
            if cutoff == 0:                                         # the case cannot pass vacuously
                assert want["n_circular"] >= 2 and (want["kid_flag"] & 1).any() and want["U"] > 100
            if cutoff == CUTOFFS[-1]:
                assert want["U"] == 0 and want["offsets"].tolist() == [0]
            for on in (True, False):
                _same(ix.unitigs(cutoff, want_kmer_tf=on), want, on, (seed, cutoff, on, "host"))
                layout = ix.unitigs_layout_t(cutoff)
                assert layout[3:] == (want["U"], int(want["offsets"][-1]), want["n_live"], want["n_circular"])
                _same(ix.unitigs_t(cutoff, want_kmer_tf=on, layout=layout), want, on, (seed, cutoff, on, "device"))
            _same(ix.unitigs_t(cutoff), want, False, (seed, cutoff, "one call"))


def test_depth_and_power_of_two_lengths(depth):
    """2. Paths of 1 .. 20 001 k-mers and circles of 2 .. 4097: a missed round, a 2^r cycle taken for a finished path, cycle start and
    direction, the detection round."""
    ix, want = depth["ix"], depth["want"]
    m = np.diff(want["offsets"].astype(np.int64)) - 22
    assert sorted(m[want["circular"] == 0].tolist()) == sorted(depth["paths"])
    assert sorted(m[want["circular"] == 1].tolist()) == sorted(depth["circles"])
    _same(ix.unitigs(0, want_kmer_tf=True), want, True, "host")
    _same(ix.unitigs_t(0, want_kmer_tf=True), want, True, "device")
    none = ix.unitigs(1)                                             # every tf is 1
    assert none["U"] == 0 and none["offsets"].tolist() == [0] and (none["kid_unitig"] == R.NONE).all()


def test_refusals_touch_nothing(cases):
    """3. Both-strand handles, a 13-mer handle, NULL outputs: the status, and not one output byte."""
    import torch
    from pf13 import pf13_path
    L = _lib.lib()
    buf = torch.full((1 << 16,), 0xEE, dtype=torch.uint8, device="cuda")
    p = vp(buf.data_ptr())
    n4 = [C.c_uint64(77) for _ in range(4)]
    r4 = [C.byref(x) for x in n4]
    hp = [vp(0x5A5A) for _ in range(10)]
    hr = [C.byref(x) for x in hp]

    def every_call(h, status):
        assert L.aix_unitigs_layout_dev(h, 0, p, p, p, *r4, None) == status
        assert L.aix_unitigs_emit_dev(h, 0, p, p, p, 1, p, p, p, p, p, p, p, None) == status
        assert L.aix_unitigs(h, 0, r4[0], *hr) == status

    for seed in (1, 2):
        with _open(cases[seed]) as ix:
            assert not ix.canonical_only
            every_call(ix._h, _lib.AIX_ERR_UNSUPPORTED)
            with pytest.raises(_lib.AixError):
                ix.unitigs()
    with Index.open_13(pf13_path(), None) as ix13:
        every_call(ix13._h, _lib.AIX_ERR_MODE)
    every_call(None, _lib.AIX_ERR_ARG)
    with _open(cases[0]) as ix:
        h, ARG = ix._h, _lib.AIX_ERR_ARG
        for i in range(3):
            a = [p, p, p]
            a[i] = None
            assert L.aix_unitigs_layout_dev(h, 0, *a, *r4, None) == ARG
            assert L.aix_unitigs_emit_dev(h, 0, *a, 1, p, p, p, p, p, p, p, None) == ARG
        for i in range(4):
            a = list(r4)
            a[i] = None
            assert L.aix_unitigs_layout_dev(h, 0, p, p, p, *a, None) == ARG
        for i in range(6):                                          # kmer_tf alone may be NULL
            a = [p] * 6
            a[i] = None
            assert L.aix_unitigs_emit_dev(h, 0, p, p, p, 1, *a, None, None) == ARG
        assert L.aix_unitigs(h, 0, None, *hr) == ARG
        for i in range(6):
            a = list(hr)
            a[i] = None
            assert L.aix_unitigs(h, 0, r4[0], *a) == ARG
        # a layout that does not belong to the cutoff: every kid of cutoff 0 is live, at cutoff 3 some tf are <= 3
        layout = ix.unitigs_layout_t(0)
        with pytest.raises(_lib.AixError) as e:
            ix.unitigs_t(3, layout=layout)
        assert e.value.status == ARG
    torch.cuda.synchronize()
    assert bool((buf == 0xEE).all()) and [x.value for x in n4] == [77] * 4 and [x.value for x in hp] == [0x5A5A] * 10


_CHILD = """
import hashlib, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from aindex_amd.engine import Index
h = hashlib.sha256()
for p in sys.argv[2:]:
    with Index.open_23(p + ".pf", p + ".tf.bin", p + ".kmers.bin") as ix:
        for cutoff in (0, 3):
            u = ix.unitigs(cutoff, want_kmer_tf=True)
            for k in %r:
                h.update(np.ascontiguousarray(u[k]).tobytes())
print("digest", h.hexdigest())
""" % (ARRAYS + ("kmer_tf",),)


def test_answers_do_not_depend_on_any_switch(cases):
    """4. Verification table on / off and its lane widths in this process; AIX_DBJ_FILTER 0, 1, 2 each in a fresh child."""
    with _open(cases[3]) as ix:
        want = {c: _digest(ix.unitigs(c, want_kmer_tf=True)) for c in (0, 3)}
        assert want[0] == _digest(_ref(ix, 0)) and want[0] != want[3]
        for table, lanes in ((False, 0), (True, 1), (True, 4), (True, 8)):
            ix.set_bucket_table(table, lanes)
            for filt in (True, False):
                ix.set_absence_filter(filt)
                for c in (0, 3):
                    assert _digest(ix.unitigs(c, want_kmer_tf=True)) == want[c], (table, lanes, filt, c)
        ix.set_bucket_table(False, 0)                               # every probe through the MPHF records: its three filters, the fast path flag
        for fp, ee, canon in ((True, True, True), (False, False, False), (True, False, True)):
            ix.set_fingerprint_filter(fp)
            ix.set_early_exit(ee)
            ix.set_canonical_fastpath(canon)
            for c in (0, 3):
                assert _digest(ix.unitigs(c, want_kmer_tf=True)) == want[c], (fp, ee, canon, c)
    h = hashlib.sha256()
    with _open(cases[3]) as ix:
        for c in (0, 3):
            u = ix.unitigs(c, want_kmer_tf=True)
            for k in ARRAYS + ("kmer_tf",):
                h.update(np.ascontiguousarray(u[k]).tobytes())
    kids = []
    for policy in ("0", "1", "2"):
        env = dict(os.environ, AIX_DBJ_FILTER=policy, AIX_NO_TORCH="1")
        kids.append(subprocess.Popen([sys.executable, "-c", _CHILD, ROOT, cases[3]], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE))
    for policy, k in zip("012", kids):
        out, err = k.communicate(timeout=300)
        assert k.returncode == 0, (policy, err.decode()[-2000:])
        assert out.decode().split()[-2:] == ["digest", h.hexdigest()], policy


def test_determinism_canaries_and_dead_kids(cases):
    """5. Two calls are byte-identical; 64 poisoned elements behind every device output survive; dead kids carry NONE, 0, 0."""
    import torch
    L = _lib.lib()
    with _open(cases[6]) as ix:
        want = _ref(ix, 3)
        a, b = ix.unitigs(3, want_kmer_tf=True), ix.unitigs(3, want_kmer_tf=True)
        assert _digest(a) == _digest(b) == _digest(want)
        dead = ix.tf_array() <= 3
        assert dead.any() and (a["kid_unitig"][dead] == R.NONE).all() and not a["kid_pos"][dead].any() and not a["kid_flag"][dead].any()
        ku, kp, kf, U, total, live, circ = ix.unitigs_layout_t(3)
        sizes = {"offsets": (U + 1, torch.int64), "bases": (total, torch.uint8), "circular": (U, torch.uint8), "tf_sum": (U, torch.int64),
                 "tf_min": (U, torch.int32), "tf_max": (U, torch.int32), "kmer_tf": (live, torch.int32)}
        poison = {torch.int64: 0x6B6B6B6B6B6B6B6B, torch.int32: 0x6B6B6B6B, torch.uint8: 0x6B}
        t = {k: torch.full((s + 64,), poison[dt], dtype=dt, device="cuda") for k, (s, dt) in sizes.items()}
        q = lambda k: vp(t[k].data_ptr())
        _lib.check(L.aix_unitigs_emit_dev(ix._h, 3, vp(ku.data_ptr()), vp(kp.data_ptr()), vp(kf.data_ptr()), U, q("offsets"), q("bases"), q("circular"),
                                          q("tf_sum"), q("tf_min"), q("tf_max"), q("kmer_tf"), None))
        torch.cuda.synchronize()
        for k, (s, dt) in sizes.items():
            assert bool((t[k][s:] == poison[dt]).all()), k
            assert np.array_equal(_host(t[k][:s]), want[k]), k
        # the per-kid arrays are written for n kids and no further
        n = ix.n
        pads = [torch.full((n + 64,), poison[dt], dtype=dt, device="cuda") for dt in (torch.int64, torch.int32, torch.uint8)]
        outs = [C.c_uint64() for _ in range(4)]
        _lib.check(L.aix_unitigs_layout_dev(ix._h, 3, *[vp(x.data_ptr()) for x in pads], *[C.byref(x) for x in outs], None))
        for x, k, dt in zip(pads, ("kid_unitig", "kid_pos", "kid_flag"), (torch.int64, torch.int32, torch.uint8)):
            assert bool((x[n:] == poison[dt]).all()) and np.array_equal(_host(x[:n]), want[k]), k
        assert [x.value for x in outs] == [U, total, live, circ]


def _check_walks(ix, u, cutoff):
    import torch
    m = np.diff(u["offsets"].astype(np.int64)) - 22
    lin = np.nonzero(u["circular"] == 0)[0]
    off = u["offsets"].astype(np.int64)
    first = D.encode(np.ascontiguousarray(u["bases"][off[lin, None] + np.arange(23)[None, :]]))
    L = int(m[lin].max())
    b, ln, st, _, _ = ix.walk_t(torch.from_numpy(first.view(np.int64)).cuda(), L, "next", cutoff, "unitig", want_tf=False)
    b, ln = b.cpu().numpy(), _host(ln)
    assert (ln >= m[lin] - 1).all()                                  # (the walk does not cut hairpins: it may go on)
    for j, i in enumerate(lin.tolist()):
        assert np.array_equal(b[j, : m[i] - 1], u["bases"][off[i] + 23: off[i + 1]]), i
    return lin.shape[0], L


def test_linear_unitigs_agree_with_the_bounded_walk(cases, depth):
    """6. HIP against HIP: walk_t in unitig mode from the first k-mer of every linear unitig spells that unitig."""
    count, longest = _check_walks(depth["ix"], depth["ix"].unitigs(0), 0)
    assert count == len(depth["paths"]) and longest == 20001
    with _open(cases[9]) as ix:
        for cutoff in (0, 3):
            count, longest = _check_walks(ix, ix.unitigs(cutoff), cutoff)
            assert count > 400 and longest >= 2                      # not vacuous: hundreds of paths, not all of them single k-mers


def test_list_surface(cases, small23_prefix, tmp_path):
    """7. get_unitigs, get_unitig_of_kmers and write_unitigs against the arrays."""
    from aindex_amd.aindex import AIndex
    with _open(small23_prefix) as probe:
        canonical = probe.canonical_only
    prefix = small23_prefix if canonical else cases[0]            # kmer_counter's keys are not all canonical: then a graph case
    ai = AIndex.load_23mer_index(prefix + ".pf", prefix + ".tf.bin", prefix + ".kmers.bin")
    try:
        ix = ai._wrapper._need23()
        for cutoff in (0, 3):
            want = _ref(ix, cutoff)
            strings, m = want["strings"], np.diff(want["offsets"].astype(np.int64)) - 22
            recs = list(zip(strings, want["tf_sum"].tolist(), [bool(c) for c in want["circular"].tolist()]))
            assert ai.get_unitigs(cutoff) == recs
            assert ai.get_unitigs(cutoff, min_kmers=5) == [r for r, k in zip(recs, m.tolist()) if k >= 5]
            path = str(tmp_path / f"u{cutoff}.fa")
            assert ai.write_unitigs(path, cutoff, min_kmers=2) == int((m >= 2).sum())
            lines = open(path).read().split("\n")
            assert lines[-1] == "" and len(lines) == 2 * int((m >= 2).sum()) + 1
            keep = [i for i in range(want["U"]) if m[i] >= 2]
            for j, i in enumerate(keep):
                s, c = int(want["tf_sum"][i]), " circular" if want["circular"][i] else ""
                assert lines[2 * j] == f">u{i} LN:i:{len(strings[i])} KC:i:{s} km:f:{s / m[i]:.1f}{c}" and lines[2 * j + 1] == strings[i]
            assert any(ln.endswith(" circular") for ln in lines[::2])
            # member k-mers as stored and reverse-complemented, dead and absent k-mers, items of another length
            codes, tfs = ix.checker_array() & np.uint64(R.MASK), ix.tf_array()
            rng = np.random.default_rng(cutoff)
            kids = rng.choice(codes.shape[0], 300, replace=False)
            fwd = [bytes(r).decode() for r in D.decode(codes[kids])]
            rev = [bytes(r).decode() for r in D.decode(D.revcomp(codes[kids]))]
            absent = "ACGTTGCATGCATGCAAGCTAGC"
            assert ai.get_tf_value(absent) == 0
            got = ai.get_unitig_of_kmers(fwd + ["", fwd[0][:22], absent] + rev, cutoff)
            assert got[300:303] == [None, None, None] and len(got) == 603
            dead = 0
            for j, kid in enumerate(kids.tolist()):
                if tfs[kid] <= cutoff:
                    assert got[j] is None and got[303 + j] is None
                    dead += 1
                    continue
                u, pos, flag = int(want["kid_unitig"][kid]), int(want["kid_pos"][kid]), int(want["kid_flag"][kid]) & 1
                assert got[j] == (u, pos, flag) and got[303 + j] == (u, pos, flag ^ 1)
                word = strings[u][pos:pos + 23]
                assert (word if got[j][2] == 0 else word[::-1].translate(str.maketrans("ACGT", "TGCA"))) == fwd[j]
            assert dead > 0 or cutoff == 0
        assert ai.get_unitig_of_kmers([]) == [] and ai.get_unitig_of_kmers(["ACGT"]) == [None]
    finally:
        ai._wrapper.close()


# ---------------------------------------------------------------------------------------------
# planted topologies, many trips of every grid-stride loop, the natural second trip, streams
# ---------------------------------------------------------------------------------------------
def _numpy(u):
    """a device-form answer as the numpy dict that _digest and unitigs_check.check take"""
    return {k: (_host(v) if hasattr(v, "cpu") else v) for k, v in u.items()}


@pytest.fixture(scope="module")
def topo(tmp_path_factory):
    """name -> {"prefix", "case", "want": cutoff -> the restatement's answer in the index's kid order}: the planted topologies as index files,
    each built and answered once, when a test first asks for it"""
    d = str(tmp_path_factory.mktemp("ugt"))
    planted, made = UC.topology_cases(), {}

    def get(name):
        if name not in made:
            case = planted[name]
            prefix = os.path.join(d, name)
            open(prefix + ".pf", "wb").write(builder.build_pf_codes(case.codes, 23))
            rc, checker, tf = O.index_scatter(O.OracleMphf(prefix + ".pf"), np.ascontiguousarray(D.decode(case.codes)).reshape(-1), case.tfs)
            assert rc == 0
            checker.tofile(prefix + ".kmers.bin")
            tf.tofile(prefix + ".tf.bin")
            codes = checker & np.uint64(R.MASK)
            made[name] = {"prefix": prefix, "case": case, "codes": codes, "tfs": tf,
                          "want": {c: R.unitigs(codes, tf, c) for c in UC.topology_cutoffs(name)}}
        return made[name]
    return get


@pytest.mark.parametrize("name", sorted(UC.topology_cases()))
def test_planted_topologies_host_and_device_forms(topo, name):
    """8. Hairpin ends, self-loops with neighbours, lollipops, a bubble and a tip at the cutoff, circles that a cutoff opens, hundreds of
    small circles beside a long path, isolated keys, one key, tf at 2^32 - 1: the restatement's arrays in both forms at cutoffs 0 and 3
    (`heavy`: 0xFFFFFFFE too), and unitigs_check.check accepts them. test_unitigs_cpu.py asserts that each case holds its structure."""
    t = topo(name)
    with _open(t["prefix"]) as ix:
        assert ix.canonical_only and ix.n == t["case"].codes.shape[0]
        for cutoff in UC.topology_cutoffs(name):
            want = t["want"][cutoff]
            _same(ix.unitigs(cutoff, want_kmer_tf=True), want, True, (name, cutoff, "host"))
            layout = ix.unitigs_layout_t(cutoff)
            assert layout[3:] == (want["U"], int(want["offsets"][-1]), want["n_live"], want["n_circular"])
            got = ix.unitigs_t(cutoff, want_kmer_tf=True, layout=layout)
            _same(got, want, True, (name, cutoff, "device"))
            KC.check(t["codes"], t["tfs"], cutoff, _numpy(got))
        if name == "isolated_one":
            u = ix.unitigs(0)
            assert u["U"] == 1 and u["offsets"].tolist() == [0, 23] and u["bases"].tobytes().decode() == R.spell([int(t["codes"][0])])
        if name == "heavy":
            assert int(ix.unitigs(0)["tf_sum"].max()) == 6 * 0xFFFFFFFF and ix.unitigs(0xFFFFFFFF)["U"] == 0


def test_many_trips_of_every_loop_on_small_cases(cases, depth, topo, monkeypatch):
    """9. AIX_UG_TEST_GRID = 1, 2, 3 workgroups for k_ug_ports and every grid-stride launch: hundreds of trips per workgroup, the tail of
    the last trip inside a live wave (18 484 ports are no multiple of 16), the filter gauge carried from trip to trip. The restatement's
    digest at cutoffs 0 and 3 in this process; with 2 workgroups, AIX_DBJ_FILTER 0, 1, 2 each in a fresh child."""
    many = topo("many_circles")
    assert (2 * many["codes"].shape[0]) % 16 != 0
    opened = []
    try:
        sets = [(depth["ix"], {0: _digest(depth["want"]), 3: _digest(R.unitigs(depth["ix"].checker_array() & np.uint64(R.MASK), depth["ix"].tf_array(), 3))})]
        for prefix, want in ((cases[3], None), (many["prefix"], many["want"])):
            ix = _open(prefix)
            opened.append(ix)
            sets.append((ix, {c: _digest(want[c] if want else _ref(ix, c)) for c in (0, 3)}))
        assert len({d[0] for _, d in sets}) == 3
        for grid in ("1", "2", "3"):
            monkeypatch.setenv("AIX_UG_TEST_GRID", grid)
            for i, (ix, want) in enumerate(sets):
                for c in (0, 3):
                    assert _digest(ix.unitigs(c, want_kmer_tf=True)) == want[c], (grid, i, c, "host")
                    assert _digest(_numpy(ix.unitigs_t(c, want_kmer_tf=True))) == want[c], (grid, i, c, "device")
        monkeypatch.delenv("AIX_UG_TEST_GRID")
        h = hashlib.sha256()
        for ix, want in sets[1:]:
            for c in (0, 3):
                u = ix.unitigs(c, want_kmer_tf=True)
                assert _digest(u) == want[c]
                for k in ARRAYS + ("kmer_tf",):
                    h.update(np.ascontiguousarray(u[k]).tobytes())
    finally:
        for ix in opened:
            ix.close()
    kids = []
    for policy in ("0", "1", "2"):
        env = dict(os.environ, AIX_DBJ_FILTER=policy, AIX_UG_TEST_GRID="2", AIX_NO_TORCH="1")
        kids.append(subprocess.Popen([sys.executable, "-c", _CHILD, ROOT, cases[3], many["prefix"]], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE))
    for policy, k in zip("012", kids):
        out, err = k.communicate(timeout=300)
        assert k.returncode == 0, (policy, err.decode()[-2000:])
        assert out.decode().split()[-2:] == ["digest", h.hexdigest()], policy


def _midsize_text(rng):
    """plain text (records end with a newline): a 1.3 Mbp genome; 150-bp reads of either strand at 6 x over a further 150 kbp with 0.5 %
    substitutions; circular sequences of 3 .. 99 991 bases, each with its first 22 bases appended and written twice; the reads of
    test_gpu_debruijn._seeded_reads (tandem arrays, a planted repeat)."""
    from test_gpu_debruijn import _seeded_reads
    nl = np.array([10], np.uint8)
    parts = [D.LETTERS[rng.integers(0, 4, 1_300_000)], nl]
    g = rng.integers(0, 4, 150_000).astype(np.uint8)
    n_reads = 6 * len(g) // 150
    reads = g[rng.integers(0, len(g) - 150, n_reads)[:, None] + np.arange(150)[None, :]]
    reads = np.where(rng.random(reads.shape) < 0.005, (reads + rng.integers(1, 4, reads.shape)) % 4, reads).astype(np.uint8)
    flip = rng.random(n_reads) < 0.5
    reads[flip] = (3 - reads[flip])[:, ::-1]
    parts.append(np.concatenate([D.LETTERS[reads], np.full((n_reads, 1), 10, np.uint8)], axis=1).reshape(-1))
    circles = (3, 4097, 65_536, 65_537, 99_991)
    for m in circles:
        unit = np.array([0, 1, 2], np.uint8) if m == 3 else rng.integers(0, 4, m).astype(np.uint8)
        ring = D.LETTERS[np.tile(unit, 22 // m + 2)[: m + 22]]
        parts += [ring, nl, ring, nl]
    parts.append(_seeded_reads(rng)[1])
    return np.concatenate(parts), circles


def test_natural_second_trip_and_grids_at_their_caps(monkeypatch):
    """10. An index of 2.2 .. 3 million keys built on the device: k_ug_ports makes a second trip over at least 2^17 ports, every
    grid-stride launch over ports runs at its cap of 4096 workgroups, the ranking takes 21 or 22 rounds, circles of 3 .. 99 991 k-mers
    are ranked beside them. unitigs_check.check (link table through torch on the device) accepts the device form at cutoffs 0 and 1;
    cutoff 0 with AIX_UG_TEST_GRID=512, and with AIX_DBJ_FILTER 0 and 1 (read per call), is byte-identical. The restatement does not run
    at this size in the suite; run once on a CPU (6.5 minutes) it gave the figures below, and check() accepted its answer.
    On an MI355X: n = 2 273 469, U = 38 886 (1076 at cutoff 1, where the genome, written once, is dead), n_circular = 5 (3, 4097, 65 536,
    65 537 and 99 991 k-mers), longest unitig 1 299 978 k-mers; the whole test takes 0.9 s of wall time."""
    import time
    import torch
    from aindex_amd import counting
    t0 = time.time()
    plain, circles = _midsize_text(np.random.default_rng(20251))
    keys, counts = counting.count_distinct_t(torch.from_numpy(plain).cuda(), 23, _lib.CANON_TRUE_RC)
    pf = builder.build_pf_codes_t(keys, 23)
    ix = Index.build_23_codes_t(pf, keys, counts.to(torch.int32))
    torch.cuda.synchronize()
    try:
        n = ix.n
        assert 2 ** 21 + 2 ** 16 <= n <= 3_000_000 and ix.canonical_only
        codes, tfs = ix.checker_array() & np.uint64(R.MASK), ix.tf_array()
        t1 = time.time()
        got = {}
        for cutoff in (0, 1):
            got[cutoff] = _numpy(ix.unitigs_t(cutoff, want_kmer_tf=True))
            KC.check(codes, tfs, cutoff, got[cutoff], device="cuda")
        u = got[0]
        m = np.diff(u["offsets"].astype(np.int64)) - 22
        print("n", n, "U", u["U"], "n_circular", u["n_circular"], "longest", int(m.max()), "U at cutoff 1", got[1]["U"],
              "circles", sorted(m[u["circular"] == 1].tolist())[-6:], "build %.1f s, two cutoffs with check %.1f s" % (t1 - t0, time.time() - t1))
        assert u["n_circular"] >= 5 and u["U"] >= 10 ** 4 and int(m.max()) >= 2 ** 19
        assert set(circles) <= set(m[u["circular"] == 1].tolist())
        assert got[1]["U"] < u["U"]
        monkeypatch.setenv("AIX_UG_TEST_GRID", "512")
        assert _digest(_numpy(ix.unitigs_t(0, want_kmer_tf=True))) == _digest(u)
        monkeypatch.delenv("AIX_UG_TEST_GRID")
        for policy in ("0", "1"):                                    # the gauge carried into the natural second trip; the filter always on
            monkeypatch.setenv("AIX_DBJ_FILTER", policy)
            assert _digest(_numpy(ix.unitigs_t(0, want_kmer_tf=True))) == _digest(u), policy
        print("whole test %.1f s" % (time.time() - t0))
    finally:
        ix.close()


def test_links_in_numpy_and_in_torch_on_the_device(cases, topo):
    """11. unitigs_check.links through torch on the device equals its numpy form on the graph cases and on two planted ones (plumbing of
    the checker, not a kernel)."""
    import torch
    sets = [G.make_graph_case(seed)[:2] for seed in SEEDS] + [(topo(name)["codes"], topo(name)["tfs"]) for name in ("hairpin_ends", "many_circles")]
    for i, (codes, tfs) in enumerate(sets):
        for cutoff in (0, 3):
            want = KC.links(codes, tfs, cutoff)
            got = KC._links_on(codes, tfs, cutoff, "cuda")
            assert (want >= 0).sum() > 100 and got.dtype == want.dtype and np.array_equal(got, want), (i, cutoff)


def test_side_streams_and_two_threads(cases):
    """12. (a) unitigs_t under a side stream; (b) the layout made under stream A (the call synchronises its stream) and emitted under
    stream B; (c) two host threads, each under a stream of its own, four calls each at cutoffs 0 and 3 on ONE handle — queries are
    thread-safe per handle (include/aindex_hip.h), as test_concurrent_host_calls_one_handle relies on: per-call scratch, one counter
    record per call, nothing on the handle is written. The restatement's arrays / digest every time."""
    import threading
    import torch
    with _open(cases[6]) as ix:
        want = {c: _ref(ix, c) for c in (0, 3)}
        digest = {c: _digest(want[c]) for c in (0, 3)}
        assert digest[0] != digest[3]
        a, b = torch.cuda.Stream(), torch.cuda.Stream()
        for c in (0, 3):
            with torch.cuda.stream(a):
                got = ix.unitigs_t(c, want_kmer_tf=True)
            a.synchronize()
            _same(got, want[c], True, (c, "side stream"))
            with torch.cuda.stream(a):
                layout = ix.unitigs_layout_t(c)
            with torch.cuda.stream(b):
                got = ix.unitigs_t(c, want_kmer_tf=True, layout=layout)
            b.synchronize()
            _same(got, want[c], True, (c, "layout on one stream, emit on another"))
        errors = []

        def worker(stream, first):
            try:
                with torch.cuda.stream(stream):
                    for it in range(4):
                        for c in ((0, 3) if first else (3, 0)):
                            got = _numpy(ix.unitigs_t(c, want_kmer_tf=True))
                            if _digest(got) != digest[c]:
                                errors.append((first, it, c))
            except Exception as e:                                   # noqa: BLE001
                errors.append(repr(e))
        threads = [threading.Thread(target=worker, args=(s, i == 0)) for i, s in enumerate((a, b))]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
