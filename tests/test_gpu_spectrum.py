"""GPU: k-mers by frequency (aix_spectrum.hip) — per-kid values, spectrum and statistics, stable top-N / threshold selection, batch
kid -> k-mer — against the compiled reference's goldens (tests/golden/*/frequency.json) and tests/spectrum_ref.py. Every comparison is exact."""
import ctypes as C
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle_lib as O
import spectrum_ref as S
from aindex_amd import _lib, engine
from aindex_amd.engine import Index

SETS = ["small23", "graph23"]
vp = _lib.vp
CANARY = 0x5A5A5A5A


def _open(gold, name):
    p = os.path.join(gold, name, name)
    return Index.open_23(p + ".pf", p + ".tf.bin", p + ".kmers.bin")


def _doc(gold, name):
    """the golden document; its (packed) list of every kid's k-mer is replaced by the oracle's decode of the checker once that matches it"""
    doc = json.load(open(os.path.join(gold, name, "frequency.json")))
    kmers = S.kmers23(O.OracleIndex23.from_prefix(os.path.join(gold, name, name)))
    assert S.same(kmers, doc["kmers"])
    doc["kmers"] = kmers
    return doc


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _strings(rows):
    return [r.decode("ascii") for r in np.ascontiguousarray(rows).view(f"S{rows.shape[1]}").reshape(-1).tolist()] if rows.shape[0] else []


def _check_goldens(ix, doc, dev=True):
    import torch
    v = np.array(doc["values"], dtype=np.uint32)
    if dev:
        assert np.array_equal(_u32(ix.kmer_values_t()), v)
    for nbins in (2, 5, 64):
        hist, st = ix.tf_spectrum(nbins)
        assert np.array_equal(hist, S.spectrum(v, nbins)) and int(hist.sum()) == doc["n"]
        assert {k: st[k] for k in ("n", "non_zero", "max", "min_non_zero", "sum")} == S.stats(v)
        assert (st["non_zero_wide"], st["max_wide"], st["sum_wide"]) == (st["non_zero"], st["max"], st["sum"])
        if dev:
            ht, stt = ix.tf_spectrum_t(nbins)
            assert np.array_equal(ht.cpu().numpy().view(np.uint64), hist) and stt.cpu().numpy().tolist() == [st[f] for f in _lib.STATS_FIELDS]
    assert ix.tf_stats() == ix.tf_spectrum(2)[1]
    for sel in doc["selections"]:
        if sel["max_kmers"] == 0:
            continue
        kid, tf, kmers, total = ix.top_kmers(sel["max_kmers"] or 0, sel["min_tf"])
        assert S.same(kid.tolist(), sel["kid"]) and S.same(tf.tolist(), sel["tf"]) and total == sel["total"], (sel["min_tf"], sel["max_kmers"])
        assert _strings(kmers) == [doc["kmers"][k] for k in kid.tolist()]
        assert ix.top_kmers(sel["max_kmers"] or 0, sel["min_tf"], want_kmers=False)[2] is None
        if dev:
            kt, tt, st_, total_t = ix.top_kmers_t(sel["max_kmers"] or 0, sel["min_tf"])
            torch.cuda.synchronize()
            assert np.array_equal(_u32(kt), kid) and np.array_equal(_u32(tt), tf) and total_t == total
            assert np.array_equal(st_.cpu().numpy(), kmers)


@pytest.mark.parametrize("name", SETS)
def test_goldens_through_host_and_device_forms(gold, name):
    with _open(gold, name) as ix:
        _check_goldens(ix, _doc(gold, name))


def test_answers_do_not_depend_on_any_switch(gold):
    """verification table on / off and its lane widths, absence filter, fingerprints, early exit, canonical fast path: the goldens every time"""
    for name in SETS:
        doc = _doc(gold, name)
        doc["selections"] = doc["selections"][:3]
        with _open(gold, name) as ix:
            for table, lanes in ((True, 8), (True, 1), (False, 0)):
                for filt in (True, False):
                    for fp, ee, canon in ((True, True, True), (False, False, False), (True, False, True)):
                        ix.set_bucket_table(table, lanes)
                        ix.set_absence_filter(filt)
                        ix.set_fingerprint_filter(fp)
                        ix.set_early_exit(ee)
                        ix.set_canonical_fastpath(canon)
                        _check_goldens(ix, doc, dev=False)


def test_batch_decode_on_the_goldens(gold):
    import torch
    for name in SETS:
        doc = _doc(gold, name)
        with _open(gold, name) as ix:
            kids = doc["info_kids"] + [doc["n"], doc["n"] + 1, 1 << 40, (1 << 64) - 1]
            want = [tuple(r) for r in doc["info"]] + [(0, "", "")] * 4
            rows, rc, tf = ix.kmers_by_kid(np.array(kids, dtype=np.uint64), want_rc=True, want_tf=True)
            assert list(zip(tf.tolist(), _strings(rows), _strings(rc))) == want
            assert not rows[-4:].any() and not rc[-4:].any()                                   # beyond the index: NUL rows
            r2, none_rc, none_tf = ix.kmers_by_kid(np.array(kids, dtype=np.uint64))
            assert np.array_equal(r2, rows) and none_rc is None and none_tf is None
            kt = torch.from_numpy(np.array(kids, dtype=np.uint64).view(np.int64)).cuda()
            rt, rct, tft = ix.kmers_by_kid_t(kt, want_rc=True, want_tf=True)
            torch.cuda.synchronize()
            assert np.array_equal(rt.cpu().numpy(), rows) and np.array_equal(rct.cpu().numpy(), rc) and np.array_equal(_u32(tft), tf)
            every = ix.kmers_by_kid(np.arange(doc["n"], dtype=np.uint64))[0]
            assert _strings(every) == doc["kmers"]
            assert ix.kmers_by_kid(np.zeros(0, np.uint64))[0].shape == (0, 23)


def test_list_surface_on_the_goldens(gold, small23_prefix):
    from aindex_amd.aindex import AIndex
    doc = _doc(gold, "small23")
    ai = AIndex.load_from_prefix(small23_prefix)
    w = ai._wrapper
    full = next(s for s in doc["selections"] if (s["min_tf"], s["max_kmers"]) == (1, None))
    it = ai.iter_kmers_by_frequency(min_tf=1)
    first = next(it)
    assert w._checker_host is None, "the first item must arrive without the checker having been downloaded"
    v = np.array(doc["values"], dtype=np.uint32)

    def want(min_tf, max_kmers, sel=None):
        """the golden selection as (k-mer, tf) pairs: spectrum_ref's order, held against the golden's (packed) lists where there is one"""
        idx, val, _ = S.select(v, min_tf, max_kmers or 0)
        assert sel is None or (S.same(idx.tolist(), sel["kid"]) and S.same(val.tolist(), sel["tf"]))
        return [(doc["kmers"][k], t) for k, t in zip(idx.tolist(), val.tolist())]
    assert [first] + list(it) == want(1, None, full)
    saved, ai._FREQ_CHUNK = ai._FREQ_CHUNK, 100                                                # many fetches, the same list
    try:
        assert list(ai.iter_kmers_by_frequency(min_tf=1)) == want(1, None)
    finally:
        ai._FREQ_CHUNK = saved
    for sel in doc["selections"]:
        w_ = [] if sel["max_kmers"] == 0 else want(sel["min_tf"], sel["max_kmers"], sel)
        assert list(ai.iter_kmers_by_frequency(min_tf=sel["min_tf"], max_kmers=sel["max_kmers"], kmer_type="23mer")) == w_
        if sel["max_kmers"] is not None:
            assert ai.get_top_kmers(sel["max_kmers"], min_tf=sel["min_tf"]) == w_
    assert list(ai.iter_kmers_by_frequency(min_tf=1, max_kmers=-5901 + 3)) == want(1, 3)
    assert list(ai.iter_kmers_by_frequency(min_tf=1 << 40)) == [] and list(ai.iter_kmers_by_frequency(kmer_type="13mer")) == []
    v = np.array(doc["values"], dtype=np.int64)
    st = ai.get_kmer_frequency_stats()
    assert st == {"kmer_type": "23mer", "total_kmers": doc["n"], "non_zero_kmers": int((v > 0).sum()), "zero_kmers": int((v == 0).sum()), "max_tf": int(v.max()),
                  "min_tf": int(v[v > 0].min()), "avg_tf": int(v.sum()) / int((v > 0).sum()), "total_tf": int(v.sum()), "coverage": int((v > 0).sum()) / doc["n"]}
    assert ai.get_kmer_frequency_stats("13mer")["total_kmers"] == 0
    with pytest.raises(ValueError):
        ai.get_kmer_frequency_stats("17mer")
    assert ai.get_tf_spectrum(max_tf=20) == S.spectrum(v.astype(np.uint32), 22).tolist() and ai.get_tf_spectrum(max_tf=0) == [0, doc["n"]]
    kids = doc["info_kids"] + [1 << 40, -1]
    assert ai.get_kmers_by_kid_batch(kids) == [ai.get_kmer_by_kid(k) for k in kids] == [r[1] for r in doc["info"]] + ["", ""]
    assert ai.get_kmer_info_batch(kids) == [w.get_kmer_info(k) for k in kids] == [tuple(r) for r in doc["info"]] + [(0, "", "")] * 2
    assert ai.get_kmers_by_kid_batch([]) == [] and ai.get_kmer_info_batch([]) == []
    assert w.get_13mer_statistics() == {}


# ------------------------------------------------------------------------------------------------
# array level: the shapes where select and compaction break
# ------------------------------------------------------------------------------------------------
WG, TILE = 256, 4096                                                 # workgroup and compaction tile of aix_spectrum.hip
SIZES = [1, 63, 64, 65, WG - 1, WG, WG + 1, TILE - 1, TILE, TILE + 1, (1 << 20) + 3]


def _patterns(n):
    rng = np.random.default_rng(n)
    i = np.arange(n, dtype=np.uint64)
    straddle = np.full(n, 3, dtype=np.uint32)                                                  # one class (7) on both sides of every workgroup / tile edge
    straddle[(i % WG >= WG - 2) | (i % WG < 2)] = 7
    straddle[::97] = 9
    skew = rng.choice(np.array([1, 1, 1, 1, 1, 2, 2, 3, 40, 70000], dtype=np.uint32), n)    # a real spectrum: nearly everything 1 or 2
    return {"equal": np.full(n, 5, dtype=np.uint32), "ascending": (i + 1).astype(np.uint32), "descending": (n - i).astype(np.uint32),
            "extremes": np.where(rng.random(n) < 0.5, 0, 0xFFFFFFFF).astype(np.uint32), "straddle": straddle, "skew": skew,
            "random": rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)}


def _select(vt, v, min_v, max_items, ref, pad=5):
    """top_values_t into canary-filled buffers of the selection's size + pad; checks the entries and that nothing lies beyond them.
    ref: the full order per min_v, computed once per pattern."""
    import torch
    if min_v not in ref:
        ref[min_v] = S.select(v, min_v, 0)
    want_idx, want_val, want_total = ref[min_v]
    if max_items:
        want_idx, want_val = want_idx[:max_items], want_val[:max_items]
    m = want_idx.shape[0]
    idx_t = torch.full((m + pad,), CANARY, dtype=torch.int32, device=vt.device)
    val_t = torch.full((m + pad,), CANARY, dtype=torch.int32, device=vt.device)
    gi, gv, total = engine.top_values_t(vt, max_items, min_v, idx_t=idx_t, val_t=val_t)
    torch.cuda.synchronize()
    assert total == want_total and gi.numel() == m, (min_v, max_items, total, want_total, gi.numel(), m)
    assert np.array_equal(_u32(gi), want_idx) and np.array_equal(_u32(gv), want_val), (min_v, max_items)
    assert (_u32(idx_t)[m:] == CANARY).all() and (_u32(val_t)[m:] == CANARY).all(), "entries past the selection must stay as they were"
    if 1 < m < 5000:                                                                           # too small a buffer: untouched, total still reported
        si = torch.full((m - 1,), CANARY, dtype=torch.int32, device=vt.device)
        sv = torch.full((m - 1,), CANARY, dtype=torch.int32, device=vt.device)
        a, b, t2 = engine.top_values_t(vt, max_items, min_v, idx_t=si, val_t=sv)
        torch.cuda.synchronize()
        assert a is None and b is None and t2 == want_total and (_u32(si) == CANARY).all() and (_u32(sv) == CANARY).all()


@pytest.mark.parametrize("n", SIZES)
def test_array_level_shapes_and_patterns(n):
    import torch
    for name, v in _patterns(n).items():
        vt = torch.from_numpy(v.view(np.int32)).cuda()
        vmax = int(v.max())
        for nbins in (2, 9, min(vmax, 1 << 20) + 3, 5000):                                     # nbins = 2; beyond max + 2; more bins than LDS holds
            ht, st = engine.spectrum_t(vt, nbins)
            hist = ht.cpu().numpy().view(np.uint64)
            assert np.array_equal(hist, S.spectrum(v, nbins)), (name, nbins)
            assert int(hist.sum()) == n
            got = dict(zip(_lib.STATS_FIELDS, st.cpu().numpy().tolist()))
            assert {k: got[k] for k in ("n", "non_zero", "max", "min_non_zero", "sum")} == S.stats(v), name
        ref = {}
        cls = int((v == vmax).sum())                                                           # the class the first cuts fall into
        inside = int((v == 9).sum()) + max(1, int((v == 7).sum()) // 2) if name == "straddle" else max(1, cls // 2)
        cuts = {1, 2, n, n + 7, max(1, n // 2), cls, max(1, cls - 1), cls + 1, inside}         # a cut of 1, of the class size, inside a class
        if n > 100_000:
            cuts = {1, 100, cls, inside, n + 7}
        for max_items in sorted(cuts):
            _select(vt, v, 1, max_items, ref)
        _select(vt, v, 0, 0, ref)                                                              # everything, zeros included
        _select(vt, v, 0, 3, ref)
        _select(vt, v, vmax, 0, ref)                                                           # min_v == max
        if n <= 100_000:
            _select(vt, v, 5, 2, ref)
        if vmax < 0xFFFFFFFF:
            _select(vt, v, vmax + 1, 4, ref)                                                   # min_v > max: nothing


def test_array_level_u64_view_and_empty_input():
    import torch
    rng = np.random.default_rng(3)
    wide = rng.integers(0, 6, 10_001, dtype=np.uint64)
    wide[::7] += np.uint64(1 << 32)                                                            # the u32 view drops it
    wide[5] = np.uint64(1 << 33)                                                               # view 0, not zero at full width
    wt = torch.from_numpy(wide.view(np.int64)).cuda()
    v = (wide & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    ht, st = engine.spectrum_t(wt, 8)
    got = dict(zip(_lib.STATS_FIELDS, st.cpu().numpy().view(np.uint64).tolist()))
    assert np.array_equal(ht.cpu().numpy().view(np.uint64), S.spectrum(v, 8)) and {k: got[k] for k in ("n", "non_zero", "max", "min_non_zero", "sum")} == S.stats(v)
    assert (got["non_zero_wide"], got["max_wide"], got["sum_wide"]) == (int((wide != 0).sum()), int(wide.max()), int(wide.sum(dtype=np.uint64)))
    gi, gv, total = engine.top_values_t(wt, 50, 1)
    wi, wv, wt_ = S.select(v, 1, 50)
    assert np.array_equal(_u32(gi), wi) and np.array_equal(_u32(gv), wv) and total == wt_
    empty = torch.zeros(0, dtype=torch.int32, device="cuda")
    ht, st = engine.spectrum_t(empty, 4)
    assert ht.cpu().numpy().tolist() == [0, 0, 0, 0] and st.cpu().numpy().tolist() == [0] * 8
    gi, gv, total = engine.top_values_t(empty, 5, 0)
    assert gi.numel() == 0 and total == 0
    assert engine.top_values_t(torch.from_numpy(v.view(np.int32)).cuda(), 5, 1 << 32)[2] == 0


# ------------------------------------------------------------------------------------------------
# values are not tf
# ------------------------------------------------------------------------------------------------
def test_values_of_perturbed_and_both_strand_indexes(small23_prefix, tmp_path):
    """Slots that hold a duplicate of another slot's code, the reverse complement of another slot's code, a code outside the key set, bits
    46 and above: v_i is what the probe of the slot's k-mer finds, not tf[i]. Expected values: the oracle on the same perturbed files."""
    import graph_cases as G
    checker = np.fromfile(small23_prefix + ".kmers.bin", dtype=np.uint64)
    tf = np.fromfile(small23_prefix + ".tf.bin", dtype=np.uint32)
    pf = open(small23_prefix + ".pf", "rb").read()
    n = checker.shape[0]
    a = 10
    b = next(i for i in range(20, n) if tf[i] != tf[a])
    c = 30
    d = next(i for i in range(40, n) if tf[i] != tf[c])
    checker[a] = checker[b]                                                                    # a duplicate: the probe finds slot b
    checker[c] = S.revcomp_codes(checker[d:d + 1], 23)[0]                                      # the other strand of slot d
    checker[50] = np.uint64(0x2AAAAAAAAAAA ^ 0x1234567)                                        # (almost surely) not a key
    checker[60] |= np.uint64(1 << 50)                                                          # the decoded k-mer hashes here, the stored word differs
    checker[n - 1] |= np.uint64(1 << 63)
    prefix = str(tmp_path / "perturbed")
    open(prefix + ".pf", "wb").write(pf)
    checker.tofile(prefix + ".kmers.bin")
    tf.tofile(prefix + ".tf.bin")
    orc = O.OracleIndex23.from_prefix(prefix)
    want = S.values23(orc)
    assert int((want != tf).sum()) >= 4 and want[a] == tf[b] and want[c] == tf[d] and want[60] == 0
    kids = np.array([a, b, c, d, 50, 60, n - 1, n], dtype=np.uint64)
    for ix in (Index.create_23(pf, checker, tf), Index.open_23(prefix + ".pf", prefix + ".tf.bin", prefix + ".kmers.bin")):
        with ix:
            for table in (True, False):
                ix.set_bucket_table(table)
                assert np.array_equal(_u32(ix.kmer_values_t()), want)
                hist, st = ix.tf_spectrum(32)
                assert np.array_equal(hist, S.spectrum(want, 32)) and st["sum"] == int(want.sum(dtype=np.uint64))
                kid, val, _, total = ix.top_kmers(40, 1, want_kmers=False)
                wi, wv, wt = S.select(want, 1, 40)
                assert np.array_equal(kid, wi) and np.array_equal(val, wv) and total == wt
                rows, rc, t = ix.kmers_by_kid(kids, want_rc=True, want_tf=True)               # the label keeps the low 46 bits, tf is tf[kid] itself
                assert list(zip(t.tolist(), _strings(rows), _strings(rc))) == S.info23(orc, kids.tolist())
    for seed in (1, 2):                                                                        # both strands stored, with different tf
        gp, codes, tfs, _ = G.write_graph_case(seed, str(tmp_path))
        gorc = O.OracleIndex23.from_prefix(gp)
        gwant = S.values23(gorc)
        with Index.open_23(gp + ".pf", gp + ".tf.bin", gp + ".kmers.bin") as ix:
            assert not ix.canonical_only
            assert np.array_equal(_u32(ix.kmer_values_t()), gwant)
            kid, val, _, total = ix.top_kmers(0, 0, want_kmers=False)
            wi, wv, wt = S.select(gwant, 0, 0)
            assert np.array_equal(kid, wi) and np.array_equal(val, wv) and total == wt == gorc.n
            assert np.array_equal(ix.tf_spectrum(7)[0], S.spectrum(gwant, 7))


# ------------------------------------------------------------------------------------------------
# 13-mer handles
# ------------------------------------------------------------------------------------------------
_TABLE13 = []


def _table13():
    """(tf uint64[4^13], its u32 view, the non-zero entries): mostly zero, ties, entries above 2^32; made once"""
    if not _TABLE13:
        n = 4 ** 13
        rng = np.random.default_rng(13)
        tf = np.zeros(n, dtype=np.uint64)
        hot = rng.choice(n, 5000, replace=False)
        tf[hot] = rng.integers(1, 9, 5000).astype(np.uint64)
        tf[hot[:50]] += np.uint64(1 << 32)                                                     # u32 view: the low word
        tf[hot[50]] = np.uint64(1 << 40)                                                       # u32 view: 0
        tf[[0, n - 1]] = np.uint64(0xFFFFFFFF)
        _TABLE13.append((tf, (tf & np.uint64(0xFFFFFFFF)).astype(np.uint32), hot))
    return _TABLE13[0]


def test_13mer_list_surface_through_a_loaded_prefix(tmp_path):
    """a written 13-mer prefix loaded the public way: labels are the base-4 spelling of the index, get_13mer_statistics at full width"""
    from pf13 import pf13_path
    from aindex_amd.aindex import AIndex
    tf, v, _ = _table13()
    n = tf.shape[0]
    prefix = str(tmp_path / "t13")
    os.symlink(pf13_path(), prefix + ".pf")
    tf.tofile(prefix + ".tf.bin")
    ai = AIndex.load_from_prefix(prefix, kmer_size=13, load_aindex=False)
    wi, wv, _ = S.select(v, 2, 30)
    assert ai.get_top_kmers(30, min_tf=2) == list(zip(S.spell13(wi), wv.tolist()))
    assert ai.get_top_kmers(1 << 70, min_tf=8) == list(zip(S.spell13(S.select(v, 8, 0)[0]), S.select(v, 8, 0)[1].tolist()))   # any Python int cuts
    st = ai.get_kmer_frequency_stats()
    assert st["kmer_type"] == "13mer" and st["total_kmers"] == n and st["total_tf"] == int(v.sum(dtype=np.uint64)) and st["max_tf"] == 0xFFFFFFFF
    assert ai._wrapper.get_13mer_statistics() == {"total_kmers": n, "non_zero_kmers": int((tf != 0).sum()), "max_frequency": 1 << 40,
                                                  "total_count": int(tf.sum(dtype=np.uint64))}
    assert ai.get_tf_spectrum(max_tf=3) == S.spectrum(v, 5).tolist()
    assert list(ai.iter_kmers_by_frequency(min_tf=1 << 33)) == []


def test_13mer_handle_and_counted_tensor(gold):
    import torch
    from pf13 import pf13_path
    tf, v, hot = _table13()
    n = tf.shape[0]
    with Index.create_13(open(pf13_path(), "rb").read(), tf) as ix:
        assert np.array_equal(_u32(ix.kmer_values_t()), v)
        hist, st = ix.tf_spectrum(12)
        assert np.array_equal(hist, S.spectrum(v, 12)) and int(hist.sum()) == n
        assert {k: st[k] for k in ("n", "non_zero", "max", "min_non_zero", "sum")} == S.stats(v)
        assert (st["non_zero_wide"], st["max_wide"], st["sum_wide"]) == (int((tf != 0).sum()), 1 << 40, int(tf.sum(dtype=np.uint64)))
        for min_tf, top in ((1, 25), (8, 0), (1, 0), (0xFFFFFFFF, 10)):
            kid, val, kmers, total = ix.top_kmers(top, min_tf)
            wi, wv, wt = S.select(v, min_tf, top)
            assert np.array_equal(kid, wi) and np.array_equal(val, wv) and total == wt, (min_tf, top)
            assert _strings(kmers) == S.spell13(wi)
        kids = np.array([0, 27, n - 1, n, 1 << 40, int(hot[0])], dtype=np.uint64)
        rows, rc, t = ix.kmers_by_kid(kids, want_rc=True, want_tf=True)
        assert _strings(rows) == S.spell13([0, 27, n - 1]) + ["", ""] + S.spell13([int(hot[0])])
        assert _strings(rc)[:3] == ["T" * 13, "ACGTTTTTTTTTT", "A" * 13] and t.tolist() == [int(v[k]) if k < n else 0 for k in kids.tolist()]
        # what count13_t leaves in HBM
        reads = open(os.path.join(gold, "count13", "synth.txt"), "rb").read()
        want = O.count13(O.OracleMphf(pf13_path()), reads, 0)
        ct = ix.count13_t(torch.from_numpy(np.frombuffer(reads, dtype=np.uint8).copy()).cuda())
        ht, stt = engine.spectrum_t(ct, 40)
        cv = (want & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        assert np.array_equal(ht.cpu().numpy().view(np.uint64), S.spectrum(cv, 40)) and stt.cpu().numpy().tolist()[:5] == list(S.stats(cv).values())
        gi, gv, total = engine.top_values_t(ct, 100, 1)
        wi, wv, wt = S.select(cv, 1, 100)
        assert np.array_equal(_u32(gi), wi) and np.array_equal(_u32(gv), wv) and total == wt


def test_bad_arguments_and_sizes(gold):
    L = _lib.lib()
    with _open(gold, "small23") as ix:
        h = ix._h
        hist, st = np.zeros(4, np.uint64), np.zeros(8, np.uint64)
        p = lambda a: a.ctypes.data_as(vp)
        assert L.aix_tf_spectrum(h, 1, p(hist), p(st)) == _lib.AIX_ERR_ARG and L.aix_tf_spectrum(h, 0, p(hist), p(st)) == _lib.AIX_ERR_ARG
        assert L.aix_tf_spectrum(h, 4, None, p(st)) == _lib.AIX_ERR_ARG and L.aix_tf_spectrum(h, 4, p(hist), None) == _lib.AIX_ERR_ARG
        assert L.aix_tf_spectrum(h, (1 << 32) + 1, p(hist), p(st)) == _lib.AIX_ERR_NOMEM
        assert L.aix_tf_spectrum(None, 4, p(hist), p(st)) == _lib.AIX_ERR_ARG
        assert L.aix_spectrum_dev(None, 4, 0, 1, p(hist), p(st), None) == _lib.AIX_ERR_ARG
        assert L.aix_spectrum_dev(None, 2, 0, 4, p(hist), p(st), None) == _lib.AIX_ERR_ARG
        m, t = C.c_uint64(), C.c_uint64()
        assert L.aix_select_dev(None, 5, 1, 1, None, None, 0, C.byref(m), C.byref(t), None) == _lib.AIX_ERR_ARG
        assert L.aix_select_dev(None, 0, 1, 1, None, None, 0, None, C.byref(t), None) == _lib.AIX_ERR_ARG
        assert L.aix_top_kmers(h, 1, 1, None, None, None, C.byref(m), C.byref(t)) == _lib.AIX_ERR_ARG
        kid = np.zeros(1, np.uint64)
        out = np.zeros(23, np.uint8)
        assert L.aix_kmers_by_kid(h, p(kid), 1 << 56, p(out), None, None) == _lib.AIX_ERR_NOMEM
        assert L.aix_kmers_by_kid(h, None, 1, p(out), None, None) == _lib.AIX_ERR_ARG and L.aix_kmers_by_kid(h, p(kid), 1, None, None, None) == _lib.AIX_ERR_ARG
        assert L.aix_kmers_by_kid(h, None, 0, None, None, None) == 0
        assert L.aix_kmer_values_dev(h, None, None) == _lib.AIX_ERR_ARG
        with pytest.raises(ValueError):
            ix.tf_spectrum(1)
        # sizing call: cap 0 reports the counts and writes nothing
        assert L.aix_top_kmers_dev(h, 2, 25, None, None, None, 0, C.byref(m), C.byref(t), None) == 0
        assert (m.value, t.value) == (25, int((np.array(_doc(gold, "small23")["values"]) >= 2).sum()))
