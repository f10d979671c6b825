"""De Bruijn neighbours and walks on the GPU (aix_debruijn.hip) against the committed reference answers and against the test-side
restatement (tests/debruijn_ref.py) over the oracle. Every comparison is exact equality; every walk is bounded by max_steps."""
import ctypes as C
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import debruijn_ref as D
import oracle_lib as O
from aindex_amd import _lib, builder
from aindex_amd.engine import Index

SETS = ["small23", "graph23"]
vp = _lib.vp


def _open(gold, name):
    p = os.path.join(gold, name, name)
    return Index.open_23(p + ".pf", p + ".tf.bin", p + ".kmers.bin")


def _doc(gold, name):
    return json.load(open(os.path.join(gold, name, "debruijn.json")))


def _rows(recs):
    """CONT records -> int array [N, 8] in the order of the goldens"""
    return np.concatenate([recs["tf"], np.stack([recs["n"], recs["sum"], recs["best_tf"], recs["best_base"]], axis=-1)], axis=-1).astype(np.int64)


def _walk_lists(bases, length, stop, tf, last):
    n = len(length)
    return ([bytes(bases[i, :length[i]]).decode() for i in range(n)], [int(x) for x in stop], [tf[i, :length[i]].tolist() for i in range(n)],
            [int(x) for x in last])


def _check_goldens(ix, doc, forms=("ascii", "codes"), dev=True):
    import torch
    q = np.frombuffer("".join(doc["queries"]).encode("latin-1"), dtype=np.uint8)
    codes = D.encode(q)
    for rec in doc["neighbours"]:
        want = {"next": np.array(rec["next"], np.int64), "prev": np.array(rec["prev"], np.int64)}
        for form in forms:
            src = q if form == "ascii" else codes
            for d in ("next", "prev"):
                assert np.array_equal(_rows(ix.neighbours(src, d, rec["cutoff"])), want[d]), (form, d, rec["cutoff"])
            both = _rows(ix.neighbours(src, "both", rec["cutoff"]))
            assert both.shape == (len(doc["queries"]), 2, 8)
            assert np.array_equal(both[:, 0], want["next"]) and np.array_equal(both[:, 1], want["prev"]), (form, rec["cutoff"])
            if dev:
                t = torch.from_numpy(src.copy()).cuda() if form == "ascii" else torch.from_numpy(src.view(np.int64).copy()).cuda()
                got = ix.neighbours_t(t, "both", rec["cutoff"]).cpu().numpy().view(np.uint32).astype(np.int64)
                assert np.array_equal(got[:, 0], want["next"]) and np.array_equal(got[:, 1], want["prev"]), (form, rec["cutoff"], "dev")
                for d in ("next", "prev"):
                    got = ix.neighbours_t(t, d, rec["cutoff"]).cpu().numpy().view(np.uint32).astype(np.int64)
                    assert np.array_equal(got, want[d]), (form, d, rec["cutoff"], "dev")
    for w in doc["walks"]:
        idx = np.array(w["seeds"])
        want = (w["bases"], w["stop"], w["tf"], w["last"])
        tag = (w["dir"], w["mode"], w["L"], w["cutoff"])
        for form in forms:
            src = np.ascontiguousarray(q.reshape(-1, 23)[idx]).reshape(-1) if form == "ascii" else codes[idx].copy()
            got = ix.walk(src, w["L"], w["dir"], w["cutoff"], w["mode"])
            assert not got[0][np.arange(w["L"])[None, :] >= got[1][:, None]].any(), (form, tag)
            assert _walk_lists(*got) == want, (form, tag)
            assert ix.walk(src, w["L"], w["dir"], w["cutoff"], w["mode"], want_tf=False)[3] is None
            if dev:
                t = torch.from_numpy(src).cuda() if form == "ascii" else torch.from_numpy(src.view(np.int64)).cuda()
                b, ln, st, tf, last = ix.walk_t(t, w["L"], ("next", "prev")[w["dir"]], w["cutoff"], ("greedy", "unitig")[w["mode"]])
                got = (b.cpu().numpy(), ln.cpu().numpy().view(np.uint32), st.cpu().numpy(), tf.cpu().numpy().view(np.uint32), last.cpu().numpy().view(np.uint64))
                assert _walk_lists(*got) == want, (form, tag, "dev")


@pytest.mark.parametrize("name", SETS)
def test_goldens_through_every_form(gold, name):
    """1. The reference's answers: host and device forms, ASCII and code inputs, NEXT / PREV / BOTH, greedy and unitig."""
    with _open(gold, name) as ix:
        _check_goldens(ix, _doc(gold, name))


def test_list_surface_on_the_goldens(gold, small23_prefix):
    from aindex_amd.aindex import AIndex
    doc = _doc(gold, "small23")
    ai = AIndex.load_from_prefix(small23_prefix)
    try:
        items = list(doc["queries"][:60])
        items[3:3] = ["", "ACGT", items[0] + "A"]
        keep = [i for i, s in enumerate(items) if len(s) == 23]
        rec0 = doc["neighbours"][0]
        for fn, key in ((ai.get_next_batch, "next"), (ai.get_prev_batch, "prev")):
            got = fn(items)
            assert [got[i] for i in (3, 4, 5)] == [{}, {}, {}]
            for j, i in enumerate(keep):
                r = rec0[key][j]
                assert got[i] == {"A": r[0], "C": r[1], "G": r[2], "T": r[3], "n": r[4], "sum": r[5], "best_hit_tf": r[6], "best_hit": "ACGT"[r[7]]}
        w = {(x["dir"], x["mode"], x["cutoff"]): x for x in doc["walks"] if x["L"] == 200}
        seeds = [doc["queries"][i] for i in w[(0, 0, 0)]["seeds"]]
        nxt, prv = w[(0, 0, 0)], w[(1, 0, 0)]
        probe = seeds[:20] + ["ACGT"]
        got_n = ai.extend_batch(probe, 200, 0, "greedy", "next")
        got_p = ai.extend_batch(probe, 200, 0, "greedy", "prev")
        got_b = ai.extend_batch(probe, 200, 0, "greedy", "both")
        assert got_n[-1] == ("", "") and got_b[-1] == ("", "", "")
        for j in range(20):
            assert got_n[j] == (nxt["bases"][j], D.STOP_NAMES[nxt["stop"][j]])
            assert got_p[j] == (prv["bases"][j][::-1], D.STOP_NAMES[prv["stop"][j]])
            assert got_b[j] == (prv["bases"][j][::-1] + seeds[j] + nxt["bases"][j], D.STOP_NAMES[prv["stop"][j]], D.STOP_NAMES[nxt["stop"][j]])
        un = w[(0, 1, 0)]
        got_u = ai.extend_batch(seeds[:20], 200, 0, "unitig")
        assert got_u == [(un["bases"][j], D.STOP_NAMES[un["stop"][j]]) for j in range(20)]
    finally:
        ai._wrapper.close()


def test_neighbours_equal_the_composition_of_tf_codes(gold):
    """2. A consistency check, HIP against HIP: the tf of a neighbours call are tf_codes_t on the 4 N neighbour codes."""
    import torch
    with _open(gold, "small23") as ix:
        checker = ix.checker_array()
        rng = np.random.default_rng(5)
        codes = np.concatenate([checker, D.revcomp(checker[::3]), rng.integers(0, 1 << 46, 20000, dtype=np.uint64)])
        t = torch.from_numpy(codes.view(np.int64)).cuda()
        for d, name in ((D.NEXT, "next"), (D.PREV, "prev")):
            nb = np.stack([D.neigh(codes, d, b) for b in range(4)], axis=1).reshape(-1)
            tf = ix.tf_codes_t(torch.from_numpy(nb.view(np.int64)).cuda()).cpu().numpy().view(np.uint32).reshape(-1, 4)
            got = ix.neighbours_t(t, name).cpu().numpy().view(np.uint32)
            assert np.array_equal(got[:, :4], tf)
            assert np.array_equal(got[:, 4], (tf != 0).sum(axis=1)) and np.array_equal(got[:, 5], tf.sum(axis=1, dtype=np.uint32))
            assert (tf != 0).any(axis=1).mean() > 0.2


def _seeded_reads(rng):
    """A 300 kbp random genome with a 400 bp repeat planted 12 times and 10 tandem arrays (units of 24 .. 36 bp, 30 copies), read at
    8 x by 150 bp reads of either strand with 0.5 % substitutions."""
    g = rng.integers(0, 4, 300_000).astype(np.uint8)
    rep = rng.integers(0, 4, 400).astype(np.uint8)
    for p in rng.choice(np.arange(1000, 280_000, 2000), 12, replace=False):
        g[p:p + 400] = rep
    arrays = []
    for a in range(10):
        unit = rng.integers(0, 4, 24 + (a * 4) % 13).astype(np.uint8)
        p = 1000 + 29_000 * a + 700
        g[p:p + 30 * len(unit)] = np.tile(unit, 30)
        arrays.append((p, len(unit)))
    n_reads = 8 * len(g) // 150
    starts = rng.integers(0, len(g) - 150, n_reads)
    reads = g[starts[:, None] + np.arange(150)[None, :]]
    sub = rng.random(reads.shape) < 0.005
    reads = np.where(sub, (reads + rng.integers(1, 4, reads.shape)) % 4, reads).astype(np.uint8)
    flip = rng.random(n_reads) < 0.5
    reads[flip] = (3 - reads[flip])[:, ::-1]
    plain = np.concatenate([D.LETTERS[reads], np.full((n_reads, 1), 10, np.uint8)], axis=1).reshape(-1)
    return D.LETTERS[g], plain, arrays


@pytest.fixture(scope="module")
def seeded(tmp_path_factory):
    """The index of the reads' own distinct 23-mers built on the device, and the oracle over the same .pf / keys / tf."""
    import torch
    from aindex_amd import counting
    rng = np.random.default_rng(20240)
    genome, plain, arrays = _seeded_reads(rng)
    keys, counts = counting.count_distinct_t(torch.from_numpy(plain).cuda(), 23, _lib.CANON_TRUE_RC)
    pf = builder.build_pf_codes_t(keys, 23)
    ix = Index.build_23_codes_t(pf, keys, counts.to(torch.int32))
    torch.cuda.synchronize()
    d = tmp_path_factory.mktemp("dbj")
    paths = [str(d / n) for n in ("s.pf", "s.tf.bin", "s.kmers.bin")]
    open(paths[0], "wb").write(pf)
    ix.tf_array().tofile(paths[1])
    ix.checker_array().tofile(paths[2])
    orc = O.OracleIndex23(*paths)
    # seeds: genome windows everywhere, every window of the tandem arrays, read windows (substitutions), both strands
    w = np.lib.stride_tricks.sliding_window_view(genome, 23)
    at = rng.integers(0, w.shape[0], 90_000)
    arr = np.concatenate([np.arange(p - 30, p + 30 * u) for p, u in arrays])
    rw = np.lib.stride_tricks.sliding_window_view(plain[: 151 * 200], 23)
    rw = rw[(rw != 10).all(axis=1)]
    seeds = np.concatenate([D.encode(np.ascontiguousarray(w[at])), D.encode(np.ascontiguousarray(w[arr])), D.encode(np.ascontiguousarray(rw))])
    seeds[::7] = D.revcomp(seeds[::7])
    seeds = seeds[rng.permutation(seeds.shape[0])]
    assert seeds.shape[0] >= 100_000
    yield {"ix": ix, "freq": D.oracle_freq(orc, threads=8), "seeds": seeds}
    ix.close()


def test_seeded_index_against_the_helper_over_the_oracle(seeded):
    """3. >= 10^5 seeds on an index built on the device: neighbours in both directions, a greedy and a unitig leg; every stop reason
    occurs at least 100 times in the helper's answer."""
    import torch
    ix, freq, seeds = seeded["ix"], seeded["freq"], seeded["seeds"]
    t = torch.from_numpy(seeds.view(np.int64)).cuda()
    want = D.neighbours(freq, seeds, D.BOTH, 2)
    got = ix.neighbours_t(t, "both", 2).cpu().numpy().view(np.uint32)
    assert np.array_equal(got.astype(np.int64), _rows(want))
    assert (want["n"] > 1).sum() >= 100 and (want["n"] == 0).sum() >= 100
    hist = np.zeros(5, np.int64)
    for direction, mode, cutoff, L in ((D.NEXT, D.GREEDY, 0, 40), (D.PREV, D.UNITIG, 1, 40)):
        wb, wl, ws, wt, wlast = D.walk(freq, seeds, direction, L, cutoff, mode)
        hist += np.bincount(ws, minlength=5)
        b, ln, st, tf, last = ix.walk_t(t, L, direction, cutoff, mode)
        torch.cuda.synchronize()
        assert np.array_equal(ln.cpu().numpy().view(np.uint32), wl) and np.array_equal(st.cpu().numpy(), ws)
        assert np.array_equal(last.cpu().numpy().view(np.uint64), wlast)
        assert np.array_equal(b.cpu().numpy(), wb) and np.array_equal(tf.cpu().numpy().view(np.uint32), wt)
        print("dir", direction, "mode", mode, "stops", np.bincount(ws, minlength=5).tolist(), "mean length", float(wl.mean()))
    print("stop histogram", dict(zip(D.STOP_NAMES, hist.tolist())))
    assert (hist >= 100).all(), hist


def test_answers_do_not_depend_on_any_switch(gold, monkeypatch):
    """4. Verification table on / off and 8, 4, 2, 1 lanes per line, absence filter, fingerprints, early exit, canonical fast path, and the
    three absence-filter policies of these kernels: the goldens every time."""
    for name in SETS:
        doc = _doc(gold, name)
        doc["walks"] = [w for w in doc["walks"] if w["L"] != 7]
        with _open(gold, name) as ix:
            n = 0
            for policy in ("0", "1", "2"):
                monkeypatch.setenv("AIX_DBJ_FILTER", policy)
                for table, lanes in ((True, 8), (True, 1), (False, 0)):
                    for filt in (True, False):
                        for fp, ee, canon in ((True, True, True), (False, False, False), (True, False, True)):
                            ix.set_bucket_table(table, lanes)
                            ix.set_absence_filter(filt)
                            ix.set_fingerprint_filter(fp)
                            ix.set_early_exit(ee)
                            ix.set_canonical_fastpath(canon)
                            _check_goldens(ix, doc, forms=("codes",), dev=False)
                            n += 1
            for lanes in (4, 2):
                ix.set_bucket_table(True, lanes)
                _check_goldens(ix, doc, forms=("ascii",), dev=False)
            assert n == 54


def test_rows_beyond_the_length_stay_untouched_past_4_gib(gold):
    """5. S * max_steps = 4.3 * 10^9 cells: rows written into canary-filled tensors; what lies at or beyond a row's length keeps the canary
    everywhere, and sampled rows — the last ones, whose offsets pass 2^32, among them — equal the helper's."""
    import torch
    L, S = 4100, (1 << 20) + 64
    assert S * L > 1 << 32
    p = os.path.join(gold, "small23", "small23")
    freq = D.oracle_freq(O.OracleIndex23.from_prefix(p))
    with _open(gold, "small23") as ix:
        checker = ix.checker_array()
        rng = np.random.default_rng(8)
        seeds = rng.integers(0, 1 << 46, S, dtype=np.uint64)
        stored_at = np.concatenate([rng.choice(S, 3000, replace=False), np.arange(S - 40, S)])
        seeds[stored_at] = checker[rng.integers(0, checker.shape[0], stored_at.shape[0])]
        t = torch.from_numpy(seeds.view(np.int64)).cuda()
        bases = torch.full((S, L), 0xEE, dtype=torch.uint8, device="cuda")
        b, ln, st, tf, last = ix.walk_t(t, L, "next", 0, "greedy", want_tf=False, bases_t=bases)
        torch.cuda.synchronize()
        assert tf is None and b.data_ptr() == bases.data_ptr()
        ln_h = ln.cpu().numpy().view(np.uint32)
        written = 0
        for lo in range(0, S, 1 << 16):                              # every byte that is not the canary lies below its row's length
            blk = bases[lo:lo + (1 << 16)]
            inside = torch.arange(L, device="cuda")[None, :] < ln[lo:lo + (1 << 16), None]
            assert bool(((blk != 0xEE) == inside).all()), lo
            written += int(inside.sum())
        assert written == int(ln_h.sum(dtype=np.int64)) > 10_000
        sample = np.unique(np.concatenate([stored_at[::25], np.arange(S - 40, S), np.arange(0, S, 40_000)]))
        assert (sample.astype(np.int64) * L > 1 << 32).sum() >= 40
        wb, wl, ws, _, wlast = D.walk(freq, seeds[sample], D.NEXT, L, 0, D.GREEDY)
        assert np.array_equal(ln_h[sample], wl) and np.array_equal(st.cpu().numpy()[sample], ws)
        assert np.array_equal(last.cpu().numpy().view(np.uint64)[sample], wlast)
        gb = bases[torch.from_numpy(sample).cuda()].cpu().numpy()
        assert np.array_equal(np.where(np.arange(L)[None, :] < wl[:, None], gb, 0), wb)
        assert wl.max() > 20 and (wl == 0).sum() > 20                # ragged rows
        # the host form keeps the caller's bytes beyond the length too
        hb = np.full((50, 9), 0xEE, np.uint8)
        hl, hs = np.zeros(50, np.uint32), np.zeros(50, np.uint8)
        sd = np.ascontiguousarray(seeds[sample[:50]])
        _lib.check(_lib.lib().aix_walk(ix._h, sd.ctypes.data_as(vp), None, 50, 0, 9, 0, 0, hb.ctypes.data_as(vp), hl.ctypes.data_as(vp),
                                       hs.ctypes.data_as(vp), None, None))
        xb, xl, xs, _, _ = D.walk(freq, sd, D.NEXT, 9, 0, D.GREEDY)
        assert np.array_equal(hl, xl) and np.array_equal(hs, xs) and np.array_equal(hb, np.where(np.arange(9)[None, :] < xl[:, None], xb, 0xEE))
        assert 0 < (hl < 9).sum() and (hl > 0).sum() > 0


def test_empty_batches_wrong_mode_and_bad_arguments(gold):
    """6. N = 0 and S = 0 succeed; a 13-mer handle is AIX_ERR_MODE; max_steps out of range, a bad direction or mode, both or neither
    input form, a missing output are AIX_ERR_ARG; a product S * max_steps that no buffer holds is AIX_ERR_NOMEM. Nothing aborts."""
    import torch
    from pf13 import pf13_path
    L_ = _lib.lib()
    with _open(gold, "graph23") as ix:
        assert ix.neighbours(b"").shape == (0,) and ix.neighbours(np.zeros(0, np.uint64), "both").shape == (0, 2)
        b, ln, st, tf, last = ix.walk(b"", 5)
        assert b.shape == (0, 5) and ln.shape == (0,) and st.shape == (0,) and tf.shape == (0, 5) and last.shape == (0,)
        e64, e8 = torch.zeros(0, dtype=torch.int64, device="cuda"), torch.zeros(0, dtype=torch.uint8, device="cuda")
        assert ix.neighbours_t(e64, "both").shape == (0, 2, 8) and ix.neighbours_t(e8).shape == (0, 8)
        assert ix.walk_t(e64, 3)[0].shape == (0, 3)
        assert L_.aix_neighbours(ix._h, None, None, 0, 2, 0, None) == 0 and L_.aix_walk(ix._h, None, None, 0, 0, 1, 0, 0, None, None, None, None, None) == 0
        buf = np.zeros(256, np.uint64)
        p = buf.ctypes.data_as(vp)
        ARG = _lib.AIX_ERR_ARG
        assert L_.aix_neighbours(ix._h, p, p, 1, 0, 0, p) == ARG and L_.aix_neighbours(ix._h, None, None, 1, 0, 0, p) == ARG
        assert L_.aix_neighbours(ix._h, p, None, 1, 3, 0, p) == ARG and L_.aix_neighbours(ix._h, p, None, 1, -1, 0, p) == ARG
        assert L_.aix_neighbours(ix._h, p, None, 1, 0, 0, None) == ARG
        for steps in (0, (1 << 20) + 1, 1 << 40):
            assert L_.aix_walk(ix._h, p, None, 1, 0, steps, 0, 0, p, p, p, None, None) == ARG
            assert L_.aix_walk_dev(ix._h, p, None, 1, 0, steps, 0, 0, p, p, p, None, None, None) == ARG
        assert L_.aix_walk(ix._h, p, None, 1, 2, 4, 0, 0, p, p, p, None, None) == ARG        # BOTH is not a walk direction
        assert L_.aix_walk(ix._h, p, None, 1, 0, 4, 0, 2, p, p, p, None, None) == ARG
        assert L_.aix_walk(ix._h, p, None, 1, 0, 4, 0, 0, None, p, p, None, None) == ARG
        assert L_.aix_walk(ix._h, p, p, 1, 0, 4, 0, 0, p, p, p, None, None) == ARG
        assert L_.aix_walk(ix._h, p, None, 1 << 50, 0, 1 << 20, 0, 0, p, p, p, None, None) == _lib.AIX_ERR_NOMEM
        assert L_.aix_walk_dev(ix._h, p, None, 1 << 50, 0, 1 << 20, 0, 0, p, p, p, None, None, None) == _lib.AIX_ERR_NOMEM
        with pytest.raises(ValueError):
            ix.walk(buf[:1], 0)
        with pytest.raises(ValueError):
            ix.walk(buf[:1], 5, "both")
        assert ix.walk(buf[:2], 1 << 20, want_tf=False)[1].shape == (2,)                      # the largest max_steps is accepted
    with Index.open_13(pf13_path(), None) as ix13:
        p = np.zeros(64, np.uint64).ctypes.data_as(vp)
        assert L_.aix_neighbours(ix13._h, p, None, 1, 0, 0, p) == _lib.AIX_ERR_MODE
        assert L_.aix_neighbours_dev(ix13._h, p, None, 1, 0, 0, p, None) == _lib.AIX_ERR_MODE
        assert L_.aix_walk(ix13._h, p, None, 1, 0, 4, 0, 0, p, p, p, None, None) == _lib.AIX_ERR_MODE
        assert L_.aix_walk_dev(ix13._h, p, None, 1, 0, 4, 0, 0, p, p, p, None, None, None) == _lib.AIX_ERR_MODE
        with pytest.raises(_lib.AixError):
            ix13.neighbours(np.zeros(1, np.uint64))
