"""De Bruijn neighbours and walks, host side (no GPU): the committed reference answers against the test-side restatement over the
oracle, the ABI surface, the public methods, the list surface's placing of wrong-length items, and the argument errors that need no device;
the graph cases of the GPU fuzz (tests/graph_cases.py): a scalar restatement against the vectorised one, and what the cases must contain."""
import functools
import json
import os
import re

import numpy as np
import pytest

import debruijn_ref as D
import graph_cases as G
import oracle_lib as O
from aindex_amd import _lib
from aindex_amd.aindex import AIndex
from aindex_amd.engine import Index
from aindex_amd.wrapper import AindexWrapper

NEW = ["aix_neighbours", "aix_neighbours_dev", "aix_walk", "aix_walk_dev"]
SETS = ["small23", "graph23"]


def load_set(gold, name):
    doc = json.load(open(os.path.join(gold, name, "debruijn.json")))
    return doc, os.path.join(gold, name, name)


@pytest.mark.parametrize("name", SETS)
def test_helper_reproduces_every_golden(gold, name):
    doc, prefix = load_set(gold, name)
    freq = D.oracle_freq(O.OracleIndex23.from_prefix(prefix))
    codes = D.encode("".join(doc["queries"]).encode("latin-1"))
    assert codes.shape[0] == len(doc["queries"]) > 150
    for rec in doc["neighbours"]:
        for key, direction in (("next", D.NEXT), ("prev", D.PREV)):
            got = D.cont(freq, codes, direction, rec["cutoff"])
            want = np.array(rec[key], dtype=np.uint32)
            assert np.array_equal(got["tf"], want[:, :4]), (name, key, rec["cutoff"])
            for j, f in enumerate(("n", "sum", "best_tf", "best_base")):
                assert np.array_equal(got[f], want[:, 4 + j]), (name, key, rec["cutoff"], f)
    assert len(doc["walks"]) == 24
    for w in doc["walks"]:
        seeds = codes[np.array(w["seeds"])]
        bases, length, stop, tf, last = D.walk(freq, seeds, w["dir"], w["L"], w["cutoff"], w["mode"])
        tag = (name, w["dir"], w["mode"], w["L"], w["cutoff"])
        assert [bases[i, :length[i]].tobytes().decode() for i in range(len(seeds))] == w["bases"], tag
        assert stop.tolist() == w["stop"] and last.tolist() == w["last"], tag
        assert [tf[i, :length[i]].tolist() for i in range(len(seeds))] == w["tf"], tag
        assert not bases[np.arange(w["L"])[None, :] >= length[:, None]].any(), tag


def test_goldens_hold_every_stop_reason_a_tie_and_an_empty_cont(gold):
    stops, tie, zero, at_cutoff = set(), False, False, False
    for name in SETS:
        doc, _ = load_set(gold, name)
        for w in doc["walks"]:
            stops |= set(w["stop"])
        for rec in doc["neighbours"]:
            rows = np.array(rec["next"] + rec["prev"], dtype=np.int64)
            t = np.sort(rows[:, :4], axis=1)
            tie |= bool(((t[:, 3] == t[:, 2]) & (t[:, 2] > 0)).any())
            zero |= bool((rows[:, 4] == 0).any())
        if "cutoff_equal_to_a_tf" in doc:                           # the inclusive comparison: a tf equal to the cutoff is met and zeroed
            c = doc["cutoff_equal_to_a_tf"]
            r0 = np.array(doc["neighbours"][0]["next"])[:, :4]
            rc = np.array([r for r in doc["neighbours"] if r["cutoff"] == c][0]["next"])[:, :4]
            at_cutoff = bool((r0 == c).any()) and bool((rc[r0 == c] == 0).all())
    assert stops == {D.MAX_STEPS, D.DEAD_END, D.BRANCH, D.JOIN, D.LOOP} and tie and zero and at_cutoff


def test_header_declares_and_lib_binds_the_entry_points():
    declared = _lib.header_symbols()
    L = _lib.lib()
    for name in NEW:
        assert name in declared, name
        res, args = _lib.SIGNATURES[name]
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert [len(_lib.SIGNATURES[n][1]) for n in NEW] == [7, 8, 13, 14]
    text = open(_lib.HEADER).read()
    for name in NEW:                                                # every declaration names the reference lines it replaces
        at = text.index(f" {name}(")
        comment = text[text[:at].rfind("\n/* "):at]                # the comment block in front of the declaration
        assert re.search(r"debrujin\.cpp:\d+", comment), name
    # the record and the constants the binding mirrors
    assert _lib.cont_dtype().itemsize == 32 and _lib.cont_dtype() == D.CONT_DTYPE
    consts = dict(re.findall(r"#define (AIX_(?:DIR|WALK|STOP)_\w+)\s+(\d+)", text))
    assert [int(consts[f"AIX_DIR_{n}"]) for n in ("NEXT", "PREV", "BOTH")] == [_lib.DIR_NEXT, _lib.DIR_PREV, _lib.DIR_BOTH] == [D.NEXT, D.PREV, D.BOTH]
    assert [int(consts[f"AIX_WALK_{n}"]) for n in ("GREEDY", "UNITIG")] == [_lib.WALK_GREEDY, _lib.WALK_UNITIG] == [D.GREEDY, D.UNITIG]
    assert [int(consts[f"AIX_STOP_{n.upper()}"]) for n in _lib.STOP_NAMES] == [0, 1, 2, 3, 4] and _lib.STOP_NAMES == D.STOP_NAMES
    assert int(consts["AIX_WALK_MAX_STEPS"]) == _lib.WALK_MAX_STEPS == 1 << 20
    assert int(re.search(r"#define AIX_ERR_MODE\s+(-\d+)", text).group(1)) == _lib.AIX_ERR_MODE


def test_public_methods_exist():
    for m in ("neighbours", "walk", "neighbours_t", "walk_t"):
        assert callable(getattr(Index, m)), m
    for cls in (AindexWrapper, AIndex):
        for m in ("get_next_batch", "get_prev_batch", "extend_batch"):
            assert callable(getattr(cls, m)), (cls, m)


def test_list_surface_places_empty_answers_for_wrong_length_items():
    items = ["ACGTACGTACGTACGTACGTACG", "", "ACGTACGTACGTACGTACGTAC", b"TTTTTTTTTTTTTTTTTTTTTTT", "ACGTACGTACGTACGTACGTACGT"]
    flat, keep = AindexWrapper._split_fixed(items, 23)
    assert keep.tolist() == [0, 3]
    recs = np.zeros(2, dtype=_lib.cont_dtype())
    recs["tf"] = [[1, 0, 5, 5], [0, 0, 0, 0]]
    recs["n"], recs["sum"], recs["best_tf"], recs["best_base"] = [3, 0], [11, 0], [5, 0], [3, 3]
    got = AindexWrapper._place_conts(len(items), keep, recs)
    assert got == [{"A": 1, "C": 0, "G": 5, "T": 5, "n": 3, "sum": 11, "best_hit": "T", "best_hit_tf": 5}, {}, {},
                   {"A": 0, "C": 0, "G": 0, "T": 0, "n": 0, "sum": 0, "best_hit": "T", "best_hit_tf": 0}, {}]
    bases = np.frombuffer(b"ACG\0\0" + b"\0\0\0\0\0", dtype=np.uint8).reshape(2, 5)
    length = np.array([3, 0], np.uint32)
    right = (AindexWrapper._row_strings(bases, length, False), ["dead_end", "loop"])
    left = (AindexWrapper._row_strings(bases, length, True), ["branch", "max_steps"])
    assert right[0] == ["ACG", ""] and left[0] == ["GCA", ""]
    assert AindexWrapper._place_extensions(items, keep, "next", right, left) == [("ACG", "dead_end"), ("", ""), ("", ""), ("", "loop"), ("", "")]
    assert AindexWrapper._place_extensions(items, keep, "prev", right, left) == [("GCA", "branch"), ("", ""), ("", ""), ("", "max_steps"), ("", "")]
    both = AindexWrapper._place_extensions(items, keep, "both", right, left)
    assert both == [("GCA" + items[0] + "ACG", "branch", "dead_end"), ("", "", ""), ("", "", ""), ("T" * 23, "max_steps", "loop"), ("", "", "")]
    # nothing of the right length: no handle is needed to answer
    w = AindexWrapper.__new__(AindexWrapper)
    assert w.get_next_batch(["ACGT", ""]) == [{}, {}] and w.extend_batch(["ACGT"], direction="both") == [("", "", "")]
    with pytest.raises(ValueError):
        w.extend_batch(["ACGT"], direction="sideways")


def test_argument_errors_that_need_no_device():
    L = _lib.lib()
    buf = np.zeros(64, np.uint64)
    p = buf.ctypes.data_as(_lib.vp)
    assert L.aix_neighbours(None, p, None, 1, 0, 0, p) == _lib.AIX_ERR_ARG
    assert L.aix_neighbours_dev(None, p, None, 1, 0, 0, p, None) == _lib.AIX_ERR_ARG
    assert L.aix_walk(None, p, None, 1, 0, 7, 0, 0, p, p, p, None, None) == _lib.AIX_ERR_ARG
    assert L.aix_walk_dev(None, p, None, 1, 0, 7, 0, 0, p, p, p, None, None, None) == _lib.AIX_ERR_ARG
    with pytest.raises(ValueError):
        Index._dir("both", False)
    with pytest.raises(ValueError):
        Index._walk_mode("eager")
    assert Index._dir("prev", False) == 1 and Index._dir("both", True) == 2 and Index._walk_mode("unitig") == 1


# ------------------------------------------------------------------------------------------------
# The graph cases of test_gpu_fuzz.py::test_fuzz_debruijn. The GPU test compares the kernels with debruijn_ref over the oracle; here
# debruijn_ref itself is compared with a second statement of the same rules, one k-mer at a time over a dict, and the cases are shown
# to hold the situations they were built for (a GPU test over a case without them would pass and say nothing).
# ------------------------------------------------------------------------------------------------
GRAPH_SEEDS = range(12)
_M46 = (1 << 46) - 1


class Scalar:
    """get_freq (hash.hpp:123-140), print_next / print_prev (debrujin.cpp:30-75, 121-167) and the bounded walk of include/aindex_hip.h,
    on Python ints over a dict of the stored codes. Nothing of debruijn_ref is called."""

    def __init__(self, codes, tfs):
        self.table = dict(zip(codes.tolist(), tfs.tolist()))
        self.rc_cache, self.cont_cache = {}, {}

    def rc(self, x):
        y = self.rc_cache.get(x)
        if y is None:
            y, v = 0, x
            for _ in range(23):                                     # the bases in reverse order, each complemented
                y = (y << 2) | (3 - (v & 3))
                v >>= 2
            self.rc_cache[x] = y
        return y

    def freq(self, kmer):
        t = self.table.get(kmer)                                    # the k-mer as given; a stored 0 counts as stored
        if t is not None:
            return t
        return self.table.get(self.rc(kmer), 0)                     # not stored: its reverse complement, 0 when that is not stored either

    @staticmethod
    def neigh(kmer, direction, b):
        return ((kmer << 2) | b) & _M46 if direction == D.NEXT else (kmer >> 2) | (b << 44)

    def cont(self, kmer, direction, cutoff):
        """(A, C, G, T, n, sum, best_hit_tf, best_hit 0..3); a pure function of its arguments, kept per k-mer (the walks of a case
        pass through the same k-mers many times)"""
        key = (kmer, direction, cutoff)
        if key not in self.cont_cache:
            self.cont_cache[key] = self._cont(kmer, direction, cutoff)
        return self.cont_cache[key]

    def _cont(self, kmer, direction, cutoff):
        A, C, G, T = (self.freq(self.neigh(kmer, direction, b)) for b in range(4))
        if cutoff > 0:
            if A <= cutoff: A = 0
            if C <= cutoff: C = 0
            if G <= cutoff: G = 0
            if T <= cutoff: T = 0
        total = (A + C + G + T) & 0xFFFFFFFF                        # uint32_t sum
        n = int(bool(A)) + int(bool(C)) + int(bool(G)) + int(bool(T))
        best = best_tf = None
        if A >= C and A >= G and A >= T: best, best_tf = 0, A
        if C >= A and C >= G and C >= T: best, best_tf = 1, C
        if G >= C and G >= A and G >= T: best, best_tf = 2, G
        if T >= C and T >= G and T >= A: best, best_tf = 3, T
        return A, C, G, T, n, total, best_tf, best

    def walk(self, seed, direction, max_steps, cutoff, mode):
        """(bases, stop, tf list, last)"""
        seed &= _M46
        cur, bases, tfs, stop = seed, [], [], D.MAX_STEPS
        seed_c = min(seed, self.rc(seed))
        for _ in range(max_steps):
            c = self.cont(cur, direction, cutoff)
            if c[4] == 0:
                stop = D.DEAD_END
                break
            if mode == D.UNITIG and c[4] > 1:
                stop = D.BRANCH
                break
            nxt = self.neigh(cur, direction, c[7])
            if mode == D.UNITIG and self.cont(nxt, 1 - direction, cutoff)[4] > 1:
                stop = D.JOIN
                break
            if min(nxt, self.rc(nxt)) == seed_c:
                stop = D.LOOP
                break
            bases.append("ACGT"[c[7]])
            tfs.append(c[6])
            cur = nxt
        return "".join(bases), stop, tfs, cur


WALK_L = 64
WALK_LEGS = [(d, m, c) for d in (D.NEXT, D.PREV) for m in (D.GREEDY, D.UNITIG) for c in (0, 3)]


@functools.lru_cache(maxsize=None)
def graph_ref(seed):
    """The case and debruijn_ref's answers over a dict-backed freq: neighbours per (direction, cutoff), walks per (direction, mode, cutoff)."""
    codes, tfs, seeds = G.make_graph_case(seed)
    freq = G.dict_freq(codes, tfs)
    nb = {(d, c): D.neighbours(freq, seeds, d, c) for d in (D.NEXT, D.PREV) for c in (0, 3)}
    walks = {leg: D.walk(freq, seeds, leg[0], WALK_L, leg[2], leg[1]) for leg in WALK_LEGS}
    return codes, tfs, seeds, nb, walks


def test_graph_case_is_deterministic_and_of_the_promised_shape():
    for seed in GRAPH_SEEDS:
        codes, tfs, seeds = G.make_graph_case(seed)
        again = G.make_graph_case(seed)
        assert all(np.array_equal(a, b) for a, b in zip((codes, tfs, seeds), again))
        assert codes.dtype == np.uint64 and tfs.dtype == np.uint32 and seeds.dtype == np.uint64 and codes.shape == tfs.shape
        assert np.array_equal(codes, np.unique(codes)) and int(codes.max()) <= _M46
        assert 1000 < codes.shape[0] < 10_000 and seeds.shape[0] <= 20_000
        canonical = bool(np.all(codes <= D.revcomp(codes)))
        assert canonical == (seed % 3 == 0), seed                   # mode 0 is the canonical fast path, the other two are not
        high = (seeds >> np.uint64(46)) != 0
        assert 0.03 < high.mean() < 0.07
        stored = np.isin(seeds & D.MASK46, codes)
        assert stored.sum() >= codes.shape[0] and (~stored & ~np.isin(D.revcomp(seeds & D.MASK46), codes)).sum() >= 500
        assert set(G.TF_POOL.tolist()) <= set(tfs.tolist())


@pytest.mark.parametrize("seed", GRAPH_SEEDS)
def test_scalar_restatement_equals_the_vectorised_helper(seed):
    """Every seed's CONT in both directions at cutoff 0 and 3, and every seed's walk in both directions and both modes at cutoff 0 and 3
    with max_steps 1, 7 and 64, stated one k-mer at a time over a dict == debruijn_ref over a dict-backed freq."""
    codes, tfs, seeds, nb, walks = graph_ref(seed)
    sc = Scalar(codes, tfs)
    kmers = (seeds & D.MASK46).tolist()
    for (d, cutoff), recs in nb.items():
        want = np.concatenate([recs["tf"], np.stack([recs["n"], recs["sum"], recs["best_tf"], recs["best_base"]], axis=-1)], axis=-1).tolist()
        got = [list(sc.cont(k, d, cutoff)) for k in kmers]
        assert got == want, (seed, d, cutoff)
    freq = G.dict_freq(codes, tfs)
    raw = seeds.tolist()                                            # the walk masks bits 46 .. 63 itself
    for (d, m, cutoff), long_walk in walks.items():
        for L in (1, 7, WALK_L):
            bases, length, stop, tf, last = long_walk if L == WALK_L else D.walk(freq, seeds, d, L, cutoff, m)
            got = [sc.walk(s, d, L, cutoff, m) for s in raw]
            want = [(bytes(bases[i, :length[i]]).decode(), int(stop[i]), tf[i, :length[i]].tolist(), int(last[i])) for i in range(len(raw))]
            assert got == want, (seed, d, m, cutoff, L)
            assert not bases[np.arange(L)[None, :] >= length[:, None]].any()


def test_graph_cases_hold_what_they_were_built_for():
    """Floors over seeds 0 .. 11 together, computed from debruijn_ref alone: the situations the GPU fuzz is there to meet."""
    stops = np.zeros((2, 5), np.int64)
    fwd_decides = zero_shadows = wraps = zero_quads = stored_zero_quads = 0
    ties = {2: 0, 3: 0, 4: 0}
    at = {2: 0, 3: 0, 4: 0}
    for seed in GRAPH_SEEDS:
        codes, tfs, seeds, nb, walks = graph_ref(seed)
        for (d, m, cutoff), w in walks.items():
            stops[d] += np.bincount(w[2], minlength=5)
        k = seeds & D.MASK46

        def stored(x):                                              # (is stored, its tf)
            i = np.minimum(np.searchsorted(codes, x), codes.shape[0] - 1)
            return codes[i] == x, tfs[i]

        for d in (D.NEXT, D.PREV):
            probed = np.stack([D.neigh(k, d, b) for b in range(4)], axis=1)
            f_in, f_tf = stored(probed)
            r_in, r_tf = stored(D.revcomp(probed))
            fwd_decides += int((f_in & r_in & (f_tf != r_tf)).sum())
            zero_shadows += int((f_in & r_in & (f_tf == 0) & (r_tf > 0)).sum())
            raw = nb[(d, 0)]["tf"]
            assert np.array_equal(raw, np.where(f_in, f_tf, np.where(r_in, r_tf, 0)))
            wraps += int((raw.astype(np.uint64).sum(axis=1) > 0xFFFFFFFF).sum())
            for v in at:
                at[v] += int((raw == v).sum())
            for cutoff in (0, 3):
                t = nb[(d, cutoff)]["tf"]
                top = t.max(axis=1)
                width = (t == top[:, None]).sum(axis=1)
                for m in ties:
                    ties[m] += int(((width == m) & (top > 0)).sum())
                zero_quads += int((top == 0).sum())
                stored_zero_quads += int(((top == 0) & (f_in | r_in).any(axis=1)).sum())
    print("stops next", dict(zip(D.STOP_NAMES, stops[0].tolist())), "prev", dict(zip(D.STOP_NAMES, stops[1].tolist())))
    print("forward decides", fwd_decides, "stored 0 shadows", zero_shadows, "sum wraps", wraps, "ties", ties, "all-zero quads", zero_quads,
          "of them with a stored neighbour", stored_zero_quads, "tf at 2 / 3 / 4", at)
    assert (stops >= 50).all(), stops
    assert fwd_decides >= 200 and zero_shadows >= 50 and wraps >= 10
    assert min(ties.values()) >= 20 and zero_quads >= 20 and stored_zero_quads >= 20
    assert min(at.values()) >= 20
