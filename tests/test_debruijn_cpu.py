"""De Bruijn neighbours and walks, host side (no GPU): the committed reference answers against the test-side restatement over the
oracle, the ABI surface, the public methods, the list surface's placing of wrong-length items, and the argument errors that need no device."""
import json
import os
import re

import numpy as np
import pytest

import debruijn_ref as D
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
