"""Batch position queries, host side (no GPU): the ABI surface, the sorted / disjoint check of the read intervals, and the list
surface's placing of wrong-length items."""
import ctypes as C
import json
import os
import re

import numpy as np

from aindex_amd import _lib
from aindex_amd.wrapper import AindexWrapper

NEW = ["aix_aindex_attach", "aix_aindex_attach_dev", "aix_aindex_detach", "aix_ridx_sorted_disjoint", "aix_ridx_attach", "aix_positions_query",
       "aix_positions_query_dev", "aix_positions_locate", "aix_positions_locate_dev"]


def test_header_declares_and_lib_binds_the_entry_points():
    declared = _lib.header_symbols()
    L = _lib.lib()
    for name in NEW:
        assert name in declared, name
        res, args = _lib.SIGNATURES[name]
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == list(args) and len(args) >= 1, name
    assert len(_lib.SIGNATURES["aix_positions_query"][1]) == 8 and len(_lib.SIGNATURES["aix_positions_query_dev"][1]) == 11
    # every declaration names the reference lines it replaces
    text = open(_lib.HEADER).read()
    for name in NEW:
        at = text.index(f" {name}(")
        comment = text[text.rfind("/*", 0, at):at]
        assert re.search(r"(python_wrapper\.cpp|hash\.hpp):\d+", comment), name
    # the new fields sit at the end of aix_info_t, behind what was there
    names = [f for f, _ in _lib.Info._fields_]
    assert names[-4:] == ["aindex_attached", "ridx_on_device", "aindex_entries", "ridx_reads"] and names.index("reserved0") == len(names) - 5
    fields = re.findall(r"\b(\w+);", re.sub(r"/\*.*?\*/", "", text[text.index("typedef struct {"):text.index("} aix_info_t;")], flags=re.S))
    assert fields == names


def _sorted_disjoint(triples) -> bool:
    t = np.ascontiguousarray(triples, dtype=np.uint64).reshape(-1, 3)
    return bool(_lib.lib().aix_ridx_sorted_disjoint(t.ctypes.data_as(C.c_void_p) if t.shape[0] else None, t.shape[0]))


def test_ridx_sorted_disjoint_check(small23_prefix):
    n, p = C.c_uint64(), C.c_void_p()
    _lib.check(_lib.lib().aix_ridx_load((small23_prefix + ".ridx").encode(), C.byref(n), C.byref(p)))
    try:
        t = np.frombuffer(C.string_at(p, 24 * n.value), dtype=np.uint64).reshape(-1, 3).copy()
    finally:
        _lib.lib().aix_free(p)
    assert t.shape[0] > 100
    assert _sorted_disjoint(t) is True
    sh = t[np.random.default_rng(3).permutation(t.shape[0])]
    assert not np.array_equal(sh, t) and _sorted_disjoint(sh) is False
    assert _sorted_disjoint([[0, 0, 150], [1, 150, 300]]) is False            # overlapping pair: the second starts on the first's end
    assert _sorted_disjoint([[0, 0, 150], [1, 100, 300]]) is False
    assert _sorted_disjoint([[0, 0, 150], [1, 151, 301]]) is True
    assert _sorted_disjoint([[0, 10, 5]]) is False                            # end before start
    assert _sorted_disjoint(np.zeros((0, 3), np.uint64)) is True              # empty list
    # the same answer as the Python mirror's own flag
    w = AindexWrapper.__new__(AindexWrapper)
    w.load_reads_index(small23_prefix + ".ridx")
    assert w._ridx_sorted is True


def test_list_surface_places_empty_lists_for_wrong_length_items(gold):
    items = ["ACGTACGTACGTACGTACGTACG", "", "ACGTACGTACGTACGTACGTAC", b"TTTTTTTTTTTTTTTTTTTTTTT", "ACGTACGTACGTACGTACGTACGT", "ccccccccccccccccccccccc"]
    flat, keep = AindexWrapper._split_fixed(items, 23)
    assert keep.tolist() == [0, 3, 5] and flat == b"ACGTACGTACGTACGTACGTACG" + b"T" * 23 + b"c" * 23
    got = AindexWrapper._spread_lists(len(items), keep, np.array([0, 2, 2, 5], np.uint64), np.array([7, 9, 1, 2, 3], np.uint64))
    assert got == [[7, 9], [], [], [], [], [1, 2, 3]]
    flat, keep = AindexWrapper._split_fixed(["ACGT", "ACGTACGTACGTA"], 13)
    assert keep.tolist() == [1] and flat == b"ACGTACGTACGTA"
    flat, keep = AindexWrapper._split_fixed([], 23)
    assert keep.shape == (0,) and flat == b"" and AindexWrapper._spread_lists(0, keep, np.zeros(1, np.uint64), np.zeros(0, np.uint64)) == []
    # the committed reference answers meet the test-input condition of the GPU tests: at least a third of the k-mers have occurrences
    a = json.load(open(os.path.join(gold, "small23", "access.json")))
    assert len(a["kmers"]) == 180 and 3 * sum(1 for p in a["positions"] if p) >= len(a["kmers"])
