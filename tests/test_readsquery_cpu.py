"""Batch read retrieval, host side (no GPU): the ABI surface, the list surface's placing of wrong-length items, the host mirror of the
max_reads rule, and the golden answers of the compiled reference."""
import hashlib
import json
import os
import re

import numpy as np

from aindex_amd import _lib
from aindex_amd.wrapper import AindexWrapper

NEW = ["aix_reads_attach", "aix_reads_attach_dev", "aix_reads_detach", "aix_reads_info", "aix_reads_fetch", "aix_reads_fetch_dev", "aix_reads_fetch_rid",
       "aix_reads_fetch_rid_dev", "aix_reads_by_kmers", "aix_reads_by_kmers_dev"]


def test_header_declares_and_lib_binds_the_entry_points():
    declared = _lib.header_symbols()
    L = _lib.lib()
    for name in NEW:
        assert name in declared, name
        res, args = _lib.SIGNATURES[name]
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == list(args) and len(args) >= 1, name
    assert len(_lib.SIGNATURES["aix_reads_fetch"][1]) == 7 and len(_lib.SIGNATURES["aix_reads_fetch_dev"][1]) == 10
    assert len(_lib.SIGNATURES["aix_reads_by_kmers"][1]) == 8 and len(_lib.SIGNATURES["aix_reads_by_kmers_dev"][1]) == 12
    # every declaration names the reference lines it replaces
    text = open(_lib.HEADER).read()
    for name in NEW:
        at = text.index(f" {name}(")
        tail = text[at:text.index(";", at) + 200].split("\n")[0]
        comment = text[text.rfind("/*", 0, at):at] + tail
        assert re.search(r"python_wrapper\.cpp:\d+", comment), name
    # aix_info_t did not grow
    names = [f for f, _ in _lib.Info._fields_]
    assert names[-4:] == ["aindex_attached", "ridx_on_device", "aindex_entries", "ridx_reads"]
    # the public surface
    from aindex_amd.aindex import AIndex
    from aindex_amd.engine import Index
    for m in ("attach_reads", "attach_reads_t", "detach_reads", "fetch_reads", "fetch_reads_by_rid", "reads_by_kmers", "fetch_reads_t", "fetch_reads_by_rid_t",
              "reads_by_kmers_t"):
        assert callable(getattr(Index, m)), m
    for m in ("get_reads_batch", "get_reads_by_rid_batch", "get_reads_by_kmer_batch", "get_reads_array", "get_reads_by_kmers_array"):
        assert callable(getattr(AIndex, m)) and callable(getattr(AindexWrapper, m)), m


def test_list_surface_places_empty_lists_for_wrong_length_items():
    items = ["ACGTACGTACGTACGTACGTACG", "", "ACGTACGTACGTACGTACGTAC", b"TTTTTTTTTTTTTTTTTTTTTTT", "ACGTACGTACGTACGTACGTACGT"]
    flat, keep = AindexWrapper._split_fixed(items, 23)
    assert keep.tolist() == [0, 3]
    reads = AindexWrapper._csr_strings(np.array([0, 4, 4, 9], np.uint64), np.frombuffer(b"ACGTNN\xe9~t", dtype=np.uint8))
    assert reads == ["ACGT", "", "NN\xe9~t"]
    assert AindexWrapper._spread_lists(len(items), keep, np.array([0, 2, 3], np.uint64), reads) == [["ACGT", ""], [], [], ["NN\xe9~t"], []]
    w = AindexWrapper.__new__(AindexWrapper)
    w._is_13mer_mode, w.aindex_loaded = False, False
    assert w.get_reads_by_kmer_batch(items, 5) == [[], [], [], [], []]
    assert w.get_reads_by_kmer_batch([], 5) == []


def _host_wrapper(reads: bytes, triples, positions):
    """A wrapper over host arrays only: reads, intervals and a fixed k-mer -> positions map (no index, no device)."""
    w = AindexWrapper.__new__(AindexWrapper)
    w._is_13mer_mode, w.aindex_loaded, w._ix23, w._ix13 = False, True, None, None
    w._reads = np.frombuffer(reads, dtype=np.uint8)
    w.reads_size = len(reads)
    t = np.asarray(triples, dtype=np.uint64).reshape(-1, 3)
    w._ridx_rid, w._ridx_start, w._ridx_end = t[:, 0].copy(), t[:, 1].copy(), t[:, 2].copy()
    w.n_reads, w._ridx_sorted = t.shape[0], True
    w.get_positions = lambda kmer: positions.get(kmer, [])
    return w


def test_host_mirror_of_the_max_reads_rule():
    reads = b"AAAA\nCCCC\n\nGGGG\nTTTT"
    triples = [[0, 0, 4], [1, 5, 9], [2, 10, 10], [3, 11, 15], [4, 16, 20]]
    pos = {"k1": [6, 1, 7, 12, 2, 17], "k2": [10, 12], "k3": [400], "k4": []}
    w = _host_wrapper(reads, triples, pos)
    assert w.get_reads_se_by_kmer("k1", 100) == ["CCCC", "AAAA", "GGGG", "TTTT"]            # each read once, in order of first occurrence
    assert w.get_reads_se_by_kmer("k1", 2) == ["CCCC", "AAAA"] and w.get_reads_se_by_kmer("k1", 1) == ["CCCC"]
    assert w.get_reads_se_by_kmer("k1", 0) == ["CCCC"]                                     # the limit is tested after an append: 0 -> one read
    assert w.get_reads_se_by_kmer("k3", 0) == [] and w.get_reads_se_by_kmer("k4", 0) == []
    for m in (0, 1, 2, 3, 100, 10 ** 6):
        kmers = ["k1", "k2", "k3", "k4", "k1"]
        koff, rid, roff, data = w._reads_csr_host(kmers, m)
        flat = AindexWrapper._csr_strings(roff, data)
        assert [flat[int(koff[i]):int(koff[i + 1])] for i in range(len(kmers))] == [w.get_reads_se_by_kmer(s, m) for s in kmers]
        assert [w.get_read_by_rid(int(r)) for r in rid.tolist()] == flat
    # the host path of the batch surface (no device intervals) goes through the same loop
    assert w.get_reads_by_rid_batch([1, 0, 2, 9, 4]) == ["CCCC", "AAAA", "", "", "TTTT"]
    assert w.get_reads_batch([0, 5, 16, 16, 3], [4, 9, 19, 20, 2], [False, True, True, False, False]) == ["AAAA", "GGGG", "AAA", "", ""]


def _digest(strings) -> str:
    """tests/golden/make_golden_reads.py: digest()"""
    h = hashlib.sha256()
    for s in strings:
        b = s.encode("latin-1")
        h.update(len(b).to_bytes(8, "little") + b)
    return h.hexdigest()


def test_golden_files_are_well_formed(gold):
    total = 0
    n_bytes = 0
    for rel in (os.path.join("small23", "reads_access.json"), os.path.join("compute_reads", "reads_access.json")):
        path = os.path.join(gold, rel)
        n_bytes += os.path.getsize(path)
        for f in json.load(open(path))["files"]:
            data = open(os.path.join(gold, f["reads"]), "rb").read()
            size, n = f["size"], f["n_reads"]
            assert size == len(data) and os.path.exists(os.path.join(gold, f["reads"][: f["reads"].rfind(".")] + ".ridx"))
            # every rid: lengths and one digest over all answers (make_golden_reads.digest); every eighth answer and the out-of-range ones in full
            assert f["rids"] == list(range(n)) + [n, n + 1, 2 ** 40] and len(f["by_rid_len"]) == len(f["rids"]) and f["by_rid_len"][-3:] == [0, 0, 0]
            w = AindexWrapper.__new__(AindexWrapper)
            w._reads = None
            w.load_reads(os.path.join(gold, f["reads"]))
            host = [w.get_read_by_rid(r) for r in f["rids"]]                       # the existing host method reproduces the reference
            assert [len(x) for x in host] == f["by_rid_len"] and _digest(host) == f["by_rid_sha256"] and sum(f["by_rid_len"]) > 0
            assert len(f["by_rid_sample"]) >= n // 8 + 3 and all(host[f["rids"].index(int(r))] == x for r, x in f["by_rid_sample"].items())
            tr = f["triples"]
            assert len(tr) == len(f["get_read"]) and 3 * sum(1 for t in tr if t[2]) >= len(tr)
            assert any(a == b for a, b, _ in tr) and any(a > b for a, b, _ in tr) and any(b == size - 1 for _, b, _ in tr)
            assert any(b == size and a < size for a, b, _ in tr) and any(a >= size for a, _, _ in tr)
            assert any("\n" in s for s in f["get_read"]) and all(len(s) == (b - a if a < size and b < size and a <= b else 0) for (a, b, _), s in zip(tr, f["get_read"]))
            # the answers are what the rule of get_read (python_wrapper.cpp:677-698) gives on the committed file
            comp = bytes.maketrans(b"ACGT", b"TGCA")
            for (a, b, rc), s in zip(tr, f["get_read"]):
                want = data[a:b] if a < size and b < size and a <= b else b""
                assert s.encode("latin-1") == (want[::-1].translate(comp) if rc else want)
            total += len(tr)
            if f["reads"].startswith("small23"):
                assert data.count(b"N") == 120 and len(tr) >= 600 and sum(s.count("N") for s in f["get_read"]) >= 120
            else:
                assert any("~" in s for s in f["get_read"])
    assert total >= 600 and n_bytes < 300_000
