"""Sequences against the indexed reads, host side (no GPU): the ABI surface, the plain-Python reference (tests/seqhits_ref.py) pinned
against hand-computed cases over tests/golden/small23, and the conditions that keep the GPU tests from passing on empty answers."""
import bisect
import json
import os
import re

import numpy as np
import pytest

import seqhits_ref as R
from aindex_amd import _lib

NEW = ["aix_seq_hits", "aix_seq_hits_dev", "aix_seq_votes", "aix_seq_votes_dev"]


@pytest.fixture(scope="module")
def ref(small23_prefix):
    return R.Ref(small23_prefix)


def test_header_declares_and_lib_binds_the_entry_points():
    declared = _lib.header_symbols()
    L = _lib.lib()
    text = open(_lib.HEADER).read()
    for name in NEW:
        assert name in declared, name
        res, args = _lib.SIGNATURES[name]
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
        at = text.index(f" {name}(")
        decl = text[text.rfind("/*", 0, at):text.index(";", at) + 80]
        assert re.search(r"python_wrapper\.cpp:\d+", decl), name     # every declaration names the reference lines it replaces
    assert [len(_lib.SIGNATURES[n][1]) for n in NEW] == [11, 14, 13, 16]


def test_codec_of_the_reference():
    w = b"ACGTACGTACGTACGTACGTACG"
    assert R.encode23(w) == int("00011011" * 5 + "000110", 2) and R.decode23(R.encode23(w)) == w
    assert R.rc_bytes(w) == b"CGTACGTACGTACGTACGTACGT"
    assert R.rc_bytes(b"acgtNACGTACGTACGTACGTAC") == b"GTACGTACGTACGTACGTTTTTT"      # bytes outside upper-case ACGT read as A


def test_the_positions_array_of_small23(ref):
    """All 20 821 non-zero entries are window starts inside one read without N; the array stops at 51 612 of 60 400 bytes."""
    pos = np.asarray(ref.positions, dtype=np.uint64)
    nz = (pos[pos != 0] - np.uint64(1)).tolist()
    assert len(nz) == 20821 and max(nz) == 51612 and len(ref.reads) == 60400
    for p in nz:
        i = bisect.bisect_right(ref.start, p) - 1              # the read that holds byte p (get_rid gives the read before it when p is a read's first byte)
        w = ref.reads[p:p + 23]
        assert ref.locate(p)[0] and ref.start[i] <= p and p + 23 <= ref.end[i] and set(w) <= set(b"ACGT")
        assert p in ref.get_positions(w) and ref.strand(w, p) == 0 and ref.strand(R.revcomp(w), p) == 1


def test_hand_computed_cases(ref, gold):
    # read 0 is the bytes [0, 150) of the file; its first window is stored at position 0 and nowhere else
    r0 = ref.reads[0:150]
    assert ref.reads[150:151] == b"\n" and (ref.rid[0], ref.start[0], ref.end[0]) == (0, 0, 150)
    first = ref.hits(r0[:23])
    assert (0, 0, 0, 0, 4) in first and all(h[0] == 0 for h in first)
    # a read against the index votes for itself on diagonal 0, forward; its reverse complement on diagonal 127 = 150 - 23, reverse
    v = {(r, s, d): (n, a, b) for r, s, d, n, a, b in ref.votes(r0)}
    assert v[(0, 0, 0)] == (107, 0, 127)
    vr = {(r, s, d): (n, a, b) for r, s, d, n, a, b in ref.votes(R.revcomp(r0))}
    assert vr[(0, 1, 127)] == (107, 0, 127)
    # window q of the reverse complement is window 127 - q of the read: the same positions, the other strand
    fw, rv = ref.hits(r0), ref.hits(R.revcomp(r0))
    assert sorted((127 - q, p, r, l, f ^ 1) for q, p, r, l, f in rv) == sorted(fw)
    # locate: the first interval with end + 1 >= pos wins, so a read's first byte still belongs to the read before it; far beyond the
    # file: nothing. The compiled reference's own answers (access.json) for 300-odd probes agree.
    assert ref.locate(150) == (True, 0, 0) and ref.locate(151) == (True, 0, 0) and ref.locate(152) == (True, 1, 151) and ref.locate(10 ** 9) == (False, 0, 0)
    a = json.load(open(os.path.join(gold, "small23", "access.json")))
    assert len(a["probes"]) > 300 and [ref.locate(p)[1:] for p in a["probes"]] == list(zip(a["rid"], a["start"]))
    assert [ref.get_positions(k.encode()) for k in a["kmers"]] == a["positions"] and sum(map(len, a["positions"])) == 930
    # lengths below 23 have no window; cut lists are prefixes; min_votes filters
    assert ref.hits(b"") == [] and ref.hits(r0[:22]) == [] and ref.votes(r0[:22]) == []
    per_w = {}
    for h in fw:
        per_w.setdefault(h[0], []).append(h)
    assert ref.hits(r0, 1) == [hs[0] for _, hs in sorted(per_w.items())]
    assert ref.votes(r0, 1000) == [] and all(x[3] >= 5 for x in ref.votes(r0, 5)) and len(ref.votes(r0, 5)) < len(ref.votes(r0, 1))
    # a dirty window: N reads as A for the code, the strand is told on the raw bytes, so a hit of it is strand 2
    w = bytearray(r0[40:63]); w[3] = ord("N")
    assert all(h[4] & 3 == 2 for h in ref.hits(bytes(w)))


def test_standard_queries_are_not_vacuous(ref, small23_prefix):
    qs = R.standard_queries(small23_prefix)
    assert len(qs) == 68 and [len(q) for q in qs[-8:]] == [300, 260, 150, 150, 0, 22, 23, 24]
    hits = [ref.hits(q) for q in qs]
    votes = [ref.votes(q) for q in qs]
    assert 3 * sum(1 for h in hits if h) >= len(qs)
    assert sum(1 for v in votes if any(x[3] >= 10 for x in v)) >= 20
    assert {x[1] for v in votes for x in v} == {0, 1}
    assert sum(1 for h in hits for x in h if x[4] & 3 == 2) > 0
    assert all(x[4] & 4 for h in hits for x in h)            # the clean index has no unlocated hit: test 3 plants them
