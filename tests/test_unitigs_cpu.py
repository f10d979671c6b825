"""The test-side restatement of the De Bruijn compaction (tests/unitigs_ref.py) pinned with literal answers, and its partition properties
on the fuzz graphs. No GPU: test_gpu_unitigs.py holds the kernels to this restatement."""
import numpy as np
import pytest

import graph_cases as G
import unitigs_cases as UC
import unitigs_ref as R

_E = {c: i for i, c in enumerate("ACGT")}


def _enc(s: str) -> int:
    x = 0
    for c in s:
        x = (x << 2) | _E[c]
    return x


def _rc(s: str) -> str:
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def _keys(seqs, tf=None):
    """(codes ascending, tfs): the canonical 23-mers of every window of `seqs`, tf 1 unless `tf` names the window"""
    table = {}
    for s in seqs:
        for i in range(len(s) - 22):
            table.setdefault(min(_enc(s[i:i + 23]), _enc(_rc(s[i:i + 23]))), 1)
    for w, t in (tf or {}).items():
        table[min(_enc(w), _enc(_rc(w)))] = t
    codes = np.array(sorted(table), dtype=np.uint64)
    return codes, np.array([table[int(c)] for c in codes], dtype=np.uint32)


def _answer(seqs, cutoff=0, tf=None):
    r = R.unitigs(*_keys(seqs, tf), cutoff)
    return list(zip(r["strings"], r["circular"].tolist(), r["tf_sum"].tolist())), r


def test_revcomp_and_spelling_helpers():
    s = "GATTACAGGCTTAACCGGATCTG"
    assert R.rc(_enc(s)) == _enc(_rc(s)) and R.rc(R.rc(_enc(s))) == _enc(s)
    assert R.spell([_enc(s), R.nxt(_enc(s), 1)]) == s + "C"
    assert R.prv(R.nxt(_enc(s), 1), _E["G"]) == _enc(s)           # back across the edge: the base that fell off the front


def test_one_kmer_and_short_paths():
    assert _answer(["GATTACAGGCTTAACCGGATCTG"])[0] == [("CAGATCCGGTTAAGCCTGTAATC", 0, 1)]          # the stored key = the smaller strand
    got, r = _answer(["TTGCAAGGCTTAACCGGATCTGAC"])
    assert got == [("GTCAGATCCGGTTAAGCCTTGCAA", 0, 2)]
    assert r["kid_pos"].tolist() == [0, 1] and r["kid_flag"].tolist() == [0, 0]
    got, r = _answer(["CCGATTGCAAGGCTTAACCGTATCT"])
    assert got == [("AGATACGGTTAAGCCTTGCAATCGG", 0, 3)]
    assert r["kid_unitig"].tolist() == [0, 0, 0] and r["kid_pos"].tolist() == [0, 2, 1] and r["kid_flag"].tolist() == [0, 0, 1]
    assert r["offsets"].tolist() == [0, 25] and r["kmer_tf"].tolist() == [1, 1, 1] and r["n_live"] == 3


def test_fork_and_join_cut_at_the_hub():
    stem, a1, a2 = "ACGGTCATTGCAGGCTAATCCGTAGGCA", "AGTTC", "CTGAG"
    want = [("ACGGTCATTGCAGGCTAATCCGTAGGCA", 0, 6), ("ATTGCAGGCTAATCCGTAGGCAAGTTC", 0, 5), ("ATTGCAGGCTAATCCGTAGGCACTGAG", 0, 5)]
    assert _answer([stem + a1, stem + a2])[0] == want               # the hub ends the stem; each arm starts behind it
    assert _answer([_rc(stem + a1), _rc(stem + a2)])[0] == want      # the same keys read as a join


def test_hairpin_and_homopolymer_are_linear():
    half = "ACGGTCATTGC"
    seq = "GGTCA" + "A" + half + _rc(half)                           # its last k-mer x has next(x, 'T') == rc x
    x = _enc(seq[-23:])
    assert R.nxt(x, _E["T"]) == R.rc(x)
    got, r = _answer([seq])
    assert got == [("ACGGTCATTGCGCAATGACCGTTTGACC", 0, 6)] and r["n_circular"] == 0
    got, r = _answer(["A" * 23])
    assert got == [("A" * 23, 0, 1)] and r["kid_flag"].tolist() == [0]


def test_circles_start_at_the_smallest_code_and_leave_through_r():
    got, r = _answer([("AC" * 20)[:24]])
    assert got == [("ACACACACACACACACACACACAC", 1, 2)] and r["kid_pos"].tolist() == [0, 1] and r["kid_flag"].tolist() == [2, 2]
    got, r = _answer([("ACG" * 20)[:25]])
    assert got == [("ACGACGACGACGACGACGACGACGA", 1, 3)] and r["kid_pos"].tolist() == [0, 1, 2]
    unit = "GATTCCAGTCATGGCATCAAGTCC"
    got, r = _answer([(unit * 3)[:46]])
    assert got == [("AAGTCCGATTCCAGTCATGGCATCAAGTCCGATTCCAGTCATGGCA", 1, 24)]
    assert sorted(r["kid_pos"].tolist()) == list(range(24)) and r["kid_pos"][0] == 0 and r["kid_flag"][0] == 2
    assert set(r["kid_flag"].tolist()) == {2, 3} and r["offsets"].tolist() == [0, 46]


def test_stored_zero_and_cutoff():
    p3 = "CCGATTGCAAGGCTTAACCGTATCT"
    got, r = _answer([p3], tf={p3[1:24]: 0})                         # the middle k-mer is stored with tf 0: dead at every cutoff
    assert got == [("AGATACGGTTAAGCCTTGCAATC", 0, 1), ("ATACGGTTAAGCCTTGCAATCGG", 0, 1)]
    assert r["kid_unitig"].tolist() == [0, 1, R.NONE] and r["kid_pos"].tolist() == [0, 0, 0] and r["kid_flag"].tolist() == [0, 0, 0]
    p5 = "TGCAAGGCTTAACCGGATCTGACCGTA"
    tf = {p5[i:i + 23]: 5 for i in range(5)}
    tf[p5[2:25]] = 2
    assert _answer([p5], 0, tf)[0] == [("TACGGTCAGATCCGGTTAAGCCTTGCA", 0, 22)]
    got, r = _answer([p5], 3, tf)                                    # tf 2 <= 3: the path falls apart around it
    assert got == [("AAGGCTTAACCGGATCTGACCGTA", 0, 10), ("GGTCAGATCCGGTTAAGCCTTGCA", 0, 10)]
    assert r["tf_min"].tolist() == [5, 5] and r["tf_max"].tolist() == [5, 5] and r["n_live"] == 4
    r = R.unitigs(*_keys([p5], tf), 5)                               # nothing is live
    assert r["U"] == 0 and r["offsets"].tolist() == [0] and r["bases"].shape == (0,)


@pytest.mark.parametrize("seed", [0, 3, 6, 9])
@pytest.mark.parametrize("cutoff", [0, 3])
def test_partition_properties_on_graph_cases(seed, cutoff):
    codes, tfs, _ = G.make_graph_case(seed)
    r = R.unitigs(codes, tfs, cutoff)
    live = tfs.astype(np.int64) > cutoff
    assert r["n_live"] == int(live.sum()) and ((r["kid_unitig"] != R.NONE) == live).all()
    m = np.diff(r["offsets"].astype(np.int64)) - 22
    assert m.sum() == r["n_live"] and (m >= 1).all()                 # the member counts sum to n_live
    text = r["bases"].tobytes().decode()
    off = r["offsets"].tolist()
    for kid in np.nonzero(live)[0].tolist():                         # every live key is in exactly one unitig at (pos, strand)
        u, pos = int(r["kid_unitig"][kid]), int(r["kid_pos"][kid])
        assert pos < m[u]
        word = text[off[u] + pos: off[u] + pos + 23]
        assert _enc(_rc(word) if r["kid_flag"][kid] & 1 else word) == int(codes[kid])
        assert bool(r["kid_flag"][kid] & 2) == bool(r["circular"][u])
    seen = np.zeros(int(m.sum()), bool)                              # no slot of a unitig is claimed twice
    at = (r["offsets"][:-1].astype(np.int64) - 22 * np.arange(r["U"]))[r["kid_unitig"][live].astype(np.int64)] + r["kid_pos"][live]
    seen[at] = True
    assert seen.all() and np.unique(at).shape[0] == at.shape[0]
    first = [_enc(text[off[u]: off[u] + 23]) for u in range(r["U"])]
    assert first == sorted(first) and len(set(first)) == len(first) and first == r["first"].tolist()   # ids ascend by first code
    assert 414 <= r["U"] <= 990 and 2 <= r["n_circular"] <= 4 and 65 <= int((m == 1).sum()) <= 439
    assert {24, 30} <= set(m[r["circular"] == 1].tolist())


def test_depth_case_has_the_prescribed_lengths():
    codes, tfs, paths, circles = UC.depth_case()
    r = R.unitigs(codes, tfs, 0)
    m = np.diff(r["offsets"].astype(np.int64)) - 22
    assert sorted(m[r["circular"] == 0].tolist()) == sorted(paths) and sorted(m[r["circular"] == 1].tolist()) == sorted(circles)
