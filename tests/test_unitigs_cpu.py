"""The test-side restatement of the De Bruijn compaction (tests/unitigs_ref.py) pinned with literal answers, and its partition properties
on the fuzz graphs. No GPU: test_gpu_unitigs.py holds the kernels to this restatement."""
import numpy as np
import pytest

import graph_cases as G
import unitigs_cases as UC
import unitigs_check as KC
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


# ---------------------------------------------------------------------------------------------
# the planted topologies (unitigs_cases.topology_cases) and the checker that scales (unitigs_check.py)
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def topologies():
    """name -> (case, cutoff -> the restatement's answer), computed once"""
    return {name: (c, {cut: R.unitigs(c.codes, c.tfs, cut) for cut in UC.topology_cutoffs(name)}) for name, c in UC.topology_cases().items()}


def _shuffled(codes, tfs, seed):
    """the key set in another kid order: the MPHF's order is not the sorted one"""
    order = np.random.default_rng(seed).permutation(codes.shape[0])
    return codes[order], tfs[order]


def test_small_topologies_literally():
    half = "ACGGTCATTGC"
    got, r = _answer(["A" + half + _rc(half)])                       # a hairpin k-mer alone: its only successor is its own reverse complement
    assert got == [("AACGGTCATTGCGCAATGACCGT", 0, 1)] and r["n_circular"] == 0 and r["kid_flag"].tolist() == [0]
    got, r = _answer(["CA" + half + _rc(half)])
    assert got == [("ACGGTCATTGCGCAATGACCGTTG", 0, 2)] and r["n_circular"] == 0 and r["kid_pos"].tolist() == [0, 1] and r["kid_flag"].tolist() == [1, 1]
    a, c = "A" * 22, "C" * 22                                        # A^23 is its own successor besides A^22 C: nothing merges
    assert _answer([a + "A", a + "C", "T" + a])[0] == [(a + "A", 0, 1), (a + "C", 0, 1), ("T" + a, 0, 1)]
    assert _answer([c + "C", c + "A", "G" + c])[0] == [(c + "A", 0, 1), (c + "C", 0, 1), ("G" + c, 0, 1)]
    assert _answer(["T" * 23, "T" * 22 + "A", "G" + "T" * 22])[0] == _answer([a + "A", a + "C", "T" + a])[0]     # the same keys
    s = ("GATTCCAGTCATGGCATCAAGTCC" * 3)[:46]                        # the circle of 24 with one weak member
    tf = {s[i:i + 23]: 5 for i in range(24)}
    tf[s[5:28]] = 2
    got, r = _answer([s], 0, tf)
    assert got == [("AAGTCCGATTCCAGTCATGGCATCAAGTCCGATTCCAGTCATGGCA", 1, 117)] and r["n_circular"] == 1
    got, r = _answer([s], 3, tf)                                     # opened behind the weak member, spelled from the smaller end
    assert got == [("AGTCATGGCATCAAGTCCGATTCCAGTCATGGCATCAAGTCCGAT", 0, 115)] and r["n_circular"] == 0
    assert sorted(r["kid_pos"].tolist()) == [0] + list(range(23)) and set(r["kid_flag"].tolist()) == {0, 1}


def test_topology_predicates_hold(topologies):
    assert len(topologies) >= 9
    for name, (case, ans) in topologies.items():
        codes = case.codes.tolist()
        assert codes == sorted(set(codes)) and all(c == R.canon(c) for c in codes[:: max(1, len(codes) // 500)]), name
        case.pred(ans)
    assert topologies["isolated_one"][1][0]["strings"] == [R.spell([int(topologies["isolated_one"][0].codes[0])])]
    many = topologies["many_circles"][0]
    assert (2 * many.codes.shape[0]) % 16 != 0                       # the GPU tests want a port count that is no multiple of 16


@pytest.mark.parametrize("cutoff", [0, 3])
def test_check_accepts_the_restatement(topologies, cutoff):
    for seed in (0, 3, 6, 9):
        codes, tfs = _shuffled(*G.make_graph_case(seed)[:2], seed)
        KC.check(codes, tfs, cutoff, R.unitigs(codes, tfs, cutoff))
    for i, (name, (case, ans)) in enumerate(topologies.items()):
        KC.check(case.codes, case.tfs, cutoff, ans[cutoff])
        codes, tfs = _shuffled(case.codes, case.tfs, 100 + i)
        KC.check(codes, tfs, cutoff, R.unitigs(codes, tfs, cutoff))
    heavy, ans = topologies["heavy"]
    KC.check(heavy.codes, heavy.tfs, UC.HEAVY_CUTOFF, ans[UC.HEAVY_CUTOFF])
    KC.check(heavy.codes, heavy.tfs, 0xFFFFFFFF, R.unitigs(heavy.codes, heavy.tfs, 0xFFFFFFFF))        # nothing is live


def _respell(codes, tfs, r, ku, kp, kf):
    """the answer that belongs to per-kid arrays: unitigs in id order, members in position order, whatever they claim"""
    live = np.nonzero(ku != np.uint64(R.NONE))[0]
    U = int(ku[live].max()) + 1
    members = [[] for _ in range(U)]
    for kid in live.tolist():
        members[int(ku[kid])].append((int(kp[kid]), kid))
    out = dict(r, U=U, kid_unitig=ku, kid_pos=kp, kid_flag=kf, offsets=np.zeros(U + 1, np.uint64), circular=np.zeros(U, np.uint8),
               tf_sum=np.zeros(U, np.uint64), tf_min=np.zeros(U, np.uint32), tf_max=np.zeros(U, np.uint32))
    text, seq, at = [], [], 0
    for u, ms in enumerate(members):
        kids = [kid for _, kid in sorted(ms)]
        t = [int(tfs[kid]) for kid in kids]
        text.append(R.spell([R.rc(int(codes[kid])) if kf[kid] & 1 else int(codes[kid]) for kid in kids]))
        out["offsets"][u], out["circular"][u] = at, (kf[kids[0]] >> 1) & 1
        out["tf_sum"][u], out["tf_min"][u], out["tf_max"][u] = sum(t), min(t), max(t)
        seq += t
        at += len(kids) + 22
    out["offsets"][U] = at
    out["bases"] = np.frombuffer("".join(text).encode(), dtype=np.uint8).copy()
    out["kmer_tf"] = np.array(seq, dtype=np.uint32)
    out["n_circular"] = int(out["circular"].sum())
    return out


def _mutants(codes, tfs, r):
    """name -> a wrong answer, each wrong in one way. The first seven change the per-kid arrays and respell everything from them, so
    that the answer is consistent with itself and only the rule in question is broken."""
    m = np.diff(r["offsets"].astype(np.int64)) - 22
    ku, kp, kf = r["kid_unitig"], r["kid_pos"], r["kid_flag"]
    of = lambda u: np.nonzero(ku == np.uint64(u))[0]
    path = int(np.nonzero((r["circular"] == 0) & (m >= 4))[0][0])
    ring = int(np.nonzero((r["circular"] == 1) & (m >= 3))[0][0])
    out = {}

    def per_kid(name, change):
        a, b, c = ku.copy(), kp.copy(), kf.copy()
        change(a, b, c)
        out[name] = _respell(codes, tfs, r, a, b, c)

    def reverse(a, b, c):
        b[of(path)] = m[path] - 1 - b[of(path)]
        c[of(path)] ^= 1
    per_kid("a path spelled from the other end", reverse)

    def rotate(a, b, c):
        b[of(ring)] = (b[of(ring)] + 1) % m[ring]
    per_kid("a circle rotated by one", rotate)

    def turn(a, b, c):
        b[of(ring)] = (m[ring] - b[of(ring)]) % m[ring]
        c[of(ring)] ^= 1
    per_kid("a circle run in the other direction from the right start", turn)

    def swap(a, b, c):
        a[of(path)], a[of(ring)] = ring, path
    per_kid("two ids swapped", swap)

    def split(a, b, c):                                              # the second half becomes the unitig behind `path`
        a[(a != np.uint64(R.NONE)) & (a > np.uint64(path))] += np.uint64(1)
        back = of(path)[kp[of(path)] >= 2]
        a[back], b[back] = path + 1, kp[back] - 2
    per_kid("a unitig split at an interior link", split)

    def edit(name, change):
        o = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in r.items()}
        change(o)
        out[name] = o

    def pos(o):
        o["kid_pos"][of(path)[0]] += 1 if kp[of(path)[0]] + 1 < m[path] else -1
    edit("one kid_pos off by one", pos)

    def flag(o):
        o["kid_flag"][of(path)[1]] ^= 1
    edit("one strand flag flipped", flag)

    def shift(o):
        o["offsets"][1:-1] += 1
    edit("offsets shifted by one", shift)

    def base(o):
        at = int(r["offsets"][path]) + 30 % (m[path] + 22)
        o["bases"][at] = ord("ACGT"[("ACGT".index(chr(o["bases"][at])) + 1) % 4])
    edit("one base of bases changed", base)

    def ncirc(o):
        o["n_circular"] += 1
    edit("n_circular off by one", ncirc)
    dead = np.nonzero(ku == np.uint64(R.NONE))[0]
    if dead.shape[0]:
        def raise_dead(o):
            o["kid_unitig"][dead[0]] = 0
        edit("a dead kid given an id", raise_dead)
    spread = np.nonzero(r["tf_min"] != r["tf_max"])[0]
    if spread.shape[0]:
        def minmax(o):
            o["tf_min"], o["tf_max"] = r["tf_max"].copy(), r["tf_min"].copy()
        edit("tf_min and tf_max exchanged", minmax)

        def two_tf(o):
            u = int(spread[0])
            j = int(r["offsets"][u]) - 22 * u
            t = r["kmer_tf"][j: j + m[u]]
            a, b = int(t.argmin()), int(t.argmax())
            o["kmer_tf"][j + a], o["kmer_tf"][j + b] = t[b], t[a]
        edit("two entries of kmer_tf exchanged inside a unitig", two_tf)
    return out


STRUCTURAL = ("a path spelled from the other end", "a circle rotated by one", "a circle run in the other direction from the right start", "two ids swapped",
              "a unitig split at an interior link", "one kid_pos off by one", "one strand flag flipped", "offsets shifted by one", "one base of bases changed",
              "n_circular off by one")
WITH_TF = ("a dead kid given an id", "tf_min and tf_max exchanged", "two entries of kmer_tf exchanged inside a unitig")


@pytest.fixture(scope="module")
def mutants():
    """base -> (codes, tfs, cutoff, name -> wrong answer): the depth case (every tf 1: no dead kid, no spread), graph case 3 at cutoff 3"""
    codes, tfs = UC.depth_case()[:2]
    d = _shuffled(codes, tfs, 1)
    g = _shuffled(*G.make_graph_case(3)[:2], 2)
    out = {}
    for base, (c, t), cutoff in (("depth", d, 0), ("graph", g, 3)):
        r = R.unitigs(c, t, cutoff)
        KC.check(c, t, cutoff, r)
        out[base] = (c, t, cutoff, _mutants(c, t, r))
    assert set(out["depth"][3]) == set(STRUCTURAL) and set(out["graph"][3]) == set(STRUCTURAL + WITH_TF)
    return out


@pytest.mark.parametrize("name", STRUCTURAL + WITH_TF)
@pytest.mark.parametrize("base", ["depth", "graph"])
def test_check_rejects_the_mutant(mutants, base, name):
    codes, tfs, cutoff, wrong = mutants[base]
    if name not in wrong:
        assert base == "depth" and name in WITH_TF                   # every tf of the depth case is 1
        return
    with pytest.raises(AssertionError):
        KC.check(codes, tfs, cutoff, wrong[name])


def test_links_are_symmetric_and_cut_self_loops(topologies):
    """links() against its own definition on the cases that were built for it: p <-> t both ways, never within a node; the hairpin ends
    and the homopolymers have no link on the side that meets themselves."""
    for name in ("hairpin_ends", "selfloop", "lollipop", "many_circles"):
        case = topologies[name][0]
        link = KC.links(case.codes, case.tfs, 0)
        p = np.nonzero(link >= 0)[0]
        assert p.shape[0] and np.array_equal(link[link[p]], p) and ((link[p] >> 1) != (p >> 1)).all(), name
    case = topologies["selfloop"][0]
    link = KC.links(case.codes, case.tfs, 0)
    assert case.codes[0] == 0 and link[0] == -1 and link[1] == -1    # A^23: out-degree 2 on either side
