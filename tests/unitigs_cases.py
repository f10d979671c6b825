"""Key sets for the compaction tests (a helper, not a conftest).

  depth_case()   (codes uint64[n] ascending, tfs uint32[n] all 1, paths, circles): one canonical key set of ~33 000 keys whose unitigs are
                 linear paths of exactly PATHS k-mers and circles of exactly CIRCLES k-mers — the lengths around 2^r at which list ranking
                 can go wrong (a missed round, a cycle of 2^r nodes taken for a finished path, cycle start and direction), and one path
                 deep enough to need 16 rounds.
  topology_cases()  name -> Case(codes uint64[n] ascending, tfs uint32[n], pred): small canonical key sets with one planted structure
                 each, the ones the link rule exists for (the list is above the function). pred(answer) takes cutoff -> the restatement's
                 answer on (codes, tfs) for cutoffs 0 and 3 (`heavy`: 0xFFFFFFFE as well) and asserts that the structure is there.
"""
import collections
import itertools

import numpy as np

import unitigs_ref as R

PATHS = (1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 20001)
CIRCLES = (2, 3, 24, 64, 1000, 4096, 4097)


def _codes_of(seq) -> list:
    """the oriented 23-mer codes of every window of a sequence of values 0..3"""
    x, out = 0, []
    for i, b in enumerate(seq):
        x = ((x << 2) | int(b)) & R.MASK
        if i >= R.K - 1:
            out.append(x)
    return out


def depth_case(seed: int = 20250):
    rng = np.random.default_rng(seed)
    taken = set()

    def draw(m: int, circle: bool):
        while True:                                                # redraw a unit that collapses (a shorter period, a k-mer met before)
            if circle:
                unit = rng.integers(0, 4, m)
                seq = np.tile(unit, (m + R.K - 1) // m + 1)[: m + R.K - 1]
            else:
                seq = rng.integers(0, 4, m + R.K - 1)
            keys = {R.canon(x) for x in _codes_of(seq.tolist())}
            if len(keys) == m and not (keys & taken):
                taken.update(keys)
                return

    for m in PATHS:
        draw(m, False)
    for m in CIRCLES:
        draw(m, True)
    codes = np.array(sorted(taken), dtype=np.uint64)
    return codes, np.ones(codes.shape[0], np.uint32), PATHS, CIRCLES


Case = collections.namedtuple("Case", "codes tfs pred")
TOPOLOGY_CUTOFFS = (0, 3)
HEAVY_CUTOFF = 0xFFFFFFFE
HAIRPIN_PATHS = (1, 2, 5, 40)
LOLLIPOPS = (7, 64, 1000)
OPENED = (24, 4096)
SMALL_CIRCLES = {5: 100, 6: 120, 7: 120, 8: 120, 9: 120}           # of 2, 3 and 4 k-mers: every circle there is (2 + 10 + 27)
LONG_PATH = 5000


def _comp(seq) -> list:
    return [3 - b for b in reversed(seq)]


def _members(r) -> np.ndarray:
    return np.diff(r["offsets"].astype(np.int64)) - (R.K - 1)


class _Keys:
    """canonical code -> tf of one case. add() takes a sequence whose windows are all new and all different as canonical keys, or refuses."""

    def __init__(self, seed: int):
        self.rng = np.random.default_rng(seed)
        self.table = {}

    def base(self, n: int) -> list:
        return self.rng.integers(0, 4, int(n)).tolist()

    def add(self, seq, tf=5):
        """the canonical codes of the windows of `seq`, in order; None when one of them is met twice. tf: one value, or one per window."""
        keys = [R.canon(x) for x in _codes_of(seq)]
        if len(set(keys)) != len(keys) or any(k in self.table for k in keys):
            return None
        for j, k in enumerate(keys):
            self.table[k] = tf[j] if isinstance(tf, (list, tuple)) else tf
        return keys

    def draw(self, make, tf=5):
        while True:                                                # redraw until nothing collapses and nothing is shared
            seq = make()
            keys = self.add(seq, tf)
            if keys is not None:
                return seq, keys

    def circle(self, m: int, tf=5):
        return self.draw(lambda: (lambda unit: (unit * (R.K // m + 2))[: m + R.K - 1])(self.base(m)), tf)

    def arrays(self):
        codes = np.array(sorted(self.table), dtype=np.uint64)
        return codes, np.array([self.table[int(c)] for c in codes], dtype=np.uint32)


def _unitig_of(codes, r, keys) -> np.ndarray:
    return r["kid_unitig"][np.searchsorted(codes, np.array(keys, dtype=np.uint64))]


def _hairpin_ends():
    """Paths whose end k-mer x = a + h + rc(h) has next(x, comp a) == rc x: x is its own only successor, which is no link. At the right
    end, at the left end (the sequence reversed and complemented before it is windowed: other k-mers, since they are drawn anew), at
    both ends, and one whose x has a second successor with tf 2: an arm of 3 k-mers that a cutoff of 3 kills."""
    ks = _Keys(101)

    def right(m):
        half, a = ks.base(11), ks.base(1)
        seq = ks.base(m - 1) + a + half + _comp(half)
        x = _codes_of(seq)[-1]
        assert R.nxt(x, 3 - a[0]) == R.rc(x)
        return seq

    want = []
    for m in HAIRPIN_PATHS:
        ks.draw(lambda: right(m))
        ks.draw(lambda: _comp(right(m)))
        want += [m, m]
    for m in (24, 40):                                             # both ends: g + rc(g) + c ... a + h + rc(h)
        ks.draw(lambda: (lambda g, h: g + _comp(g) + ks.base(1) + ks.base(m - 24) + ks.base(1) + h + _comp(h))(ks.base(11), ks.base(11)))
        want.append(m)
    seq, _ = ks.draw(lambda: right(5))
    b = next(b for b in range(4) if b != 3 - seq[-23])             # another base than the one that closes the hairpin
    ks.draw(lambda: seq[-22:] + [b] + ks.base(2), tf=2)
    codes, tfs = ks.arrays()

    def pred(ans):
        assert ans[0]["n_circular"] == 0 and ans[3]["n_circular"] == 0
        assert sorted(_members(ans[0]).tolist()) == sorted(want + [5, 3]) and not ans[0]["circular"].any()
        assert sorted(_members(ans[3]).tolist()) == sorted(want + [5]) and ans[3]["n_live"] == codes.shape[0] - 3
    return Case(codes, tfs, pred)


def _selfloop():
    """c * 23 with c * 22 + d and e + c * 22 for every base c, as canonical keys: A * 23 and C * 23 with two neighbours each (d and e
    are chosen so that T and G give the keys of A and C again). The homopolymer is its own successor: out-degree 2, counting itself.
    Each neighbour ends a tail of 11 k-mers."""
    ks = _Keys(102)
    homo = []
    for c, d, e in ((0, 1, 3), (3, 0, 2), (1, 0, 2), (2, 1, 3)):
        for seq in ([c] * 23, [c] * 22 + [d], [e] + [c] * 22):
            for x in _codes_of(seq):
                ks.table[R.canon(x)] = 5
        homo.append(R.canon(_codes_of([c] * 23)[0]))
    assert len(ks.table) == 6 and sorted(set(homo)) == [0, _codes_of([1] * 23)[0]]
    ks.draw(lambda: ks.base(10) + [3] + [0] * 21)                   # ... T A^21, the next window is T A^22
    ks.draw(lambda: [0] * 21 + [1] + ks.base(10))                   # A^21 C ..., the window before is A^22 C
    ks.draw(lambda: ks.base(10) + [2] + [1] * 21)
    ks.draw(lambda: [1] * 21 + [0] + ks.base(10))
    codes, tfs = ks.arrays()

    def pred(ans):
        for c in TOPOLOGY_CUTOFFS:
            r = ans[c]
            m = _members(r)
            assert sorted(m.tolist()) == [1, 1, 11, 11, 11, 11] and r["n_circular"] == 0
            for u in _unitig_of(codes, r, sorted(set(homo))).tolist():
                assert m[u] == 1
            assert not r["kid_flag"][np.searchsorted(codes, np.array(sorted(set(homo)), dtype=np.uint64))].any()
    return Case(codes, tfs, pred)


def _lollipop():
    """A stem of 30 k-mers that runs into a circle of m: stem + the unit repeated + 22 more bases. The circle's first k-mer has
    in-degree 2, so the circle is ONE LINEAR unitig of m k-mers that starts there, and the stem stops in front of it."""
    ks = _Keys(103)
    rings = []
    for m in LOLLIPOPS:
        _, keys = ks.draw(lambda: (lambda unit: ks.base(30) + (unit * (R.K // m + 2))[: m + R.K - 1])(ks.base(m)))
        rings.append(keys[30:])
    codes, tfs = ks.arrays()

    def pred(ans):
        for c in TOPOLOGY_CUTOFFS:
            r = ans[c]
            m = _members(r)
            assert r["n_circular"] == 0 and sorted(m.tolist()) == sorted([30] * len(LOLLIPOPS) + list(LOLLIPOPS))
            for keys in rings:
                u = np.unique(_unitig_of(codes, r, keys))
                assert u.shape[0] == 1 and m[int(u[0])] == len(keys)
    return Case(codes, tfs, pred)


def _bubble_tip_cutoff():
    """L + v + R with v = two different bases: a bubble of two arms of 23 k-mers, one with tf 5 and one with tf 2; a tip of 4 k-mers with
    tf 3 leaves R after its 20th window (18 + 23 + 20 + 18 = 79 k-mers on the strong way). At cutoff 0 the hubs cut: six unitigs. At cutoff 3 the weak arm and the tip are dead and one
    unitig spans everything else."""
    ks = _Keys(104)
    left, right = ks.base(40), ks.base(60)
    strong, _ = ks.draw(lambda: left + [ks.rng.integers(0, 4)] + right)
    v = next(b for b in range(4) if b != strong[40])
    assert ks.add(left[-22:] + [v] + right[:22], tf=2) is not None
    b = next(b for b in range(4) if b != right[42])
    ks.draw(lambda: right[20:42] + [b] + ks.base(3), tf=3)
    codes, tfs = ks.arrays()

    def pred(ans):
        m0, m3 = _members(ans[0]), _members(ans[3])
        assert ans[3]["U"] < ans[0]["U"] and m3.max() > m0.max()
        assert sorted(m0.tolist()) == [4, 18, 18, 20, 23, 23] and m3.tolist() == [79]
    return Case(codes, tfs, pred)


def _opened_circle():
    """Circles with one member at tf 2 and the rest at tf 5: circular at cutoff 0, one linear unitig of m - 1 k-mers at cutoff 3."""
    ks = _Keys(105)
    for m in OPENED:
        ks.circle(m, tf=[5] * 5 + [2] + [5] * (m - 6))
    codes, tfs = ks.arrays()

    def pred(ans):
        assert ans[0]["n_circular"] == len(OPENED) and sorted(_members(ans[0]).tolist()) == sorted(OPENED)
        assert ans[3]["n_circular"] == 0 and sorted(_members(ans[3]).tolist()) == sorted(m - 1 for m in OPENED)
    return Case(codes, tfs, pred)


def _many_circles():
    """Hundreds of disjoint circles of 2 .. 9 k-mers beside one path of 5000: the ranking goes on for 13 rounds while every circle's
    ports stay open, and the cycle phase meets lengths that do and do not divide 2^r. Of 2, 3 and 4 k-mers there are only 2, 10 and 27
    circles whose k-mers are all different as canonical keys (a unit and its reverse complement spell the same circle): all of them are
    here; SMALL_CIRCLES of the other lengths. Every second circle has tf 2 and is gone at cutoff 3."""
    ks = _Keys(106)
    lengths = []
    for m in (2, 3, 4):
        for unit in itertools.product(range(4), repeat=m):
            if ks.add((list(unit) * (R.K // m + 2))[: m + R.K - 1], tf=(5, 2)[len(lengths) % 2]) is not None:
                lengths.append(m)
    assert [lengths.count(m) for m in (2, 3, 4)] == [2, 10, 27]
    for m, count in SMALL_CIRCLES.items():
        for _ in range(count):
            ks.circle(m, tf=(5, 2)[len(lengths) % 2])
            lengths.append(m)
    ks.draw(lambda: ks.base(LONG_PATH + R.K - 1))
    codes, tfs = ks.arrays()
    assert len(lengths) >= 600

    def pred(ans):
        for c, kept in ((0, lengths), (3, lengths[0::2])):
            r = ans[c]
            m = _members(r)
            assert r["n_circular"] == len(kept) and r["U"] == len(kept) + 1
            assert sorted(m[r["circular"] == 1].tolist()) == sorted(kept) and m[r["circular"] == 0].tolist() == [LONG_PATH]
    return Case(codes, tfs, pred)


def _isolated(count: int):
    """Random canonical keys, none a neighbour of another: every unitig is one k-mer, spelled as stored."""
    ks = _Keys(107 + count)
    for _ in range(count):
        ks.draw(lambda: ks.base(R.K), tf=int(ks.rng.integers(1, 7)))
    codes, tfs = ks.arrays()

    def pred(ans):
        for c in TOPOLOGY_CUTOFFS:
            r = ans[c]
            assert r["U"] == r["n_live"] == int((tfs > c).sum()) and (_members(r) == 1).all() and not r["kid_flag"].any()
            assert r["bases"].shape[0] == R.K * r["U"]
        assert ans[0]["U"] == count and (count == 1 or 0 < ans[3]["U"] < count)
    return Case(codes, tfs, pred)


def _heavy():
    """A path of 6 k-mers with tf 0xFFFFFFFF beside one with tf 1: tf_sum is above 2^34; at cutoff 0xFFFFFFFE only the heavy path lives."""
    ks = _Keys(108)
    ks.draw(lambda: ks.base(6 + R.K - 1), tf=0xFFFFFFFF)
    ks.draw(lambda: ks.base(6 + R.K - 1), tf=1)
    codes, tfs = ks.arrays()

    def pred(ans):
        assert sorted(ans[0]["tf_sum"].tolist()) == [6, 6 * 0xFFFFFFFF] and 6 * 0xFFFFFFFF > 1 << 34
        for c in (3, HEAVY_CUTOFF):
            r = ans[c]
            assert r["U"] == 1 and r["n_live"] == 6 and r["tf_sum"].tolist() == [6 * 0xFFFFFFFF]
            assert r["tf_min"].tolist() == [0xFFFFFFFF] and r["tf_max"].tolist() == [0xFFFFFFFF]
    return Case(codes, tfs, pred)


def topology_cases() -> dict:
    return {"hairpin_ends": _hairpin_ends(), "selfloop": _selfloop(), "lollipop": _lollipop(), "bubble_tip_cutoff": _bubble_tip_cutoff(),
            "opened_circle": _opened_circle(), "many_circles": _many_circles(), "isolated": _isolated(5000), "isolated_one": _isolated(1),
            "heavy": _heavy()}


def topology_cutoffs(name: str) -> tuple:
    return TOPOLOGY_CUTOFFS + ((HEAVY_CUTOFF,) if name == "heavy" else ())
