"""Key sets for the unitig-graph tests (a helper, not a conftest): small canonical key sets with one planted structure each, built with the
_Keys of unitigs_cases.py.

  link_cases()   name -> Case(codes uint64[n] ascending, tfs uint32[n], cutoffs, pred). pred(ans) takes cutoff -> (un, lk), the answers of
                 unitigs_ref.unitigs and unitig_links_ref.links on (codes, tfs), and asserts that the structure is there.

A bubble is planted as L + mid + R for every arm: flanks of 40 bases (18 k-mers lie inside a flank: the source and the sink unitig) and
mids of 0 or 1 bases (an arm has 22 + len(mid) k-mers).

No case has an arm spelled against the other (the word x of the rule odd), because there is none to plant. Both arms leave the source
through P + a and P + b (P: its last 22 bases) and reach the sink through a' + Q and b' + Q. An arm is spelled from the source iff
P + a < rc(Q) + comp(a'): unless P == rc(Q) the 22 leading bases decide alike for both arms. With P == rc(Q) the sink's entering end
leaves through c + P and sees P + a and P + b as well as rc(a' + Q) and rc(b' + Q); in-degree 2 needs {a, b} == {comp a', comp b'}, and
then either an arm's first k-mer is the reverse complement of its own last one (a == comp a') or of the other arm's last one
(a == comp b'): the same stored key twice. So x is even in every simple bubble, which the bubble cases assert.
"""
import collections
import itertools

import numpy as np

import unitig_links_ref as RL
import unitigs_cases as UC
import unitigs_ref as R

Case = collections.namedtuple("Case", "codes tfs cutoffs pred")
NONE32 = RL.NONE32


def members(un) -> np.ndarray:
    return np.diff(un["offsets"].astype(np.int64)) - (R.K - 1)


def histogram(lk) -> list:
    return np.bincount(np.diff(lk["link_off"].astype(np.int64)), minlength=5).tolist()


def mate_pairs(lk) -> list:
    m = lk["bubble_mate"].tolist()
    return [(u, w) for u, w in enumerate(m) if w != NONE32 and u < w]


def arm_x(lk, u: int) -> int:
    """the word x through which the source end of arm u enters the other arm"""
    off, to = lk["link_off"].tolist(), lk["link_to"].tolist()
    f = to[off[2 * u + 1]] ^ 1
    return next(t for t in to[off[f]:off[f + 1]] if t != 2 * u)


def _answers(ks, cutoffs):
    codes, tfs = ks.arrays()
    ans = {}
    for c in cutoffs:
        un = R.unitigs(codes, tfs, c)
        ans[c] = (un, RL.links(codes, tfs, c, un))
    return codes, tfs, ans


def _plant(ks, left, mids, right, tf=5):
    """L + mid + R for every mid; the first in full, the others from 22 bases before the mid to 22 bases behind it"""
    for j, mid in enumerate(mids):
        t = tf[j] if isinstance(tf, (list, tuple)) else tf
        seq = (left if j == 0 else left[-22:]) + list(mid) + (right if j == 0 else right[:22])
        if ks.add(seq, tf=t) is None:
            return False
    return True


def _flanked(seed, mids_of, tf=5, extra=None):
    """a _Keys with one planted structure, redrawn (the next seed) until no k-mer collapses"""
    for s in itertools.count(seed):
        ks = UC._Keys(s)
        left, right = ks.base(40), ks.base(40)
        if _plant(ks, left, mids_of(left, right), right, tf) and (extra is None or extra(ks, left, right)):
            return ks


def _two_arm_case(seed, odd, mids_of, lengths, tf, cutoffs=(0,)):
    """a bubble of two arms, redrawn until the word x of the rule is odd (the arms are spelled in opposite directions) or even"""
    for s in itertools.count(seed, 100):
        ks = _flanked(s, mids_of, tf)
        codes, tfs, ans = _answers(ks, cutoffs)
        pairs = mate_pairs(ans[0][1])
        if len(pairs) == 1 and (arm_x(ans[0][1], pairs[0][0]) & 1) == odd:
            break

    def pred(a):
        un, lk = a[0]
        assert un["U"] == 4 and sorted(members(un).tolist()) == sorted([18, 18] + lengths) and lk["E"] == 8 and histogram(lk) == [2, 4, 2, 0, 0]
        (u, w), = mate_pairs(lk)
        assert sorted(members(un)[[u, w]].tolist()) == lengths and lk["bubble_mate"][u] == w and lk["bubble_mate"][w] == u
        assert (arm_x(lk, u) & 1) == odd and (arm_x(lk, w) & 1) == odd
        if 3 in a:                                                  # the weak arm is dead: one unitig, no link
            assert a[3][0]["U"] == 1 and a[3][1]["E"] == 0 and members(a[3][0]).tolist() == [18 + 18 + lengths[-1]]
    return Case(codes, tfs, cutoffs, pred)


def _indel_mids(left, right):
    b = next(b for b in range(4) if b != right[0] and b != left[-1])
    return [[b], []]


def _same_source_and_sink():
    """S + a + S[:22] and S[-22:] + b + S[:22]: both arms leave the right end of S and come back to its left end"""
    for s in itertools.count(301):
        ks = UC._Keys(s)
        stem = ks.base(40)
        if ks.add(stem + [0] + stem[:22]) is not None and ks.add(stem[-22:] + [1] + stem[:22]) is not None:
            break
    codes, tfs, ans = _answers(ks, (0,))

    def pred(a):
        un, lk = a[0]
        assert un["U"] == 3 and sorted(members(un).tolist()) == [18, 23, 23] and un["n_circular"] == 0 and lk["E"] == 8
        (u, w), = mate_pairs(lk)
        hub = 3 - u - w
        off, to = lk["link_off"].tolist(), lk["link_to"].tolist()
        assert {t >> 1 for t in to[off[2 * u]:off[2 * u + 2]]} == {hub} and histogram(lk) == [0, 4, 2, 0, 0]
    return Case(codes, tfs, (0,), pred)


def _near(seed, mids_of, extra, check):
    ks = _flanked(seed, mids_of, 5, extra)
    codes, tfs, _ = _answers(ks, ())

    def pred(a):
        un, lk = a[0]
        assert mate_pairs(lk) == [] and (lk["bubble_mate"] == NONE32).all()
        check(un, lk)
    return Case(codes, tfs, (0,), pred)


def _two_mids(left, right):
    return [[0], [1]]


def _three_arms():
    def check(un, lk):
        assert sorted(members(un).tolist()) == [18, 18, 23, 23, 23] and histogram(lk) == [2, 6, 0, 2, 0]
    return _near(311, lambda l, r: [[0], [1], [2]], None, check)


def _sink_in_degree_3():
    def extra(ks, left, right):
        z = ks.base(29) + [2]                                       # a third way into the sink: 30 k-mers that end in front of R
        return ks.add(z + right[:22]) is not None

    def check(un, lk):
        assert sorted(members(un).tolist()) == [18, 18, 23, 23, 30] and histogram(lk) == [3, 5, 1, 1, 0]
    return _near(321, _two_mids, extra, check)


def _different_sinks():
    """L + a + R1 and L + b + R2, and a second way into either sink, so that both sinks have in-degree 2"""
    for s in itertools.count(331):
        ks = UC._Keys(s)
        left, r1, r2 = ks.base(40), ks.base(40), ks.base(40)
        if all(ks.add(q) is not None for q in (left + [0] + r1, left[-22:] + [1] + r2, ks.base(29) + [2] + r1[:22], ks.base(29) + [2] + r2[:22])):
            break
    codes, tfs, _ = _answers(ks, ())

    def pred(a):
        un, lk = a[0]
        assert mate_pairs(lk) == [] and sorted(members(un).tolist()) == [18, 18, 18, 23, 23, 30, 30] and histogram(lk) == [5, 6, 3, 0, 0]
    return Case(codes, tfs, (0,), pred)


def _hairpin_arm():
    """one arm runs into a hairpin end (its only link is u+ -> u-), the other is a tip"""
    for s in itertools.count(341):
        ks = UC._Keys(s)
        left, half, a = ks.base(40), ks.base(11), ks.base(1)
        seq = left + [0] + ks.base(5) + a + half + UC._comp(half)
        if ks.add(seq) is None or ks.add(left[-22:] + [1] + ks.base(9)) is None:
            continue
        x = UC._codes_of(seq)[-1]
        assert R.nxt(x, 3 - a[0]) == R.rc(x)
        break
    codes, tfs, _ = _answers(ks, ())

    def pred(a):
        un, lk = a[0]
        assert mate_pairs(lk) == [] and sorted(members(un).tolist()) == [10, 18, 29]
        off, to = lk["link_off"].tolist(), lk["link_to"].tolist()
        assert sum(1 for e in range(2 * un["U"]) for t in to[off[e]:off[e + 1]] if t == e ^ 1) == 1   # the self-dual link of the hairpin
        u = int(np.argmax(members(un)))
        assert off[2 * u + 1] - off[2 * u] == 1 and off[2 * u + 2] - off[2 * u + 1] == 1                  # both degrees 1, and still no arm
    return Case(codes, tfs, (0,), pred)


def _third_attachment():
    """a bubble, and a third way that joins the first arm in front of its k-mer 10: that arm is two unitigs of 10 and 13 k-mers, and what
    is left looks like a bubble from both sides except for the other arm's link"""
    def extra(ks, left, right):
        arm = left[-22:] + [0] + right[:22]
        z = ks.base(29) + [next(b for b in range(4) if b != arm[9])]
        return ks.add(z + arm[10:32]) is not None

    def check(un, lk):
        assert sorted(members(un).tolist()) == [10, 13, 18, 18, 23, 30] and histogram(lk) == [3, 6, 3, 0, 0]
    return _near(351, _two_mids, extra, check)


def _degrees():
    """stems with 2, 3 and 4 continuations of 11 k-mers: ends of every degree 0 .. 4"""
    for s in itertools.count(361):
        ks = UC._Keys(s)
        ok = True
        for d in (2, 3, 4):
            stem = ks.base(40)
            for b in range(d):
                ok = ok and ks.add((stem if b == 0 else stem[-22:]) + [b] + ks.base(10)) is not None
        if ok:
            break
    codes, tfs, _ = _answers(ks, ())

    def pred(a):
        un, lk = a[0]
        assert sorted(members(un).tolist()) == [11] * 9 + [18] * 3 and histogram(lk) == [12, 9, 1, 1, 1] and lk["E"] == 18
        assert mate_pairs(lk) == []
    return Case(codes, tfs, (0,), pred)


def _tip_of_one():
    """a path of 38 k-mers and one k-mer that leaves it behind its k-mer 19: a unitig of one k-mer, which holds both of its ends"""
    for s in itertools.count(371):
        ks = UC._Keys(s)
        path = ks.base(60)
        if ks.add(path) is not None and ks.add(path[20:42] + [next(b for b in range(4) if b != path[42])], tf=2) is not None:
            break
    codes, tfs, _ = _answers(ks, ())

    def pred(a):
        un, lk = a[0]
        assert sorted(members(un).tolist()) == [1, 18, 20] and lk["E"] == 4 and histogram(lk) == [3, 2, 1, 0, 0] and (2 * un["U"]) % 16 != 0
        tip = int(np.argmin(members(un)))
        off = lk["link_off"].tolist()
        assert sorted([off[2 * tip + 1] - off[2 * tip], off[2 * tip + 2] - off[2 * tip + 1]]) == [0, 1]
        assert a[3][0]["U"] == 1 and a[3][1]["E"] == 0
    return Case(codes, tfs, (0, 3), pred)


def link_cases() -> dict:
    return {"bubble_snp": _two_arm_case(201, 0, _two_mids, [23, 23], [5, 2], (0, 3)),
            "bubble_indel": _two_arm_case(211, 0, _indel_mids, [22, 23], 5),
            "bubble_same_source_and_sink": _same_source_and_sink(),
            "near_three_arms": _three_arms(), "near_sink_in_degree_3": _sink_in_degree_3(), "near_different_sinks": _different_sinks(),
            "near_hairpin_arm": _hairpin_arm(), "near_third_attachment": _third_attachment(),
            "degrees_0_to_4": _degrees(), "tip_of_one": _tip_of_one()}
