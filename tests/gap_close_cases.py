"""Inputs for the gap-closing tests (a helper, not a conftest): hand-made contig graphs with joins.

  case(name)        (graph, params, want): one motif with its join of interest at graph["probe"] (the owner end) and the literal answer
                    want = (status, states, dist, path) under params = dict(tolerance, max_fill, max_states). NAMES lists them.
  make_batch(seed, J)
                    J joins in random id order and orientation over random mixtures of the motifs; all four statuses occur under PARAMS.

Every contig is X + random bases + X with one 22-mer X that is its own reverse complement, so the 22 bases that two linked contigs
share are equal whatever the orientations: the bases are consistent over every overlap. A graph is a dict U, offsets, bases, link_off,
link_to, E, join, join_count, join_gap (numpy, the dtypes of the library)."""
import numpy as np

NONE32 = 0xFFFFFFFF
_HALF = "ACCGTTAGCAT"
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
X = _HALF + "".join(_COMP[c] for c in reversed(_HALF))                     # 22 bases, X == rc(X)
PARAMS = dict(tolerance=10, max_fill=16, max_states=256)                   # make_batch: b = 7 bubbles exhaust 256 states, b = 6 do not


class Builder:
    """contigs, links and joins in logical words (node, orientation); build() maps them to ids in the order `order` (None: as made, or
    a random permutation with shuffle=True) and flips every contig at random with shuffle=True"""

    def __init__(self, seed: int, shuffle: bool = False, dual: bool = True):
        self.rng = np.random.default_rng(70_000 + seed)
        self.shuffle, self.dual, self.lens, self.links, self.joins, self.order = shuffle, dual, [], [], [], None

    def node(self, length: int) -> int:
        assert length >= 44
        self.lens.append(length)
        return len(self.lens) - 1

    def link(self, a, b):
        """a -> b and, in a dual-closed graph, b ^ 1 -> a ^ 1"""
        self.links.append((a, b))
        if self.dual:
            self.links.append(((b[0], b[1] ^ 1), (a[0], a[1] ^ 1)))

    def join(self, e, t, gap: int):
        self.joins.append((e, t, gap))

    def path(self, *words):
        for a, b in zip(words, words[1:]):
            self.link(a, b)

    def build(self) -> dict:
        U, rng = len(self.lens), self.rng
        perm = list(range(U)) if self.order is None else list(self.order)
        flip = [0] * U
        if self.shuffle:
            perm, flip = rng.permutation(U).tolist(), rng.integers(0, 2, U).tolist()
        word = lambda w: 2 * perm[w[0]] + (w[1] ^ flip[w[0]])
        self.word = word
        lens = [0] * U
        for n, ln in enumerate(self.lens):
            lens[perm[n]] = ln
        ends = [set() for _ in range(2 * U)]
        for a, b in self.links:
            ends[word(a)].add(word(b))
        order = [sorted(l) if not self.shuffle else rng.permutation(sorted(l)).tolist() for l in ends]
        join, gap = np.full(2 * U, NONE32, np.uint32), np.zeros(2 * U, np.int64)
        for e, t, g in self.joins:
            e, t = word(e), word(t)
            assert join[e] == NONE32 and join[t ^ 1] == NONE32
            join[e], join[t ^ 1], gap[e], gap[t ^ 1] = t, e ^ 1, g, g
        letters = np.frombuffer(b"ACGT", np.uint8)
        text = b"".join(X.encode() + letters[rng.integers(0, 4, ln - 44)].tobytes() + X.encode() for ln in lens)
        return {"U": U, "offsets": np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64), "bases": np.frombuffer(text, np.uint8).copy(),
                "link_off": np.concatenate([[0], np.cumsum([len(l) for l in order])]).astype(np.uint64),
                "link_to": np.array([x for l in order for x in l], np.uint32), "E": sum(len(l) for l in order), "join": join,
                "join_count": (join != NONE32).astype(np.uint64) * np.uint64(5), "join_gap": gap}


F = lambda n: (n, 0)                                                       # a node entered forwards
R = lambda n: (n, 1)


# ---- motifs: each adds its contigs to b and returns (e, t, [intermediates of the wanted path]) in logical words -----------------
def diamond(b, arm_a: int, arm_b: int, gap: int):
    s, a, c, t = b.node(60), b.node(arm_a), b.node(arm_b), b.node(60)
    b.path(F(s), F(a), F(t))
    b.path(F(s), F(c), F(t))
    b.join(F(s), F(t), gap)
    return F(s), F(t), [F(a)]


def direct(b, gap: int):
    s, t = b.node(60), b.node(60)
    b.link(F(s), F(t))
    b.join(F(s), F(t), gap)
    return F(s), F(t), []


def selfloop(b, gap: int):
    s, r, t = b.node(60), b.node(80), b.node(60)
    b.path(F(s), F(r), F(r), F(t))
    b.join(F(s), F(t), gap)
    return F(s), F(t), [F(r), F(r)]


def bubbles(b, n: int):
    """n two-armed bubbles with a contig between two of them, all of 50 bases: 2^n paths of equal length (2 n - 1) * 28 - 22"""
    s, t = b.node(50), b.node(50)
    at = [F(s)]
    for i in range(n):
        arms = [F(b.node(50)), F(b.node(50))]
        for x in at:
            for y in arms:
                b.link(x, y)
        at = arms
        if i + 1 < n:
            j = F(b.node(50))
            for x in at:
                b.link(x, j)
            at = [j]
    for x in at:
        b.link(x, F(t))
    b.join(F(s), F(t), (2 * n - 1) * 28 - 22)
    return F(s), F(t), None


def fan(b, n: int, gap: int = 16):
    """n contigs of 60 bases side by side: n intermediates in the first round, n hits in the next"""
    s, t = b.node(60), b.node(60)
    for _ in range(n):
        b.path(F(s), F(b.node(60)), F(t))
    b.join(F(s), F(t), gap)
    return F(s), F(t), None


def chain(b, lens, gap=None, reverse_some: bool = False):
    """one path through contigs of `lens`; every other one entered backwards with reverse_some"""
    s, t = b.node(60), b.node(60)
    mid = [(b.node(ln), int(reverse_some and i % 2)) for i, ln in enumerate(lens)]
    b.path(F(s), *mid, F(t))
    b.join(F(s), F(t), sum(ln - 22 for ln in lens) - 22 if gap is None else gap)
    return F(s), F(t), mid


def joined_intermediate(b):
    """the only path leads through a contig that the scaffolder joined to another one"""
    s, m, t, x = b.node(60), b.node(60), b.node(60), b.node(60)
    b.path(F(s), F(m), F(t))
    b.join(F(s), F(t), 16)
    b.join(R(m), F(x), 30)
    return F(s), F(t), None


def three_members(b, gap2: int = None):
    """a - c - z joined in a row, the first join filled by two contigs of 60 and 100 bases, the second by one of 70 (or open with gap2)"""
    a, c, z = b.node(60), b.node(60), b.node(60)
    p, q, r = b.node(60), b.node(100), b.node(70)
    b.path(F(a), F(p), R(q), F(c), F(r), F(z))
    b.join(F(a), F(c), 38 + 78 - 22)
    b.join(F(c), F(z), 48 - 22 if gap2 is None else gap2)
    return (a, c, z), (p, q, r)


# ---- literal cases ----------------------------------------------------------------------------------------------------------
def _p(tolerance=10, max_fill=16, max_states=1024):
    return dict(tolerance=tolerance, max_fill=max_fill, max_states=max_states)


def _bubble_case(n):
    return lambda b: (bubbles(b, n), _p(0, 32, 4096), (3, 2 ** (n + 2) - 4, 0, []))


CASES = {
    "diamond_60_60": lambda b: (diamond(b, 60, 60, 16), _p(10), (3, 4, 0, [])),
    "diamond_60_100": lambda b: (diamond(b, 60, 100, 16), _p(10), (1, 2, 16, "path")),
    "diamond_60_100_tol50": lambda b: (diamond(b, 60, 100, 16), _p(50), (3, 4, 0, [])),
    "direct_tol5": lambda b: (direct(b, -20), _p(5), (1, 1, -22, "path")),
    "direct_tol1": lambda b: (direct(b, -20), _p(1), (2, 0, 0, [])),
    "selfloop": lambda b: (selfloop(b, 94), _p(10), (1, 3, 94, "path")),
    "selfloop_tol70": lambda b: (selfloop(b, 94), _p(70), (3, 6, 0, [])),
    "selfloop_fill1": lambda b: (selfloop(b, 94), _p(10, max_fill=1), (2, 1, 0, [])),
    "bubbles_1": _bubble_case(1), "bubbles_2": _bubble_case(2), "bubbles_3": _bubble_case(3), "bubbles_6": _bubble_case(6), "bubbles_10": _bubble_case(10),
    "joined_intermediate": lambda b: (joined_intermediate(b), _p(10), (2, 0, 0, [])),
    "fill_exact": lambda b: (chain(b, [50] * 5), _p(0, max_fill=5), (1, 6, 5 * 28 - 22, "path")),
    "fill_one_short": lambda b: (chain(b, [50] * 5), _p(0, max_fill=4), (2, 4, 0, [])),
    # one intermediate of 60 bases ends at d = 16: stored iff 16 <= gap + tolerance, a hit iff |16 - gap| <= tolerance
    "reach_exact": lambda b: (chain(b, [60], gap=10), _p(6), (1, 2, 16, "path")),
    "reach_one_above": lambda b: (chain(b, [60], gap=9), _p(6), (2, 0, 0, [])),
    "hit_at_gap_minus_tol": lambda b: (chain(b, [60], gap=22), _p(6), (1, 2, 16, "path")),
    "hit_beyond_gap_minus_tol": lambda b: (chain(b, [60], gap=23), _p(6), (2, 1, 0, [])),
    "mixed_strands": lambda b: (chain(b, [60, 100, 44], reverse_some=True), _p(0), (1, 4, 38 + 78 + 22 - 22, "path")),
    "fan_63": lambda b: (fan(b, 63), _p(10), (3, 126, 0, [])),
    "fan_64": lambda b: (fan(b, 64), _p(10), (3, 128, 0, [])),
    "fan_65": lambda b: (fan(b, 65), _p(10), (3, 130, 0, [])),
}
NAMES = tuple(CASES)


def case(name: str, dual: bool = True):
    """-> (graph, params, want): want = (status, states, dist, [path words]) at graph["probe"], the owner end of the join of interest.
    dual=False: only the links from the owner's side, a graph that is not dual-closed; the answers are the same."""
    b = Builder(0, dual=dual)
    (e, t, path), params, want = CASES[name](b)
    g = b.build()
    g["probe"] = b.word(e)
    assert g["probe"] < b.word(t) ^ 1
    if want[3] == "path":
        want = want[:3] + ([b.word(w) for w in path],)
    return g, params, want


def non_owner_case(gap2=None):
    """three_members with the middle contig given the largest id: the scaffold a, c, z traverses c -> z from its non-owner side.
    -> (graph, (a, c, z), (p, q, r)) as contig ids"""
    b = Builder(1)
    (a, c, z), (p, q, r) = three_members(b, gap2)
    b.order = [0, 5, 1, 2, 3, 4]                                            # node -> id: c is contig 5
    g = b.build()
    ids = lambda ns: tuple(b.order[n] for n in ns)
    return g, ids((a, c, z)), ids((p, q, r))


def below_min_gap_case():
    """two joins in a row: a direct link estimated at -20 (closed at -22) and a join without a link estimated at -5 (open: min_gap 'N')"""
    b = Builder(2)
    a, c, z = b.node(60), b.node(60), b.node(60)
    b.link(F(a), F(c))
    b.join(F(a), F(c), -20)
    b.join(F(c), F(z), -5)
    return b.build()


def make_batch(seed: int, J: int) -> dict:
    b = Builder(100 + seed, shuffle=True)
    rng, n = np.random.default_rng(71_000 + seed), 0
    while n < J:
        k = int(rng.integers(0, 12))
        if k >= 10 and n + 2 > J:
            continue
        if k == 0:
            diamond(b, 60, 60, 16)
        elif k == 1:
            diamond(b, 60, 100, 16)
        elif k == 2:
            direct(b, int(rng.integers(-40, 0)))
        elif k == 3:
            selfloop(b, (36, 94, 152, 120)[int(rng.integers(0, 4))])
        elif k == 4:
            bubbles(b, int(rng.integers(1, 8)))
        elif k == 5:
            fan(b, (3, 63, 64, 65, 70)[int(rng.integers(0, 5))])
        elif k == 6:
            chain(b, rng.integers(44, 90, int(rng.integers(1, 18))).tolist(), reverse_some=True)
        elif k == 7:
            chain(b, [60], gap=int(rng.integers(0, 40)))
        elif k == 8:
            chain(b, [50] * 3, gap=10_000)                                 # far longer than any path: the search runs into dead ends
        elif k == 9:
            s, t = b.node(60), b.node(60)                                  # no link at all
            b.join(F(s), F(t), 100)
        elif k == 10:
            joined_intermediate(b)
        else:
            three_members(b, None if rng.integers(0, 2) else 400)
        n += 2 if k >= 10 else 1
    return b.build()
