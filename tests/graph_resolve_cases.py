"""Inputs for the repeat-resolution tests (a helper, not a conftest), of two kinds.

  planted(name)   Planted(codes, tfs, reads, contigs, n_split, n_removed): an index whose graph holds a planted repeat, the reads that
                  resolve it (100 bp every 3 bases, alternately reverse-complemented) and the contigs the resolution must give, up to
                  strand. The flank bases next to every repeat are set pairwise distinct, so the repeat is one unitig with the wanted
                  d x d shape: the tests assert n_split, they never skip.
  make_resolve_graph(seed)
                  a link structure with hand-set link_support and pair_support (mark reads no bases): cells at exactly min, min - 1, noise
                  and noise + 1; d = 2, 3, 4; 2 x 1 and 3 x 2 shapes, a 3 x 2 that pruning turns into 2 x 2; closed lattices in which every
                  link joins two split unitigs, in all four word orientations; tf_sum and cells above 2^32 and near 2^64. "want" maps a
                  unitig to the copies it must get.
"""
import collections

import numpy as np

import unitigs_cases as UC
import unitigs_ref as R

K = 23
READ_LEN, READ_STEP = 100, 3
FLANK, REPEAT = 120, 40
_RC = str.maketrans("ACGT", "TGCA")
Planted = collections.namedtuple("Planted", "codes tfs reads contigs n_split n_removed")
PLANTED = ("two_copy", "inverted", "adjacent", "three_copy", "four_copy", "twice", "ambiguous", "tandem", "hairpin_ends", "weak_fork")


def rc(s: str) -> str:
    return s[::-1].translate(_RC)


def canon_str(s: str) -> str:
    return min(s, rc(s))


def reads_of(genome: str) -> list:
    starts = list(range(0, len(genome) - READ_LEN + 1, READ_STEP))
    if starts[-1] != len(genome) - READ_LEN:
        starts.append(len(genome) - READ_LEN)
    return [(rc(genome[a:a + READ_LEN]) if i & 1 else genome[a:a + READ_LEN]).encode() for i, a in enumerate(starts)]


def _index(sequences, reads):
    """codes and tfs of the canonical 23-mers of `sequences`; tf = the occurrences in the reads, at least 1"""
    count = collections.Counter()
    enc = lambda s: UC._codes_of(["ACGT".index(c) for c in s])
    for r in reads:
        count.update(R.canon(x) for x in enc(r.decode()))
    keys = sorted({R.canon(x) for s in sequences for x in enc(s)})
    return np.array(keys, dtype=np.uint64), np.array([max(1, count[k]) for k in keys], dtype=np.uint32)


class _Draw:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)

    def seq(self, n, first=None, last=None):
        s = "".join("ACGT"[b] for b in self.rng.integers(0, 4, n).tolist())
        if first:
            s = first + s[1:]
        if last:
            s = s[:-1] + last
        return s


def planted(name: str) -> Planted:
    d = _Draw(7000 + PLANTED.index(name))
    rep = lambda: d.seq(REPEAT)
    n_split, n_removed, extra = 1, 0, []
    if name in ("two_copy", "three_copy", "four_copy"):
        r, n = rep(), {"two_copy": 2, "three_copy": 3, "four_copy": 4}[name]
        genomes = [d.seq(FLANK, last="ACGT"[i]) + r + d.seq(FLANK, first="TGCA"[(i + 1) % 4]) for i in range(n)]
    elif name == "inverted":                                           # in R's orientation: left A / comp(first C), right first B / comp(last B)
        genomes = [(lambda r: d.seq(FLANK, last="A") + r + d.seq(FLANK, first="A", last="G") + rc(r) + d.seq(FLANK, first="G"))(rep())]
    elif name == "adjacent":
        # S holds both repeats, overlapping by 22 bases: R1 = S[:40] ends in the k-mer x = S[17:40], R2 = S[18:] starts with its
        # successor S[18:41]. x has a second successor (X), S[18:41] a second predecessor (Y): R1 -> R2 is one link between two split unitigs
        s = d.seq(17) + "A" + d.seq(22) + "A" + d.seq(23)
        genomes = [d.seq(FLANK, last="A") + s + d.seq(FLANK, first="A"), d.seq(FLANK, last="C") + s[:40] + d.seq(FLANK, first="C"),
                   d.seq(FLANK, last="C") + s[18:] + d.seq(FLANK, first="C")]
        n_split, n_removed = 2, 2                                      # Y's last k-mer C + S[18:40] is also followed by X's first, S[18:40] + C:
                                                                       # a link Y -> X that no read follows, and its dual
    elif name == "twice":
        genomes = [(lambda r: d.seq(FLANK, last="A") + r + d.seq(FLANK, first="A", last="C") + r + d.seq(FLANK, first="C"))(rep())]
    elif name == "ambiguous":                                          # A R B, C R D and A R D: no one-to-one pairing
        r = rep()
        a, b, c, e = d.seq(FLANK, last="A"), d.seq(FLANK, first="A"), d.seq(FLANK, last="C"), d.seq(FLANK, first="C")
        genomes, n_split = [a + r + b, c + r + e, a + r + e], 0
    elif name == "tandem":                                             # R R: the self-link forbids the split
        # the 40 cyclic k-mers of r are one unitig r + r[:22]; its last k-mer r[39] + r[:22] is followed by its first (base r[22]) and by B
        r = d.seq(22) + "A" + d.seq(16) + "A"
        genomes, n_split = [d.seq(FLANK, last="C") + r + r + r[:22] + d.seq(FLANK, first="C")], 0
        n_removed = 2                                                  # A's last k-mer C + r[:22] is also followed by B's first, r[:22] + C: unread
    elif name == "weak_fork":                                          # a branch in the index that no read follows
        p, q = d.seq(FLANK, last="A"), d.seq(FLANK, first="A")
        genomes, extra, n_split, n_removed = [p + q], [p[-(K - 1):] + d.seq(30, first="C")], 0, 2
    else:
        assert name == "hairpin_ends"
        case = UC.topology_cases()[name]
        return Planted(case.codes, case.tfs, None, None, None, None)
    reads = [r for g in genomes for r in reads_of(g)]
    codes, tfs = _index(genomes + extra, reads)
    if name in ("ambiguous", "tandem"):
        contigs = None                                                 # the unitigs, unchanged
    else:
        contigs = sorted(canon_str(s) for s in genomes + extra)
    return Planted(codes, tfs, reads, contigs, n_split, n_removed)


# ---- link structures ------------------------------------------------------------------------------------
MIN_LINK, MIN_PAIR, MAX_NOISE = 5, 7, 2
BIG_CELLS = ((1 << 64) - 5, (1 << 64) - 9, (1 << 63) + 3, (1 << 40) + 1)
BIG_TF = ((1 << 64) - 1, (1 << 63) + 12345, (1 << 33) + 7, 3 * (1 << 60))


class _Net:
    def __init__(self, rng):
        self.rng, self.ends, self.flip, self.sup = rng, [], [], {}

    def node(self):
        self.ends += [[], []]
        self.flip.append(int(self.rng.integers(0, 2)))
        return len(self.flip) - 1

    def link(self, a, b, support):
        """a's right end to b's left end (right / left as the node's flip says), and the dual"""
        e, t = 2 * a + self.flip[a], 2 * b + self.flip[b]
        self.ends[e].append(t)
        self.sup[(e, t)] = support
        if (t ^ 1, e ^ 1) != (e, t):
            self.ends[t ^ 1].append(e ^ 1)
            self.sup[(t ^ 1, e ^ 1)] = support

    def local(self, e, t):
        return self.ends[e].index(t)


def make_resolve_graph(seed: int, motifs: int = 40) -> dict:
    rng = np.random.default_rng(52_000 + seed)
    net = _Net(rng)
    cells, want, big = {}, {}, []
    firm = lambda: int(rng.integers(MIN_LINK, 60))

    def centre(n_left, n_right, weak_left=0):
        c = net.node()
        lefts, rights = [net.node() for _ in range(n_left)], [net.node() for _ in range(n_right)]
        for i, a in enumerate(lefts):
            net.link(a, c, int(rng.integers(0, MIN_LINK)) if i < weak_left else firm())
        for b in rights:
            net.link(c, b, firm())
        return c, lefts, rights

    def cell(c, a, b, v):
        """the cell of centre c between its left neighbour a and its right neighbour b"""
        f = net.flip[c]
        right = (2 * c + f, 2 * b + net.flip[b])                       # the link c -> b at c's right end
        left = (2 * c + (f ^ 1), (2 * a + net.flip[a]) ^ 1)            # the dual of a -> c at c's left end
        cells[(c, left if f else right, right if f else left)] = v     # keyed by (unitig, link at end 2 c, link at end 2 c + 1)

    def permutation(c, lefts, rights, strong, other, spoil=None):
        perm = rng.permutation(len(rights)).tolist()
        for i, a in enumerate(lefts):
            for j, b in enumerate(rights):
                cell(c, a, b, strong() if perm[i] == j else other())
        if spoil is not None:
            i = int(rng.integers(0, len(lefts)))
            on = spoil[0] == "strong"
            j = perm[i] if on else next(j for j in range(len(rights)) if j != perm[i])
            cell(c, lefts[i], rights[j], spoil[1])

    strong = lambda: int(rng.integers(MIN_PAIR, 200))
    noise = lambda: int(rng.integers(0, MAX_NOISE + 1))
    kinds = ["exact", "min-1", "noise+1", "d2", "d3", "d4", "2x1", "3x2", "pruned", "lattice", "big", "unseen"]
    for i in range(motifs):
        kind = kinds[i % len(kinds)]
        if kind == "exact":                                            # strong cells at exactly min, the others at exactly noise
            c, ls, rs = centre(2, 2)
            permutation(c, ls, rs, lambda: MIN_PAIR, lambda: MAX_NOISE)
            want[c] = 2
        elif kind == "min-1":
            c, ls, rs = centre(2, 2)
            permutation(c, ls, rs, strong, noise, spoil=("strong", MIN_PAIR - 1))
            want[c] = 1
        elif kind == "noise+1":
            c, ls, rs = centre(3, 3)
            permutation(c, ls, rs, strong, noise, spoil=("other", MAX_NOISE + 1))
            want[c] = 1
        elif kind in ("d2", "d3", "d4"):
            n = int(kind[1])
            c, ls, rs = centre(n, n)
            permutation(c, ls, rs, strong, noise)
            want[c] = n
        elif kind in ("2x1", "3x2"):
            c, ls, rs = centre(int(kind[0]), int(kind[2]))
            for a in ls:
                for b in rs:
                    cell(c, a, b, strong())
            want[c] = 1
        elif kind == "pruned":                                         # 3 x 2; the weak left link goes, what is left pairs up
            c, ls, rs = centre(3, 2, weak_left=1)
            permutation(c, ls[1:], rs, strong, noise)
            for b in rs:
                cell(c, ls[0], b, strong())                            # cells of a removed link are ignored
            want[c] = 2
        elif kind == "lattice":                                        # x_i -> y_j -> x_i: every link joins two split unitigs
            xs, ys = [net.node(), net.node()], [net.node(), net.node()]
            for x in xs:
                for y in ys:
                    net.link(x, y, firm())
                    net.link(y, x, firm())
            for c, around in ((xs[0], ys), (xs[1], ys), (ys[0], xs), (ys[1], xs)):
                permutation(c, around, around, strong, noise)
                want[c] = 2
        elif kind == "big":                                            # products beyond 64 bits decide the abundances
            c, ls, rs = centre(4, 4)
            vals = list(BIG_CELLS)
            permutation(c, ls, rs, lambda: vals.pop(), noise)
            want[c] = 4
            big.append(c)
        else:                                                          # all cells zero: nobody passed
            c, ls, rs = centre(2, 2)
            want[c] = 1
    U = len(net.flip)
    for e in range(2 * U):                                             # list order is not insertion order
        net.ends[e] = [net.ends[e][k] for k in rng.permutation(len(net.ends[e])).tolist()]
    n_circ = 3
    lens = rng.integers(K, 90, U + n_circ)
    g = {"U": U + n_circ, "offsets": np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)}
    g["bases"] = np.frombuffer("".join("ACGT"[b] for b in rng.integers(0, 4, int(lens.sum())).tolist()).encode(), dtype=np.uint8).copy()
    g["circular"] = np.array([0] * U + [1] * n_circ, dtype=np.uint8)
    g["tf_sum"] = rng.integers(1, 1 << 40, U + n_circ, dtype=np.uint64)
    for c, v in zip(big, BIG_TF * (len(big) // len(BIG_TF) + 1)):
        g["tf_sum"][c] = v
    g["tf_min"] = rng.integers(1, 100, U + n_circ).astype(np.uint32)
    g["tf_max"] = g["tf_min"] + rng.integers(0, 100, U + n_circ).astype(np.uint32)
    ends = net.ends + [[] for _ in range(2 * n_circ)]
    g["link_off"] = np.concatenate([[0], np.cumsum([len(l) for l in ends])]).astype(np.uint64)
    g["link_to"] = np.array([t for l in ends for t in l], dtype=np.uint32)
    g["E"] = int(g["link_to"].shape[0])
    g["link_support"] = np.array([net.sup[(e, t)] for e, l in enumerate(ends) for t in l], dtype=np.uint64)
    pair = np.zeros(16 * g["U"], np.uint64)
    for (c, l0, l1), v in cells.items():
        pair[16 * c + 4 * net.local(*l0) + net.local(*l1)] = v
    g["pair_support"] = pair
    g["want"] = want
    g["thresholds"] = (MIN_LINK, MIN_PAIR, MAX_NOISE)
    return g


def asymmetric(g: dict) -> dict:
    """g with the support of one link that is not its own dual raised by one: mark must refuse it"""
    lo, to = g["link_off"].tolist(), g["link_to"].tolist()
    e = next(e for e in range(2 * g["U"]) if lo[e + 1] > lo[e] and to[lo[e]] != e ^ 1)
    sup = g["link_support"].copy()
    sup[lo[e]] += np.uint64(1)
    return dict(g, link_support=sup)
