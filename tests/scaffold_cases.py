"""Inputs for the scaffolding tests (a helper, not a conftest), of two kinds.

  planted(name)   Planted(codes, tfs, genomes, pairs, insert, jitter, sizes, n_cut): an index whose graph holds repeats of 150 bases,
                  longer than the 100 bp mates, so threading cannot split them; pairs of insert 400 (every 3 bases, alternately given as
                  the reverse-complemented pair) that bridge them; `sizes` = the sorted member counts of the scaffolds wanted. The flank
                  bases next to every repeat are pairwise distinct, so every repeat is one unitig.
  make_scaffold_graph(seed)
                  contigs with hand-set scaffold links (mark reads no bases): counts at min_pairs and below, dominance met exactly and
                  missed by one (also above 2^32, where a 64-bit product decides otherwise), a best link whose dual is not the best of its
                  end, ends with 1, 5 and 70 links, chains of 2, 64, 65 and 257 contigs with members flipped at random, cycles of 2, 3 and
                  65 contigs with a unique weakest join and with ties the end id decides, gaps negative, 0, 1 and large, contigs of exactly
                  23 bases, a circular contig and a short one whose links must be ignored. "want_join" / "want_free" name ends that must /
                  must not be joined under "params".
"""
import collections

import numpy as np

import graph_resolve_cases as RC

READ_LEN, STEP, INSERT, FLANK, REPEAT, JITTER = 100, 3, 400, 500, 150, 5
MIN_BASES = 200                                                            # planted: above a repeat's unitig (150 + 22 bases at most)
Planted = collections.namedtuple("Planted", "codes tfs genomes pairs insert jitter sizes n_cut")
PLANTED = ("two_copy", "jitter", "inverted", "chain3", "cycle")
rc = RC.rc


def pairs_of(genome: str, rng, jitter: int) -> list:
    """(left, right) of a fragment every STEP bases, both in fragment orientation; every other pair is given from the other strand"""
    out = []
    for i, a in enumerate(range(0, len(genome) - INSERT - jitter, STEP)):
        ins = INSERT + (int(rng.integers(-jitter, jitter + 1)) if jitter else 0)
        left, right = genome[a:a + READ_LEN], genome[a + ins - READ_LEN:a + ins]
        if i & 1:
            left, right = rc(right), rc(left)
        out.append((left.encode(), right.encode()))
    return out


def planted(name: str) -> Planted:
    d = RC._Draw(9100 + PLANTED.index(name))
    rep = lambda: d.seq(REPEAT)
    jitter, n_cut, circular = (JITTER if name == "jitter" else 0), 0, False
    if name in ("two_copy", "jitter"):
        r = rep()
        genomes = [d.seq(FLANK, last="ACGT"[i]) + r + d.seq(FLANK, first="TGCA"[(i + 1) % 4]) for i in range(2)]
        sizes = [1, 2, 2]
    elif name == "inverted":
        genomes = [(lambda r: d.seq(FLANK, last="A") + r + d.seq(FLANK, first="A", last="G") + rc(r) + d.seq(FLANK, first="G"))(rep())]
        sizes = [1, 3]
    elif name == "chain3":
        r1, r2 = rep(), rep()
        genomes = [d.seq(FLANK, last="A") + r1 + d.seq(FLANK, first="T", last="A") + r2 + d.seq(FLANK, first="T"),
                   d.seq(FLANK, last="C") + r1 + d.seq(FLANK, first="G", last="C") + r2 + d.seq(FLANK, first="G")]
        sizes = [1, 1, 3, 3]
    else:
        assert name == "cycle"
        r = rep()
        ring = d.seq(FLANK, first="T", last="A") + r + d.seq(FLANK, first="G", last="C") + r + d.seq(FLANK, first="C", last="G") + r
        genomes, sizes, n_cut, circular = [ring], [1, 3], 1, True
    rng = np.random.default_rng(77 + PLANTED.index(name))
    lin = [g + g[:INSERT + STEP] for g in genomes] if circular else genomes
    pairs = [p for g in lin for p in pairs_of(g, rng, jitter)]
    codes, tfs = RC._index(lin, [m for p in pairs for m in p])
    return Planted(codes, tfs, genomes, pairs, INSERT, jitter, sizes, n_cut)


def mates(pairs) -> list:
    """the sequences of a batch: left mate, right mate, left mate, .."""
    return [m for p in pairs for m in p]


def located(p: Planted, text: str):
    """(genome index, strand, start) of an oriented contig in the planted genomes (a ring is searched doubled)"""
    for gi, g in enumerate(p.genomes):
        for strand, s in ((0, g), (1, rc(g))):
            at = (s + s if p.n_cut else s).find(text)
            if at >= 0:
                return gi, strand, at
    return None


# ---- hand-set scaffold graphs ----------------------------------------------------------------------------
MIN_PAIRS, DOMINANCE, MIN_CONTIG, INSERT_G, MIN_GAP = 4, 3, 40, 300, 1
BIG_THIRD = 6148914691236517206                                            # ceil(2^64 / 3): times 3 it wraps to 2 in 64 bits


def make_scaffold_graph(seed: int) -> dict:
    rng = np.random.default_rng(61_000 + seed)
    lens, circ, flip, links = [], [], [], {}
    want_join, want_free, chains = [], [], {}

    def node(length=None, circular=0):
        lens.append(int(rng.integers(MIN_CONTIG, 91)) if length is None else length)
        circ.append(circular)
        flip.append(int(rng.integers(0, 2)))
        return len(lens) - 1

    def link(a, b, count, d=None, dsum=None):
        """a's exit to b's entry, in the orientation their flips give; returns (e, t)"""
        e, t = 2 * a + flip[a], 2 * b + flip[b]
        d = int(rng.integers(50, 280)) if d is None else d
        links[(e, t)] = (count, count * d if dsum is None else dsum)
        return e, t

    firm = lambda: int(rng.integers(MIN_PAIRS, 60))
    # counts at exactly min_pairs and one below
    want_join.append(link(node(), node(), MIN_PAIRS))
    want_free.append(link(node(), node(), MIN_PAIRS - 1)[0])
    # dominance met exactly and missed by one; the same above 2^32; a product that wraps in 64 bits
    for best, other, joined in ((30, 10, True), (29, 10, False), (3 * ((1 << 33) + 1), (1 << 33) + 1, True), (3 * ((1 << 33) + 1) - 1, (1 << 33) + 1, False),
                                ((1 << 63) + 5, BIG_THIRD, False)):
        a, b, c = node(), node(), node()
        e, t = link(a, b, best, d=1)
        link(a, c, other, d=1)
        (want_join if joined else want_free).append((e, t) if joined else e)
    # a best link whose dual is not the best of its end
    a, b, c = node(), node(), node()
    e, t = link(a, b, 20)
    want_join.append(link(c, b, 60))
    want_free.append(e)
    # ends with 1, 5 and 70 links
    for n in (1, 5, 70):
        h = node()
        outs = [node() for _ in range(n)]
        k = int(rng.integers(0, n))
        for i, x in enumerate(outs):
            got = link(h, x, 1000 if i == k else int(rng.integers(1, 300)))
            if i == k:
                want_join.append(got)
    # chains, members flipped at random; gaps negative, 0, 1 and large
    for n in (2, 64, 65, 257):
        ids = [node() for _ in range(n)]
        for i in range(n - 1):
            d = (INSERT_G + 7, INSERT_G, INSERT_G - 1, 1)[i % 4] if n == 65 else None
            want_join.append(link(ids[i], ids[i + 1], firm(), d=d))
        chains["chain%d" % n] = ids
    ids = [node(23) for _ in range(3)]                                     # contigs of exactly 23 bases: joined only with min_contig_bases 0
    for i in range(2):
        want_free.append(link(ids[i], ids[i + 1], firm())[0])
    chains["tiny"] = ids
    # cycles: a unique weakest join; ties on count, where the end id decides; counts that the key clamps to 2^32 - 1
    for tag, n, counts in (("cycle2", 2, [50, 20]), ("cycle3", 3, [50, 20, 50]), ("cycle65", 65, [50] * 30 + [20] + [50] * 34), ("tied", 5, [20, 50, 20, 50, 20]),
                           ("clamped", 3, [(1 << 32) + 5, (1 << 32) + 1, (1 << 32) + 9])):
        ids = [node() for _ in range(n)]
        for i in range(n):
            want_join.append(link(ids[i], ids[(i + 1) % n], counts[i]))
        chains[tag] = ids
    # a circular contig and a short one carrying links that must be ignored
    for special in (node(circular=1), node(30)):
        x = node()
        want_free.append(link(special, x, 500)[0])
        want_free.append(link(node(), special, 500)[0])
    # ids in random order
    U = len(lens)
    perm = rng.permutation(U).tolist()
    word = lambda w: 2 * perm[w >> 1] + (w & 1)
    canon = lambda e, t: (e, t) if e < t ^ 1 else (t ^ 1, e ^ 1)
    links = {canon(word(e), word(t)): v for (e, t), v in links.items()}
    inv = np.argsort(perm)
    lens, circ = [lens[i] for i in inv], [circ[i] for i in inv]
    g = {"U": U, "offsets": np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64), "circular": np.array(circ, np.uint8)}
    g["bases"] = np.frombuffer("".join("ACGT"[b] for b in rng.integers(0, 4, int(sum(lens))).tolist()).encode(), dtype=np.uint8).copy()
    g.update(slinks_of(links, U))
    small = [(k, v) for k, v in sorted(links.items()) if v[0] <= 300]
    obs = []
    for (e, t), (count, dsum) in small:
        d = dsum // count
        ds = [d] * count
        if count >= 2 and d >= 3:                                          # unequal d in a bundle, the same sum
            ds[0], ds[1] = d - 2, d + 2
        obs += [(e << 32 | t, x) for x in ds]
    obs += [((1 << 64) - 1, 0)] * 37
    order = rng.permutation(len(obs)).tolist()
    g["obs_key"] = np.array([obs[i][0] for i in order], np.uint64)
    g["obs_d"] = np.array([obs[i][1] for i in order], np.uint32)
    g["obs_slinks"] = slinks_of(dict(small), U)
    g["want_join"] = [canon(word(e), word(t)) for e, t in want_join]
    g["want_free"] = [word(e) for e in want_free]
    g["chains"] = {k: [perm[i] for i in v] for k, v in chains.items()}
    g["params"] = dict(insert_size=INSERT_G, min_pairs=MIN_PAIRS, dominance=DOMINANCE, min_contig_bases=MIN_CONTIG)
    return g


def make_chains(seed: int, U: int) -> dict:
    """U contigs in random id order and orientation, joined into chains and cycles of 1 to 40: the same dict as make_scaffold_graph without
    the expectations"""
    rng = np.random.default_rng(63_000 + seed)
    lens = rng.integers(23, 60, U)
    flip = rng.integers(0, 2, U).tolist()
    ids, links, at, k = rng.permutation(U).tolist(), {}, 0, 0
    while at < U:
        n = min(int(rng.integers(1, min(41, U // 5))), U - at)
        run = ids[at:at + n]
        k += 1
        for i in range(n - 1 if n < 3 or k % 2 else n):                    # every other run of three or more is closed into a cycle
            a, b = run[i], run[(i + 1) % n]
            e, t = 2 * a + flip[a], 2 * b + flip[b]
            count = int(rng.integers(MIN_PAIRS, 9))
            links[(e, t) if e < t ^ 1 else (t ^ 1, e ^ 1)] = (count, count * int(rng.integers(250, 320)))
        at += n
    g = {"U": U, "offsets": np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64), "circular": np.zeros(U, np.uint8)}
    g["bases"] = np.frombuffer("".join("ACGT"[b] for b in rng.integers(0, 4, int(lens.sum())).tolist()).encode(), dtype=np.uint8).copy()
    g.update(slinks_of(links, U))
    g["params"] = dict(insert_size=INSERT_G, min_pairs=MIN_PAIRS, dominance=DOMINANCE, min_contig_bases=0)
    return g


def make_pair_batch(seed: int, P: int, offsets, read_len: int = 100):
    """hand-set step arrays of P pairs over contigs with `offsets` (no index behind them): mates with 0 to 3 steps anywhere, ties for the
    most windows, mates that start before their contig or end behind it. -> (offs uint64[2 P + 1], steps dict)"""
    rng = np.random.default_rng(62_000 + seed)
    off = [int(x) for x in offsets]
    U = len(off) - 1
    sso, rows = [0], []
    home = 0
    for m in range(2 * P):
        q = 0
        if m % 2 == 0:
            home = int(rng.integers(0, U))
        u = home
        for _ in range(int(rng.integers(0, 4))):
            if rng.integers(0, 3) == 0:
                u = int(rng.integers(0, U))                                # mostly on the pair's contig: same-contig pairs and links both occur
            w = int(rng.integers(1, 30))
            if q + w > read_len - 22:
                break
            rows.append((u, int(rng.integers(0, off[u + 1] - off[u] - 22)), int(rng.integers(0, 2)), q, q + w - 1))
            q += w + int(rng.integers(0, 5))
        sso.append(len(rows))
    cols = list(zip(*rows)) if rows else [[]] * 5
    steps = {"seq_step_off": np.array(sso, np.uint64)}
    for k, dt, col in zip(("step_unitig", "step_pos", "step_flag", "q_first", "q_last"), (np.uint32, np.uint32, np.uint8, np.uint32, np.uint32), cols):
        steps[k] = np.array(col, dtype=dt)
    return np.arange(2 * P + 1, dtype=np.uint64) * np.uint64(read_len), steps


def make_pairs_before_contig(offsets, circular, read_len: int = 100):
    """three hand-set pairs between the first two linear contigs u -> v whose right mate claims a q_first beyond its own length, so that
    it ends in front of v: d far below 0, d == 0 and d == 1. -> (offs, steps, (u, v))"""
    off = [int(x) for x in offsets]
    u, v = [i for i, c in enumerate(circular) if not c][:2]
    Lu = off[u + 1] - off[u]
    rows = []
    for d in (-1000, 0, 1):                                                # d = (L_u - 0) + (0 - q_first + read_len)
        rows += [(u, 0, 0, 0, 0), (v, 0, 0, Lu + read_len - d, Lu + read_len - d)]
    steps = {"seq_step_off": np.arange(7, dtype=np.uint64)}
    for k, dt, col in zip(("step_unitig", "step_pos", "step_flag", "q_first", "q_last"), (np.uint32, np.uint32, np.uint8, np.uint32, np.uint32), zip(*rows)):
        steps[k] = np.array(col, dtype=dt)
    return np.arange(7, dtype=np.uint64) * np.uint64(read_len), steps, (u, v)


def slinks_of(links: dict, U: int) -> dict:
    """the CSR over ends of canonical links {(e, t): (count, dsum)}: every link and its dual"""
    ends = [[] for _ in range(2 * U)]
    for (e, t), (count, dsum) in links.items():
        ends[e].append((t, count, dsum))
        ends[t ^ 1].append((e ^ 1, count, dsum))
    flat = [x for l in ends for x in sorted(l)]
    return {"slink_off": np.concatenate([[0], np.cumsum([len(l) for l in ends])]).astype(np.uint64), "slink_to": np.array([x[0] for x in flat], np.uint32),
            "slink_count": np.array([x[1] for x in flat], np.uint64), "slink_dsum": np.array([x[2] for x in flat], np.uint64), "S": len(flat)}
