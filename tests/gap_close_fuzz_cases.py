"""Inputs for the gap-closing fuzz (a helper, not a conftest): contig graphs in which the searches of different joins meet.

  tangled(seed, U)  joins marked from bundled random observations (chains and rings of 2 .. 6 contigs, noise links that break dominance
                    in places), random links per end over all 2 U ends (duplicates, self-links, links into joined contigs, into the
                    source contig and into t ^ 1), and for about 70 % of the joins a planted walk of 0 .. 5 unjoined contigs, partly
                    through a few hub contigs that many walks share. A planted join is observed at the distance that puts its estimated
                    gap within 12 bases of the walk, so join and join_gap are exactly what the marking gives for obs_key / obs_d.
  corridor(k, m)    k joins whose only paths run through one chain of m unjoined contigs: the path total k m exceeds U = 2 k + m.
  giant()           hand-set arrays without bases: a gap of 2^30 closed at exactly gap + tolerance through two contigs of about 2^29
                    bases, side links into contigs of 2^40 and 2^33 bases, a gap of -2^30, filled positions beyond 2^32.
  budget_values(r)  the values of max_states at which a search changes between complete and exhausted; edge_param_sets(r) has them
                    with the edges of max_fill and tolerance.

A graph is a dict in the format of gap_close_cases (U, offsets, bases, link_off, link_to, E, join, join_count, join_gap) with circular,
obs_key, obs_d and params (the arguments of the marking) beside them. The bases of a tangled graph are random: two linked contigs do
not share their 22 bases, which no call compares."""
import numpy as np

import gap_close_cases as GC
import scaffold_ref as SF

NONE32 = SF.NONE32
SEEDS = tuple(range(8))
PARAM_SETS = (dict(tolerance=10, max_fill=16, max_states=256), dict(tolerance=40, max_fill=64, max_states=4096), dict(tolerance=0, max_fill=3, max_states=65))
LENGTHS = (23, 24, 30, 45, 60, 61, 100, 150, 300)
LENGTH_WEIGHTS = (0.04, 0.04, 0.07, 0.15, 0.15, 0.15, 0.15, 0.15, 0.1)
INSERT = 5000
MARK = dict(insert_size=INSERT, min_pairs=2, dominance=2, min_contig_bases=24)
CORRIDOR_PARAMS = dict(tolerance=0, max_fill=16, max_states=256)
GIANT_PARAMS = dict(tolerance=1 << 20, max_fill=4, max_states=64)
SMALL = (16, 48)                                                           # tangled(*SMALL): the graph of the budget and fill edges
FULL = dict(tolerance=10, max_fill=16, max_states=4096)                    # ... and the complete search its budgets are read from


def _csr(lists):
    return (np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint64), np.array([x for l in lists for x in l], np.uint32))


def _canonical(e, t):
    return (t ^ 1, e ^ 1) if t ^ 1 < e else (e, t)


def _observations(rng, pairs, dist):
    """c observations per pair whose distances average dist[pair] exactly, a few dead entries between them, in random order"""
    key, d = [], []
    for (e, t), c in pairs.items():
        x = dist[(e, t)]
        ds = [x] * c
        if c >= 2 and x >= 2:
            ds[0], ds[1] = x + 1, x - 1
        key += [e << 32 | t] * c
        d += ds
    for _ in range(5):
        key.append(SF.NOKEY)
        d.append(0)
    order = rng.permutation(len(key))
    return np.array(key, np.uint64)[order], np.array(d, np.uint32)[order]


def tangled(seed: int, U: int = 128) -> dict:
    rng = np.random.default_rng(90_000 + seed)
    lens = rng.choice(LENGTHS, U, p=LENGTH_WEIGHTS).tolist()
    L = lambda w: lens[w >> 1]
    circular = np.zeros(U, np.uint8)
    circular[rng.choice(U, 4, replace=False)] = 1
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    bases = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(offsets[-1]))].copy()
    # the scaffold graph: chains and rings over a random order of the contigs in random orientations, and noise
    perm, pairs, rings, i = rng.permutation(U).tolist(), {}, set(), 0

    def observe(e, t, c):
        k = _canonical(e, t)
        pairs[k] = pairs.get(k, 0) + c

    while i + 6 <= (3 * U) // 5:
        n = int(rng.integers(2, 7))
        words = [2 * perm[i + j] + int(rng.integers(0, 2)) for j in range(n)]
        ring = rng.random() < 0.3
        for e, t in list(zip(words, words[1:])) + ([(words[-1], words[0])] if ring else []):
            observe(e, t, int(rng.integers(2, 6)))
            if ring:
                rings.add(_canonical(e, t))                              # the joins of a ring always get a walk: the cut one may close
        i += n
    for _ in range(U // 5):
        e, t = (int(x) for x in rng.integers(0, 2 * U, 2))
        if e >> 1 != t >> 1:
            observe(e, t, int(rng.integers(1, 5)))
    mark = lambda dist: SF.mark(offsets, circular, SF.bundle(*_observations(rng, pairs, dist), U), **MARK)
    jn = mark({k: 100 for k in pairs})["join"].tolist()                  # which ends are joined depends on the counts alone
    free = [u for u in rng.permutation(U).tolist() if jn[2 * u] == NONE32 and jn[2 * u + 1] == NONE32]
    hubs = free[:6]
    # the contig graph: random lists, then the planted walks
    dual = bool(seed & 1)
    lists = [[] for _ in range(2 * U)]
    for w in range(2 * U):
        for _ in range(int(rng.integers(0, 7)) if rng.random() < (0.15 if dual else 0.3) else int(rng.integers(0, 3))):   # degree 0 .. 6, mostly small
            kind = rng.random()
            if kind < 0.1:
                lists[w].append(w)                                       # a self-loop
            elif kind < 0.2:
                lists[w].append(w ^ 1)
            elif kind < 0.3 and lists[w]:
                lists[w].append(lists[w][-1])                            # a duplicate entry
            else:
                lists[w].append(int(rng.integers(0, 2 * U)))
    dist = {}
    for k in pairs:
        dist[k] = int(rng.integers(1, 1001))
    for e in range(2 * U):
        t = jn[e]
        if t == NONE32 or e > t ^ 1:
            continue
        gap = int(rng.integers(-30, 400))
        if rng.random() < 0.7 or (e, t) in rings:
            walk = []
            for _ in range(int(rng.integers(0, 6))):
                u = hubs[int(rng.integers(0, len(hubs)))] if rng.random() < 0.5 else free[int(rng.integers(0, len(free)))]
                walk.append(2 * u + int(rng.integers(0, 2)))
            both = rng.random() < 0.5                                    # the walk's dual beside it
            for a, b in zip([e] + walk, walk + [t]):
                lists[a].insert(int(rng.integers(0, len(lists[a]) + 1)), b)
                if both:
                    lists[b ^ 1].insert(int(rng.integers(0, len(lists[b ^ 1]) + 1)), a ^ 1)
            gap = -22 + sum(L(w) - 22 for w in walk) + (0 if rng.random() < 0.3 else int(rng.integers(-12, 13)))
        dist[(e, t)] = INSERT - gap
    if dual:
        for a, b in [(a, b) for a in range(2 * U) for b in lists[a]]:
            if a ^ 1 not in lists[b ^ 1]:
                lists[b ^ 1].append(a ^ 1)
    key, d = _observations(rng, pairs, dist)
    mk = SF.mark(offsets, circular, SF.bundle(key, d, U), **MARK)
    assert mk["join"].tolist() == jn
    link_off, link_to = _csr(lists)
    return {"U": U, "offsets": offsets, "bases": bases, "circular": circular, "link_off": link_off, "link_to": link_to, "E": len(link_to), "join": mk["join"],
            "join_count": mk["join_count"], "join_gap": mk["join_gap"], "obs_key": key, "obs_d": d, "params": dict(MARK)}


def corridor(k: int = 8, m: int = 8) -> dict:
    """-> the graph with "corridor", the m contig ids of the shared chain; every join closes through all of them under CORRIDOR_PARAMS"""
    assert k * m > 2 * k + m
    b = GC.Builder(500, shuffle=True)
    mid = [(b.node(50), i % 2) for i in range(m)]
    for _ in range(k):
        s, t = b.node(60), b.node(60)
        b.path(GC.F(s), *mid, GC.F(t))
        b.join(GC.F(s), GC.F(t), m * 28 - 22)
    g = b.build()
    g.update(circular=np.zeros(g["U"], np.uint8), corridor=[b.word(w) >> 1 for w in mid])
    return g


GIANT_HALF = (1 << 29) + (1 << 19) + 33                                     # two of them: -22 + 2 (L - 22) = 2^30 + 2^20


def giant() -> dict:
    """contigs Z A B P Q X Y C D = 0 .. 8. Z -> A (gap 7, no link), A -> B (gap 2^30; A -> P -> Q reversed -> B), C -> D (gap -2^30, a
    direct link). X (2^40 + 50 bases) and Y (2^33 + 50) are linked from A and P and lead on to B: cut to 32 bits they would be 50 bases
    long and stored. The scaffold Z A P Q B has every position behind Z beyond 2^33."""
    lens = [(1 << 33) + 7, 100, 100, GIANT_HALF, GIANT_HALF, (1 << 40) + 50, (1 << 33) + 50, 64, 64]
    U = len(lens)
    Z, A, B, P, Q, X, Y, Cc, D = range(U)
    lists = [[] for _ in range(2 * U)]
    for a, b in ((2 * A, 2 * X), (2 * A, 2 * P), (2 * A, 2 * Y), (2 * P, 2 * Y), (2 * P, 2 * Q + 1), (2 * P, 2 * X), (2 * Q + 1, 2 * B), (2 * X, 2 * B), (2 * Y, 2 * B),
                 (2 * Cc, 2 * D)):
        lists[a].append(b)
    join, gap = np.full(2 * U, NONE32, np.uint32), np.zeros(2 * U, np.int64)
    for e, t, x in ((2 * Z, 2 * A, 7), (2 * A, 2 * B, 1 << 30), (2 * Cc, 2 * D, -(1 << 30))):
        join[e], join[t ^ 1], gap[e], gap[t ^ 1] = t, e ^ 1, x, x
    link_off, link_to = _csr(lists)
    g = {"U": U, "offsets": np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64), "link_off": link_off, "link_to": link_to, "E": len(link_to), "join": join,
         "join_count": (join != NONE32).astype(np.uint64) * np.uint64(5), "join_gap": gap, "circular": np.zeros(U, np.uint8)}
    g.update(members(g))
    return g


def members(g, min_gap: int = 1) -> dict:
    """member_off and member from the layout's map alone (what the emit derives; no bases are needed)"""
    lay = SF.layout(g["offsets"], g["join"], g["join_count"], g["join_gap"], min_gap)
    sc, rank, flag = (lay[k].tolist() for k in ("contig_scaffold", "contig_rank", "contig_flag"))
    order = sorted(range(len(sc)), key=lambda u: (sc[u], rank[u]))
    return {"member_off": np.searchsorted(np.array([sc[u] for u in order]), np.arange(lay["n_scaffolds"] + 1)).astype(np.uint64),
            "member": np.array([2 * u + flag[u] for u in order], np.uint32)}


def budget_values(closure, most: int = 12) -> list:
    """up to `most` distinct state counts n >= 2 of the joins of a complete search: the two smallest, the two largest and those nearest 64
    and 128 (a search with max_states = n is complete, with n - 1 exhausted)"""
    ns = sorted({int(n) for n, s in zip(closure["close_states"], closure["close_status"]) if s in (1, 2, 3) and n >= 2})
    ends = ns[:2] + ns[-2:]
    near = sorted((n for n in ns if n not in ends), key=lambda n: min(abs(n - 64), abs(n - 128)))
    return sorted(set(ends + near[:most - len(set(ends))]))


def edge_param_sets(closure):
    """closure: the search of tangled(*SMALL) under FULL. -> (ns, sets): max_states at n and n - 1 for every n of budget_values, then
    max_fill at 0, 1, 2 and 64, then tolerance at 0 and 2^20"""
    ns = budget_values(closure)
    sets = [dict(FULL, max_states=m) for n in ns for m in (n, n - 1)]
    return ns, sets + [dict(FULL, max_fill=f) for f in (0, 1, 2, 64)] + [dict(FULL, tolerance=t) for t in (0, 1 << 20)]


def without_direct_links(g) -> dict:
    """the graph with every entry e -> join[e] taken out of the link lists"""
    lo, to, jn = g["link_off"].tolist(), g["link_to"].tolist(), g["join"].tolist()
    link_off, link_to = _csr([[y for y in to[lo[a]:lo[a + 1]] if y != jn[a]] for a in range(2 * g["U"])])
    return dict(g, link_off=link_off, link_to=link_to, E=len(link_to))
