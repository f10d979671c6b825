"""Array-level inputs of the graph cleaning that no index can produce (a helper, not a conftest). The contract above the aix_graph_*
declarations of include/aindex_hip.h is written for arrays: a unitig set is valid whether or not it is a compaction. Every graph that
unitigs_t + unitig_links_t return is one, so contigs of many short members, equal first 23-mers, products beyond 64 bits and positions
beyond 2^31 never come out of an index. This module makes them; tests/graph_clean_ref.py and tests/graph_clean_check.py judge them.

  shred(g, rng, p_cut)   the inverse of the compaction on the test side: every unitig of m k-mers is cut at each of its m - 1 inner
                         boundaries with probability p_cut; the piece over k-mers [a, b) has the bases s[a : b + 22], is stored
                         reverse-complemented (GR.rc_bytes) with probability 1/2 and gets its id by a random permutation. Compacting
                         a shred under the zero mask gives back g, up to the rotation of circles (GR.canonical_form).
      The link rule. For piece i with id_i and flip f_i let R(i) = 2 id_i + f_i (the end that lies on the right in the spelling of g, and
      also the link word that enters the piece in the direction of g) and L(i) = 2 id_i + 1 - f_i.
        consecutive pieces: R(i) -> R(i + 1) and the dual L(i + 1) -> L(i);
        a circular unitig is kept whole with probability 1/4 and always when m = 1; else its pieces are linear and the last links to the
        first: R(last) -> R(first), L(first) -> L(last) (one piece of m >= 2: the closing link u+ -> u+ of the contract);
        a link e -> t of g, t = 2 v + r: the source end is R(last piece of u) for e = 2 u and L(first piece of u) for e = 2 u + 1; the
        word is R(first piece of v) for r = 0 and L(last piece of v) for r = 1; the order of the links of an end is kept.
      tf_min / tf_max are copied to every piece; tf_sum is split as tot // m * (b - a), the remainder on the first piece.
  union(a, b)            the disjoint union; of two shreds of one graph it gives every contig a twin with the same first 23-mer
  emit_coverage(g, out)  replays the chunking of k_gc_emit (16 output bytes per lane) from the map of a compaction: which member counts per
                         chunk, (segment length, orientation), (source address mod 8, orientation) occur, and in which orientations the
                         16-byte source window reaches past the end of the input bases
  make_mark_graph(seed)  link structures for aix_graph_mark_dev (mark reads no bases: offsets, circular, tf_sum, link_off, link_to only):
                         forks and bubbles with lengths around every threshold and abundances up to 2^64, so that a comparison that is
                         not exact in 128 bits decides differently (MUTANTS)
"""
import functools

import numpy as np

import graph_cases as G
import graph_clean_ref as GR
import unitig_links_cases as LC
import unitig_links_ref as RL
import unitigs_cases as UC
import unitigs_ref as R

K = 23
NONE32 = GR.NONE32


# ---- shred and union -------------------------------------------------------------------------------------------------------------------
def shred(g: dict, rng, p_cut: float, last_reversed_first: bool = False) -> dict:
    """last_reversed_first: the first piece of one linear unitig is stored reversed and gets the largest id, so it is stored last: under
    the zero mask it is the first member of its contig, reversed, and the emission's source window for the first bytes of that contig
    reaches past the end of `bases` (a reversed member that is not the first is read from at least 22 + 1 bytes before its end, so its
    16-byte window never does)."""
    U = g["U"]
    off, lo, to = GR._lists(g)
    text = g["bases"].tobytes()
    circ = g["circular"].tolist()
    pieces, first, last, whole = [], [0] * U, [0] * U, [False] * U
    for u in range(U):
        m = off[u + 1] - off[u] - (K - 1)
        whole[u] = bool(circ[u]) and (m == 1 or rng.random() < 0.25)
        cuts = [] if whole[u] else (np.nonzero(rng.random(m - 1) < p_cut)[0] + 1).tolist()
        bounds = [0] + cuts + [m]
        first[u] = len(pieces)
        pieces += [(u, a, b) for a, b in zip(bounds[:-1], bounds[1:])]
        last[u] = len(pieces) - 1
    P = len(pieces)
    flip = (rng.random(P) < 0.5).astype(np.int64).tolist()
    ids = rng.permutation(P).tolist()
    if last_reversed_first:
        linear = [u for u in range(U) if not circ[u] and last[u] > first[u]]   # of two pieces or more
        i = first[linear[int(rng.integers(0, len(linear)))]]
        j = ids.index(P - 1)
        ids[i], ids[j] = ids[j], ids[i]
        flip[i] = 1
    Rw = lambda i: 2 * ids[i] + flip[i]
    Lw = lambda i: 2 * ids[i] + 1 - flip[i]
    links = [[] for _ in range(2 * P)]
    for u in range(U):
        for i in range(first[u], last[u]):
            links[Rw(i)].append(Rw(i + 1))
            links[Lw(i + 1)].append(Lw(i))
        if circ[u] and not whole[u]:
            links[Rw(last[u])].append(Rw(first[u]))
            links[Lw(first[u])].append(Lw(last[u]))
        for side in (0, 1):
            e = 2 * u + side
            src = Rw(last[u]) if side == 0 else Lw(first[u])
            for t in to[lo[e]:lo[e + 1]]:
                v = t >> 1
                links[src].append(Rw(first[v]) if t & 1 == 0 else Lw(last[v]))
    at = [0] * P
    for i, j in enumerate(ids):
        at[j] = i
    out = {"U": P, "offsets": np.zeros(P + 1, np.uint64), "circular": np.zeros(P, np.uint8), "tf_sum": np.zeros(P, np.uint64),
           "tf_min": np.zeros(P, np.uint32), "tf_max": np.zeros(P, np.uint32), "piece_of": np.zeros(P, np.int64)}
    strings, total = [], 0
    for j in range(P):
        i = at[j]
        u, a, b = pieces[i]
        m = off[u + 1] - off[u] - (K - 1)
        s = text[off[u] + a: off[u] + b + K - 1]
        strings.append(GR.rc_bytes(s) if flip[i] else s)
        total += len(s)
        tot = int(g["tf_sum"][u])
        out["offsets"][j + 1] = total
        out["circular"][j] = whole[u]
        out["tf_sum"][j] = tot // m * (b - a) + (tot - tot // m * m if a == 0 else 0)
        out["tf_min"][j], out["tf_max"][j] = g["tf_min"][u], g["tf_max"][u]
        out["piece_of"][j] = u
    out["bases"] = np.frombuffer(b"".join(strings), dtype=np.uint8).copy()
    out["link_off"] = np.concatenate([[0], np.cumsum([len(l) for l in links])]).astype(np.uint64)
    out["link_to"] = np.array([t for l in links for t in l], dtype=np.uint32)
    out["E"] = int(out["link_to"].shape[0])
    return out


def union(a: dict, b: dict) -> dict:
    """the disjoint union of two unitig sets: the ids, ends, link words and offsets of b are shifted behind those of a"""
    out = {"U": a["U"] + b["U"], "E": a["E"] + b["E"]}
    out["offsets"] = np.concatenate([a["offsets"], b["offsets"][1:] + a["offsets"][-1]])
    out["link_off"] = np.concatenate([a["link_off"], b["link_off"][1:] + a["link_off"][-1]])
    out["link_to"] = np.concatenate([a["link_to"], b["link_to"] + np.uint32(2 * a["U"])])
    for k in ("bases", "circular", "tf_sum", "tf_min", "tf_max"):
        out[k] = np.concatenate([a[k], b[k]])
    return out


# ---- the chunking of the emission, replayed from a map ---------------------------------------------------------------------------------
def emit_coverage(g: dict, out: dict) -> dict:
    """Output byte o belongs to chunk o >> 4 and to the member that contributes it (a member contributes its oriented spelling from
    byte 0, the first of its contig, or from byte 22). A segment is a maximal run of one member within one chunk: n bytes from index i0
    of the oriented spelling, loaded as 16 bytes from src = in_lo + i0 forwards and src = in_lo + len - i0 - n reversed.
    -> {"members": set of segment counts per chunk, "length": {(n, reversed)}, "shift": {(src & 7, reversed)},
        "past_end": {reversed: a window with src + 16 > offsets[U]}}"""
    off, noff = g["offsets"].astype(np.int64), out["offsets"].astype(np.int64)
    mem = np.nonzero(out["unitig_contig"] != NONE32)[0]
    c, pos = out["unitig_contig"][mem].astype(np.int64), out["unitig_pos"][mem].astype(np.int64)
    order = np.lexsort((pos, c))
    mem, c, pos = mem[order], c[order], pos[order]
    rev = (out["unitig_flag"][mem] & 1).astype(np.int64)
    total, total_in = int(noff[-1]), int(off[-1])
    if total == 0:
        return {"members": set(), "length": set(), "shift": set(), "past_end": set()}
    begin = noff[c] + pos + np.where(pos > 0, K - 1, 0)
    n_bytes = np.append(begin[1:], total) - begin
    assert begin[0] == 0 and (n_bytes > 0).all()
    j = np.repeat(np.arange(mem.shape[0]), n_bytes)
    start = np.ones(total, bool)
    start[1:] = (j[1:] != j[:-1]) | (np.arange(1, total) % 16 == 0)
    seg = np.nonzero(start)[0]
    n = np.append(seg[1:], total) - seg
    sj = j[seg]
    i0 = np.where(pos[sj] > 0, K - 1, 0) + seg - begin[sj]
    in_lo = off[mem[sj]]
    ln = off[mem[sj] + 1] - in_lo
    r = rev[sj]
    assert (i0 + n <= ln).all()
    src = np.where(r == 1, in_lo + ln - i0 - n, in_lo + i0)
    return {"members": set(np.bincount(seg >> 4).tolist()) - {0}, "length": set(zip(n.tolist(), r.tolist())),
            "shift": set(zip((src & 7).tolist(), r.tolist())), "past_end": set(r[src + 16 > total_in].tolist())}


def merge_coverage(items) -> dict:
    out = {"members": set(), "length": set(), "shift": set(), "past_end": set()}
    for cov in items:
        for k in out:
            out[k] |= cov[k]
    return out


# ---- the inputs the GPU tests use, and their references (computed once per process) -----------------------------------------------------
SHRED_INPUTS = (0, 3, "two_stems", "lollipop", "many_circles", "opened_circle", "hairpin_ends", "bubble_tip_cutoff")
P_CUTS = (0.1, 0.5, 1.0)
FORCED = (0, 0.5)                                                  # this shred is made with last_reversed_first
MASKS = ("zero", "10 %", "50 %", "mark")
UNION_OF = ((0, 0.5), (0, 0.1))                                    # the two shreds of the union case
SHRED_SEED = 20261


def graph_of_codes(codes, tfs, cutoff=0) -> dict:
    un = R.unitigs(codes, tfs, cutoff)
    return GR.graph(un, RL.links(codes, tfs, cutoff, un))


@functools.lru_cache(maxsize=None)
def planted_cases() -> dict:
    """name -> Case: every topology case, every link case, and the ring with two stems of test_graph_clean_cpu.py"""
    import test_graph_clean_cpu as TC
    every = dict(UC.topology_cases())
    every.update(LC.link_cases())
    codes, tfs = TC._lollipop_two_stems()
    every["two_stems"] = UC.Case(codes, tfs, None)
    return every


@functools.lru_cache(maxsize=None)
def source_graph(name) -> dict:
    """graph case `name` (an int seed of graph_cases.py) or planted case `name`, at cutoff 0"""
    if isinstance(name, int):
        codes, tfs = G.make_graph_case(name)[:2]
    else:
        case = planted_cases()[name]
        codes, tfs = case.codes, case.tfs
    return graph_of_codes(codes, tfs, 0)


@functools.lru_cache(maxsize=None)
def shred_of(name, p_cut) -> dict:
    tag = SHRED_INPUTS.index(name) if name in SHRED_INPUTS else 100 + sorted(planted_cases()).index(name)
    rng = np.random.default_rng((SHRED_SEED, tag, int(round(p_cut * 100))))
    return shred(source_graph(name), rng, p_cut, last_reversed_first=(name, p_cut) == FORCED)


@functools.lru_cache(maxsize=None)
def union_case() -> dict:
    return union(*[shred_of(*x) for x in UNION_OF])


def _input(key) -> dict:
    return union_case() if key == "union" else shred_of(*key)


@functools.lru_cache(maxsize=None)
def mask_of(key, mask: str) -> np.ndarray:
    """key: (name, p_cut) or "union"."""
    g = _input(key)
    if mask == "mark":
        return GR.mark(g, 46, 46)
    if mask == "zero":
        return np.zeros(g["U"], np.uint8)
    rng = np.random.default_rng((SHRED_SEED, g["U"], MASKS.index(mask)))
    return (rng.random(g["U"]) < {"10 %": 0.1, "50 %": 0.5}[mask]).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def reference(key, mask: str) -> dict:
    return GR.compact(_input(key), mask_of(key, mask))


@functools.lru_cache(maxsize=None)
def reference_clean(key, rounds: int = 3):
    return GR.clean(_input(key), 46, 46, rounds)


# ---- link structures for the mark ------------------------------------------------------------------------------------------------------
MARK_M = (1, 2, 3, 11, 45, 46, 47, 1000, 32766, 32767, 32768, 10 ** 6)
MARK_TF = (1, 3, 1000, 2 ** 32 - 1, 2 ** 32, 2 ** 53, 2 ** 60, 3 * 2 ** 60, 2 ** 62, 2 ** 63, 2 ** 64 - 40000)
MARK_THRESHOLDS = ((46, 46), (32767, 32767), (1, 0), (0, 1), (45, 47))
MARK_SEEDS = (0, 1, 2, 3)


@functools.lru_cache(maxsize=None)
def make_mark_graph(seed: int, motifs: int = 300) -> dict:
    """About `motifs` forks and bubbles under a random id permutation, and five circular unitigs.
    Fork: a hub end with 1 .. 4 siblings, each entered forwards or backwards; one sibling in four continues into another unitig and is
    no tip candidate. Bubble: a source end, two arms in either orientation, a sink. The siblings of a motif share one length m four
    times out of five, and one abundance (plus 0 .. 2) half of the time: equal and nearly equal means are common."""
    rng = np.random.default_rng((20262, seed))
    m, tf, links = [], [], {}
    bit = lambda: int(rng.integers(0, 2))
    draw_m = lambda: MARK_M[int(rng.integers(0, len(MARK_M)))]
    draw_tf = lambda: MARK_TF[int(rng.integers(0, len(MARK_TF)))]

    def new(mm, t):
        m.append(mm)
        tf.append(t + int(rng.integers(0, 3)))
        return len(m) - 1

    def link(e, t):                                                # e -> t and its dual (no motif plants a self-dual link)
        links.setdefault(e, []).append(t)
        links.setdefault(t ^ 1, []).append(e ^ 1)

    def siblings(k):
        mm, t = draw_m(), draw_tf()
        return [new(mm if rng.random() < 0.8 else draw_m(), t if rng.random() < 0.5 else draw_tf()) for _ in range(k)]

    for _ in range(motifs):
        if rng.random() < 0.6:
            hub = 2 * new(draw_m(), draw_tf()) + bit()
            for s in siblings(int(rng.integers(1, 5))):
                w = 2 * s + bit()
                link(hub, w)
                if rng.random() < 0.25:
                    link(w, 2 * new(draw_m(), draw_tf()) + bit())   # the far end of s, entered as w, is the end w
        else:
            source, sink = 2 * new(draw_m(), draw_tf()) + bit(), 2 * new(draw_m(), draw_tf()) + bit()
            for s in siblings(2):
                w = 2 * s + bit()
                link(source, w)
                link(w, sink)
    ring = [new(draw_m(), draw_tf()) for _ in range(5)]
    U = len(m)
    perm = rng.permutation(U)
    g = {"U": U, "circular": np.zeros(U, np.uint8), "tf_sum": np.zeros(U, np.uint64)}
    length = np.zeros(U, np.int64)
    length[perm] = np.array(m) + (K - 1)
    g["offsets"] = np.concatenate([[0], np.cumsum(length)]).astype(np.uint64)
    g["circular"][perm[ring]] = 1
    for i in range(U):
        g["tf_sum"][perm[i]] = tf[i]
    word = lambda t: 2 * int(perm[t >> 1]) + (t & 1)
    ends = [[] for _ in range(2 * U)]
    for e, l in links.items():
        ends[word(e)] = [word(t) for t in l]
    g["link_off"] = np.concatenate([[0], np.cumsum([len(l) for l in ends])]).astype(np.uint64)
    g["link_to"] = np.array([t for l in ends for t in l], dtype=np.uint32)
    g["E"] = int(g["link_to"].shape[0])
    return g


def _products(g, w, u):
    off = g["offsets"]
    mw, mu = int(off[w + 1]) - int(off[w]) - (K - 1), int(off[u + 1]) - int(off[u]) - (K - 1)
    return int(g["tf_sum"][w]), mw, int(g["tf_sum"][u]), mu


def _mod64(g, w, u):
    tw, mw, tu, mu = _products(g, w, u)
    a, b = tw * mu % 2 ** 64, tu * mw % 2 ** 64
    return a > b or (a == b and w < u)


def _double(g, w, u):
    tw, mw, tu, mu = _products(g, w, u)
    a, b = float(tw) * float(mu), float(tu) * float(mw)
    return a > b or (a == b and w < u)


def _floor_means(g, w, u):
    tw, mw, tu, mu = _products(g, w, u)
    a, b = tw // mw, tu // mu
    return a > b or (a == b and w < u)


def _larger_id(g, w, u):
    tw, mw, tu, mu = _products(g, w, u)
    a, b = tw * mu, tu * mw
    return a > b or (a == b and w > u)


MUTANTS = {"products mod 2^64": _mod64, "products in double": _double, "floor means": _floor_means, "ties to the larger id": _larger_id}


def mark_with(g: dict, outranks, tip: int, bub: int) -> np.ndarray:
    """GR.mark with another `outranks`"""
    saved = GR.outranks
    GR.outranks = outranks
    try:
        return GR.mark(g, tip, bub)
    finally:
        GR.outranks = saved


# (tips, arms) of GR.mark(make_mark_graph(seed), tip, bub), per seed in the order of MARK_THRESHOLDS
MARK_COUNTS = {0: ((127, 44), (222, 86), (17, 0), (0, 12), (104, 56)),
               1: ((117, 43), (195, 90), (12, 0), (0, 5), (95, 53)),
               2: ((130, 48), (207, 98), (22, 0), (0, 5), (113, 64)),
               3: ((127, 46), (219, 89), (19, 0), (0, 7), (105, 54))}
