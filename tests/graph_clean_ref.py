"""Test-side restatement of the graph cleaning (a helper, not a conftest): tips, bubble arms and the recompaction of a unitig graph into
contigs, sequentially, over the dict answers of unitigs_ref.unitigs and unitig_links_ref.links. It restates the contract above the
aix_graph_* declarations of include/aindex_hip.h:

  graph(un, lk)        the nine arrays of a unitig set G as one dict (U, E, offsets, bases, circular, tf_sum, tf_min, tf_max, link_off, link_to)
  mark(g, tip, bub)    remove uint8[U]: 1 = clipped tip, 2 = weaker bubble arm; every decision from the input graph alone
  compact(g, remove)   G' in the format of G, plus unitig_contig uint32[U], unitig_pos uint64[U], unitig_flag uint8[U], C, E, n_circular,
                       and "strings" / "chains" (the members of every contig as (unitig, reversed)) for the tests
  clean(g, tip, bub, rounds)  mark then compact until nothing is removed or `rounds` is reached -> (G', rounds done)

It walks left and right from every surviving unitig in ascending order; nothing here ranks lists or jumps pointers.
"""
import numpy as np

K = 23
NONE32 = 0xFFFFFFFF
MAX_THRESHOLD = 32767
GRAPH_KEYS = ("offsets", "bases", "circular", "tf_sum", "tf_min", "tf_max", "link_off", "link_to")
MAP_KEYS = ("unitig_contig", "unitig_pos", "unitig_flag")
_DTYPES = {"offsets": np.uint64, "bases": np.uint8, "circular": np.uint8, "tf_sum": np.uint64, "tf_min": np.uint32, "tf_max": np.uint32,
           "link_off": np.uint64, "link_to": np.uint32}


def base_code(c: int) -> int:
    """two bits of an ASCII base: A 0, C 1, G 2, T 3 (any other byte: whatever the formula gives)"""
    return ((c >> 1) ^ (c >> 2)) & 3


def comp_byte(c: int) -> int:
    """A <-> T, C <-> G as the emission does it: bit 1 of the byte tells C / G from A / T"""
    return c ^ (0x04 if c & 2 else 0x15)


def rc_bytes(b: bytes) -> bytes:
    return bytes(comp_byte(c) for c in reversed(b))


def code23(b: bytes) -> int:
    x = 0
    for c in b[:K]:
        x = (x << 2) | base_code(c)
    return x


def graph(un: dict, lk: dict) -> dict:
    g = {k: np.ascontiguousarray(np.asarray(un[k] if k in un else lk[k]), dtype=_DTYPES[k]) for k in GRAPH_KEYS}
    g["U"], g["E"] = int(g["offsets"].shape[0]) - 1, int(g["link_to"].shape[0])
    if "bubble_mate" in lk:
        g["bubble_mate"] = np.asarray(lk["bubble_mate"], dtype=np.uint32)
    return g


def _lists(g):
    off = [int(v) for v in g["offsets"]]
    lo = [int(v) for v in g["link_off"]]
    to = [int(v) for v in g["link_to"]]
    return off, lo, to


def bubbles(U, link_off, link_to) -> list:
    """bubble_mate by the literal rule of the unitig-graph block of the header"""
    off, to = [int(v) for v in link_off], [int(v) for v in link_to]
    deg = lambda e: off[e + 1] - off[e]
    tgt = lambda e: to[off[e]:off[e + 1]]
    mate = [NONE32] * U
    for u in range(U):
        if deg(2 * u) != 1 or deg(2 * u + 1) != 1:
            continue
        tR, tL = tgt(2 * u)[0], tgt(2 * u + 1)[0]
        f = tL ^ 1
        if deg(f) != 2 or 2 * u not in tgt(f):
            continue
        x = [t for t in tgt(f) if t != 2 * u]
        if len(x) != 1 or x[0] >> 1 == u:
            continue
        x = x[0]
        if deg(tR ^ 1) != 2:
            continue
        if deg(x) == 1 and tgt(x)[0] == tR and deg(x ^ 1) == 1 and tgt(x ^ 1)[0] == tL:
            mate[u] = x >> 1
    return mate


def outranks(g, w: int, u: int) -> bool:
    """mean(w) > mean(u), or equal means and w < u; exact in integers"""
    off = g["offsets"]
    mw, mu = int(off[w + 1]) - int(off[w]) - (K - 1), int(off[u + 1]) - int(off[u]) - (K - 1)
    a, b = int(g["tf_sum"][w]) * mu, int(g["tf_sum"][u]) * mw
    return a > b or (a == b and w < u)


def mark(g: dict, tip_max_kmers: int = 46, bubble_max_kmers: int = 46, bubble_mate=None) -> np.ndarray:
    assert 0 <= tip_max_kmers <= MAX_THRESHOLD and 0 <= bubble_max_kmers <= MAX_THRESHOLD
    U = g["U"]
    off, lo, to = _lists(g)
    circ = g["circular"].tolist()
    m = [off[u + 1] - off[u] - (K - 1) for u in range(U)]
    deg = lambda e: lo[e + 1] - lo[e]
    tgt = lambda e: to[lo[e]:lo[e + 1]]
    mate = [int(v) for v in (bubble_mate if bubble_mate is not None else bubbles(U, lo, to))]

    def attached(u):
        """the linked end of tip candidate u, or None"""
        if circ[u] or tip_max_kmers == 0 or m[u] > tip_max_kmers:
            return None
        d0, d1 = deg(2 * u), deg(2 * u + 1)
        if d0 == 0 and d1 == 1:
            return 2 * u + 1
        if d1 == 0 and d0 == 1:
            return 2 * u
        return None

    remove = np.zeros(U, np.uint8)
    for u in range(U):
        a = attached(u)
        if a is not None:
            f = tgt(a)[0] ^ 1
            for x in tgt(f):
                w = x >> 1
                if w != u and (attached(w) is None or outranks(g, w, u)):
                    remove[u] = 1
        w = mate[u]
        if bubble_max_kmers and w != NONE32 and m[u] <= bubble_max_kmers and m[w] <= bubble_max_kmers and outranks(g, w, u):
            assert remove[u] == 0
            remove[u] = 2
    return remove


def compact(g: dict, remove) -> dict:
    U = g["U"]
    off, lo, to = _lists(g)
    circ = g["circular"].tolist()
    text = g["bases"].tobytes()
    m = [off[u + 1] - off[u] - (K - 1) for u in range(U)]
    alive = [not r for r in np.asarray(remove).tolist()]
    assert len(alive) == U

    def surv(e):
        return [t for t in to[lo[e]:lo[e + 1]] if alive[e >> 1] and alive[t >> 1]]

    for e in range(2 * U):
        for t in surv(e):
            assert (e ^ 1) in surv(t ^ 1), "a surviving link without its dual"
            assert not circ[e >> 1] and not circ[t >> 1], "a link of a circular unitig"

    def merge(e):
        s = surv(e)
        if len(s) != 1 or len(surv(s[0] ^ 1)) != 1:
            return None
        if s[0] >> 1 == e >> 1 and not (s[0] == e and m[e >> 1] >= 2):   # a hairpin (u+ -> u-), or the self-loop of one k-mer
            return None
        return s[0]

    def oriented(u, f):
        s = text[off[u]:off[u + 1]]
        return rc_bytes(s) if f else s

    seen = [False] * U
    found = []                                                     # (first code, first member, chain, circular)
    for u in range(U):
        if not alive[u] or seen[u]:
            continue
        chain, circular = [(u, 0)], bool(circ[u])
        if not circular:
            e = 2 * u
            while merge(e) is not None:
                t = merge(e)
                if t >> 1 == u:                                     # back at the start: u is the smallest member of this cycle
                    assert t == 2 * u
                    circular = True
                    break
                chain.append((t >> 1, t & 1))
                e = t
            if not circular:
                e = 2 * u + 1
                while merge(e) is not None:
                    t = merge(e)
                    chain.insert(0, (t >> 1, (t & 1) ^ 1))
                    e = t
                other = [(v, f ^ 1) for v, f in reversed(chain)]
                ka = (code23(oriented(*chain[0])), chain[0][0])
                kb = (code23(oriented(*other[0])), other[0][0])
                if kb < ka:
                    chain = other
        for v, _ in chain:
            assert alive[v] and not seen[v]
            seen[v] = True
        found.append((code23(oriented(*chain[0])), chain[0][0], chain, circular))
    found.sort(key=lambda f: (f[0], f[1]))

    C = len(found)
    res = {"U": C, "C": C, "n_circular": sum(f[3] for f in found), "offsets": np.zeros(C + 1, np.uint64), "circular": np.zeros(C, np.uint8),
           "tf_sum": np.zeros(C, np.uint64), "tf_min": np.zeros(C, np.uint32), "tf_max": np.zeros(C, np.uint32),
           "unitig_contig": np.full(U, NONE32, np.uint32), "unitig_pos": np.zeros(U, np.uint64), "unitig_flag": np.zeros(U, np.uint8)}
    strings, at = [], 0
    for c, (_, _, chain, circular) in enumerate(found):
        s, pos = b"", 0
        for j, (v, f) in enumerate(chain):
            o = oriented(v, f)
            if j:
                assert s[-(K - 1):] == o[:K - 1], "members of a contig overlap by 22 bases"
            s += o if j == 0 else o[K - 1:]
            res["unitig_contig"][v], res["unitig_pos"][v] = c, pos
            res["unitig_flag"][v] = f | (2 if circular and not circ[v] else 0)   # bit 1: a merged cycle
            pos += m[v]
        members = [v for v, _ in chain]
        res["offsets"][c], res["circular"][c] = at, circular
        res["tf_sum"][c] = sum(int(g["tf_sum"][v]) for v in members)
        res["tf_min"][c] = min(int(g["tf_min"][v]) for v in members)
        res["tf_max"][c] = max(int(g["tf_max"][v]) for v in members)
        assert len(s) == pos + K - 1
        strings.append(s.decode("latin-1"))
        at += len(s)
    res["offsets"][C] = at
    res["bases"] = np.frombuffer("".join(strings).encode("latin-1"), dtype=np.uint8).copy()
    cid, flag = res["unitig_contig"].tolist(), res["unitig_flag"].tolist()
    link_off, link_to = [0], []
    for c, (_, _, chain, circular) in enumerate(found):
        for side in (0, 1):
            if not circular:
                v, f = chain[-1] if side == 0 else chain[0]
                port = 2 * v + (side ^ f)
                assert merge(port) is None
                link_to += [2 * cid[t >> 1] + ((t ^ flag[t >> 1]) & 1) for t in surv(port)]
            link_off.append(len(link_to))
    res["link_off"], res["link_to"] = np.array(link_off, dtype=np.uint64), np.array(link_to, dtype=np.uint32)
    res["E"] = len(link_to)
    res["bubble_mate"] = np.array(bubbles(C, link_off, link_to), dtype=np.uint32)
    res["strings"], res["chains"] = strings, [f[2] for f in found]
    return res


def clean(g: dict, tip_max_kmers: int = 46, bubble_max_kmers: int = 46, rounds: int = 1):
    done = 0
    while done < rounds:
        remove = mark(g, tip_max_kmers, bubble_max_kmers)
        if not remove.any():
            break
        g = compact(g, remove)
        done += 1
    return g, done


def canonical_form(g: dict) -> dict:
    """G up to the rotation and strand of circular unitigs and the id order that follows: every circular spelling is rotated / reversed to
    the one that starts at its smallest canonical 23-mer, read as that canonical k-mer (the rule of the compaction), ids are re-sorted by
    the first 23-mer and the link words renumbered. Circular unitigs have no links, so only ids move."""
    U = g["U"]
    off, lo, to = _lists(g)
    text = g["bases"].tobytes()
    rows = []
    for u in range(U):
        s = text[off[u]:off[u + 1]]
        flip = 0
        if g["circular"][u]:
            mm = len(s) - (K - 1)
            ring = s[:mm]
            best = None
            for strand, r in ((0, ring), (1, rc_bytes(ring))):
                dbl = r + r + r[:K]
                while len(dbl) < mm + K:
                    dbl += r
                for i in range(mm):
                    w = dbl[i:i + K]
                    if code23(w) <= code23(rc_bytes(w)):            # this window is the stored (canonical) k-mer
                        key = code23(w)
                        if best is None or key < best[0]:
                            best = (key, strand, i)
            _, strand, i = best
            r = ring if strand == 0 else rc_bytes(ring)
            rot = r[i:] + r[:i]
            s = (rot * ((K - 1) // mm + 2))[:mm + K - 1]
        rows.append((code23(s), u, s, flip))
    rows.sort(key=lambda r: (r[0], r[1]))
    new_id = {r[1]: i for i, r in enumerate(rows)}
    out = {"U": U, "offsets": np.zeros(U + 1, np.uint64), "strings": [r[2].decode("latin-1") for r in rows]}
    for k in ("circular", "tf_sum", "tf_min", "tf_max"):
        out[k] = np.array([g[k][r[1]] for r in rows], dtype=g[k].dtype)
    out["offsets"][1:] = np.cumsum([len(r[2]) for r in rows])
    link_off, link_to = [0], []
    for r in rows:
        for side in (0, 1):
            e = 2 * r[1] + side
            link_to += [2 * new_id[t >> 1] + (t & 1) for t in to[lo[e]:lo[e + 1]]]
            link_off.append(len(link_to))
    out["link_off"], out["link_to"] = np.array(link_off, dtype=np.uint64), np.array(link_to, dtype=np.uint32)
    out["E"] = len(link_to)
    return out
