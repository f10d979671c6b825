"""Test-side restatement of the repeat resolution (a helper, not a conftest): the transitions of threaded sequences through every unitig,
weak-link removal, repeat splitting and the resolved unitig set, sequentially, in plain Python. It restates the contract above the
aix_thread_pairs_dev / aix_graph_resolve_* declarations of include/aindex_hip.h:

  pairs(g, steps, pair_support=None)                 -> (pair_support uint64[16 U], n_pairs); ValueError on a violation
  mark(g, link_support, pair_support, min_link_support, min_pair_support, max_pair_noise)
                                                     -> {"link_remove" uint8[E], "copies" uint8[U], n_links_removed, n_split, n_copies_added}
  layout(g, link_remove, copies)                     -> {"copy_base" uint32[U], U, total_bases, E}
  emit(g, link_remove, copies, pair_support, min_pair_support)
                                                     -> G_r: the eight arrays of a unitig set, "unitig_origin" uint32[U'], U, E
  resolve(g, link_support, pair_support, ...)        -> mark, layout and emit as one dict

g holds the eight arrays of a unitig set (graph_clean_ref.graph); steps is the dict of seqthread_ref.thread. One link, one unitig, one
step at a time; all arithmetic in Python integers.
"""
import numpy as np

K = 23
NONE32 = 0xFFFFFFFF
NO_LINK = (1 << 64) - 1
BROKEN = (1 << 64) - 2
MAX_U = (1 << 31) - 4
M64 = (1 << 64) - 1
GRAPH_KEYS = ("offsets", "bases", "circular", "tf_sum", "tf_min", "tf_max", "link_off", "link_to")


def _lists(g):
    return [int(v) for v in g["offsets"]], [int(v) for v in g["link_off"]], [int(v) for v in g["link_to"]], [int(v) for v in g["circular"]]


def _check_link_off(lo, U, E):
    if len(lo) != 2 * U + 1 or lo[0] != 0 or lo[-1] != E or E > 8 * U:
        raise ValueError("link_off")
    for e in range(2 * U):
        if lo[e + 1] < lo[e] or lo[e + 1] - lo[e] > 4:
            raise ValueError("link_off")


def find(lo, to, e, t):
    """the first index in the list of end e whose word is t, or None"""
    return next((j for j in range(lo[e], lo[e + 1]) if to[j] == t), None)


def validate(g):
    """the unitig-set validation of the cleaning block, duality of every link included -> (off, lo, to, circ, src, dual)"""
    off, lo, to, circ = _lists(g)
    U, E = len(off) - 1, len(to)
    if U > MAX_U:
        raise OverflowError("U")
    _check_link_off(lo, U, E)
    if any(off[u + 1] < off[u] + K for u in range(U)):
        raise ValueError("offsets")
    src, dual = [0] * E, [0] * E
    for e in range(2 * U):
        for j in range(lo[e], lo[e + 1]):
            t = to[j]
            if t >= 2 * U or circ[e >> 1] or circ[t >> 1]:
                raise ValueError("a link word")
            src[j] = e
    for j in range(E):
        d = find(lo, to, to[j] ^ 1, src[j] ^ 1)
        if d is None:
            raise ValueError("a link without its dual")
        dual[j] = d
    return off, lo, to, circ, src, dual


def pairs(g, steps, pair_support=None):
    lo, to = [int(v) for v in g["link_off"]], [int(v) for v in g["link_to"]]
    U, E = len(g["offsets"]) - 1, len(to)
    _check_link_off(lo, U, E)
    su, sf, sl = [int(v) for v in steps["step_unitig"]], [int(v) for v in steps["step_flag"]], [int(v) for v in steps["step_link"]]
    T = len(su)
    out = [0] * (16 * U) if pair_support is None else [int(v) for v in pair_support]
    assert len(out) == 16 * U
    if any(u >= U for u in su) or any(l >= E and l not in (NO_LINK, BROKEN) for l in sl) or (T and sl[0] < E):
        raise ValueError("steps")
    adds = []
    for i in range(1, T - 1):
        a, b = sl[i], sl[i + 1]
        if a >= E or b >= E:
            continue
        u, s = su[i], sf[i] & 1
        e_prev, e = 2 * su[i - 1] + (sf[i - 1] & 1), 2 * u + s
        if not lo[e_prev] <= a < lo[e_prev + 1] or to[a] != e or not lo[e] <= b < lo[e + 1]:
            raise ValueError("a transition that is none of this graph")
        d = find(lo, to, e ^ 1, e_prev ^ 1)
        if d is None:
            raise ValueError("a link without its dual")
        x, y = (b - lo[2 * u], d - lo[2 * u + 1]) if s == 0 else (d - lo[2 * u], b - lo[2 * u + 1])
        adds.append(16 * u + 4 * x + y)
    for c in adds:                                                 # validated first, written second
        out[c] = (out[c] + 1) & M64
    return np.array(out, dtype=np.uint64), len(adds)


def _matching(lo, pair, keep, u, min_pair, max_noise):
    """(A, B, match) of unitig u over its surviving links: local indices A at end 2 u, B at end 2 u + 1, match[x] = its one strong y.
    match is None when the cells of A x B are no perfect matching of strong cells over noise (max_noise None: noise is not checked)."""
    A = [j - lo[2 * u] for j in range(lo[2 * u], lo[2 * u + 1]) if keep[j]]
    B = [j - lo[2 * u + 1] for j in range(lo[2 * u + 1], lo[2 * u + 2]) if keep[j]]
    cell = lambda x, y: pair[16 * u + 4 * x + y]
    if len(A) != len(B) or len(A) < 2:
        return A, B, None
    if max_noise is not None and any(max_noise < cell(x, y) < min_pair for x in A for y in B):
        return A, B, None
    match = {}
    for x in A:
        strong = [y for y in B if cell(x, y) >= min_pair]
        if len(strong) != 1:
            return A, B, None
        match[x] = strong[0]
    if sorted(match.values()) != B:
        return A, B, None
    return A, B, match


def mark(g, link_support=None, pair_support=None, min_link_support=2, min_pair_support=2, max_pair_noise=0):
    off, lo, to, circ, src, dual = validate(g)
    U, E = len(off) - 1, len(to)
    weak_on = link_support is not None and min_link_support > 0
    split_on = pair_support is not None and min_pair_support > 0
    sup = [int(v) for v in link_support] if link_support is not None else None
    if sup is not None and (len(sup) != E or any(sup[j] != sup[dual[j]] for j in range(E))):
        raise ValueError("link_support is not symmetric")
    if split_on and max_pair_noise >= min_pair_support:
        raise ValueError("max_pair_noise")
    weak = [weak_on and sup[j] < min_link_support for j in range(E)]
    firm = [any(not weak[j] for j in range(lo[e], lo[e + 1])) for e in range(2 * U)]    # the end has a link that is not weak
    remove = [1 if weak[j] and (firm[src[j]] or firm[to[j] ^ 1]) else 0 for j in range(E)]
    keep = [not r for r in remove]
    copies = [1] * U
    if split_on:
        pair = [int(v) for v in pair_support]
        assert len(pair) == 16 * U
        for u in range(U):
            if circ[u]:
                continue
            if any(keep[j] and to[j] >> 1 == u for j in range(lo[2 * u], lo[2 * u + 2])):
                continue                                           # a hairpin or a tandem self-link
            A, B, match = _matching(lo, pair, keep, u, min_pair_support, max_pair_noise)
            if match is not None:
                copies[u] = len(A)
    return {"link_remove": np.array(remove, dtype=np.uint8), "copies": np.array(copies, dtype=np.uint8), "n_links_removed": sum(remove),
            "n_split": sum(c > 1 for c in copies), "n_copies_added": sum(c - 1 for c in copies)}


def layout(g, link_remove, copies):
    off = [int(v) for v in g["offsets"]]
    U, E = len(off) - 1, len(g["link_to"])
    cp = [int(c) for c in copies]
    if any(not 1 <= c <= 4 for c in cp) or any(off[u + 1] < off[u] + K for u in range(U)):
        raise ValueError("copies")
    base, at, total = [NONE32] * U, U, off[U]
    for u in range(U):
        if cp[u] > 1:
            base[u] = at
            at += cp[u] - 1
            total += (cp[u] - 1) * (off[u + 1] - off[u])
    if at > MAX_U:
        raise OverflowError("U'")
    return {"copy_base": np.array(base, dtype=np.uint32), "U": at, "total_bases": total, "E": E - sum(1 for r in link_remove if r)}


def emit(g, link_remove, copies, pair_support=None, min_pair_support=2):
    off, lo, to, circ, src, dual = validate(g)
    U, E = len(off) - 1, len(to)
    keep = [not int(r) for r in link_remove]
    if any(keep[j] != keep[dual[j]] for j in range(E)):
        raise ValueError("link_remove is not symmetric")
    lay = layout(g, link_remove, copies)
    base, cp = [int(v) for v in lay["copy_base"]], [int(c) for c in copies]
    pair = [int(v) for v in pair_support] if pair_support is not None else None
    A, match = {}, {}
    for u in range(U):
        if cp[u] == 1:
            continue
        if pair is None or min_pair_support == 0 or circ[u] or any(keep[j] and to[j] >> 1 == u for j in range(lo[2 * u], lo[2 * u + 2])):
            raise ValueError("a split that the arrays do not support")
        A[u], _, match[u] = _matching(lo, pair, keep, u, min_pair_support, None)
        if match[u] is None or len(A[u]) != cp[u]:
            raise ValueError("a split that the arrays do not support")

    def rank_of(j):
        """the copy of unitig src[j] >> 1 that owns link j"""
        e = src[j]
        u = e >> 1
        if cp[u] == 1:
            return 0
        if e & 1 == 0:
            return A[u].index(j - lo[e])
        return next(r for r, x in enumerate(A[u]) if match[u][x] == j - lo[e])

    ident = lambda u, r: u if r == 0 else base[u] + r - 1
    U2 = lay["U"]
    origin = list(range(U)) + [0] * (U2 - U)
    rank = [0] * U2
    for u in range(U):
        for r in range(1, cp[u]):
            origin[ident(u, r)], rank[ident(u, r)] = u, r
    text = g["bases"].tobytes()
    res = {"U": U2, "offsets": np.zeros(U2 + 1, np.uint64), "unitig_origin": np.array(origin, dtype=np.uint32)}
    for k in ("circular", "tf_min", "tf_max"):
        res[k] = np.array([g[k][origin[i]] for i in range(U2)], dtype=g[k].dtype)
    tf = [int(g["tf_sum"][origin[i]]) for i in range(U2)]
    for u in A:                                                    # the abundance follows the strong cells
        p = [pair[16 * u + 4 * x + match[u][x]] for x in A[u]]
        rest = tf[u]
        for r in range(1, cp[u]):
            tf[ident(u, r)] = tf[u] * p[r] // sum(p)
            rest -= tf[ident(u, r)]
        tf[u] = rest
    res["tf_sum"] = np.array(tf, dtype=np.uint64)
    strings = [text[off[origin[i]]:off[origin[i] + 1]] for i in range(U2)]
    res["offsets"][1:] = np.cumsum([len(s) for s in strings]) if U2 else []
    res["bases"] = np.frombuffer(b"".join(strings), dtype=np.uint8).copy()
    link_off, link_to = [0], []
    for i in range(U2):
        u, r = origin[i], rank[i]
        for side in (0, 1):
            e = 2 * u + side
            mine = [j for j in range(lo[e], lo[e + 1]) if keep[j] and rank_of(j) == r]
            assert cp[u] == 1 or len(mine) == 1
            for j in mine:
                t = to[j]
                link_to.append(2 * ident(t >> 1, rank_of(dual[j])) + (t & 1))
            link_off.append(len(link_to))
    res["link_off"], res["link_to"] = np.array(link_off, dtype=np.uint64), np.array(link_to, dtype=np.uint32)
    res["E"] = len(link_to)
    assert res["E"] == lay["E"] and len(res["bases"]) == lay["total_bases"]
    res["copy_base"] = lay["copy_base"]
    return res


def resolve(g, link_support=None, pair_support=None, min_link_support=2, min_pair_support=2, max_pair_noise=0):
    m = mark(g, link_support, pair_support, min_link_support, min_pair_support, max_pair_noise)
    res = emit(g, m["link_remove"], m["copies"], pair_support, min_pair_support)
    res.update(m)
    return res
