"""Test-side restatement of the threading (a helper, not a conftest): the k-mer map through a compaction round, the node words, and the
path of every sequence through a unitig or contig graph with the support of its links, sequentially, in plain Python / numpy. It
restates the contract above the aix_graph_kidmap_dev / aix_thread_nodes_dev / aix_seq_thread* declarations of include/aindex_hip.h:

  kidmap(ku, kp, kf, offsets, unitig_contig, unitig_pos, unitig_flag)   -> (ku', kp', kf'); ValueError on a violation
  nodes(ku, kp, kf, offsets)                                            -> node uint64[n]: unitig << 33 | pos << 2 | flag, all ones = dead
  thread(kid_of, node, g, seqs, support=None)                           -> the seven arrays of aix_seq_thread_dev (+ "support" uint64[E])

kid_of is a dict canonical code -> kid; g holds offsets, circular, link_off, link_to (the arrays of unitigs_ref / unitig_links_ref /
graph_clean_ref). One window at a time, one sequence at a time; nothing here scans or compares neighbours in parallel.
"""
import numpy as np

import unitigs_ref as R

K = 23
NONE64 = (1 << 64) - 1
NONE32 = 0xFFFFFFFF
NO_LINK = (1 << 64) - 1
BROKEN = (1 << 64) - 2
DEAD = (1 << 64) - 1
MAX_U = (1 << 31) - 4
KEYS = ("seq_step_off", "step_unitig", "step_pos", "step_flag", "q_first", "q_last", "step_link")
DTYPES = (np.uint64, np.uint32, np.uint32, np.uint8, np.uint32, np.uint32, np.uint64)
_CODE = {65: 0, 67: 1, 71: 2, 84: 3}                               # upper-case A, C, G, T only


def _m(offsets, u):
    return int(offsets[u + 1]) - int(offsets[u]) - (K - 1)


def kidmap(kid_unitig, kid_pos, kid_flag, offsets, unitig_contig, unitig_pos, unitig_flag):
    n, U = len(kid_unitig), len(offsets) - 1
    ou, op, of = np.full(n, NONE64, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    for kid in range(n):
        u, p, f = int(kid_unitig[kid]), int(kid_pos[kid]), int(kid_flag[kid])
        if u == NONE64:
            continue
        if u >= U or int(offsets[u + 1]) < int(offsets[u]) + K or p >= _m(offsets, u):
            raise ValueError("a k-mer outside its unitig")
        c = int(unitig_contig[u])
        if c == NONE32:
            continue
        uf = int(unitig_flag[u])
        pos = int(unitig_pos[u]) + (_m(offsets, u) - 1 - p if uf & 1 else p)
        if c >= MAX_U or pos > 0xFFFFFFFF:
            raise ValueError("a contig id or a position that does not fit")
        ou[kid], op[kid], of[kid] = c, pos, ((f ^ uf) & 1) | ((f | uf) & 2)
    return ou, op, of


def nodes(kid_unitig, kid_pos, kid_flag, offsets):
    n, U = len(kid_unitig), len(offsets) - 1
    if U > MAX_U:
        raise OverflowError("U")
    out = np.full(n, DEAD, np.uint64)
    for kid in range(n):
        u, p = int(kid_unitig[kid]), int(kid_pos[kid])
        if u == NONE64:
            continue
        if u >= U or int(offsets[u + 1]) < int(offsets[u]) + K or p >= _m(offsets, u):
            raise ValueError("a k-mer outside its unitig")
        if p >= 1 << 31:
            raise OverflowError("pos")
        out[kid] = (u << 33) | (p << 2) | (int(kid_flag[kid]) & 3)
    return out


def unpack(word: int):
    """(unitig, pos, flag) of a node word, None for a dead one"""
    return None if word == DEAD else (word >> 33, (word >> 2) & 0x7FFFFFFF, word & 3)


def thread(kid_of: dict, node, g: dict, seqs, support=None) -> dict:
    node = [int(v) for v in node]
    off = [int(v) for v in g["offsets"]]
    circ = [int(v) for v in g["circular"]]
    lo = [int(v) for v in g["link_off"]]
    to = [int(v) for v in g["link_to"]]
    U, E = len(off) - 1, len(to)
    m = [off[u + 1] - off[u] - (K - 1) for u in range(U)]
    sup = None if support is None else [int(v) for v in support]

    def node_of(w: bytes):
        """(u, p, s) of a 23-byte window, or None"""
        x = 0
        for ch in w:
            if ch not in _CODE:
                return None
            x = (x << 2) | _CODE[ch]
        c = R.canon(x)
        kid = kid_of.get(c)
        if kid is None or node[kid] == DEAD:
            return None
        u, p, f = unpack(node[kid])
        return u, p, (f & 1) ^ (1 if x != c else 0)

    def follows(a, b):
        (u, p, s), (v, q, t) = a, b
        if u != v or s != t:
            return False
        frm, nxt = (q, p) if s else (p, q)                         # forwards in the spelling: frm -> nxt
        if nxt == frm + 1:
            return True
        return bool(circ[u]) and nxt == 0 and frm == m[u] - 1

    def find(e, t):
        if e >= len(lo) - 1:                                       # a foreign graph: every index is checked before it is used
            return BROKEN
        for j in range(lo[e], min(lo[e + 1], E)):
            if to[j] == t:
                return j
        return BROKEN

    def link_of(a, b):
        (u, p, s), (v, q, t) = a, b
        if p != (0 if s else m[u] - 1) or q != (m[v] - 1 if t else 0):
            return BROKEN
        e, w = 2 * u + s, 2 * v + t
        j = find(e, w)
        if j != BROKEN and sup is not None:
            sup[j] += 1
            d = find(w ^ 1, e ^ 1)
            if d != BROKEN and d != j:
                sup[d] += 1
        return j

    sso, rows = [0], []
    for s in seqs:
        s = bytes(s)
        prev = None
        for q in range(max(0, len(s) - (K - 1))):
            nd = node_of(s[q:q + K])
            if nd is not None:
                if prev is not None and follows(prev, nd):
                    rows[-1][4] = q
                else:
                    link = NO_LINK if prev is None else link_of(prev, nd)
                    rows.append([nd[0], nd[1], nd[2] | (2 if circ[nd[0]] else 0), q, q, link])
            prev = nd
        sso.append(len(rows))
    cols = list(zip(*rows)) if rows else [[]] * 6
    out = {"seq_step_off": np.array(sso, dtype=np.uint64)}
    for k, dt, col in zip(KEYS[1:], DTYPES[1:], cols):
        out[k] = np.array(col, dtype=dt)
    out["support"] = None if sup is None else np.array(sup, dtype=np.uint64)
    out["U"], out["E"] = U, E
    return out


def dual_of(g: dict) -> list:
    """for every link j = (e -> t) the index of t ^ 1 -> e ^ 1 (None when the graph lacks it)"""
    lo = [int(v) for v in g["link_off"]]
    to = [int(v) for v in g["link_to"]]
    out = []
    for e in range(len(lo) - 1):
        for j in range(lo[e], lo[e + 1]):
            t = to[j]
            out.append(next((i for i in range(lo[t ^ 1], lo[(t ^ 1) + 1]) if to[i] == e ^ 1), None))
    return out
