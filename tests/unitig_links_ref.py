"""Test-side restatement of the unitig graph (a helper, not a conftest): the links between unitig ends and the simple bubbles of a
canonical 23-mer key set, sequentially, over the dict answer of unitigs_ref.unitigs. It restates the contract above the aix_unitig_links*
declarations of include/aindex_hip.h:

  end 2 u + 0   leaves linear unitig u through the last oriented k-mer of its spelling; end 2 u + 1 through rc of the first one
  links(e)      the live members of {next(x, b)}, in base order, each as the word 2 v + r: v entered at its first k-mer (r = 0) or, reversed,
                at its last (r = 1)
  bubble_mate   the literal rule, one unitig at a time

The end k-mers are read off the restated spellings (`strings`), not off kid_unitig / kid_pos / kid_flag; that every live successor of an end
enters a linear unitig at one of its two ends is asserted, not assumed.

  links(codes, tfs, cutoff, un=None)   un = unitigs_ref.unitigs(codes, tfs, cutoff) -> {"link_off" uint64[2 U + 1], "link_to" uint32[E],
                                       "bubble_mate" uint32[U], "U", "E"}
"""
import numpy as np

import unitigs_ref as R

NONE32 = 0xFFFFFFFF
_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def encode(s: str) -> int:
    x = 0
    for ch in s:
        x = (x << 2) | _CODE[ch]
    return x


def bubbles(U: int, link_off, link_to) -> list:
    """bubble_mate by the literal rule over the two link arrays (python lists or arrays)"""
    off = [int(v) for v in link_off]
    to = [int(v) for v in link_to]

    def deg(e):
        return off[e + 1] - off[e]

    def tgt(e):
        return to[off[e]:off[e + 1]]

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


def links(codes, tfs, cutoff: int = 0, un=None) -> dict:
    if un is None:
        un = R.unitigs(codes, tfs, cutoff)
    live = {int(c) for c, t in zip(np.asarray(codes, dtype=np.uint64).tolist(), np.asarray(tfs).tolist()) if t > cutoff}
    U, strings, circular = un["U"], un["strings"], un["circular"].tolist()
    first = [encode(s[:R.K]) for s in strings]
    last = [encode(s[-R.K:]) for s in strings]
    enter = {}                                                     # oriented k-mer -> the word of the unitig end it enters
    for u in range(U):
        if not circular[u]:
            enter[first[u]] = 2 * u
            enter[R.rc(last[u])] = 2 * u + 1
    assert len(enter) == 2 * (U - sum(circular))
    link_off, link_to = [0], []
    for u in range(U):
        for side in (0, 1):
            if not circular[u]:
                x = last[u] if side == 0 else R.rc(first[u])
                for b in range(4):
                    y = R.nxt(x, b)
                    if R.canon(y) in live:
                        assert y in enter, "a live successor of an end is the first k-mer of a linear unitig in the entering orientation"
                        link_to.append(enter[y])
            link_off.append(len(link_to))
    mate = bubbles(U, link_off, link_to)
    return {"link_off": np.array(link_off, dtype=np.uint64), "link_to": np.array(link_to, dtype=np.uint32),
            "bubble_mate": np.array(mate, dtype=np.uint32), "U": U, "E": len(link_to)}
