"""Test-side restatement of the De Bruijn compaction (a helper, not a conftest): all maximal unitigs of a canonical 23-mer key set,
sequentially, over a Python dict. It restates the contract above the aix_unitigs* declarations of include/aindex_hip.h:

  live(x)   canon(x) is a stored key with tf > cutoff
  x -> y    y in out(x), |out(x)| == 1, |in(y)| == 1, canon(y) != canon(x)
  spelling  path: the one of its two spellings with the smaller first oriented k-mer; cycle: from its smallest stored code, in stored
            orientation, m k-mers; ids ascend by the first oriented k-mer

It walks left and right from every unvisited stored code in ascending order; nothing here ranks lists or jumps pointers.

  unitigs(codes, tfs, cutoff)  codes uint64[n] in kid order (every code canonical), tfs uint32[n] -> the arrays of the contract as a dict
"""
import numpy as np

K = 23
MASK = (1 << 46) - 1
NONE = (1 << 64) - 1
_COMP_BYTE = [0] * 256                                            # reverse complement of four bases at a time
for _v in range(256):
    _COMP_BYTE[_v] = sum((3 - ((_v >> (2 * j)) & 3)) << (2 * (3 - j)) for j in range(4))


def rc(x: int) -> int:
    y = 0
    for _ in range(6):                                             # 24 bases: the 23-mer shifted up by one base
        y = (y << 8) | _COMP_BYTE[x & 255]
        x >>= 8
    return y >> 2


def canon(x: int) -> int:
    return min(x, rc(x))


def nxt(x: int, b: int) -> int:
    return ((x << 2) | b) & MASK


def prv(x: int, b: int) -> int:
    return (x >> 2) | (b << 44)


def spell(kmers) -> str:
    first = "".join("ACGT"[(kmers[0] >> (2 * (K - 1 - i))) & 3] for i in range(K))
    return first + "".join("ACGT"[x & 3] for x in kmers[1:])


def unitigs(codes, tfs, cutoff: int = 0) -> dict:
    codes = [int(c) for c in np.asarray(codes, dtype=np.uint64).tolist()]
    tfs = [int(t) for t in np.asarray(tfs).tolist()]
    n = len(codes)
    assert all(c == canon(c) for c in codes), "the key set must be canonical"
    kid_of = {c: i for i, c in enumerate(codes) if tfs[i] > cutoff}   # the live keys

    def out(x):
        return [y for y in (nxt(x, b) for b in range(4)) if canon(y) in kid_of]

    def inn(x):
        return [y for y in (prv(x, b) for b in range(4)) if canon(y) in kid_of]

    def right(x):                                                  # y with x -> y, or None
        o = out(x)
        if len(o) != 1 or len(inn(o[0])) != 1 or canon(o[0]) == canon(x):
            return None
        return o[0]

    def left(x):                                                   # w with w -> x, or None
        i = inn(x)
        if len(i) != 1 or len(out(i[0])) != 1 or canon(i[0]) == canon(x):
            return None
        return i[0]

    seen = set()
    found = []                                                     # (first code, oriented k-mers, circular)
    for c in sorted(kid_of):
        if c in seen:
            continue
        path, circular = [c], False
        x = right(c)
        while x is not None:
            if canon(x) == c:                                      # back at the start: c is the smallest code of this circle
                circular = True
                break
            path.append(x)
            x = right(x)
        if not circular:
            x = left(c)
            while x is not None:
                path.insert(0, x)
                x = left(x)
            other = [rc(y) for y in reversed(path)]
            if other[0] < path[0]:
                path = other
        assert not seen.intersection(canon(y) for y in path)
        seen.update(canon(y) for y in path)
        found.append((path[0], path, circular))
    assert len(seen) == len(kid_of)
    found.sort(key=lambda f: f[0])

    U = len(found)
    res = {"U": U, "n_live": len(kid_of), "n_circular": sum(f[2] for f in found),
           "kid_unitig": np.full(n, NONE, np.uint64), "kid_pos": np.zeros(n, np.uint32), "kid_flag": np.zeros(n, np.uint8),
           "offsets": np.zeros(U + 1, np.uint64), "circular": np.zeros(U, np.uint8), "tf_sum": np.zeros(U, np.uint64),
           "tf_min": np.zeros(U, np.uint32), "tf_max": np.zeros(U, np.uint32), "first": np.zeros(U, np.uint64)}
    text, kmer_tf, at = [], [], 0
    for u, (first, path, circular) in enumerate(found):
        member_tf = []
        for pos, x in enumerate(path):
            kid = kid_of[canon(x)]
            res["kid_unitig"][kid], res["kid_pos"][kid] = u, pos
            res["kid_flag"][kid] = (1 if x != codes[kid] else 0) | (2 if circular else 0)
            member_tf.append(tfs[kid])
        res["offsets"][u], res["circular"][u], res["first"][u] = at, circular, first
        res["tf_sum"][u], res["tf_min"][u], res["tf_max"][u] = sum(member_tf), min(member_tf), max(member_tf)
        text.append(spell(path))
        kmer_tf += member_tf
        at += len(path) + K - 1
    res["offsets"][U] = at
    res["bases"] = np.frombuffer("".join(text).encode(), dtype=np.uint8).copy()
    res["kmer_tf"] = np.array(kmer_tf, dtype=np.uint32)
    res["strings"] = text
    return res
