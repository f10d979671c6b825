"""A checker for the unitig graph (a helper, not a conftest), in the spirit of unitigs_check.py: array operations only, no walk, no dict,
independent of unitig_links_ref and of every kernel. It restates the contract above the aix_unitig_links* declarations of
include/aindex_hip.h as rules over the arrays; together they admit one answer only.

  check(codes, tfs, cutoff, un, lk)   AssertionError naming the first violated rule. `un` holds offsets, bases and circular of the
                                      compaction at that cutoff (accepted by unitigs_check.check), `lk` link_off, link_to, bubble_mate;
                                      all numpy arrays.
  mates(U, link_off, link_to)         bubble_mate recomputed from the two link arrays by the literal rule, vectorised
"""
import numpy as np

from unitigs_check import K, MASK, _rc

NONE32 = 0xFFFFFFFF
_VAL = np.full(256, -1, np.int64)
_VAL[np.frombuffer(b"ACGT", dtype=np.uint8)] = np.arange(4)


def _encode(rows):
    """codes (int64) of the 23-base rows of a uint8 matrix"""
    v = _VAL[rows]
    assert (v >= 0).all(), "bases are upper-case A, C, G, T"
    x = np.zeros(rows.shape[0], np.int64)
    for j in range(K):
        x = (x << 2) | v[:, j]
    return x


def mates(U, link_off, link_to):
    off = np.asarray(link_off).astype(np.int64)
    to = np.asarray(link_to).astype(np.int64)
    deg = np.diff(off)
    pad = np.concatenate([to, np.full(4, -1, np.int64)])           # reads behind a degree give -1

    def tgt(e, j):                                                  # j-th target of end e, -1 where there is none (or e is -1)
        ok = (e >= 0) & (j < deg[e * (e >= 0)])
        return np.where(ok, pad[(off[e * (e >= 0)] + j) * ok], -1)

    def dg(e):
        return np.where(e >= 0, deg[e * (e >= 0)], -1)

    u = np.arange(U, dtype=np.int64)
    tR, tL = tgt(2 * u, 0), tgt(2 * u + 1, 0)
    one = (deg[2 * u] == 1) & (deg[2 * u + 1] == 1)
    f = np.where(one, tL ^ 1, -1)
    a, b = tgt(f, 0), tgt(f, 1)
    x = np.where(a == 2 * u, b, np.where(b == 2 * u, a, -1))
    ok = one & (dg(f) == 2) & (x >= 0) & ((x >> 1) != u) & (dg(np.where(one, tR ^ 1, -1)) == 2)
    x = np.where(ok, x, -1)
    ok &= (dg(x) == 1) & (tgt(x, 0) == tR) & (dg(np.where(x >= 0, x ^ 1, -1)) == 1) & (tgt(np.where(x >= 0, x ^ 1, -1), 0) == tL)
    return np.where(ok, x >> 1, NONE32).astype(np.uint32)


def check(codes, tfs, cutoff, un, lk):
    codes = np.ascontiguousarray(codes).astype(np.uint64).view(np.int64)
    live = np.asarray(tfs).astype(np.int64) > int(cutoff)
    n = codes.shape[0]
    order = np.argsort(codes)
    sc = codes[order]
    off_b = np.asarray(un["offsets"]).astype(np.int64)
    bases, circular = np.asarray(un["bases"]), np.asarray(un["circular"])
    U = circular.shape[0]
    link_off = np.asarray(lk["link_off"]).astype(np.int64)
    link_to = np.asarray(lk["link_to"]).astype(np.int64)
    assert np.asarray(lk["link_off"]).dtype == np.uint64 and np.asarray(lk["link_to"]).dtype == np.uint32, "link_off is u64, link_to u32"
    assert link_off.shape == (2 * U + 1,) and link_off[0] == 0, "link_off has 2 U + 1 entries and starts at 0"
    deg = np.diff(link_off)
    assert ((deg >= 0) & (deg <= 4)).all(), "link_off is monotone with steps of at most 4"
    E = int(link_off[-1])
    assert link_to.shape == (E,), "link_to has link_off[2 U] entries"
    mate = np.asarray(lk["bubble_mate"])
    assert mate.dtype == np.uint32 and mate.shape == (U,), "bubble_mate is u32[U]"
    if U == 0:
        return
    assert (link_to < 2 * U).all(), "link words are below 2 U"
    first = _encode(bases[off_b[:-1, None] + np.arange(K)[None, :]])
    last = _encode(bases[off_b[1:, None] - K + np.arange(K)[None, :]])
    lin = np.repeat(circular == 0, 2)
    assert not deg[~lin].any(), "the two entries of a circular unitig have degree 0"
    x = np.stack([last, _rc(first)], 1).reshape(-1)                 # the k-mer through which end 2 u + side leaves
    there, succ = [], []
    for b in range(4):
        y = ((x << 2) | b) & MASK
        cy = np.minimum(y, _rc(y))
        i = np.searchsorted(sc, cy)
        i = i * (i < n)
        there.append(lin & (sc[i] == cy) & live[order[i]])
        succ.append(y)
    there, succ = np.stack(there, 1), np.stack(succ, 1)
    assert np.array_equal(there.sum(1), deg), "the degree of an end is the number of its live successors"
    v, r = link_to >> 1, link_to & 1
    assert not circular[v].any(), "a link enters a linear unitig"
    entered = np.where(r == 0, first[v], _rc(last[v]))              # the first k-mer of the target as it is traversed
    assert np.array_equal(entered, succ[there]), "the links of an end are its live successors, in base order"
    # the same on the bases: 22 bases of overlap, and the appended base is the target's 23rd
    e = np.repeat(np.arange(2 * U, dtype=np.int64), deg)
    base = np.nonzero(there)[1]
    u, side = e >> 1, e & 1
    j = np.arange(K - 1, dtype=np.int64)[None, :]
    src = np.where(side[:, None] == 0, _VAL[bases[off_b[u + 1, None] - (K - 1) + j]], 3 - _VAL[bases[off_b[u, None] + (K - 2) - j]])
    j = np.arange(K, dtype=np.int64)[None, :]
    dst = np.where(r[:, None] == 0, _VAL[bases[off_b[v, None] + j]], 3 - _VAL[bases[off_b[v + 1, None] - 1 - j]])
    assert np.array_equal(src, dst[:, :K - 1]), "the last 22 bases of the source equal the first 22 of the target, both as traversed"
    assert np.array_equal(dst[:, K - 1], base), "the appended base is the target's 23rd"
    pairs = np.sort(e * (2 * U) + link_to)
    assert (np.diff(pairs) > 0).all(), "no link is listed twice"
    assert np.array_equal(pairs, np.sort((link_to ^ 1) * (2 * U) + (e ^ 1))), "(e -> t) is a link iff (t ^ 1 -> e ^ 1) is one"
    want = mates(U, link_off, link_to)
    assert np.array_equal(mate, want), "bubble_mate follows the literal rule"
    has = np.nonzero(mate != NONE32)[0]
    assert np.array_equal(mate[mate[has]], has.astype(np.uint32)), "bubble_mate is symmetric"
