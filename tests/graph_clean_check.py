"""Array-only checker of a graph compaction (a helper, not a conftest): numpy over the arrays of G, remove, G' and the map, no walk and no
dict of k-mers. It holds an answer to the contract above the aix_graph_* declarations of include/aindex_hip.h from the other side than
tests/graph_clean_ref.py: it never builds a contig, it verifies one.

  check(g, remove, out)   g, out: dicts with the eight arrays of a unitig set (out also unitig_contig / unitig_pos / unitig_flag);
                          raises AssertionError with the name of the violated rule
  check_graph(g)          the format rules of a unitig set alone: offsets, degrees, link words, duality
"""
import numpy as np

K = 23
NONE32 = 0xFFFFFFFF


def _i64(a):
    return np.asarray(a).astype(np.int64)


def _code_of_rows(rows: np.ndarray) -> np.ndarray:
    """46-bit codes of rows of 23 ASCII bases"""
    two = ((rows >> 1) ^ (rows >> 2)) & 3
    code = np.zeros(rows.shape[0], np.int64)
    for i in range(K):
        code = (code << 2) | two[:, i].astype(np.int64)
    return code


def _comp(b: np.ndarray) -> np.ndarray:
    return b ^ np.where(b & 2, 0x04, 0x15).astype(np.uint8)


def _link_src(link_off: np.ndarray) -> np.ndarray:
    return np.repeat(np.arange(link_off.shape[0] - 1, dtype=np.int64), np.diff(link_off))


def check_graph(g: dict) -> None:
    off, lo, to = _i64(g["offsets"]), _i64(g["link_off"]), _i64(g["link_to"])
    U = off.shape[0] - 1
    assert (np.diff(off) >= K).all(), "offsets ascend by at least 23"
    assert g["bases"].shape[0] == (off[U] if U else 0), "bases hold offsets[U] bytes"
    assert lo.shape[0] == 2 * U + 1 and lo[0] == 0 and lo[-1] == to.shape[0], "link_off spans link_to"
    deg = np.diff(lo)
    assert ((deg >= 0) & (deg <= 4)).all(), "an end has 0 .. 4 links"
    assert (to < 2 * U).all(), "link words are below 2 U"
    for k in ("circular", "tf_sum", "tf_min", "tf_max"):
        assert np.asarray(g[k]).shape[0] == U, k
    src = _link_src(lo)
    circ = np.asarray(g["circular"]).astype(bool)
    assert not circ[src >> 1].any() and not circ[to >> 1].any(), "a circular unitig has no links"
    a = np.sort(src * (2 * U + 1) + to)
    b = np.sort((to ^ 1) * (2 * U + 1) + (src ^ 1))
    assert np.array_equal(a, b), "every link has its dual"


def check(g: dict, remove, out: dict) -> None:
    check_graph(g)
    check_graph(out)
    off, lo, to = _i64(g["offsets"]), _i64(g["link_off"]), _i64(g["link_to"])
    U = off.shape[0] - 1
    m = np.diff(off) - (K - 1)
    alive = np.asarray(remove) == 0
    circ = np.asarray(g["circular"]).astype(bool)
    cid, pos, flag = _i64(out["unitig_contig"]), _i64(out["unitig_pos"]), _i64(out["unitig_flag"])
    noff = _i64(out["offsets"])
    C = noff.shape[0] - 1
    assert cid.shape[0] == pos.shape[0] == flag.shape[0] == alive.shape[0] == U, "the map holds U entries"
    assert (cid[~alive] == NONE32).all() and (pos[~alive] == 0).all() and (flag[~alive] == 0).all(), "a removed unitig maps to nothing"
    assert ((cid[alive] >= 0) & (cid[alive] < C)).all(), "a surviving unitig maps to a contig"
    mem = np.nonzero(alive)[0]
    if C == 0:
        assert mem.shape[0] == 0 and noff.tolist() == [0] and _i64(out["link_off"]).tolist() == [0], "nothing survives: C = 0"
        return
    mc = np.diff(noff) - (K - 1)
    rev = (flag & 1).astype(bool)
    cyc = (flag & 2).astype(bool)
    assert not (cyc & circ).any(), "an input-circular unitig keeps flag 0"

    # 1. the members of every contig tile its k-mers
    order = mem[np.lexsort((pos[mem], cid[mem]))]
    oc, op, om = cid[order], pos[order], m[order]
    first = np.ones(order.shape[0], bool)
    first[1:] = oc[1:] != oc[:-1]
    assert np.array_equal(oc[first], np.arange(C)), "every contig 0 .. C - 1 has members"
    assert (op[first] == 0).all(), "a contig starts at position 0"
    assert (op[1:][~first[1:]] == (op[:-1] + om[:-1])[~first[1:]]).all(), "members follow each other without a gap"
    last = np.ones(order.shape[0], bool)
    last[:-1] = first[1:]
    assert np.array_equal((op + om)[last], mc), "the members of a contig add up to its k-mers"

    # 2. every member's oriented spelling stands in the contig where the map says (this holds the overlaps and the orientations)
    bases_in, bases_out = np.asarray(g["bases"]), np.asarray(out["bases"])
    ln = m[order] + (K - 1)
    start_in, start_out = off[order], noff[oc] + op
    within = np.arange(int(ln.sum()), dtype=np.int64) - np.repeat(np.cumsum(ln) - ln, ln)
    r = np.repeat(rev[order], ln)
    src_idx = np.repeat(start_in, ln) + np.where(r, np.repeat(ln, ln) - 1 - within, within)
    want = bases_in[src_idx]
    want = np.where(r, _comp(want), want)
    got = bases_out[np.repeat(start_out, ln) + within]
    assert np.array_equal(got, want), "a member is spelled in its contig at its position, in its orientation"

    # 3. abundance
    for k, fn, init in (("tf_sum", np.add, 0), ("tf_min", np.minimum, np.iinfo(np.uint32).max), ("tf_max", np.maximum, 0)):
        acc = np.full(C, init, dtype=np.uint64)
        fn.at(acc, oc, np.asarray(g[k]).astype(np.uint64)[order])
        assert np.array_equal(acc, np.asarray(out[k]).astype(np.uint64)), k

    # 4. merge edges: surviving degrees from the arrays
    src = _link_src(lo)
    keep = alive[src >> 1] & alive[to >> 1]
    ssrc, sto = src[keep], to[keep]
    degp = np.bincount(ssrc, minlength=2 * U)
    single = np.full(2 * U, -1, np.int64)
    single[ssrc] = sto                                              # meaningful where degp == 1
    t = np.where(degp == 1, single, 0)
    ends = np.arange(2 * U, dtype=np.int64)
    merge = (degp == 1) & (degp[t ^ 1] == 1) & (((t >> 1) != (ends >> 1)) | ((t == ends) & (np.repeat(m, 2) >= 2)))
    u = ends >> 1
    side = (ends ^ flag[u]) & 1                                     # 0: the right side of u as its contig spells it
    al = np.repeat(alive, 2)
    mg = merge & al
    v = t >> 1
    assert (cid[v[mg]] == cid[u[mg]]).all(), "a merge edge joins two members of one contig"
    assert (((t ^ flag[v]) & 1)[mg] == side[mg]).all(), "a member is oriented as its merge edges say"
    assert (cyc[v[mg]] == cyc[u[mg]]).all(), "bit 1 of the flag is one value per contig"
    right, left = mg & (side == 0), mg & (side == 1)
    mcu = mc[np.where(al, cid[u], 0)]
    wrap_r = cyc[u] & (pos[v] == 0) & (pos[u] + m[u] == mcu)
    wrap_l = cyc[u] & (pos[u] == 0) & (pos[v] + m[v] == mcu)
    assert ((pos[v] == pos[u] + m[u]) | wrap_r)[right].all(), "the right neighbour follows"
    assert ((pos[v] + m[v] == pos[u]) | wrap_l)[left].all(), "the left neighbour precedes"
    free = al & ~merge
    assert not cyc[u[free]].any(), "a member of a merged cycle has two merged ends"
    lin = free & ~circ[u]
    assert (pos[u] + m[u] == mcu)[lin & (side == 0)].all(), "an end without a merge edge is the right end of its contig (the contigs are maximal)"
    assert (pos[u] == 0)[lin & (side == 1)].all(), "an end without a merge edge is the left end of its contig (the contigs are maximal)"
    pc = circ & alive
    assert (m[pc] == mc[cid[pc]]).all(), "an input-circular unitig is a contig of its own"

    # 5. circular flags, start and order
    fm = order[first]
    want_circ = circ[fm] | cyc[fm]
    assert np.array_equal(np.asarray(out["circular"]).astype(bool), want_circ), "circular: passed through, or a merged cycle"
    cmin = np.full(C, U, np.int64)
    np.minimum.at(cmin, oc, order)
    assert (fm[cyc[fm]] == cmin[cyc[fm]]).all() and not rev[fm[cyc[fm]]].any(), "a merged cycle starts at its smallest member, forwards"
    heads = bases_out[noff[:-1, None] + np.arange(K)[None, :]]
    hc = _code_of_rows(heads)
    key = np.stack([hc, fm], axis=1)
    assert all(tuple(key[i]) < tuple(key[i + 1]) for i in np.nonzero(hc[1:] <= hc[:-1])[0]), "contig ids ascend by first 23-mer, then first member"
    linear = ~want_circ
    tails = _comp(bases_out[(noff[1:, None] - 1) - np.arange(K)[None, :]])
    assert (hc[linear] <= _code_of_rows(tails)[linear]).all(), "a path is spelled from its smaller end"

    # 6. links of G': the surviving non-merge links, rewritten, in their original order
    fl = free[ssrc] & ~circ[ssrc >> 1]
    new_src = 2 * cid[ssrc[fl] >> 1] + ((ssrc[fl] ^ flag[ssrc[fl] >> 1]) & 1)
    new_to = 2 * cid[sto[fl] >> 1] + ((sto[fl] ^ flag[sto[fl] >> 1]) & 1)
    o2 = np.argsort(new_src, kind="stable")
    assert np.array_equal(np.diff(_i64(out["link_off"])), np.bincount(new_src, minlength=2 * C)), "degrees of the contig ends"
    assert np.array_equal(_i64(out["link_to"]), new_to[o2]), "links of the contig ends"
