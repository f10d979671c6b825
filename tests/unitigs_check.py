"""A checker for the De Bruijn compaction that scales (a helper, not a conftest): array operations only, no walk, no dict, independent of
unitigs_ref.unitigs and of every kernel. It restates the contract above the aix_unitigs* declarations of include/aindex_hip.h as rules
over the output arrays; together the rules admit one output only, so an answer that check() accepts is THE answer.

  links(codes, tfs, cutoff, xp=np)       link[2 n] (int64, -1 = none) in kid order; port 2 kid + side leaves the node as stored (side 0) or as
                                         its reverse complement (side 1). word[p] = the entered port 2 kid' + (y <= rc y) of the only live
                                         successor y of the oriented k-mer, if there is exactly one; p is linked to t = word[p] iff
                                         word[t] == p and t is a port of another node. `xp` is numpy, or torch with tensors of any device
                                         (searchsorted and element-wise integer arithmetic only: plumbing, not a kernel under test).
  check(codes, tfs, cutoff, out, device=None)   AssertionError naming the first violated rule. `out` holds the arrays of the contract as
                                         numpy arrays, kmer_tf included; `device` computes the link table with torch there.
"""
import numpy as np

K = 23
MASK = (1 << 46) - 1
NONE = (1 << 64) - 1
_LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)


def _rc(x):
    """reverse complement of 23-mer codes held in int64 (numpy arrays or torch tensors): complement, reverse the 32 two-bit groups of
    the word, drop the 18 low bits that the reversal brought down. >> is arithmetic: every shifted value is masked."""
    x = x ^ MASK
    for s, m in ((2, 0x3333333333333333), (4, 0x0F0F0F0F0F0F0F0F), (8, 0x00FF00FF00FF00FF), (16, 0x0000FFFF0000FFFF), (32, 0x00000000FFFFFFFF)):
        x = ((x >> s) & m) | ((x & m) << s)
    return (x >> 18) & MASK


def links(codes, tfs, cutoff, xp=np):
    if xp is np:
        codes = np.ascontiguousarray(codes).astype(np.uint64).view(np.int64)
        live = np.asarray(tfs).astype(np.int64) > int(cutoff)
        kids = np.arange(codes.shape[0], dtype=np.int64)
    else:                                                          # torch: int64 codes, int64 tf, both on the same device
        live = tfs > int(cutoff)
        kids = xp.arange(codes.shape[0], dtype=xp.int64, device=codes.device)
    n = codes.shape[0]
    order = xp.argsort(codes)
    sc = codes[order]
    word = []
    for side in (0, 1):
        x = _rc(codes) if side else codes
        deg, ent = 0 * kids, 0 * kids - 1
        for b in range(4):
            y = ((x << 2) | b) & MASK
            ry = _rc(y)
            cy = xp.minimum(y, ry)
            i = xp.searchsorted(sc, cy)
            i = i * (i < n)
            there = live & (sc[i] == cy) & live[order[i]]
            deg = deg + there
            ent = xp.where(there, 2 * order[i] + (y <= ry), ent)
        word.append(xp.where(deg == 1, ent, 0 * kids - 1))
    word = xp.stack(word, 1).reshape(-1)                           # word[2 kid + side]
    p = xp.stack([2 * kids, 2 * kids + 1], 1).reshape(-1)
    back = word[word * (word >= 0)]
    return xp.where((word >= 0) & (back == p) & ((word >> 1) != (p >> 1)), word, 0 * p - 1)


def _links_on(codes, tfs, cutoff, device):
    import torch
    c = torch.from_numpy(np.ascontiguousarray(codes).astype(np.uint64).view(np.int64)).to(device)
    t = torch.from_numpy(np.asarray(tfs).astype(np.int64)).to(device)
    return links(c, t, cutoff, torch).cpu().numpy()


def check(codes, tfs, cutoff, out, device=None):
    codes = np.ascontiguousarray(codes).astype(np.uint64)
    tfs = np.asarray(tfs).astype(np.uint32)
    n = codes.shape[0]
    live = tfs.astype(np.int64) > int(cutoff)
    ku, kp, kf = (np.asarray(out[k]) for k in ("kid_unitig", "kid_pos", "kid_flag"))
    assert ku.shape == kp.shape == kf.shape == (n,), "the per-kid arrays have n entries"
    assert np.array_equal(ku == np.uint64(NONE), ~live), "kid_unitig == NONE iff the key is dead"
    assert not kp[~live].any() and not kf[~live].any(), "dead keys carry pos 0 and flag 0"
    U, n_live = int(out["U"]), int(live.sum())
    assert int(out["n_live"]) == n_live, "n_live counts the keys with tf > cutoff"
    off = np.asarray(out["offsets"]).astype(np.int64)
    circular = np.asarray(out["circular"])
    assert off.shape == (U + 1,) and circular.shape == (U,), "U agrees with offsets and circular"
    for k in ("tf_sum", "tf_min", "tf_max"):
        assert np.asarray(out[k]).shape == (U,), f"U agrees with {k}"
    assert int(out["n_circular"]) == int((circular != 0).sum()) and (circular <= 1).all(), "n_circular counts the circular flags"
    assert off[0] == 0, "offsets start at 0"
    m = np.diff(off) - (K - 1)
    assert (m >= 1).all() and int(m.sum()) == n_live, "member counts are at least 1 and sum to n_live"
    bases, kmer_tf = np.asarray(out["bases"]), np.asarray(out["kmer_tf"])
    assert bases.shape == (int(off[-1]),) and kmer_tf.shape == (n_live,), "bases and kmer_tf have offsets[U] and n_live entries"
    if U == 0:
        return
    lk = np.nonzero(live)[0]
    assert (ku[lk] < np.uint64(U)).all(), "unitig ids are below U"
    u_of = ku[lk].astype(np.int64)
    start = off[:-1] - (K - 1) * np.arange(U, dtype=np.int64)       # the first k-mer of unitig u, in unitig order
    assert (kp[lk] < m[u_of]).all(), "kid_pos is below the member count"
    slot = start[u_of] + kp[lk]
    assert (np.bincount(slot, minlength=n_live) == 1).all(), "each (unitig, pos) slot is claimed exactly once"
    kid = np.empty(n_live, np.int64)                                # the members in unitig order
    kid[slot] = lk
    u_seq = np.repeat(np.arange(U, dtype=np.int64), m)
    assert (kf <= 3).all() and np.array_equal((kf[kid] >> 1) & 1, circular[u_seq]), "kid_flag & 2 equals the unitig's circular"
    f = (kf[kid] & 1).astype(np.int64)
    link = links(codes, tfs, cutoff) if device is None else _links_on(codes, tfs, cutoff, device)
    leave, enter = 2 * kid + f, 2 * kid + (1 - f)
    first, last = start, start + m - 1
    inner = np.ones(n_live, bool)
    inner[last] = False
    j = np.nonzero(inner)[0]
    assert np.array_equal(link[leave[j]], enter[j + 1]), "consecutive members are linked"
    lin, cyc = circular == 0, circular != 0
    assert (link[enter[first[lin]]] == -1).all() and (link[leave[last[lin]]] == -1).all(), "a linear unitig's outer ports are unlinked"
    assert np.array_equal(link[leave[last[cyc]]], enter[first[cyc]]), "a circle's last exit links to its first entry"
    c = codes[kid].view(np.int64)
    o = np.where(f == 1, _rc(c), c)                                 # the oriented k-mers in unitig order
    longer = lin & (m > 1)
    assert (o[first[longer]] < _rc(o[last[longer]])).all(), "a linear unitig is spelled from the smaller end"
    assert not f[first[lin & (m == 1)]].any(), "a single node is spelled as stored"
    assert np.array_equal(c[first[cyc]], np.minimum.reduceat(c, first)[cyc]) and not f[first[cyc]].any(), \
        "a circle starts at its smallest stored code with f == 0"
    assert (np.diff(o[first]) > 0).all(), "ids ascend strictly by first oriented k-mer"
    want = np.empty(int(off[-1]), np.uint8)
    at = np.arange(n_live, dtype=np.int64) + (K - 1) * u_seq
    want[at + K - 1] = _LETTERS[o & 3]
    shifts = 2 * (K - 1 - np.arange(K, dtype=np.int64))
    want[off[:-1, None] + np.arange(K)[None, :]] = _LETTERS[(o[first][:, None] >> shifts[None, :]) & 3]
    assert np.array_equal(bases, want), "bases equals the spelling rebuilt from codes, orientations and offsets"
    assert np.array_equal(kmer_tf, tfs[kid]), "kmer_tf equals tf in unitig order"
    t = kmer_tf.astype(np.uint64)
    assert np.array_equal(np.asarray(out["tf_sum"]), np.add.reduceat(t, first)), "tf_sum equals the sum over kmer_tf"
    assert np.array_equal(np.asarray(out["tf_min"]), np.minimum.reduceat(kmer_tf, first)), "tf_min equals the minimum over kmer_tf"
    assert np.array_equal(np.asarray(out["tf_max"]), np.maximum.reduceat(kmer_tf, first)), "tf_max equals the maximum over kmer_tf"
