"""k-mers by frequency, restated in numpy over the oracle (a helper, not a conftest): what aix_spectrum.hip must compute.

  values23(orc)              v_i = get_tf_value_23mer(get_kmer_by_kid(i)) (python_wrapper.cpp:610-627, 718-724) for every kid of an OracleIndex23:
                             the two-strand probe of checker[i] & (2^46 - 1), forward strand first — not tf[i]
  values13(orc)              v_i = (uint32_t) tf13[i] in file order (get_13mer_tf_array, :983-991) of an OracleIndex13
  select(v, min_v, max_items) (idx, val, total): descending value, ties in ascending index (Python's stable sort(key = tf, reverse = True),
                             aindex.py:643, 671), the first max_items (0 = all) entries with v >= min_v; total = entries >= min_v
  spectrum(v, nbins)         hist[j] = #{v = j} for j < nbins - 1, hist[nbins - 1] = #{v >= nbins - 1}
  stats(v)                   n, non-zero, max, smallest non-zero (0 if none), sum (u64)
  decode(codes, k) / revcomp_codes(codes, k), spell13(idx)   the labels
  same(items, golden)        a list against its form in tests/golden/*/frequency.json: the list itself, or — beyond 64 entries — its head,
                             length and SHA-256 (make_golden_spectrum.py: packed())
"""
import hashlib
import json

import numpy as np

MASK46 = np.uint64((1 << 46) - 1)
LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)


def decode(codes, k):
    """(N, k) uint8 ASCII of 2-bit codes, first base most significant (get_bitset_dna23, kmers.cpp)"""
    c = np.ascontiguousarray(codes, dtype=np.uint64).reshape(-1, 1)
    sh = (2 * (k - 1 - np.arange(k))).astype(np.uint64).reshape(1, -1)
    return LETTERS[((c >> sh) & np.uint64(3)).astype(np.int64)]


def revcomp_codes(codes, k):
    c = np.ascontiguousarray(codes, dtype=np.uint64).reshape(-1)
    out = np.zeros_like(c)
    for j in range(k):
        out |= (np.uint64(3) - ((c >> np.uint64(2 * j)) & np.uint64(3))) << np.uint64(2 * (k - 1 - j))
    return out


def values23(orc):
    return orc.tf_batch(decode(orc.checker() & MASK46, 23))


def values13(orc):
    return (orc.tf_arr & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def select(v, min_v=1, max_items=0):
    v = np.ascontiguousarray(v, dtype=np.uint32).reshape(-1)
    keep = np.nonzero(v.astype(np.uint64) >= np.uint64(min_v))[0]
    order = keep[np.argsort(-v[keep].astype(np.int64), kind="stable")]
    total = int(keep.shape[0])
    if max_items:
        order = order[:max_items]
    return order.astype(np.uint32), v[order], total


def spectrum(v, nbins):
    v = np.ascontiguousarray(v, dtype=np.uint32).reshape(-1)
    return np.bincount(np.minimum(v, np.uint32(min(nbins - 1, 0xFFFFFFFF))).astype(np.int64), minlength=nbins).astype(np.uint64)


def stats(v):
    v = np.ascontiguousarray(v, dtype=np.uint32).reshape(-1)
    nz = v[v != 0]
    return {"n": int(v.shape[0]), "non_zero": int(nz.shape[0]), "max": int(nz.max()) if nz.shape[0] else 0,
            "min_non_zero": int(nz.min()) if nz.shape[0] else 0, "sum": int(v.sum(dtype=np.uint64))}


def info23(orc, kids):
    """[get_kmer_info(kid)] (python_wrapper.cpp:744-755): (tf[kid], k-mer, reverse complement), (0, "", "") beyond the index"""
    chk, tf = orc.checker() & MASK46, orc.tf_array()
    out = []
    for kid in kids:
        if kid >= orc.n:
            out.append((0, "", ""))
            continue
        c = chk[kid:kid + 1]
        out.append((int(tf[kid]), decode(c, 23)[0].tobytes().decode(), decode(revcomp_codes(c, 23), 23)[0].tobytes().decode()))
    return out


def spell13(idx):
    return [r.tobytes().decode() for r in decode(np.asarray(idx, dtype=np.uint64), 13)]


def same(items, golden):
    items = list(items)
    if isinstance(golden, list):
        return items == golden
    sha = hashlib.sha256(json.dumps(items, separators=(",", ":")).encode()).hexdigest()
    return len(items) == golden["len"] and items[:len(golden["head"])] == golden["head"] and sha == golden["sha256"]


def kmers23(orc):
    return [r.tobytes().decode() for r in decode(orc.checker() & MASK46, 23)]
