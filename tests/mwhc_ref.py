"""A plain reference of what aix_builder_gpu.hip computes — TEST INFRASTRUCTURE ONLY (numpy + oracle_lib, no call into aindex_amd).

MWHC construction of an emphf `.pf` over n keys given as 2-bit codes of length k, with the deterministic peeling rule of the GPU builder:

  * key i is hashed as its k ASCII bytes (first base most significant) with the oracle's Jenkins hash and trial seed s to (a, b, c) and becomes
    the edge (a % D, D + b % D, 2 D + c % D) of a 3-partite hypergraph on 3 D vertices, D = (ceil(1.23 n) + 2) // 3;
  * seeds are the first 64 outputs of mt19937_64(37); the first seed whose hypergraph peels completely is used, none -> AIX_ERR_CONFLICT;
  * peeling is round-synchronous: an edge is peeled in the first round at whose START one of its vertices has degree 1, and its hinge is the
    LOWEST-numbered vertex of that edge with degree 1 at the start of that round;
  * rounds in reverse: value(hinge) = (orientation - value(other1) - value(other2)) mod 3 with 0 replaced by 3, every other vertex stays 0;
  * 32 bit-pairs per 64-bit word; header {n, D, seed, B = 3 D}, W = ceil(B/32) words, R = ceil(B/512) cumulative non-zero-pair counts (one per
    16 words).

Nothing here depends on the order of the keys or on the order in which the edges of one round are visited, so the bytes are a function of the
key SET; tests/test_mwhc_ref_cpu.py checks this file on its own, tests/test_gpu_builder.py holds the kernels against it byte for byte.
"""
from __future__ import annotations

import math

import numpy as np

import oracle_lib as O

AIX_OK, AIX_ERR_CONFLICT = 0, -12
TRIALS = 64
ORACLE_HASH_MAX = 2048                  # key sets up to this size are hashed one key at a time by the oracle, larger ones by jenkins_np
U64 = np.uint64
_M64 = (1 << 64) - 1


# ------------------------------------------------------------------------------------------------
# std::mt19937_64 (numpy's MT19937 is the 32-bit generator)
# ------------------------------------------------------------------------------------------------
def mt19937_64(seed: int, count: int) -> list:
    nn, mm = 312, 156
    mt = [0] * nn
    mt[0] = seed & _M64
    for i in range(1, nn):
        mt[i] = (6364136223846793005 * (mt[i - 1] ^ (mt[i - 1] >> 62)) + i) & _M64
    out, idx = [], nn
    for _ in range(count):
        if idx == nn:
            for i in range(nn):
                x = (mt[i] & 0xFFFFFFFF80000000) | (mt[(i + 1) % nn] & 0x7FFFFFFF)
                mt[i] = mt[(i + mm) % nn] ^ (x >> 1) ^ (0xB5026F5AA96619E9 if x & 1 else 0)
            idx = 0
        x = mt[idx]
        idx += 1
        x ^= (x >> 29) & 0x5555555555555555
        x ^= (x << 17) & 0x71D67FFFEDA60000
        x ^= (x << 37) & 0xFFF7EEE000000000
        x ^= x >> 43
        out.append(x & _M64)
    return out


def seeds() -> list:
    return mt19937_64(37, TRIALS)


# ------------------------------------------------------------------------------------------------
# keys
# ------------------------------------------------------------------------------------------------
def ascii_of_codes(codes, k: int) -> np.ndarray:
    """uint8 [n, k]: the k-mer of every 2-bit code, first base in the most significant pair"""
    c = np.ascontiguousarray(codes).view(U64).reshape(-1)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    out = np.empty((c.shape[0], k), dtype=np.uint8)
    for j in range(k):
        out[:, j] = lut[((c >> U64(2 * (k - 1 - j))) & U64(3)).astype(np.int64)]
    return out


def revcomp_codes(codes, k: int) -> np.ndarray:
    c = np.ascontiguousarray(codes).view(U64).reshape(-1)
    out = np.zeros_like(c)
    for j in range(k):
        out |= (U64(3) - ((c >> U64(2 * j)) & U64(3))) << U64(2 * (k - 1 - j))
    return out


def dims(n: int):
    """(D, B, W, R) of a key set of size n; the double arithmetic is the builders' (mphf.hpp:26)"""
    D = (math.ceil(n * 1.23) + 2) // 3
    B = 3 * D
    return D, B, (B + 31) // 32, (B + 511) // 512


def n_for_bitpairs(B: int) -> int:
    """the smallest n whose bit-pair count is B"""
    n = 1
    while dims(n)[1] < B:
        n += 1
    assert dims(n)[1] == B, (B, n)
    return n


# ------------------------------------------------------------------------------------------------
# hash: per key through the oracle, or lookup8 restated over numpy columns (checked against the oracle in test_mwhc_ref_cpu.py)
# ------------------------------------------------------------------------------------------------
def jenkins_oracle(ascii_keys: np.ndarray, seed: int):
    h = np.array([O.jenkins(row.tobytes(), seed) for row in ascii_keys], dtype=U64).reshape(-1, 3)
    return h[:, 0].copy(), h[:, 1].copy(), h[:, 2].copy()


def _mix(a, b, c):
    for sa, sb, sc in ((43, 9, 8), (38, 23, 5), (35, 49, 11), (12, 18, 22)):
        a -= b; a -= c; a ^= c >> U64(sa)
        b -= c; b -= a; b ^= a << U64(sb)
        c -= a; c -= b; c ^= b >> U64(sc)
    return a, b, c


def jenkins_np(ascii_keys: np.ndarray, seed: int):
    n, k = ascii_keys.shape
    assert 1 <= k <= 47
    with np.errstate(over="ignore"):
        a = np.full(n, seed, dtype=U64)
        b = np.full(n, seed, dtype=U64)
        c = np.full(n, 0x9E3779B97F4A7C13, dtype=U64)
        col = lambda i: ascii_keys[:, i].astype(U64)              # noqa: E731
        word = lambda lo: sum((col(lo + j) << U64(8 * j) for j in range(1, 8)), col(lo))   # noqa: E731
        cur = 0
        if k >= 24:
            a += word(0); b += word(8); c += word(16)
            a, b, c = _mix(a, b, c)
            cur = 24
        c += U64(k)
        for i in range(k - cur):
            v = col(cur + i)
            if i < 8:
                a += v << U64(8 * i)
            elif i < 16:
                b += v << U64(8 * (i - 8))
            else:
                c += v << U64(8 * (i - 16 + 1))
        return _mix(a, b, c)


# ------------------------------------------------------------------------------------------------
# one trial
# ------------------------------------------------------------------------------------------------
def edges(ascii_keys, seed: int, D: int, hasher):
    a, b, c = hasher(ascii_keys, seed)
    d = U64(D)
    return (a % d).astype(np.int64), (b % d).astype(np.int64) + D, (c % d).astype(np.int64) + 2 * D


def peel(v, m: int):
    """v: the three vertex columns. -> (rounds, contested) with rounds = [(edge ids, hinges)] in peeling order, or (None, contested) when a
    2-core remains. Round-synchronous; the hinge of an edge is its lowest-numbered vertex of degree 1 at the start of the round."""
    n = v[0].shape[0]
    deg = np.zeros(m, dtype=np.int64)
    xe = np.zeros(m, dtype=np.int64)                               # XOR of the ids of the incident edges
    ids = np.arange(n, dtype=np.int64)
    for col in v:
        np.add.at(deg, col, 1)
        np.bitwise_xor.at(xe, col, ids)
    frontier = np.flatnonzero(deg == 1)                            # ascending
    rounds, peeled, contested = [], 0, 0
    while frontier.size:
        e_of = xe[frontier]                                        # the only edge of every degree-1 vertex
        e, first, mult = np.unique(e_of, return_index=True, return_counts=True)
        hinge = frontier[first]                                    # frontier ascends and np.unique reports first occurrences: the lowest vertex
        contested += int((mult >= 2).sum())
        rounds.append((e, hinge))
        peeled += e.size
        touched = []
        for col in v:
            u = col[e]
            np.subtract.at(deg, u, 1)
            np.bitwise_xor.at(xe, u, e)
            touched.append(u)
        cand = np.unique(np.concatenate(touched))
        frontier = cand[deg[cand] == 1]
    return (rounds if peeled == n else None), contested


def assign(v, rounds, m: int) -> np.ndarray:
    bv = np.zeros(m, dtype=np.int64)
    cols = np.stack(v, axis=1)                                     # [n, 3], ascending along the row
    for e, hinge in reversed(rounds):
        tri = cols[e]
        orient = (tri == hinge[:, None]).argmax(axis=1)
        others = bv[tri].sum(axis=1) - bv[hinge]                   # the hinge itself is still 0
        val = (orient - others) % 3
        val[val == 0] = 3
        bv[hinge] = val
    return bv


def image(n: int, D: int, seed: int, bv: np.ndarray) -> bytes:
    _, B, W, R = dims(n)
    pairs = np.zeros(W * 32, dtype=U64)
    pairs[:B] = bv.astype(U64)
    words = np.zeros(W, dtype=U64)
    for j in range(32):
        words |= pairs[j::32] << U64(2 * j)
    nz = (pairs != 0).reshape(W, 32).sum(axis=1).astype(U64)
    before = np.concatenate([np.zeros(1, dtype=U64), np.cumsum(nz, dtype=U64)])[:-1]
    ranks = before[::16]
    assert ranks.shape[0] == R
    return np.array([n, D, seed, B], dtype=U64).tobytes() + words.tobytes() + ranks.astype(U64).tobytes()


def build(codes, k: int, hasher=None):
    """-> (status, pf bytes or None, info). info: trials (seeds tried, 64 on conflict), rounds, contested (edges with at least two degree-1
    vertices at the start of their round, in the successful trial), seed."""
    codes = np.ascontiguousarray(codes).view(U64).reshape(-1)
    n = codes.shape[0]
    assert n >= 1 and 1 <= k <= 32
    if hasher is None:
        hasher = jenkins_oracle if n <= ORACLE_HASH_MAX else jenkins_np
    D, B, _, _ = dims(n)
    keys = ascii_of_codes(codes, k)
    for trial, seed in enumerate(seeds()):
        v = edges(keys, seed, D, hasher)
        rounds, contested = peel(v, B)
        if rounds is not None:
            bv = assign(v, rounds, B)
            return AIX_OK, image(n, D, seed, bv), {"trials": trial + 1, "rounds": len(rounds), "contested": contested, "seed": seed}
    return AIX_ERR_CONFLICT, None, {"trials": TRIALS, "rounds": 0, "contested": 0, "seed": None}


# ------------------------------------------------------------------------------------------------
# the key sets that tests/test_mwhc_ref_cpu.py and tests/test_gpu_builder.py share
# ------------------------------------------------------------------------------------------------
def random_codes(seed: int, n: int, k: int, canonical: bool = False) -> np.ndarray:
    """n distinct k-mer codes in random order (canonical: each the smaller of itself and its reverse complement)"""
    rng = np.random.default_rng(seed)
    space = 4 ** k
    if n > space:
        raise ValueError((n, k))
    if space <= 4 * n:
        return rng.permutation(space)[:n].astype(U64)
    c = rng.integers(0, space, size=2 * n + 64, dtype=U64)
    if canonical:
        c = np.minimum(c, revcomp_codes(c, k))
    _, first = np.unique(c, return_index=True)
    c = c[np.sort(first)]
    assert c.shape[0] >= n
    return np.ascontiguousarray(c[:n])


# bit-pair counts on both sides of a 64-bit word (32 pairs) and of a rank block (512 pairs). B = 3 D is a multiple of 3, so 32 and 512 themselves
# cannot occur: 30 | 33 and 510 | 513 are their neighbours, 96 and 1536 are the first counts that END on a word and on a rank block.
BOUNDARY_B = (3, 30, 33, 96, 510, 513, 1536)
N_MAIN, N_DUP = 30_000, 20_000
N_STRIDE2 = 16384 * 256 + 4097                                     # more keys than one trip of the grid-stride loops


def cases():
    """name -> (k, n, seed of the key set)"""
    c = {"k23_main": (23, N_MAIN, 2301), "k13": (13, 5_000, 1301)}
    for n in (1, 3, 4):
        c[f"k1_n{n}"] = (1, n, 100 + n)
    for k in (9, 17, 31, 32):
        c[f"k{k}"] = (k, 2_000, 1000 + k)
    for B in BOUNDARY_B:
        c[f"B{B}"] = (23, n_for_bitpairs(B), 5000 + B)
    return c


def case_keys(name: str) -> np.ndarray:
    k, n, seed = cases()[name]
    return random_codes(seed, n, k, canonical=(name == "k23_main"))


def sweep_keys(n: int) -> np.ndarray:
    """the small-n sweep: n = 1..33 at k = 23"""
    return random_codes(7000 + n, n, 23)


def dup_keys() -> np.ndarray:
    """N_DUP 23-mers, one of them twice"""
    c = random_codes(2323, N_DUP - 1, 23)
    return np.ascontiguousarray(np.insert(c, 12_345, c[777]))
