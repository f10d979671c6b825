"""Test-side restatement of the De Bruijn neighbour and walk semantics (a helper, not a conftest), vectorised over numpy arrays.

Everything is computed from one callable `freq(codes uint64[N]) -> uint32[N]` = PHASH_MAP::get_freq(uint64_t) (hash.hpp:123-140:
forward strand, then the reverse complement). `oracle_freq(orc)` builds it from OracleIndex23.tf_batch on the decoded codes: for a
pure-ACGT string get_freq(string) and get_freq(code) are the same computation.

  cont()   DEBRUJIN::print_next / print_prev, debrujin.cpp:30-75 and :121-167
  walk()   the bounded walk defined on top of them (greedy / unitig)
"""
import numpy as np

MASK46 = np.uint64((1 << 46) - 1)
NEXT, PREV, BOTH = 0, 1, 2
GREEDY, UNITIG = 0, 1
MAX_STEPS, DEAD_END, BRANCH, JOIN, LOOP = 0, 1, 2, 3, 4
STOP_NAMES = ("max_steps", "dead_end", "branch", "join", "loop")
LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)
CONT_DTYPE = np.dtype([("tf", "<u4", (4,)), ("n", "<u4"), ("sum", "<u4"), ("best_tf", "<u4"), ("best_base", "<u4")])

_SHIFTS = np.array([2 * (22 - j) for j in range(23)], dtype=np.uint64)
_CODE_OF = np.zeros(256, dtype=np.uint64)                       # get_dna23_bitset (kmers.cpp:12-40): anything but upper-case ACGT adds 0 bits
for _i, _c in enumerate(b"ACGT"):
    _CODE_OF[_c] = _i


def encode(kmers) -> np.ndarray:
    """bytes / uint8 array of N * 23 bytes -> uint64[N] sanitised codes, first base most significant."""
    a = np.frombuffer(kmers, dtype=np.uint8) if isinstance(kmers, (bytes, bytearray)) else np.ascontiguousarray(kmers, dtype=np.uint8)
    a = a.reshape(-1, 23)
    return (_CODE_OF[a] << _SHIFTS[None, :]).sum(axis=1, dtype=np.uint64)


def decode(codes) -> np.ndarray:
    """uint64[N] -> uint8[N, 23] ASCII"""
    c = np.ascontiguousarray(codes, dtype=np.uint64).reshape(-1)
    return LETTERS[((c[:, None] >> _SHIFTS[None, :]) & np.uint64(3)).astype(np.intp)]


def revcomp(codes) -> np.ndarray:
    x = ~np.ascontiguousarray(codes, dtype=np.uint64)
    m2, m4 = np.uint64(0x3333333333333333), np.uint64(0x0F0F0F0F0F0F0F0F)
    x = ((x >> np.uint64(2)) & m2) | ((x & m2) << np.uint64(2))
    x = ((x >> np.uint64(4)) & m4) | ((x & m4) << np.uint64(4))
    return x.byteswap() >> np.uint64(64 - 46)


def canon(codes) -> np.ndarray:
    c = np.ascontiguousarray(codes, dtype=np.uint64)
    return np.minimum(c, revcomp(c))


def neigh(codes, direction: int, b) -> np.ndarray:
    c = np.ascontiguousarray(codes, dtype=np.uint64)
    b = np.asarray(b, dtype=np.uint64)
    if direction == NEXT:
        return ((c << np.uint64(2)) | b) & MASK46                 # debrujin.cpp:34-37
    return (c >> np.uint64(2)) | (b << np.uint64(44))             # debrujin.cpp:125-128


def oracle_freq(orc, threads: int = 1):
    def freq(codes):
        codes = np.ascontiguousarray(codes, dtype=np.uint64).reshape(-1)
        if codes.shape[0] == 0:
            return np.zeros(0, np.uint32)
        return np.asarray(orc.tf_batch(np.ascontiguousarray(decode(codes)).reshape(-1), threads), dtype=np.uint32)
    return freq


def cont(freq, codes, direction: int, cutoff: int = 0) -> np.ndarray:
    """CONT per code as CONT_DTYPE records."""
    c = np.ascontiguousarray(codes, dtype=np.uint64).reshape(-1)
    n = c.shape[0]
    nb = np.stack([neigh(c, direction, b) for b in range(4)], axis=1)                 # :34-37 / :125-128
    t = freq(nb.reshape(-1)).reshape(n, 4).astype(np.uint32)                          # :39-42 / :130-133
    if cutoff > 0:
        t[t <= np.uint32(cutoff)] = 0                                                 # :44-49 / :135-140, inclusive
    out = np.zeros(n, dtype=CONT_DTYPE)
    out["tf"] = t
    out["sum"] = t.sum(axis=1, dtype=np.uint32)                                       # :51 / :142, wraps in u32
    out["n"] = (t != 0).sum(axis=1)                                                   # :52-53 / :165-166
    # :55-74 / :144-163: four overwriting ifs = the last base that is >= the other three
    best = 3 - np.argmax(t[:, ::-1], axis=1)
    out["best_base"] = best
    out["best_tf"] = t[np.arange(n), best]
    return out


def neighbours(freq, codes, dirs: int, cutoff: int = 0) -> np.ndarray:
    """The layout of aix_neighbours: N records, or (N, 2) for BOTH. Like aix_neighbours (and walk below) it ignores bits 46 .. 63 of a code."""
    codes = np.ascontiguousarray(codes, dtype=np.uint64).reshape(-1) & MASK46
    if dirs != BOTH:
        return cont(freq, codes, dirs, cutoff)
    return np.stack([cont(freq, codes, NEXT, cutoff), cont(freq, codes, PREV, cutoff)], axis=1)


def walk(freq, seeds, direction: int, max_steps: int, cutoff: int = 0, mode: int = GREEDY):
    """(bases uint8[S, L] zero beyond the length, length uint32[S], stop uint8[S], tf uint32[S, L], last uint64[S])"""
    seeds = np.ascontiguousarray(seeds, dtype=np.uint64).reshape(-1) & MASK46
    S, L = seeds.shape[0], max_steps
    cur = seeds.copy()
    length = np.zeros(S, np.uint32)
    stop = np.full(S, MAX_STEPS, np.uint8)
    bases = np.zeros((S, L), np.uint8)
    tf = np.zeros((S, L), np.uint32)
    seedc = canon(seeds)
    act = np.arange(S)
    for _ in range(L):
        if act.shape[0] == 0:
            break
        c = cont(freq, cur[act], direction, cutoff)
        go = np.ones(act.shape[0], bool)
        dead = c["n"] == 0
        stop[act[dead]] = DEAD_END
        go &= ~dead
        if mode == UNITIG:
            br = go & (c["n"] > 1)
            stop[act[br]] = BRANCH
            go &= ~br
        nxt = neigh(cur[act], direction, c["best_base"])
        if mode == UNITIG:
            idx = np.nonzero(go)[0]
            back = cont(freq, nxt[idx], 1 - direction, cutoff)
            j = idx[back["n"] > 1]
            stop[act[j]] = JOIN
            go[j] = False
        lp = go & (canon(nxt) == seedc[act])
        stop[act[lp]] = LOOP
        go &= ~lp
        g = act[go]
        bases[g, length[g]] = LETTERS[c["best_base"][go]]
        tf[g, length[g]] = c["best_tf"][go]
        length[g] += 1
        cur[g] = nxt[go]
        act = g
    return bases, length, stop, tf, cur
