"""Small De Bruijn graphs for the fuzz tests (a helper, not a conftest): key sets built from sequences, so that k-mers have
neighbours, with the strands, tf values and seeds chosen to sit on the edges of get_freq (hash.hpp:123-140) and of the CONT rule
(debrujin.cpp:30-75, 121-167).

  make_graph_case(seed)        (codes uint64[n], tfs uint32[n], seeds uint64[S]), deterministic in `seed`
  write_graph_case(seed, dir)  the same as .pf / .kmers.bin / .tf.bin files under `dir`
  dict_freq(codes, tfs)        get_freq over a Python dict, as the `freq` callable of debruijn_ref
"""
import os

import numpy as np

import debruijn_ref as D

# equal values make ties, 2 .. 5 bracket a cutoff of 3, the last four sit around 2^31 and 2^32
TF_POOL = np.array([0, 0, 1, 2, 3, 3, 4, 5, 5, 5, 1000, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0xFFFFFFFF], dtype=np.uint64)
TF_ABOVE_3 = TF_POOL[TF_POOL > 3]
CIRCLE_PERIODS = (1, 2, 3, 24, 30)
# arms of the planted hubs: (tf of the arm's first k-mer ...); None = drawn from the pool. Two arms at or above 2^31 make the u32 sum wrap.
WRAP_ARMS = ((0x80000000, 0x80000000), (0xFFFFFFFF, 0xFFFFFFFF), (0xFFFFFFFF, 0x80000000), (0x80000000, 0xFFFFFFFF, 0x7FFFFFFF))


def _windows(seq):
    """codes of every 23-base window of a sequence of values 0..3"""
    w = np.lib.stride_tricks.sliding_window_view(np.asarray(seq, dtype=np.uint8), 23)
    return D.encode(D.LETTERS[w])


def _sequences(rng, seed):
    """(sequences, hubs): every window of every sequence is a key; hubs = (direction, code of the hub k-mer, tf per arm base) of the
    planted forks (NEXT) and joins (PREV) whose arms get chosen tf values."""
    base = lambda n: rng.integers(0, 4, int(n)).astype(np.uint8)
    seqs = [base(rng.integers(23, 121)) for _ in range(int(rng.integers(24, 41)))]
    hubs = []

    def star(direction, arm_tfs):
        # a stem of at least 23 bases and len(arm_tfs) arms that leave it (fork) or enter it (join) with different bases
        stem = base(rng.integers(23, 45))
        letters = rng.permutation(4)[: len(arm_tfs)]
        for b in letters:
            arm = np.concatenate([[b], base(rng.integers(4, 30))]).astype(np.uint8)
            seqs.append(np.concatenate([stem, arm]) if direction == D.NEXT else np.concatenate([arm[::-1], stem]))
        hub = _windows(stem[-23:] if direction == D.NEXT else stem[:23])[0]
        hubs.append((direction, int(hub), {int(b): t for b, t in zip(letters, arm_tfs)}))

    for direction in (D.NEXT, D.PREV):
        for _ in range(5):                                         # forks / joins with whatever tf the pool gives
            star(direction, (None, None))
        star(direction, WRAP_ARMS[(seed + direction) % len(WRAP_ARMS)])
        star(direction, WRAP_ARMS[(seed // 4 + 2 + direction) % len(WRAP_ARMS)])
        v = [int(x) for x in rng.choice(TF_POOL[TF_POOL > 0], 6)]
        lo = [int(x) for x in rng.integers(0, 4, 2)]
        star(direction, (v[0], v[0]))                              # ties for the maximum: 2, 3 and 4 arms, with and without a lower one
        star(direction, (v[1], v[1], min(lo[0], v[1])))
        star(direction, (v[2], v[2], v[2]))
        star(direction, (v[3], v[3], v[3], min(lo[1], v[3])))
        star(direction, (v[4], v[4], v[4], v[4]))
        star(direction, (5, 5, 3, 3) if seed % 2 else (4, 4, 4, 2))  # a tie that a cutoff of 3 widens or keeps
        star(direction, (0, 0, 0, 0) if seed % 2 else (3, 2, 1, 0))  # stored neighbours, all-zero quad (at cutoff 3 in the second form)
    circles = []
    for p in CIRCLE_PERIODS:                                       # every window of the endless repetition of a unit of p bases
        unit = base(p)
        if p == 1:
            unit[0] = (seed // 3) % 4                              # A * 23 (and C, G, T in turn) is its own successor
        while p > 1 and any(np.array_equal(unit, np.roll(unit, s)) for s in range(1, p)):
            unit = base(p)                                         # a unit with a shorter period is another case of this list
        circles.append(len(seqs))
        seqs.append(np.tile(unit, 23 // p + 2)[: p + 22])
    return seqs, hubs, circles


def make_graph_case(seed):
    rng = np.random.default_rng(7_000_000 + seed)
    mode = seed % 3
    seqs, hubs, circles = _sequences(rng, seed)
    table = {}                                                     # stored code -> tf, in the order met

    def draw(pool=TF_POOL):
        return int(pool[rng.integers(0, pool.shape[0])])

    for si, s in enumerate(seqs):
        # long circles survive a cutoff of 3 and hold no stored 0: otherwise a cycle of 24 or 30 keys is almost never walked round
        pool = TF_ABOVE_3 if (si in circles and s.shape[0] > 30) else TF_POOL
        w = _windows(s)
        for c, r in zip(w.tolist(), D.revcomp(w).tolist()):
            if c in table or r in table:
                continue
            # mode 0: the canonical strand (the fast path); 1: the strand met first; 2: either
            key = min(c, r) if mode == 0 or (mode == 2 and rng.random() < 0.5) else c
            table[key] = draw(pool)
    if mode != 0:                                                  # both strands stored, with different tf: the forward strand decides
        keys = np.array(list(table), dtype=np.uint64)
        for c, r in zip(keys.tolist(), D.revcomp(keys).tolist()):
            if rng.random() < 1 / 3 and r not in table:
                t = draw()
                while t == table[c]:
                    t = draw()
                table[r] = t
    for direction, hub, arms in hubs:                              # the tf a probe of the arm's first k-mer sees: forward strand, else the other
        for b, t in arms.items():
            if t is None:
                continue
            c = int(D.neigh(np.array([hub], np.uint64), direction, b)[0])
            table[c if c in table else int(D.revcomp(np.array([c], np.uint64))[0])] = t
    codes = np.array(list(table), dtype=np.uint64)
    order = np.argsort(codes)
    codes, tfs = codes[order], np.array(list(table.values()), dtype=np.uint64)[order].astype(np.uint32)
    if codes.shape[0] == 2:                                        # hash domain 1 is never peelable (also in the reference)
        codes, tfs = codes[:1], tfs[:1]
    ends = np.concatenate([_windows(s)[[0, -1]] for s in seqs])
    around = np.concatenate([D.neigh(ends, d, b) for d in (D.NEXT, D.PREV) for b in range(4)])
    seeds = np.concatenate([codes, D.revcomp(codes), around, rng.integers(0, 1 << 46, 600, dtype=np.uint64)])
    seeds = seeds[rng.permutation(seeds.shape[0])]
    high = rng.random(seeds.shape[0]) < 0.05                       # bits 46 .. 63 are ignored
    seeds[high] |= rng.integers(1, 1 << 18, int(high.sum()), dtype=np.uint64) << np.uint64(46)
    assert 1000 < codes.shape[0] < 10_000 and seeds.shape[0] <= 20_000
    return codes, tfs, seeds


def write_graph_case(seed, tmp):
    """(prefix, codes, tfs, seeds): the case as index files, built the way make_case of test_gpu_fuzz.py builds its own."""
    import oracle_lib as O
    from aindex_amd import builder
    codes, tfs, seeds = make_graph_case(seed)
    prefix = os.path.join(tmp, f"g{seed}")
    open(prefix + ".pf", "wb").write(builder.build_pf_codes(codes, 23))
    m = O.OracleMphf(prefix + ".pf")
    rc, checker, tf = O.index_scatter(m, np.ascontiguousarray(D.decode(codes)).reshape(-1), tfs)
    assert rc == 0
    checker.tofile(prefix + ".kmers.bin")
    tf.tofile(prefix + ".tf.bin")
    return prefix, codes, tfs, seeds


def dict_freq(codes, tfs):
    """get_freq (hash.hpp:123-140) over a dict: the forward strand, the reverse complement when that is not stored; a stored 0 is found."""
    table = dict(zip(codes.tolist(), tfs.tolist()))

    def freq(q):
        q = np.ascontiguousarray(q, dtype=np.uint64).reshape(-1)
        get = table.get
        return np.array([get(c, get(r, 0)) for c, r in zip(q.tolist(), D.revcomp(q).tolist())], dtype=np.uint32).reshape(-1)
    return freq
