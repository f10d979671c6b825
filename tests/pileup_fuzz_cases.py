"""Seeded inputs for the pile-up fuzz (a helper, not a conftest), valid by construction and small: the restatement takes one Python step
per read base. What each generator plants is listed with it; tests/test_pileup_fuzz_cpu.py asserts from the restatement's outputs that
the situations are reached, so an edit here cannot hollow out the GPU test (tests/test_gpu_pileup_fuzz.py).

  steps_case(seed)        SEEDS: contigs, sequences and step arrays for aix_pile_place_dev that no threading need have written
  placements_case(seed)   PLACEMENT_SEEDS: placement arrays for aix_pileup_dev that aix_pile_place_dev would not write, and prefilled counts
  cells_case()            cells for aix_pile_call_dev that no pile-up wrote: an enumerated palette, then random ones
  rc_twin(case)           the reverse complement of an array-level pile input: equal counts, place_mism and stats
  PLACE_PARAMS            (max_gap, extend);  CALL_PARAMS  threshold sets for the call
"""
import itertools

import numpy as np

K = 23
M32 = 0xFFFFFFFF
SEEDS = tuple(range(8))
PLACEMENT_SEEDS = tuple(range(6))
PLACE_PARAMS = ((46, 22), (0, 0), (1, 1), (23, 400), (M32, M32))
LOOSE = dict(min_depth=1, min_major_permille=500, min_alt_count=1, min_alt_permille=50)          # as in test_gpu_pileup.py
ZERO = dict(min_depth=0, min_major_permille=0, min_alt_count=0, min_alt_permille=0)             # every base a variant site: total == B
CALL_PARAMS = ({}, LOOSE, ZERO, dict(min_depth=M32), dict(LOOSE, min_major_permille=1000, min_alt_permille=1000),
               dict(LOOSE, min_major_permille=1001, min_alt_permille=1001), dict(LOOSE, min_alt_permille=1 << 31), dict(LOOSE, min_major_permille=1 << 31),
               dict(min_depth=M32, min_major_permille=M32, min_alt_count=M32, min_alt_permille=M32))
LENGTHS = (1, 2, 22, 23, 63, 64, 65, 255, 256, 257, 1000)
PALETTE = (0, 1, 2, 3, M32)
RANDOM_CELLS_SEED = 77
OVERFLOW_CELLS = ((M32, M32, 1, 1), (M32 - 1, M32, 2, 1))       # under the contig base A, alt C: D = 2^33 in both, so 2^31 D is 2^64 and wraps to 0
_ACGT = np.frombuffer(b"ACGT", np.uint8)
_COMP = bytes.maketrans(b"ACGT", b"TGCA")
_STEP_KEYS = ("step_unitig", "step_pos", "step_flag", "q_first", "q_last")
_STEP_DTYPES = (np.uint32, np.uint32, np.uint8, np.uint32, np.uint32)
_PLACE_KEYS = ("place_unitig", "place_flag", "place_pos", "place_q0", "place_len")
_PLACE_DTYPES = (np.uint32, np.uint8, np.uint32, np.uint32, np.uint32)
_NOISE = np.frombuffer(b"NnacgtRY-*\x00\x7f\x80\xff", np.uint8)


def _text(rng, n):
    return _ACGT[rng.integers(0, 4, int(n))]


def _csr(counts):
    out = np.zeros(len(counts) + 1, np.uint64)
    out[1:] = np.cumsum(counts)
    return out


def _fits(lens, u, p, s, w):
    """a linear step of w + 1 windows at p on contig u fits it"""
    m = lens[u] - (K - 1)
    return (w <= p < m) if s else (0 <= p and p + w < m)


def _random_rows(rng, lens, L):
    """valid steps of one sequence of L bytes: runs on one diagonal, near misses of a run, circular steps, fresh steps"""
    rows, prev, q, windows = [], None, 0, L - (K - 1)
    U = len(lens)
    while True:
        a = q + int(rng.choice((0, 0, 1, 2, 5, 23, 24, 46, 47, int(rng.integers(0, 60)))))
        w = int(rng.choice((0, 0, 1, 3, int(rng.integers(0, 30)))))
        if a + w >= windows:
            return rows
        kind, row = rng.random(), None
        if prev is not None and kind < 0.65:
            u, p0, s, a0 = prev
            d = p0 + a0 + (K - 1) if s else p0 - a0
            if 0.45 <= kind < 0.55:
                d += int(rng.choice((-1, 1)))
            elif kind >= 0.55:
                s ^= 1
            p = d - a - (K - 1) if s else d + a
            if _fits(lens, u, p, s, w):
                row = (u, p, s, a, a + w)
        elif 0.65 <= kind < 0.8:
            row = (int(rng.integers(0, U)), int(rng.integers(0, 1 << 32)), 2 | int(rng.integers(0, 2)), a, a + w)
        if row is None:
            u, s = int(rng.integers(0, U)), int(rng.integers(0, 2))
            m = lens[u] - (K - 1)
            w = min(w, m - 1)
            row = (u, int(rng.integers(w, m)) if s else int(rng.integers(0, m - w)), s, a, a + w)
        if not row[2] & 2:
            prev = (row[0], row[1], row[2], row[3])
        rows.append(row)
        q = row[4] + 1


def steps_case(seed: int) -> dict:
    """default_rng(1000 + seed). U of (2, 3, 7, 12, 20, 28, 35, 40) contigs of 23 to 600 bases: the last one holds 300 or more (the planted
    steps lie on it), one other exactly 23. About 200 sequences of 0 to 400 bytes with about 600 steps: first the planted ones (below,
    each a sequence of its own, shuffled among sequences without steps), then random ones. Flag bytes carry random bits 2 to 7. The read
    bytes follow the contig along every linear step, then 6 % of them are substituted or made N, lower case or another byte.
    Planted, with H = 40 free read bases in front and 60 free contig bases where nothing else is said:
      two steps on one (u, s, d) with gaps 46, 47, 0, 1, 2, 23, 24, forwards and backwards; a run of four steps (gaps 0, 0, 1);
      same u and d, opposite s, gap 5; same u and s, d + 1, gap 3; d = -38; a circular step between two steps one window apart on one
      diagonal; a circular step first and last; circular steps only; a neighbour on another contig 4 bases beyond a circular step, on
      either side; cores that overlap by 21 bases; for each side and orientation a placement whose only limit below 23 is the read's end
      (5), the contig's end (7) or the neighbour's core (9), and one with none; base 0 of contig 0 and the last base of the last contig."""
    rng = np.random.default_rng(1000 + seed)
    U = (2, 3, 7, 12, 20, 28, 35, 40)[seed % 8]
    lens = [int(x) for x in rng.integers(23, 601, U)]
    lu, ou = U - 1, 0
    lens[lu] = int(rng.integers(300, 601))
    lens[int(rng.integers(0, U - 1))] = 23
    Ll, H, C = lens[lu], 40, 25                                    # planted cores: 3 windows, 25 bases
    offsets = _csr(lens)
    bases = _text(rng, int(offsets[-1]))
    planted = []                                                   # (length, rows)

    def seq(rows, tail=H):
        planted.append((rows[-1][4] + K + tail, rows))

    for gap in (46, 47, 0, 1, 2, 23, 24):
        a1 = H + 4 + gap
        seq([(lu, 60, 0, H, H + 3), (lu, 60 + a1 - H, 0, a1, a1 + 2)])
        seq([(lu, 200, 1, H, H + 3), (lu, 200 - (a1 - H), 1, a1, a1 + 2)])
    seq([(lu, 30, 0, H, H + 1), (lu, 32, 0, H + 2, H + 2), (lu, 33, 0, H + 3, H + 6), (lu, 38, 0, H + 8, H + 9)])
    seq([(lu, 200 + H, 0, H, H + 2), (lu, 200 - (H + 8) - 22, 1, H + 8, H + 9)])
    seq([(lu, 70, 0, H, H + 2), (lu, 70 + 6 + 1, 0, H + 6, H + 7)])
    seq([(lu, 2, 0, H, H + 1)])
    seq([(lu, 50, 0, H, H + 1), (ou, 7, 2, H + 2, H + 2), (lu, 53, 0, H + 3, H + 5)])
    seq([(ou, 9, 3, 0, 0), (lu, 90, 1, H, H + 2), (lu, 1 << 31, 2, H + 9, H + 9)], tail=0)
    seq([(lu, 1, 2, 3, 4), (ou, M32, 3, 9, 9), (lu, 5, 2, 30, 41)])
    seq([(ou, 0, 0, H, H), (lu, 11, 2, H + 2, H + 3), (lu, 100, 0, H + 27, H + 29)])
    seq([(lu, 100, 1, H, H + 2), (lu, 11, 3, H + 4, H + 5), (ou, 0, 0, H + 2 + 27, H + 2 + 27)])
    seq([(ou, 0, 0, H, H), (lu, 120, 0, H + 1, H + 3)])
    for side, s, which in itertools.product("LR", (0, 1), ("extend", "read", "contig", "neighbour")):
        a = 62 if (side, which) == ("L", "neighbour") else 5 if (side, which) == ("L", "read") else 60
        tail = 5 if (side, which) == ("R", "read") else 60
        room = 7 if which == "contig" else 60                      # on the contig, at the side in question
        low = (side == "L") != bool(s)                             # that side is the contig's low end
        p = (room if low else Ll - C - room) + (2 if s else 0)
        rows = [(lu, p, s, a, a + 2)]
        if which == "neighbour":
            rows = [(ou, 0, 0, 30, 30)] + rows if side == "L" else rows + [(ou, 0, 0, a + C + 9, a + C + 9)]
        seq(rows, tail)
    seq([(0, 0, 0, H, H)])
    seq([(lu, Ll - K, 0, H, H)])
    lengths, rows_of = [], []
    order = rng.permutation(len(planted))
    for i in order:                                                # sequences without steps between sequences with steps
        lengths += [planted[i][0], int(rng.choice((0, 0, 10, 22, 23, 57)))]
        rows_of += [planted[i][1], []]
    n_steps = sum(len(r) for r in rows_of)
    while len(lengths) < 200 or n_steps < 600:
        L = int(rng.choice((0, 22, 23, 24, int(rng.integers(0, 401)), int(rng.integers(100, 401)))))
        rows = _random_rows(rng, lens, L) if rng.random() < 0.85 else []
        lengths.append(L)
        rows_of.append(rows)
        n_steps += len(rows)
    seqs = []
    for L, rows in zip(lengths, rows_of):
        read = _text(rng, L).copy()
        for u, p, f, a, b in rows:
            if f & 2:
                continue
            g0 = int(offsets[u]) + (p - (b - a) if f & 1 else p)     # backwards, p is where the first window lies: the span ends at p + 22
            span = bases[g0:g0 + b - a + K]
            read[a:b + K] = np.frombuffer(span.tobytes()[::-1].translate(_COMP), np.uint8) if f & 1 else span
        hit = rng.random(L) < 0.06
        noise = np.where(rng.random(L) < 0.5, _ACGT[rng.integers(0, 4, L)], _NOISE[rng.integers(0, _NOISE.shape[0], L)])
        seqs.append(np.where(hit, noise, read).astype(np.uint8).tobytes())
    flat = [r for rows in rows_of for r in rows]
    cols = list(zip(*flat))
    steps = {"seq_step_off": _csr([len(r) for r in rows_of])}
    for k, dt, col in zip(_STEP_KEYS, _STEP_DTYPES, cols):
        steps[k] = np.array(col, dtype=dt)
    steps["step_flag"] |= (rng.integers(0, 64, len(flat)) << 2).astype(np.uint8)
    return dict(seed=seed, U=U, offsets=offsets, bases=bases, seqs=seqs, offs=_csr([len(s) for s in seqs]), steps=steps)


def _mix(rng, n):
    """70 % upper-case bases, 30 % bytes over all 256 values"""
    return np.where(rng.random(n) < 0.7, _ACGT[rng.integers(0, 4, n)], rng.integers(0, 256, n)).astype(np.uint8)


def placements_case(seed: int) -> dict:
    """default_rng(2000 + seed). U of (1, 2, 40): one contig of 1037 bases or more, the others of 23 to 300; B is no multiple of 64.
    Sequences, in this order: an empty one; every byte value twice, placed forwards and backwards; one with a placement of every length
    of LENGTHS; an empty one; 256 consecutive placements of 1, 2 and 3 bases; 3000 placements of one base on one contig base, half of
    them showing its base; two placements that overlap in the read and on the contig, one read span laid forwards and backwards over the
    same contig bases, base 0 of contig 0 and the last base of the last contig; 20 random ones (a quarter empty) with 0 to 4 placements;
    three trailing ones without a placement. Placement flags carry random bits 1 to 7. counts is prefilled with random u32 values; at
    the base under the 3000 placements all four cells lie within 100 of 2^32, at every seventh base under the longest one within 2."""
    rng = np.random.default_rng(2000 + seed)
    U = (1, 2, 40)[seed % 3]
    lens = [int(x) for x in rng.integers(23, 301, U)]
    lu = (U - 1) if seed % 2 else 0
    lens[lu] = int(rng.integers(1037, 1700))
    if sum(lens) % 64 == 0:
        lens[lu] += 1
    offsets = _csr(lens)
    B = int(offsets[-1])
    bases = _text(rng, B)
    ref = (bases >> 1 & 3) ^ (bases >> 2 & 1)                      # A, C, G, T -> 0 .. 3
    seqs, per_seq = [], []                                         # per sequence: rows (u, flag, pos, q0, len)

    def anywhere(n, u=None):
        u = int(rng.integers(0, U)) if u is None else u
        n = min(n, lens[u])
        return u, int(rng.integers(0, lens[u] - n + 1)), n

    def add(read, rows=()):
        seqs.append(np.asarray(read, np.uint8).tobytes())
        per_seq.append(list(rows))

    add([])
    every = np.concatenate((rng.permutation(256), rng.permutation(256)))
    add(every, [(lu, 0, anywhere(256, lu)[1], 0, 256), (lu, 1, anywhere(256, lu)[1], 256, 256)])
    rows = []
    for i, n in enumerate(LENGTHS):
        rows.append((lu, i & 1, anywhere(n, lu)[1], int(rng.integers(0, 1300 - n + 1)), n))
    longest = rows[-1]
    add(_mix(rng, 1300), rows)
    add([])
    rows = []
    for i in range(256):
        u, pos, n = anywhere((1, 2, 3, 1, 3, 2, 2)[i % 7])
        rows.append((u, int(rng.integers(0, 2)), pos, int(rng.integers(0, 700 - n + 1)), n))
    add(_mix(rng, 700), rows)
    hot_pos = int(rng.integers(0, lens[lu]))
    hot = int(offsets[lu]) + hot_pos
    k = np.arange(3000)
    shown = np.where(k % 4 < 2, ref[hot], (ref[hot] + 1 + k % 3) % 4)              # the channel each of them adds to
    add(_ACGT[np.where(k & 1, 3 - shown, shown)], [(lu, int(i & 1), hot_pos, int(i), 1) for i in k])
    P, Q = anywhere(85, lu)[1], anywhere(50, lu)[1]
    add(_mix(rng, 120), [(lu, 0, P, 10, 60), (lu, 0, P + 25, 30, 60), (lu, 0, Q, 5, 50), (lu, 1, Q, 5, 50), (0, 1, 0, 100, 1), (U - 1, 0, lens[U - 1] - 1, 119, 1)])
    for _ in range(20):
        L = 0 if rng.random() < 0.25 else int(rng.integers(1, 201))
        rows = []
        for _ in range(int(rng.integers(0, 5)) if L else 0):
            u, pos, n = anywhere(int(rng.integers(1, L + 1)))
            rows.append((u, int(rng.integers(0, 2)), pos, int(rng.integers(0, L - n + 1)), n))
        add(_mix(rng, L), rows)
    for L in (0, 40, 0):
        add(_mix(rng, L))
    flat = [r for rows in per_seq for r in rows]
    places = {"seq_place_off": _csr([len(r) for r in per_seq])}
    for key, dt, col in zip(_PLACE_KEYS, _PLACE_DTYPES, zip(*flat)):
        places[key] = np.array(col, dtype=dt)
    places["place_flag"] |= (rng.integers(0, 128, len(flat)) << 1).astype(np.uint8)
    counts = rng.integers(0, 1 << 32, 4 * B, dtype=np.uint64).astype(np.uint32).reshape(B, 4)
    near = list(range(int(offsets[lu]) + longest[2], int(offsets[lu]) + longest[2] + 1000, 7))
    counts[near] = (M32 - rng.integers(0, 2, (len(near), 4))).astype(np.uint32)
    counts[hot] = (M32 - rng.integers(0, 100, 4)).astype(np.uint32)
    return dict(seed=seed, U=U, offsets=offsets, bases=bases, seqs=seqs, offs=_csr([len(s) for s in seqs]), places=places, counts=counts.reshape(-1), hot=hot)


def rc_twin(case: dict) -> dict:
    """every sequence reversed with A <-> T and C <-> G swapped (other bytes stay), q0' = L - q0 - len, flag ^ 1, pos as it is"""
    p = case["places"]
    L = np.repeat(np.diff(case["offs"]), np.diff(p["seq_place_off"]).astype(np.int64))
    twin = dict(p, place_flag=p["place_flag"] ^ np.uint8(1), place_q0=(L - p["place_q0"] - p["place_len"]).astype(np.uint32))
    return dict(case, seqs=[s[::-1].translate(_COMP) for s in case["seqs"]], places=twin)


def cells_case() -> dict:
    """B = 5000 bases. Bases 0 .. 2499: every cell over PALETTE^4 (in the order of itertools.product) under the contig base A, then C, G
    and T; enumerated, no seed. Bases 2500 .. 4999: cells drawn by default_rng(RANDOM_CELLS_SEED) over {0 .. 9, 2^16, 2^31, 2^32 - 2,
    2^32 - 1} under random contig bases, with OVERFLOW_CELLS at 2517 and 2518 under A. Contigs of 25, 1000, 23, 23, 24 and then 23 to 90
    bases: waves of 64 bases straddle one, two and three contig boundaries (1025, 1048 and 1071 lie in one), and the contig of 1000 sums
    to a depth beyond 2^32."""
    rng = np.random.default_rng(RANDOM_CELLS_SEED)
    cells = np.array(list(itertools.product(PALETTE, repeat=4)) * 4, dtype=np.uint64)
    values = np.array(list(range(10)) + [1 << 16, 1 << 31, M32 - 1, M32], dtype=np.uint64)
    cells = np.concatenate((cells, values[rng.integers(0, values.shape[0], (2500, 4))]))
    bases = np.concatenate((np.repeat(_ACGT, 625), _ACGT[rng.integers(0, 4, 2500)]))
    literal = (2517, 2518)
    for g, cell in zip(literal, OVERFLOW_CELLS):
        cells[g], bases[g] = cell, ord("A")
    lens = [25, 1000, 23, 23, 24]
    left = 5000 - sum(lens)
    while left:
        n = int(rng.integers(23, 91))
        n = left if left <= 90 else left - 23 if left - n < 23 else n
        lens.append(n)
        left -= n
    return dict(U=len(lens), offsets=_csr(lens), bases=bases.astype(np.uint8), counts=cells.astype(np.uint32).reshape(-1), literal=literal)
