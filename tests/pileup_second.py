"""A second opinion on the pile-up (a helper, not a conftest): place, pile and call written from the contract block above
aix_pile_place_dev in include/aindex_hip.h alone, on whole numpy arrays. It shares no code with tests/pileup_ref.py and works the other
way round: where the restatement walks one step, one read base and one cell at a time, this one computes every step, every base of the
flat space of piled bases and every cell at once (shifted comparisons, np.bincount over flat indices, row-wise argmax). Signatures and
result dicts are those of pileup_ref. It validates nothing: its inputs (tests/pileup_fuzz_cases.py) are valid by construction and have
passed the restatement's checks by the time the two are compared.

Every function takes mutant=None or one name of MUTANTS: a near miss of the rule. tests/test_pileup_fuzz_cpu.py shows that each of them
changes an output on some input of the fuzz, which is the evidence that a kernel wrong in that way would fail the GPU test.
"""
import numpy as np

K = 23
PLACE_KEYS = ("seq_place_off", "place_unitig", "place_flag", "place_pos", "place_q0", "place_len", "place_steps")
PLACE_DTYPES = (np.uint64, np.uint32, np.uint8, np.uint32, np.uint32, np.uint32, np.uint32)
VAR_KEYS = ("var_unitig", "var_pos", "var_ref", "var_alt", "var_ref_count", "var_alt_count", "var_depth")
VAR_DTYPES = (np.uint32, np.uint32, np.uint8, np.uint8, np.uint32, np.uint32, np.uint32)

PLACE_MUTANTS = ("gap_below_max_gap",                             # merge on gap < max_gap
                 "merge_across_orientation",                      # merge without comparing orientation
                 "backward_diagonal_21",                          # backward diagonal p + a + 21
                 "circular_keeps_the_merge",                      # a circular step does not end a merge
                 "neighbour_is_the_adjacent_step",                # the neighbour is the adjacent step even when it is circular
                 "clip_at_the_extended_span",                     # the extension is clipped at the neighbour's extended span instead of its core
                 "negative_limit_kept")                           # a negative limit is not clamped to 0
PILE_MUTANTS = ("backward_not_complemented", "backward_at_pos_plus_x", "lower_case_counted", "other_byte_on_the_contig_channel", "counters_saturate")
CALL_MUTANTS = ("ties_to_the_larger_code", "polish_on_equal_counts", "depth_in_32_bits", "var_depth_not_clipped", "products_wrap_at_2_64")
MUTANTS = PLACE_MUTANTS + PILE_MUTANTS + CALL_MUTANTS

_BIG = np.int64(1) << 62
_CODE = np.full(256, -1, np.int64)
_CODE[[65, 67, 71, 84]] = (0, 1, 2, 3)
_CODE_LOWER = _CODE.copy()
_CODE_LOWER[[97, 99, 103, 116]] = (0, 1, 2, 3)
_ACGT = np.frombuffer(b"ACGT", np.uint8)


def _i64(a):
    return np.asarray(a).reshape(-1).astype(np.int64)


def _owner(csr, n):
    """the entry of a CSR that holds each of its n items"""
    return np.repeat(np.arange(csr.shape[0] - 1, dtype=np.int64), np.diff(csr)) if n else np.zeros(0, np.int64)


def place(offs, steps, offsets, max_gap: int = 46, extend: int = 22, mutant=None) -> dict:
    assert mutant is None or mutant in PLACE_MUTANTS
    so, off, sso = _i64(offs), _i64(offsets), _i64(steps["seq_step_off"])
    su, sp, sf, a, b = (_i64(steps[k]) for k in ("step_unitig", "step_pos", "step_flag", "q_first", "q_last"))
    M, T = so.shape[0] - 1, su.shape[0]
    seq = _owner(sso, T)
    lin, s = (sf & 2) == 0, sf & 1
    d = np.where(s == 1, sp + a + (21 if mutant == "backward_diagonal_21" else 22), sp - a)
    t = np.arange(T, dtype=np.int64)
    # the step each step is compared with: the one in front of it; for the mutant, the last linear one in front of it
    prev = t - 1
    if mutant == "circular_keeps_the_merge" and T:
        prev = np.maximum.accumulate(np.where(lin, t, -1))
        prev = np.concatenate(([-1], prev[:-1]))
    ok = prev >= 0
    pv = np.where(ok, prev, 0)
    gap = a - b[pv] - 1
    merged = ok & (seq[pv] == seq) & lin & lin[pv] & (su[pv] == su) & (d[pv] == d) & ((gap < max_gap) if mutant == "gap_below_max_gap" else (gap <= max_gap))
    if mutant != "merge_across_orientation":
        merged &= s[pv] == s
    head = lin & ~merged
    first = np.flatnonzero(head)                                  # the first step of every placement, in step order
    R = first.shape[0]
    li = np.flatnonzero(lin)
    pid = np.cumsum(head)[li] - 1                                 # the placement of every linear step
    n_steps = np.bincount(pid, minlength=R).astype(np.int64)
    last_step = np.zeros(R, np.int64)
    last_step[pid] = li                                           # ascending writes: the last one stays
    pseq, u, ps, pd = seq[first], su[first], s[first], d[first]
    ca, cl = a[first], b[last_step] + (K - 1)                     # the core: read bases [ca, cl]
    L, Lu = (so[1:] - so[:-1])[pseq], (off[1:] - off[:-1])[u]
    r = np.arange(R, dtype=np.int64)
    # the neighbours among the placements of the same sequence, measured from their cores
    has_l = (r > 0) & (pseq[np.maximum(r - 1, 0)] == pseq)
    has_r = (r + 1 < R) & (pseq[np.minimum(r + 1, R - 1)] == pseq) if R else has_l
    nb_l = np.where(has_l, ca - cl[np.maximum(r - 1, 0)] - 1, _BIG)
    nb_r = np.where(has_r, ca[np.minimum(r + 1, R - 1)] - cl - 1, _BIG) if R else nb_l
    if mutant == "neighbour_is_the_adjacent_step":
        tl, tr = first - 1, last_step + 1
        al = (tl >= 0) & (seq[np.maximum(tl, 0)] == pseq)
        ar = (tr < T) & (seq[np.minimum(tr, T - 1)] == pseq)
        nb_l = np.where(al, ca - (b[np.maximum(tl, 0)] + K - 1) - 1, _BIG)
        nb_r = np.where(ar, a[np.minimum(tr, T - 1)] - cl - 1, _BIG)
    ext = np.int64(extend)

    def grown(nl, nr):
        left = np.minimum(np.minimum(ext, ca), np.minimum(np.where(ps == 1, Lu - 1 - (pd - ca), pd + ca), nl))
        right = np.minimum(np.minimum(ext, L - 1 - cl), np.minimum(np.where(ps == 1, pd - cl, Lu - 1 - (pd + cl)), nr))
        if mutant != "negative_limit_kept":
            left, right = np.maximum(left, 0), np.maximum(right, 0)
        return ca - left, cl + right

    q0, q1 = grown(nb_l, nb_r)
    if mutant == "clip_at_the_extended_span" and R:
        q0, q1 = grown(np.where(has_l, ca - q1[np.maximum(r - 1, 0)] - 1, _BIG), np.where(has_r, q0[np.minimum(r + 1, R - 1)] - cl - 1, _BIG))
    pos = np.where(ps == 1, pd - q1, pd + q0)
    out = {"seq_place_off": np.concatenate(([0], np.cumsum(np.bincount(pseq, minlength=M))))[:M + 1].astype(np.uint64)}
    for k, dt, col in zip(PLACE_KEYS[1:], PLACE_DTYPES[1:], (u, ps, pos, q0, q1 - q0 + 1, n_steps)):
        out[k] = col.astype(dt)
    out["n_place"], out["n_circular_steps"] = int(R), int((~lin).sum())
    return out


def pile(seqs, places, offsets, bases, counts=None, mutant=None) -> dict:
    assert mutant is None or mutant in PILE_MUTANTS
    seqs = [bytes(x) for x in seqs]
    flat = np.frombuffer(b"".join(seqs), np.uint8)
    so = np.concatenate(([0], np.cumsum([len(x) for x in seqs]))).astype(np.int64)
    off, text = _i64(offsets), np.asarray(bases, dtype=np.uint8).reshape(-1)
    spo = _i64(places["seq_place_off"])
    pu, pf, pp, q0, ln = (_i64(places[k]) for k in PLACE_KEYS[1:6])
    R, B = pu.shape[0], int(off[-1])
    total = int(ln.sum())
    # the flat space of piled bases: base i is read base x of placement r
    r = np.repeat(np.arange(R, dtype=np.int64), ln)
    x = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(ln) - ln, ln)
    back = (pf & 1)[r] == 1
    byte = flat[(so[_owner(spo, R)] + q0)[r] + x] if total else np.zeros(0, np.uint8)
    g0 = (off[pu] + pp)[r]
    g = g0 + x if mutant == "backward_at_pos_plus_x" else np.where(back, g0 + ln[r] - 1 - x, g0 + x)
    code = (_CODE_LOWER if mutant == "lower_case_counted" else _CODE)[byte]
    counted = code >= 0
    if mutant != "backward_not_complemented":
        code = np.where(back, 3 - code, code)
    ref = _CODE[text]
    add = np.bincount((4 * g + code)[counted], minlength=4 * B).astype(np.uint64)
    if mutant == "other_byte_on_the_contig_channel":
        add += np.bincount((4 * g + ref[g])[~counted], minlength=4 * B).astype(np.uint64)
    differs = counted & (code != ref[g])
    mism = np.bincount(r[differs], minlength=R)
    cnt = np.zeros(4 * B, np.uint64) if counts is None else np.asarray(counts).reshape(-1).astype(np.uint64)
    cnt = cnt + add
    cnt = np.minimum(cnt, np.uint64(0xFFFFFFFF)) if mutant == "counters_saturate" else cnt & np.uint64(0xFFFFFFFF)
    return {"counts": cnt.astype(np.uint32), "place_mism": mism.astype(np.uint32),
            "stats": np.array([int(counted.sum()), int((~counted).sum()), int(differs.sum())], dtype=np.uint64)}


def _reaches(a1000, permille, D, wrap):
    """1000 c[alt] >= permille D per cell, exactly: 64-bit arithmetic where the largest product stays below 2^63, Python integers beyond"""
    if not wrap and (D.shape[0] == 0 or permille * int(D.max()) < 1 << 63):
        return a1000 >= np.uint64(permille) * D
    prod = [permille * v for v in D.tolist()]
    if wrap:
        prod = [v & ((1 << 64) - 1) for v in prod]
    return np.array([x >= y for x, y in zip(a1000.tolist(), prod)], dtype=bool)


def call(offsets, bases, counts, min_depth: int = 8, min_major_permille: int = 700, min_alt_count: int = 3, min_alt_permille: int = 200, mutant=None) -> dict:
    assert mutant is None or mutant in CALL_MUTANTS
    off, text = _i64(offsets), np.asarray(bases, dtype=np.uint8).reshape(-1)
    U, B = off.shape[0] - 1, int(off[-1])
    c = np.asarray(counts).reshape(B, 4).astype(np.int64)         # a count is below 2^32
    row = np.arange(B)
    r = _CODE[text]
    D = c.sum(axis=1).astype(np.uint64)                           # below 2^34
    if mutant == "depth_in_32_bits":
        D &= np.uint64(0xFFFFFFFF)
    others = c.copy()
    others[row, r] = -1
    alt = 3 - np.argmax(others[:, ::-1], axis=1) if mutant == "ties_to_the_larger_code" else np.argmax(others, axis=1)      # argmax: the first of equals
    c_ref, c_alt = c[row, r], c[row, alt]
    a1000 = (1000 * c_alt).astype(np.uint64)                      # below 2^42
    wrap = mutant == "products_wrap_at_2_64"
    deep = D >= np.uint64(min_depth)
    above = (c_alt >= c_ref) if mutant == "polish_on_equal_counts" else (c_alt > c_ref)
    polish = deep & above & _reaches(a1000, min_major_permille, D, wrap)
    variant = deep & (c_alt >= min_alt_count) & _reaches(a1000, min_alt_permille, D, wrap)
    polished = np.where(polish, _ACGT[alt], text).astype(np.uint8)
    g = np.flatnonzero(variant)
    vu = np.searchsorted(off, g, side="right") - 1
    depth = D[g] & np.uint64(0xFFFFFFFF) if mutant == "var_depth_not_clipped" else np.minimum(D[g], np.uint64(0xFFFFFFFF))
    out = {k: col.astype(dt) for k, dt, col in zip(VAR_KEYS, VAR_DTYPES, (vu, g - off[vu], text[g], _ACGT[alt[g]], c_ref[g], c_alt[g], depth))}
    starts = off[:-1]
    out.update(polished=polished, n_changed=int(polish.sum()), total=int(g.shape[0]),
               depth_sum=np.add.reduceat(D, starts).astype(np.uint64) if U else np.zeros(0, np.uint64),
               uncovered=np.add.reduceat((D == 0).astype(np.int64), starts).astype(np.uint32) if U else np.zeros(0, np.uint32))
    return out
