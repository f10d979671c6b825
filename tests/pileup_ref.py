"""Test-side restatement of the pile-up (a helper, not a conftest): the steps of threaded sequences merged into placements, the bases of
the reads counted at the contig positions, and the counts read out as polished bases, variant sites and per-contig depth, sequentially,
in plain Python / numpy. It restates the contract above the aix_pile_place_dev / aix_pileup_dev / aix_pile_call_dev declarations of
include/aindex_hip.h:

  place(offs, steps, offsets, max_gap=46, extend=22)                    -> the placement arrays, "n_place", "n_circular_steps"
  pile(seqs, places, offsets, bases, counts=None)                       -> "counts" uint32[4 B] (accumulated into a copy), "place_mism", "stats"
  call(offsets, bases, counts, min_depth=8, min_major_permille=700, min_alt_count=3, min_alt_permille=200)
                                                                        -> polished, n_changed, the variant arrays, depth_sum, uncovered

offs are the sequence offsets u64[M + 1], steps what seqthread_ref.thread returned, offsets / bases those of the graph. One step, one base
at a time; nothing here scans, and no difference array is used: every read base adds one to its cell. A violation of a validation is a
ValueError.
"""
import numpy as np

K = 23
PLACE_KEYS = ("seq_place_off", "place_unitig", "place_flag", "place_pos", "place_q0", "place_len", "place_steps")
PLACE_DTYPES = (np.uint64, np.uint32, np.uint8, np.uint32, np.uint32, np.uint32, np.uint32)
VAR_KEYS = ("var_unitig", "var_pos", "var_ref", "var_alt", "var_ref_count", "var_alt_count", "var_depth")
VAR_DTYPES = (np.uint32, np.uint32, np.uint8, np.uint8, np.uint32, np.uint32, np.uint32)
ACGT = b"ACGT"
_CODE = {65: 0, 67: 1, 71: 2, 84: 3}                               # upper-case A, C, G, T only


def _ints(a):
    return [int(v) for v in np.asarray(a).reshape(-1).tolist()]


def _check_offsets(offsets):
    off = _ints(offsets)
    if not off or off[0] != 0:
        raise ValueError("offsets start at 0")
    for u in range(len(off) - 1):
        if off[u + 1] < off[u] + K:
            raise ValueError("offsets ascend by at least 23")
    return off


def _check_csr(csr, M, total, what):
    c = _ints(csr)
    if len(c) != M + 1 or c[0] != 0 or c[M] != total or any(c[i + 1] < c[i] for i in range(M)):
        raise ValueError(what + " starts at 0, ascends and ends at its total")
    return c


def _check_seq_offs(offs):
    so = _ints(offs)
    if any(b < a or b - a >= 1 << 32 for a, b in zip(so, so[1:])):
        raise ValueError("sequence offsets ascend by less than 2^32")
    return so


def place(offs, steps, offsets, max_gap: int = 46, extend: int = 22) -> dict:
    so = _check_seq_offs(offs)
    M = len(so) - 1
    su, sp, sf, qf, ql = (_ints(steps[k]) for k in ("step_unitig", "step_pos", "step_flag", "q_first", "q_last"))
    T = len(su)
    sso = _check_csr(steps["seq_step_off"], M, T, "seq_step_off")
    off = _check_offsets(offsets)
    U = len(off) - 1
    for i in range(M):
        L = so[i + 1] - so[i]
        for t in range(sso[i], sso[i + 1]):
            u, p, a, b = su[t], sp[t], qf[t], ql[t]
            if u >= U:
                raise ValueError("a step on unitig U or beyond")
            if a > b or b + K > L:
                raise ValueError("a step outside its sequence")
            m = off[u + 1] - off[u] - (K - 1)
            if not sf[t] & 2 and not (b - a <= p < m if sf[t] & 1 else p + (b - a) < m):
                raise ValueError("a linear step outside its contig")
            if t > sso[i] and a <= ql[t - 1]:
                raise ValueError("steps that descend")
    spo, rows, n_circ = [0], [], 0
    for i in range(M):
        L = so[i + 1] - so[i]
        runs, cur = [], None                                       # [u, s, d, a_first, b_last, steps]
        for t in range(sso[i], sso[i + 1]):
            if sf[t] & 2:
                n_circ += 1
                cur = None
                continue
            u, s, a, b = su[t], sf[t] & 1, qf[t], ql[t]
            d = sp[t] + a + (K - 1) if s else sp[t] - a
            if cur is not None and cur[:3] == [u, s, d] and a - cur[4] - 1 <= max_gap:
                cur[4], cur[5] = b, cur[5] + 1
            else:
                cur = [u, s, d, a, b, 1]
                runs.append(cur)
        for j, (u, s, d, a, b, n) in enumerate(runs):
            Lu = off[u + 1] - off[u]
            last = b + K - 1                                       # the core is read bases [a, last]
            left = [extend, a, (Lu - 1 - (d - a)) if s else d + a]
            right = [extend, L - 1 - last, (d - last) if s else Lu - 1 - (d + last)]
            if j:
                left.append(a - (runs[j - 1][4] + K - 1) - 1)
            if j + 1 < len(runs):
                right.append(runs[j + 1][3] - last - 1)
            q0, q1 = a - max(0, min(left)), last + max(0, min(right))
            rows.append((u, s, (d - q1) if s else d + q0, q0, q1 - q0 + 1, n))
        spo.append(len(rows))
    cols = list(zip(*rows)) if rows else [[]] * 6
    out = {"seq_place_off": np.array(spo, dtype=np.uint64)}
    for k, dt, col in zip(PLACE_KEYS[1:], PLACE_DTYPES[1:], cols):
        out[k] = np.array(col, dtype=dt)
    out["n_place"], out["n_circular_steps"] = len(rows), n_circ
    return out


def pile(seqs, places, offsets, bases, counts=None) -> dict:
    seqs = [bytes(s) for s in seqs]
    M = len(seqs)
    pu, pf, pp, q0, ln = (_ints(places[k]) for k in PLACE_KEYS[1:6])
    Rn = len(pu)
    spo = _check_csr(places["seq_place_off"], M, Rn, "seq_place_off")
    off = _check_offsets(offsets)
    U, B = len(off) - 1, off[-1]
    text = bytes(np.asarray(bases, dtype=np.uint8).tobytes())
    if len(text) != B or any(c not in _CODE for c in text):
        raise ValueError("a contig byte that is not upper-case A, C, G or T")
    for i in range(M):
        for r in range(spo[i], spo[i + 1]):
            if pu[r] >= U or ln[r] < 1:
                raise ValueError("a placement on unitig U or beyond, or an empty one")
            if pp[r] + ln[r] > off[pu[r] + 1] - off[pu[r]] or q0[r] + ln[r] > len(seqs[i]):
                raise ValueError("a placement beyond its contig or its read")
    cnt = np.zeros(4 * B, np.uint32) if counts is None else np.array(counts, dtype=np.uint32).reshape(-1).copy()
    if cnt.shape[0] != 4 * B:
        raise ValueError("counts holds four cells per base")
    add = [0] * (4 * B)
    mism, stats = [0] * Rn, [0, 0, 0]
    for i in range(M):
        for r in range(spo[i], spo[i + 1]):
            g0 = off[pu[r]] + pp[r]
            for x in range(ln[r]):
                ch = seqs[i][q0[r] + x]
                g = g0 + ln[r] - 1 - x if pf[r] & 1 else g0 + x
                if ch not in _CODE:
                    stats[1] += 1
                    continue
                c = 3 - _CODE[ch] if pf[r] & 1 else _CODE[ch]
                add[4 * g + c] += 1
                stats[0] += 1
                if c != _CODE[text[g]]:
                    mism[r] += 1
                    stats[2] += 1
    cnt = ((cnt.astype(np.uint64) + np.array(add, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)      # counters wrap at 2^32
    return {"counts": cnt, "place_mism": np.array(mism, dtype=np.uint32), "stats": np.array(stats, dtype=np.uint64)}


def call(offsets, bases, counts, min_depth: int = 8, min_major_permille: int = 700, min_alt_count: int = 3, min_alt_permille: int = 200) -> dict:
    off = _check_offsets(offsets)
    U, B = len(off) - 1, off[-1]
    text = bytes(np.asarray(bases, dtype=np.uint8).tobytes())
    if len(text) != B or any(c not in _CODE for c in text):
        raise ValueError("a contig byte that is not upper-case A, C, G or T")
    cnt = _ints(counts)
    if len(cnt) != 4 * B:
        raise ValueError("counts holds four cells per base")
    polished = bytearray(text)
    rows, n_changed = [], 0
    depth_sum, uncovered = [0] * U, [0] * U
    for u in range(U):
        for g in range(off[u], off[u + 1]):
            c = cnt[4 * g:4 * g + 4]
            r = _CODE[text[g]]
            D = sum(c)
            alt = max((x for x in range(4) if x != r), key=lambda x: (c[x], -x))     # the largest count, ties to the smaller code
            if D >= min_depth and c[alt] > c[r] and 1000 * c[alt] >= min_major_permille * D:
                polished[g] = ACGT[alt]
                n_changed += 1
            if D >= min_depth and c[alt] >= min_alt_count and 1000 * c[alt] >= min_alt_permille * D:
                rows.append((u, g - off[u], text[g], ACGT[alt], c[r], c[alt], min(D, 0xFFFFFFFF)))
            depth_sum[u] += D
            uncovered[u] += D == 0
    cols = list(zip(*rows)) if rows else [[]] * 7
    out = {k: np.array(col, dtype=dt) for k, dt, col in zip(VAR_KEYS, VAR_DTYPES, cols)}
    out.update(polished=np.frombuffer(bytes(polished), dtype=np.uint8).copy(), n_changed=n_changed, total=len(rows),
               depth_sum=np.array(depth_sum, dtype=np.uint64), uncovered=np.array(uncovered, dtype=np.uint32))
    return out
