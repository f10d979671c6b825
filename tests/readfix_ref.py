"""Test-side restatement of the read-cleaning semantics (a helper, not a conftest): plain scalar Python, one read at a time.

Everything is computed from one callable `freq(codes uint64[N]) -> uint32[N]` = PHASH_MAP::get_freq(uint64_t) (hash.hpp:123-140),
which debruijn_ref.oracle_freq or graph_cases.dict_freq supply. The whole profile is recomputed after every fix (the kernel updates
the windows that contain the fixed base only; the test is that they agree).

  profile()    READ::set_fm (read.hpp:286-307): fm per window, 0 for a window with a byte that is not upper-case A/C/G/T;
               weak iff fm <= true_errors (read.hpp:296, Settings::TRUE_ERRORS, settings.cpp:10)
  fix_read()   the two boundary rules, the log of struct Correction and the counters of struct CorrectionErrors (read.hpp:36-117),
               the span that cut_start_to / cut_end_from keep (read.hpp:324-343)
  fix_reads()  the layout of aix_reads_fix: records, log rows, the buffer fixed in place
"""
import numpy as np

import debruijn_ref as D

CLEAN, FIXED, PARTIAL, UNFIXED, SHORT, TOO_LONG, BAD_RANGE = range(7)
STATUS_NAMES = ("clean", "fixed", "partial", "unfixed", "short", "too_long", "bad_range")
MAX_LEN = 4096
REC_FIELDS = ("status", "weak_before", "weak_after", "fixes", "n0", "nM", "trim_start", "trim_len")
REC_DTYPE = np.dtype([(f, "<u4") for f in REC_FIELDS])
_ACGT = frozenset(b"ACGT")


def profile(freq, s, t):
    """solid[i] for the W = len(s) - 22 windows of the bytes s: valid(i) and get_freq(window i) > t. One freq call per profile."""
    W = len(s) - 22
    bad = [c not in _ACGT for c in s]
    nbad = sum(bad[:22])
    valid = []
    for i in range(W):
        nbad += bad[i + 22]
        valid.append(nbad == 0)
        nbad -= bad[i]
    idx = [i for i in range(W) if valid[i]]
    solid = [False] * W
    if idx:
        a = np.frombuffer(bytes(s), dtype=np.uint8)
        win = np.lib.stride_tricks.sliding_window_view(a, 23)[idx]
        tf = freq(D.encode(np.ascontiguousarray(win)))
        for i, f in zip(idx, tf.tolist()):
            solid[i] = f > t
    return solid


def _try(freq, s, t, p, lo, hi):
    """The bases b for which every window lo .. hi of s with s[p] := b is solid; [] without probing when s[p] is no ASCII letter."""
    if not (65 <= (s[p] & 0xDF) <= 90):
        return []
    ok = []
    for b in b"ACGT":
        z = bytearray(s[lo:hi + 23])
        z[p - lo] = b
        if all(profile(freq, z, t)):
            ok.append(b)
    return ok


def fix_read(freq, s, t=1, V=8, F=4):
    """(record tuple in REC_FIELDS order, [(pos, old byte)], final bytes) for one read given as bytes; 23 <= len(s) <= MAX_LEN."""
    s = bytearray(s)
    W = len(s) - 22
    solid = profile(freq, s, t)
    weak_before = W - sum(solid)
    log, n0, nM = [], 0, 0

    def attempt(p, lo, hi):
        nonlocal n0, nM, solid
        ok = _try(freq, s, t, p, lo, hi)
        if len(ok) == 1:
            log.append((p, s[p]))
            s[p] = ok[0]
            solid = profile(freq, s, t)                  # solid() is always that of the read as fixed so far
            return True
        if ok:
            nM += 1
        else:
            n0 += 1
        return False

    c = 1                                                 # phase R
    while len(log) < F:
        i = next((i for i in range(max(c, 1), W) if solid[i - 1] and not solid[i]), None)
        if i is None:
            break
        if not attempt(i + 22, i, min(i + V - 1, W - 1)):
            c = i + 1
    c = W - 2                                             # phase L
    while len(log) < F:
        i = next((i for i in range(min(c, W - 2), -1, -1) if not solid[i] and solid[i + 1]), None)
        if i is None:
            break
        if not attempt(i, max(i - V + 1, 0), i):
            c = i - 1
    weak_after = W - sum(solid)
    best, best_at, run = 0, 0, 0
    for i in range(W):
        run = run + 1 if solid[i] else 0
        if run > best:
            best, best_at = run, i - run + 1
    fixes = len(log)
    status = CLEAN if weak_before == 0 else FIXED if weak_after == 0 else PARTIAL if fixes else UNFIXED
    return (status, weak_before, weak_after, fixes, n0, nM, best_at if best else 0, best + 22 if best else 0), log, bytes(s)


def fix_reads(freq, buf, start, end, t=1, V=8, F=4, fix_pos=None, fix_old=None):
    """The layout of aix_reads_fix: (corrected copy of buf uint8[], rec REC_DTYPE[M], fix_pos uint32[M, F], fix_old uint8[M, F]); the
    log rows given (or zeros) keep what lies at or beyond `fixes`."""
    out = np.array(np.frombuffer(buf, dtype=np.uint8) if isinstance(buf, (bytes, bytearray)) else buf, dtype=np.uint8, copy=True)
    M = len(start)
    rec = np.zeros(M, dtype=REC_DTYPE)
    fix_pos = np.zeros((M, F), np.uint32) if fix_pos is None else np.array(fix_pos, dtype=np.uint32).reshape(M, F)
    fix_old = np.zeros((M, F), np.uint8) if fix_old is None else np.array(fix_old, dtype=np.uint8).reshape(M, F)
    for r in range(M):
        a, b = int(start[r]), int(end[r])
        if a > b or b > out.shape[0]:
            rec[r]["status"] = BAD_RANGE
        elif b - a < 23:
            rec[r]["status"] = SHORT
        elif b - a > MAX_LEN:
            rec[r]["status"] = TOO_LONG
        else:
            fields, log, fixed = fix_read(freq, out[a:b].tobytes(), t, V, F)
            rec[r] = fields
            out[a:b] = np.frombuffer(fixed, dtype=np.uint8)
            for j, (p, old) in enumerate(log):
                fix_pos[r, j], fix_old[r, j] = p, old
    return out, rec, fix_pos, fix_old
