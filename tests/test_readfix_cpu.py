"""The test-side restatement of the read-cleaning rules (tests/readfix_ref.py) on hand-made cases. Every expected record, log and span
below was worked out by hand from the rules in include/aindex_hip.h, not computed. The reads are cut from a fixed random sequence whose
canonical 23-mers all have tf 5, served through graph_cases.dict_freq; t = 1, V = 8 unless a case says otherwise."""
import numpy as np
import pytest

import debruijn_ref as D
import graph_cases as G
import readfix_ref as R

RNG = np.random.default_rng(777)
GENOME = bytes(D.LETTERS[RNG.integers(0, 4, 600)])
ALT_AT = 375                                                     # a second allele of the locus GENOME[ALT_AT], in a copy of GENOME[300:450]
ALT = bytearray(GENOME[300:450])
ALT[ALT_AT - 300] = b"ACGT"[(b"ACGT".index(GENOME[ALT_AT]) + 1) % 4]


def _freq():
    w = [np.lib.stride_tricks.sliding_window_view(np.frombuffer(bytes(s), np.uint8), 23) for s in (GENOME, ALT)]
    codes = np.unique(D.canon(D.encode(np.ascontiguousarray(np.concatenate(w)))))
    return G.dict_freq(codes, np.full(codes.shape[0], 5, np.uint32))


FREQ = _freq()
TRUTH = GENOME[100:250]                                          # 150 bases, 128 windows


def _other(c, k=1):
    return b"ACGT"[(b"ACGT".index(c) + k) % 4]


def _with(read, edits):
    s = bytearray(read)
    for p, c in edits.items():
        s[p] = c
    return bytes(s)


def test_the_sequence_is_what_the_cases_assume():
    assert all(R.profile(FREQ, TRUTH, 1)) and len(R.profile(FREQ, TRUTH, 1)) == 128
    assert R.fix_read(FREQ, TRUTH) == ((R.CLEAN, 0, 0, 0, 0, 0, 0, 150), [], TRUTH)
    assert not any(R.profile(FREQ, TRUTH, 5))                    # tf 5 is weak at t = 5
    assert R.fix_read(FREQ, TRUTH, t=5)[0] == (R.UNFIXED, 128, 128, 0, 0, 0, 0, 0)


# position -> weak windows it makes: the windows max(p - 22, 0) .. min(p, 127)
@pytest.mark.parametrize("p,weak", [(0, 1), (21, 22), (22, 23), (23, 23), (127, 23), (149, 1)])
def test_one_substitution_is_fixed(p, weak):
    wrong = _other(TRUTH[p])
    rec, log, out = R.fix_read(FREQ, _with(TRUTH, {p: wrong}))
    assert out == TRUTH and log == [(p, wrong)]
    assert rec == (R.FIXED, weak, 0, 1, 0, 0, 0, 150)


def test_an_n_and_a_lower_case_base_are_fixed_left_to_right():
    low = bytes([TRUTH[100]]).lower()[0]
    rec, log, out = R.fix_read(FREQ, _with(TRUTH, {30: ord("N"), 100: low}))
    assert out == TRUTH and log == [(30, ord("N")), (100, low)]
    assert rec == (R.FIXED, 46, 0, 2, 0, 0, 0, 150)


def test_two_errors_five_apart_defeat_both_rules():
    s = _with(TRUTH, {60: _other(TRUTH[60]), 65: _other(TRUTH[65], 2)})
    rec, log, out = R.fix_read(FREQ, s)
    # windows 38 .. 65 are weak; R tries p = 60 over 38 .. 45 (43 .. 45 hold the other error), L tries p = 65 over 58 .. 65 (all hold 60)
    assert out == s and log == []
    assert rec == (R.UNFIXED, 28, 28, 0, 2, 0, 66, 62 + 22)


def test_two_solid_alleles_give_nM():
    truth = GENOME[300:450]
    third = next(c for c in b"ACGT" if c not in (truth[75], ALT[75]))
    s = _with(truth, {75: third})
    rec, log, out = R.fix_read(FREQ, s)
    assert out == s and log == []
    assert rec == (R.UNFIXED, 23, 23, 0, 0, 2, 0, 53 + 22)       # solid runs 0 .. 52 and 76 .. 127: the earlier, longer one
    assert R.fix_read(FREQ, bytes(ALT))[0][0] == R.CLEAN


def test_a_separator_in_the_range_is_never_written():
    calls = []

    def counting(codes):
        calls.append(len(codes))
        return FREQ(codes)

    s = _with(TRUTH, {60: ord("~")})
    rec, log, out = R.fix_read(counting, s)
    assert out == s and log == []
    assert rec == (R.UNFIXED, 23, 23, 0, 2, 0, 61, 67 + 22)
    assert len(calls) == 1                                       # the profile; a try on a byte that is no letter probes nothing
    for c in (ord("\n"), ord("@"), ord("["), ord("`"), ord("{"), 0, 0xC1):
        assert R.fix_read(FREQ, _with(TRUTH, {60: c}))[2][60] == c


def test_no_fixes_allowed_and_one_fix_allowed():
    s = _with(TRUTH, {60: _other(TRUTH[60])})
    assert R.fix_read(FREQ, s, F=0) == ((R.UNFIXED, 23, 23, 0, 0, 0, 61, 67 + 22), [], s)
    wrong = _other(TRUTH[30])
    s = _with(TRUTH, {30: wrong, 100: _other(TRUTH[100])})
    rec, log, out = R.fix_read(FREQ, s, F=1)
    assert out == _with(s, {30: TRUTH[30]}) and log == [(30, wrong)]
    assert rec == (R.PARTIAL, 46, 23, 1, 0, 0, 0, 78 + 22)       # windows 78 .. 100 stay weak
    rec, log, out = R.fix_read(FREQ, s, F=2)
    assert out == TRUTH and rec == (R.FIXED, 46, 0, 2, 0, 0, 0, 150) and [p for p, _ in log] == [30, 100]


def test_verify_bounds_the_windows_of_a_try():
    # errors at 60 and 70: window 48 is the first that holds 70. R tries p = 60 over 38 .. 38 + V - 1
    s = _with(TRUTH, {60: _other(TRUTH[60]), 70: _other(TRUTH[70])})
    assert R.fix_read(FREQ, s, V=10)[0] == (R.FIXED, 33, 0, 2, 0, 0, 0, 150)         # 38 .. 47 are clear of 70
    rec, log, out = R.fix_read(FREQ, s, V=11)                                        # 38 .. 48: n0 at R; L tries p = 70 over 60 .. 70, all hold 60
    assert rec == (R.UNFIXED, 33, 33, 0, 2, 0, 71, 57 + 22) and out == s


def test_the_shortest_reads():
    t23, t24, t45 = GENOME[100:123], GENOME[100:124], GENOME[100:145]
    assert R.fix_read(FREQ, t23) == ((R.CLEAN, 0, 0, 0, 0, 0, 0, 23), [], t23)
    s = _with(t23, {5: _other(t23[5])})                          # one window, no boundary
    assert R.fix_read(FREQ, s) == ((R.UNFIXED, 1, 1, 0, 0, 0, 0, 0), [], s)
    for p in (0, 23):                                            # one weak window beside one solid window
        wrong = _other(t24[p])
        assert R.fix_read(FREQ, _with(t24, {p: wrong})) == ((R.FIXED, 1, 0, 1, 0, 0, 0, 24), [(p, wrong)], t24)
    s = _with(t24, {10: _other(t24[10])})                        # both windows weak
    assert R.fix_read(FREQ, s) == ((R.UNFIXED, 2, 2, 0, 0, 0, 0, 0), [], s)
    for p, weak in ((0, 1), (44, 1), (21, 22), (23, 22)):
        wrong = _other(t45[p])
        assert R.fix_read(FREQ, _with(t45, {p: wrong})) == ((R.FIXED, weak, 0, 1, 0, 0, 0, 45), [(p, wrong)], t45)
    s = _with(t45, {22: _other(t45[22])})                        # every one of the 23 windows holds position 22
    assert R.fix_read(FREQ, s) == ((R.UNFIXED, 23, 23, 0, 0, 0, 0, 0), [], s)


def test_the_batch_layout():
    wrong = _other(TRUTH[40])
    reads = [GENOME[100:122], _with(TRUTH, {40: wrong}), GENOME[100:123]]
    buf = b"#".join(reads) + b"#" + b"A" * 4097
    start = np.array([0, 23, 174, 198, 50, 198], np.uint64)
    end = np.array([22, 173, 197, 198 + 4097, 40, len(buf) + 1], np.uint64)
    pos, old = np.full((6, 2), 0xEEEEEEEE, np.uint32), np.full((6, 2), 0xEE, np.uint8)
    out, rec, fp, fo = R.fix_reads(FREQ, buf, start, end, 1, 8, 2, pos, old)
    assert rec["status"].tolist() == [R.SHORT, R.FIXED, R.CLEAN, R.TOO_LONG, R.BAD_RANGE, R.BAD_RANGE]
    assert rec[1].tolist() == (R.FIXED, 23, 0, 1, 0, 0, 0, 150) and rec[0].tolist() == (R.SHORT, 0, 0, 0, 0, 0, 0, 0)
    assert fp.tolist() == [[0xEEEEEEEE] * 2, [40, 0xEEEEEEEE]] + [[0xEEEEEEEE] * 2] * 4
    assert fo.tolist() == [[0xEE] * 2, [wrong, 0xEE]] + [[0xEE] * 2] * 4
    diff = np.flatnonzero(out != np.frombuffer(buf, np.uint8))
    assert diff.tolist() == [23 + 40] and out[63] == TRUTH[40]
    assert pos[1, 0] == 0xEEEEEEEE                                # the caller's rows are copied, not written


def test_engine_and_list_surface_exist():
    """The public entry points of the feature, without a GPU: present, and refusing bad arguments before any device call."""
    from aindex_amd import _lib
    from aindex_amd.aindex import AIndex
    from aindex_amd.engine import Index
    assert {"aix_reads_fix", "aix_reads_fix_dev"} <= set(_lib.header_symbols()) and {"aix_reads_fix", "aix_reads_fix_dev"} <= set(_lib.SIGNATURES)
    assert _lib.readfix_dtype().itemsize == 32 and _lib.readfix_dtype().names == R.REC_DTYPE.names
    assert _lib.FIX_NAMES == R.STATUS_NAMES and _lib.READFIX_MAX_LEN == R.MAX_LEN
    for name in ("fix_reads", "fix_reads_t"):
        assert callable(getattr(Index, name))
    for name in ("correct_reads", "classify_reads", "correct_reads_file"):
        assert callable(getattr(AIndex, name))
    for v, f in ((0, 4), (17, 4), (8, 17), (8, -1)):
        with pytest.raises(ValueError):
            Index._fix_args(v, f)
