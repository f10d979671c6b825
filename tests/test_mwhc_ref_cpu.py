"""CPU: tests/mwhc_ref.py (the plain reference that tests/test_gpu_builder.py holds aix_builder_gpu.hip against) checked on its own: its seeds
against the golden `.pf` headers, its hash against the oracle, its header and status against the host builder, its `.pf` through the oracle's
evaluator, and the conditions that the GPU tests rely on (contested edges, retried seeds, bit-pair counts around a word and a rank block)."""
import numpy as np
import pytest

import mwhc_ref as R
import oracle_lib as O
from aindex_amd import _lib, builder

CASES = R.cases()
SWEEP = range(1, 34)


def _host(codes, k):
    """(status, pf) of the host builder"""
    try:
        return _lib.AIX_OK, builder.build_pf_codes(codes, k)
    except _lib.AixError as e:
        return e.status, None


_memo = {}


def _ref(name):
    if name not in _memo:
        _memo[name] = R.build(R.case_keys(name), CASES[name][0])
    return _memo[name]


def _bijection(tmp_path, pf, codes, k):
    path = str(tmp_path / "ref.pf")
    with open(path, "wb") as f:
        f.write(pf)
    m = O.OracleMphf(path)
    slots = sorted(m.lookup(row.tobytes()) for row in R.ascii_of_codes(codes, k))
    assert slots == list(range(codes.shape[0]))


def test_mt19937_64_matches_the_standard_and_the_golden_headers(gold):
    assert R.mt19937_64(5489, 10000)[-1] == 9981545732273789042            # the value the C++ standard fixes for the default-seeded engine
    s = R.seeds()
    assert len(s) == 64 and len(set(s)) == 64
    for name in ("small23", "graph23"):
        hdr = np.fromfile(f"{gold}/{name}/{name}.pf", dtype=np.uint64, count=4)
        assert int(hdr[2]) == s[1] == 5895889748689162540, name             # written by the compiled reference: its second draw, both times


@pytest.mark.parametrize("k", [1, 7, 8, 9, 13, 15, 16, 17, 23, 24, 25, 31, 32])
def test_numpy_hash_equals_the_oracle(k):
    codes = R.random_codes(k, min(500, 4 ** k), k)
    keys = R.ascii_of_codes(codes, k)
    for seed in (0, R.seeds()[0], R.seeds()[63], (1 << 64) - 1):
        for x, y in zip(R.jenkins_np(keys, seed), R.jenkins_oracle(keys, seed)):
            assert np.array_equal(x, y), (k, seed)


def test_ascii_rendering_and_revcomp():
    assert R.ascii_of_codes(np.array([0b00011011], dtype=np.uint64), 4).tobytes() == b"ACGT"
    assert R.ascii_of_codes(np.array([0b11], dtype=np.uint64), 3).tobytes() == b"AAT"
    c = R.random_codes(1, 100, 23)
    assert np.array_equal(R.revcomp_codes(R.revcomp_codes(c, 23), 23), c)
    assert R.ascii_of_codes(R.revcomp_codes(c[:1], 23), 23).tobytes() == R.ascii_of_codes(c[:1], 23).tobytes()[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))


@pytest.mark.parametrize("name", list(CASES))
def test_case_against_the_host_builder_and_the_oracle_evaluator(name, tmp_path):
    k, n, _ = CASES[name]
    codes = R.case_keys(name)
    assert codes.shape[0] == n and np.unique(codes).shape[0] == n and int(codes.max()) < 4 ** k
    st, pf, info = _ref(name)
    hst, hpf = _host(codes, k)
    assert st == hst, (name, info)
    if st != R.AIX_OK:
        assert st == R.AIX_ERR_CONFLICT and pf is None and info["trials"] == 64
        return
    D, B, W, Rk = R.dims(n)
    assert len(pf) == len(hpf) == 32 + 8 * (W + Rk)
    assert pf[:32] == hpf[:32]                                              # n, D, the seed that peeled (so the same number of trials), B
    assert np.frombuffer(pf[:32], dtype=np.uint64).tolist() == [n, D, R.seeds()[info["trials"] - 1], B]
    _bijection(tmp_path, pf, codes, k)
    # the order of the keys does not matter, nor does the hasher
    perm = np.random.default_rng(1).permutation(n)
    assert R.build(codes[perm], k)[1] == pf
    if n <= 5000:
        assert R.build(codes, k, hasher=R.jenkins_np)[1] == pf and R.build(codes, k, hasher=R.jenkins_oracle)[1] == pf


@pytest.mark.parametrize("n", list(SWEEP))
def test_small_n_sweep_against_the_host_builder(n, tmp_path):
    codes = R.sweep_keys(n)
    st, pf, info = R.build(codes, 23)
    hst, hpf = _host(codes, 23)
    assert st == hst, (n, info)
    if st == R.AIX_OK:
        assert pf[:32] == hpf[:32] and len(pf) == len(hpf)
        _bijection(tmp_path, pf, codes, 23)
        assert R.build(codes[::-1], 23)[1] == pf
    else:
        assert st == R.AIX_ERR_CONFLICT


def test_n2_is_a_conflict_and_so_is_a_duplicate():
    assert R.dims(1)[:2] == (1, 3) and R.dims(2)[:2] == (1, 3)
    c2 = R.sweep_keys(2)
    assert R.build(c2, 23)[0] == _host(c2, 23)[0] == R.AIX_ERR_CONFLICT     # both keys are the edge (0, 1, 2): nothing peels
    d = R.dup_keys()
    assert d.shape[0] == R.N_DUP and np.unique(d).shape[0] == R.N_DUP - 1
    st, pf, info = R.build(d, 23)
    assert (st, pf, info["trials"]) == (R.AIX_ERR_CONFLICT, None, 64)
    assert _host(d, 23)[0] == R.AIX_ERR_CONFLICT
    assert R.build(np.unique(d), 23)[0] == R.AIX_OK                          # the duplicate alone is what fails it


def test_the_inputs_hold_the_cases_that_matter():
    # the race that the hinge rule settles is met often: edges with two or three degree-1 vertices at the start of their round
    st, _, info = _ref("k23_main")
    assert st == R.AIX_OK and info["contested"] >= 1000 and info["rounds"] >= 5, info
    # a first seed that does not peel, so that the header's seed is seen to be the one that did
    retried = [(nm, _ref(nm)[2]["trials"]) for nm in CASES if _ref(nm)[0] == R.AIX_OK and _ref(nm)[2]["trials"] > 1]
    retried += [(n, t) for n in SWEEP for s, _, i in [R.build(R.sweep_keys(n), 23)] for t in [i["trials"]] if s == R.AIX_OK and t > 1]
    assert len(retried) >= 3, retried
    # bit-pair counts: the smallest, both sides of one 64-bit word and of one 512-pair rank block, and counts that end on either
    got = {nm: R.dims(CASES[nm][1])[1] for nm in CASES if nm.startswith("B")}
    assert got == {f"B{B}": B for B in R.BOUNDARY_B}
    assert R.dims(CASES["B3"][1])[1] == 3 and CASES["B3"][1] == 1
    Bs = sorted(got.values())
    assert max(b for b in Bs if b < 32) == 30 and min(b for b in Bs if b > 32) == 33          # 3 | B: 32 itself cannot occur
    assert max(b for b in Bs if b < 512) == 510 and min(b for b in Bs if b > 512) == 513      # nor can 512
    assert 96 in Bs and 96 % 32 == 0 and 1536 in Bs and 1536 % 512 == 0
    assert [R.dims(CASES[f"B{B}"][1])[2:] for B in (30, 33, 96, 510, 513, 1536)] == [(1, 1), (2, 1), (3, 1), (16, 1), (17, 2), (48, 3)]
    # every bit-pair count of the sweep
    assert {R.dims(n)[1] for n in SWEEP} >= {3, 6, 30, 33, 42}
    assert R.N_STRIDE2 > 16384 * 256 and R.dims(R.N_STRIDE2)[1] < 1 << 32


@pytest.mark.slow
def test_second_grid_stride_trip_size_against_the_host_builder(tmp_path):
    n = R.N_STRIDE2
    codes = R.random_codes(4242, n, 23, canonical=True)
    st, pf, info = R.build(codes, 23)
    hpf = builder.build_pf_codes(codes, 23)
    assert st == R.AIX_OK and pf[:32] == hpf[:32] and len(pf) == len(hpf), info
    path = str(tmp_path / "big.pf")
    with open(path, "wb") as f:
        f.write(pf)
    m = O.OracleMphf(path)
    sub = codes[:: 97]
    slots = [m.lookup(row.tobytes()) for row in R.ascii_of_codes(sub, 23)]
    assert len(set(slots)) == sub.shape[0] and max(slots) < n
    # all keys: every vertex value sum selects a distinct non-zero pair (the evaluator restated over numpy, whole set)
    hdr = np.frombuffer(pf[:32], dtype=np.uint64)
    D, B = int(hdr[1]), int(hdr[3])
    W = (B + 31) // 32
    words = np.frombuffer(pf[32:32 + 8 * W], dtype=np.uint64)
    pairs = ((words[:, None] >> (np.arange(32, dtype=np.uint64) * np.uint64(2))) & np.uint64(3)).reshape(-1)[:B].astype(np.int64)
    v = np.stack(R.edges(R.ascii_of_codes(codes, 23), int(hdr[2]), D, R.jenkins_np), axis=1)
    node = v[np.arange(n), pairs[v].sum(axis=1) % 3]
    assert (pairs[node] != 0).all() and np.unique(node).shape[0] == n and int((pairs != 0).sum()) == n
