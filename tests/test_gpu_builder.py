"""GPU: the MWHC builder (aix_builder_gpu.hip, aix_pf_build_codes_dev / builder.build_pf_codes_t) against tests/mwhc_ref.py, the plain
restatement of the same operation that tests/test_mwhc_ref_cpu.py checks on its own. Every comparison is exact: status, header and bytes.
The builder's output is a function of the key set (lowest-numbered degree-1 vertex is the hinge), so the bytes may be pinned."""
import ctypes as C
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import mwhc_ref as R
import oracle_lib as O
from aindex_amd import _lib, builder, counting, engine
from aindex_amd.engine import Index

vp = _lib.vp
CASES = R.cases()
_memo = {}


def _ref(name):
    """(status, pf, info) of the reference for a shared case, computed once"""
    if name not in _memo:
        _memo[name] = R.build(R.case_keys(name), CASES[name][0])
    return _memo[name]


def _dev(codes):
    import torch
    return torch.from_numpy(np.ascontiguousarray(codes).view(np.int64).copy()).cuda()


def _gpu(keys_t, k, what=""):
    """(status, pf) of the GPU builder; prints the time of the call"""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    try:
        st, pf = _lib.AIX_OK, builder.build_pf_codes_t(keys_t, k)
    except _lib.AixError as e:
        st, pf = e.status, None
    print(f"[gpu builder] {what} n={keys_t.numel()} k={k}: status {st}, {1e3 * (time.perf_counter() - t0):.1f} ms")
    return st, pf


def _host_status(codes, k):
    try:
        builder.build_pf_codes(codes, k)
        return _lib.AIX_OK
    except _lib.AixError as e:
        return e.status


def _raw(ptr, n, k, out=True, length=True, device=0):
    """aix_pf_build_codes_dev called directly -> (status, pf_out after, pf_len after); both start as canaries"""
    p, ln = vp(0x5A5A5A5A5A5A5A50), C.c_uint64(0xA5A5A5A5)
    st = _lib.lib().aix_pf_build_codes_dev(vp(ptr) if ptr else None, n, k, device, None, C.byref(p) if out else None, C.byref(ln) if length else None)
    if st == _lib.AIX_OK:
        _lib.lib().aix_free(p)
    return st, p.value, ln.value


@pytest.mark.parametrize("name", list(CASES))
def test_bytes_equal_the_reference(name):
    k = CASES[name][0]
    want_st, want, info = _ref(name)
    st, pf = _gpu(_dev(R.case_keys(name)), k, name)
    assert st == want_st, (name, info)
    assert pf == want, (name, info)                                           # k = 13 and 23 have hash paths of their own, every other k the generic one


def test_small_n_sweep():
    """n = 1..33 at k = 23: the status is the host builder's (n = 2 cannot peel: 64 trials, then AIX_ERR_CONFLICT), the bytes are the reference's"""
    seen = set()
    for n in range(1, 34):
        codes = R.sweep_keys(n)
        st, pf = _gpu(_dev(codes), 23, "sweep")
        assert st == _host_status(codes, 23), n
        want_st, want, info = R.build(codes, 23)
        assert st == want_st and pf == want, (n, info)
        seen.add(st)
    assert seen == {_lib.AIX_OK, _lib.AIX_ERR_CONFLICT}


def test_same_keys_same_bytes_whatever_the_stream_order_or_offset():
    import torch
    want_st, want, info = _ref("k23_main")
    assert want_st == R.AIX_OK and info["contested"] >= 1000                   # edges that two or three degree-1 vertices bid for in one round
    codes = R.case_keys("k23_main")
    keys = _dev(codes)
    a = _gpu(keys, 23, "default stream")[1]
    big = torch.randint(0, 1 << 62, (1 << 25,), dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    sorted_big = torch.sort(big)[0]                                            # queued on the default stream, runs beside the build
    with torch.cuda.stream(side):
        b = builder.build_pf_codes_t(keys, 23)
    torch.cuda.synchronize()
    assert bool((sorted_big[1:] >= sorted_big[:-1]).all())
    perm = np.random.default_rng(9).permutation(codes.shape[0])
    c = _gpu(_dev(codes[perm]), 23, "shuffled")[1]
    buf = torch.full((codes.shape[0] + 5,), -1, dtype=torch.int64, device="cuda")
    view = buf[3:3 + codes.shape[0]]
    view.copy_(keys)
    assert view.storage_offset() == 3 and view.data_ptr() % 16 == 8
    d = _gpu(view, 23, "offset view")[1]
    assert a == want and b == want and c == want and d == want
    assert bool((buf[:3] == -1).all()) and bool((buf[-2:] == -1).all()) and torch.equal(view, keys)   # the input is read only


def test_duplicate_key_is_a_conflict_and_leaves_nothing_behind():
    d = R.dup_keys()
    keys = _dev(d)
    with pytest.raises(_lib.AixError) as ei:
        builder.build_pf_codes_t(keys, 23)
    assert ei.value.status == _lib.AIX_ERR_CONFLICT
    st, p, ln = _raw(keys.data_ptr(), keys.numel(), 23)
    assert (st, p, ln) == (_lib.AIX_ERR_CONFLICT, 0x5A5A5A5A5A5A5A50, 0xA5A5A5A5)   # outputs untouched
    # a valid build in the same process afterwards is still the reference's
    assert _gpu(_dev(R.case_keys("k13")), 13, "after conflict")[1] == _ref("k13")[1]
    assert _gpu(_dev(np.unique(d)), 23, "without the duplicate")[1] == R.build(np.unique(d), 23)[1]


def test_arguments():
    import torch
    one = torch.tensor([27], dtype=torch.int64, device="cuda")
    ptr = one.data_ptr()
    untouched = (0x5A5A5A5A5A5A5A50, 0xA5A5A5A5)
    assert _raw(ptr, 1, 23)[0] == _lib.AIX_OK
    for args, kw in (((ptr, 0, 23), {}), ((ptr, 1, 0), {}), ((ptr, 1, 33), {}), ((ptr, 1, -1), {}), ((0, 1, 23), {}), ((ptr, 1, 23), {"out": False}),
                     ((ptr, 1, 23), {"length": False})):
        st, p, ln = _raw(*args, **kw)
        assert st == _lib.AIX_ERR_ARG and (p, ln) == untouched, (args, kw)
    # n or 3 D beyond 32 bits: refused before d_codes is read (the tensor holds ONE key) or the device is touched
    for n in (1 << 32, 3_500_000_000):
        D = R.dims(n)[0]
        assert n >> 32 or 3 * D >= 1 << 32
        st, p, ln = _raw(ptr, n, 23)
        assert st == _lib.AIX_ERR_UNSUPPORTED and (p, ln) == untouched, n
    assert _raw(ptr, 1, 23)[0] == _lib.AIX_OK
    assert one.item() == 27


def test_end_to_end_k23_every_key_equals_the_oracle(tmp_path):
    import torch
    codes = R.case_keys("k23_main")
    n = codes.shape[0]
    keys = _dev(codes)
    counts = torch.arange(1, n + 1, dtype=torch.int32, device="cuda")
    pf = builder.build_pf_codes_t(keys, 23)
    assert pf == _ref("k23_main")[1]
    path = str(tmp_path / "e2e.pf")
    with open(path, "wb") as f:
        f.write(pf)
    m = O.OracleMphf(path)
    kmers = R.ascii_of_codes(codes, 23)
    with Index.build_23_codes_t(pf, keys, counts) as ix:
        slots = ix.hash_ascii(kmers)
        assert np.array_equal(np.sort(slots), np.arange(n, dtype=np.uint64))
        want = np.array([m.lookup(row.tobytes()) for row in kmers], dtype=np.uint64)
        assert np.array_equal(slots, want)                                     # every key, not a prefix
        assert np.array_equal(ix.tf_array()[slots.astype(np.int64)], np.arange(1, n + 1, dtype=np.uint32))
        assert np.array_equal(ix.tf_ascii(kmers), np.arange(1, n + 1, dtype=np.uint32))


@pytest.mark.slow
def test_second_trip_of_the_grid_stride_loops():
    """n = 16384 * 256 + 4097 keys: every kernel's loop goes round a second time"""
    import torch
    n = R.N_STRIDE2
    g = engine.synth_genome_t(31, 4_400_000)
    keys_all, _ = counting.count_distinct_t(g, 23, _lib.CANON_TRUE_RC)
    assert keys_all.numel() >= n
    keys = keys_all[:n].contiguous()
    st, a = _gpu(keys, 23, "first")
    st2, b = _gpu(keys, 23, "second")
    assert st == st2 == _lib.AIX_OK and a == b
    codes = keys.cpu().numpy().view(np.uint64)
    assert a[:32] == builder.build_pf_codes(codes, 23)[:32]
    with Index.build_23_codes_t(a, keys, None) as ix:
        slots = ix.hash_ascii(R.ascii_of_codes(codes, 23))
    assert np.array_equal(np.sort(slots), np.arange(n, dtype=np.uint64))
    want_st, want, info = R.build(codes, 23)                                    # hashed by jenkins_np (checked against the oracle on the CPU)
    assert want_st == R.AIX_OK and a == want, info
