"""The index handle's resources over its life: what aix_index_info / aix_reads_info report after every step that allocates, attaches
or releases something (the byte ledger device_bytes and the owner flags), that a closed handle gives its device memory back, and
attachment over attachment. One seeded canonical 23-mer index (the recipe of test_gpu_parity's canon_case) and one 13-mer handle.
Every comparison is exact equality; no test provokes a failure on the device."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from aindex_amd import _lib, builder, synth
from aindex_amd.engine import Index

# Recorded with lifecycle() below on commit dfba76c ("Pile reads onto contigs: base counts, variant sites, polished consensus"),
# the parent of the commit that made the handle own its blocks, on an MI355X. OPEN is the full record after open; STEPS lists, step
# by step, the fields that change (everything else must stay as it was).
OPEN = {
    "23.k": 23, "23.device": 0, "23.n": 299978, "23.mphf_n": 299978, "23.hash_domain": 122991, "23.seed": 18006821046139946489,
    "23.bitpairs": 368973, "23.device_bytes": 11808080, "23.canonical_only": 1, "23.bucket_table": 1, "23.buckets": 74995,
    "23.bucket_unfiled_keys": 2492, "23.bucket_lanes": 8, "23.absence_filter_words": 74995, "23.minimizer_lines": 0, "23.minimizer_unfiled_keys": 0,
    "23.count23_backend": 0, "23.count23_passes": 0, "23.positions_backend": 0, "23.aindex_attached": 0, "23.ridx_on_device": 0,
    "23.aindex_entries": 0, "23.ridx_reads": 0, "13.k": 13, "13.device": 0, "13.n": 67108864, "13.mphf_n": 67108864, "13.hash_domain": 27514635,
    "13.seed": 18006821046139946489, "13.bitpairs": 82543905, "13.device_bytes": 1424721200, "13.canonical_only": 0, "13.bucket_table": 0,
    "13.buckets": 0, "13.bucket_unfiled_keys": 0, "13.bucket_lanes": 8, "13.absence_filter_words": 0, "13.minimizer_lines": 0,
    "13.minimizer_unfiled_keys": 0, "13.count23_backend": 0, "13.count23_passes": 0, "13.positions_backend": 0, "13.aindex_attached": 0,
    "13.ridx_on_device": 0, "13.aindex_entries": 0, "13.ridx_reads": 0, "23.reads": (0, 0), "13.reads": (0, 0),
}
STEPS = (
    ("early_exit", {"23.device_bytes": 12546032}),
    ("count13", {"13.device_bytes": 1425888048}),
    ("count23", {"23.device_bytes": 13778416, "23.count23_backend": 2, "23.count23_passes": 1}),
    ("binned", {}),
    ("aindex_owned", {"23.device_bytes": 18578072, "23.aindex_attached": 1, "23.aindex_entries": 299978}),
    ("ridx", {"23.device_bytes": 18582872, "23.ridx_on_device": 1, "23.ridx_reads": 200}),
    ("reads_owned", {"23.device_bytes": 18613072, "23.reads": (1, 30200)}),
    ("reads_detached", {"23.device_bytes": 18582872, "23.reads": (0, 0)}),
    ("reads_borrowed", {"23.reads": (2, 30200)}),
    ("detached", {"23.device_bytes": 13778416, "23.aindex_attached": 0, "23.ridx_on_device": 0, "23.aindex_entries": 0, "23.ridx_reads": 0, "23.reads": (0, 0)}),
)
ATTACH_STEPS = (
    ("aindex_owned", {"23.device_bytes": 16607736, "23.aindex_attached": 1, "23.aindex_entries": 299978}),
    ("aindex_borrowed", {"23.device_bytes": 11808080, "23.aindex_attached": 2}),
    ("aindex_owned_again", {"23.device_bytes": 16607736, "23.aindex_attached": 1}),
    ("reads_owned", {"23.device_bytes": 16637936, "23.reads": (1, 30200)}),
    ("reads_borrowed", {"23.device_bytes": 16607736, "23.reads": (2, 30200)}),
    ("reads_owned_again", {"23.device_bytes": 16637936, "23.reads": (1, 30200)}),
    ("ridx", {"23.device_bytes": 16642736, "23.ridx_on_device": 1, "23.ridx_reads": 200}),
)


@contextlib.contextmanager
def _env(**kw):
    saved = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def make_case(d):
    """the index files, the inputs of every step (host and device) under directory d"""
    from pf13 import pf13_path
    keys, counts = synth.canonical_distinct(synth.genome_codes(23, 300_000), 23)
    pf = builder.build_pf_codes(keys, 23)
    prefix = str(d / "canon")
    open(prefix + ".pf", "wb").write(pf)
    n = keys.shape[0]
    checker, tf = np.empty(n, dtype=np.uint64), np.empty(n, dtype=np.uint32)
    vp = _lib.vp
    pfa = np.frombuffer(pf, dtype=np.uint8)
    flatk = np.ascontiguousarray(synth.decode_kmers(keys, 23)).reshape(-1)
    _lib.check(_lib.lib().aix_index_scatter(pfa.ctypes.data_as(vp), pfa.shape[0], flatk.ctypes.data_as(vp), counts.ctypes.data_as(vp), n, 0,
                                            checker.ctypes.data_as(vp), tf.ctypes.data_as(vp)))
    checker.tofile(prefix + ".kmers.bin")
    tf.tofile(prefix + ".tf.bin")
    asc = synth.genome_ascii(23, 300_000)
    reads = synth.reads_plain(41, asc, 200, 150)                     # 30 200 bytes: four pieces of 8192 windows
    ridx = np.array([[r, 151 * r, 151 * r + 150] for r in range(200)], dtype=np.uint64)
    return {"prefix": prefix, "pf13": pf13_path(), "n": n, "reads": reads.tobytes(), "ridx": ridx,
            "indices": np.arange(n + 1, dtype=np.uint64), "positions": np.arange(1, n + 1, dtype=np.uint64),   # one occurrence per k-mer: a valid positions index
            "queries_t": torch.from_numpy(np.ascontiguousarray(synth.random_kmers_ascii(5, 70_001, 23)).reshape(-1).copy()).cuda(),
            "indices_t": torch.arange(n + 1, dtype=torch.int64, device="cuda"), "positions_t": torch.arange(1, n + 1, dtype=torch.int64, device="cuda"),
            "reads_t": torch.from_numpy(reads.copy()).cuda()}


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    return make_case(tmp_path_factory.mktemp("lifecycle"))


def _open(case):
    p = case["prefix"]
    return Index.open_23(p + ".pf", p + ".tf.bin", p + ".kmers.bin"), Index.open_13(case["pf13"], None)


def _snap(ix23, ix13):
    rec = {"23." + k: v for k, v in ix23.info.items()}
    rec.update({"13." + k: v for k, v in ix13.info.items()})
    rec["23.reads"], rec["13.reads"] = ix23.reads_info(), ix13.reads_info()
    return rec


def lifecycle(case, ix23, ix13):
    """The steps of a handle's life, (name, record) after each"""
    yield "open", _snap(ix23, ix13)
    ix23.set_early_exit(True)
    yield "early_exit", _snap(ix23, ix13)
    ix13.count13(case["reads"], _lib.FMT_PLAIN)
    yield "count13", _snap(ix23, ix13)
    with _env(AIX_COUNT23_HIST_MIN="0", AIX_COUNT23_PIECE="8192"):    # the histogram back end in four pieces: second stream and events
        ix23.count23_fixed(case["reads"], _lib.FMT_PLAIN, _lib.CANON_TRUE_RC)
    yield "count23", _snap(ix23, ix13)
    with _env(AIX_LOOKUP_BINNED_MIN="0"):
        ix23.tf_ascii_t(case["queries_t"])
        torch.cuda.synchronize()
    st = (C.c_uint64 * 4)()
    _lib.check(_lib.lib().aix_lookup_binned_stats(ix23._h, C.cast(st, _lib.vp)))
    assert st[0] + st[1] == 1                                        # the batch was a candidate: its one piece went through the gate
    yield "binned", _snap(ix23, ix13)
    ix23.attach_aindex(case["indices"], case["positions"])
    yield "aindex_owned", _snap(ix23, ix13)
    assert ix23.attach_ridx(case["ridx"])
    yield "ridx", _snap(ix23, ix13)
    ix23.attach_reads(case["reads"])
    yield "reads_owned", _snap(ix23, ix13)
    ix23.detach_reads()
    yield "reads_detached", _snap(ix23, ix13)
    ix23.attach_reads_t(case["reads_t"])
    yield "reads_borrowed", _snap(ix23, ix13)
    ix23.detach_reads()
    ix23.detach_aindex()
    yield "detached", _snap(ix23, ix13)


def attach_over_attach(case, ix23, ix13):
    """owned, borrowed, owned again: the positions index, then the reads; the caller closes with everything attached"""
    ix23.attach_aindex(case["indices"], case["positions"])
    yield "aindex_owned", _snap(ix23, ix13)
    ix23.attach_aindex_t(case["indices_t"], case["positions_t"])
    yield "aindex_borrowed", _snap(ix23, ix13)
    ix23.attach_aindex(case["indices"], case["positions"])
    yield "aindex_owned_again", _snap(ix23, ix13)
    ix23.attach_reads(case["reads"])
    yield "reads_owned", _snap(ix23, ix13)
    ix23.attach_reads_t(case["reads_t"])
    yield "reads_borrowed", _snap(ix23, ix13)
    ix23.attach_reads(case["reads"])
    yield "reads_owned_again", _snap(ix23, ix13)
    assert ix23.attach_ridx(case["ridx"])
    yield "ridx", _snap(ix23, ix13)


def _check(steps, first, deltas):
    want = dict(first)
    names = []
    for (name, got), (want_name, delta) in zip(steps, deltas):
        assert name == want_name
        want.update(delta)
        print(name, {k: got[k] for k in delta})
        assert got == want, (name, {k: (got[k], want[k]) for k in got if got[k] != want[k]})
        names.append(name)
    assert len(names) == len(deltas)
    return want


def test_ledger_is_pinned(case):
    """info (every field) and reads_info of both handles after each step equal what the parent commit reported."""
    ix23, ix13 = _open(case)
    try:
        _check(lifecycle(case, ix23, ix13), OPEN, (("open", {}),) + STEPS)
    finally:
        ix23.close()
        ix13.close()


def test_attach_over_attach_and_close_while_attached(case):
    """Attach owned, then borrowed, then owned again, for the positions index and for the reads: after each step the owner state and
    the ledger equal the parent's; the handle is closed with everything attached."""
    ix23, ix13 = _open(case)
    try:
        _check(attach_over_attach(case, ix23, ix13), OPEN, ATTACH_STEPS)
    finally:
        ix23.close()
        ix13.close()


def _free_after_cycle(case):
    ix23, ix13 = _open(case)
    held = ix23.info["device_bytes"]
    for _ in lifecycle(case, ix23, ix13):
        pass
    ix23.close()
    ix13.close()
    _lib.lib().aix_scratch_trim()
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0], held


def test_a_handle_gives_back_what_it_took(case):
    """Twelve cycles of open, the whole sequence, close in one process. Free device memory (after aix_scratch_trim) behind cycle 12
    is not below that behind cycle 2 by more than the device_bytes of the freshly opened 23-mer handle; cycle 1 pays for what the
    runtime allocates once. The margin is a condition, not a measurement: a leaked index-sized block per cycle exceeds it ten times
    over, while a leaked 4-byte flag is below the driver's allocation granularity and cannot be seen this way."""
    free, held = [], 0
    for _ in range(12):
        f, held = _free_after_cycle(case)
        free.append(f)
    print("free after each cycle:", free, "margin:", held)
    assert free[11] + held >= free[1]
