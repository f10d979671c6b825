"""The calling idioms the Python layer is written in, without a GPU and without the library: the grow-and-retry protocol of
aindex_amd._calls (driven by a fake entry point on CPU tensors) and the batching generator of AIndex (CPU tensors, a limit of a few
dozen bytes)."""
import numpy as np
import pytest
import torch

from aindex_amd import _calls, _lib
from aindex_amd.aindex import AIndex

DTYPES = (torch.int32, torch.int64, torch.uint8)


class FakeEntry:
    """an entry point that reports `total` entries and records what it was called with"""

    def __init__(self, total: int, status: int = 0):
        self.total, self.status, self.calls = total, status, []

    def __call__(self, pointers, cap, total_ref):
        self.calls.append((list(pointers), cap))
        total_ref._obj.value = self.total
        return self.status


def grow(total: int, hint):
    fake = FakeEntry(total)
    outs, got = _calls.grow_retry("aix_fake_dev", DTYPES, "cpu", hint, fake)
    assert got == total and [o.dtype for o in outs] == list(DTYPES) and all(o.shape == (total,) for o in outs)
    return fake.calls


def test_nothing_to_report_is_one_sizing_pass():
    (pointers, cap), = grow(0, 0)
    assert cap == 0 and pointers == [None] * len(DTYPES)


def test_no_hint_sizes_then_fills_at_exactly_the_total():
    (p0, cap0), (p1, cap1) = grow(5, 0)
    assert cap0 == 0 and p0 == [None] * len(DTYPES)
    assert cap1 == 5 and all(p is not None and p.value for p in p1) and len({p.value for p in p1}) == len(DTYPES)


def test_a_large_enough_hint_is_one_pass_cut_to_the_total():
    (pointers, cap), = grow(5, 8)
    assert cap == 8 and all(p is not None and p.value for p in pointers)


def test_a_hint_of_exactly_the_total_is_one_pass():
    (pointers, cap), = grow(5, 5)
    assert cap == 5 and all(p is not None and p.value for p in pointers)


def test_a_hint_below_the_total_is_retried_at_the_total():
    (_, cap0), (_, cap1) = grow(5, 3)
    assert (cap0, cap1) == (3, 5)


def test_a_negative_hint_is_no_hint():
    assert [cap for _, cap in grow(0, -7)] == [0]
    (p0, cap0), (_, cap1) = grow(5, -1)
    assert (cap0, cap1) == (0, 5) and p0 == [None] * len(DTYPES)


def test_a_failing_entry_point_raises_under_its_symbol():
    fake = FakeEntry(5, status=3)
    with pytest.raises(_lib.AixError, match="aix_fake_dev") as e:
        _calls.grow_retry("aix_fake_dev", DTYPES, "cpu", 0, fake)
    assert e.value.status == 3 and len(fake.calls) == 1


# ---- AIndex._batches ---------------------------------------------------------------------------------------------
LENGTHS = [7, 12, 9, 30, 3, 3, 11]                                  # running sizes 7 19 28 | 30 | 3 6 17 against a limit of 24
SEQS = [bytes([65 + i]) * n for i, n in enumerate(LENGTHS)]


def batches(seqs, limit, even):
    got = list(AIndex._batches(seqs, "cpu", limit, even))
    for data, offs in got:
        assert data.dtype == torch.uint8 and offs.dtype == torch.int64 and offs[0] == 0 and offs[-1] == data.numel()
    lens = [np.diff(offs.numpy()).tolist() for _, offs in got]
    assert [n for b in lens for n in b] == [len(s) for s in seqs]                       # the offsets reproduce the input lengths
    assert b"".join(bytes(data.numpy()) for data, _ in got) == b"".join(seqs)
    return [len(b) for b in lens]


def test_a_batch_closes_with_the_sequence_that_reaches_the_limit():
    assert batches(SEQS, 24, False) == [3, 1, 3]
    assert batches(SEQS, 19, False) == [2, 2, 3]                   # reaching the limit exactly closes too; the last batch stays below it


def test_with_the_even_rule_a_batch_closes_on_an_even_count_only():
    assert batches(SEQS, 24, True) == [4, 3]                        # 28 bytes at three sequences: one more; the last batch may be odd
    assert batches(SEQS, 19, True) == [2, 2, 3]
    assert batches(SEQS, 6, False) == [1, 1, 1, 1, 2, 1] and batches(SEQS, 6, True) == [2, 2, 2, 1]


def test_the_last_batch_closes_below_the_limit():
    assert batches(SEQS, 1 << 20, False) == [len(SEQS)] and batches(SEQS, 1 << 20, True) == [len(SEQS)]
    assert batches(SEQS[:1], 1 << 20, True) == [1]


def test_empty_sequences_and_empty_input():
    assert batches([b"", b"ACGT", b""], 4, False) == [2, 1]
    assert list(AIndex._batches([], "cpu", 24, False)) == [] and list(AIndex._batches([], "cpu", 24, True)) == []
