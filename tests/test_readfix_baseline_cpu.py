"""The composed baseline of scripts/gpu_readfix.py (coverage profile + torch boundaries + candidate lookups) on CPU tensors against
tests/readfix_ref.py: the measurement compares the fused kernel with it by SHA-256, so it has to follow the same rules."""
import importlib.util
import os

import numpy as np
import pytest

import debruijn_ref as D
import readfix_cases as K
import readfix_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script():
    spec = importlib.util.spec_from_file_location("gpu_readfix", os.path.join(ROOT, "scripts", "gpu_readfix.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("t,V,F", [(1, 8, 4), (1, 3, 2), (1, 16, 1), (1, 8, 0)])
def test_composed_baseline_follows_the_rules(t, V, F):
    import torch
    genome, buf, start, end, _, _ = K.planted_case(n_reads=600, n_with_n=0)
    _, freq = K.genome_freq(genome)
    freq = K.MemoFreq(freq)
    reads = buf.reshape(600, 151)[:, :150].copy()
    rng = np.random.default_rng(9)
    extra = rng.random(reads.shape) < 0.02                         # close pairs of errors on top of the planted ones: n0, PARTIAL, UNFIXED
    extra[::2] = False
    extra[::8, 60], extra[::8, 65] = True, True                    # nothing but two errors five apart: UNFIXED
    reads[extra] = D.LETTERS[(np.searchsorted(D.LETTERS, reads[extra]) + 1) % 4]
    flat = np.concatenate([reads, np.full((600, 1), 10, np.uint8)], axis=1).reshape(-1)
    want_buf, want_rec, want_pos, want_old = R.fix_reads(freq, flat, start, end, t, V, F)

    def profile(x):
        w = np.lib.stride_tricks.sliding_window_view(x.numpy(), 23, axis=1)
        return torch.from_numpy(freq(D.encode(np.ascontiguousarray(w).reshape(-1, 23))).astype(np.int64).reshape(x.shape[0], -1))

    def tf_codes(c):
        return torch.from_numpy(freq(c.numpy().astype(np.uint64)).astype(np.int64))

    got = torch.from_numpy(reads.copy())
    rec, pos, old = _script().composed_fix(got, profile, tf_codes, t, V, F)
    assert np.array_equal(rec.numpy().astype(np.uint32), np.stack([want_rec[f] for f in R.REC_FIELDS], axis=1))
    assert np.array_equal(pos.numpy().astype(np.uint32), want_pos) and np.array_equal(old.numpy(), want_old)
    assert np.array_equal(got.numpy(), want_buf.reshape(600, 151)[:, :150])
    if F == 4:
        hist = np.bincount(want_rec["status"], minlength=4)
        assert (hist >= 10).all() and want_rec["n0"].sum() >= 10, hist
