"""The absence filter's key (filter_key of the 46-bit code, filterkey_ref.py) against the key it replaces (Jenkins' lookup8 on the ASCII
of the code): false positives on uniform queries and on one-substitution neighbours of keys, balance over the binned path's slices, and
how the key bits of a key and of its neighbours differ. numpy only; the two query sets and the two filters are computed once."""
import numpy as np
import pytest

import filterkey_ref as F
from aindex_amd import synth

N_QUERIES = 4_000_000
FP_CAP = 1.10               # pass C is 0.13 of a 1.70 ms step and scales with the survivors: 10 % more of them is under 1 % of a step
SLICES, SLICE_CAP = 8, 1.25  # a slice region of the binned path holds its share of a piece plus a quarter


@pytest.fixture(scope="module")
def world():
    keys, _ = synth.canonical_distinct(synth.genome_codes(37, 1_000_000), 23)
    assert keys.shape[0] == 999_978
    nwords = F.filter_words(keys.shape[0])
    assert nwords == 249_995
    uniform = F.canonical(synth.sm64(7, np.arange(N_QUERIES, dtype=np.uint64)) & np.uint64(4 ** 23 - 1))
    sets = {"uniform": uniform, "neighbour": F.neighbours(keys, N_QUERIES)}
    sets = {k: v[~np.isin(v, keys)] for k, v in sets.items()}                  # queries that are keys are dropped
    filters = {}
    for name, key in (("new", F.new_key), ("jenkins", F.old_key)):
        w, m = key(keys, nwords)
        filters[name] = (key, F.build_filter(w, m, nwords))
        assert F.passes(filters[name][1], w, m).all()                          # a key passes its own filter
    return {"keys": keys, "nwords": nwords, "sets": sets, "filters": filters}


@pytest.mark.parametrize("which", ["uniform", "neighbour"])
def test_false_positives_no_worse_than_jenkins(world, which):
    q = world["sets"][which]
    assert q.shape[0] > 0.9 * N_QUERIES
    share = {}
    for name, (key, filt) in world["filters"].items():
        w, m = key(q, world["nwords"])
        share[name] = float(F.passes(filt, w, m).mean())
    print(which, "false-positive share: jenkins %.4f %%, new %.4f %%, ratio %.3f" % (100 * share["jenkins"], 100 * share["new"], share["new"] / share["jenkins"]))
    assert share["jenkins"] > 0
    assert share["new"] <= FP_CAP * share["jenkins"]


@pytest.mark.parametrize("which", ["uniform", "neighbour"])
def test_slices_are_balanced(world, which):
    q, nwords = world["sets"][which], world["nwords"]
    w, _ = F.new_key(q, nwords)
    assert w.min() >= 0 and w.max() < nwords
    per = np.bincount(w * SLICES // nwords, minlength=SLICES)
    print(which, "queries per slice / mean:", np.round(per / per.mean(), 4).tolist())
    assert per.shape[0] == SLICES and per.max() <= SLICE_CAP * per.mean()


def test_key_bits_of_neighbours_differ(world):
    keys = world["keys"][:: world["keys"].shape[0] // 1000][:1000]
    nb = np.stack([keys ^ (np.uint64(x) << np.uint64(2 * p)) for p in range(23) for x in (1, 2, 3)], axis=1)   # (1000, 69), not made canonical
    hw0, hb0 = F.filter_key(keys)
    hw1, hb1 = F.filter_key(nb)
    same_hw = float((hw1 == hw0[:, None]).mean())
    same_hb = float((hb1 == hb0[:, None]).mean())
    same_hb16 = float(((hb1 & np.uint32(0xFFFF)) == (hb0[:, None] & np.uint32(0xFFFF))).mean())                # the 16 bits the mask takes: 2^-16 by chance
    print("neighbours with the same hw %.3g, the same hb %.3g, the same low 16 bits of hb %.3g" % (same_hw, same_hb, same_hb16))
    assert same_hw < 2.0 ** -12 and same_hb < 2.0 ** -12 and same_hb16 < 2.0 ** -12
