"""CPU: tests/spectrum_ref.py (numpy over the oracle) reproduces tests/golden/*/frequency.json (the compiled reference's answers), so that
the GPU tests may hold aix_spectrum.hip against either."""
import json
import os

import numpy as np
import pytest

import oracle_lib as O
import spectrum_ref as S

SETS = ("small23", "graph23")


def _load(gold, name):
    prefix = os.path.join(gold, name, name)
    return O.OracleIndex23.from_prefix(prefix), json.load(open(os.path.join(gold, name, "frequency.json")))


@pytest.mark.parametrize("name", SETS)
def test_ref_reproduces_the_goldens(gold, name):
    orc, doc = _load(gold, name)
    assert orc.n == doc["n"]
    v = S.values23(orc)
    assert v.tolist() == doc["values"]
    assert S.same(S.kmers23(orc), doc["kmers"])
    for sel in doc["selections"]:
        if sel["max_kmers"] == 0:                                  # freq_list[:0]: the list surface's business, 0 means "all" below it
            assert sel["kid"] == []
            continue
        idx, val, total = S.select(v, sel["min_tf"], sel["max_kmers"] or 0)
        assert S.same(idx.tolist(), sel["kid"]) and S.same(val.tolist(), sel["tf"]) and total == sel["total"], (sel["min_tf"], sel["max_kmers"])
    assert [list(t) for t in S.info23(orc, doc["info_kids"])] == doc["info"]


def test_the_goldens_hold_the_cases_that_matter(gold):
    doc = json.load(open(os.path.join(gold, "small23", "frequency.json")))
    by = {(s["min_tf"], s["max_kmers"]): s for s in doc["selections"]}
    assert by[(2, 25)]["tf"] == [18] * 8 + [17] * 10 + [16] * 7 and doc["values"].count(16) == 32      # a cut inside a tie class
    assert by[(1, 18)]["tf"] == [18] * 8 + [17] * 10                                                    # a cut on a class boundary
    assert by[(1, 10 ** 4)]["kid"]["len"] == doc["n"] and by[(19, 10)]["kid"] == [] and by[(19, 10)]["total"] == 0
    assert doc["info_kids"][-1] == doc["n"] and doc["info"][-1] == [0, "", ""]


def test_spectrum_and_stats_of_the_ref():
    v = np.array([0, 1, 1, 2, 7, 7, 7, 0xFFFFFFFF, 0], dtype=np.uint32)
    assert S.spectrum(v, 2).tolist() == [2, 7] and S.spectrum(v, 4).tolist() == [2, 2, 1, 4] and S.spectrum(v, 9).tolist() == [2, 2, 1, 0, 0, 0, 0, 3, 1]
    assert S.stats(v) == {"n": 9, "non_zero": 7, "max": 0xFFFFFFFF, "min_non_zero": 1, "sum": 25 + 0xFFFFFFFF}
    assert S.stats(np.zeros(3, np.uint32)) == {"n": 3, "non_zero": 0, "max": 0, "min_non_zero": 0, "sum": 0}
    idx, val, total = S.select(v, 1, 3)
    assert (idx.tolist(), val.tolist(), total) == ([7, 4, 5], [0xFFFFFFFF, 7, 7], 7)
    assert S.select(v, 0, 0)[0].tolist() == [7, 4, 5, 6, 3, 1, 2, 0, 8] and S.spell13([0, 27, 4 ** 13 - 1]) == ["A" * 13, "AAAAAAAAAACGT", "T" * 13]
