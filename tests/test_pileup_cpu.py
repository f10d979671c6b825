"""Pins the test-side restatement of the pile-up (tests/pileup_ref.py) and the cases of tests/pileup_cases.py, without a GPU: literals
worked by hand, the properties of the contract on the threading batches, the planted heterozygous genome, and the refusals — those of
the restatement, and those of the entry points that are decided before any device call."""
import ctypes as C

import numpy as np
import pytest

import graph_cases as G
import pileup_cases as PC
import pileup_ref as PR
import seqthread_cases as SC
from aindex_amd import _lib

NEW = ("aix_pile_place_dev", "aix_pileup_dev", "aix_pile_call_dev", "aix_pileup")


def _one_contig(n, seed=1):
    """a graph of one linear contig of n bases, and its text as the graph spells it"""
    text = PC.random_text(np.random.default_rng(seed), n)
    g = PC.ref_graph(*PC.kmer_table([text]))
    assert len(g["strings"]) == 1 and g["strings"][0] in (text, PC.rc(text))
    return g, g["strings"][0]


def _places(p):
    return [tuple(int(p[k][i]) for k in PR.PLACE_KEYS[1:]) for i in range(p["n_place"])]


def _cells(piled, text, lo=0):
    """{(local base, channel): count} of the non-zero cells, channels as letters"""
    c = piled["counts"].reshape(-1, 4)
    return {(int(g) - lo, "ACGT"[int(x)]): int(c[g, x]) for g, x in zip(*np.nonzero(c))}


def _expect(text, lo, hi, alt=None, skip=()):
    want = {(g, text[g]): 1 for g in range(lo, hi) if g not in skip}
    for g, b in (alt or {}).items():
        del want[(g, text[g])]
        want[(g, b)] = 1
    return want


def test_literal_substitution_in_the_middle_both_strands():
    g, c = _one_contig(80)
    read = PC.substitute(c[10:70], 30)
    for text, flag in ((read, 0), (PC.rc(read), 1)):
        steps, places, piled = PC.chain(g, [text])
        assert places["seq_place_off"].tolist() == [0, 1] and steps["seq_step_off"].tolist() == [0, 2]
        assert list(zip(steps["q_first"].tolist(), steps["q_last"].tolist())) == [(0, 6 if flag else 7), (30 if flag else 31, 37)]
        assert _places(places) == [(0, flag, 10, 0, 60, 2)] and places["n_circular_steps"] == 0
        assert _cells(piled, c) == _expect(c, 10, 70, {40: read[30]})
        assert piled["place_mism"].tolist() == [1] and piled["stats"].tolist() == [60, 0, 1]
        for k, dt in zip(PR.PLACE_KEYS, PR.PLACE_DTYPES):
            assert places[k].dtype == dt, k
        out = PR.call(g["g"]["offsets"], g["g"]["bases"], piled["counts"], 1, 700, 1, 200)
        assert [out[k].tolist() for k in PR.VAR_KEYS] == [[0], [40], [ord(c[40])], [ord(read[30])], [0], [1], [1]]
        assert out["polished"].tobytes().decode() == c[:40] + read[30] + c[41:] and out["n_changed"] == 1
        assert out["depth_sum"].tolist() == [60] and out["uncovered"].tolist() == [20]
        for k, dt in zip(PR.VAR_KEYS, PR.VAR_DTYPES):
            assert out[k].dtype == dt, k


def test_literal_substitution_near_the_end_is_counted_only_through_extend():
    g, c = _one_contig(80)
    read = PC.substitute(c[10:70], 54)                              # 5 bases in front of the read's last base: no window behind it
    steps, places, piled = PC.chain(g, [read])
    assert steps["q_last"].tolist() == [31] and _places(places) == [(0, 0, 10, 0, 60, 1)]
    assert _cells(piled, c) == _expect(c, 10, 70, {64: read[54]}) and piled["stats"].tolist() == [60, 0, 1]
    steps, places, piled = PC.chain(g, [read], extend=0)
    assert _places(places) == [(0, 0, 10, 0, 54, 1)]
    assert _cells(piled, c) == _expect(c, 10, 64) and piled["stats"].tolist() == [54, 0, 0]
    steps, places, piled = PC.chain(g, [PC.rc(read)], extend=3)     # backwards the core begins at read base 6; three more reach the substitution at 5
    assert _places(places) == [(0, 1, 10, 3, 57, 1)] and _cells(piled, c) == _expect(c, 10, 67, {64: read[54]})
    steps, places, piled = PC.chain(g, [PC.rc(read)], extend=0)
    assert _places(places) == [(0, 1, 10, 6, 54, 1)] and _cells(piled, c) == _expect(c, 10, 64)


def test_literal_two_substitutions_merge_by_max_gap():
    g, c = _one_contig(120)
    read = PC.substitute(PC.substitute(c[5:115], 40), 70)
    steps, places, piled = PC.chain(g, [read])
    assert list(zip(steps["q_first"].tolist(), steps["q_last"].tolist())) == [(0, 17), (41, 47), (71, 87)]
    assert _places(places) == [(0, 0, 5, 0, 110, 3)] and piled["place_mism"].tolist() == [2]
    assert _cells(piled, c) == _expect(c, 5, 115, {45: read[40], 75: read[70]})
    # 23 windows lie between the steps: at max_gap 20 they stay apart. Each core grows up to the core next to it, so the one base between
    # two cores is claimed from both sides and counts twice
    steps, places, piled = PC.chain(g, [read], max_gap=20)
    assert _places(places) == [(0, 0, 5, 0, 41, 1), (0, 0, 45, 40, 31, 1), (0, 0, 75, 70, 40, 1)]
    want = _expect(c, 5, 115, {45: read[40], 75: read[70]})
    want[(45, read[40])] = want[(75, read[70])] = 2
    assert _cells(piled, c) == want and piled["place_mism"].tolist() == [1, 2, 1] and piled["stats"].tolist() == [112, 0, 4]
    steps, places, piled = PC.chain(g, [read], max_gap=22)
    assert places["n_place"] == 3
    assert PC.chain(g, [read], max_gap=23)[1]["n_place"] == 1


def test_literal_n_and_lower_case_count_nowhere():
    g, c = _one_contig(120)
    read = c[5:45] + "N" + c[46:75] + c[75].lower() + c[76:115]
    comp = dict(zip("ACGTNacgt", "TGCANtgca"))
    for text, flag in ((read, 0), ("".join(comp[ch] for ch in reversed(read)), 1)):
        steps, places, piled = PC.chain(g, [text])
        assert _places(places) == [(0, flag, 5, 0, 110, 3)]
        assert _cells(piled, c) == _expect(c, 5, 115, skip=(45, 75))
        assert piled["place_mism"].tolist() == [0] and piled["stats"].tolist() == [108, 2, 0]


def test_literal_read_across_a_link_is_clipped_by_contig_end_and_neighbour():
    rng = np.random.default_rng(5)
    x, y1, y2 = PC.random_text(rng, 40), PC.random_text(rng, 30), PC.random_text(rng, 30)
    if y1[0] == y2[0]:
        y2 = PC.substitute(y2, 0)
    g = PC.ref_graph(*PC.kmer_table([x + y1, x + y2]))
    stem_text, arm_text = x, x[18:] + y1                            # 18 and 30 k-mers
    ids = {}
    for u, s in enumerate(g["strings"]):
        for name, t in (("stem", stem_text), ("arm", arm_text)):
            if s in (t, PC.rc(t)):
                ids[name] = (u, int(s != t))
    assert len(g["strings"]) == 3 and set(ids) == {"stem", "arm"}
    read = x[5:] + y1[:25]                                          # windows 0 .. 12 on the stem, 13 .. 37 on the arm
    steps, places, piled = PC.chain(g, [read])
    assert list(zip(steps["q_first"].tolist(), steps["q_last"].tolist())) == [(0, 12), (13, 37)]
    (su, sf), (au, af) = ids["stem"], ids["arm"]
    # the stem's core ends at the last base of its contig and the arm's begins at its first: nothing to extend into, and the neighbour's
    # core (the 22 shared bases belong to both contigs) leaves a negative room, which is 0
    assert _places(places) == [(su, sf, 0 if sf else 5, 0, 35, 1), (au, af, 52 - 47 if af else 0, 13, 47, 1)]
    off = g["g"]["offsets"].tolist()
    c = piled["counts"].reshape(-1, 4)
    depth = c.sum(axis=1)
    assert depth[off[su]:off[su + 1]].sum() == 35 and depth[off[au]:off[au + 1]].sum() == 47 and depth.sum() == 82
    assert piled["place_mism"].tolist() == [0, 0] and piled["stats"].tolist() == [82, 0, 0]
    # a read that hangs over the end of its contig: the extension stops at the contig's last base
    gg, cc = _one_contig(80)
    tail = cc[50:] + PC.rc(cc[:12])
    steps, places, piled = PC.chain(gg, [tail])
    assert _places(places) == [(0, 0, 50, 0, 30, 1)] and _cells(piled, cc) == _expect(cc, 50, 80)


def test_literal_circular_step_is_skipped_and_counted():
    rng = np.random.default_rng(9)
    ring, line = PC.random_text(rng, 40), PC.random_text(rng, 60)
    g = PC.ref_graph(*PC.kmer_table([ring + ring[:22], line]))
    circ = g["g"]["circular"].tolist()
    assert sorted(circ) == [0, 1] and sorted(len(s) for s in g["strings"]) == [60, 62]
    # the third read leaves the line after 30 bases (a substitution, then the ring): its extension runs on over 22 bases that are not the line's
    steps, places, piled = PC.chain(g, [(ring * 3)[7:77], line[3:50], line[:30] + PC.substitute(line[30], 0) + (ring * 2)[:40]])
    assert steps["seq_step_off"].tolist() == [0, 1, 2, 4] and (steps["step_flag"] & 2).tolist() == [2, 0, 0, 2]
    assert places["seq_place_off"].tolist() == [0, 0, 1, 2] and places["n_circular_steps"] == 2
    lin = circ.index(0)
    f = int(g["strings"][lin] != line)
    assert _places(places) == [(lin, f, 60 - 50 if f else 3, 0, 47, 1), (lin, f, 60 - 52 if f else 0, 0, 52, 1)]
    off = g["g"]["offsets"].tolist()
    depth = piled["counts"].reshape(-1, 4).sum(axis=1)
    assert depth[off[1 - lin]:off[2 - lin]].sum() == 0 and depth.sum() == 99 and piled["place_mism"][1] >= 1


def test_literal_short_reads_and_a_contig_of_23_bases():
    g, c = _one_contig(80)
    steps, places, piled = PC.chain(g, [c[30:52], c[30:53], c[30:54], "", PC.rc(c[57:80])])
    assert places["seq_place_off"].tolist() == [0, 0, 1, 2, 2, 3]
    assert _places(places) == [(0, 0, 30, 0, 23, 1), (0, 0, 30, 0, 24, 1), (0, 1, 57, 0, 23, 1)]
    want = _expect(c, 30, 54)
    for gg in range(30, 53):
        want[(gg, c[gg])] = 2
    want.update(_expect(c, 57, 80))
    assert _cells(piled, c) == want
    g1, c1 = _one_contig(23, seed=3)
    flank = "ACGTTGCA"
    steps, places, piled = PC.chain(g1, [c1, flank + c1 + flank, PC.rc(flank + c1)])
    assert _places(places) == [(0, 0, 0, 0, 23, 1), (0, 0, 0, 8, 23, 1), (0, 1, 0, 0, 23, 1)]     # clipped at both ends of the contig
    assert _cells(piled, c1) == {(gg, c1[gg]): 3 for gg in range(23)}
    out = PR.call(g1["g"]["offsets"], g1["g"]["bases"], piled["counts"], 1)
    assert out["total"] == 0 and out["depth_sum"].tolist() == [69] and out["uncovered"].tolist() == [0]


def test_call_ties_thresholds_and_64_bit_sums():
    off, bases = np.array([0, 23], np.uint64), np.frombuffer(b"ACGT" * 5 + b"ACG", np.uint8)
    cnt = np.zeros((23, 4), np.uint32)
    cnt[0] = (2, 5, 5, 0)                                          # A: alt ties between C and G go to C; 5 > 2 but 5000 < 700 * 12
    cnt[1] = (7, 1, 0, 0)                                          # C with A in the majority: 7000 >= 700 * 8
    cnt[2] = (0, 0, 0xFFFFFFFF, 0xFFFFFFFF)                        # G: D does not fit 32 bits
    cnt[3] = (3, 0, 0, 4)                                          # T: depth 7 < 8
    cnt[4] = (6, 2, 0, 0)                                          # A: alt count 2 < 3
    cnt[5] = (0, 13, 0, 3)                                         # C: 3000 < 200 * 16
    out = PR.call(off, bases, cnt.reshape(-1))
    assert out["polished"].tobytes() == b"AAGTACGT" + (b"ACGT" * 5 + b"ACG")[8:] and out["n_changed"] == 1
    assert [out[k].tolist() for k in PR.VAR_KEYS] == [[0, 0, 0], [0, 1, 2], [65, 67, 71], [67, 65, 84], [2, 1, 0xFFFFFFFF], [5, 7, 0xFFFFFFFF],
                                                      [12, 8, 0xFFFFFFFF]]
    assert out["depth_sum"].tolist() == [12 + 8 + 2 * 0xFFFFFFFF + 7 + 8 + 16] and out["uncovered"].tolist() == [17]
    # permille products beyond 2^64 are exact, not wrapped: at a threshold of 2^31 and D = 2^33 the product is 2^64, which 64 bits
    # would store as 0, below 1000 c[alt] = 1000 (2^32 - 1)
    M = 0xFFFFFFFF
    cnt[:] = 0
    cnt[4] = (M, M, 1, 1)                                          # A: D = 2^33, alt C; no variant site at min_alt_permille 2^31
    cnt[8] = (M - 1, M, 2, 1)                                      # A: D = 2^33, alt C with c[alt] > c[r]; not polished at min_major_permille 2^31
    loose = PR.call(off, bases, cnt.reshape(-1), 1, 400, 1, 50)
    assert loose["var_pos"].tolist() == [4, 8] and loose["var_alt"].tolist() == [67, 67] and loose["var_depth"].tolist() == [M, M]
    assert loose["polished"].tobytes() == b"ACGTACGTCCGT" + (b"ACGT" * 5 + b"ACG")[12:] and loose["n_changed"] == 1
    out = PR.call(off, bases, cnt.reshape(-1), 1, 400, 1, 1 << 31)
    assert out["total"] == 0 and out["n_changed"] == 1
    out = PR.call(off, bases, cnt.reshape(-1), 1, 1 << 31, 1, 50)
    assert out["n_changed"] == 0 and out["polished"].tobytes() == bases.tobytes() and out["var_pos"].tolist() == [4, 8]
    assert out["depth_sum"].tolist() == [1 << 34] and out["uncovered"].tolist() == [21]


@pytest.fixture(scope="module", params=(0, 3))
def batch_case(request):
    codes, tfs, _ = G.make_graph_case(request.param)
    g = PC.ref_graph(codes, tfs, 0)
    b = SC.batch(g["un"], g["lk"], request.param)
    return g, b.seqs, PC.chain(g, b.seqs), request.param


def test_property_reverse_complement_gives_equal_counts(batch_case):
    g, seqs, (steps, places, piled), seed = batch_case
    clean = [s for s in seqs if set(s) <= set(b"ACGT")]
    assert len(clean) > 100
    fw = PC.chain(g, clean)
    bw = PC.chain(g, [PC.rc(s.decode()).encode() for s in clean])
    assert np.array_equal(fw[2]["counts"], bw[2]["counts"]) and fw[2]["counts"].sum() > 0
    assert fw[1]["n_place"] == bw[1]["n_place"] and fw[1]["n_circular_steps"] == bw[1]["n_circular_steps"]
    assert sorted(fw[2]["place_mism"].tolist()) == sorted(bw[2]["place_mism"].tolist())


def test_property_cells_sum_to_the_cover_minus_other_bytes(batch_case):
    g, seqs, (steps, places, piled), seed = batch_case
    off = g["g"]["offsets"].astype(np.int64)
    cover, other = np.zeros(int(off[-1]), np.int64), np.zeros(int(off[-1]), np.int64)
    spo = places["seq_place_off"].tolist()
    for i, s in enumerate(seqs):
        for r in range(spo[i], spo[i + 1]):
            g0, n, q0 = int(off[places["place_unitig"][r]]) + int(places["place_pos"][r]), int(places["place_len"][r]), int(places["place_q0"][r])
            cover[g0:g0 + n] += 1
            bad = np.array([ch not in b"ACGT" for ch in s[q0:q0 + n]], dtype=np.int64)
            other[g0:g0 + n] += bad[::-1] if places["place_flag"][r] & 1 else bad
    assert np.array_equal(piled["counts"].reshape(-1, 4).sum(axis=1), cover - other)
    assert piled["stats"].tolist() == [int((cover - other).sum()), int(other.sum()), int(piled["place_mism"].sum())]
    assert other.sum() > 0 and piled["stats"][2] > 0 and places["n_circular_steps"] > 0 and (seed != 0 or (places["place_steps"] > 1).any())
    assert (places["place_flag"] == 1).any() and (places["place_flag"] == 0).any()


def test_property_two_halves_equal_the_whole(batch_case):
    g, seqs, (steps, places, piled), seed = batch_case
    half = len(seqs) // 2
    a = PC.chain(g, seqs[:half])
    b = PC.chain(g, seqs[half:], counts=a[2]["counts"])
    assert np.array_equal(b[2]["counts"], piled["counts"])
    assert a[1]["n_place"] + b[1]["n_place"] == places["n_place"]
    assert (a[2]["stats"] + b[2]["stats"]).tolist() == piled["stats"].tolist()
    wrapped = PC.chain(g, seqs, counts=np.full(piled["counts"].shape[0], 0xFFFFFFFF, np.uint32))[2]["counts"]      # counters wrap at 2^32
    assert np.array_equal(wrapped, piled["counts"] - np.uint32(1))


@pytest.fixture(scope="module")
def planted():
    p = PC.planted()
    g = PC.ref_graph(p["codes"], p["tfs"], 1, 3)
    steps, places, piled = PC.chain(g, p["reads"])
    return p, g, places, piled


def test_planted_sites_come_back_and_nothing_else(planted):
    p, g, places, piled = planted
    assert len(PC.SITES) == 39 and [len(s) for s in g["strings"]] == [PC.GENOME]
    out = PR.call(g["g"]["offsets"], g["g"]["bases"], piled["counts"], min_depth=8, min_alt_count=3, min_alt_permille=200)
    got = list(zip(out["var_pos"].tolist(), [chr(x) for x in out["var_ref"].tolist()], [chr(x) for x in out["var_alt"].tolist()]))
    assert got == PC.expected_sites(p, g["strings"][0]) and out["var_unitig"].tolist() == [0] * 39
    assert out["var_depth"].tolist() == [30] * 39 and out["var_alt_count"].min() >= 9 and out["var_ref_count"].min() >= 19
    assert out["n_changed"] == 0 and out["polished"].tobytes().decode() == g["strings"][0]
    assert places["n_place"] == len(p["reads"]) and places["n_circular_steps"] == 0
    # without the end extension sites are lost and the alternative allele is undercounted
    bare = PC.chain(g, p["reads"], extend=0)[2]["counts"]
    lost = PR.call(g["g"]["offsets"], g["g"]["bases"], bare, min_depth=8, min_alt_count=3, min_alt_permille=200)
    assert lost["total"] < 39 and lost["var_alt_count"].max() < 9


def test_planted_polishing_restores_corrupted_bases(planted):
    p, g, places, piled = planted
    contig = g["strings"][0]
    rng = np.random.default_rng(11)
    depth = piled["counts"].reshape(-1, 4).sum(axis=1)
    depth[[x for x, _, _ in PC.expected_sites(p, contig)]] = 0          # (at a planted site no allele reaches the 700 permille of a clear majority)
    where = sorted(rng.choice(np.nonzero(depth >= 8)[0], 10, replace=False).tolist())
    bad = contig
    for x in where:
        bad = PC.substitute(bad, x, int(rng.integers(1, 4)))
    assert sum(a != b for a, b in zip(bad, contig)) == 10
    out = PR.call(g["g"]["offsets"], np.frombuffer(bad.encode(), np.uint8), piled["counts"], min_depth=8, min_alt_count=3, min_alt_permille=200)
    assert out["polished"].tobytes().decode() == contig and out["n_changed"] == 10


def test_the_restatement_refuses_what_the_contract_refuses():
    g, c = _one_contig(80)
    seqs = [c[10:70].encode(), c[:30].encode()]
    steps, places, piled = PC.chain(g, seqs)
    offs, off, bases = PC.seq_offs(seqs), g["g"]["offsets"], g["g"]["bases"]
    assert places["n_place"] == 2

    def changed(d, key, i, v):
        out = dict(d)
        out[key] = d[key].copy()
        out[key][i] = v
        return out

    for bad in (changed(steps, "seq_step_off", 0, 1), changed(steps, "seq_step_off", 2, 1), changed(steps, "seq_step_off", 1, 3),
                changed(steps, "step_unitig", 0, 1), changed(steps, "q_last", 0, 38), changed(steps, "q_first", 0, 38), changed(steps, "step_pos", 0, 21),
                changed(steps, "step_pos", 1, 58)):
        with pytest.raises(ValueError):
            PR.place(offs, bad, off)
    two = PC.chain(g, [PC.substitute(c[10:70], 30)])[0]
    with pytest.raises(ValueError):                                 # descending steps
        PR.place(np.array([0, 60], np.uint64), changed(two, "q_first", 1, 7), off)
    with pytest.raises(ValueError):
        PR.place(offs, steps, np.array([0, 22], np.uint64))
    with pytest.raises(ValueError):
        PR.place(offs[::-1].copy(), steps, off)
    back = changed(steps, "step_flag", 0, 1)                        # backwards: b - a <= p
    with pytest.raises(ValueError):
        PR.place(offs, changed(back, "step_pos", 0, 36), off)
    for bad in (changed(places, "seq_place_off", 2, 1), changed(places, "place_unitig", 0, 1), changed(places, "place_pos", 0, 21), changed(places, "place_q0", 1, 1),
                changed(places, "place_len", 1, 0)):
        with pytest.raises(ValueError):
            PR.pile(seqs, bad, off, bases)
    lower = bases.copy()
    lower[5] |= 0x20
    with pytest.raises(ValueError):
        PR.pile(seqs, places, off, lower)
    with pytest.raises(ValueError):
        PR.call(off, lower, piled["counts"])
    with pytest.raises(ValueError):
        PR.call(np.array([1, 80], np.uint64), bases, piled["counts"])


def test_new_symbols_are_declared_and_bound():
    assert set(NEW) <= set(_lib.header_symbols()) and set(NEW) <= set(_lib.SIGNATURES)


def test_null_pointers_are_refused_before_any_device_call():
    """Runs without a GPU: a NULL pointer where one is needed is decided before anything is allocated or launched."""
    L = _lib.lib()
    a = np.zeros(8, np.uint64)
    p = a.ctypes.data_as(C.c_void_p)
    n = C.c_uint64(77)
    ARG = _lib.AIX_ERR_ARG
    place = lambda **o: L.aix_pile_place_dev(*[o.get(k, v) for k, v in (("M", 1), ("offs", p), ("sso", p), ("T", 1), ("su", p), ("sp", p), ("sf", p), ("qf", p), ("ql", p),
                                                                       ("U", 1), ("offsets", p), ("max_gap", 46), ("extend", 22), ("spo", p), ("pu", p), ("pf", p),
                                                                       ("pp", p), ("pq", p), ("pl", p), ("ps", p), ("n", C.byref(n)), ("circ", None), ("stream", None))])
    for k in ("offs", "sso", "su", "sp", "sf", "qf", "ql", "offsets", "spo", "pu", "pf", "pp", "pq", "pl", "ps", "n"):
        assert place(**{k: None}) == ARG, k
    assert place(M=0) == ARG and place(U=(1 << 31) - 3) == _lib.AIX_ERR_UNSUPPORTED and n.value == 77
    pile = lambda **o: L.aix_pileup_dev(*[o.get(k, v) for k, v in (("seqs", p), ("offs", p), ("M", 1), ("spo", p), ("R", 1), ("pu", p), ("pf", p), ("pp", p), ("pq", p),
                                                                   ("pl", p), ("U", 1), ("offsets", p), ("bases", p), ("counts", p), ("mism", None), ("stats", None),
                                                                   ("stream", None))])
    for k in ("seqs", "offs", "spo", "pu", "pf", "pp", "pq", "pl", "offsets", "bases", "counts"):
        assert pile(**{k: None}) == ARG, k
    assert pile(M=0) == ARG and pile(U=0) == ARG and pile(counts=C.c_void_p(p.value + 4)) == ARG
    call = lambda **o: L.aix_pile_call_dev(*[o.get(k, v) for k, v in (("U", 1), ("offsets", p), ("bases", p), ("counts", p), ("d", 8), ("maj", 700), ("ac", 3), ("ap", 200),
                                                                      ("polished", None), ("changed", None), ("v0", p), ("v1", p), ("v2", p), ("v3", p), ("v4", p),
                                                                      ("v5", p), ("v6", p), ("cap", 1), ("total", C.byref(n)), ("dsum", None), ("unc", None),
                                                                      ("stream", None))])
    for k in ("offsets", "bases", "counts", "v0", "v1", "v2", "v3", "v4", "v5", "v6", "total"):
        assert call(**{k: None}) == ARG, k
    assert call(counts=C.c_void_p(p.value + 8)) == ARG and n.value == 77
    outs = [C.c_void_p() for _ in range(12)]
    assert L.aix_pileup(None, 0, p, p, 1, 46, 22, C.byref(n), C.byref(n), None, *[C.byref(x) for x in outs]) == ARG
