"""Array-level inputs of the graph cleaning without a GPU: the generators of tests/graph_arrays.py are held to the restatement
(tests/graph_clean_ref.py) and the array checker (tests/graph_clean_check.py), and the conditions that make the inputs worth running on
the GPU — every trip count of the member walk of k_gc_emit, ties of first 23-mers, decisions that only an exact 128-bit comparison gets
right — are asserted here, on the very inputs test_gpu_graph_arrays.py uses."""
import numpy as np
import pytest

import graph_arrays as GA
import graph_clean_check as GK
import graph_clean_ref as GR

NONE32 = GR.NONE32
CANONICAL_KEYS = ("offsets", "circular", "tf_sum", "tf_min", "tf_max", "link_off", "link_to")
MAX_BASES = 40_000


def _property_inputs():
    """graph cases 0 and 3, every topology case, every link case and the ring with two stems, of at most 40 000 bases"""
    names = [0, 3] + sorted(GA.planted_cases())
    return [nm for nm in names if int(GA.source_graph(nm)["offsets"][-1]) <= MAX_BASES]


def _first_codes(g):
    return GK._code_of_rows(g["bases"][g["offsets"][:-1].astype(np.int64)[:, None] + np.arange(GA.K)[None, :]])


@pytest.mark.parametrize("p_cut", (0.5, 1.0))
def test_compacting_a_shred_gives_back_the_graph(p_cut):
    """The shred is a valid unitig set; GR.compact(shred, zeros) passes the checker and equals the original graph in canonical form:
    strings, offsets, circular, tf_sum / min / max, link_off and link_to. p_cut 1.0 cuts at every boundary."""
    names = _property_inputs()
    assert len(names) >= 20 and {0, 3, "lollipop", "opened_circle", "many_circles", "hairpin_ends", "selfloop"} <= set(names)
    for i, name in enumerate(names):
        g = GA.source_graph(name)
        sh = GA.shred(g, np.random.default_rng((515, i, int(p_cut * 10))), p_cut)
        GK.check_graph(sh)
        m_in = np.diff(g["offsets"].astype(np.int64)) - 22
        kept = sh["piece_of"][sh["circular"] == 1]                  # the circles kept whole
        assert g["circular"][kept].all() and np.unique(kept).shape[0] == kept.shape[0], name
        if p_cut == 1.0:                                           # every other piece is one k-mer
            assert (np.diff(sh["offsets"].astype(np.int64))[sh["circular"] == 0] == 23).all(), name
            assert sh["U"] - kept.shape[0] == int(m_in.sum()) - int(m_in[kept].sum()), name
        sums = [0] * g["U"]
        for u, v in zip(sh["piece_of"].tolist(), sh["tf_sum"].tolist()):
            sums[u] += v
        assert sums == g["tf_sum"].tolist(), name                  # the pieces add up to the original
        zeros = np.zeros(sh["U"], np.uint8)
        out = GR.compact(sh, zeros)
        GK.check(sh, zeros, out)
        assert out["C"] == g["U"] and out["n_circular"] == int(g["circular"].sum()), name
        a, b = GR.canonical_form(out), GR.canonical_form(g)
        assert a["strings"] == b["strings"], name
        for k in CANONICAL_KEYS:
            assert np.array_equal(a[k], b[k]), (name, k)


def test_pinned_sizes():
    """Graph case 0 goes from U = 585 to 2035 pieces and back to 585 contigs; cut everywhere, the circle of 4096 k-mers becomes one merged
    cycle of 4096 one-k-mer members that starts at its smallest member, and the ring of the largest lollipop a chain of 1000 members."""
    g, sh, out = GA.source_graph(0), GA.shred_of(0, 0.5), GA.reference((0, 0.5), "zero")
    assert (g["U"], sh["U"], out["C"]) == (585, 2035, 585)
    sh, out = GA.shred_of("opened_circle", 1.0), GA.reference(("opened_circle", 1.0), "zero")
    assert sorted(np.bincount(out["unitig_contig"]).tolist()) == [24, 4096] and out["circular"].tolist() == [1, 1] and not sh["circular"].any()
    assert (out["unitig_flag"] & 2).all() and sorted(out["unitig_pos"].tolist()) == sorted(list(range(24)) + list(range(4096)))
    for c in (0, 1):
        mem = np.nonzero(out["unitig_contig"] == c)[0]
        assert out["unitig_pos"][mem.min()] == 0 and out["unitig_flag"][mem.min()] == 2
    out = GA.reference(("lollipop", 1.0), "zero")
    assert sorted(np.bincount(out["unitig_contig"]).tolist()) == [7, 30, 30, 30, 64, 1000] and not out["circular"].any()
    out = GA.reference(("lollipop", 1.0), "mark")                 # the stems are clipped piece by piece only; nothing closes in one round
    assert out["C"] >= 6


def test_every_gpu_input_passes_the_checker():
    """Every shred the GPU test compacts, under each of its masks (zero, 10 %, 50 %, the mark), and the union under the same masks: the
    restatement's answer passes the array checker; under the zero mask it is the source graph again."""
    for name in GA.SHRED_INPUTS:
        want = GR.canonical_form(GA.source_graph(name))
        for p_cut in GA.P_CUTS:
            key = (name, p_cut)
            sh = GA.shred_of(*key)
            GK.check_graph(sh)
            for mask in GA.MASKS:
                out = GA.reference(key, mask)
                GK.check(sh, GA.mask_of(key, mask), out)
                if mask in ("10 %", "50 %") and sh["U"] >= 100:
                    assert 0 < GA.mask_of(key, mask).sum() < sh["U"], (key, mask)
            got = GR.canonical_form(GA.reference(key, "zero"))
            assert got["strings"] == want["strings"] and all(np.array_equal(got[k], want[k]) for k in CANONICAL_KEYS), key
    un = GA.union_case()
    GK.check_graph(un)
    for mask in GA.MASKS:
        GK.check(un, GA.mask_of("union", mask), GA.reference("union", mask))
    assert sum(int(GA.mask_of((name, p), "mark").any()) for name in GA.SHRED_INPUTS for p in GA.P_CUTS) >= 6   # the mark mask is not the zero mask


def test_the_union_of_two_shreds_ties_every_first_code():
    """Every contig of the union has a twin with the same first 23-mer: the order is decided by the id of the first member, and a path
    whose two ends tie is spelled from the end with the smaller member id."""
    un, out = GA.union_case(), GA.reference("union", "zero")
    one = GA.source_graph(0)
    assert out["C"] == 2 * one["U"] == 1170
    hc = _first_codes(out)
    ties = np.nonzero(hc[1:] == hc[:-1])[0]
    assert ties.shape[0] >= 100 and ties.shape[0] == 582
    first = np.array([ch[0][0] for ch in out["chains"]])
    assert (first[ties] < first[ties + 1]).all()                  # as the contract orders them
    half = GA.shred_of(*GA.UNION_OF[0])["U"]
    assert ((first[ties] < half) != (first[ties + 1] < half)).all()   # the twins come from the two shreds
    for mask in GA.MASKS[1:]:
        hc = _first_codes(GA.reference("union", mask))
        assert (hc[1:] == hc[:-1]).sum() >= 100, mask


def _coverage_inputs():
    return [((name, p_cut), mask) for name in (0, 3) for p_cut in GA.P_CUTS for mask in ("zero", "10 %")]


def test_emission_coverage_conditions():
    """What the inputs of the GPU test reach in k_gc_emit, replayed from the restatement's map: every member count 1 .. 16 per 16-byte
    chunk, all 32 (segment length, orientation) pairs, all 16 (source address mod 8, orientation) pairs, a source window past the end of
    `bases` in both orientations, and an input whose offsets[U] is no multiple of 8. The graphs an index gives reach three members."""
    for name in (0, 3):
        g = GA.source_graph(name)
        for remove in (np.zeros(g["U"], np.uint8), GR.mark(g, 46, 46)):
            assert GA.emit_coverage(g, GR.compact(g, remove))["members"] <= {1, 2, 3}, name
    per_input = {k: GA.emit_coverage(GA.shred_of(*k[0]), GA.reference(*k)) for k in _coverage_inputs()}
    cov = GA.merge_coverage(per_input.values())
    assert cov["members"] == set(range(1, 17))
    assert cov["length"] == {(n, r) for n in range(1, 17) for r in (0, 1)}
    assert cov["shift"] == {(s, r) for s in range(8) for r in (0, 1)}
    assert cov["past_end"] == {0, 1}
    assert 1 in per_input[(GA.FORCED, "zero")]["past_end"]        # the forced piece: stored last, reversed, first member of its contig
    sh = GA.shred_of(*GA.FORCED)
    out = GA.reference(GA.FORCED, "zero")
    last = sh["U"] - 1
    assert out["unitig_flag"][last] == 1 and out["unitig_pos"][last] == 0 and np.bincount(out["unitig_contig"])[out["unitig_contig"][last]] > 1
    assert any(int(GA.shred_of(*k[0])["offsets"][-1]) % 8 for k in per_input)
    assert 16 in per_input[((0, 1.0), "zero")]["members"] and 16 in per_input[((3, 1.0), "zero")]["members"]   # the launch-geometry input has them too
    # a merged cycle of one-k-mer members, and chains of them in both orientations
    for key in (("opened_circle", 1.0), ("lollipop", 1.0)):
        c = GA.emit_coverage(GA.shred_of(*key), GA.reference(key, "zero"))
        assert 16 in c["members"] and {(1, 0), (1, 1)} <= c["length"], key


def test_emit_coverage_on_a_hand_made_map():
    """two members of 1 and 2 k-mers, the second reversed, in one contig of 25 bases: chunk 0 holds 16 bytes of member 0, chunk 1 seven
    of member 0 and two of member 1"""
    g = {"offsets": np.array([0, 23, 47], np.uint64)}
    out = {"offsets": np.array([0, 25], np.uint64), "unitig_contig": np.array([0, 0], np.uint32), "unitig_pos": np.array([0, 1], np.uint64),
           "unitig_flag": np.array([0, 1], np.uint8)}
    c = GA.emit_coverage(g, out)
    assert c["members"] == {1, 2} and c["length"] == {(16, 0), (7, 0), (2, 1)}
    assert c["shift"] == {(0, 0), (7, 1)} and c["past_end"] == set()   # reversed: src = 23 + 24 - 22 - 2 = 23
    out["unitig_flag"] = np.array([0, 0], np.uint8)
    assert GA.emit_coverage(g, out)["past_end"] == {0}             # forwards: src = 23 + 22, and 45 + 16 > 47


@pytest.mark.parametrize("seed", GA.MARK_SEEDS)
def test_mark_graphs_tell_an_exact_comparison_from_its_mutants(seed):
    """The link structures for aix_graph_mark_dev are valid, give the pinned counts at the five threshold pairs, and at (32767, 32767)
    each of four wrong comparisons — products mod 2^64, products in double, floor means, ties to the larger id — changes a decision."""
    g = GA.make_mark_graph(seed)
    U = g["U"]
    GK.check_graph(dict(g, bases=np.broadcast_to(np.uint8(65), (int(g["offsets"][-1]),)), tf_min=np.zeros(U, np.uint32), tf_max=np.zeros(U, np.uint32)))
    m = np.diff(g["offsets"].astype(np.int64)) - 22
    assert 1100 <= U <= 1300 and set(m.tolist()) == set(GA.MARK_M) and int(g["circular"].sum()) == 5
    assert int(g["tf_sum"].max()) >= 2 ** 64 - 40000 and {int(v) for v in g["tf_sum"]} >= {1, 2 ** 32, 2 ** 53, 2 ** 53 + 1, 2 ** 63}
    mate = np.array(GR.bubbles(U, g["link_off"], g["link_to"]), np.uint32)
    assert (mate != NONE32).sum() >= 200
    counts = []
    for tip, bub in GA.MARK_THRESHOLDS:
        remove = GR.mark(g, tip, bub)
        counts.append((int((remove == 1).sum()), int((remove == 2).sum())))
    assert tuple(counts) == GA.MARK_COUNTS[seed]
    exact = GR.mark(g, 32767, 32767)
    assert np.array_equal(GA.mark_with(g, GR.outranks, 32767, 32767), exact)
    for name, fn in GA.MUTANTS.items():
        assert (GA.mark_with(g, fn, 32767, 32767) != exact).sum() >= 2, name
    assert GR.outranks is not None and np.array_equal(GR.mark(g, 32767, 32767), exact)   # the restatement is as it was
