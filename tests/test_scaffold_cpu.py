"""Pins the test-side restatement of the scaffolding (tests/scaffold_ref.py) and the inputs of tests/scaffold_cases.py, without a GPU:
literals, the planted genomes recovered as scaffolds with exact gaps, the properties of the contract, and the refusals of the
handle-less entry points that are decided before any device call. Every test asks the built library for the entry points first."""
import ctypes as C

import numpy as np
import pytest

import graph_clean_ref as GR
import scaffold_cases as SC
import scaffold_ref as SF
import seqthread_ref as SR
import unitig_links_ref as RL
import unitigs_ref as R
from aindex_amd import _lib

NONE32 = SF.NONE32
MAX_INSERT = 1000


def offsets_of(seqs):
    return np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)


def restated(p, pairs=None):
    """a planted case through the restatements: the graph, its mates threaded, the observations, the scaffolds"""
    un = R.unitigs(p.codes, p.tfs, 0)
    lk = RL.links(p.codes, p.tfs, 0, un)
    g = GR.graph(un, lk)
    node = SR.nodes(un["kid_unitig"], un["kid_pos"], un["kid_flag"], un["offsets"])
    kid_of = {int(c): i for i, c in enumerate(p.codes.tolist())}
    seqs = SC.mates(p.pairs if pairs is None else pairs)
    steps = SR.thread(kid_of, node, g, seqs)
    key, d, counts, hist = SF.mate_links(offsets_of(seqs), steps, g["offsets"], g["circular"], 1, MAX_INSERT)
    res = SF.scaffold(g["offsets"], g["bases"], g["circular"], key, d, p.insert, 2, 2, SC.MIN_BASES, 1)
    return dict(g=g, steps=steps, key=key, d=d, counts=counts, hist=hist, res=res, seqs=seqs)


ENTRY_POINTS = ("aix_mate_links_dev", "aix_mate_bundle_dev", "aix_scaffold_mark_dev", "aix_scaffold_layout_dev", "aix_scaffold_emit_dev", "aix_scaffold")


@pytest.fixture(scope="module", autouse=True)
def library():
    """The restatement is pinned for the library that states the same contract: without its entry points every test here fails."""
    L = _lib.lib()
    return [getattr(L, name) for name in ENTRY_POINTS]


@pytest.fixture(scope="module")
def every():
    return {name: (SC.planted(name), restated(SC.planted(name))) for name in SC.PLANTED}


def scaffolds_of(res):
    """[(text, [(contig, flag, gap)])]"""
    text, so, mo = res["scaffold_bases"].tobytes().decode(), res["scaffold_offsets"].tolist(), res["member_off"].tolist()
    return [(text[so[s]:so[s + 1]], [(int(w) >> 1, int(w) & 1, int(gp)) for w, gp in zip(res["member"][mo[s]:mo[s + 1]], res["member_gap"][mo[s]:mo[s + 1]])])
            for s in range(len(so) - 1)]


def check_against_genome(p, g, res, tolerance):
    """every scaffold lies in one genome on one strand, its members in genome order, every gap within `tolerance` of the true distance"""
    off, text = g["offsets"].tolist(), g["bases"].tobytes().decode()
    for s, members in scaffolds_of(res):
        prev = None
        for u, f, gap in members:
            piece = text[off[u]:off[u + 1]]
            where = SC.located(p, SC.rc(piece) if f else piece)
            assert where is not None
            if prev is not None:
                ring = len(p.genomes[where[0]]) if p.n_cut else 0
                true = where[2] - prev[1]
                if ring:
                    true %= ring
                assert where[:2] == prev[0] and abs(gap - true) <= tolerance, (u, gap, true)
            prev = (where[:2], where[2] + len(piece))


def test_literals_of_the_two_copy_case(every):
    """A R B and C R D with R of 150 bases: five unitigs, two joins of 57 pairs each over a gap of 106 = 150 - 44 bases."""
    p, r = every["two_copy"]
    g, res = r["g"], r["res"]
    assert len(p.pairs) == 500 and g["offsets"].tolist() == LIT["offsets"] and r["counts"].tolist() == LIT["counts"]
    assert {int(f): int(c) for f, c in enumerate(r["hist"]) if c} == LIT["hist"]
    assert sorted(collections_count(r["key"], r["d"]).items()) == LIT["observations"]
    for k in ("slink_off", "slink_to", "slink_count", "slink_dsum", "join", "join_count", "join_gap", "contig_scaffold", "contig_rank", "contig_pos", "contig_flag",
              "scaffold_offsets", "member_off", "member", "member_gap"):
        assert res[k].tolist() == LIT[k], k
    for k, dt in (("slink_off", np.uint64), ("slink_to", np.uint32), ("slink_count", np.uint64), ("slink_dsum", np.uint64), ("join", np.uint32), ("join_count", np.uint64),
                  ("join_gap", np.int64), ("contig_scaffold", np.uint32), ("contig_rank", np.uint32), ("contig_pos", np.uint64), ("contig_flag", np.uint8),
                  ("scaffold_offsets", np.uint64), ("scaffold_bases", np.uint8), ("member_off", np.uint64), ("member", np.uint32), ("member_gap", np.int64)):
        assert res[k].dtype == dt, k
    assert (res["n_scaffolds"], res["total_bases"], res["n_cut"], res["n_joins"], res["S"]) == LIT["sizes"]
    assert SF.insert_size(r["hist"]) == 400


def collections_count(key, d):
    out = {}
    for k, x in zip(key.tolist(), d.tolist()):
        if k != SF.NOKEY:
            out[(k >> 32, k & SF.M32, x)] = out.get((k >> 32, k & SF.M32, x), 0) + 1
    return out


N32 = NONE32
LIT = {"offsets": [0, 522, 1044, 1194, 1716, 2238], "counts": [214, 286, 0, 0], "hist": {400: 214},
       # unitig 2 is R (150 bases); 57 pairs bridge it between the flanks, 43 reach from either flank into R and from R into either flank
       "observations": [((0, 4, 422), 43), ((0, 7, 294), 57), ((2, 4, 422), 43), ((2, 8, 294), 57), ((4, 7, 422), 43), ((4, 8, 422), 43)],
       "slink_off": [0, 2, 2, 4, 4, 6, 8, 10, 10, 10, 12], "slink_to": [4, 7, 4, 8, 7, 8, 1, 3, 1, 5, 3, 5],
       "slink_count": [43, 57, 43, 57, 43, 43, 43, 43, 57, 43, 57, 43],
       "slink_dsum": [18146, 16758, 18146, 16758, 18146, 18146, 18146, 18146, 16758, 18146, 16758, 18146],
       "join": [7, N32, 8, N32, N32, N32, 1, N32, N32, 3], "join_count": [57, 0, 57, 0, 0, 0, 57, 0, 0, 57], "join_gap": [106, 0, 106, 0, 0, 0, 106, 0, 0, 106],
       "contig_scaffold": [0, 1, 2, 0, 1], "contig_rank": [0, 0, 0, 1, 1], "contig_pos": [0, 0, 0, 628, 628], "contig_flag": [0, 0, 0, 1, 0],
       "scaffold_offsets": [0, 1150, 2300, 2450], "member_off": [0, 2, 4, 5], "member": [0, 7, 2, 8, 4], "member_gap": [0, 106, 0, 106, 0],
       "sizes": (3, 2450, 0, 2, 12)}


@pytest.mark.parametrize("name", SC.PLANTED)
def test_planted_genomes_come_back_as_scaffolds(every, name):
    p, r = every[name]
    res = r["res"]
    assert sorted(len(m) for _, m in scaffolds_of(res)) == p.sizes and res["n_cut"] == p.n_cut
    check_against_genome(p, r["g"], res, p.jitter)                        # a fixed insert: every d of a bundle is equal, the gap is exact
    assert SF.insert_size(r["hist"]) == p.insert                          # the median of the same-contig pairs is the planted insert
    assert r["counts"].sum() == len(p.pairs) and r["counts"][1] > 0


@pytest.mark.parametrize("name", SC.PLANTED)
def test_properties(every, name):
    p, r = every[name]
    g, res, steps = r["g"], r["res"], r["steps"]
    U = g["U"]
    # a pair and its reverse complement give the same observation, wherever neither mate has two steps tied for the most windows
    back = [(SC.rc(b.decode()).encode(), SC.rc(a.decode()).encode()) for a, b in p.pairs]
    r2 = restated(p, back)
    sso, w = steps["seq_step_off"].tolist(), (steps["q_last"].astype(np.int64) - steps["q_first"] + 1).tolist()
    tied = lambda m: sorted(w[sso[m]:sso[m + 1]])[-2:].count(max(w[sso[m]:sso[m + 1]], default=0)) == 2
    clear = [i for i in range(len(p.pairs)) if not tied(2 * i) and not tied(2 * i + 1)]
    assert len(clear) > len(p.pairs) // 2
    assert np.array_equal(r2["key"][clear], r["key"][clear]) and np.array_equal(r2["d"][clear], r["d"][clear])
    # join is symmetric
    jn = res["join"].tolist()
    for e, t in enumerate(jn):
        if t != NONE32:
            assert jn[t ^ 1] == e ^ 1 and res["join_count"][t ^ 1] == res["join_count"][e] and res["join_gap"][t ^ 1] == res["join_gap"][e]
    # every contig is in exactly one scaffold; stripped of its N runs a scaffold is its members' oriented bases
    assert sorted(int(w) >> 1 for w in res["member"]) == list(range(U))
    off, text = g["offsets"].tolist(), g["bases"].tobytes()
    for s, members in scaffolds_of(res):
        pieces = [SF.rc_bytes(text[off[u]:off[u + 1]]) if f else text[off[u]:off[u + 1]] for u, f, _ in members]
        assert [x for x in s.encode().split(b"N") if x] == pieces
        assert len(s) == sum(len(x) for x in pieces) + sum(max(gap, 1) for _, _, gap in members[1:])
    # no joins: the scaffolds are the contigs
    none = SF.scaffold(g["offsets"], g["bases"], g["circular"], r["key"][:0], r["d"][:0], p.insert)
    assert np.array_equal(none["scaffold_offsets"], g["offsets"]) and np.array_equal(none["scaffold_bases"], g["bases"])
    assert none["member"].tolist() == [2 * u for u in range(U)] and none["contig_scaffold"].tolist() == list(range(U)) and not none["contig_pos"].any()
    assert np.array_equal(none["member_off"], np.arange(U + 1, dtype=np.uint64)) and not none["member_gap"].any() and none["S"] == 0
    # the histogram is accumulated
    twice = SF.mate_links(offsets_of(r["seqs"]), steps, g["offsets"], g["circular"], 1, MAX_INSERT, insert_hist=r["hist"])[3]
    assert np.array_equal(twice, r["hist"] * np.uint64(2))


@pytest.mark.parametrize("seed", (0, 1))
def test_scaffold_graph_structures(seed):
    g = SC.make_scaffold_graph(seed)
    U, par = g["U"], g["params"]
    sl = {k: g[k] for k in ("slink_off", "slink_to", "slink_count", "slink_dsum")}
    got = SF.bundle(g["obs_key"], g["obs_d"], U)
    for k in sl:
        assert got[k].dtype == g["obs_slinks"][k].dtype and np.array_equal(got[k], g["obs_slinks"][k]), k
    degree = np.diff(g["slink_off"].astype(np.int64))
    assert {1, 5, 70} <= set(degree.tolist())
    mk = SF.mark(g["offsets"], g["circular"], sl, **par)
    jn = mk["join"].tolist()
    for e, t in g["want_join"]:
        assert jn[e] == t and jn[t ^ 1] == e ^ 1, (e, t)
    for e in g["want_free"]:
        assert jn[e] == NONE32, e
    assert mk["n_joins"] == len(g["want_join"]) == sum(t != NONE32 for t in jn) // 2
    # a 64-bit product would have decided the wrapped case otherwise
    wrapped = [e for e in g["want_free"] if any(int(c) == SC.BIG_THIRD for c in g["slink_count"][int(g["slink_off"][e]):int(g["slink_off"][e + 1])])]
    assert len(wrapped) == 1 and (SC.BIG_THIRD * par["dominance"]) & SF.NOKEY <= (1 << 63) + 5 < SC.BIG_THIRD * par["dominance"]
    gaps = set(mk["join_gap"].tolist())
    assert {-7, 0, 1, 299} <= gaps
    lay = SF.layout(g["offsets"], mk["join"], mk["join_count"], mk["join_gap"], SC.MIN_GAP)
    assert lay["n_cut"] == 5
    members = lambda ids: sorted(lay["contig_rank"][ids].tolist()) == list(range(len(ids))) and len(set(lay["contig_scaffold"][ids].tolist())) == 1
    for tag, ids in g["chains"].items():
        assert members(ids) == (tag != "tiny"), tag
        if tag != "tiny":
            first = ids[int(np.argmin(lay["contig_rank"][ids]))]
            assert first == min(ids[0], ids[-1]) or tag in ("cycle2", "cycle3", "cycle65", "tied", "clamped")
    lens = np.diff(g["offsets"].astype(np.int64))
    assert (lens == 23).sum() == 3
    em = SF.emit(g["offsets"], g["bases"], mk["join"], mk["join_gap"], lay, SC.MIN_GAP)
    assert int(em["scaffold_offsets"][-1]) == lay["total_bases"] == int(lens.sum()) + sum(max(int(x), 1) for e, x in enumerate(mk["join_gap"]) if jn[e] != NONE32) // 2 - \
        sum(max(int(mk["join_gap"][e]), 1) for e in cut_ends(mk, lay))
    ids0 = np.argsort(lay["contig_scaffold"], kind="stable")
    firsts = [int(u) for u in ids0 if lay["contig_rank"][u] == 0]
    assert firsts == sorted(firsts) and len(firsts) == lay["n_scaffolds"]
    # with min_contig_bases 0 the contigs of 23 bases and the short one join too
    mk0 = SF.mark(g["offsets"], g["circular"], sl, **dict(par, min_contig_bases=0))
    lay0 = SF.layout(g["offsets"], mk0["join"], mk0["join_count"], mk0["join_gap"], SC.MIN_GAP)
    t = g["chains"]["tiny"]
    assert mk0["n_joins"] > mk["n_joins"] and len(set(lay0["contig_scaffold"][t].tolist())) == 1
    with pytest.raises(ValueError):
        SF.mark(g["offsets"], g["circular"], dict(sl, slink_count=np.concatenate([[sl["slink_count"][0] + np.uint64(1)], sl["slink_count"][1:]])), **par)
    with pytest.raises(ValueError):
        SF.bundle(np.array([(3 << 32) | 2], np.uint64), np.array([5], np.uint32), U)       # within one contig
    with pytest.raises(ValueError):
        SF.bundle(g["obs_key"][g["obs_key"] != SF.NOKEY][:1], np.array([0], np.uint32), U)  # d == 0
    bad = mk["join"].copy()
    bad[g["want_join"][0][0]] = NONE32
    with pytest.raises(ValueError):
        SF.layout(g["offsets"], bad, mk["join_count"], mk["join_gap"])
    with pytest.raises(ValueError):
        SF.emit(g["offsets"], g["bases"], mk["join"], mk["join_gap"], dict(lay, contig_flag=lay["contig_flag"] ^ np.uint8(1)))
    with pytest.raises(ValueError):
        SF.emit(g["offsets"], g["bases"], mk["join"], mk["join_gap"], dict(lay, total_bases=lay["total_bases"] + 1))


def cut_ends(mk, lay):
    """one end per join that the layout cut: a join e -> t that no scaffold realises as a member left through e and the next entered as t"""
    jn, rank, flag = mk["join"].tolist(), lay["contig_rank"].tolist(), lay["contig_flag"].tolist()
    follows = lambda e, t: flag[e >> 1] == e & 1 and flag[t >> 1] == t & 1 and rank[t >> 1] == rank[e >> 1] + 1
    return [e for e, t in enumerate(jn) if t != NONE32 and e < t ^ 1 and not follows(e, t) and not follows(t ^ 1, e ^ 1)]


def test_cycle_cuts():
    """the weakest join goes; ties on count are decided by the smaller end id; counts are clamped to 2^32 - 1 in the key"""
    g = SC.make_scaffold_graph(0)
    sl = {k: g[k] for k in ("slink_off", "slink_to", "slink_count", "slink_dsum")}
    mk = SF.mark(g["offsets"], g["circular"], sl, **g["params"])
    lay = SF.layout(g["offsets"], mk["join"], mk["join_count"], mk["join_gap"], SC.MIN_GAP)
    jn, jc = mk["join"].tolist(), mk["join_count"].tolist()
    cut = cut_ends(mk, lay)
    assert len(cut) == 5
    for tag in ("cycle2", "cycle3", "cycle65", "tied", "clamped"):
        ids = set(g["chains"][tag])
        ends = [e for e in range(2 * g["U"]) if e >> 1 in ids and jn[e] != NONE32 and e < jn[e] ^ 1]
        assert len(ends) == len(ids)
        key = lambda e: (min(jc[e], SF.M32), e)
        mine = [e for e in cut if e >> 1 in ids]
        assert mine == [min(ends, key=key)], tag


@pytest.mark.parametrize("U", (65, 257, 3 * 256 + 1))
def test_chains_in_random_order(U):
    """make_chains: chains and cycles among U contigs; every contig in one scaffold, every cycle cut once, positions that add up"""
    c = SC.make_chains(U, U)
    mk = SF.mark(c["offsets"], c["circular"], c, **c["params"])
    lay = SF.layout(c["offsets"], mk["join"], mk["join_count"], mk["join_gap"])
    em = SF.emit(c["offsets"], c["bases"], mk["join"], mk["join_gap"], lay)
    assert mk["n_joins"] == c["S"] // 2 and lay["n_cut"] > 0 and lay["n_scaffolds"] == U - mk["n_joins"] + lay["n_cut"]
    assert sorted(int(w) >> 1 for w in em["member"]) == list(range(U)) and len(cut_ends(mk, lay)) == lay["n_cut"]
    assert int(em["scaffold_offsets"][-1]) == lay["total_bases"] and (em["scaffold_bases"] == ord("N")).sum() == \
        sum(max(int(x), 1) for x, w in zip(em["member_gap"], em["member"]) if lay["contig_rank"][int(w) >> 1])


def test_a_mate_that_ends_before_its_contig_is_discordant():
    """hand-set steps only: d < 1 is no observation, d == 1 is the smallest one"""
    g = SC.make_scaffold_graph(0)
    offs, steps, (u, v) = SC.make_pairs_before_contig(g["offsets"], g["circular"])
    key, d, counts, hist = SF.mate_links(offs, steps, g["offsets"], g["circular"], 1, 150)
    assert key.tolist() == [SF.NOKEY, SF.NOKEY, (2 * u) << 32 | 2 * v] and d.tolist() == [0, 0, 1]
    assert counts.tolist() == [0, 1, 2, 0] and not hist.any()


def test_null_pointers_and_sizes_are_refused_before_any_device_call():
    """Runs without a GPU: the handle-less entry points decide a NULL pointer and an impossible size before anything is allocated or
    launched."""
    L = _lib.lib()
    a = np.zeros(64, np.uint64)
    p = a.ctypes.data_as(C.c_void_p)
    n = [C.c_uint64(77) for _ in range(4)]
    r = [C.byref(x) for x in n]
    ARG, UNS, BIG = _lib.AIX_ERR_ARG, _lib.AIX_ERR_UNSUPPORTED, (1 << 31) - 3
    call = lambda fn, spec, **o: fn(*[o.get(k, v) for k, v in spec])
    ml = (("P", 1), ("offs", p), ("sso", p), ("T", 1), ("su", p), ("sp", p), ("sf", p), ("qf", p), ("ql", p), ("U", 1), ("off", p), ("circ", p), ("maw", 1), ("mi", 1000),
          ("hist", p), ("key", p), ("d", p), ("counts", p), ("st", None))
    for k in ("offs", "sso", "su", "sp", "sf", "qf", "ql", "off", "circ", "hist", "key", "d", "counts"):
        assert call(L.aix_mate_links_dev, ml, **{k: None}) == ARG, k
    assert call(L.aix_mate_links_dev, ml, maw=0) == ARG and call(L.aix_mate_links_dev, ml, mi=0) == ARG and call(L.aix_mate_links_dev, ml, mi=(1 << 20) + 1) == ARG
    assert call(L.aix_mate_links_dev, ml, U=BIG) == UNS and call(L.aix_mate_links_dev, ml, U=0, circ=None) == ARG
    bd = (("N", 1), ("key", p), ("d", p), ("U", 1), ("lo", p), ("to", p), ("cnt", p), ("ds", p), ("cap", 2), ("tot", r[0]), ("st", None))
    for k in ("key", "d", "lo", "to", "cnt", "ds", "tot"):
        assert call(L.aix_mate_bundle_dev, bd, **{k: None}) == ARG, k
    assert call(L.aix_mate_bundle_dev, bd, U=BIG) == UNS and call(L.aix_mate_bundle_dev, bd, N=1 << 32) == UNS      # a bundle is named by 32 bits
    mk = (("U", 1), ("off", p), ("circ", p), ("lo", p), ("to", p), ("cnt", p), ("ds", p), ("S", 2), ("ins", 300), ("mp", 2), ("dom", 2), ("mb", 0), ("jn", p), ("jc", p),
          ("jg", p), ("n", r[0]), ("st", None))
    for k in ("off", "circ", "lo", "to", "cnt", "ds", "jn", "jc", "jg", "n"):
        assert call(L.aix_scaffold_mark_dev, mk, **{k: None}) == ARG, k
    assert call(L.aix_scaffold_mark_dev, mk, mp=0) == ARG and call(L.aix_scaffold_mark_dev, mk, dom=0) == ARG and call(L.aix_scaffold_mark_dev, mk, S=3) == ARG
    assert call(L.aix_scaffold_mark_dev, mk, U=BIG) == UNS
    ly = (("U", 1), ("off", p), ("jn", p), ("jc", p), ("jg", p), ("mg", 1), ("cs", p), ("cr", p), ("cp", p), ("cf", p), ("n0", r[0]), ("n1", r[1]), ("n2", r[2]), ("st", None))
    for k in ("off", "jn", "jc", "jg", "cs", "cr", "cp", "cf", "n0", "n1", "n2"):
        assert call(L.aix_scaffold_layout_dev, ly, **{k: None}) == ARG, k
    assert call(L.aix_scaffold_layout_dev, ly, mg=0) == ARG and call(L.aix_scaffold_layout_dev, ly, U=BIG) == UNS
    em = (("U", 1), ("off", p), ("bases", p), ("jn", p), ("jg", p), ("mg", 1), ("cs", p), ("cr", p), ("cp", p), ("cf", p), ("Sc", 1), ("tot", 23), ("so", p), ("sb", p),
          ("mo", p), ("mm", p), ("mgap", p), ("st", None))
    for k in ("off", "bases", "jn", "jg", "cs", "cr", "cp", "cf", "so", "sb", "mo", "mm", "mgap"):
        assert call(L.aix_scaffold_emit_dev, em, **{k: None}) == ARG, k
    assert call(L.aix_scaffold_emit_dev, em, mg=0) == ARG and call(L.aix_scaffold_emit_dev, em, Sc=0) == ARG and call(L.aix_scaffold_emit_dev, em, Sc=2) == ARG
    assert call(L.aix_scaffold_emit_dev, em, tot=22) == ARG and call(L.aix_scaffold_emit_dev, em, U=BIG) == UNS
    outs = [C.byref(C.c_void_p()) for _ in range(12)]
    host = lambda **o: L.aix_scaffold(*[o.get(k, v) for k, v in (("U", 1), ("off", p), ("bases", p), ("circ", p), ("N", 1), ("key", p), ("d", p), ("ins", 300), ("mp", 2),
                                                                  ("dom", 2), ("mb", 0), ("mg", 1))], *r, *outs)
    for k in ("off", "bases", "circ", "key", "d"):
        assert host(**{k: None}) == ARG, k
    assert host(mp=0) == ARG and host(dom=0) == ARG and host(mg=0) == ARG and host(U=BIG) == UNS and host(N=1 << 32) == UNS
    assert host() == ARG                                                  # offsets[1] == 0: no contig of 23 bases
    assert all(x.value == 77 for x in n)
