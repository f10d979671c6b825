"""Pins the test-side restatement of the gap closing (tests/gap_close_ref.py) and the inputs of tests/gap_close_cases.py, without a GPU:
literals, the planted genomes recovered whole as filled scaffolds, the properties of the contract, and the refusals of the handle-less
entry points that are decided before any device call. Every test asks the built library for the entry points first."""
import ctypes as C

import numpy as np
import pytest

import gap_close_cases as GC
import gap_close_ref as GF
import graph_clean_ref as GR
import scaffold_cases as SC
import scaffold_ref as SF
import seqthread_ref as SR
import unitig_links_ref as RL
import unitigs_ref as R
from aindex_amd import _lib

NONE32 = SF.NONE32
ENTRY_POINTS = ("aix_gap_close_dev", "aix_scaffold_fill_layout_dev", "aix_scaffold_fill_emit_dev", "aix_scaffold_fill")
GRAPH = ("offsets", "link_off", "link_to", "join", "join_gap")


@pytest.fixture(scope="module", autouse=True)
def library():
    """The restatement is pinned for the library that states the same contract: without its entry points every test here fails."""
    L = _lib.lib()
    return [getattr(L, name) for name in ENTRY_POINTS]


def restated(p):
    """a planted case through the restatements: the graph, its mates threaded, the scaffolds (as tests/test_scaffold_cpu.py)"""
    un = R.unitigs(p.codes, p.tfs, 0)
    lk = RL.links(p.codes, p.tfs, 0, un)
    g = GR.graph(un, lk)
    node = SR.nodes(un["kid_unitig"], un["kid_pos"], un["kid_flag"], un["offsets"])
    kid_of = {int(c): i for i, c in enumerate(p.codes.tolist())}
    seqs = SC.mates(p.pairs)
    steps = SR.thread(kid_of, node, g, seqs)
    offs = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    key, d, _, _ = SF.mate_links(offs, steps, g["offsets"], g["circular"], 1, 1000)
    return g, SF.scaffold(g["offsets"], g["bases"], g["circular"], key, d, p.insert, 2, 2, SC.MIN_BASES, 1)


def filled(g, res, **kw):
    return GF.fill(g["offsets"], g["bases"], g["link_off"], g["link_to"], res["join"], res["join_gap"], res["member_off"], res["member"], **kw)


@pytest.fixture(scope="module")
def every():
    out = {}
    for name in SC.PLANTED:
        p = SC.planted(name)
        g, res = restated(p)
        out[name] = (p, g, res, filled(g, res, tolerance=10))
    return out


def texts(bases, offsets):
    text, so = bases.tobytes().decode(), offsets.tolist()
    return [text[a:b] for a, b in zip(so, so[1:])]


def at_probe(g, r):
    e = g["probe"]
    return int(r["close_status"][e]), int(r["close_states"][e]), int(r["close_dist"][e]), r["path"][int(r["path_off"][e]):int(r["path_off"][e + 1])].tolist()


def search(g, **params):
    return GF.search(*[g[k] for k in GRAPH], **params)


def scaffolds_of(g, min_gap=1):
    lay = SF.layout(g["offsets"], g["join"], g["join_count"], g["join_gap"], min_gap)
    return SF.emit(g["offsets"], g["bases"], g["join"], g["join_gap"], lay, min_gap)


@pytest.mark.parametrize("dual", (True, False))
@pytest.mark.parametrize("name", GC.NAMES)
def test_literals_of_the_hand_made_cases(name, dual):
    g, params, want = GC.case(name, dual)
    r = search(g, **params)
    assert at_probe(g, r) == want
    e, t = g["probe"], int(g["join"][g["probe"]])
    assert r["close_status"][t ^ 1] == want[0] and r["close_dist"][t ^ 1] == want[2] and r["close_states"][t ^ 1] == want[1]
    assert r["counts"][want[0] - 1] >= 1 and r["counts"][4] == (g["join"] != NONE32).sum() // 2 == r["counts"][:4].sum()
    if want[0] == 3:                                                      # the budget: exactly the states of the complete search, and one fewer
        n = want[1]
        assert at_probe(g, search(g, **dict(params, max_states=n)))[:2] == (3, n)
        if n > 1:
            assert at_probe(g, search(g, **dict(params, max_states=n - 1))) == (4, n - 1, 0, [])


def test_hits_of_the_ambiguous_cases():
    """2 hits in the diamond, 3 around the self-linked repeat, 2^b behind b bubbles: the states less the intermediates"""
    for name, hits in (("diamond_60_60", 2), ("selfloop_tol70", 3), ("bubbles_1", 2), ("bubbles_3", 8), ("bubbles_6", 64), ("bubbles_10", 1024)):
        g, params, want = GC.case(name)
        off, U, lo, to, jn, jg = GF._graph(*[g[k] for k in GRAPH])
        e = g["probe"]
        # the rule with a budget nobody reaches and every hit counted
        states, got, cand = 0, 0, [(x, -22, 0) for x in to[lo[e]:lo[e + 1]]]
        while cand:
            w, d, k = cand.pop()
            L = off[(w >> 1) + 1] - off[w >> 1]
            if w == jn[e]:
                keep = abs(d - jg[e]) <= params["tolerance"]
                got += keep
            else:
                keep = k < params["max_fill"] and jn[w & ~1] == NONE32 and jn[w | 1] == NONE32 and d + L - 22 <= jg[e] + params["tolerance"]
                if keep:
                    cand += [(y, d + L - 22, k + 1) for y in to[lo[w]:lo[w + 1]]]
            states += keep
        assert (got, states) == (hits, want[1]), name                     # depth first here, breadth first there: the same set


def test_literals_of_the_two_copy_case(every):
    """A R B and C R D with R of 150 bases (contig 2): both joins close through R at 150 - 44 = 106 bases, and R's own scaffold is what
    drop_absorbed leaves out."""
    p, g, res, f = every["two_copy"]
    assert g["link_off"].tolist() == [0, 1, 1, 2, 2, 4, 6, 7, 7, 7, 8] and g["link_to"].tolist() == [4, 4, 7, 8, 1, 3, 5, 5]
    for k, v in LIT.items():
        assert f[k].tolist() == v, k
    for k, dt in (("close_status", np.uint8), ("close_dist", np.int64), ("close_states", np.uint32), ("path_off", np.uint64), ("path", np.uint32),
                  ("fill_uses", np.uint32), ("counts", np.uint64), ("fmember_off", np.uint64), ("fmember", np.uint32), ("fmember_flag", np.uint8),
                  ("fmember_gap", np.int64), ("fmember_pos", np.uint64), ("fscaffold_offsets", np.uint64), ("fscaffold_bases", np.uint8)):
        assert f[k].dtype == dt, k
    assert (f["total"], f["n_fmembers"], f["total_bases"]) == (2, 7, 2450)


LIT = {"close_status": [1, 0, 1, 0, 0, 0, 1, 0, 0, 1], "close_dist": [106, 0, 106, 0, 0, 0, 106, 0, 0, 106], "close_states": [2, 0, 2, 0, 0, 0, 2, 0, 0, 2],
       "path_off": [0, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2], "path": [4, 4], "fill_uses": [0, 0, 2, 0, 0], "counts": [2, 0, 0, 0, 2],
       "fmember_off": [0, 3, 6, 7], "fmember": [0, 4, 7, 2, 4, 8, 4], "fmember_flag": [0, 3, 1, 0, 3, 1, 0], "fmember_gap": [0, 0, 106, 0, 0, 106, 0],
       "fmember_pos": [0, 522, 650, 0, 522, 650, 0], "fscaffold_offsets": [0, 1150, 2300, 2450]}
FILLED_LENGTHS = {"two_copy": [1150, 1150], "jitter": [1150, 1150], "inverted": [1800], "chain3": [1800, 1800], "cycle": [1844]}


@pytest.mark.parametrize("name", SC.PLANTED)
def test_planted_genomes_come_back_filled(every, name):
    p, g, res, f = every[name]
    n_joins = int((res["join"] != NONE32).sum()) // 2
    assert f["counts"].tolist() == [n_joins, 0, 0, 0, n_joins] and n_joins > 0       # every join closes, the cut one of the ring too
    seqs = texts(f["fscaffold_bases"], f["fscaffold_offsets"])
    assert all(SC.located(p, s) is not None for s in seqs) and not any("N" in s for s in seqs)
    fo, mo = f["fmember_off"].tolist(), res["member_off"].tolist()
    multi = [s for s in range(len(seqs)) if mo[s + 1] - mo[s] > 1]
    assert [len(seqs[s]) for s in multi] == FILLED_LENGTHS[name]
    if name != "cycle":
        assert sorted(len(s) for s in seqs if len(s) > 200) == sorted(len(x) for x in p.genomes)      # the whole planted genomes
    # drop_absorbed: a single-contig scaffold whose contig fills a gap goes; only the multi-member scaffolds remain
    uses = f["fill_uses"].tolist()
    kept = [s for s in range(len(seqs)) if not (fo[s + 1] - fo[s] == 1 and uses[int(f["fmember"][fo[s]]) >> 1] >= 1)]
    assert kept == multi


@pytest.mark.parametrize("name", SC.PLANTED)
def test_properties_of_the_planted_cases(every, name):
    p, g, res, f = every[name]
    check_properties(g, res["join"], res["join_gap"], res, f, dict(tolerance=10))


@pytest.mark.parametrize("seed,J", ((0, 65), (1, 257)))
def test_properties_of_the_generated_batches(seed, J):
    g = GC.make_batch(seed, J)
    em = scaffolds_of(g)
    f = filled(g, dict(em, join=g["join"], join_gap=g["join_gap"]), **GC.PARAMS)
    assert f["counts"][4] == J and (f["counts"][:3] > 0).all()
    check_properties(g, g["join"], g["join_gap"], em, f, GC.PARAMS)


def reversed_graph(g, join, join_gap):
    """every contig reverse-complemented in place: word w becomes w ^ 1, a link a -> b stays a link between the same ends"""
    U = g["U"]
    lists = [[] for _ in range(2 * U)]
    lo, to = g["link_off"].tolist(), g["link_to"].tolist()
    for a in range(2 * U):
        lists[a ^ 1] = [w ^ 1 for w in to[lo[a]:lo[a + 1]]]
    jn = np.full(2 * U, NONE32, np.uint32)
    jg = np.zeros(2 * U, np.int64)
    for e, t in enumerate(join.tolist()):
        if t != NONE32:
            jn[e ^ 1], jg[e ^ 1] = t ^ 1, join_gap[e]
    return (g["offsets"], np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint64), np.array([x for l in lists for x in l], np.uint32), jn, jg)


def check_properties(g, join, join_gap, em, f, params):
    U, jn = g["U"], join.tolist()
    po, path = f["path_off"].tolist(), f["path"].tolist()
    # status, dist and states are equal at both ends; only the owner of a closed join has a path
    for e, t in enumerate(jn):
        if t == NONE32:
            assert f["close_status"][e] == 0 and po[e + 1] == po[e]
            continue
        for k in ("close_status", "close_dist", "close_states"):
            assert f[k][e] == f[k][t ^ 1], (k, e)
        assert f["close_status"][e] in (1, 2, 3, 4) and (po[e + 1] == po[e] or (f["close_status"][e] == 1 and e < t ^ 1))
    # the graph with every contig turned round: the same statuses, the paths reversed (nothing here is exhausted in one direction only)
    rev = GF.search(*reversed_graph(g, join, join_gap), **params)
    rpo, rpath = rev["path_off"].tolist(), rev["path"].tolist()
    for e, t in enumerate(jn):
        if t != NONE32 and e < t ^ 1 and f["close_status"][e] != 4 and rev["close_status"][e ^ 1] != 4:
            assert rev["close_status"][e ^ 1] == f["close_status"][e] and rev["close_dist"][e ^ 1] == f["close_dist"][e]
            o = min(e ^ 1, t)                                             # the owner of e ^ 1 -> t ^ 1 read as a join of the reversed graph: t -> e
            mine = [w ^ 1 for w in path[po[e]:po[e + 1]]]
            assert rpath[rpo[o]:rpo[o + 1]] == (mine if o == e ^ 1 else [w ^ 1 for w in reversed(mine)])
    # no closure gives the identity
    none = GF.fill_layout(*[g[k] for k in GRAPH[:3]], join, join_gap, em["member_off"], em["member"], GF.no_closure(U))
    assert np.array_equal(none["fmember"], em["member"]) and np.array_equal(none["fmember_off"], em["member_off"]) and not none["fmember_flag"].any()
    assert np.array_equal(none["fmember_gap"], em["member_gap"]) and np.array_equal(none["fscaffold_offsets"], em["scaffold_offsets"])
    assert np.array_equal(GF.fill_emit(g["offsets"], g["bases"], none), em["scaffold_bases"])
    # the filled scaffold with its fill members removed and 'N' restored is the scaffold
    off, text = g["offsets"].tolist(), g["bases"].tobytes()
    fo, fm, ff, fg, fp = (f[k].tolist() for k in ("fmember_off", "fmember", "fmember_flag", "fmember_gap", "fmember_pos"))
    fseq, seq, mg = texts(f["fscaffold_bases"], f["fscaffold_offsets"]), texts(em["scaffold_bases"], em["scaffold_offsets"]), em["member_gap"].tolist()
    i = 0
    for s in range(len(fo) - 1):
        back = ""
        for j in range(fo[s], fo[s + 1]):
            w = fm[j]
            piece = text[off[w >> 1]:off[(w >> 1) + 1]]
            piece = (SF.rc_bytes(piece) if w & 1 else piece).decode()
            assert fseq[s][fp[j]:fp[j] + len(piece) - 22 * (ff[j] & 1)] == piece[22 * (ff[j] & 1):]
            if ff[j] & 2:
                continue
            if j > fo[s]:
                back += "N" * max(mg[i], 1)
                assert fg[j] == (f["close_dist"][fm[j] ^ 1] if ff[j] else mg[i])
            back += piece
            i += 1
        assert back == seq[s]
    assert i == U


def test_a_non_owner_traversal_reverses_the_path():
    g, (a, c, z), (p, q, r) = GC.non_owner_case()
    em = scaffolds_of(g)
    assert em["member"].tolist()[:3] == [2 * a, 2 * c, 2 * z] and c > z    # c -> z is owned by z's side
    f = filled(g, dict(em, join=g["join"], join_gap=g["join_gap"]), tolerance=0)
    assert f["counts"].tolist() == [2, 0, 0, 0, 2]
    po, path = f["path_off"].tolist(), f["path"].tolist()
    assert path[po[2 * a]:po[2 * a + 1]] == [2 * p, 2 * q + 1] and path[po[2 * z + 1]:po[2 * z + 2]] == [2 * r + 1] and po[2 * c + 1] == po[2 * c]
    assert f["fmember"].tolist()[:6] == [2 * a, 2 * p, 2 * q + 1, 2 * c, 2 * r, 2 * z] and f["fmember_flag"].tolist()[:6] == [0, 3, 3, 1, 3, 1]
    assert f["fmember_gap"].tolist()[:6] == [0, 0, 0, 94, 0, 26] and f["fmember_pos"].tolist()[:6] == [0, 60, 98, 176, 214, 262]
    assert f["fscaffold_offsets"].tolist()[:2] == [0, 300] and f["fill_uses"].tolist() == [int(u in (p, q, r)) for u in range(6)]
    # the second join left open at 400: its 'N' run stays
    g2, _, _ = GC.non_owner_case(400)
    em2 = scaffolds_of(g2)
    f2 = filled(g2, dict(em2, join=g2["join"], join_gap=g2["join_gap"]), tolerance=0)
    assert f2["counts"].tolist() == [1, 1, 0, 0, 2] and f2["fmember_flag"].tolist()[:5] == [0, 3, 3, 1, 0] and f2["fmember_gap"].tolist()[:5] == [0, 0, 0, 94, 400]
    assert f2["fmember_pos"].tolist()[:5] == [0, 60, 98, 176, 214 + 400]


def test_a_gap_below_min_gap_and_a_negative_distance():
    g = GC.below_min_gap_case()
    em = scaffolds_of(g, 3)
    f = filled(g, dict(em, join=g["join"], join_gap=g["join_gap"]), tolerance=5, min_gap=3)
    assert f["counts"].tolist() == [1, 1, 0, 0, 2] and f["close_dist"].tolist() == [-22, 0, 0, -22, 0, 0] and f["total"] == 0
    assert f["fmember"].tolist() == [0, 2, 4] and f["fmember_flag"].tolist() == [0, 1, 0] and f["fmember_gap"].tolist() == [0, -22, -5]
    assert f["fmember_pos"].tolist() == [0, 60, 98 + 3] and f["fscaffold_offsets"].tolist() == [0, 161]
    s = f["fscaffold_bases"].tobytes().decode()
    assert s[98:101] == "NNN" and s.count("N") == 3 and s[38:60] == GC.X == s[:22]


def test_the_restatement_refuses():
    g, params, _ = GC.case("diamond_60_100")
    em = scaffolds_of(g)
    cl = search(g, **params)
    args = lambda **o: [o.get(k, g[k]) for k in GRAPH]
    for bad in (dict(tolerance=(1 << 20) + 1), dict(tolerance=-1), dict(max_fill=65), dict(max_states=0), dict(max_states=4097)):
        with pytest.raises(ValueError):
            search(g, **dict(params, **bad))
    big = g["join_gap"].copy()
    big[g["join"] != NONE32] = (1 << 30) + 1
    lone = g["join"].copy()
    lone[g["probe"]] = NONE32
    for o in (dict(join_gap=big), dict(join=lone), dict(link_to=g["link_to"] + np.uint32(2 * g["U"])), dict(link_off=g["link_off"][::-1].copy())):
        with pytest.raises(ValueError):
            GF.search(*args(**o), **params)
    lay = lambda **o: GF.fill_layout(*args(), o.get("member_off", em["member_off"]), o.get("member", em["member"]), {**cl, **o})
    assert lay()["n_fmembers"] == g["U"] + 1
    e = g["probe"]
    t = int(g["join"][e])
    free = [x for x in range(2 * g["U"]) if g["join"][x] == NONE32][0]
    poke = lambda k, i, v: {k: np.concatenate([cl[k][:i], [v], cl[k][i + 1:]]).astype(cl[k].dtype)}
    other = [u for u in range(g["U"]) if 2 * u not in (e, t) and 2 * u != int(cl["path"][0])][0]
    for o in (poke("close_dist", e, 17), poke("close_dist", t ^ 1, 17), poke("close_status", free, 2), poke("close_status", e, 5), poke("close_status", t ^ 1, 2),
              poke("path", 0, 2 * other + 1), poke("path", 0, 2 * g["U"]), dict(member=em["member"][::-1].copy()),
              dict(path_off=np.roll(cl["path_off"], 1)), dict(member=np.zeros_like(em["member"]))):
        with pytest.raises(ValueError):
            lay(**o)
    good = lay()
    for o in (dict(fmember_pos=good["fmember_pos"] + np.uint64(1)), dict(fmember_flag=good["fmember_flag"] | np.uint8(2)), dict(total_bases=good["total_bases"] + 1),
              dict(fmember=good["fmember"] + np.uint32(2 * g["U"])), dict(fscaffold_offsets=good["fscaffold_offsets"] + np.uint64(1))):
        with pytest.raises(ValueError):
            GF.fill_emit(g["offsets"], g["bases"], {**good, **o})


def test_null_pointers_and_sizes_are_refused_before_any_device_call():
    """Runs without a GPU: the four entry points decide a NULL pointer and an impossible size before anything is allocated or launched."""
    L = _lib.lib()
    a = np.zeros(64, np.uint64)
    p = a.ctypes.data_as(C.c_void_p)
    n = [C.c_uint64(77) for _ in range(3)]
    r = [C.byref(x) for x in n]
    ARG, UNS, BIG = _lib.AIX_ERR_ARG, _lib.AIX_ERR_UNSUPPORTED, (1 << 31) - 3
    call = lambda fn, spec, **o: fn(*[o.get(k, v) for k, v in spec])
    gc = (("U", 1), ("off", p), ("lo", p), ("lt", p), ("E", 1), ("jn", p), ("jg", p), ("tol", 50), ("mf", 16), ("ms", 1024), ("cs", p), ("cd", p), ("cn", p), ("po", p),
          ("pa", p), ("cap", 4), ("tot", r[0]), ("fu", p), ("ct", p), ("st", None))
    for k in ("off", "lo", "lt", "jn", "jg", "cs", "cd", "cn", "po", "pa", "tot", "fu", "ct"):
        assert call(L.aix_gap_close_dev, gc, **{k: None}) == ARG, k
    for o in (dict(tol=(1 << 20) + 1), dict(mf=65), dict(ms=0), dict(ms=4097), dict(U=0), dict(E=1 << 60)):      # U == 0 with a link
        assert call(L.aix_gap_close_dev, gc, **o) == ARG, o
    assert call(L.aix_gap_close_dev, gc, U=BIG) == UNS
    ly = (("U", 1), ("off", p), ("lo", p), ("lt", p), ("E", 1), ("jn", p), ("jg", p), ("mg", 1), ("Sc", 1), ("mo", p), ("mm", p), ("cs", p), ("cd", p), ("po", p), ("pa", p),
          ("pt", 1), ("fo", p), ("fm", p), ("ff", p), ("fg", p), ("fp", p), ("fso", p), ("n0", r[0]), ("n1", r[1]), ("st", None))
    for k in ("off", "lo", "lt", "jn", "jg", "mo", "mm", "cs", "cd", "po", "pa", "fo", "fm", "ff", "fg", "fp", "fso", "n0", "n1"):
        assert call(L.aix_scaffold_fill_layout_dev, ly, **{k: None}) == ARG, k
    for o in (dict(mg=0), dict(Sc=0), dict(Sc=2), dict(pt=1 << 60), dict(U=0, Sc=0, E=0)):                        # U == 0 with a path entry
        assert call(L.aix_scaffold_fill_layout_dev, ly, **o) == ARG, o
    assert call(L.aix_scaffold_fill_layout_dev, ly, U=BIG) == UNS
    em = (("U", 1), ("off", p), ("bases", p), ("mg", 1), ("Sc", 1), ("fo", p), ("Mf", 1), ("fm", p), ("ff", p), ("fg", p), ("fp", p), ("fso", p), ("tot", 23), ("out", p),
          ("st", None))
    for k in ("off", "bases", "fo", "fm", "ff", "fg", "fp", "fso", "out"):
        assert call(L.aix_scaffold_fill_emit_dev, em, **{k: None}) == ARG, k
    for o in (dict(mg=0), dict(Sc=0), dict(Sc=2), dict(Mf=0), dict(tot=22), dict(U=0, Sc=0, Mf=0, tot=1)):
        assert call(L.aix_scaffold_fill_emit_dev, em, **o) == ARG, o
    assert call(L.aix_scaffold_fill_emit_dev, em, U=BIG) == UNS
    outs = [C.byref(C.c_void_p()) for _ in range(14)]
    spec = (("U", 1), ("off", p), ("bases", p), ("lo", p), ("lt", p), ("E", 1), ("jn", p), ("jg", p), ("Sc", 1), ("mo", p), ("mm", p), ("tol", 50), ("mf", 16), ("ms", 1024),
            ("mg", 1))
    host = lambda **o: L.aix_scaffold_fill(*[o.get(k, v) for k, v in spec], *o.get("r", r), *o.get("outs", outs))
    for k in ("off", "bases", "lo", "lt", "jn", "jg", "mo", "mm"):
        assert host(**{k: None}) == ARG, k
    for o in (dict(tol=(1 << 20) + 1), dict(mf=65), dict(ms=0), dict(mg=0), dict(Sc=0), dict(Sc=2), dict(r=[None] + r[1:]), dict(outs=[None] + outs[1:])):
        assert host(**o) == ARG, list(o)
    assert host(U=BIG) == UNS
    assert host() == ARG                                                  # offsets[1] == 0: no contig of 23 bases
    assert all(x.value == 77 for x in n)
