"""The phasing restatement (tests/phase_ref.py) pinned on literals worked by hand, its refusals, the property that a batch and its reverse
complement give the same observations, the presence of the five symbols, and the planted diploid case of tests/phase_cases.py through
the restated chain. No GPU: tests/test_gpu_phase.py holds the kernels to this restatement."""
import ctypes as C

import numpy as np
import pytest

import phase_cases as HC
import phase_ref as HR
import pileup_cases as PC
import pileup_fuzz_cases as FC
import pileup_ref as PR

NONE = HR.NONE
SYMBOLS = ("aix_phase_observe_dev", "aix_phase_bundle_dev", "aix_phase_solve_dev", "aix_phase_tag_dev", "aix_phase_solve")


def _links(rows):
    """[(lo, hi, cis, trans)] -> the link arrays, cis links first"""
    flat = [(lo, hi, r) for lo, hi, c, t in rows for r in [0] * c + [1] * t]
    cols = list(zip(*flat)) if flat else [[]] * 3
    return {k: np.array(col, dtype=dt) for k, dt, col in zip(HR.LINK_KEYS, HR.LINK_DTYPES, cols)}


def _solve(V, rows, reads=2, permille=800, unitig=None):
    edges = HR.bundle(V, _links(rows))
    return edges, HR.solve(np.zeros(V, np.uint32) if unitig is None else np.array(unitig, np.uint32), edges, reads, permille)


def _lay(contigs, reads):
    """reads: per sequence a list of (contig, pos, strand, text) laid at contig base pos — text is what the contig shows there, so a
    backward placement stores its reverse complement (bases only; other bytes stay) -> (seqs, places, offsets)"""
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    seqs, rows, spo = [], [], [0]
    for parts in reads:
        seq = b""
        for u, pos, s, text in parts:
            t = text.encode()
            rows.append((u, s, pos, len(seq), len(t)))
            seq += t[::-1].translate(comp) if s else t
        seqs.append(seq)
        spo.append(len(rows))
    cols = list(zip(*rows)) if rows else [[]] * 5
    places = {"seq_place_off": np.array(spo, np.uint64)}
    places.update({k: np.array(col, dtype=dt) for k, dt, col in zip(PR.PLACE_KEYS[1:6], PR.PLACE_DTYPES[1:6], cols)})
    return seqs, places, PC.seq_offs(contigs)


def test_symbols_are_declared_and_bound():
    from aindex_amd import _lib
    declared = _lib.header_symbols()
    assert all(s in declared and s in _lib.SIGNATURES for s in SYMBOLS)
    assert "#define AIX_PHASE_NONE 0xFFu" in open(_lib.HEADER).read() and _lib.PHASE_NONE == NONE == 0xFF


def test_null_pointers_and_sizes_are_refused_before_any_device_call():
    """Runs without a GPU: a NULL pointer where one is needed, a bad group and a size beyond a limit are decided before anything is
    allocated or launched."""
    from aindex_amd import _lib
    L = _lib.lib()
    a = np.zeros(8, np.uint64)
    p = a.ctypes.data_as(C.c_void_p)
    n, m = C.c_uint64(7), C.c_uint64(7)
    ARG, UNS = _lib.AIX_ERR_ARG, _lib.AIX_ERR_UNSUPPORTED
    big = (1 << 31) - 3

    def observe(**o):
        d = dict(seqs=p, offs=p, M=2, group=1, spo=p, R=1, pu=p, pf=p, pp=p, pq=p, pl=p, U=1, offsets=p, V=1, vu=p, vp=p, vr=p, va=p, foff=p, osite=p, oall=p,
                 ocap=1, ot=C.byref(n), llo=p, lhi=p, lrel=p, lcap=1, lt=C.byref(m), stats=None, stream=None)
        assert set(o) <= set(d)
        d.update(o)
        return L.aix_phase_observe_dev(*d.values())
    for k in ("seqs", "offs", "spo", "pu", "pf", "pp", "pq", "pl", "offsets", "vu", "vp", "vr", "va", "foff", "osite", "oall", "ot", "llo", "lhi", "lrel", "lt"):
        assert observe(**{k: None}) == ARG, k
    assert observe(group=0) == ARG and observe(group=3) == ARG and observe(group=2, M=3) == ARG and observe(M=0) == ARG and observe(U=0) == ARG
    assert observe(V=big) == UNS and observe(U=big) == UNS and observe(M=1 << 33) == UNS
    bundle = lambda V=2, N=1, **o: L.aix_phase_bundle_dev(V, N, *[o.get(k, p) for k in ("lo", "hi", "rel", "elo", "ehi", "cis", "trans", "eoff")], o.get("n", C.byref(n)), None)
    for k in ("lo", "hi", "rel", "elo", "ehi", "cis", "trans", "eoff", "n"):
        assert bundle(**{k: None}) == ARG, k
    assert bundle(V=big) == UNS and bundle(N=1 << 32) == UNS
    solve = lambda V=2, E=1, **o: L.aix_phase_solve_dev(V, o.get("vu", p), o.get("eoff", p), E, o.get("lo", p), o.get("cis", p), o.get("trans", p), 2, 800,
                                                        o.get("block", p), o.get("phase", p), None, None, None, None)
    for k in ("vu", "eoff", "lo", "cis", "trans", "block", "phase"):
        assert solve(**{k: None}) == ARG, k
    assert solve(V=0) == ARG and solve(V=big) == UNS
    tag = lambda F=1, n_obs=1, V=1, **o: L.aix_phase_tag_dev(F, o.get("foff", p), n_obs, o.get("site", p), o.get("allele", p), V, o.get("block", p), o.get("phase", p),
                                                             *[o.get(k, p) for k in ("tb", "h0", "h1", "other")], None)
    for k in ("foff", "site", "allele", "block", "phase", "tb", "h0", "h1", "other"):
        assert tag(**{k: None}) == ARG, k
    assert tag(F=0) == ARG and tag(V=0) == ARG and tag(V=big) == UNS
    outs = [C.c_void_p() for _ in range(10)]
    host = lambda V=2, N=1, **o: L.aix_phase_solve(V, o.get("vu", p), N, o.get("lo", p), o.get("hi", p), o.get("rel", p), 2, 800, o.get("n", C.byref(n)),
                                                   *[None if o.get("out") == i else C.byref(x) for i, x in enumerate(outs)])
    for k in ("vu", "lo", "hi", "rel", "n"):
        assert host(**{k: None}) == ARG, k
    for i in (0, 1, 2, 3, 4, 6, 7):                                 # edge_state (5), site_parent (8) and counts (9) are nullable
        assert host(out=i) == ARG, i
    assert host(V=big) == UNS and host(N=1 << 32) == UNS
    assert (n.value, m.value) == (7, 7) and all(x.value is None for x in outs)


def test_two_sites_three_fragments():
    """alleles (0,0), (1,1), (0,1): cis 2, trans 1"""
    contig = "ACGTACGTAC" * 5                                       # sites at 10 (A -> C) and 30 (A -> G)
    sites = HC.sites_dict([(10, "A", "C"), (30, "A", "G")])
    show = lambda a, b: contig[5:10] + "AC"[a] + contig[11:30] + "AG"[b] + contig[31:40]
    seqs, places, off = _lay([contig], [[(0, 5, 0, show(0, 0))], [(0, 5, 1, show(1, 1))], [(0, 5, 0, show(0, 1))]])
    obs = HR.observe(seqs, places, off, sites)
    assert obs["frag_obs_off"].tolist() == [0, 2, 4, 6] and obs["obs_site"].tolist() == [0, 1] * 3 and obs["obs_allele"].tolist() == [0, 0, 1, 1, 0, 1]
    assert (obs["link_lo"].tolist(), obs["link_hi"].tolist(), obs["link_rel"].tolist()) == ([0, 0, 0], [1, 1, 1], [0, 0, 1])
    assert obs["stats"].tolist() == [6, 6, 0, 0, 6, 3]
    edges = HR.bundle(2, obs)
    assert (edges["edge_lo"].tolist(), edges["edge_hi"].tolist(), edges["edge_cis"].tolist(), edges["edge_trans"].tolist()) == ([0], [1], [2], [1])
    assert edges["edge_off"].tolist() == [0, 0, 1] and edges["n_edges"] == 1
    s = HR.solve(sites["var_unitig"], edges, 2, 600)                 # 2000 >= 1800
    assert s["site_phase"].tolist() == [0, 0] and s["site_block"].tolist() == [0, 0] and s["site_parent"].tolist() == [HR.NO_SITE, 0]
    assert s["edge_state"].tolist() == [1] and s["counts"].tolist() == [1, 2, 1, 1, 0, 0]
    for reads, permille in ((2, 800), (4, 600)):                     # 2000 < 2400; 3 < 4
        s = HR.solve(sites["var_unitig"], edges, reads, permille)
        assert s["site_phase"].tolist() == [NONE, NONE] and s["site_block"].tolist() == [0, 1] and s["edge_state"].tolist() == [0]
        assert s["counts"].tolist() == [0] * 6


def test_thresholds_are_exact():
    assert _solve(2, [(0, 1, 3, 3)], 0, 0)[1]["site_phase"].tolist() == [NONE, NONE]           # cis == trans: undecided whatever the threshold
    assert _solve(2, [(0, 1, 999, 1)], 1, 1000)[1]["site_phase"].tolist() == [NONE, NONE]      # one dissenting read at 1000 permille
    assert _solve(2, [(0, 1, 999, 0)], 1, 1000)[1]["site_phase"].tolist() == [0, 0]
    assert _solve(2, [(0, 1, 999, 0)], 1, 1001)[1]["site_phase"].tolist() == [NONE, NONE]      # above 1000 nothing is decided
    assert _solve(2, [(0, 1, 1, 0)], 0, 0)[1]["site_phase"].tolist() == [0, 0]                 # min_link_reads 0 counts as 1
    assert _solve(2, [(0, 1, 4, 1)], 2, 800)[1]["site_phase"].tolist() == [0, 0]               # 4000 >= 4000
    assert _solve(2, [(0, 1, 4, 1)], 2, 801)[1]["site_phase"].tolist() == [NONE, NONE]
    assert not HR.decided(1 << 31, 1 << 31, 0, 0) and HR.decided((1 << 32) - 1, 0, (1 << 32) - 1, 1000)


def test_a_trans_edge_a_triangle_and_an_edge_across_blocks():
    assert _solve(2, [(0, 1, 0, 5)])[1]["site_phase"].tolist() == [0, 1]
    edges, s = _solve(3, [(0, 1, 5, 0), (1, 2, 5, 0), (0, 2, 0, 3)])
    assert edges["edge_lo"].tolist() == [0, 0, 1] and edges["edge_hi"].tolist() == [1, 2, 2] and edges["edge_off"].tolist() == [0, 0, 1, 3]
    assert s["site_phase"].tolist() == [0, 0, 0] and s["site_block"].tolist() == [0, 0, 0] and s["site_parent"].tolist() == [HR.NO_SITE, 0, 1]
    assert s["edge_state"].tolist() == [1, 2, 1] and s["counts"].tolist() == [1, 3, 3, 2, 1, 0]
    edges, s = _solve(3, [(0, 2, 5, 0), (1, 2, 0, 3)])
    assert s["site_block"].tolist() == [0, 1, 0] and s["site_phase"].tolist() == [0, NONE, 0] and s["edge_state"].tolist() == [1, 3]
    assert s["counts"].tolist() == [1, 2, 2, 1, 0, 1]
    # signs add up along the way to the root: 0 -t- 1 -c- 2 -t- 3
    assert _solve(4, [(0, 1, 0, 4), (1, 2, 4, 0), (2, 3, 0, 4)])[1]["site_phase"].tolist() == [0, 1, 1, 0]


def test_each_parent_tie_break():
    assert _solve(3, [(0, 2, 6, 0), (1, 2, 5, 0)])[1]["site_parent"].tolist()[2] == 0          # the larger n
    assert _solve(3, [(0, 2, 5, 0), (1, 2, 4, 1)])[1]["site_parent"].tolist()[2] == 0          # n equal: the larger m
    assert _solve(3, [(0, 2, 5, 0), (1, 2, 5, 0)])[1]["site_parent"].tolist()[2] == 1          # n and m equal: the larger lo
    assert _solve(3, [(0, 2, 9, 9), (1, 2, 2, 0)])[1]["site_parent"].tolist()[2] == 1          # an undecided edge is no candidate


def test_observe_literals():
    a, b = "ACGTTGCAAC" * 4, "TTGACCATGA" * 3                       # contigs of 40 and 30 bases
    sites = {k: np.concatenate((x, y)) for (k, x), y in zip(HC.sites_dict([(5, "G", "T"), (14, "T", "A"), (24, "T", "C")]).items(),
                                                            HC.sites_dict([(0, "T", "G"), (29, "A", "C")], 1).values())}
    sub = lambda text, at, c: text[:at] + c + text[at + 1:]
    reads = [
        [(0, 5, 0, a[5:15])],                                       # 0: sites 0 and 1 at the first and the last base of a placement, forwards
        [(0, 5, 1, sub(sub(a[5:15], 0, "T"), 9, "A"))],             # 1: the same span backwards, both alternative: its mate disagrees twice
        [(0, 0, 0, a[:20])],                                        # 2: sites 0 and 1
        [(0, 10, 1, a[10:30])],                                     # 3: sites 1 and 2: its mate agrees at site 1
        [(0, 0, 0, a[:20]), (0, 10, 0, sub(a[10:30], 4, "A"))],     # 4: two placements of one read disagree at site 1: the link is (0, 2)
        [],                                                         # 5: an empty mate
        [(0, 5, 0, sub(sub(a[5:25], 0, "g"), 9, "N")), (0, 24, 0, sub(a[24:30], 0, "A"))],      # 6: lower case, N, and a third base beside a T
        [(0, 20, 0, a[20:]), (1, 0, 0, b[:10])],                    # 7: sites 2 and 3 lie on two contigs: no link
        [(1, 0, 1, sub(b, 29, "C"))],                               # 8: the first and the last base of the last contig, backwards
        [(0, 16, 0, a[16:22])],                                     # 9: a placement without a site
    ]
    seqs, places, off = _lay([a, b], reads)
    rows = lambda o: [list(zip(o["obs_site"].tolist()[i:j], o["obs_allele"].tolist()[i:j])) for i, j in zip(o["frag_obs_off"].tolist(), o["frag_obs_off"].tolist()[1:])]
    links = lambda o: list(zip(o["link_lo"].tolist(), o["link_hi"].tolist(), o["link_rel"].tolist()))
    obs = HR.observe(seqs, places, off, sites)
    assert rows(obs) == [[(0, 0), (1, 0)], [(0, 1), (1, 1)], [(0, 0), (1, 0)], [(1, 0), (2, 0)], [(0, 0), (2, 0)], [], [], [(2, 0), (3, 0)], [(3, 0), (4, 1)], []]
    assert links(obs) == [(0, 1, 0), (0, 1, 0), (0, 1, 0), (1, 2, 0), (0, 2, 0), (3, 4, 1)]
    assert obs["stats"].tolist() == [20, 18, 3, 1, 14, 6]
    # fragments of two: (0, 1) is discordant at both sites; (2, 3) sees site 1 twice, concordant; (6, 7) keeps site 3 alone: the third base
    # at site 2 drops what mate 7 shows there
    paired = HR.observe(seqs, places, off, sites, 2)
    assert rows(paired) == [[], [(0, 0), (1, 0), (2, 0)], [(0, 0), (2, 0)], [(3, 0)], [(3, 0), (4, 1)]]
    assert links(paired) == [(0, 1, 0), (1, 2, 0), (0, 2, 0), (3, 4, 1)]
    assert paired["stats"].tolist() == [20, 14, 3, 3, 8, 4]


def test_tag_a_fragment_over_two_blocks():
    solved = {"site_block": np.array([0, 0, 2, 3, 3], np.uint32), "site_phase": np.array([0, 1, NONE, 0, 1], np.uint8)}
    obs = {"frag_obs_off": np.array([0, 5, 5, 6, 8], np.uint64), "obs_site": np.array([0, 1, 2, 3, 4, 2, 4, 3], np.uint32),
           "obs_allele": np.array([1, 0, 1, 0, 0, 0, 1, 0], np.uint8)}
    t = HR.tag(obs, solved)
    assert t["tag_block"].tolist() == [0, HR.NO_SITE, HR.NO_SITE, 3]
    assert (t["tag_h0"].tolist(), t["tag_h1"].tolist(), t["tag_other"].tolist()) == ([0, 0, 0, 2], [2, 0, 0, 0], [2, 0, 0, 0])


def test_every_refusal():
    a = "ACGTTGCAAC" * 4
    sites = HC.sites_dict([(5, "G", "T"), (14, "T", "A")])
    seqs, places, off = _lay([a], [[(0, 0, 0, a[:20])], [(0, 10, 1, a[10:30])]])
    assert HR.observe(seqs, places, off, sites)["stats"][0] == 3
    over = lambda d, k, j, v: dict(d, **{k: np.concatenate((d[k][:j], [v], d[k][j + 1:])).astype(d[k].dtype)})
    for bad_sites in (over(sites, "var_unitig", 1, 1), over(sites, "var_pos", 1, 40), over(sites, "var_pos", 1, 5), over(sites, "var_pos", 1, 4),
                      over(sites, "var_ref", 0, ord("g")), over(sites, "var_alt", 0, ord("N")), over(sites, "var_alt", 0, ord("G"))):
        with pytest.raises(ValueError):
            HR.observe(seqs, places, off, bad_sites)
    for bad_places in (over(places, "seq_place_off", 1, 3), over(places, "place_unitig", 0, 1), over(places, "place_pos", 1, 21), over(places, "place_q0", 0, 1),
                       over(places, "place_len", 0, 0)):
        with pytest.raises(ValueError):
            HR.observe(seqs, bad_places, off, sites)
    for group in (0, 3):
        with pytest.raises(ValueError):
            HR.observe(seqs, places, off, sites, group)
    with pytest.raises(ValueError):
        HR.observe(seqs + [b""], dict(places, seq_place_off=np.array([0, 1, 2, 2], np.uint64)), off, sites, 2)
    with pytest.raises(ValueError):
        HR.observe(seqs, places, np.array([0, 22], np.uint64), sites)
    for row in ((1, 1, 1, 0), (1, 0, 1, 0), (0, 2, 1, 0)):
        with pytest.raises(ValueError):
            HR.bundle(2, _links([row]))
    with pytest.raises(ValueError):
        HR.bundle(2, dict(_links([(0, 1, 1, 0)]), link_rel=np.array([2], np.uint8)))
    edges = HR.bundle(3, _links([(0, 2, 2, 0), (1, 2, 2, 0)]))
    unit = np.zeros(3, np.uint32)
    assert HR.solve(unit, edges)["site_block"].tolist() == [0, 1, 1]
    for bad_edges in (over(edges, "edge_off", 0, 1), over(edges, "edge_off", 3, 1), over(edges, "edge_off", 1, 1), over(edges, "edge_lo", 1, 2),
                      over(edges, "edge_lo", 1, 0), over(edges, "edge_lo", 0, 1)):
        with pytest.raises(ValueError):
            HR.solve(unit, bad_edges)
    for bad_unit in ([0, 1, 1], [1, 1, 0], [0, 1, 0]):
        with pytest.raises(ValueError):
            HR.solve(np.array(bad_unit, np.uint32), edges)
    solved = HR.solve(unit, edges)
    obs = {"frag_obs_off": np.array([0, 2], np.uint64), "obs_site": np.array([1, 2], np.uint32), "obs_allele": np.array([0, 1], np.uint8)}
    assert HR.tag(obs, solved)["tag_h1"].tolist() == [1]
    for bad_obs in (over(obs, "frag_obs_off", 0, 1), over(obs, "frag_obs_off", 1, 3), over(obs, "obs_site", 0, 3), over(obs, "obs_allele", 1, 2)):
        with pytest.raises(ValueError):
            HR.tag(bad_obs, solved)
    for bad_solved in (over(solved, "site_block", 1, 2), over(solved, "site_phase", 0, 2)):
        with pytest.raises(ValueError):
            HR.tag(obs, bad_solved)


@pytest.mark.parametrize("seed", FC.PLACEMENT_SEEDS[:3])
def test_a_batch_and_its_reverse_complement_observe_the_same(seed):
    case = FC.placements_case(seed)
    sites = HC.random_sites(case, 500 + seed, 400)
    got = HR.observe(case["seqs"], case["places"], case["offsets"], sites)
    twin = FC.rc_twin(case)
    want = HR.observe(twin["seqs"], twin["places"], twin["offsets"], sites)
    assert got["stats"][0] > 100 and got["stats"][2] > 10 and got["stats"][4] > 10
    for k in got:
        assert np.array_equal(got[k], want[k]), k


@pytest.fixture(scope="module")
def planted():
    p = HC.planted()
    G = PC.ref_graph(p["codes"], p["tfs"], 1, 3)
    assert [len(s) for s in G["strings"]] == [HC.GENOME]
    contig = G["strings"][0]
    want, _ = HC.expected_sites(p, contig)
    out = dict(p=p, G=G, truth=HC.truth(p, contig))
    for name, seqs, group in (("reads", p["reads"], 1), ("mates", p["mates"], 2)):
        _, places, piled = PC.chain(G, seqs)
        called = PR.call(G["g"]["offsets"], G["g"]["bases"], piled["counts"])
        assert [(int(x), chr(r), chr(a)) for x, r, a in zip(called["var_pos"], called["var_ref"], called["var_alt"])] == want, name
        out[name] = (called,) + HC.phase(seqs, places, G["g"]["offsets"], called, group)
    return out


def _blocks(solved):
    out = {}
    for v, (b, p) in enumerate(zip(solved["site_block"].tolist(), solved["site_phase"].tolist())):
        if p != NONE:
            out.setdefault(b, []).append(v)
    return out


def _gap_sides(called):
    """the indices of the first site behind the two stretches without one"""
    pos = called["var_pos"].tolist()
    wide = [v for v in range(1, len(pos)) if pos[v] - pos[v - 1] > 100]
    assert len(wide) == 2 and pos[wide[0]] - pos[wide[0] - 1] == HC.GAP_READ[1] and pos[wide[1]] - pos[wide[1] - 1] == HC.GAP_PAIR[1]
    return wide


def test_planted_genome_and_sites(planted):
    truth = planted["truth"]
    assert len(truth) == len(planted["p"]["sites"]) > 100 and 0 < sum(truth) < len(truth)          # the contig carries A's bases, then B's
    assert truth == sorted(truth) or truth == sorted(truth, reverse=True)


@pytest.mark.parametrize("name", ("reads", "mates"))
def test_planted_blocks_and_phases(planted, name):
    called, obs, edges, solved, tags = planted[name]
    truth, blocks = planted["truth"], _blocks(solved)
    a, b = _gap_sides(called)
    firsts = sorted(blocks)
    assert firsts == ([0, a, b] if name == "reads" else [0, b])       # the pairs close the stretch no read bridges
    assert sum(len(v) for v in blocks.values()) == len(truth) == solved["counts"][1] and solved["counts"][0] == len(firsts)
    flip = {}
    for first, members in blocks.items():
        flips = {(1 ^ int(solved["site_phase"][v])) ^ truth[v] for v in members}
        assert len(flips) == 1, first                               # the alternative base lies on haplotype 1 ^ p, up to the block's flip
        flip[first] = flips.pop()
    trans = [j for j in range(edges["n_edges"]) if solved["edge_state"][j] and edges["edge_trans"][j] > edges["edge_cis"][j]]
    assert trans and all(truth[edges["edge_lo"][j]] != truth[edges["edge_hi"][j]] for j in trans)  # where the coverage switches
    assert solved["counts"][4] == 0 and solved["counts"][2] == solved["counts"][3] + solved["counts"][5]
    p = planted["p"]
    haps = p["read_hap"] if name == "reads" else p["pair_hap"]
    clean = p["read_clean"] if name == "reads" else [True] * len(haps)
    tagged = 0
    for f, (blk, h0, h1, other) in enumerate(zip(*(tags[k].tolist() for k in HR.TAG_KEYS))):
        if blk == HR.NO_SITE or not clean[f]:
            continue
        # B's base at a site is allele `truth`, so B lies on haplotype truth ^ p = 1 ^ flip, and A on haplotype flip
        mine = haps[f] ^ flip[blk]
        assert (h0, h1)[mine] > 0 and (h0, h1)[1 - mine] == 0, f
        tagged += 1
    assert tagged > len(haps) * 0.8
