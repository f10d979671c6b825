"""The gap-closing fuzz without a GPU: the inputs of tests/gap_close_fuzz_cases.py through the restatement (tests/gap_close_ref.py) and
through a second opinion written from the contract alone (tests/gap_close_walks.py). The two searches agree on every input; the
property checks accept the restatement's outputs and refuse single-word corruptions of them; the inputs reach the situations the GPU
test (test_gpu_gap_close_fuzz.py) relies on, asserted here from the restatement so that an edit of the generator cannot hollow it out;
and every near miss of the rule (gap_close_walks.MUTANTS) gives another answer than the rule on at least one of the inputs."""
import numpy as np
import pytest

import gap_close_fuzz_cases as FC
import gap_close_ref as GF
import gap_close_walks as W
import scaffold_ref as SF

NONE32 = SF.NONE32
GRAPH = ("offsets", "link_off", "link_to", "join", "join_gap")
CLOSE = ("close_status", "close_dist", "close_states", "path_off", "path", "fill_uses", "counts")


def _search(g, fn=GF.search, **kw):
    return fn(*[g[k] for k in GRAPH], **kw)


def _equal(a, b):
    return a["total"] == b["total"] and all(a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]) for k in CLOSE)


def _members(g):
    if "bases" not in g:
        return FC.members(g)
    lay = SF.layout(g["offsets"], g["join"], g["join_count"], g["join_gap"])
    return dict(SF.emit(g["offsets"], g["bases"], g["join"], g["join_gap"], lay), n_cut=lay["n_cut"])


def _fill(g, em, cl):
    lay = GF.fill_layout(*[g[k] for k in GRAPH], em["member_off"], em["member"], cl)
    return dict(lay, fscaffold_bases=GF.fill_emit(g["offsets"], g["bases"], lay)) if "bases" in g else lay


@pytest.fixture(scope="module")
def runs():
    """every input once: (name, graph, params, members, the restatement's closure and fill), shared and left unchanged"""
    out = []
    for seed in FC.SEEDS:
        g = FC.tangled(seed)
        em = _members(g)
        for i, p in enumerate(FC.PARAM_SETS):
            cl = _search(g, **p)
            out.append((("tangled", seed, i), g, p, em, cl, _fill(g, em, cl)))
    for name, g, p in (("corridor", FC.corridor(), FC.CORRIDOR_PARAMS), ("giant", FC.giant(), FC.GIANT_PARAMS)):
        em = _members(g)
        cl = _search(g, **p)
        out.append(((name,), g, p, em, cl, _fill(g, em, cl)))
    return out


def _edge_inputs():
    """the small graph at the budgets where a search turns from complete to exhausted, and at the edges of max_fill and tolerance"""
    g = FC.tangled(*FC.SMALL)
    ns, sets = FC.edge_param_sets(_search(g, **FC.FULL))
    return g, ns, sets


def test_the_two_searches_agree(runs):
    for name, g, p, em, cl, f in runs:
        assert _equal(cl, _search(g, W.search_dfs, **p)), name
    g, ns, sets = _edge_inputs()
    assert len(ns) >= 10 and min(ns) <= 2 and max(ns) > 256 and min(abs(n - 64) for n in ns) <= 1 and min(abs(n - 128) for n in ns) <= 9
    for p in sets:
        assert _equal(_search(g, **p), _search(g, W.search_dfs, **p)), p


def test_the_property_checks_accept_the_restatement(runs):
    for name, g, p, em, cl, f in runs:
        W.check_closure(g, p, cl)
        W.check_fill(g, em, cl, f)


def _poked(d, k, i, v):
    a = d[k].copy()
    a[i] = v
    return dict(d, **{k: a})


def test_the_property_checks_refuse_corruptions(runs):
    """one word of a correct output changed: every one is seen"""
    for name, g, p, em, cl, f in runs:
        if name[0] == "tangled" and name[2] != 0:
            continue
        jn = g["join"].tolist()
        owners = [e for e, t in enumerate(jn) if t != NONE32 and e < t ^ 1]
        closed = [e for e in owners if cl["close_status"][e] == 1]
        with_path = [e for e in closed if cl["path_off"][e + 1] > cl["path_off"][e]]
        free = jn.index(NONE32)
        e, q = closed[0], int(cl["path_off"][with_path[0]])
        t = jn[e]
        bad = [_poked(cl, "close_dist", e, int(cl["close_dist"][e]) + 1), _poked(cl, "close_dist", t ^ 1, int(cl["close_dist"][e]) - 1), _poked(cl, "close_status", e, 2),
               _poked(cl, "close_status", t ^ 1, 3), _poked(cl, "close_status", free, 2), _poked(cl, "close_states", e, int(cl["close_states"][e]) + 1),
               _poked(cl, "path", q, int(cl["path"][q]) ^ 1), _poked(cl, "fill_uses", int(cl["path"][q]) >> 1, 0), _poked(cl, "counts", 0, int(cl["counts"][0]) + 1),
               _poked(cl, "counts", 4, int(cl["counts"][4]) - 1), _poked(cl, "path_off", with_path[0] + 1, q)]
        for i, c in enumerate(bad):
            with pytest.raises(W.Violation):
                W.check_closure(g, p, c)
                pytest.fail("closure corruption %d of %s went unseen" % (i, name))
        j3, j1 = int(np.nonzero(f["fmember_flag"] == 3)[0][0]), int(np.nonzero(f["fmember_flag"] == 1)[0][0])
        open_ = np.nonzero((f["fmember_flag"] == 0) & (f["fmember_gap"] != 0))[0].tolist()
        bad = [_poked(f, "fmember_pos", j3, int(f["fmember_pos"][j3]) + 1), _poked(f, "fmember_flag", j3, 1), _poked(f, "fmember_flag", j1, 0),
               _poked(f, "fmember", j3, int(f["fmember"][j3]) ^ 1), _poked(f, "fmember_gap", j1, int(f["fmember_gap"][j1]) + 1),
               _poked(f, "fscaffold_offsets", 1, int(f["fscaffold_offsets"][1]) + 1),
               _poked(f, "fmember_off", 1, int(f["fmember_off"][1]) + 1), dict(f, total_bases=f["total_bases"] + 1), dict(f, n_fmembers=f["n_fmembers"] - 1)]
        bad += [_poked(f, "fmember_gap", j0, int(f["fmember_gap"][j0]) - 1) for j0 in open_[:1]]
        if "bases" in g:
            x = int(f["fscaffold_offsets"][-1]) // 2
            bad += [_poked(f, "fscaffold_bases", x, int(f["fscaffold_bases"][x]) ^ 0x04), _poked(f, "fscaffold_bases", 0, ord("N"))]
        for i, c in enumerate(bad):
            with pytest.raises(W.Violation):
                W.check_fill(g, em, cl, c)
                pytest.fail("fill corruption %d of %s went unseen" % (i, name))


def test_the_inputs_reach_what_the_gpu_test_relies_on(runs):
    seen = dict.fromkeys(("status1", "status2", "status3", "status4", "closed_beyond_64_states", "tiny_after_exhausted_4096", "fill_uses_above_1",
                          "contig_in_two_filled_scaffolds", "cut_cycle", "non_owner_traversal", "closed_join_cut_from_a_cycle", "duplicate_link", "link_into_source_contig",
                          "link_into_joined_contig", "link_into_dual_of_target", "self_loop_off_the_path", "contig_of_23", "contig_of_24", "circular_contig"), 0)
    for name, g, p, em, cl, f in runs:
        if name[0] != "tangled":
            continue
        U, jn = g["U"], g["join"].tolist()
        lo, to = g["link_off"].tolist(), g["link_to"].tolist()
        st, ns, po = cl["close_status"].tolist(), cl["close_states"].tolist(), cl["path_off"].tolist()
        owners = [e for e, t in enumerate(jn) if t != NONE32 and e < t ^ 1]
        for k in range(4):
            seen["status%d" % (k + 1)] += int(cl["counts"][k])
        seen["closed_beyond_64_states"] += sum(st[e] == 1 and ns[e] > 64 for e in owners)
        if p["max_states"] == 4096:                                       # one workgroup takes the joins in this order
            seen["tiny_after_exhausted_4096"] += sum(st[a] == 4 and ns[b] <= 2 for a, b in zip(owners, owners[1:]))
        seen["fill_uses_above_1"] += int((cl["fill_uses"] > 1).sum())
        fo, fm, ff = f["fmember_off"].tolist(), f["fmember"].tolist(), f["fmember_flag"].tolist()
        where = {}
        for s in range(len(fo) - 1):
            for j in range(fo[s], fo[s + 1]):
                if ff[j] == 3:
                    where.setdefault(fm[j] >> 1, set()).add(s)
        seen["contig_in_two_filled_scaffolds"] += sum(len(v) > 1 for v in where.values())
        seen["cut_cycle"] += em["n_cut"]
        mo, mem = em["member_off"].tolist(), em["member"].tolist()
        first = set(mo[:-1])
        adjacent = {(mem[i - 1], mem[i]) for i in range(1, U) if i not in first}
        seen["non_owner_traversal"] += sum(st[a] == 1 and a > b ^ 1 and po[(b ^ 1) + 1] > po[b ^ 1] for a, b in adjacent)
        seen["closed_join_cut_from_a_cycle"] += sum(st[e] == 1 and (e, jn[e]) not in adjacent and (jn[e] ^ 1, e ^ 1) not in adjacent for e in owners)
        kept = []
        _search(g, W.search_dfs, kept=kept, **p)
        for e, w, d, k in kept:                                           # what the searches themselves met behind a stored intermediate
            if w == jn[e]:
                continue
            mine = to[lo[w]:lo[w + 1]]
            seen["link_into_source_contig"] += any(y >> 1 == e >> 1 for y in mine)
            seen["link_into_joined_contig"] += any(y != jn[e] and jn[y] != NONE32 for y in mine)
            seen["link_into_dual_of_target"] += (jn[e] ^ 1) in mine
            seen["duplicate_link"] += len(set(mine)) < len(mine)
            seen["self_loop_off_the_path"] += w in mine and st[e] == 1 and w not in cl["path"][po[e]:po[e + 1]].tolist()
        lens = np.diff(g["offsets"].astype(np.int64))
        seen["contig_of_23"] += int((lens == 23).sum())
        seen["contig_of_24"] += int((lens == 24).sum())
        seen["circular_contig"] += int(g["circular"].sum())
    assert all(seen.values()), {k: v for k, v in seen.items() if not v}
    name, g, p, em, cl, f = next(r for r in runs if r[0] == ("corridor",))
    k, m = 8, len(g["corridor"])                                          # k joins through m contigs: k m path entries, more than the 2 k + m contigs
    assert cl["total"] == k * m > g["U"] and cl["counts"].tolist() == [k, 0, 0, 0, k] and all(cl["fill_uses"][u] == k for u in g["corridor"]) and cl["fill_uses"].sum() == k * m
    fo, fm = f["fmember_off"].tolist(), f["fmember"].tolist()
    multi = [s for s in range(len(fo) - 1) if em["member_off"][s + 1] - em["member_off"][s] > 1]
    assert len(multi) == k and all({w >> 1 for w in fm[fo[s]:fo[s + 1]]} >= set(g["corridor"]) for s in multi)


@pytest.mark.parametrize("mutant", W.MUTANTS)
def test_every_near_miss_is_told_from_the_rule(runs, mutant):
    inputs = [(g, p, cl) for name, g, p, em, cl, f in runs]
    g, ns, sets = _edge_inputs()
    inputs += [(g, p, None) for p in sets]
    killed = 0
    for g, p, cl in inputs:
        cl = _search(g, **p) if cl is None else cl
        killed += not _equal(cl, _search(g, W.search_dfs, mutant=mutant, **p))
    assert killed > 0, mutant


def test_giant_lengths():
    """the hit lies exactly at gap + tolerance, one base of tolerance fewer loses it; nothing stored lies beyond 2^30 + 2^20; the oversized
    contigs are dropped, not wrapped; the filled positions pass 2^32"""
    g, p = FC.giant(), FC.GIANT_PARAMS
    kept = []
    cl = _search(g, W.search_dfs, kept=kept, **p)
    assert _equal(cl, _search(g, **p))
    A, B, P, Q, Cc = 1, 2, 3, 4, 7
    assert cl["close_status"].tolist()[2 * A] == 1 and cl["close_dist"][2 * A] == (1 << 30) + (1 << 20) == int(g["join_gap"][2 * A]) + p["tolerance"]
    assert cl["path"].tolist() == [2 * P, 2 * Q + 1] and cl["close_states"][2 * A] == 3 and cl["counts"].tolist() == [1, 2, 0, 0, 3]
    assert cl["close_status"][2 * Cc] == 2 and cl["close_states"][2 * Cc] == 0 and cl["close_status"][0] == 2
    assert kept and max(d for e, w, d, k in kept) == (1 << 30) + (1 << 20) and all(-22 <= d for e, w, d, k in kept)
    less = _search(g, **dict(p, tolerance=p["tolerance"] - 1))
    assert less["close_status"][2 * A] == 2 and less["close_states"][2 * A] == 1 and _equal(less, _search(g, W.search_dfs, **dict(p, tolerance=p["tolerance"] - 1)))
    em = FC.members(g)
    assert em["member"].tolist()[:3] == [0, 2 * A, 2 * B]
    f = GF.fill_layout(*[g[k] for k in GRAPH], em["member_off"], em["member"], cl)
    assert f["fmember"].tolist()[:5] == [0, 2 * A, 2 * P, 2 * Q + 1, 2 * B] and f["fmember_flag"].tolist()[:5] == [0, 0, 3, 3, 1]
    assert f["fmember_pos"][1] == (1 << 33) + 14 and min(f["fmember_pos"].tolist()[1:5]) > 1 << 32
    assert f["fmember_pos"][4] == (1 << 33) + 14 + 100 + (1 << 30) + (1 << 20) + 22 and f["fscaffold_offsets"][-1] > 1 << 40
    W.check_fill(g, em, cl, f)
