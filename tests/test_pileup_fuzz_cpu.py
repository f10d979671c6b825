"""The pile-up fuzz without a GPU: the inputs of tests/pileup_fuzz_cases.py through the restatement (tests/pileup_ref.py) and through a
second opinion written from the contract alone on whole arrays (tests/pileup_second.py). The two agree on every input and parameter
set; the inputs reach the situations the GPU test (test_gpu_pileup_fuzz.py) relies on, asserted here by name from the restatement's
outputs so that an edit of a generator cannot hollow it out; every near miss of the rule (pileup_second.MUTANTS) gives another answer
than the rule on at least one input; and an array-level pile input and its reverse complement give equal counts, place_mism and stats."""
import itertools

import numpy as np
import pytest

import pileup_fuzz_cases as FC
import pileup_ref as PR
import pileup_second as PS

M32 = FC.M32
CALL_KEYS = PR.VAR_KEYS + ("polished", "depth_sum", "uncovered")
SIDES, WHICH = ("left", "right"), ("extend", "read", "contig", "neighbour")


def _same(a, b, keys, scalars=()):
    return all(a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]) for k in keys) and all(a[k] == b[k] for k in scalars)


def same_place(a, b):
    return _same(a, b, PR.PLACE_KEYS, ("n_place", "n_circular_steps"))


def same_pile(a, b):
    return _same(a, b, ("counts", "place_mism", "stats"))


def same_call(a, b):
    return _same(a, b, CALL_KEYS, ("n_changed", "total"))


@pytest.fixture(scope="module")
def step_runs():
    """every steps case under every parameter set through the restatement, once: {(seed, i): (case, places, piled)}, left unchanged"""
    out = {}
    for seed in FC.SEEDS:
        c = FC.steps_case(seed)
        for i, (max_gap, extend) in enumerate(FC.PLACE_PARAMS):
            places = PR.place(c["offs"], c["steps"], c["offsets"], max_gap, extend)
            out[seed, i] = (c, places, PR.pile(c["seqs"], places, c["offsets"], c["bases"]))
    return out


@pytest.fixture(scope="module")
def place_runs():
    """every placements case piled onto its prefilled counts and onto zero by the restatement: {seed: (case, piled, from zero)}"""
    out = {}
    for seed in FC.PLACEMENT_SEEDS:
        c = FC.placements_case(seed)
        out[seed] = (c, PR.pile(c["seqs"], c["places"], c["offsets"], c["bases"], c["counts"]), PR.pile(c["seqs"], c["places"], c["offsets"], c["bases"]))
    return out


@pytest.fixture(scope="module")
def cell_runs():
    c = FC.cells_case()
    return c, [PR.call(c["offsets"], c["bases"], c["counts"], **th) for th in FC.CALL_PARAMS]


def test_place_the_two_agree(step_runs):
    for (seed, i), (c, places, piled) in step_runs.items():
        assert same_place(places, PS.place(c["offs"], c["steps"], c["offsets"], *FC.PLACE_PARAMS[i])), (seed, i)
    empty = {k: np.zeros(0, dt) for k, dt in zip(FC._STEP_KEYS, FC._STEP_DTYPES)}
    for offs in ([0], [0, 0, 30]):                                   # M = 0, and T = 0
        steps = dict(empty, seq_step_off=np.zeros(len(offs), np.uint64))
        assert same_place(PR.place(np.array(offs, np.uint64), steps, [0, 23]), PS.place(np.array(offs, np.uint64), steps, [0, 23]))


def test_pile_the_two_agree(step_runs, place_runs):
    for (seed, i), (c, places, piled) in step_runs.items():
        assert same_pile(piled, PS.pile(c["seqs"], places, c["offsets"], c["bases"])), (seed, i)
    for seed, (c, piled, zero) in place_runs.items():
        args = (c["seqs"], c["places"], c["offsets"], c["bases"])
        assert same_pile(piled, PS.pile(*args, c["counts"])) and same_pile(zero, PS.pile(*args)), seed
        assert same_pile(PR.pile(*args, piled["counts"]), PS.pile(*args, piled["counts"])), (seed, "twice")


def test_call_the_two_agree(step_runs, cell_runs):
    c, wants = cell_runs
    for th, want in zip(FC.CALL_PARAMS, wants):
        assert same_call(want, PS.call(c["offsets"], c["bases"], c["counts"], **th)), th
    for (seed, i), (c, places, piled) in step_runs.items():
        if i in (0, 3):
            for th in ({}, FC.LOOSE):
                assert same_call(PR.call(c["offsets"], c["bases"], piled["counts"], **th), PS.call(c["offsets"], c["bases"], piled["counts"], **th)), (seed, i)
    assert same_call(PR.call([0], [], []), PS.call([0], [], []))      # U = 0


def _placements_in_steps(c, places, extend):
    """Per placement of the restatement: its steps, its core, the four limits of each side recomputed from the step arrays, and what the
    restatement grew. -> dicts with r, seq, t0, e (first and last step), u, s, d, limits {side: {name: value}}, grown {side: bases},
    across {side: the adjacent step at that side is circular}."""
    st = c["steps"]
    sso, so, off = st["seq_step_off"].tolist(), c["offs"].tolist(), c["offsets"].tolist()
    su, sp, sf, qf, ql = (st[k].tolist() for k in FC._STEP_KEYS)
    spo, q0, ln, ns = (places[k].tolist() for k in ("seq_place_off", "place_q0", "place_len", "place_steps"))
    out = []
    for i in range(len(so) - 1):
        linear = [t for t in range(sso[i], sso[i + 1]) if not sf[t] & 2]
        L, at, prev_last = so[i + 1] - so[i], 0, None
        for r in range(spo[i], spo[i + 1]):
            t0, e = linear[at], linear[at + ns[r] - 1]
            assert e - t0 == ns[r] - 1                                # the steps of a placement are adjacent
            at += ns[r]
            u, s, a, last = su[t0], sf[t0] & 1, qf[t0], ql[e] + 22
            d = sp[t0] + a + 22 if s else sp[t0] - a
            Lu = off[u + 1] - off[u]
            nxt = qf[linear[at]] if at < len(linear) else None
            limits = {"left": {"extend": extend, "read": a, "contig": Lu - 1 - (d - a) if s else d + a},
                      "right": {"extend": extend, "read": L - 1 - last, "contig": d - last if s else Lu - 1 - (d + last)}}
            if prev_last is not None:
                limits["left"]["neighbour"] = a - prev_last - 1
            if nxt is not None:
                limits["right"]["neighbour"] = nxt - last - 1
            out.append(dict(r=r, seq=i, t0=t0, e=e, u=u, s=s, d=d, limits=limits, grown={"left": a - q0[r], "right": q0[r] + ln[r] - 1 - last},
                            across={"left": t0 > sso[i] and bool(sf[t0 - 1] & 2), "right": e + 1 < sso[i + 1] and bool(sf[e + 1] & 2)}))
            prev_last = last
    return out


def test_the_inputs_reach_what_the_gpu_test_relies_on(step_runs, place_runs, cell_runs):
    finite = [g for g, _ in FC.PLACE_PARAMS if g < M32]
    names = ["gap_of_max_gap_%d_merges" % g for g in finite] + ["gap_of_max_gap_%d_plus_1_parts" % g for g in finite]
    names += ["run_of_three_or_more", "same_u_d_opposite_s_parts", "same_u_s_d_differs_by_1_parts", "negative_d", "circular_between_two_that_would_merge",
              "circular_first_and_last", "sequence_of_circular_only", "stepless_sequence_between_placed_ones", "neighbour_across_circular_left",
              "neighbour_across_circular_right", "cores_overlap_neighbour_limit_negative", "base_0_of_contig_0", "last_base_of_last_contig",
              "contig_of_23", "flag_bits_2_to_7", "placements_under_every_param_set_differ"]
    names += ["bound_%s_%s_%s" % (side, "bw" if s else "fw", w) for side, s, w in itertools.product(SIDES, (0, 1), WHICH)]
    seen = dict.fromkeys(names, 0)
    assert sum(k.startswith("bound_") for k in seen) == 16
    for (seed, i), (c, places, piled) in step_runs.items():
        max_gap, extend = FC.PLACE_PARAMS[i]
        st = c["steps"]
        sso = st["seq_step_off"].tolist()
        su, sp, sf, qf, ql = (st[k].tolist() for k in FC._STEP_KEYS)
        rows = _placements_in_steps(c, places, extend)
        of_step = {}
        for p in rows:
            of_step.update({t: p["r"] for t in range(p["t0"], p["e"] + 1)})
        diag = lambda t: (su[t], sf[t] & 1, sp[t] + qf[t] + 22 if sf[t] & 1 else sp[t] - qf[t])
        for j in range(len(sso) - 1):
            ts = list(range(sso[j], sso[j + 1]))
            lin = [t for t in ts if not sf[t] & 2]
            seen["circular_first_and_last"] += bool(lin) and len(ts) >= 3 and bool(sf[ts[0]] & 2) and bool(sf[ts[-1]] & 2)
            seen["sequence_of_circular_only"] += bool(ts) and not lin
            for x, y in zip(lin, lin[1:]):                            # consecutive linear steps
                gap, (u0, s0, d0), (u1, s1, d1) = qf[y] - ql[x] - 1, diag(x), diag(y)
                together = of_step[x] == of_step[y]
                if y == x + 1 and (u0, s0, d0) == (u1, s1, d1) and max_gap < M32:
                    seen["gap_of_max_gap_%d_merges" % max_gap] += gap == max_gap and together
                    seen["gap_of_max_gap_%d_plus_1_parts" % max_gap] += gap == max_gap + 1 and not together
                if y == x + 1 and gap <= max_gap:
                    seen["same_u_d_opposite_s_parts"] += (u0, d0) == (u1, d1) and s0 != s1 and not together
                    seen["same_u_s_d_differs_by_1_parts"] += (u0, s0) == (u1, s1) and abs(d0 - d1) == 1 and not together
                seen["circular_between_two_that_would_merge"] += y > x + 1 and (u0, s0, d0) == (u1, s1, d1) and gap <= max_gap and not together
        spo = places["seq_place_off"].tolist()
        R = places["n_place"]
        seen["stepless_sequence_between_placed_ones"] += sum(sso[j] == sso[j + 1] and 0 < spo[j] == spo[j + 1] < R for j in range(len(sso) - 1))
        seen["run_of_three_or_more"] += int((places["place_steps"] >= 3).sum())
        for p in rows:
            seen["negative_d"] += p["d"] < 0
            for side in SIDES:
                lim, grown = p["limits"][side], p["grown"][side]
                assert grown == max(0, min(lim.values()))             # (what the limits are for)
                low = min(lim, key=lim.get)
                if sum(v == lim[low] for v in lim.values()) == 1 and lim[low] >= 1:          # the strict minimum, and it lets the core grow
                    seen["bound_%s_%s_%s" % (side, "bw" if p["s"] else "fw", low)] += 1
                    if low == "neighbour" and p["across"][side]:
                        seen["neighbour_across_circular_" + side] += 1
                seen["cores_overlap_neighbour_limit_negative"] += lim.get("neighbour", 0) < 0 and grown == 0
        pu, pp, pl = (places[k] for k in ("place_unitig", "place_pos", "place_len"))
        lens = np.diff(c["offsets"].astype(np.int64))
        seen["base_0_of_contig_0"] += int(((pu == 0) & (pp == 0)).sum())
        seen["last_base_of_last_contig"] += int(((pu == c["U"] - 1) & (pp.astype(np.int64) + pl == lens[-1])).sum())
        seen["contig_of_23"] += int((lens == 23).sum())
        seen["flag_bits_2_to_7"] += int((st["step_flag"] >= 4).sum())
        seen["placements_under_every_param_set_differ"] += i > 0 and not same_place(places, step_runs[seed, i - 1][1])
        assert 2 <= c["U"] <= 40 and lens.min() >= 23 and lens.max() <= 600 and len(c["seqs"]) >= 200 and len(su) >= 600
        assert max(len(s) for s in c["seqs"]) <= 400 and min(len(s) for s in c["seqs"]) == 0 and int(pl.sum()) < 300_000
    assert all(seen.values()), sorted(k for k, v in seen.items() if not v)
    assert {step_runs[seed, 0][0]["U"] for seed in FC.SEEDS} >= {2, 40}

    seen = dict.fromkeys(["every_byte_value_placed", "run_of_200_placements_of_at_most_3", "3000_on_one_base_half_mismatch", "overlap_in_read_and_on_contig",
                          "one_span_forwards_and_backwards", "empty_sequences", "trailing_sequences_without_placement", "B_no_multiple_of_64", "cells_wrap",
                          "other_bytes", "base_0_and_last_base"] + ["length_%d" % n for n in FC.LENGTHS] + ["U_%d" % u for u in (1, 2, 40)], 0)
    for seed, (c, piled, zero) in place_runs.items():
        p = c["places"]
        spo = p["seq_place_off"].astype(np.int64)
        pu, pf, pp, q0, ln = (p[k].astype(np.int64) for k in FC._PLACE_KEYS)
        R, B = pu.shape[0], int(c["offsets"][-1])
        owner = np.repeat(np.arange(len(c["seqs"])), np.diff(spo))
        placed = set()
        for r in range(R):
            placed |= set(c["seqs"][owner[r]][q0[r]:q0[r] + ln[r]])
        seen["every_byte_value_placed"] += placed == set(range(256))
        for n in FC.LENGTHS:
            seen["length_%d" % n] += int((ln == n).sum())
        run = best = 0
        for n in ln.tolist():
            run = run + 1 if n <= 3 else 0
            best = max(best, run)
        seen["run_of_200_placements_of_at_most_3"] += best >= 200
        g0 = c["offsets"].astype(np.int64)[pu] + pp
        on_hot = (ln == 1) & (g0 == c["hot"])
        seen["3000_on_one_base_half_mismatch"] += on_hot.sum() >= 3000 and int(piled["place_mism"][on_hot].sum()) * 2 == int(on_hot.sum())
        twins = overlaps = 0
        for a, b in zip(range(R), range(1, R)):
            if owner[a] == owner[b] and pu[a] == pu[b]:
                both = q0[a] < q0[b] + ln[b] and q0[b] < q0[a] + ln[a] and pp[a] < pp[b] + ln[b] and pp[b] < pp[a] + ln[a]
                twin = (q0[a], ln[a], pp[a]) == (q0[b], ln[b], pp[b]) and (pf[a] ^ pf[b]) & 1
                twins += bool(twin) and ln[a] >= 23
                overlaps += bool(both and not twin) and ln[a] >= 23
        seen["one_span_forwards_and_backwards"] += twins > 0
        seen["overlap_in_read_and_on_contig"] += overlaps > 0
        lens = [len(s) for s in c["seqs"]]
        seen["empty_sequences"] += lens.count(0) >= 3 and lens[0] == 0
        seen["trailing_sequences_without_placement"] += spo[-4] == spo[-1] == R and lens[-2] > 0
        seen["B_no_multiple_of_64"] += B % 64 != 0
        seen["U_%d" % c["U"]] += 1
        wrapped = c["counts"].astype(np.uint64) + zero["counts"] > M32
        seen["cells_wrap"] += int(wrapped.sum()) >= 20 and bool(wrapped[4 * c["hot"]:4 * c["hot"] + 4].all()) and bool((piled["counts"][wrapped] < c["counts"][wrapped]).all())
        seen["other_bytes"] += int(piled["stats"][1]) > 100 and int(piled["stats"][2]) > 100
        seen["base_0_and_last_base"] += bool((g0 == 0).any() and (g0 + ln == B).any())
        assert int(ln.sum()) < 300_000 and (p["place_flag"] >= 2).any()
    n = len(FC.PLACEMENT_SEEDS)
    short = sorted(k for k, v in seen.items() if not v or (v != n and not k.startswith(("length_", "U_"))))
    assert not short, short                                           # what is planted in every case is found in every case

    c, wants = cell_runs
    by = dict(zip(("default", "loose", "zero", "depth", "p1000", "p1001", "alt31", "major31", "all"), wants))
    off, bases, cells = c["offsets"].astype(np.int64), c["bases"], c["counts"].reshape(-1, 4).astype(np.int64)
    B = 5000
    assert off[-1] == B == bases.shape[0] and {(int(b), tuple(x)) for b, x in zip(bases[:2500].tolist(), cells[:2500].tolist())} == set(
        itertools.product(b"ACGT", itertools.product(FC.PALETTE, repeat=4)))
    crossed = {int(((off[1:-1] > w) & (off[1:-1] < min(w + 64, B))).sum()) for w in range(0, B, 64)}
    assert crossed >= {0, 1, 2, 3} and 1000 in np.diff(off) and np.diff(off).min() == 23
    assert by["loose"]["depth_sum"].max() > 1 << 32 and (by["loose"]["var_depth"] == M32).sum() > 100
    assert by["zero"]["total"] == B and by["depth"]["total"] > 0 and by["all"]["total"] == 0 and by["p1001"]["total"] == 0 < by["p1000"]["total"] < by["loose"]["total"]
    code = PS._CODE[bases]
    others = cells.copy()
    others[np.arange(B), code] = -1
    top = np.sort(others, axis=1)
    for r in range(4):                                                # a tie for the alternative under each contig base, and equal counts of alt and contig
        tie = (code == r) & (top[:, 3] == top[:, 2]) & (top[:, 3] > 0)
        assert tie.sum() > 20 and (cells[tie, code[tie]] == top[tie, 3]).sum() > 3, r
    lit = list(c["literal"])
    assert [tuple(x) for x in cells[lit].tolist()] == list(FC.OVERFLOW_CELLS) and bases[lit].tolist() == [65, 65]
    g_of = lambda res: (off[res["var_unitig"]] + res["var_pos"]).tolist()
    assert lit[0] not in g_of(by["alt31"]) and lit[0] in g_of(by["loose"])           # the wrapped product 0 would make it a site
    assert by["major31"]["polished"][lit[1]] == 65                    # the wrapped product 0 would polish it to C
    wrapped = [PS.call(c["offsets"], c["bases"], c["counts"], mutant="products_wrap_at_2_64", **FC.CALL_PARAMS[i]) for i in (6, 7)]
    assert lit[0] in g_of(wrapped[0]) and wrapped[1]["polished"][lit[1]] == 67


@pytest.mark.parametrize("mutant", PS.MUTANTS)
def test_every_near_miss_is_told_from_the_rule(step_runs, place_runs, cell_runs, mutant):
    killed = 0
    if mutant in PS.PLACE_MUTANTS:
        for (seed, i), (c, places, piled) in step_runs.items():
            killed += not same_place(places, PS.place(c["offs"], c["steps"], c["offsets"], *FC.PLACE_PARAMS[i], mutant=mutant))
    elif mutant in PS.PILE_MUTANTS:
        for (seed, i), (c, places, piled) in step_runs.items():
            killed += i == 0 and not same_pile(piled, PS.pile(c["seqs"], places, c["offsets"], c["bases"], mutant=mutant))
        for seed, (c, piled, zero) in place_runs.items():
            killed += not same_pile(piled, PS.pile(c["seqs"], c["places"], c["offsets"], c["bases"], c["counts"], mutant=mutant))
    else:
        c, wants = cell_runs
        for th, want in zip(FC.CALL_PARAMS, wants):
            killed += not same_call(want, PS.call(c["offsets"], c["bases"], c["counts"], mutant=mutant, **th))
    assert killed > 0, mutant


def test_a_batch_and_its_reverse_complement_pile_alike(place_runs):
    for seed, (c, piled, zero) in place_runs.items():
        t = FC.rc_twin(c)
        assert t["seqs"] != c["seqs"] and not np.array_equal(t["places"]["place_q0"], c["places"]["place_q0"])
        assert same_pile(piled, PR.pile(t["seqs"], t["places"], t["offsets"], t["bases"], t["counts"])), seed
