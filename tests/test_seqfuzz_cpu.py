"""The cases of the sequence-search fuzz (seqfuzz_cases.py) under the restatements and the brute-force searches alone, no GPU: what
test_gpu_seqfuzz.py compares the device with is not empty, reaches every seed_step of its list and every byte of the dirt alphabet, and the
restatements agree with searches that know nothing of seeds or bands. The counts are conditions on the inputs, not measurements.

Obtained with this generator, per seed at its own seed_step and max_per_kmer 0 — seq_find records at hd 3, seq_edit records at ed 2,
records of strand 1, records with dist >= 1, proposals without an interval, proposals rejected by the band (required: 30, 30, 5, 5, 1, 1):
   seed  0  step 677        241 229 224 248   10   110      seed  6  step 2           61  66  67  93 1643 3003
   seed  1  step 1           49  42  38  59  154  1952      seed  7  step 47          60  62  68  50   15   80
   seed  2  step 24         201 267 222 314  112   965      seed  8  step 2^63 + 1   129 127 116 150   25   62
   seed  3  step 2^32       169 157 147 258   19    93      seed  9  step 23         114 135  75 139  118  469
   seed  4  step 22         108 108  96 172  154   495      seed 10  step 10^6        66  77  70  91   34   45
   seed  5  step 678         73  90  75 123   20    43      seed 11  step 5          133 128 127 159  257 3800
Over all seeds: dist 0 .. 3 all seen; every byte of DIRT inside the compared span of a record of a dirty pattern, on the read side, and
in a dirty pattern with a record of strand 1; every seed_step has patterns with records. The restatements equal the brute-force
searches wherever the header's conditions hold; where the index stores k-mers as met (seed % 3 != 0) the generator breaks 'every
occurrence indexed' for k-mers met as their larger strand alone, and those windows are charged like edits (seqfuzz_cases.dead_seeds)."""
import numpy as np
import pytest

import seqfuzz_cases as S
import seqfind_ref as F


def _reduce(rows, skip):
    out = {}
    for s, e, rid, local, strand, d in rows:
        if rid not in skip:
            out[(rid, strand)] = min(out.get((rid, strand), 99), d)
    return out


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """every seed's case, its restatement and what the tests below look at, computed once"""
    tmp = str(tmp_path_factory.mktemp("seqfuzz"))
    out = []
    for seed in range(S.N_SEEDS):
        case = S.make_case(seed, tmp)
        ref = S.make_ref(case)
        pats = case[5]
        step = S.step_of(seed, pats)
        sf, se = {}, {}
        find = [ref.find(p, 3, step, 0, sf) for p, _ in pats]
        edit = [ref.find_ed(p, 2, step, 0, se) for p, _ in pats]
        out.append(dict(seed=seed, case=case, ref=ref, step=step, find=find, edit=edit, sf=sf, se=se))
    return out


def test_oracle_positions_hold_every_occurrence(world):
    """Every fourth seed attaches OracleIndex23.positions(reads): with tf equal to the true counts it holds, per bucket, the entries of
    seqedit_ref.full_index over all reads (the order inside a bucket is the same too: both walk the buffer upwards)."""
    import seqedit_ref as E
    n = 0
    for w in world:
        if w["seed"] % 4:
            continue
        prefix, reads, ridx, indices, positions, _ = w["case"]
        find, fpos = E.full_index(S.make_ref(w["case"], ridx=S.all_intervals(reads)))
        assert np.array_equal(find, indices) and int(indices[-1]) == positions.shape[0] > 1000
        for h in range(indices.shape[0] - 1):
            a, b = int(indices[h]), int(indices[h + 1])
            assert set(positions[a:b].tolist()) == set(fpos[a:b].tolist()) and 0 not in positions[a:b]
        n += 1
    assert n == 3


def test_restatements_against_brute_force(world):
    """F.find == F.brute record for record and E.find_ed, reduced to {(rid, strand): min dist}, == E.brute_ed, on the clean patterns with
    max_per_kmer 0 and seed_step 1 and 23, for hd / ed below len // 23 - dead seeds (seqfuzz_cases.dead_seeds: 0 in the canonical cases),
    on the reads without an N."""
    checked = found = dead = 0
    for w in world:
        ref, seed = w["ref"], w["seed"]
        skip = S.n_reads_of(ref)
        for p, kind in w["case"][5]:
            if kind != "clean":
                continue
            u = S.dead_seeds(ref, p)
            assert u == 0 or seed % 3
            dead += u
            top = len(p) // 23 - u
            table = ref.brute_ed(p, 2) if top > 0 else {}
            for d in (0, 1, 3):
                if d >= top:
                    continue
                want = [r for r in ref.brute(p, d) if r[1] not in skip]
                for step in (1, 23):
                    assert [r for r in ref.find(p, d, step) if r[1] not in skip] == want, (seed, len(p), d, step)
                    checked += 1
                found += len(want)
            for d in (0, 1, 2):
                if d >= top:
                    continue
                want = {k: v for k, v in table.items() if v <= d and k[0] not in skip}
                for step in (1, 23):
                    assert _reduce(ref.find_ed(p, d, step), skip) == want, (seed, len(p), d, step)
                    checked += 1
                found += len(want)
    print("comparisons", checked, "records", found, "dead seed windows", dead)
    assert checked > 2000 and found > 1000 and dead > 0


def test_every_seed(world):
    for w in world:
        find = [r for rs in w["find"] for r in rs]
        edit = [r for rs in w["edit"] for r in rs]
        fig = (len(find), len(edit), sum(r[3] == 1 for r in find) + sum(r[4] == 1 for r in edit), sum(r[4] >= 1 for r in find) + sum(r[5] >= 1 for r in edit),
               w["se"].get("no_interval", 0), w["se"].get("rejected", 0), w["sf"].get("rejected", 0))
        print("seed", w["seed"], "step", w["step"], "mode", w["seed"] % 3, "reads", len(w["case"][1]), "find(hd 3) edit(ed 2) strand-1 dist>=1 no_interval rejected", fig)
        assert fig[0] >= 30 and fig[1] >= 30 and fig[2] >= 5 and fig[3] >= 5 and fig[4] >= 1 and fig[5] >= 1 and fig[6] >= 1, (w["seed"], fig)


def test_over_all_seeds(world):
    dists, read_dirt, pat_dirt, n_gain, stepped = set(), set(), set(), 0, {}
    for w in world:
        ref, pats, step = w["ref"], w["case"][5], w["step"]
        for (p, kind), fr, er in zip(pats, w["find"], w["edit"]):
            dists |= {r[4] for r in fr} | {r[5] for r in er}
            if fr or er:
                stepped.setdefault(step, []).append(len(p))
            if kind != "dirty":
                continue
            for a, rid, local, strand, d in fr:
                x = ref.reads[a:a + len(p)]
                read_dirt |= set(x) & set(S.DIRT)
                if strand == 1:
                    pat_dirt |= set(p) & set(S.DIRT)
                y = F.comp_rev(p) if strand else p
                if b"N" in p and d < sum(1 for u, v in zip(x, y) if u != v):
                    n_gain += 1
            for s, e, rid, local, strand, d in er:
                read_dirt |= set(ref.reads[s:e]) & set(S.DIRT)
                if strand == 1:
                    pat_dirt |= set(p) & set(S.DIRT)
    print("dist values", sorted(dists), "dirt on the read side", sorted(read_dirt), "on the pattern side, strand 1", sorted(pat_dirt), "N forgiven", n_gain,
          "patterns with records per step", {k: len(v) for k, v in stepped.items()})
    assert {0, 1, 2, 3} <= dists
    assert read_dirt == set(S.DIRT) and pat_dirt == set(S.DIRT) and n_gain >= 1
    assert set(stepped) == set(S.steps(700)) and len(stepped) == S.N_SEEDS
    for big in (1 << 32, (1 << 63) + 1):                      # one seed, at offset 0: the records come from it
        w = next(w for w in world if w["step"] == big)
        assert all(len(range(0, len(p) - 22, big)) <= 1 for p, _ in w["case"][5])
        assert sum(len(w["ref"].proposals_ed(p, big)) for p, _ in w["case"][5]) >= 30


def test_beyond_4gib_case(world):
    """test_search_beyond_4gib puts 2^31 and 2^32 at the offsets h .. h + 3 of seed 2's reads image: each lies inside a read, and records of
    every search it compares run across it."""
    w = world[2]
    ref, pats = w["ref"], [p for p, _ in w["case"][5]]
    h = S.beyond_offset(w["case"])
    assert 10_000 <= len(w["case"][1]) <= 30_000
    find = [(r[0], r[0] + len(p)) for p in pats for r in ref.find(p, 2, 7)]
    e21 = [(r[0], r[1]) for p in pats for r in ref.find_ed(p, 2, 1)]
    e723 = [(r[0], r[1]) for p in pats for r in ref.find_ed(p, 7, 23)]
    for at in range(h, h + 4):
        assert ref.interval(at - 1, 3) is not None
        n = [sum(1 for a, b in rows if a < at < b) for rows in (find, e21, e723)]
        assert min(n) >= 1, (at, n)
    print("offset", h, "records across it: find, edit (2, 1), edit (7, 23)", n)


def test_hostile_case(world):
    """Seed 1's case with the hostile attachments: every planted kind lies in a list that a seed of some pattern reads, and each of the four
    odd intervals decides a proposal."""
    case = world[1]["case"]
    ind, pos, ridx, pats, info = S.hostile_case(case)
    ref = S.make_ref(case, indices=ind, positions=pos, ridx=ridx)
    base = S.make_ref(case)
    reads = case[1]
    vals = S.plant_values(reads)
    assert sorted({k for k, _ in info["planted"]}) == sorted(vals) and len(info["planted"]) == 3 * len(vals)
    seen = set()
    for p, _ in pats:
        for q in range(len(p) - 22):
            h = ref.bucket(p[q:q + 23])
            if h is not None:
                raw = pos[int(ind[h]):int(ind[h + 1])].tolist()
                seen |= {k for k, v in vals.items() if v in raw}
    assert seen == set(vals)
    row = lambda name: [int(x) for x in ridx[info[name]]]
    beyond, empty, seed23 = row("beyond"), row("empty"), row("seed23")
    cut = info["cut"]
    n = dict(beyond=0, beyond_clip=0, empty=0, seed23=0, span=0, clip=0)
    for p, _ in pats:
        L = len(p)
        for a, strand, p0 in ref.proposals_ed(p, 1):
            i = ref.seed_interval(p0)
            if beyond[1] <= p0 and a + L > len(reads):
                n["beyond"] += 1                                # the interval would hold it, the reads do not: dropped by seq_find
                n["beyond_clip"] += i is not None               # seq_edit: hi = len(reads)
            if empty[1] <= p0 < empty[1] + len(pats[-2][0]):
                assert i is None
                n["empty"] += 1
            if i is not None and ref.start[i] == seed23[1]:
                n["seed23"] += 1
            if cut - 23 < p0 <= cut:
                assert i is None
                n["span"] += 1
            if i is not None and ref.start[i] == cut + 1 and a - 2 < cut + 1:
                n["clip"] += 1
    got = [r for p, _ in pats for r in ref.find_ed(p, 2, 1)]
    was = [r for p, _ in pats for r in base.find_ed(p, 2, 1)]
    kept23 = [r for r in got if r[2] == seed23[0] and r[1] - r[0] == 23 and r[5] == 0]
    print("proposals decided by the odd intervals", n, "records", len(got), "without the hostile attachments", len(was), "in the 23-byte interval", len(kept23))
    assert all(v >= 1 for v in n.values()) and kept23 and any(r[2] == 1000 for r in got) and got != was
    st = {}
    assert not any(r[0] >= beyond[1] for r in ref.find(pats[-3][0], 3, 1, 0, st)) and st["bounds"] >= 1     # the last read with three bytes behind it
    assert any(r[1] == seed23[0] for r in ref.find(pats[-1][0], 0, 1)) and ref.find(pats[0][0], 3, 1) == [] and base.find(pats[0][0], 3, 1) != []
