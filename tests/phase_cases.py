"""Cases for the phasing tests (a helper, not a conftest): the planted diploid genome, random sites under the placements of
pileup_fuzz_cases.placements_case, hand-made chains of sites, and the restated chain place -> observe -> bundle -> solve -> tag.

  planted()                          the planted case (below)
  truth(p, contig)                   per site 1 iff the alternative base is haplotype B's, on the contig as the graph spells it
  random_sites(case, seed, n)        n sites on the contigs of a placements_case: ref = the contig's base, alt = another base
  chain_links(V, signs, n, cut)      the links of a chain of V sites: n links per edge (v - 1, v), all of sign signs[v % len(signs)]; with
                                     cut, every edge whose v is a multiple of it gets n links of the other sign too: a tie, undecided
  phase(seqs, places, offsets, sites, group, **thresholds)   (obs, edges, solved, tags) of the restatements

The planted case. default_rng(SEED): haplotype A is a random text of GENOME bases; haplotype B differs from it at SITES. The sites lie
40 to 60 bases apart from base 150 on, so a read of READ = 100 bases covers two or three, except for two stretches without a site: one
of GAP_READ = 150 bases behind base 1500, which no read bridges but a pair does, and one of GAP_PAIR = 420 bases behind base 3700,
longer than INSERT = 300, which nothing bridges. Reads start every 5 bases of A and every 10 of B where they start below MID = 3000, and
the other way round from there on, strands alternating; every ninth read carries one substitution. So the cleaning pops B's arm of every
bubble in the first half and A's arm in the second: the contig carries A's bases, then B's. The pairs are fragments of INSERT bases
starting every 10 bases of the stronger and every 20 of the weaker haplotype, error-free, mates of READ bases in alternating
orientation; sequences 2 i and 2 i + 1 are the mates of fragment i. The k-mers are counted from the reads. With these constants the
restated chain (pileup_cases.chain on the graph at cutoff 1 after three cleaning rounds, the default call thresholds) returns one contig
and exactly the planted sites, for the reads and for the mates alike; tests/test_phase_cpu.py checks that.
"""
import numpy as np

import phase_ref as HR
import pileup_cases as PC
import pileup_ref as PR

SEED, GENOME, READ, INSERT, MID = 11, 6000, 100, 300, 3000
GAP_READ, GAP_PAIR = (1500, 150), (3700, 420)                      # (the first base behind which no site lies, the bases without one)


def _site_positions(rng):
    out, x = [], 150
    while x < GENOME - 150:
        out.append(x)
        x += int(rng.integers(40, 61))
        for at, n in (GAP_READ, GAP_PAIR):
            if out[-1] < at <= x:
                x = out[-1] + n
    return tuple(out)


def planted() -> dict:
    rng = np.random.default_rng(SEED)
    hA = PC.random_text(rng, GENOME)
    sites = _site_positions(rng)
    hB = hA
    for x in sites:
        hB = PC.substitute(hB, x, int(rng.integers(1, 4)))
    reads, read_hap, read_clean = [], [], []
    for x in range(0, GENOME - READ + 1, 5):
        for hap, text in enumerate((hA, hB)):
            strong = (x < MID) == (hap == 0)
            if not strong and x % 10:
                continue
            r, clean = text[x:x + READ], True
            if len(reads) % 9 == 8:
                r, clean = PC.substitute(r, int(rng.integers(0, READ)), int(rng.integers(1, 4))), False
            reads.append(PC.rc(r) if len(reads) % 2 else r)
            read_hap.append(hap)
            read_clean.append(clean)
    mates, pair_hap = [], []
    for x in range(0, GENOME - INSERT + 1, 10):
        for hap, text in enumerate((hA, hB)):
            strong = (x < MID) == (hap == 0)
            if not strong and x % 20:
                continue
            left, right = text[x:x + READ], PC.rc(text[x + INSERT - READ:x + INSERT])
            mates += [right, left] if len(pair_hap) % 2 else [left, right]
            pair_hap.append(hap)
    codes, tfs = PC.kmer_table(reads)
    return dict(hA=hA, hB=hB, sites=sites, reads=reads, read_hap=read_hap, read_clean=read_clean, mates=mates, pair_hap=pair_hap, codes=codes, tfs=tfs)


def expected_sites(p, contig):
    """([(pos, ref, alt)] of the planted sites on `contig`: the base it spells there and the other haplotype's, ascending; whether the
    contig runs in the direction of the haplotypes)"""
    fwd = contig[:100] == p["hA"][:100]                             # no site lies in the first 150 bases
    assert fwd or contig[-100:] == PC.rc(p["hA"][:100])
    rows = []
    for x in p["sites"]:
        a, b = (p["hA"][x], p["hB"][x]) if fwd else (PC.rc(p["hA"][x]), PC.rc(p["hB"][x]))
        pos = x if fwd else GENOME - 1 - x
        assert contig[pos] in (a, b)
        rows.append((pos, contig[pos], b if contig[pos] == a else a))
    return sorted(rows), fwd


def truth(p, contig):
    """per site, in contig order: 1 iff the alternative base is haplotype B's (the contig spells A's there)"""
    rows, fwd = expected_sites(p, contig)
    out = []
    for pos, ref, alt in rows:
        x = pos if fwd else GENOME - 1 - pos
        out.append(int((alt if fwd else PC.rc(alt)) == p["hB"][x]))
    return out


def sites_dict(rows, unitig=0):
    """[(pos, ref, alt)] on one contig as the four site arrays"""
    cols = list(zip(*rows)) if rows else [[]] * 3
    return {"var_unitig": np.full(len(rows), unitig, np.uint32), "var_pos": np.array(cols[0], dtype=np.uint32),
            "var_ref": np.array([ord(c) for c in cols[1]], dtype=np.uint8), "var_alt": np.array([ord(c) for c in cols[2]], dtype=np.uint8)}


def random_sites(case: dict, seed: int, n: int) -> dict:
    """default_rng(seed): at most n distinct global bases of the case's contigs, base 0 and the last base among them; ref the contig's
    base, alt another base"""
    rng = np.random.default_rng(seed)
    off, bases = case["offsets"].astype(np.int64), case["bases"]
    B = int(off[-1])
    g = np.unique(np.concatenate(([0, B - 1], rng.choice(B, min(max(n - 2, 0), B), replace=False))))
    u = np.searchsorted(off, g, side="right") - 1
    ref = bases[g]
    alt = np.frombuffer(b"ACGT", np.uint8)[(np.searchsorted(np.frombuffer(b"ACGT", np.uint8), ref) + rng.integers(1, 4, g.shape[0])) % 4]
    return {"var_unitig": u.astype(np.uint32), "var_pos": (g - off[u]).astype(np.uint32), "var_ref": ref.astype(np.uint8), "var_alt": alt.astype(np.uint8)}


def chain_links(V: int, signs=(0,), n: int = 3, cut: int = 0) -> dict:
    lo, hi, rel = [], [], []
    for v in range(1, V):
        s = signs[v % len(signs)]
        tie = cut and v % cut == 0
        rels = [s] * n + ([1 - s] * n if tie else [])
        lo += [v - 1] * len(rels)
        hi += [v] * len(rels)
        rel += rels
    return {"link_lo": np.array(lo, dtype=np.uint32), "link_hi": np.array(hi, dtype=np.uint32), "link_rel": np.array(rel, dtype=np.uint8)}


def phase(seqs, places, offsets, sites, group: int = 1, **thr):
    seqs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
    obs = HR.observe(seqs, places, offsets, sites, group)
    edges = HR.bundle(len(sites["var_unitig"]), obs)
    solved = HR.solve(sites["var_unitig"], edges, **thr)
    return obs, edges, solved, HR.tag(obs, solved)
