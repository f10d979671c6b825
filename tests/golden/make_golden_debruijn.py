"""Generate tests/golden/small23/debruijn.json and the tiny key set tests/golden/graph23/ (+ its debruijn.json) from the COMPILED
REFERENCE (oracle/_ref, built by `make -C oracle ref`). Run from the repository root:  python tests/golden/make_golden_debruijn.py

Every frequency comes from the reference's pybind11 module (AindexWrapper.get_tf_values on the decoded neighbour strings; for a pure-ACGT
string that is the computation of PHASH_MAP::get_freq(uint64_t), hash.hpp:123-140). The CONT rule (DEBRUJIN::print_next / print_prev) and
the walk are applied below by a scalar restatement, one k-mer at a time, that follows debrujin.cpp line by line; tests/debruijn_ref.py
holds a second, vectorised one, and tests/test_debruijn_cpu.py checks that the two agree on every answer written here.
Only data is written: query strings, the reference's frequencies and what the rules make of them.

graph23 is a hand-made key set that holds what small23 (reads of a random genome) does not: a circular sequence (LOOP), a fork with equal
counts (a tie between two non-zero successors, BRANCH) and two sequences that merge (JOIN). Its keys are the forward-strand 23-mers of
the sequences of graph23_sequences() with their counts; compute_mphf_seq and compute_index of the reference turn them into .pf / .tf.bin / .kmers.bin."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLD = os.path.join(ROOT, "tests", "golden")
REF = os.path.join(ROOT, "oracle", "_ref")
TMP = "/tmp/aix_golden_debruijn"
MASK46 = (1 << 46) - 1
NEXT, PREV = 0, 1
GREEDY, UNITIG = 0, 1
MAX_STEPS, DEAD_END, BRANCH, JOIN, LOOP = 0, 1, 2, 3, 4


def enc(s: str) -> int:                                             # get_dna23_bitset, kmers.cpp:12-40: other bytes add 0 bits
    u = 0
    for ch in s:
        u = (u << 2) | {"A": 0, "C": 1, "G": 2, "T": 3}.get(ch, 0)
    return u


def dec(u: int) -> str:
    return "".join("ACGT"[(u >> (2 * (22 - j))) & 3] for j in range(23))


def rc_code(u: int) -> int:
    return enc("".join({"A": "T", "C": "G", "G": "C", "T": "A"}[c] for c in reversed(dec(u))))


class Ref:
    """get_freq(code) through the compiled reference, cached."""
    def __init__(self, prefix):
        sys.path.insert(0, REF)
        import aindex_cpp
        self.w = aindex_cpp.AindexWrapper()
        self.w.load_from_prefix_23mer(prefix)
        self.cache = {}

    def freq4(self, codes):
        miss = [c for c in codes if c not in self.cache]
        if miss:
            for c, t in zip(miss, self.w.get_tf_values([dec(c) for c in miss])):
                self.cache[c] = int(t)
        return [self.cache[c] for c in codes]


def cont(ref: Ref, kmer: int, direction: int, cutoff: int):
    """debrujin.cpp:30-75 (print_next) / :121-167 (print_prev) -> (tf[4], n, sum, best_tf, best_base, best_ukmer)"""
    if direction == NEXT:
        k4 = [((kmer << 2) | b) & 0x00003fffffffffff for b in range(4)]           # :34-37
    else:
        k4 = [(kmer >> 2) | (b << 44) for b in range(4)]                          # :125-128
    A, C, G, T = ref.freq4(k4)                                                     # :39-42 / :130-133
    if cutoff > 0:                                                                 # :44-49 / :135-140
        if A <= cutoff: A = 0
        if C <= cutoff: C = 0
        if G <= cutoff: G = 0
        if T <= cutoff: T = 0
    sm = (A + C + G + T) & 0xFFFFFFFF                                              # :51 / :142 (uint32_t)
    n = int(bool(A)) + int(bool(C)) + int(bool(G)) + int(bool(T))                  # :52-53 / :165-166
    best = None
    if A >= C and A >= G and A >= T: best = (0, A)                                 # :55-59 / :144-148
    if C >= A and C >= G and C >= T: best = (1, C)                                 # :60-64 / :149-153
    if G >= C and G >= A and G >= T: best = (2, G)                                 # :65-69 / :154-158
    if T >= C and T >= G and T >= A: best = (3, T)                                 # :70-74 / :159-163
    return [A, C, G, T], n, sm, best[1], best[0], k4[best[0]]


def walk(ref: Ref, seed: int, direction: int, L: int, cutoff: int, mode: int):
    cur, bases, tfs, stop = seed, "", [], MAX_STEPS
    seedc = min(seed, rc_code(seed))
    while len(bases) < L:
        _, n, _, btf, bb, nxt = cont(ref, cur, direction, cutoff)
        if n == 0:
            stop = DEAD_END
            break
        if mode == UNITIG and n > 1:
            stop = BRANCH
            break
        if mode == UNITIG and cont(ref, nxt, 1 - direction, cutoff)[1] > 1:
            stop = JOIN
            break
        if min(nxt, rc_code(nxt)) == seedc:
            stop = LOOP
            break
        bases += "ACGT"[bb]
        tfs.append(btf)
        cur = nxt
    return bases, stop, tfs, cur


def rng_dna(seed: int, n: int) -> str:
    return "".join("ACGT"[i] for i in np.random.default_rng(seed).integers(0, 4, n))


def rc_str(s: str) -> str:
    return "".join({"A": "T", "C": "G", "G": "C", "T": "A"}[c] for c in reversed(s))


def run(cmd):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if r.returncode != 0:
        sys.stderr.write(r.stderr.decode(errors="replace")[-2000:])
        raise SystemExit(f"{cmd} failed with {r.returncode}")


def graph23_sequences():
    circle = rng_dna(11, 60)
    stem, arm_a, arm_c = rng_dna(12, 40), rng_dna(13, 30), rng_dna(14, 30)
    left1, left2, trunk = rng_dna(15, 35), rng_dna(16, 35), rng_dna(17, 45)
    return {
        "circle": [circle + circle[:22]] * 2,                       # all 60 cyclic 23-mers, tf 2
        "fork": [stem + "A" + arm_a, stem + "C" + arm_c],           # the last 23-mer of the stem has successors A and C, tf 1 each
        "merge": [left1 + "G" + trunk, left2 + "T" + trunk],        # the first 23-mer of the trunk has two predecessors
        "heavy": [left1 + "G" + trunk] * 3,                         # one side of the merge outweighs the other (cutoff = an occurring tf)
    }


def make_graph23():
    d = os.path.join(GOLD, "graph23")
    os.makedirs(d, exist_ok=True)
    shutil.rmtree(TMP, ignore_errors=True)
    os.makedirs(TMP)
    seqs = [s for group in graph23_sequences().values() for s in group]
    counts, canon_of = {}, {}
    for s in seqs:
        for i in range(len(s) - 22):
            k = s[i:i + 23]
            key = canon_of.setdefault(min(k, rc_str(k)), k)          # one strand per k-mer: the one met first
            counts[key] = counts.get(key, 0) + 1
    dat, keys, pf = os.path.join(TMP, "graph23.dat"), os.path.join(TMP, "keys.txt"), os.path.join(d, "graph23.pf")
    with open(dat, "w") as f, open(keys, "w") as g:
        for k, c in counts.items():
            f.write(f"{k}\t{c}\n")
            g.write(k + "\n")
    run([os.path.join(REF, "compute_mphf_seq"), keys, pf])
    run([os.path.join(REF, "compute_index"), dat, pf, os.path.join(d, "graph23"), "1", "0"])
    for name in os.listdir(d):                                       # keep what the handle opens
        if name not in ("graph23.pf", "graph23.tf.bin", "graph23.kmers.bin", "debruijn.json"):
            os.remove(os.path.join(d, name))
    return seqs


def windows(s: str):
    return [s[i:i + 23] for i in range(len(s) - 22)]


def answers(prefix: str, queries, cutoffs, walk_seeds, walk_cutoffs):
    ref = Ref(prefix)
    doc = {"queries": queries, "neighbours": [], "walks": []}
    codes = [enc(q) for q in queries]
    for cutoff in cutoffs:
        rec = {"cutoff": cutoff}
        for name, direction in (("next", NEXT), ("prev", PREV)):
            rows = []
            for u in codes:
                tf, n, sm, btf, bb, _ = cont(ref, u, direction, cutoff)
                rows.append(tf + [n, sm, btf, bb])
            rec[name] = rows
        doc["neighbours"].append(rec)
    for cutoff in walk_cutoffs:
        for mode in (GREEDY, UNITIG):
            for direction in (NEXT, PREV):
                for L in (1, 7, 200):
                    res = [walk(ref, codes[i], direction, L, cutoff, mode) for i in walk_seeds]
                    doc["walks"].append({"cutoff": cutoff, "mode": mode, "dir": direction, "L": L, "seeds": list(walk_seeds),
                                         "bases": [r[0] for r in res], "stop": [r[1] for r in res], "tf": [r[2] for r in res],
                                         "last": [r[3] for r in res]})
    return doc


def conditions(docs):
    stops, tie, zero = set(), False, False
    for doc in docs:
        for w in doc["walks"]:
            stops |= set(w["stop"])
        for rec in doc["neighbours"]:
            for rows in (rec["next"], rec["prev"]):
                for r in rows:
                    nz = sorted(x for x in r[:4] if x)
                    tie |= len(nz) >= 2 and nz[-1] == nz[-2]
                    zero |= r[4] == 0
    return stops, tie, zero


def main():
    # ---- small23 ----
    prefix = os.path.join(GOLD, "small23", "small23")
    reads = open(prefix + ".reads").read().split("\n")
    stored = [ln.split("\t")[0] for ln in open(prefix + ".dat").read().split("\n") if ln]
    tfs = sorted(int(ln.split("\t")[1]) for ln in open(prefix + ".dat").read().split("\n") if ln)
    q = []
    for r in reads[:3]:
        q += windows(r.replace("~", "")[:150])
    q += stored[:20] + [rc_str(s) for s in stored[40:60]]
    q += [rng_dna(500 + i, 23) for i in range(20)]
    q += ["A" * 23, "T" * 23]
    for i, s in enumerate(stored[80:85]):                            # N and lower case: sanitised to A
        p = (5 * i) % 23
        q += [s[:p] + "N" + s[p + 1:], s.lower(), s[:p] + s[p].lower() + s[p + 1:]]
    q = [s for s in q if len(s) == 23]
    mid_tf = tfs[len(tfs) // 2]                                      # a cutoff equal to an occurring tf pins `<=`
    small = answers(prefix, q, [0, 1, mid_tf], list(range(0, len(q), 20)), [0, mid_tf])
    small["cutoff_equal_to_a_tf"] = mid_tf
    # ---- graph23 ----
    seqs = make_graph23()
    gq = []
    gq += windows(seqs[0])[::3] + windows(seqs[2]) + windows(seqs[3])[12:] + windows(seqs[4])[::2] + windows(seqs[5])[:40:2]
    gq += [rc_str(s) for s in gq[::7]] + ["A" * 23, rng_dna(900, 23)]
    graph = answers(os.path.join(GOLD, "graph23", "graph23"), gq, [0, 1, 3], list(range(0, len(gq), 6)), [0, 1])
    # ---- what the goldens must contain ----
    stops, tie, zero = conditions([small, graph])
    assert stops == {MAX_STEPS, DEAD_END, BRANCH, JOIN, LOOP}, stops
    assert tie, "no CONT with a tie between two non-zero successors"
    assert zero, "no all-zero CONT"
    assert any(mid_tf in r[:4] for r in small["neighbours"][0]["next"]), "the cutoff equal to a tf meets no such tf"
    for name, doc in (("small23", small), ("graph23", graph)):
        path = os.path.join(GOLD, name, "debruijn.json")
        with open(path, "w") as fh:
            json.dump(doc, fh, separators=(",", ":"))
        print(name, "queries", len(doc["queries"]), "walk legs", len(doc["walks"]), os.path.getsize(path), "bytes")
    print("stops", sorted(stops), "tie", tie, "all-zero", zero)


if __name__ == "__main__":
    main()
