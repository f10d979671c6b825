"""Cases for the pile-up tests (a helper, not a conftest): graphs restated from k-mers, the whole restated chain thread -> place -> pile,
and the planted heterozygous genome of the issue.

  kmer_table(texts)                       (codes ascending, tfs): the canonical 23-mers of the texts with their counts
  ref_graph(codes, tfs, cutoff, rounds)   dict un, lk, g, kid_of, node: the restated unitig graph, `rounds` cleaning rounds with the map composed
  chain(G, seqs, ...)                     (steps, places, piled) of the restatements on graph G
  rc(text)                                reverse complement of an upper-case str
  expected_sites(p, contig)               [(pos, ref, alt)] of the planted sites on the contig as the graph spells it
  planted()                               the planted case: two haplotypes that differ at SITES, reads of both, the k-mers counted from the reads
"""
import numpy as np

import graph_clean_ref as GR
import pileup_ref as PR
import seqthread_ref as SR
import unitig_links_ref as RL
import unitigs_ref as R

K = 23
_RC = str.maketrans("ACGT", "TGCA")
GENOME, READ, SITES = 4000, 100, tuple(range(150, 3850, 97))


def rc(s: str) -> str:
    return s[::-1].translate(_RC)


def kmer_table(texts):
    table = {}
    for t in texts:
        for q in range(len(t) - K + 1):
            w = t[q:q + K]
            if set(w) <= set("ACGT"):
                c = R.canon(RL.encode(w))
                table[c] = table.get(c, 0) + 1
    codes = np.array(sorted(table), dtype=np.uint64)
    return codes, np.array([table[int(c)] for c in codes.tolist()], dtype=np.uint32)


def ref_graph(codes, tfs, cutoff: int = 0, rounds: int = 0) -> dict:
    un = R.unitigs(codes, tfs, cutoff)
    lk = RL.links(codes, tfs, cutoff, un)
    g = GR.graph(un, lk)
    km = (un["kid_unitig"], un["kid_pos"], un["kid_flag"])
    done = 0
    while done < rounds:
        remove = GR.mark(g, 46, 46)
        if not remove.any():
            break
        nxt = GR.compact(g, remove)
        km = SR.kidmap(*km, g["offsets"], nxt["unitig_contig"], nxt["unitig_pos"], nxt["unitig_flag"])
        g = nxt
        done += 1
    return dict(un=un, lk=lk, g=g, kid_of={int(c): i for i, c in enumerate(np.asarray(codes).tolist())}, node=SR.nodes(*km, g["offsets"]), rounds=done,
                strings=[g["bases"].tobytes()[int(a):int(b)].decode() for a, b in zip(g["offsets"][:-1], g["offsets"][1:])])


def seq_offs(seqs):
    offs = np.zeros(len(seqs) + 1, np.uint64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    return offs


def chain(G: dict, seqs, max_gap: int = 46, extend: int = 22, counts=None):
    seqs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
    steps = SR.thread(G["kid_of"], G["node"], G["g"], seqs)
    places = PR.place(seq_offs(seqs), steps, G["g"]["offsets"], max_gap, extend)
    return steps, places, PR.pile(seqs, places, G["g"]["offsets"], G["g"]["bases"], counts)


def random_text(rng, n: int) -> str:
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n).tolist())


def substitute(s: str, i: int, step: int = 1) -> str:
    return s[:i] + "ACGT"[("ACGT".index(s[i]) + step) % 4] + s[i + 1:]


def planted() -> dict:
    """default_rng(7): a genome of 4000 bases; haplotype two differs at SITES; reads of 100 bases every 5 bases of haplotype one and every
    10 of haplotype two, strands alternating; every ninth read carries one substitution; the k-mers are counted from the reads."""
    rng = np.random.default_rng(7)
    h1 = random_text(rng, GENOME)
    h2 = h1
    for p in SITES:
        h2 = substitute(h2, p, int(rng.integers(1, 4)))
    reads = []
    for hap, step in ((h1, 5), (h2, 10)):
        for x in range(0, GENOME - READ + 1, step):
            r = hap[x:x + READ]
            if len(reads) % 9 == 8:
                r = substitute(r, int(rng.integers(0, READ)), int(rng.integers(1, 4)))
            reads.append(rc(r) if len(reads) % 2 else r)
    codes, tfs = kmer_table(reads)
    return dict(h1=h1, h2=h2, reads=reads, codes=codes, tfs=tfs)


def expected_sites(p, contig):
    """[(pos, ref, alt)] of the planted sites on the contig as the graph spells it"""
    if contig == p["h1"]:
        return [(x, p["h1"][x], p["h2"][x]) for x in SITES]
    assert contig == rc(p["h1"])
    return sorted((GENOME - 1 - x, rc(p["h1"][x]), rc(p["h2"][x])) for x in SITES)
