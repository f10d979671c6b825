"""Generate tests/golden/small23/frequency.json and tests/golden/graph23/frequency.json from the COMPILED REFERENCE (oracle/_ref, built
by `make -C oracle ref`). Run from the repository root:  python tests/golden/make_golden_spectrum.py

Everything a k-mer answers comes from the reference's pybind11 module: get_kmer_by_kid(kid) and get_tf_values of those strings for every kid
(the enumeration of AIndex.iter_kmers_by_frequency, aindex/core/aindex.py:654-679), get_kmer_info for a sample of kids. The selection is the
loop of aindex.py:659-679 restated below on (kid, tf) pairs: keep tf >= min_tf, list.sort(key = tf, reverse = True) — Python's stable sort —
and the cut freq_list[:max_kmers]. Only data is written. To keep the fixtures small, a list of more than HEAD entries is written as its
first HEAD entries, its length and the SHA-256 of its compact JSON form (digest() below; the tests apply the same function to their lists)."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLD = os.path.join(ROOT, "tests", "golden")
REF = os.path.join(ROOT, "oracle", "_ref")


HEAD = 64


def digest(items):
    return hashlib.sha256(json.dumps(list(items), separators=(",", ":")).encode()).hexdigest()


def packed(items):
    items = list(items)
    return items if len(items) <= HEAD else {"head": items[:HEAD], "len": len(items), "sha256": digest(items)}


def selection(values, min_tf, max_kmers):
    freq_list = [(kid, tf) for kid, tf in enumerate(values) if tf >= min_tf]      # aindex.py:661-668
    total = len(freq_list)
    freq_list.sort(key=lambda x: x[1], reverse=True)                              # :671
    if max_kmers is not None:
        freq_list = freq_list[:max_kmers]                                         # :674-675
    return {"min_tf": min_tf, "max_kmers": max_kmers, "total": total, "kid": packed(k for k, _ in freq_list), "tf": packed(t for _, t in freq_list)}


def document(prefix, cases, info_kids):
    sys.path.insert(0, REF)
    import aindex_cpp
    w = aindex_cpp.AindexWrapper()
    w.load_from_prefix_23mer(prefix)
    n = int(w.get_hash_size())
    kmers = [w.get_kmer_by_kid(kid) for kid in range(n)]
    values = [int(t) for t in w.get_tf_values(kmers)]
    kids = [k if k >= 0 else n + k + 1 for k in info_kids]                        # -1 = n (one beyond the index)
    info = [list(w.get_kmer_info(k)) for k in kids]
    return {"n": n, "kmers": packed(kmers), "values": values, "selections": [selection(values, a, b) for a, b in cases],
            "info_kids": kids, "info": [[int(t), a, b] for t, a, b in info]}


def main():
    small = document(os.path.join(GOLD, "small23", "small23"),
                     [(2, 25), (1, 18), (1, 8), (1, 1), (1, 10 ** 4), (19, 10), (1, None), (0, None), (16, None), (17, 3), (18, 8), (1, 0)],
                     [0, 1, 2, 17, 100, 2500, 5899, 5900, -1])
    v = small["values"]
    assert small["n"] == 5901 and max(v) == 18 and min(v) == 1
    assert (v.count(18), v.count(17), v.count(16)) == (8, 10, 32), "the tie classes the top-25 and top-18 cuts rely on"
    s25, s18 = small["selections"][0], small["selections"][1]
    assert s25["tf"].count(16) == 7 and len(s25["kid"]) == 25, "top-25 must cut inside the class of 16"
    assert s18["tf"][-1] == 17 and len(s18["kid"]) == 18, "top-18 must end exactly on a class boundary"
    assert small["selections"][4]["total"] == 5901 == small["selections"][4]["kid"]["len"] and small["selections"][5]["kid"] == []
    assert small["info"][-1] == [0, "", ""]
    graph = document(os.path.join(GOLD, "graph23", "graph23"), [(1, None), (1, 5), (2, None), (2, 7), (3, 1000), (4, None), (0, 3)], [0, 1, 5, -2, -1])
    assert graph["info"][-1] == [0, "", ""] and len(set(graph["values"])) >= 3
    for name, doc in (("small23", small), ("graph23", graph)):
        path = os.path.join(GOLD, name, "frequency.json")
        with open(path, "w") as fh:
            json.dump(doc, fh, separators=(",", ":"))
        print(name, "n", doc["n"], "selections", len(doc["selections"]), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
