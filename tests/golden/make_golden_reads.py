"""Generate tests/golden/small23/reads_access.json and tests/golden/compute_reads/reads_access.json from the COMPILED REFERENCE
(oracle/_ref/aindex_cpp, built by `make -C oracle ref`): the answers of AindexWrapper.get_read_by_rid and get_read
(python_wrapper.cpp:666-698) on committed reads files. Run from the repository root:  python tests/golden/make_golden_reads.py

Only data the reference's module returns is written; the reads files themselves and their .ridx files are already committed.
Strings are stored as latin-1 text (one character per byte). To keep the files small the get_read_by_rid answers are stored in full for
every eighth rid and the out-of-range ones, and for ALL rids as their lengths plus one SHA-256 over the answers in rid order (digest()
below), which a test recomputes from what it got: equal digests and lengths mean equal answers for every rid."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLD = os.path.join(ROOT, "tests", "golden")
REF = os.path.join(ROOT, "oracle", "_ref")

FILES = {
    os.path.join("small23", "reads_access.json"): [("small23/small23.reads", 600, 23)],
    os.path.join("compute_reads", "reads_access.json"): [("compute_reads/pe.reads", 40, 29), ("compute_reads/edge_pe_iupac.reads", 40, 31)],
}


def digest(strings) -> str:
    """SHA-256 over the answers in order, each as its length (8 bytes, little endian) followed by its latin-1 bytes."""
    h = hashlib.sha256()
    for s in strings:
        b = s.encode("latin-1")
        h.update(len(b).to_bytes(8, "little") + b)
    return h.hexdigest()


def _text(b) -> str:
    return b if isinstance(b, str) else bytes(b).decode("latin-1")


def triples(data: bytes, n: int, seed: int):
    """n seeded (start, end, revcomp) triples plus the fixed edge cases; at least a third with revcomp."""
    size = len(data)
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        a = int(rng.integers(0, size))
        ln = int(rng.choice([0, 1, 15, 16, 17, 23, 63, 64, 65])) if i % 3 else int(rng.integers(0, min(size, 160)))
        out.append((a, min(a + ln, size - 1 if i % 5 else size), bool(i % 2)))
    seps = [i for i, c in enumerate(data) if c in b"\n~"]
    for s in seps[:: max(1, len(seps) // 40)]:                       # spans across '\n' and '~'
        out.append((max(s - 9, 0), min(s + 11, size - 1), bool(s % 2)))
    ns = [i for i, c in enumerate(data) if c == ord("N")]
    for s in ns[:: max(1, len(ns) // 30)]:                           # spans over the N runs
        out.append((max(s - 20, 0), min(s + 25, size - 1), bool(s % 2)))
        out.append((max(s - 3, 0), min(s + 40, size - 1), not s % 2))
    for rc in (False, True):
        out += [(0, 0, rc), (5, 5, rc), (7, 3, rc), (size - 1, size - 1, rc), (size - 20, size - 1, rc), (size - 20, size, rc), (0, size, rc),
                (size, size, rc), (size, size + 5, rc), (size + 100, size + 200, rc), (size - 1, size, rc), (3, 2 ** 40, rc), (2 ** 40, 2 ** 40 + 1, rc)]
    return out


def main():
    sys.path.insert(0, REF)
    import aindex_cpp  # the reference's pybind11 module, compiled by oracle/Makefile
    for out_name, sources in FILES.items():
        doc = {"files": []}
        for rel, n, seed in sources:
            path = os.path.join(GOLD, rel)
            data = open(path, "rb").read()
            w = aindex_cpp.AindexWrapper()
            w.load_reads(path)
            n_reads = int(w.n_reads)
            rids = list(range(n_reads)) + [n_reads, n_reads + 1, 2 ** 40]
            by_rid = [_text(w.get_read_by_rid(r)) for r in rids]
            tr = triples(data, n, seed)
            doc["files"].append({
                "reads": rel, "size": len(data), "n_reads": n_reads,
                "rids": rids, "by_rid_len": [len(x) for x in by_rid], "by_rid_sha256": digest(by_rid),
                "by_rid_sample": {str(r): x for r, x in list(zip(rids, by_rid))[::8] + list(zip(rids, by_rid))[-3:]},
                "triples": [[a, b, int(rc)] for a, b, rc in tr], "get_read": [_text(w.get_read(a, b, rc)) for a, b, rc in tr],
            })
            print(rel, "reads", n_reads, "triples", len(tr), "revcomp", sum(1 for t in tr if t[2]))
        with open(os.path.join(GOLD, out_name), "w") as fh:
            json.dump(doc, fh, separators=(",", ":"))
        print("wrote", out_name, os.path.getsize(os.path.join(GOLD, out_name)), "bytes")


if __name__ == "__main__":
    main()
