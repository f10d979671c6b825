"""Batch read retrieval on the MI355X: rate of Index.fetch_reads_by_rid_t / fetch_reads_t in GB/s of bytes delivered, beside the two
ceilings measured in the same process (a device-to-device copy of the same byte count: streaming; the library's random-read probe at
16-byte elements: random-line), and get_reads_by_kmer_batch against the per-k-mer host loop. One JSON line per leg on stdout and in --out.

  a  fetch_reads_by_rid_t of --n1 and --n2 random reads of a --reads x 150 bp synthetic reads buffer (synth_reads_t), and the same spans
     through fetch_reads_t with every span reverse-complemented
  b  one span list with a --long bp span among 10^5 short ones (the tiling of the output space)
  c  get_reads_by_kmer_batch of --kmers stored k-mers of an index built here through the project's tools (--work), against
     [get_reads_by_kmer(s) for s in kmers] on the first --host-kmers of them in the same process (that loop is the code of the parent commit:
     the single-item methods did not change)
Times are host clocks around calls that end in a device synchronise (each call is a sizing pass plus a filling pass and allocates its
outputs); median and range of --reps repetitions after --warmup."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, warmup, reps):
    import torch
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    ts.sort()
    return {"median_ms": 1e3 * ts[len(ts) // 2], "min_ms": 1e3 * ts[0], "max_ms": 1e3 * ts[-1], "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="abc")
    ap.add_argument("--reads", type=int, default=5_000_000)
    ap.add_argument("--n1", type=int, default=1_000_000)
    ap.add_argument("--n2", type=int, default=10_000_000)
    ap.add_argument("--long", type=int, default=100_000_000)
    ap.add_argument("--kmers", type=int, default=100_000)
    ap.add_argument("--host-kmers", type=int, default=10_000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--work", default="/tmp/aix_reads_fetch")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "readsquery", "readsquery.json"))
    a = ap.parse_args()
    import ctypes as C
    import torch
    from aindex_amd import _lib, engine, tools
    from aindex_amd.engine import Index
    L, vp = _lib.lib(), _lib.vp
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    os.makedirs(a.work, exist_ok=True)
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    emit({"leg": "machine", "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "library": L.aix_version().decode()})
    gold = os.path.join(ROOT, "tests", "golden", "small23", "small23")

    def ceilings(nbytes):
        """Streaming: a device-to-device copy of nbytes. Random-line: nbytes / 16 random 16-byte reads over the reads buffer's size."""
        src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        t = timed(lambda: dst.copy_(src), a.warmup, a.reps)
        copy = nbytes / (t["median_ms"] * 1e-3) / 1e9
        del src, dst
        table = torch.empty(a.reads * 151 // 16 * 16, dtype=torch.uint8, device="cuda")
        sink = torch.zeros(1 << 20, dtype=torch.int64, device="cuda")
        n_acc = nbytes // 16
        st = vp(torch.cuda.current_stream().cuda_stream)
        t = timed(lambda: _lib.check(L.aix_bench_gather_dev(vp(table.data_ptr()), table.numel() // 16, 16, 4, n_acc, 99, vp(sink.data_ptr()), st)), a.warmup, a.reps)
        gather = n_acc * 16 / (t["median_ms"] * 1e-3) / 1e9
        return copy, gather

    if "a" in a.legs or "b" in a.legs:
        g = engine.synth_genome_t(29, 8_000_000)
        reads_t = engine.synth_reads_t(43, g, a.reads, 150, rc_half=True, n_rate_ppm=500)
        starts = np.arange(a.reads, dtype=np.uint64) * np.uint64(151)
        with Index.open_23(gold + ".pf", gold + ".tf.bin", gold + ".kmers.bin") as ix:
            ix.attach_reads_t(reads_t)
            assert ix.attach_ridx(np.stack([np.arange(a.reads, dtype=np.uint64), starts, starts + np.uint64(150)], axis=1))
            if "a" in a.legs:
                for n in (a.n1, a.n2):
                    rid = torch.randint(0, a.reads, (n,), dtype=torch.int64, device="cuda", generator=torch.Generator("cuda").manual_seed(n))
                    nbytes = 150 * n
                    copy, gather = ceilings(nbytes)
                    fwd = timed(lambda: ix.fetch_reads_by_rid_t(rid), a.warmup, a.reps)
                    s_t = rid * 151
                    e_t = s_t + 150
                    rc_t = torch.ones(n, dtype=torch.uint8, device="cuda")
                    rev = timed(lambda: ix.fetch_reads_t(s_t, e_t, rc_t), a.warmup, a.reps)
                    off, by = ix.fetch_reads_by_rid_t(rid)
                    assert by.numel() == nbytes and torch.equal(by[:150], reads_t[int(rid[0]) * 151:int(rid[0]) * 151 + 150])
                    for name, t in (("forward", fwd), ("revcomp", rev)):
                        rate = nbytes / (t["median_ms"] * 1e-3) / 1e9
                        emit({"leg": "a", "form": name, "reads": n, "bytes": nbytes, **t, "gb_per_s": rate, "gb_per_s_best": nbytes / (t["min_ms"] * 1e-3) / 1e9,
                              "gb_per_s_worst": nbytes / (t["max_ms"] * 1e-3) / 1e9, "copy_gb_per_s": copy, "gather16_gb_per_s": gather,
                              "fraction_of_copy": rate / copy, "fraction_of_gather16": rate / gather})
                    del off, by, rid, s_t, e_t, rc_t
            if "b" in a.legs:
                n = 100_000
                rng = np.random.default_rng(3)
                s = (rng.integers(0, a.reads, n) * 151).astype(np.int64)
                e = s + 150
                long_len = min(a.long, reads_t.numel() - 1000)
                s[n // 2], e[n // 2] = 333, 333 + long_len
                s_t, e_t = torch.from_numpy(s).cuda(), torch.from_numpy(e).cuda()
                nbytes = int((e - s).sum())
                copy, gather = ceilings(nbytes)
                t = timed(lambda: ix.fetch_reads_t(s_t, e_t), a.warmup, a.reps)
                off, by = ix.fetch_reads_t(s_t, e_t)
                o = int(off[n // 2])
                assert by.numel() == nbytes and torch.equal(by[o:o + long_len], reads_t[333:333 + long_len])
                rate = nbytes / (t["median_ms"] * 1e-3) / 1e9
                emit({"leg": "b", "spans": n, "long_span": long_len, "bytes": nbytes, **t, "gb_per_s": rate, "gb_per_s_best": nbytes / (t["min_ms"] * 1e-3) / 1e9,
                      "gb_per_s_worst": nbytes / (t["max_ms"] * 1e-3) / 1e9, "copy_gb_per_s": copy, "gather16_gb_per_s": gather, "fraction_of_copy": rate / copy})
                del off, by
        del reads_t
        torch.cuda.empty_cache()

    if "c" in a.legs:
        from aindex_amd import synth
        from aindex_amd.aindex import AIndex
        genome = bytes(synth.genome_ascii(77, 600_000))
        rng = np.random.default_rng(9)
        at = rng.integers(0, len(genome) - 150, 120_000)
        reads = [genome[int(p):int(p) + 150] for p in at]
        cwd = os.getcwd()
        os.chdir(a.work)
        try:
            open("c.reads", "wb").write(b"".join(r + b"\n" for r in reads))
            open("c.fa", "wb").write(b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(reads)))
            assert tools.main(["kmer_counter", "c.fa", "23", "c.dat"]) == 0
            open("keys.txt", "w").write("".join(r.split("\t")[0] + "\n" for r in open("c.dat").read().split("\n") if r))
            assert tools.main(["compute_mphf_seq", "keys.txt", "c.pf"]) == 0
            assert tools.main(["compute_index", "c.dat", "c.pf", "c", "4", "0"]) == 0
            assert tools.main(["compute_reads", "c.reads", "-", "reads", "c"]) == 0
            assert tools.main(["compute_aindex", "c.reads", "c.pf", "c", "4", "23", "c.tf.bin", "c.kmers.bin", "keys.txt"]) == 0
        finally:
            os.chdir(cwd)
        prefix = os.path.join(a.work, "c")
        ai = AIndex.load_from_prefix(prefix)
        ai.load_aindex(prefix + ".index.bin", prefix + ".indices.bin", 100)
        ai.load_reads(prefix + ".reads")
        pick = rng.integers(0, ai.n_kmers, a.kmers)
        kmers = [ai.get_kmer_by_kid(int(i)) for i in pick]
        ai.get_reads_by_kmer_batch(kmers[:100])                              # uploads
        t = timed(lambda: ai.get_reads_by_kmer_batch(kmers, 100), 1, max(3, a.reps // 2))
        got = ai.get_reads_by_kmer_batch(kmers, 100)
        t0 = time.perf_counter()
        host = [ai.get_reads_by_kmer(s, 100) for s in kmers[:a.host_kmers]]
        host_s = time.perf_counter() - t0
        assert got[:a.host_kmers] == host
        emit({"leg": "c", "kmers": a.kmers, "reads_returned": sum(map(len, got)), **t, "kmers_per_s": a.kmers / (t["median_ms"] * 1e-3),
              "host_loop_kmers": a.host_kmers, "host_loop_s": host_s, "host_loop_kmers_per_s": a.host_kmers / host_s,
              "speedup": (a.kmers / (t["median_ms"] * 1e-3)) / (a.host_kmers / host_s)})
        ai._wrapper.close()

    with open(a.out, "w") as fh:
        for d in lines:
            fh.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
