"""Batch position queries on the MI355X: time of Index.positions_batch_t (device-resident CSR) on an evenly loaded and on a skewed
query set of equal output size, the host array surface and the list surface. One JSON line per leg on stdout and in --out.

The index is built on the device from synthetic reads (seeded): --reads reads of 150 bases over a --genome bp genome plus 10^5 copies of
one extra read whose 128 23-mers are the heavy ones. Every leg uses the same index and writes its query set once (--work/queries_*.npy).
Times are host clocks around calls that end in a device synchronise; median and range of --reps repetitions after --warmup.
Baselines (never the code under test), each in a fresh child process on the same index files (--work) and the same 10^4 present k-mers:
--parent-tree DIR: [ai.get_positions(s) for s in kmers] with the aindex_amd package of a checkout of the parent commit (built there);
oracle/_ref: the compiled reference's aindex_cpp.AindexWrapper.get_positions loop on one core. A baseline whose tree / module is not
there is reported as not run. Roofline: the bytes that must move over the rate of the library's own random-read probe (16-byte reads
over a 4 GiB table, the probe behind bench.py --full's random_read leg), measured in the same process."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEAVY_COPIES = 100_000


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


def child_loop(kind, tree, prefix, kmers_path):
    """One baseline in this (fresh) process: load the index files, time the per-k-mer loop, print one JSON line."""
    kmers = [bytes(r).decode() for r in np.load(kmers_path)]
    if kind == "parent":
        sys.path.insert(0, tree)                      # the parent checkout's package, before this tree's
        from aindex_amd.aindex import AIndex
        import aindex_amd
        assert os.path.realpath(os.path.dirname(os.path.dirname(aindex_amd.__file__))) == os.path.realpath(tree)
        ai = AIndex.load_from_prefix(prefix)
        ai.load_aindex(prefix + ".index.bin", prefix + ".indices.bin", 0)
        get = ai.get_positions
    else:
        sys.path.insert(0, tree)
        import aindex_cpp
        w = aindex_cpp.AindexWrapper()
        so = os.dup(1)
        os.dup2(os.open(os.devnull, os.O_WRONLY), 1)  # the reference logs to stdout
        try:
            w.load_from_prefix_23mer(prefix)
            w.load_aindex_from_prefix_23mer(prefix, 0, prefix + ".reads")
        finally:
            os.dup2(so, 1)
        get = w.get_positions
    for s in kmers[:200]:
        get(s)
    ts = []
    for _ in range(3):
        t = time.perf_counter()
        got = [get(s) for s in kmers]
        ts.append(time.perf_counter() - t)
    ts.sort()
    print(json.dumps({"kmers": len(kmers), "entries": sum(map(len, got)), "median_ms": 1e3 * ts[1], "min_ms": 1e3 * ts[0], "max_ms": 1e3 * ts[2], "reps": 3,
                      "first_lists": [p[:4] for p in got[:3]]}), flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child_loop(*sys.argv[2:6])
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-baselines", action="store_true", help="GPU legs only (e.g. under a kernel trace)")
    ap.add_argument("--parent-tree", default="", help="a built checkout of the parent commit for the per-k-mer loop baseline")
    ap.add_argument("--reads", type=int, default=5_000_000)
    ap.add_argument("--genome", type=int, default=20_000_000)
    ap.add_argument("--queries", type=int, default=1_000_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posquery"), help="directory of posquery.json")
    ap.add_argument("--work", default=os.path.join(ROOT, "build", "posquery"), help="directory of the query sets (tens of MB, not for git)")
    a = ap.parse_args()
    import torch
    from aindex_amd import _lib, builder, counting, engine, synth
    from aindex_amd.engine import Index
    from aindex_amd.wrapper import AindexWrapper
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: no timing is taken without one")
    os.makedirs(a.out, exist_ok=True)
    os.makedirs(a.work, exist_ok=True)
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)

    g = engine.synth_genome_t(29, a.genome)
    heavy_read = np.concatenate([synth.genome_ascii(1234, 150), np.frombuffer(b"\n", dtype=np.uint8)])
    reads_t = torch.cat([engine.synth_reads_t(43, g, a.reads, 150, rc_half=True), torch.from_numpy(np.tile(heavy_read, HEAVY_COPIES)).cuda()])
    keys, counts = counting.count_distinct_t(reads_t, 23, _lib.CANON_TRUE_RC)
    pf = builder.build_pf_codes_t(keys, 23)
    ix = Index.build_23_codes_t(pf, keys, counts.to(torch.int32))
    ind_t, pos_t = ix.positions_fill_t(reads_t)
    ix.attach_aindex_t(ind_t, pos_t)
    n_reads = reads_t.numel() // 151
    starts = np.arange(n_reads, dtype=np.uint64) * np.uint64(151)
    assert ix.attach_ridx(np.stack([np.arange(n_reads, dtype=np.uint64), starts, starts + np.uint64(150)], axis=1))
    torch.cuda.synchronize()
    keys_h = keys.cpu().numpy().view(np.uint64)
    counts_h = counts.cpu().numpy()
    emit({"leg": "index", "reads": n_reads, "keys": int(keys_h.shape[0]), "positions_entries": int(pos_t.numel()), "info": {k: v for k, v in ix.info.items() if "aindex" in k or "ridx" in k}})

    n = a.queries
    light = keys_h[counts_h < 1000]
    pick = (synth.sm64(5, np.arange(n, dtype=np.uint64)) % np.uint64(light.shape[0])).astype(np.int64)
    even = synth.decode_kmers(light[pick], 23)
    hw = np.lib.stride_tricks.sliding_window_view(heavy_read[:150], 23)
    sets = {"even": even}

    def run(name, q, locate=False):
        qt = torch.from_numpy(np.ascontiguousarray(q).reshape(-1)).cuda()
        out = ix.positions_batch_t(qt, locate=locate)
        torch.cuda.synchronize()
        off = out[0].cpu().numpy()
        entries, lens = int(off[-1]), np.diff(off)
        t = timed(lambda: ix.positions_batch_t(qt, locate=locate), a.warmup, a.reps)
        must = 23 * q.shape[0] + 128 * q.shape[0] + 16 * q.shape[0] + 8 * entries + (24 if locate else 8) * entries
        d = {"leg": name, "queries": int(q.shape[0]), "entries": entries, "longest_list": int(lens.max()), "median_list": float(np.median(lens[lens > 0])),
             "locate": locate, **t, "bytes_that_must_move": must, "GB_per_s_of_those_at_median": must / t["median_ms"] / 1e6,
             "entries_per_s_at_median": entries / t["median_ms"] * 1e3, "note": "one call = sizing call + filling call (three walks of the flat space)"}
        emit(d)
        return d

    e = run("even", even)
    # skewed: the same number of queries and (to within one heavy list) of entries, nine tenths of them in heavy lists
    n_heavy = max(1, int(0.9 * e["entries"]) // HEAVY_COPIES)
    rest = e["entries"] - n_heavy * HEAVY_COPIES
    mean_light = e["entries"] / n
    n_light = min(n - n_heavy, int(rest / mean_light))
    skew = np.concatenate([hw[np.arange(n_heavy) % hw.shape[0]], even[:n_light], synth.random_kmers_ascii(7, n - n_heavy - n_light, 23)])
    skew = skew[np.random.default_rng(3).permutation(n)]
    sets["skewed"] = skew
    s = run("skewed", skew)
    emit({"leg": "skewed_over_even", "entries_ratio": s["entries"] / e["entries"], "time_ratio_median": s["median_ms"] / e["median_ms"],
          "time_ratio_range": [s["min_ms"] / e["max_ms"], s["max_ms"] / e["min_ms"]]})
    run("even_locate", even, locate=True)
    run("skewed_locate", skew, locate=True)
    for k, v in sets.items():
        np.save(os.path.join(a.work, f"queries_{k}.npy"), v)
    # host surfaces: numpy CSR through aix_positions_query (upload, two passes, download), then Python lists built from it
    sub = np.ascontiguousarray(even[:100_000]).reshape(-1)
    t = timed(lambda: ix.positions_batch(sub), 1, 5)
    off, pos = ix.positions_batch(sub)
    emit({"leg": "host_array_surface", "queries": 100_000, "entries": int(off[-1]), **t})
    keep = np.arange(100_000)
    t0 = time.perf_counter()
    lists = AindexWrapper._spread_lists(100_000, keep, off, pos)
    dt = time.perf_counter() - t0
    emit({"leg": "list_surface_object_construction", "queries": 100_000, "entries": int(off[-1]), "ms": 1e3 * dt, "lists": len(lists),
          "note": "what get_positions_batch adds on top of the array surface: list[list[int]] objects"})
    # roofline: the library's random-read probe on this device, in this process
    from aindex_amd._lib import check, lib, vp
    nel = 4096 * (1 << 20) // 16
    table = torch.empty(nel * 2, dtype=torch.int64, device="cuda")
    table.random_(0, 1 << 40)
    sink = torch.zeros(8, dtype=torch.int64, device="cuda")
    acc = 200_000_000
    probe = lambda: check(lib().aix_bench_gather_dev(vp(table.data_ptr()), nel, 16, 1, acc, 99, vp(sink.data_ptr()), vp(torch.cuda.current_stream().cuda_stream)))
    tp = timed(probe, 1, 5)
    del table
    rate = acc * 16 / (tp["median_ms"] * 1e-3)
    emit({"leg": "roofline", "probe": "aix_bench_gather_dev: 2e8 uniform-random 16-byte reads over a 4 GiB table", **tp, "accesses_per_s": acc / (tp["median_ms"] * 1e-3),
          "bytes_per_s": rate, "fraction_of_it": {d["leg"]: d["bytes_that_must_move"] / rate / (d["median_ms"] * 1e-3) for d in lines if "bytes_that_must_move" in d},
          "note": "fraction = (bytes that must move / probe rate) / median time of the whole call; above 1 means the call moves its bytes faster than 16-byte random reads would"})
    if a.skip_baselines:
        json.dump(lines, open(os.path.join(a.out, "posquery.json"), "w"), indent=1)
        ix.close()
        return
    # baselines in fresh child processes, on the index written to disk once
    import subprocess
    prefix = os.path.join(a.work, "posq")
    open(prefix + ".pf", "wb").write(pf)
    ix.tf_array().tofile(prefix + ".tf.bin")
    ix.checker_array().tofile(prefix + ".kmers.bin")
    ind_t.cpu().numpy().tofile(prefix + ".indices.bin")
    pos_t.cpu().numpy().tofile(prefix + ".index.bin")
    reads_t.cpu().numpy().tofile(prefix + ".reads")
    with open(prefix + ".ridx", "w") as f:
        f.write("".join(f"{i}\t{151 * i}\t{151 * i + 150}\n" for i in range(n_reads)))
    kp = os.path.join(a.work, "queries_baseline.npy")
    np.save(kp, even[:10_000])
    want = ix.positions_batch(np.ascontiguousarray(even[:10_000]).reshape(-1))
    for kind, tree in (("parent", a.parent_tree), ("reference", os.path.join(ROOT, "oracle", "_ref"))):
        name = "baseline_per_kmer_loop_parent_commit" if kind == "parent" else "baseline_reference_aindex_cpp_loop_1_core"
        if not tree or not os.path.isdir(tree):
            emit({"leg": name, "status": "not run: " + (tree or "--parent-tree") + " is not there"})
            continue
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, tree, prefix, kp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        last = r.stdout.decode().strip().split("\n")[-1] if r.stdout.strip() else ""
        if r.returncode != 0 or not last.startswith("{"):
            emit({"leg": name, "status": f"failed rc={r.returncode}", "stderr_tail": r.stderr.decode()[-400:]})
            continue
        d = json.loads(last)
        d["same_answers_as_batch"] = d["entries"] == int(want[0][-1]) and d.pop("first_lists") == [want[1][int(want[0][i]):int(want[0][i + 1])][:4].tolist() for i in range(3)]
        emit({"leg": name, "status": "ok", **d, "us_per_kmer_at_median": d["median_ms"] * 1e3 / d["kmers"]})
    json.dump(lines, open(os.path.join(a.out, "posquery.json"), "w"), indent=1)
    ix.close()


if __name__ == "__main__":
    main()
