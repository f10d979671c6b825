"""k-mers by frequency on the MI355X: values, spectrum, top-N and threshold selection of aix_spectrum.hip against the same calls of the parent commit.

  python scripts/gpu_spectrum.py --parent-tree <built checkout of the parent commit> [--genome 50000000] [--out profiles/spectrum]

The driver starts one child process per step, each under its own time limit, and stops at the first that fails:
  device    this tree. 23-mer index of the genome's own 23-mers (config 3 of bench.py: synth_genome_t(23, --genome)) and a 13-mer table that count13_t
            makes of --reads13 reads; both are written as index files and loaded through AIndex.load_from_prefix. Legs: values, spectrum,
            top-100, top-10^6, all >= 1 (engine level, no strings), get_kmer_frequency_stats() and get_top_kmers(100) end to end; on the 13-mer
            table the array level over the tensor count13_t leaves in HBM as well. In the same process: tf_codes_t on the n codes of the
            checker (the all-hit lookup the values pass is held against), each streaming pass on its own, and a device-to-device copy of 1 GiB.
  baseline  the package of --parent-tree (never the code under test): the same public calls, and for the engine-level legs what the parent's
            iter_kmers_by_frequency computes before it yields (AIndex._frequencies: checker download, numpy decode, one batch lookup; then
            the stable argsort and the cut), restated here line by line.
Both children build the same seeded files and write a SHA-256 of every answer; the driver asserts that they are equal, that the slowest timed
call of this tree is faster than the fastest of the parent, and writes spectrum.json. Times are host clocks around calls that end in a device
synchronise: median and range of --reps runs after --warmup. A leg that was not run is reported as not run."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK46 = (1 << 46) - 1
TOPS = (("top_100", 100), ("top_1e6", 1_000_000), ("all_ge_1", 0))


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


def sha(*arrays):
    h = hashlib.sha256()
    for x in arrays:
        h.update(x.encode() if isinstance(x, str) else np.ascontiguousarray(x).tobytes())
    return h.hexdigest()


def u32(x):
    return np.asarray(x).astype(np.uint64).astype(np.uint32)


# ---- the seeded inputs, identical in both children: index files under --work/<kind> -----------------------------------------
def write_indexes(a, d):
    import torch
    from aindex_amd import _lib, builder, counting, engine
    from aindex_amd.engine import Index
    os.makedirs(d, exist_ok=True)
    g = engine.synth_genome_t(23, a.genome)
    keys, counts = counting.count_distinct_t(g, 23, _lib.CANON_TRUE_RC)
    pf = builder.build_pf_codes_t(keys, 23)
    p23 = os.path.join(d, "g23")
    with Index.build_23_codes_t(pf, keys, counts.to(torch.int32)) as ix:
        open(p23 + ".pf", "wb").write(pf if isinstance(pf, (bytes, bytearray)) else pf.cpu().numpy().tobytes())
        ix.checker_array().tofile(p23 + ".kmers.bin")
        ix.tf_array().tofile(p23 + ".tf.bin")
    del keys, counts, g
    p13 = os.path.join(d, "g13")
    pf13 = builder.all_13mers_pf_path()
    if not os.path.exists(p13 + ".pf"):
        os.symlink(pf13, p13 + ".pf")
    g13 = engine.synth_genome_t(13, 4_000_000)
    with Index.open_13(pf13, None) as ix:
        ct = ix.count13_t(engine.synth_reads_t(14, g13, a.reads13, 150, n_rate_ppm=1000))
        ct.cpu().numpy().view(np.uint64).tofile(p13 + ".tf.bin")
    torch.cuda.empty_cache()
    return p23, p13, ct


def parent_frequencies(ai, kt):
    """(tf uint64[n]) as the parent's iter_kmers_by_frequency has it before it sorts"""
    return ai._frequencies(kt)[1]


def parent_select(tf, min_tf, max_kmers):
    keep = np.nonzero(tf >= np.uint64(max(min_tf, 0)))[0]
    order = keep[np.argsort(-tf[keep].astype(np.int64), kind="stable")]       # descending tf, ties in enumeration order
    if max_kmers:
        order = order[:max_kmers]
    return order, tf[order]


def child(kind, a):
    import torch
    sys.path.insert(0, a.parent_tree if kind == "baseline" else ROOT)
    import aindex_amd
    tree = os.path.realpath(os.path.dirname(os.path.dirname(aindex_amd.__file__)))
    assert tree == os.path.realpath(a.parent_tree if kind == "baseline" else ROOT), tree
    from aindex_amd import engine
    from aindex_amd.aindex import AIndex
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)
        json.dump(lines, open(os.path.join(a.work, f"{kind}.json"), "w"), indent=1)

    W, R = a.warmup, a.reps
    p23, p13, ct = write_indexes(a, os.path.join(a.work, kind))
    for table, prefix, ksz in (("index23", p23, 23), ("table13", p13, 13)):
        if table not in a.tables.split(","):
            continue
        ai = AIndex.load_from_prefix(prefix, kmer_size=ksz, load_aindex=False)
        kt = f"{ksz}mer"
        n = ai.n_kmers
        emit({"leg": f"{table}/loaded", "tree": kind, "n": int(n)})
        if kind == "device":
            ix = ai._wrapper._freq_index(kt)
            vt = ix.kmer_values_t()
            torch.cuda.synchronize()
            emit({"leg": f"{table}/values", "n": int(n), **timed(lambda: ix.kmer_values_t(out_t=vt), W, R), "sha256": sha(vt.cpu().numpy().view(np.uint32))})
            hist, _ = ix.tf_spectrum(a.nbins)
            emit({"leg": f"{table}/spectrum", "nbins": a.nbins, **timed(lambda: ix.tf_spectrum(a.nbins), W, R), "sha256": sha(hist), "head": hist[:6].tolist()})
            for leg, top in TOPS:
                kid, tf, _, total = ix.top_kmers(top, 1, want_kmers=False)
                emit({"leg": f"{table}/{leg}", "selected": int(kid.shape[0]), "total": int(total), **timed(lambda: ix.top_kmers(top, 1, want_kmers=False), W, R),
                      "sha256": sha(kid, tf)})
            # the passes on their own, over the values already in HBM (4 B per key per pass)
            emit({"leg": f"{table}/pass_spectrum_t", "bytes": 4 * int(n), **timed(lambda: engine.spectrum_t(vt, a.nbins), W, R)})
            for leg, top in TOPS:
                emit({"leg": f"{table}/pass_select_{leg}", "bytes_per_pass": 4 * int(n), **timed(lambda: engine.top_values_t(vt, top, 1), W, R)})
            kids = torch.arange(min(int(n), 1 << 24), dtype=torch.int64, device="cuda")      # the iterator's stream: kid -> k ASCII bytes
            t = timed(lambda: ix.kmers_by_kid_t(kids), W, R)
            emit({"leg": f"{table}/decode_kmers_by_kid_t", "kids": kids.numel(), **t, "bytes_written_per_s": kids.numel() * ksz / t["median_ms"] * 1e3})
            del kids
            if ksz == 23:                                          # the ceiling of the values pass: one all-hit lookup of the same n codes
                codes = torch.from_numpy((ix.checker_array() & np.uint64(MASK46)).view(np.int64)).cuda()
                emit({"leg": f"{table}/tf_codes_t_on_the_n_codes", "n": int(n), **timed(lambda: ix.tf_codes_t(codes), W, R)})
                del codes
            else:                                                  # the tensor count13_t left in HBM, array level
                ht, _ = engine.spectrum_t(ct, a.nbins)
                emit({"leg": f"{table}/counted_tensor_spectrum_t", **timed(lambda: engine.spectrum_t(ct, a.nbins), W, R), "sha256": sha(ht.cpu().numpy().view(np.uint64))})
                gi, gv, _ = engine.top_values_t(ct, 100, 1)
                emit({"leg": f"{table}/counted_tensor_top_100", **timed(lambda: engine.top_values_t(ct, 100, 1), W, R), "sha256": sha(gi.cpu().numpy().view(np.uint32), gv.cpu().numpy().view(np.uint32))})
            del vt
        else:
            tf = parent_frequencies(ai, kt)
            emit({"leg": f"{table}/values", "n": int(n), **timed(lambda: parent_frequencies(ai, kt), W, R), "sha256": sha(u32(tf))})
            spec = lambda: np.bincount(np.minimum(parent_frequencies(ai, kt), np.uint64(a.nbins - 1)).astype(np.int64), minlength=a.nbins).astype(np.uint64)
            emit({"leg": f"{table}/spectrum", "nbins": a.nbins, **timed(spec, W, R), "sha256": sha(spec())})
            for leg, top in TOPS:
                order, val = parent_select(tf, 1, top)
                emit({"leg": f"{table}/{leg}", "selected": int(order.shape[0]), **timed(lambda: parent_select(parent_frequencies(ai, kt), 1, top), W, R),
                      "sha256": sha(u32(order), u32(val))})
            if ksz == 23:
                ix = ai._wrapper._need23()
                codes = torch.from_numpy((ix.checker_array() & np.uint64(MASK46)).view(np.int64)).cuda()
                emit({"leg": f"{table}/tf_codes_t_on_the_n_codes", "n": int(n), **timed(lambda: ix.tf_codes_t(codes), W, R)})
                del codes
            else:                                                  # what a caller of the parent does with the counted tensor: download, numpy
                cv = lambda: ct.cpu().numpy().view(np.uint64) & np.uint64(0xFFFFFFFF)
                cspec = lambda: np.bincount(np.minimum(cv(), np.uint64(a.nbins - 1)).astype(np.int64), minlength=a.nbins).astype(np.uint64)
                emit({"leg": f"{table}/counted_tensor_spectrum_t", **timed(cspec, W, R), "sha256": sha(cspec())})
                o, v = parent_select(cv(), 1, 100)
                emit({"leg": f"{table}/counted_tensor_top_100", **timed(lambda: parent_select(cv(), 1, 100), W, R), "sha256": sha(u32(o), u32(v))})
            del tf
        st = ai.get_kmer_frequency_stats()
        emit({"leg": f"{table}/get_kmer_frequency_stats", **timed(lambda: ai.get_kmer_frequency_stats(), W, R), "sha256": sha(json.dumps(st, sort_keys=True)), "answer": st})
        top = ai.get_top_kmers(100)
        emit({"leg": f"{table}/get_top_kmers_100", **timed(lambda: ai.get_top_kmers(100), W, R), "sha256": sha(repr(top)), "first": list(top[0]) if top else None})
        if ksz == 13:
            s13 = ai._wrapper.get_13mer_statistics()
            emit({"leg": f"{table}/get_13mer_statistics", **timed(lambda: ai._wrapper.get_13mer_statistics(), W, R), "sha256": sha(json.dumps(s13, sort_keys=True))})
        del ai
    if kind == "device":
        src = torch.empty(1 << 28, dtype=torch.int32, device="cuda").random_(0, 1 << 20)
        dst = torch.empty_like(src)
        t = timed(lambda: dst.copy_(src), 2, 7)
        emit({"leg": "device_copy_1GiB", "bytes_read_plus_written": 2 * src.numel() * 4, **t, "bytes_per_s": 2 * src.numel() * 4 / t["median_ms"] * 1e3})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default="")
    ap.add_argument("--parent-tree", default="", help="a built checkout of the parent commit for the baseline")
    ap.add_argument("--genome", type=int, default=50_000_000)
    ap.add_argument("--reads13", type=int, default=4_000_000, help="reads of 150 bases that count13_t counts into the 13-mer table")
    ap.add_argument("--nbins", type=int, default=256)
    ap.add_argument("--tables", default="index23,table13")
    ap.add_argument("--only", default="", help="device | baseline: start this child alone; compare: start none. The comparison uses the lines kept under --out")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--limit", type=int, default=1080, help="seconds a child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectrum"))
    ap.add_argument("--work", default=os.path.join(ROOT, "build", "spectrum"), help="scratch directory of the children's index and result files")
    a = ap.parse_args()
    os.makedirs(a.work, exist_ok=True)
    if a.child:
        return child(a.child, a)
    os.makedirs(a.out, exist_ok=True)
    docs = {}
    for kind in ("device", "baseline"):
        kept = os.path.join(a.out, f"{kind}_child.json")           # a child's lines, kept so that the two children can run in separate calls
        if a.only in ("", kind) and (kind == "device" or os.path.isdir(a.parent_tree or "-")):
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", kind] + sys.argv[1:]
            r = subprocess.run(cmd)
            if r.returncode != 0:
                raise SystemExit(f"{kind} ended with status {r.returncode}: nothing more is started")
            json.dump(json.load(open(os.path.join(a.work, f"{kind}.json"))), open(kept, "w"), indent=1)
        if os.path.exists(kept):
            docs[kind] = json.load(open(kept))
    out = {"arguments": {k: v for k, v in vars(a).items() if k in ("genome", "reads13", "nbins", "warmup", "reps")}, "device": docs.get("device", "not run")}
    if "baseline" in docs and "device" in docs:
        out["baseline_parent_commit"] = docs["baseline"]
        base = {d["leg"]: d for d in docs["baseline"]}
        cmp_ = []
        for d in docs["device"]:
            bl = base.get(d["leg"])
            if bl and "sha256" in d and "sha256" in bl:
                cmp_.append({"leg": d["leg"], "same_answers": d["sha256"] == bl["sha256"], "device_ms": [d["median_ms"], d["min_ms"], d["max_ms"]],
                             "parent_ms": [bl["median_ms"], bl["min_ms"], bl["max_ms"]], "parent_over_device_median": bl["median_ms"] / d["median_ms"],
                             "slowest_device_call_beats_fastest_parent_call": d["max_ms"] < bl["min_ms"]})
        out["comparison"] = cmp_
        out["legs_not_run_on_the_parent"] = [d["leg"] for d in docs["device"] if "sha256" in d and d["leg"] not in base]
    else:
        out["baseline_parent_commit"] = "not run"
    json.dump(out, open(os.path.join(a.out, "spectrum.json"), "w"), indent=1)
    print(json.dumps(out.get("comparison", [])))
    if "comparison" in out:
        assert all(c["same_answers"] for c in out["comparison"]), [c["leg"] for c in out["comparison"] if not c["same_answers"]]
        lost = [c["leg"] for c in out["comparison"] if not c["slowest_device_call_beats_fastest_parent_call"]]
        assert not lost, "the device path's slowest call did not beat the parent's fastest: " + str(lost)


if __name__ == "__main__":
    main()
