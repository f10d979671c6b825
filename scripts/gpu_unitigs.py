"""De Bruijn compaction on the MI355X: Index.unitigs_layout_t / unitigs_t on the two indexes of scripts/gpu_debruijn.py.

  python scripts/gpu_unitigs.py [--genome 50000000] [--out profiles/unitigs]

The driver starts one child process per step, each under its own time limit, and stops at the first that fails:
  unitigs   layout and emit, timed separately as whole calls, on the clean index (the distinct 23-mers of the genome: essentially one
            unitig, the deepest ranking) and on the index of reads with 0.5 % substitutions (many short unitigs); in the same process
            neighbours_t(all stored codes, "both") on the same handle — 8 probes per key, as the ports pass makes — and the library's
            16-byte random-read probe; U, the histogram of unitig lengths, n_circular, the scratch the chain asks for
  baseline  the only earlier route, in a process of its own: walk_t(mode="unitig") in both directions from --seeds stored k-mers of each
            index (bounded by --steps; it visits a unitig once per member and direction and cannot deliver the compaction)
`--child trace [--only <index>]` makes one layout and one emit call on each index, or on the one named (the program to put behind
`rocprofv3 --kernel-trace --stats --`): the per-kernel totals give the ports pass, the number of jumping rounds (calls of k_ug_jump) and
the time of a round, the sorts and the emit; `--phases <kernel_trace.csv>` digests such a trace.
Times are host clocks around calls that end in a device synchronise: median and range of --reps runs after --warmup."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gpu_debruijn as GD  # noqa: E402  (the seeded indexes and the timer of the De Bruijn measurements)


def scratch_bytes(n, u, n_live, cyclic):
    """what ug_layout / ug_emit of aix_unitigs.hip allocate at their peaks, from their allocation lists"""
    rank = 4 * 2 * n + 2 * 8 * 2 * n                                # port words + two ranking buffers
    cyc = 4 * 2 * n + 8 * 2 * n + 4 * 8 * 2 * n if cyclic else 0    # port words + the final ranking buffer + four cycle buffers
    place = 8 * 2 * n + (2 * 8 * 2 * n if cyclic else 0) + 12 * n + 12 * u
    emit = max(2 * 12 * n, 12 * n + 4 * n_live + 32 * u)             # the sort's two key / kid buffers; then one of them, tf and the reduce-by-key records
    return {"layout_peak": max(rank, cyc, place), "emit_peak_without_rocprim_temporaries": emit}


def phases(trace_csv):
    """A rocprofv3 kernel trace (`*_kernel_trace.csv` of a `--child trace` run) from the first k_ug_ports on, in launch order: the k_ug_*
    kernels by name, every other kernel (rocPRIM's) under the k_ug_* kernel that precedes it; the time of every jumping round."""
    import csv
    rows = sorted(csv.DictReader(open(trace_csv)), key=lambda r: int(r["Start_Timestamp"]))
    first = next(i for i, r in enumerate(rows) if "k_ug_ports" in r["Kernel_Name"])
    after = {"place": "rocPRIM radix sort of the starts", "keys": "rocPRIM radix sort of the nodes", "emit": "rocPRIM reduce_by_key"}
    phase, acc, rounds = None, {}, []
    for r in rows[first:]:
        ms = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        if "k_ug_" in r["Kernel_Name"]:
            phase = r["Kernel_Name"].split("k_ug_")[1].split("(")[0]
            key = "k_ug_" + phase
            if phase == "jump":
                rounds.append(round(ms, 3))
        else:
            key = after.get(phase, f"other after k_ug_{phase}")
        a = acc.setdefault(key, {"kernel": key, "launches": 0, "total_ms": 0.0, "max_ms": 0.0})
        a["launches"] += 1
        a["total_ms"] = round(a["total_ms"] + ms, 3)
        a["max_ms"] = round(max(a["max_ms"], ms), 3)
    return {"kernels": list(acc.values()), "jump_rounds_ms": rounds}


def child(kind, a):
    import torch
    sys.path.insert(0, ROOT)
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)
        json.dump(lines, open(os.path.join(a.work, f"{kind}.json"), "w"), indent=1)

    idx = GD.build_indexes(a, clean_only=(kind == "trace" and a.only == "clean"))
    emit({"leg": "indexes", **{k: int(v[0].n) for k, v in idx.items()}})
    for name, (ix, _) in idx.items():
        if kind == "trace":
            if a.only in ("", name):
                ix.unitigs_t(0, want_kmer_tf=True)
            continue
        codes = torch.from_numpy(ix.checker_array().view(np.int64)).cuda() & GD.MASK46
        if kind == "baseline":
            gen = torch.Generator(device="cuda")
            gen.manual_seed(17)
            seeds = codes[torch.randint(0, codes.numel(), (a.seeds,), device="cuda", generator=gen)]
            t = GD.timed(lambda: [ix.walk_t(seeds, a.steps, d, 0, "unitig", want_tf=False) for d in ("next", "prev")], a.warmup, a.reps)
            emit({"leg": f"walk_unitig_both_directions_{name}", "seeds": a.seeds, "max_steps": a.steps, **t,
                  "extrapolated_to_every_stored_kmer_ms": t["median_ms"] * ix.n / a.seeds})
            continue
        layout = ix.unitigs_layout_t(0)
        ku, kp, kf, U, total, live, circ = layout
        tl = GD.timed(lambda: ix.unitigs_layout_t(0), a.warmup, a.reps)
        te = GD.timed(lambda: ix.unitigs_t(0, want_kmer_tf=True, layout=layout), a.warmup, a.reps)
        tn = GD.timed(lambda: ix.neighbours_t(codes, "both"), a.warmup, a.reps)
        u = ix.unitigs_t(0, layout=layout)
        m = (u["offsets"][1:] - u["offsets"][:-1] - 22)
        hist = torch.bincount(torch.floor(torch.log2(m.to(torch.float64))).to(torch.int64), minlength=1).tolist()
        emit({"leg": f"unitigs_{name}", "keys": int(ix.n), "U": U, "n_live": live, "n_circular": circ, "total_bases": total, "longest": int(m.max()),
              "layout": tl, "emit_with_kmer_tf": te, "neighbours_t_all_stored_codes_both": tn,
              "length_histogram_log2_buckets": hist, "scratch_bytes": scratch_bytes(int(ix.n), U, live, circ > 0)})
        del codes, u, layout, ku, kp, kf
    if kind == "unitigs":
        from aindex_amd._lib import check, lib, vp
        nel = 4096 * (1 << 20) // 16
        table = torch.empty(nel * 2, dtype=torch.int64, device="cuda")
        table.random_(0, 1 << 40)
        sink = torch.zeros(8, dtype=torch.int64, device="cuda")
        acc = 200_000_000
        for width in (16, 8):
            tp = GD.timed(lambda: check(lib().aix_bench_gather_dev(vp(table.data_ptr()), nel * 16 // width, width, 1, acc, 99, vp(sink.data_ptr()),
                                                                   vp(torch.cuda.current_stream().cuda_stream))), 1, 5)
            emit({"leg": f"random_read_{width}B", "probe": f"aix_bench_gather_dev: 2e8 uniform-random {width}-byte reads over a 4 GiB table", **tp,
                  "accesses_per_s": acc / tp["median_ms"] * 1e3})
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default="")
    ap.add_argument("--only", default="", help="--child trace: the one index to run (clean, reads_0.5pct_substitutions); default both")
    ap.add_argument("--genome", type=int, default=50_000_000)
    ap.add_argument("--genome-reads", type=int, default=20_000_000, help="leading part of the genome the reads with substitutions cover (6 x)")
    ap.add_argument("--seeds", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--limit", type=int, default=540, help="seconds a child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unitigs"))
    ap.add_argument("--work", default=os.path.join(ROOT, "build", "unitigs"), help="scratch directory of the children's result files")
    ap.add_argument("--phases", default="", help="a *_kernel_trace.csv of a --child trace run: print its per-phase digest and stop")
    a = ap.parse_args()
    if a.phases:
        print(json.dumps(phases(a.phases), indent=1))
        return
    os.makedirs(a.work, exist_ok=True)
    if a.child:
        return child(a.child, a)
    os.makedirs(a.out, exist_ok=True)
    out = {}
    for kind in ("unitigs", "baseline"):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", kind] + sys.argv[1:]
        r = subprocess.run(cmd)
        if r.returncode != 0:
            raise SystemExit(f"{kind} ended with status {r.returncode}: nothing more is started")
        out[kind] = json.load(open(os.path.join(a.work, f"{kind}.json")))
        json.dump(out, open(os.path.join(a.out, "unitigs.json"), "w"), indent=1)
    print(json.dumps(out["unitigs"][1:3]))


if __name__ == "__main__":
    main()
