"""De Bruijn neighbours and walks on the MI355X: Index.neighbours_t / walk_t against what a caller could compose before they existed.

  python scripts/gpu_debruijn.py --parent-tree <built checkout of the parent commit> [--genome 50000000] [--out profiles/debruijn]

The driver starts one child process per step, each under its own time limit, and stops at the first that fails:
  fused     this tree: neighbours of --kmers k-mers in BOTH directions (genome windows; uniform-random) and walks of --seeds genome windows,
            max_steps --steps, greedy and unitig, on the index of the genome's own 23-mers and on an index of reads with 0.5 %
            substitutions; each walk under the three absence-filter policies (AIX_DBJ_FILTER 0 gauge, 1 always, 2 never); the library's
            tf_codes_t on the same neighbour codes and its 16-byte random-read probe, in the same process
  baseline  the package of --parent-tree (never the code under test): the composition (tf_codes_t on the 8 N neighbour codes plus torch
            reductions) and the host-driven step loop (max_steps rounds of tf_codes_t on 4 S codes, twice that in unitig mode, plus torch
            selection)
Both children build the same seeded indexes on the device and write a SHA-256 of every answer; the driver asserts that they are equal
and writes debruijn.json. `--child trace` makes one call of each kernel on the clean index (the program to put behind
`rocprofv3 --kernel-trace --stats --`). Times are host clocks around calls that end in a device synchronise: median and range of --reps runs after
--warmup. The useful share of lane trips comes from the walks' own lengths: a wave holds 16 consecutive seeds and runs as many trips as
its longest walk needs (one more when that walk ends on a stop test)."""
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


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(t.cpu().numpy()).tobytes())
    return h.hexdigest()


# ---- torch restatement used by the baseline only ------------------------------------------------------------------------
def t_rc(x):
    """reverse complement of 46-bit codes in an int64 tensor"""
    y = x ^ MASK46                                                  # complement of the 23 bases
    for k, m in ((2, 0x3333333333333333), (4, 0x0F0F0F0F0F0F0F0F), (8, 0x00FF00FF00FF00FF), (16, 0x0000FFFF0000FFFF), (32, 0x00000000FFFFFFFF)):
        y = ((y >> k) & m) | ((y & m) << k)                         # (the mask clears what an arithmetic shift smears)
    return (y >> 18) & MASK46


def t_neigh(u, direction, b):
    return (((u << 2) | b) & MASK46) if direction == 0 else ((u >> 2) | (b << 44))


def t_cont(ix, u, direction, cutoff):
    import torch
    b = torch.arange(4, device=u.device, dtype=torch.int64)[None, :]
    nb = t_neigh(u[:, None], direction, b).reshape(-1)
    t = ix.tf_codes_t(nb).view(-1, 4).to(torch.int64) & 0xFFFFFFFF
    if cutoff > 0:
        t = torch.where(t <= cutoff, torch.zeros_like(t), t)
    n = (t != 0).sum(dim=1)
    sm = t.sum(dim=1) & 0xFFFFFFFF
    best = 3 - torch.argmax(t.flip(1), dim=1)                       # the last base that is >= the other three
    btf = t.gather(1, best[:, None])[:, 0]
    return t, n, sm, btf, best


def composed_neighbours(ix, codes, cutoff=0):
    import torch
    out = []
    for d in (0, 1):
        t, n, sm, btf, best = t_cont(ix, codes, d, cutoff)
        out.append(torch.cat([t, n[:, None], sm[:, None], btf[:, None], best[:, None]], dim=1))
    return torch.stack(out, dim=1).to(torch.int32)


def step_loop_walk(ix, seeds, direction, L, cutoff, unitig):
    import torch
    S, dev = seeds.numel(), seeds.device
    letters = torch.tensor([65, 67, 71, 84], dtype=torch.uint8, device=dev)
    bases = torch.zeros((S, L), dtype=torch.uint8, device=dev)
    length = torch.zeros(S, dtype=torch.int64, device=dev)
    stop = torch.zeros(S, dtype=torch.uint8, device=dev)
    cur = seeds.clone()
    seedc = torch.minimum(seeds, t_rc(seeds))
    alive = torch.ones(S, dtype=torch.bool, device=dev)
    rows = torch.arange(S, device=dev)
    for _ in range(L):
        _, n, _, _, best = t_cont(ix, cur, direction, cutoff)
        nxt = t_neigh(cur, direction, best)
        go = alive.clone()
        dead = go & (n == 0)
        stop[dead] = 1
        go &= ~dead
        if unitig:
            br = go & (n > 1)
            stop[br] = 2
            go &= ~br
            _, n2, _, _, _ = t_cont(ix, nxt, 1 - direction, cutoff)
            jn = go & (n2 > 1)
            stop[jn] = 3
            go &= ~jn
        lp = go & (torch.minimum(nxt, t_rc(nxt)) == seedc)
        stop[lp] = 4
        go &= ~lp
        idx = rows[go]
        bases[idx, length[idx]] = letters[best[idx]]
        length[idx] += 1
        cur = torch.where(go, nxt, cur)
        alive = go
    return bases, length.to(torch.int32), stop


# ---- the seeded inputs, identical in both children ----------------------------------------------------------------------
def build_indexes(a, clean_only=False):
    import torch
    from aindex_amd import _lib, builder, counting, engine
    from aindex_amd.engine import Index
    out = {}
    g = engine.synth_genome_t(29, a.genome)
    keys, counts = counting.count_distinct_t(g, 23, _lib.CANON_TRUE_RC)
    out["clean"] = (Index.build_23_codes_t(builder.build_pf_codes_t(keys, 23), keys, counts.to(torch.int32)), g)
    if clean_only:
        torch.cuda.synchronize()
        return out
    g2 = g[: a.genome_reads]
    reads = engine.synth_reads_t(43, g2, 6 * a.genome_reads // 150, 150, rc_half=True).view(-1, 151)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    hit = torch.rand(reads.shape, device="cuda", generator=gen) < 0.005
    hit[:, 150] = False
    lut = torch.tensor([65, 67, 71, 84], dtype=torch.uint8, device="cuda")
    code = ((reads >> 1) ^ (reads >> 2)) & 3                        # A C G T -> 0 1 2 3
    other = (code + torch.randint(1, 4, reads.shape, device="cuda", generator=gen, dtype=torch.uint8)) & 3
    reads = torch.where(hit, lut[other.long()], reads).reshape(-1).contiguous()
    keys2, counts2 = counting.count_distinct_t(reads, 23, _lib.CANON_TRUE_RC)
    out["reads_0.5pct_substitutions"] = (Index.build_23_codes_t(builder.build_pf_codes_t(keys2, 23), keys2, counts2.to(torch.int32)), g2)
    torch.cuda.synchronize()
    return out


def window_codes(g, n, seed):
    import torch
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    at = torch.randint(0, g.numel() - 23, (n,), device="cuda", generator=gen)
    w = g[at[:, None] + torch.arange(23, device="cuda")[None, :]]
    two = (((w >> 1) ^ (w >> 2)) & 3).to(torch.int64)              # A C G T -> 0 1 2 3
    sh = torch.tensor([2 * (22 - j) for j in range(23)], device="cuda", dtype=torch.int64)
    return (two << sh[None, :]).sum(dim=1)


def child(kind, a):
    import torch
    if kind == "baseline":
        sys.path.insert(0, a.parent_tree)
    else:
        sys.path.insert(0, ROOT)
    import aindex_amd
    tree = os.path.realpath(os.path.dirname(os.path.dirname(aindex_amd.__file__)))
    assert tree == os.path.realpath(a.parent_tree if kind == "baseline" else ROOT), tree
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)
        json.dump(lines, open(os.path.join(a.work, f"{kind}.json"), "w"), indent=1)

    if kind == "trace":                                            # one call of each kernel, for rocprofv3 --kernel-trace --stats -- python ... --child trace
        ix, g = build_indexes(a, clean_only=True)["clean"]
        ix.neighbours_t(window_codes(g, a.kmers, 11), "both")
        seeds = window_codes(g, a.seeds, 13)
        for mode in ("greedy", "unitig"):
            ix.walk_t(seeds, a.steps, "next", 0, mode, want_tf=False)
        torch.cuda.synchronize()
        return
    idx = build_indexes(a)
    emit({"leg": "indexes", "tree": kind, **{k: int(v[0].n) for k, v in idx.items()}})
    ix, g = idx["clean"]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    sets = {"genome_windows": window_codes(g, a.kmers, 11), "uniform_random": torch.randint(0, 1 << 46, (a.kmers,), device="cuda", generator=gen)}
    for name, codes in sets.items():
        if kind == "fused":
            got = ix.neighbours_t(codes, "both")
            t = timed(lambda: ix.neighbours_t(codes, "both"), a.warmup, a.reps)
            b = torch.arange(4, device="cuda", dtype=torch.int64)[None, None, :]
            nb = torch.stack([t_neigh(codes[:, None], 0, b[0]), t_neigh(codes[:, None], 1, b[0])], dim=1).reshape(-1)
            tl = timed(lambda: ix.tf_codes_t(nb), a.warmup, a.reps)
            emit({"leg": "neighbours_" + name, "kmers": a.kmers, "probes": 8 * a.kmers, **t, "probes_per_s": 8 * a.kmers / t["median_ms"] * 1e3,
                  "tf_codes_t_on_the_same_8N_codes": tl, "fraction_of_tf_codes_t_rate": tl["median_ms"] / t["median_ms"], "sha256": sha(got)})
        else:
            got = composed_neighbours(ix, codes)
            t = timed(lambda: composed_neighbours(ix, codes), a.warmup, a.reps)
            emit({"leg": "neighbours_" + name, "kmers": a.kmers, **t, "sha256": sha(got)})
    for iname, (ix, g) in idx.items():
        seeds = window_codes(g, a.seeds, 13)
        for mode in ("greedy", "unitig"):
            leg = f"walk_{iname}_{mode}"
            if kind == "fused":
                res = {}
                for pol in ("1", "0", "2"):
                    os.environ["AIX_DBJ_FILTER"] = pol
                    res[pol] = timed(lambda: ix.walk_t(seeds, a.steps, "next", 0, mode, want_tf=False), a.warmup, a.reps)
                os.environ.pop("AIX_DBJ_FILTER")
                t = timed(lambda: ix.walk_t(seeds, a.steps, "next", 0, mode, want_tf=False), a.warmup, a.reps)
                b, ln, st, _, _ = ix.walk_t(seeds, a.steps, "next", 0, mode, want_tf=False)
                l64 = ln.to(torch.int64)
                trips = torch.minimum(l64 + (st != 0).to(torch.int64), torch.tensor(a.steps, device="cuda"))
                pad = (-trips.numel()) % 16
                wave = torch.cat([trips, trips.new_zeros(pad)]).view(-1, 16).max(dim=1).values
                steps = int(l64.sum())
                probes = int(trips.sum()) * (8 if mode == "unitig" else 4)
                emit({"leg": leg, "seeds": a.seeds, "max_steps": a.steps, **t, "steps_taken": steps, "mean_length": steps / a.seeds,
                      "stops": torch.bincount(st.to(torch.int64), minlength=5).tolist(), "steps_per_s": steps / t["median_ms"] * 1e3,
                      "probes_per_s": probes / t["median_ms"] * 1e3, "useful_lane_trip_share": float(trips.sum()) / float(16 * wave.sum()),
                      "filter_always": res["1"], "filter_gauge": res["0"], "filter_never": res["2"], "sha256": sha(b, ln, st)})
            else:
                b, ln, st = step_loop_walk(ix, seeds, 0, a.steps, 0, mode == "unitig")
                t = timed(lambda: step_loop_walk(ix, seeds, 0, a.steps, 0, mode == "unitig"), a.warmup, a.reps)
                emit({"leg": leg, "seeds": a.seeds, "max_steps": a.steps, **t, "sha256": sha(b, ln, st)})
    if kind == "fused":
        from aindex_amd._lib import check, lib, vp
        nel = 4096 * (1 << 20) // 16
        table = torch.empty(nel * 2, dtype=torch.int64, device="cuda")
        table.random_(0, 1 << 40)
        sink = torch.zeros(8, dtype=torch.int64, device="cuda")
        acc = 200_000_000
        tp = timed(lambda: check(lib().aix_bench_gather_dev(vp(table.data_ptr()), nel, 16, 1, acc, 99, vp(sink.data_ptr()), vp(torch.cuda.current_stream().cuda_stream))), 1, 5)
        emit({"leg": "random_read", "probe": "aix_bench_gather_dev: 2e8 uniform-random 16-byte reads over a 4 GiB table", **tp, "accesses_per_s": acc / tp["median_ms"] * 1e3})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default="")
    ap.add_argument("--parent-tree", default="", help="a built checkout of the parent commit for the two baselines")
    ap.add_argument("--genome", type=int, default=50_000_000)
    ap.add_argument("--genome-reads", type=int, default=20_000_000, help="leading part of the genome the reads with substitutions cover (6 x)")
    ap.add_argument("--kmers", type=int, default=10_000_000)
    ap.add_argument("--seeds", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--limit", type=int, default=540, help="seconds a child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "debruijn"))
    ap.add_argument("--work", default=os.path.join(ROOT, "build", "debruijn"), help="scratch directory of the children's result files")
    a = ap.parse_args()
    os.makedirs(a.work, exist_ok=True)
    if a.child:
        return child(a.child, a)
    os.makedirs(a.out, exist_ok=True)
    kinds = ["fused"] + (["baseline"] if a.parent_tree and os.path.isdir(a.parent_tree) else [])
    docs = {}
    for kind in kinds:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", kind] + sys.argv[1:]
        r = subprocess.run(cmd)
        if r.returncode != 0:
            raise SystemExit(f"{kind} ended with status {r.returncode}: nothing more is started")
        docs[kind] = json.load(open(os.path.join(a.work, f"{kind}.json")))
    out = {"fused": docs["fused"]}
    if "baseline" in docs:
        out["baseline_parent_commit"] = docs["baseline"]
        base = {d["leg"]: d for d in docs["baseline"]}
        cmp_ = []
        for d in docs["fused"]:
            if d["leg"] in base and "sha256" in d:
                bl = base[d["leg"]]
                cmp_.append({"leg": d["leg"], "same_answers": d["sha256"] == bl["sha256"], "fused_median_ms": d["median_ms"], "baseline_median_ms": bl["median_ms"],
                             "baseline_over_fused": bl["median_ms"] / d["median_ms"]})
        out["comparison"] = cmp_
        json.dump(out, open(os.path.join(a.out, "debruijn.json"), "w"), indent=1)
        assert all(c["same_answers"] for c in cmp_), [c["leg"] for c in cmp_ if not c["same_answers"]]
        assert all(c["baseline_over_fused"] >= 1.0 for c in cmp_), "a fused path lost to its baseline: " + str([c["leg"] for c in cmp_ if c["baseline_over_fused"] < 1.0])
    else:
        out["baseline_parent_commit"] = "not run: --parent-tree is not there"
        json.dump(out, open(os.path.join(a.out, "debruijn.json"), "w"), indent=1)
    print(json.dumps(out.get("comparison", [])))


if __name__ == "__main__":
    main()
