"""Sequences against indexed reads on the MI355X: Index.seq_hits_t / seq_votes_t against what a caller could compose before they existed.

  python scripts/gpu_seqhits.py --parent-tree <built checkout of the parent commit> [--genome 50000000] [--out profiles/seqhits]

The driver starts one child process per step, each under its own time limit, and stops at the first that fails:
  fused     this tree: seq_hits_t and seq_votes_t (min_votes 2) of --seqs sequences of --length bases cut from the genome, half of them
            reverse-complemented, on an index of 6 x reads with 0.5 % substitutions (built on the device, positions filled and attached
            device-resident, reads and intervals attached); the library's 16-byte random-read probe in the same process
  baseline  the package of --parent-tree (never the code under test): windows packed to N x 23 on the device, positions_batch_t(...,
            locate=True), a 23-byte fetch_reads_t per hit, strand by comparison and grouping by a packed key in torch
Both children build the same seeded index and write a SHA-256 of every answer; the driver asserts that they are equal and writes
seqhits.json. `--child trace` makes one call of each entry point (the program to put behind `rocprofv3 --kernel-trace --stats --`).
Times are host clocks around calls that end in a device synchronise: median and range of --reps runs after --warmup.

The baseline is written for this index and these sizes, not as a general restatement: it sets bit 2 of every flag (every position of
an index built from whole reads lies in an interval), takes the reverse complement with a plain ACGT table (clean queries), and packs its
group key as 17 bits of sequence, 24 of read id, 1 of strand and 20 of diagonal range, guarded by asserts. With other --seqs / --length /
--genome the asserts, or the SHA-256 comparison, can fail for reasons that lie in the baseline and not in the library."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats(ts):
    order = [round(1e3 * t, 3) for t in ts]                         # in the order they were taken: an outlier shows where it fell
    ts = sorted(ts)
    return {"median_ms": 1e3 * ts[len(ts) // 2], "min_ms": 1e3 * ts[0], "max_ms": 1e3 * ts[-1], "reps": len(ts), "times_ms": order}


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
    return stats(ts)


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(t.cpu().numpy()).tobytes())
    return h.hexdigest()


def build(a):
    """the index of reads with substitutions (as scripts/gpu_debruijn.py builds it), everything attached; the queries"""
    import torch
    from aindex_amd import _lib, builder, counting, engine
    from aindex_amd.engine import Index
    g = engine.synth_genome_t(29, a.genome)
    n_reads = 6 * a.genome // 150
    reads = engine.synth_reads_t(43, g, n_reads, 150, rc_half=True).view(-1, 151)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    hit = torch.rand(reads.shape, device="cuda", generator=gen) < 0.005
    hit[:, 150] = False
    lut = torch.tensor([65, 67, 71, 84], dtype=torch.uint8, device="cuda")
    code = ((reads >> 1) ^ (reads >> 2)) & 3                        # A C G T -> 0 1 2 3
    other = (code + torch.randint(1, 4, reads.shape, device="cuda", generator=gen, dtype=torch.uint8)) & 3
    reads = torch.where(hit, lut[other.long()], reads).reshape(-1).contiguous()
    del hit, code, other
    keys, counts = counting.count_distinct_t(reads, 23, _lib.CANON_TRUE_RC)
    ix = Index.build_23_codes_t(builder.build_pf_codes_t(keys, 23), keys, counts.to(torch.int32))
    ind_t, pos_t = ix.positions_fill_t(reads)
    ix.attach_aindex_t(ind_t, pos_t)
    st = np.arange(n_reads, dtype=np.uint64) * np.uint64(151)
    assert ix.attach_ridx(np.stack([np.arange(n_reads, dtype=np.uint64), st, st + np.uint64(150)], axis=1))
    ix.attach_reads_t(reads)
    at = torch.randint(0, a.genome - a.length, (a.seqs,), device="cuda", generator=gen)
    q = g[at[:, None] + torch.arange(a.length, device="cuda")[None, :]]
    comp = torch.zeros(256, dtype=torch.uint8, device="cuda")
    comp[torch.tensor([65, 67, 71, 84], device="cuda")] = torch.tensor([84, 71, 67, 65], dtype=torch.uint8, device="cuda")
    rc = comp[q.long()].flip(1)
    q = torch.where((torch.arange(a.seqs, device="cuda") % 2 == 1)[:, None], rc, q).reshape(-1).contiguous()
    offs = torch.arange(a.seqs + 1, device="cuda", dtype=torch.int64) * a.length
    torch.cuda.synchronize()
    return ix, q, offs, comp, (ind_t, pos_t, reads, g)


def composed(ix, q, offs, comp, a, marks):
    """The parent commit's composition. marks gets the host clock after the positions-and-strand part."""
    import torch
    M, L = a.seqs, a.length
    nwin = L - 22
    starts = (offs[:-1, None] + torch.arange(nwin, device="cuda")[None, :]).reshape(-1)
    win = q[starts[:, None] + torch.arange(23, device="cuda")[None, :]].contiguous()            # N x 23
    koff, pos, rid, local = ix.positions_batch_t(win.reshape(-1), 0, locate=True)
    cnt = koff[1:] - koff[:-1]
    widx = torch.repeat_interleave(torch.arange(M * nwin, device="cuda"), cnt)
    qoff = (widx % nwin).to(torch.int32)
    ob, by = ix.fetch_reads_t(pos, pos + 23)
    assert by.numel() == 23 * pos.numel()
    by = by.view(-1, 23)
    rcwin = comp[win.long()].flip(1)                                # per window, not per hit
    s0 = (by == win[widx]).all(dim=1)
    s1 = (by == rcwin[widx]).all(dim=1)
    strand = torch.where(s0, 0, torch.where(s1, 1, 2)).to(torch.uint8)
    flag = strand | 4                                               # every position of this index lies in a read
    seq_off = koff[torch.arange(M + 1, device="cuda") * nwin]
    torch.cuda.synchronize()
    marks.append(time.perf_counter())
    hits = (seq_off, qoff, pos, rid, local, flag)
    keep = strand < 2
    seq = (widx // nwin)[keep]
    k_rid, k_st, k_q = rid[keep], strand[keep].to(torch.int64), qoff[keep].to(torch.int64)
    diag = torch.where(k_st == 0, local[keep] - k_q, local[keep] + k_q)
    db = int(diag.min())
    key = (((seq << 24 | k_rid) << 1 | k_st) << 20) | (diag - db)   # seqs < 2^17, reads < 2^24, diagonal range < 2^20
    assert a.seqs < (1 << 17) and int(k_rid.max()) < (1 << 24) and int(diag.max()) - db < (1 << 20)
    key, order = torch.sort(key, stable=True)
    uniq, counts = torch.unique_consecutive(key, return_counts=True)
    ends = torch.cumsum(counts, 0)
    first = ends - counts
    ok = counts >= a.min_votes
    qs = k_q[order]
    first, last, uniq, counts = first[ok], (ends - 1)[ok], uniq[ok], counts[ok]
    v_seq = uniq >> 45
    voff = torch.searchsorted(v_seq, torch.arange(M + 1, device="cuda"))
    votes = (voff, (uniq >> 21) & 0xFFFFFF, ((uniq >> 20) & 1).to(torch.uint8), (uniq & 0xFFFFF) + db, counts.to(torch.int32), qs[first].to(torch.int32),
             qs[last].to(torch.int32))
    torch.cuda.synchronize()
    return hits, votes


def child(kind, a):
    import torch
    sys.path.insert(0, a.parent_tree if kind == "baseline" else ROOT)
    import aindex_amd
    tree = os.path.realpath(os.path.dirname(os.path.dirname(aindex_amd.__file__)))
    assert tree == os.path.realpath(a.parent_tree if kind == "baseline" else ROOT), tree
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)
        json.dump(lines, open(os.path.join(a.work, f"{kind}.json"), "w"), indent=1)

    ix, q, offs, comp, keep = build(a)
    windows = a.seqs * (a.length - 22)
    if kind == "trace":
        ix.seq_hits_t(q, offs)
        ix.seq_votes_t(q, offs, min_votes=a.min_votes)
        torch.cuda.synchronize()
        return
    emit({"leg": "index", "tree": kind, "keys": int(ix.n), "positions": int(keep[1].numel()), "reads_bytes": int(keep[2].numel()), "windows": windows})
    if kind == "fused":
        h = ix.seq_hits_t(q, offs)
        v = ix.seq_votes_t(q, offs, min_votes=a.min_votes)
        T, R = h[1].numel(), v[1].numel()
        th = timed(lambda: ix.seq_hits_t(q, offs, cap_hint=T), a.warmup, a.reps)
        tv = timed(lambda: ix.seq_votes_t(q, offs, min_votes=a.min_votes, cap_hint=R), a.warmup, a.reps)
        th2 = timed(lambda: ix.seq_hits_t(q, offs), 0, 3)
        fl = h[5]
        emit({"leg": "hits", **th, "hits": T, "windows": windows, "hits_per_s": T / th["median_ms"] * 1e3, "windows_per_s": windows / th["median_ms"] * 1e3,
              "sized_then_filled": th2, "strand_counts": torch.bincount((fl & 3).to(torch.int64), minlength=3).tolist(), "sha256": sha(*h)})
        emit({"leg": "votes", **tv, "records": R, "hits_per_s": T / tv["median_ms"] * 1e3, "windows_per_s": windows / tv["median_ms"] * 1e3,
              "largest_group": int(v[4].max()) if R else 0, "sha256": sha(*v)})
        from aindex_amd._lib import check, lib, vp
        del h, v
        nel = 4096 * (1 << 20) // 16
        table = torch.empty(nel * 2, dtype=torch.int64, device="cuda")
        table.random_(0, 1 << 40)
        sink = torch.zeros(8, dtype=torch.int64, device="cuda")
        acc = 200_000_000
        tp = timed(lambda: check(lib().aix_bench_gather_dev(vp(table.data_ptr()), nel, 16, 1, acc, 99, vp(sink.data_ptr()), vp(torch.cuda.current_stream().cuda_stream))), 1, 5)
        emit({"leg": "random_read", "probe": "aix_bench_gather_dev: 2e8 uniform-random 16-byte reads over a 4 GiB table", **tp, "accesses_per_s": acc / tp["median_ms"] * 1e3})
    else:
        marks = []
        h, v = composed(ix, q, offs, comp, a, marks)
        sh, sv = sha(*h), sha(*v)
        del h, v
        part, whole = [], []
        for i in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            marks.clear()
            t = time.perf_counter()
            composed(ix, q, offs, comp, a, marks)
            t1 = time.perf_counter()
            if i >= a.warmup:
                part.append(marks[0] - t)
                whole.append(t1 - t)
        emit({"leg": "hits", **stats(part), "what": "windows packed, positions_batch_t(locate=True), fetch_reads_t of 23 bytes per hit, strand in torch", "sha256": sh})
        emit({"leg": "votes", **stats(whole), "what": "the above plus the grouping in torch (packed key, stable sort, unique_consecutive)", "sha256": sv})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default="")
    ap.add_argument("--parent-tree", default="", help="a built checkout of the parent commit for the baseline")
    ap.add_argument("--genome", type=int, default=50_000_000)
    ap.add_argument("--seqs", type=int, default=10_000)
    ap.add_argument("--length", type=int, default=10_000)
    ap.add_argument("--min-votes", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--limit", type=int, default=540, help="seconds a child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seqhits"))
    ap.add_argument("--work", default=os.path.join(ROOT, "build", "seqhits"), help="scratch directory of the children's result files")
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
    out = {"sizes": {"genome": a.genome, "seqs": a.seqs, "length": a.length, "min_votes": a.min_votes}, "fused": docs["fused"]}
    if "baseline" in docs:
        out["baseline_parent_commit"] = docs["baseline"]
        base = {d["leg"]: d for d in docs["baseline"]}
        cmp_ = []
        for d in docs["fused"]:
            if d["leg"] in ("hits", "votes"):
                bl = base[d["leg"]]
                cmp_.append({"leg": d["leg"], "same_answers": d["sha256"] == bl["sha256"], "fused_ms": [d["min_ms"], d["median_ms"], d["max_ms"]],
                             "baseline_ms": [bl["min_ms"], bl["median_ms"], bl["max_ms"]], "baseline_over_fused": bl["median_ms"] / d["median_ms"],
                             "not_slower": d["median_ms"] <= bl["median_ms"] and d["max_ms"] <= bl["max_ms"] and d["min_ms"] <= bl["min_ms"]})
        out["comparison"] = cmp_
    else:
        out["baseline_parent_commit"] = "not run: --parent-tree is not there"
    json.dump(out, open(os.path.join(a.out, "seqhits.json"), "w"), indent=1)
    print(json.dumps(out.get("comparison", [])))
    if "comparison" in out:
        assert all(c["same_answers"] for c in out["comparison"]), [c["leg"] for c in out["comparison"] if not c["same_answers"]]
        assert all(c["not_slower"] for c in out["comparison"]), "a fused call lost to its baseline: " + str([c["leg"] for c in out["comparison"] if not c["not_slower"]])


if __name__ == "__main__":
    main()
