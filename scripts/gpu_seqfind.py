"""Sequences with mismatches on the MI355X: Index.seq_find_t against what a caller could compose before it existed.

  python scripts/gpu_seqfind.py --parent-tree <built checkout of the parent commit> [--genome 50000000] [--out profiles/seqfind]

The driver starts one child process per step, each under its own time limit, and stops at the first that fails:
  fused     this tree: seq_find_t (hd 3, seed_step 23) of --seqs patterns of --length bases cut from the genome, every second one
            reverse-complemented, two substitutions planted in each, on the index of scripts/gpu_seqhits.py (6 x reads of 150 with 0.5 %
            substitutions, built on the device, everything attached device-resident)
  baseline  the package of --parent-tree (never the code under test): seq_hits_t on the seed windows as separate 23-byte sequences,
            one fetch_reads_t of L bytes per proposal, comparison under the N rule and unique in torch
Both children build the same seeded index and patterns and write a SHA-256 of the answer (find_offsets, pos, rid, local, strand, dist);
the driver asserts that they are equal and writes seqfind.json. `--child trace` makes one call of seq_find_t (the program to put behind
`rocprofv3 --kernel-trace --stats --`, which gives the share of k_sf_verify in the call). Times are host clocks around calls that end in
a device synchronise: median and range of --reps runs after --warmup; the fused call is given the record count as cap_hint, so it searches once. The fused call counts as faster only if the two ranges do not overlap.

The baseline is written for this index and these sizes: every read is 150 bytes at 151 i, so containment is arithmetic on the position,
and patterns hold clean ACGT."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def patterns(a, q):
    """two substitutions per pattern, at seeded places (A -> C -> G -> T -> A)"""
    import torch
    gen = torch.Generator(device="cuda")
    gen.manual_seed(99)
    q = q.view(a.seqs, a.length).clone()
    nxt = torch.zeros(256, dtype=torch.uint8, device="cuda")
    nxt[torch.tensor([65, 67, 71, 84], device="cuda")] = torch.tensor([67, 71, 84, 65], dtype=torch.uint8, device="cuda")
    j = torch.randint(0, a.length // 2, (a.seqs, 2), device="cuda", generator=gen)
    j[:, 1] += a.length // 2                                        # two different places
    rows = torch.arange(a.seqs, device="cuda")
    for c in range(2):
        q[rows, j[:, c]] = nxt[q[rows, j[:, c]].long()]
    return q.reshape(-1).contiguous()


def composed(ix, q, offs, comp, a):
    """The parent commit's composition of aix_seq_find (hd = a.hd, seed_step 23)."""
    import torch
    M, L = a.seqs, a.length
    seeds = torch.arange(0, L - 22, 23, device="cuda")
    ns = seeds.numel()
    starts = (offs[:-1, None] + seeds[None, :]).reshape(-1)
    win = q[starts[:, None] + torch.arange(23, device="cuda")[None, :]].reshape(-1).contiguous()
    woffs = torch.arange(M * ns + 1, device="cuda", dtype=torch.int64) * 23
    so, _, pos, _, _, flag = ix.seq_hits_t(win, woffs)
    cnt = so[1:] - so[:-1]
    widx = torch.repeat_interleave(torch.arange(M * ns, device="cuda"), cnt)
    seq, qo = widx // ns, (widx % ns) * 23
    strand = (flag & 3).long()
    ok = strand < 2
    a0 = torch.where(strand == 0, pos - qo, pos - (L - 23 - qo))
    ok &= (a0 >= 0) & (a0 % 151 + L <= 150)                         # reads of 150 at 151 i: containment
    seq, a0, strand = seq[ok], a0[ok], strand[ok]
    _, by = ix.fetch_reads_t(a0, a0 + L)
    x = by.view(-1, L)
    pat = q.view(M, L)[seq]
    y = torch.where((strand == 1)[:, None], comp[pat.long()].flip(1), pat)
    d = ((x != y) & (x != 78) & (y != 78)).sum(dim=1)
    keep = d <= a.hd
    key = (seq[keep] << 40) | (a0[keep] << 1) | strand[keep]       # 2^39 bytes of reads, 2^23 patterns
    assert int(a0.max()) < (1 << 39) and M < (1 << 23)
    key, inv = torch.unique(key, sorted=True, return_inverse=True)
    dist = torch.zeros(key.numel(), dtype=torch.int64, device="cuda")
    dist[inv] = d[keep]
    pos_o = (key >> 1) & ((1 << 39) - 1)
    fo = torch.zeros(M + 1, dtype=torch.int64, device="cuda")
    fo[1:] = torch.cumsum(torch.bincount(key >> 40, minlength=M), 0)
    return fo, pos_o, pos_o // 151, pos_o % 151, (key & 1).to(torch.uint8), dist.to(torch.int32)


def child(a):
    import torch
    want_tree = a.parent_tree if a.child == "baseline" else ROOT
    sys.path.insert(0, want_tree)
    import aindex_amd
    tree = os.path.realpath(os.path.dirname(os.path.dirname(aindex_amd.__file__)))
    assert tree == os.path.realpath(want_tree), tree             # the baseline never runs the package under test
    import gpu_seqhits as G
    ix, q, offs, comp, keep = G.build(a)
    q = patterns(a, q)
    if a.child == "baseline":
        fn = lambda: composed(ix, q, offs, comp, a)
    else:
        # the timed call is told the record count of a first one, so it runs the search once, not once to size and once to fill
        n = int(ix.seq_find_t(q, offs, a.hd, 23)[1].numel())
        fn = lambda: ix.seq_find_t(q, offs, a.hd, 23, cap_hint=n)
    if a.child == "trace":
        fn()
        torch.cuda.synchronize()
        return
    out = fn()
    res = {"what": a.child, "records": int(out[1].numel()), "sha256": G.sha(*out), "time": G.timed(fn, a.warmup, a.reps)}
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default="")
    ap.add_argument("--genome", type=int, default=50_000_000)
    ap.add_argument("--seqs", type=int, default=1_000_000)
    ap.add_argument("--length", type=int, default=100)
    ap.add_argument("--hd", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--limit", type=int, default=420, help="seconds per child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seqfind"))
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.parent_tree:
        sys.exit("--parent-tree is needed: the baseline runs the parent commit's package")
    res = {}
    for what in ("fused", "baseline"):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", what] + [x for k in ("parent_tree", "genome", "seqs", "length", "hd", "warmup", "reps")
                                                                             for x in ("--" + k.replace("_", "-"), str(getattr(a, k)))]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        if p.returncode != 0:
            sys.exit(f"{what} failed with exit status {p.returncode}; nothing more is started\n{p.stderr[-2000:]}")
        res[what] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert res["fused"]["sha256"] == res["baseline"]["sha256"], "the fused call and the composition differ"
    f, b = res["fused"]["time"], res["baseline"]["time"]
    res["ranges_overlap"] = not (f["max_ms"] < b["min_ms"] or b["max_ms"] < f["min_ms"])
    os.makedirs(a.out, exist_ok=True)
    json.dump(res, open(os.path.join(a.out, "seqfind.json"), "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
