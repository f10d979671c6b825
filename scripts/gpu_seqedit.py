"""Sequences with indels on the MI355X: Index.seq_edit_t next to Index.seq_find_t on the same patterns, and next to the host composition.

  python scripts/gpu_seqedit.py [--parent-tree <built checkout of the parent commit>] [--genome 50000000] [--out profiles/seqedit]

The driver starts one child process per step, each under its own time limit, and stops at the first that fails:
  fused     this tree: seq_edit_t (ed 2, seed_step 23) and seq_find_t (hd 2, seed_step 23) of --seqs patterns of --length bases cut from
            the genome, every second one reverse-complemented, ONE inserted or deleted base planted in each, on the index of
            scripts/gpu_seqhits.py (6 x reads of 150 with 0.5 % substitutions, built on the device, everything attached device-resident).
            The proposals of the two calls are the same; the Hamming verification is the floor of the banded one.
  host      what a caller composes without the feature, from entry points this change does not touch (the package of --parent-tree when
            given, else this tree's): seq_hits_t on the seed windows as separate 23-byte sequences, one fetch_reads_t of the band's text
            per proposal, the bytes to the host, and the banded programme of tests/seqedit_ref.py on --sample proposals; its time for all
            proposals is the sample's, scaled.
`--child trace` makes --reps calls of seq_edit_t (the program to put behind `rocprofv3 --kernel-trace --stats --`: k_se_verify's total time
over --reps against the call's median gives the kernel's share). Times are host clocks around calls that end in a device synchronise:
median and range of --reps runs after --warmup; the timed calls are given the record count as cap_hint, so they search once. No ratio is
fixed in advance."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def patterns(a, q):
    """One indel per pattern at a seeded place j in [10, L - 10): rows of L + 1 genome bytes -> rows of L. Rows i with i % 4 < 2 lose byte j
    (a base deleted from the pattern); rows with i % 4 >= 2 gain one before j (A -> C -> G -> T -> A of the byte there) and drop their
    last byte."""
    import torch
    M, L = a.seqs, a.length
    gen = torch.Generator(device="cuda")
    gen.manual_seed(99)
    q = q.view(M, L + 1)
    j = torch.randint(10, L - 10, (M, 1), device="cuda", generator=gen)
    c = torch.arange(L, device="cuda")[None, :]
    ins = (torch.arange(M, device="cuda")[:, None] % 4) >= 2
    idx = torch.where(ins, c - (c > j).long(), c + (c >= j).long())
    out = torch.gather(q, 1, idx)
    nxt = torch.zeros(256, dtype=torch.uint8, device="cuda")
    nxt[torch.tensor([65, 67, 71, 84], device="cuda")] = torch.tensor([67, 71, 84, 65], dtype=torch.uint8, device="cuda")
    out = torch.where(ins & (c == j), nxt[out.long()], out)
    return out.reshape(-1).contiguous(), torch.arange(M + 1, device="cuda", dtype=torch.int64) * L


def host_composition(ix, q, offs, a):
    """seq_hits_t on the step-23 seeds, the band's text of every proposal to the host, the restatement's DP on a sample"""
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import seqedit_ref as E
    M, L, ed = a.seqs, a.length, a.ed
    t0 = time.perf_counter()
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
    seq, qo, strand, pos = seq[ok], qo[ok], strand[ok], pos[ok]
    a0 = torch.where(strand == 0, pos - qo, pos - (L - 23 - qo))
    rstart = (pos // 151) * 151                                    # reads of 150 at 151 i: the interval of the seed
    lo = torch.maximum(rstart, a0 - ed)
    hi = torch.minimum(rstart + 150, a0 + L + ed)
    toff, text = ix.fetch_reads_t(lo, hi)
    cols = [t.cpu().numpy() for t in (seq, strand, a0, pos, lo, toff)]
    text_h, q_h = text.cpu().numpy().tobytes(), q.cpu().numpy().tobytes()
    torch.cuda.synchronize()
    t_dev = time.perf_counter() - t0
    P = int(cols[0].shape[0])
    pick = np.random.default_rng(3).choice(P, min(a.sample, P), replace=False)

    class Shim(E.EditRef):                                         # band_dp over the fetched text of one proposal
        def __init__(self):
            self._dp = {}
    sh, kept = Shim(), 0
    t1 = time.perf_counter()
    for i in pick.tolist():
        s, st, av, pv, lv, to = (int(c[i]) for c in cols)
        n = int(cols[5][i + 1] - to) if i + 1 < P else len(text_h) - to
        sh.reads, sh.start, sh.end = text_h[to:to + n], [0], [n]   # text columns [lo, hi) moved to 0
        r = sh._band_dp(av - lv, st, 0, q_h[s * L:(s + 1) * L], ed)
        kept += r is not None
    t_dp = time.perf_counter() - t1
    return {"proposals": P, "device_and_copy_ms": 1e3 * t_dev, "sample": len(pick), "sample_survivors": kept, "dp_sample_ms": 1e3 * t_dp,
            "dp_all_scaled_ms": 1e3 * t_dp * P / max(len(pick), 1), "dp_us_per_proposal": 1e6 * t_dp / max(len(pick), 1)}


def child(a):
    import torch
    want_tree = a.parent_tree if (a.child == "host" and a.parent_tree) else ROOT
    sys.path.insert(0, want_tree)
    import aindex_amd
    tree = os.path.realpath(os.path.dirname(os.path.dirname(aindex_amd.__file__)))
    assert tree == os.path.realpath(want_tree), tree
    import gpu_seqhits as G
    a.length += 1                                                  # rows of L + 1 genome bytes for patterns()
    ix, q, offs, comp, keep = G.build(a)
    a.length -= 1
    q, offs = patterns(a, q)
    if a.child == "host":
        res = {"what": "host", "tree": "parent" if a.parent_tree else "this tree (entry points unchanged by the feature)", **host_composition(ix, q, offs, a)}
        print("RESULT " + json.dumps(res), flush=True)
        return
    ne = int(ix.seq_edit_t(q, offs, a.ed, 23)[1].numel())
    f_edit = lambda: ix.seq_edit_t(q, offs, a.ed, 23, cap_hint=ne)
    if a.child == "trace":
        for _ in range(a.reps):
            f_edit()
        torch.cuda.synchronize()
        return
    nf = int(ix.seq_find_t(q, offs, a.ed, 23)[1].numel())
    f_find = lambda: ix.seq_find_t(q, offs, a.ed, 23, cap_hint=nf)
    oe, of = f_edit(), f_find()
    hits = int(ix.seq_hits_t(q, offs, cap_hint=0)[0][-1]) if a.seqs <= 100_000 else None
    res = {"what": "fused", "ed": a.ed, "edit_records": ne, "find_records": nf, "patterns_found_edit": int((oe[0][1:] > oe[0][:-1]).sum()),
           "patterns_found_find": int((of[0][1:] > of[0][:-1]).sum()), "dist_counts": torch.bincount(oe[6].long(), minlength=a.ed + 1).tolist(),
           "all_window_hits": hits, "sha256_edit": G.sha(*oe), "seq_edit_t": G.timed(f_edit, a.warmup, a.reps), "seq_find_t": G.timed(f_find, a.warmup, a.reps)}
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default="")
    ap.add_argument("--genome", type=int, default=50_000_000)
    ap.add_argument("--seqs", type=int, default=1_000_000)
    ap.add_argument("--length", type=int, default=100)
    ap.add_argument("--ed", type=int, default=2)
    ap.add_argument("--sample", type=int, default=2000, help="proposals the host DP is timed on")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--limit", type=int, default=300, help="seconds per child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seqedit"))
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        return child(a)
    res = {"sizes": {"genome": a.genome, "seqs": a.seqs, "length": a.length, "ed": a.ed}}
    for what in ("fused", "host"):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", what]
        cmd += [x for k in ("parent_tree", "genome", "seqs", "length", "ed", "sample", "warmup", "reps") for x in ("--" + k.replace("_", "-"), str(getattr(a, k)))
                if getattr(a, k) != ""]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            sys.exit(f"{what} failed with exit status {p.returncode}; nothing more is started\n{p.stderr[-2000:]}")
        res[what] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    os.makedirs(a.out, exist_ok=True)
    json.dump(res, open(os.path.join(a.out, "seqedit.json"), "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
