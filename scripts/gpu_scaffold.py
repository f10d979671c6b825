"""Scaffolding on the MI355X: Index.mate_links_t + Index.mate_bundle_t on the reads index of scripts/gpu_seqthread.py, and what
scaffolding does to an assembly whose repeats are longer than its reads.

  python scripts/gpu_scaffold.py [--genome 50000000] [--reads 800000] [--out profiles/scaffold]

The driver starts one child process under a time limit. Whole calls, host clocks around calls that end in a device synchronise: median
and range of --reps runs after --warmup. Legs:
  links      mate_links_t + mate_bundle_t on the step arrays of --reads reads of 150 bp (0.5 % substitutions) taken two by two as
             pairs and threaded through the unitig graph of the reads index at cutoff 0, against the torch route: the anchors by two
             scatter_reduce passes over the steps, gathers for the coordinates, torch.unique(return_counts) on the keys, index_add_ for
             dsum, a sort of both directions for the lists. The route validates nothing: that favours the route.
  assembly   a genome of --asm-genome bases with --asm-repeats planted two-copy repeats of 200 .. 350 bases, error-free pairs of 100 bp at
             insert 500 +- 30 and 30 x: contigs, N50 and longest of the cleaned graph (3 rounds, thresholds 46) before and after
             scaffolding, the misjoins (adjacent members that are not neighbours in that relative orientation in the genome) and the
             distribution of gap - true distance"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gpu_debruijn as GD  # noqa: E402  (the seeded indexes and the timer of the De Bruijn measurements)
import gpu_graph_resolve as GR  # noqa: E402  (n50)
import gpu_seqthread as GS  # noqa: E402  (the reads with substitutions)

NONE = -1


def torch_links(graph, steps, offs, min_windows, max_insert):
    """obs_key, obs_d, counts, hist of mate_links_t from torch gathers; nothing is validated"""
    import torch
    sso, su, sp, sf, qf, ql = [t.to(torch.int64) for t in steps[:6]]
    off, circ = graph["offsets"], graph["circular"]
    M, T = sso.numel() - 1, su.numel()
    dev = su.device
    seq = torch.repeat_interleave(torch.arange(M, device=dev), sso[1:] - sso[:-1])
    w = ql - qf + 1
    best = torch.zeros(M, dtype=torch.int64, device=dev).scatter_reduce(0, seq, w, "amax", include_self=True)
    idx = torch.arange(T, device=dev)
    first = torch.full((M,), T, dtype=torch.int64, device=dev).scatter_reduce(0, seq[w == best[seq]], idx[w == best[seq]], "amin", include_self=True)
    has = (best >= max(min_windows, 1)) & (first < T)
    j = first.clamp(max=max(T - 1, 0))
    u, s = su[j], sf[j] & 1
    has &= circ[u] == 0
    L = off[u + 1] - off[u]
    x0 = torch.where(s == 1, L - 23 - sp[j], sp[j]) - qf[j]
    uA, uB, sA, sB, xA, xB, hA, hB, LA = u[0::2], u[1::2], s[0::2], s[1::2], x0[0::2], x0[1::2], has[0::2], has[1::2], L[0::2]
    LB = (offs[2::2] - offs[1::2])[: uA.numel()]
    both = hA & hB
    F = xB + LB - xA
    same = both & (uA == uB) & (sA == sB) & (F >= 1) & (F <= max_insert)
    d = (LA - xA) + (xB + LB)
    link = both & (uA != uB) & (d <= max_insert)
    e, t = 2 * uA + sA, 2 * uB + sB
    swap = (t ^ 1) < e
    e, t = torch.where(swap, t ^ 1, e), torch.where(swap, e ^ 1, t)
    key = torch.where(link, e << 32 | t, torch.full_like(e, -1))
    hist = torch.bincount(F[same], minlength=max_insert + 1)
    counts = torch.stack([same.sum(), link.sum(), (both & ~same & ~link).sum(), (~both).sum()])
    return key, torch.where(link, d, torch.zeros_like(d)).to(torch.int32), counts, hist


def torch_bundle(key, d, U):
    """the four arrays of mate_bundle_t: torch.unique with counts, index_add_ for dsum, both directions sorted"""
    import torch
    live = key != -1
    uniq, inv, cnt = torch.unique(key[live], return_inverse=True, return_counts=True)
    dsum = torch.zeros_like(cnt).index_add_(0, inv, d[live].to(torch.int64))
    e, t = uniq >> 32, uniq & 0xFFFFFFFF
    both = torch.cat([uniq, (t ^ 1) << 32 | (e ^ 1)])
    order = torch.argsort(both)
    both = both[order]
    off = torch.searchsorted(both, torch.arange(2 * U + 1, device=key.device) << 32)
    return off, (both & 0xFFFFFFFF).to(torch.int32), torch.cat([cnt, cnt])[order], torch.cat([dsum, dsum])[order]


def pairs_t(g, n, read_len, insert, jitter, seed):
    """n pairs as one byte tensor of 2 n reads (left, right, left, ..), both mates on the fragment's strand; every other fragment is taken
    from the reverse strand. -> (bytes, offsets)"""
    import torch
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    G = g.numel()
    start = torch.randint(0, G - insert - jitter, (n,), device="cuda", generator=gen)
    ins = insert + torch.randint(-jitter, jitter + 1, (n,), device="cuda", generator=gen)
    k = torch.arange(read_len, device="cuda")[None, :]
    left, right = g[start[:, None] + k], g[(start + ins - read_len)[:, None] + k]
    comp = torch.zeros(256, dtype=torch.uint8, device="cuda")
    comp[torch.tensor([65, 67, 71, 84], device="cuda")] = torch.tensor([84, 71, 67, 65], dtype=torch.uint8, device="cuda")
    back = torch.arange(n, device="cuda") % 2 == 1
    rc = lambda x: comp[x.long()].flip(1)
    a = torch.where(back[:, None], rc(right), left)
    b = torch.where(back[:, None], rc(left), right)
    return torch.stack([a, b], 1).reshape(-1).contiguous(), torch.arange(2 * n + 1, dtype=torch.int64, device="cuda") * read_len


def assembly(a, emit):
    import numpy as np
    import torch
    from aindex_amd import _lib, builder, counting, engine
    from aindex_amd.engine import Index
    g = engine.synth_genome_t(61, a.asm_genome)
    rng = np.random.default_rng(62)
    slot = a.asm_genome // (2 * a.asm_repeats)
    for r in range(a.asm_repeats):                                    # copy a piece of slot 2 r into slot 2 r + 1
        n = int(rng.integers(200, 351))
        src, dst = 2 * r * slot + int(rng.integers(200, slot - 800)), (2 * r + 1) * slot + int(rng.integers(200, slot - 800))
        g[dst:dst + n] = g[src:src + n]
    n_pairs = 30 * a.asm_genome // 200
    data, offs = pairs_t(g, n_pairs, 100, 500, 30, 63)
    keys, counts = counting.count_distinct_t(g, 23, _lib.CANON_TRUE_RC)      # the k-mers of the genome: the graph is exact, the pairs decide
    ix = Index.build_23_codes_t(builder.build_pf_codes_t(keys, 23), keys, counts.to(torch.int32))
    graph = ix.thread_graph_t(0, 46, 46, 3)
    steps = ix.seq_thread_t(graph, data, offs)
    key, d, kinds, hist = ix.mate_links_t(graph, steps, offs, 1, 1000)
    insert = ix.insert_size_t(hist)
    sl = ix.mate_bundle_t(key, d, graph["U"])
    joins = ix.scaffold_mark_t(graph, sl, insert, a.min_pairs, a.dominance, a.min_contig_bases)
    sc = ix.scaffold_t(graph, joins, 1)
    before = (graph["offsets"][1:] - graph["offsets"][:-1]).cpu().tolist()
    after = (sc["scaffold_offsets"][1:] - sc["scaffold_offsets"][:-1]).cpu().tolist()
    # where every joined contig lies in the genome
    text = bytes(g.cpu().numpy())
    back = text[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))
    G = len(text)
    off, bases = graph["offsets"].cpu().tolist(), bytes(graph["bases"].cpu().numpy())
    mo, mem, gap = sc["member_off"].cpu().tolist(), sc["member"].cpu().tolist(), sc["member_gap"].cpu().tolist()

    def place(w):
        """(strand, start, end) in the coordinates of the strand the ORIENTED member reads forwards on; None when it is not unique"""
        u, f = w >> 1, w & 1
        s = bases[off[u]:off[u + 1]]
        fw, bw = text.find(s), back.find(s)
        if (fw >= 0) == (bw >= 0) or (fw >= 0 and text.find(s, fw + 1) >= 0) or (bw >= 0 and back.find(s, bw + 1) >= 0):
            return None
        strand, at = (0, fw) if fw >= 0 else (1, bw)
        if f:                                                          # the reversed member reads forwards on the other strand
            strand, at = strand ^ 1, G - at - len(s)
        return strand, at, at + len(s)

    misjoins, unplaced, errors = 0, 0, []
    for i in range(len(mo) - 1):
        for j in range(mo[i] + 1, mo[i + 1]):
            p, q = place(mem[j - 1]), place(mem[j])
            if p is None or q is None:
                unplaced += 1
            elif p[0] != q[0] or not -23 <= q[1] - p[2] <= 1000:
                misjoins += 1
            else:
                errors.append(gap[j] - (q[1] - p[2]))
    e = np.array(errors if errors else [0])
    emit({"leg": "assembly", "genome": a.asm_genome, "planted_repeats": a.asm_repeats, "repeat_bases": [200, 350], "pairs": n_pairs, "read_len": 100,
          "insert": [500, 30], "keys": int(ix.n), "steps": steps[1].numel(), "pair_kinds": dict(zip(("same_contig", "link", "discordant", "unanchored"), kinds.cpu().tolist())),
          "insert_size_median": insert, "scaffold_links": sl["S"] // 2, "thresholds": {"min_pairs": a.min_pairs, "dominance": a.dominance,
                                                                                      "min_contig_bases": a.min_contig_bases},
          "joins": joins["n_joins"], "cycles_cut": sc["n_cut"], "contigs_before": len(before), "n50_before": GR.n50(before), "longest_before": max(before),
          "scaffolds_after": len(after), "n50_after": GR.n50(after), "longest_after": max(after), "misjoins": misjoins, "joins_with_a_member_not_unique_in_genome": unplaced,
          "gap_minus_true": {"n": len(errors), "min": int(e.min()), "p05": float(np.percentile(e, 5)), "median": float(np.median(e)), "p95": float(np.percentile(e, 95)),
                             "max": int(e.max()), "mean_abs": float(np.abs(e).mean())}})


def child(kind, a):
    import torch
    sys.path.insert(0, ROOT)
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)
        json.dump(lines, open(os.path.join(a.work, f"scaffold_{kind}.json"), "w"), indent=1)

    assembly(a, emit)
    if a.skip_links:
        return
    print("building the reads index", flush=True)
    idx = GD.build_indexes(a)
    ix, g = idx["reads_0.5pct_substitutions"]
    reads = GS.noisy_reads(g, 6 * a.genome_reads // 150)[: a.reads]
    seqs = reads[:, :150].contiguous()
    M = seqs.shape[0] // 2 * 2
    flat = seqs[:M].reshape(-1)
    offs = torch.arange(M + 1, dtype=torch.int64, device="cuda") * 150
    del reads
    graph = ix.thread_graph_t(0)
    steps = ix.seq_thread_t(graph, flat, offs)
    mi = a.max_insert
    key, d, kinds, hist = ix.mate_links_t(graph, steps, offs, 1, mi)
    sl = ix.mate_bundle_t(key, d, graph["U"])
    res = {"leg": "links", "keys": int(ix.n), "pairs": M // 2, "U": graph["U"], "steps": steps[1].numel(), "max_insert": mi,
           "pair_kinds": dict(zip(("same_contig", "link", "discordant", "unanchored"), kinds.cpu().tolist())), "scaffold_links": sl["S"] // 2}
    scratch = torch.zeros_like(hist)

    def ours():
        k, x, _, _ = ix.mate_links_t(graph, steps, offs, 1, mi, scratch)
        return ix.mate_bundle_t(k, x, graph["U"], cap_hint=2 * k.numel())  # S <= 2 N, which a caller knows: one pass, as AIndex calls it

    def route():
        k, x, c, h = torch_links(graph, steps, offs, 1, mi)
        return (k, x, c, h) + torch_bundle(k, x, graph["U"])

    got = route()
    res["torch_route_equal"] = bool(torch.equal(got[0], key) and torch.equal(got[1], d) and torch.equal(got[2], kinds) and torch.equal(got[3], hist) and
                                    torch.equal(got[4], sl["slink_off"]) and torch.equal(got[5], sl["slink_to"]) and torch.equal(got[6], sl["slink_count"]) and
                                    torch.equal(got[7], sl["slink_dsum"]))
    res["mate_links_t_plus_mate_bundle_t"] = GD.timed(ours, a.warmup, a.reps)
    res["mate_links_t"] = GD.timed(lambda: ix.mate_links_t(graph, steps, offs, 1, mi, scratch), a.warmup, a.reps)
    res["mate_bundle_t"] = GD.timed(lambda: ix.mate_bundle_t(key, d, graph["U"], cap_hint=2 * key.numel()), a.warmup, a.reps)
    res["mate_bundle_t_without_cap_hint"] = GD.timed(lambda: ix.mate_bundle_t(key, d, graph["U"]), a.warmup, a.reps)      # a sizing pass, then the fill
    res["torch_route"] = GD.timed(route, a.warmup, a.reps)
    res["torch_route_over_calls"] = res["torch_route"]["median_ms"] / res["mate_links_t_plus_mate_bundle_t"]["median_ms"]
    emit(res)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default="")
    ap.add_argument("--genome", type=int, default=50_000_000)
    ap.add_argument("--genome-reads", type=int, default=20_000_000, help="leading part of the genome the reads with substitutions cover (6 x)")
    ap.add_argument("--reads", type=int, default=800_000, help="reads of 150 bp threaded, two by two as pairs")
    ap.add_argument("--max-insert", type=int, default=100_000, help="of the links leg: most pairs of two unrelated reads then observe a link")
    ap.add_argument("--asm-genome", type=int, default=2_000_000)
    ap.add_argument("--asm-repeats", type=int, default=200)
    ap.add_argument("--min-pairs", type=int, default=3)
    ap.add_argument("--dominance", type=int, default=2)
    ap.add_argument("--min-contig-bases", type=int, default=400, help="above a repeat's own contig (350 + 22 bases at most)")
    ap.add_argument("--skip-links", action="store_true")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--limit", type=int, default=840, help="seconds the child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scaffold"))
    ap.add_argument("--work", default=os.path.join(ROOT, "build", "scaffold"), help="scratch directory of the child's result file")
    a = ap.parse_args()
    os.makedirs(a.work, exist_ok=True)
    if a.child:
        return child(a.child, a)
    os.makedirs(a.out, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", "run"] + sys.argv[1:]
    r = subprocess.run(cmd)
    if r.returncode != 0:
        raise SystemExit(f"the child ended with status {r.returncode}")
    out = json.load(open(os.path.join(a.work, "scaffold_run.json")))
    args, skip = [], 0
    for x in sys.argv[1:]:                                             # where the files went is not part of the measurement
        if skip or x in ("--work", "--out", "--limit"):
            skip = 0 if skip else 1
            continue
        args.append(x)
    with open(os.path.join(a.out, "scaffold.json"), "w") as f:
        json.dump({"command": " ".join(["python scripts/gpu_scaffold.py"] + args), "legs": out}, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
