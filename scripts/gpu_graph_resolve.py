"""Repeat resolution on the MI355X: Index.thread_pairs_t and Index.graph_resolve_t on the reads index of scripts/gpu_seqthread.py, and
what the resolution does to an assembly with planted repeats.

  python scripts/gpu_graph_resolve.py [--genome 50000000] [--reads 800000] [--out profiles/resolve]

The driver starts one child process under a time limit. Whole calls, host clocks around calls that end in a device synchronise: median
and range of --reps runs after --warmup. Legs:
  pairs      thread_pairs_t on the step arrays of --reads reads of 150 bp (0.5 % substitutions) threaded through the unitig graph of the
             reads index at cutoff 0, against the torch route: the transitions selected by masks, the dual of the entry link found by a
             gather of the (at most four) words of its end, the cells counted by torch.bincount. The route validates nothing: that
             favours the route.
  resolve    mark + layout + emit (graph_resolve_t, compact = False) on that graph with the support and the pairs of those reads, next to
             one graph_compact_t round under a zero mask on the same graph
  assembly   a genome of --asm-genome bases with --asm-repeats planted two-copy repeats of 30 .. 140 bases, error-free reads of 150 bp at
             30 x: contigs and N50 of the cleaned graph (3 rounds, thresholds 46) before and after the resolution, and the number of output
             contigs that are no substring of the genome or of its reverse complement"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gpu_debruijn as GD  # noqa: E402  (the seeded indexes and the timer of the De Bruijn measurements)
import gpu_seqthread as GS  # noqa: E402  (the reads with substitutions)


def torch_pairs(graph, steps):
    """the 16 U array of thread_pairs_t from torch gathers and bincount; nothing is validated"""
    import torch
    lo, to = graph["link_off"], graph["link_to"].to(torch.int64)
    U, E = graph["U"], graph["E"]
    su, sf, sl = steps[1].to(torch.int64), steps[3].to(torch.int64) & 1, steps[6]
    ok = (sl >= 0) & (sl < E)
    i = torch.nonzero(ok[1:-1] & ok[2:]).reshape(-1) + 1
    u, s, b = su[i], sf[i], sl[i + 1]
    e, ep = 2 * u + s, 2 * su[i - 1] + sf[i - 1]
    first = lo[e ^ 1]
    deg = lo[(e ^ 1) + 1] - first
    k = torch.arange(4, device=lo.device)[None, :]
    words = to[(first[:, None] + k).clamp(max=max(E - 1, 0))]
    hit = (k < deg[:, None]) & (words == (ep ^ 1)[:, None])
    d = hit.to(torch.uint8).argmax(dim=1)                            # the first one
    x = torch.where(s == 0, b - lo[2 * u], d)
    y = torch.where(s == 0, d, b - lo[2 * u + 1])
    return torch.bincount(16 * u + 4 * x + y, minlength=16 * U)


def n50(lengths):
    lengths = sorted(lengths, reverse=True)
    half, run = sum(lengths) / 2, 0
    for n in lengths:
        run += n
        if run >= half:
            return n
    return 0


def assembly(a, emit):
    import numpy as np
    import torch
    from aindex_amd import _lib, builder, counting, engine
    from aindex_amd.engine import Index
    g = engine.synth_genome_t(61, a.asm_genome)
    rng = np.random.default_rng(62)
    slot = a.asm_genome // (2 * a.asm_repeats)
    for r in range(a.asm_repeats):                                    # copy a piece of slot 2 r into slot 2 r + 1
        n = int(rng.integers(30, 141))
        src, dst = 2 * r * slot + int(rng.integers(200, slot - 400)), (2 * r + 1) * slot + int(rng.integers(200, slot - 400))
        g[dst:dst + n] = g[src:src + n]
    n_reads = 30 * a.asm_genome // 150
    reads = engine.synth_reads_t(63, g, n_reads, 150, rc_half=True).view(-1, 151)[:, :150].contiguous()
    keys, counts = counting.count_distinct_t(g, 23, _lib.CANON_TRUE_RC)      # the k-mers of the genome: the graph is exact, the reads decide
    ix = Index.build_23_codes_t(builder.build_pf_codes_t(keys, 23), keys, counts.to(torch.int32))
    graph = ix.thread_graph_t(0, 46, 46, 3)
    flat = reads.reshape(-1)
    offs = torch.arange(n_reads + 1, dtype=torch.int64, device="cuda") * 150
    sup = torch.zeros(graph["E"], dtype=torch.int64, device="cuda")
    steps = ix.seq_thread_t(graph, flat, offs, link_support=sup)
    pair, n_pairs = ix.thread_pairs_t(graph, steps)
    res = ix.graph_resolve_t(graph, sup, pair, compact=True)
    before = (graph["offsets"][1:] - graph["offsets"][:-1]).cpu().tolist()
    after = (res["offsets"][1:] - res["offsets"][:-1]).cpu().tolist()
    text = bytes(g.cpu().numpy())
    back = text[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))
    out, off = bytes(res["bases"].cpu().numpy()), res["offsets"].cpu().tolist()
    circ = res["circular"].cpu().tolist()
    wrong = sum(1 for i in range(res["U"]) if not circ[i] and out[off[i]:off[i + 1]] not in text and out[off[i]:off[i + 1]] not in back)
    emit({"leg": "assembly", "genome": a.asm_genome, "planted_repeats": a.asm_repeats, "reads": n_reads, "keys": int(ix.n), "transitions": n_pairs,
          "contigs_before": len(before), "n50_before": n50(before), "longest_before": max(before), "links_before": graph["E"],
          "links_removed": res["resolved"]["n_links_removed"], "unitigs_split": res["resolved"]["n_split"], "copies_added": res["resolved"]["n_copies_added"],
          "contigs_after": len(after), "n50_after": n50(after), "longest_after": max(after), "links_after": res["E"],
          "circular_contigs_after": int(sum(circ)), "contigs_not_in_genome": wrong})


def child(kind, a):
    import torch
    sys.path.insert(0, ROOT)
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)
        json.dump(lines, open(os.path.join(a.work, f"resolve_{kind}.json"), "w"), indent=1)

    assembly(a, emit)
    idx = GD.build_indexes(a)
    ix, g = idx["reads_0.5pct_substitutions"]
    reads = GS.noisy_reads(g, 6 * a.genome_reads // 150)[: a.reads]
    seqs = reads[:, :150].contiguous()
    M = seqs.shape[0]
    flat = seqs.reshape(-1)
    offs = torch.arange(M + 1, dtype=torch.int64, device="cuda") * 150
    del reads
    graph = ix.thread_graph_t(0)
    sup = torch.zeros(graph["E"], dtype=torch.int64, device="cuda")
    steps = ix.seq_thread_t(graph, flat, offs, link_support=sup)
    pair, n_pairs = ix.thread_pairs_t(graph, steps)
    res = {"leg": "pairs", "keys": int(ix.n), "reads": M, "U": graph["U"], "E": graph["E"], "steps": steps[1].numel(), "transitions": n_pairs}
    scratch = torch.zeros_like(pair)
    res["thread_pairs_t"] = GD.timed(lambda: ix.thread_pairs_t(graph, steps, scratch), a.warmup, a.reps)
    want = torch_pairs(graph, steps)
    res["torch_route_equal"] = bool(torch.equal(want, pair))
    res["torch_route"] = GD.timed(lambda: torch_pairs(graph, steps), a.warmup, a.reps)
    res["torch_route_over_thread_pairs_t"] = res["torch_route"]["median_ms"] / res["thread_pairs_t"]["median_ms"]
    emit(res)
    out = ix.graph_resolve_t(graph, sup, pair, compact=False)
    res = {"leg": "resolve", "U": graph["U"], "E": graph["E"], "links_removed": out["n_links_removed"], "unitigs_split": out["n_split"], "U_resolved": out["U"]}
    res["graph_resolve_t"] = GD.timed(lambda: ix.graph_resolve_t(graph, sup, pair, compact=False), a.warmup, a.reps)
    res["graph_resolve_mark_t"] = GD.timed(lambda: ix.graph_resolve_mark_t(graph, sup, pair), a.warmup, a.reps)
    zero = torch.zeros(graph["U"], dtype=torch.uint8, device="cuda")
    res["graph_compact_t_zero_mask"] = GD.timed(lambda: ix.graph_compact_t(graph, None, zero), a.warmup, a.reps)
    res["graph_resolve_t_over_graph_compact_t"] = res["graph_resolve_t"]["median_ms"] / res["graph_compact_t_zero_mask"]["median_ms"]
    emit(res)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default="")
    ap.add_argument("--genome", type=int, default=50_000_000)
    ap.add_argument("--genome-reads", type=int, default=20_000_000, help="leading part of the genome the reads with substitutions cover (6 x)")
    ap.add_argument("--reads", type=int, default=800_000, help="reads of 150 bp threaded")
    ap.add_argument("--asm-genome", type=int, default=2_000_000)
    ap.add_argument("--asm-repeats", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--limit", type=int, default=840, help="seconds the child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resolve"))
    ap.add_argument("--work", default=os.path.join(ROOT, "build", "resolve"), help="scratch directory of the child's result file")
    a = ap.parse_args()
    os.makedirs(a.work, exist_ok=True)
    if a.child:
        return child(a.child, a)
    os.makedirs(a.out, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", "run"] + sys.argv[1:]
    r = subprocess.run(cmd)
    if r.returncode != 0:
        raise SystemExit(f"the child ended with status {r.returncode}")
    out = json.load(open(os.path.join(a.work, "resolve_run.json")))
    json.dump(out, open(os.path.join(a.out, "resolve.json"), "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
