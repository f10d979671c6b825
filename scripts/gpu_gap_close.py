"""Gap closing on the MI355X: what Index.gap_close_t and Index.scaffold_fill_t do to the scaffolds of an assembly whose repeats are
longer than its reads, and the time of the search against a torch route.

  python scripts/gpu_gap_close.py [--asm-genome 2000000] [--joins 100000] [--out profiles/gapclose]

The driver starts one child process under a time limit. Whole calls, host clocks around calls that end in a device synchronise: median
and range of --reps runs after --warmup. Legs:
  exact      the genome of scripts/gpu_scaffold.py (--asm-genome bases, --asm-repeats planted two-copy repeats of 200 .. 350 bases,
             error-free pairs of 100 bp at insert 500 +- 30 and 30 x, the index built from the genome's k-mers): the joins by status,
             scaffolds and N50 before and after filling (with drop_absorbed), and the filled scaffolds that are no substring of the genome
  noisy      the same genome indexed FROM THE PAIRS, which carry --error-rate substitutions, at --noisy-cutoff and after the cleaning
             rounds: the same counts
  search     gap_close_t on the generated graph of tests/gap_close_cases.py (make_batch: --joins joins over mixed motifs, 2 states to
             the budget) against a level-synchronous torch route: frontier gathers, repeat_interleave over the degrees, masks, index_add_
             for hits and states. The route has no budget rule and walks no path back: that favours the route."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gpu_debruijn as GD  # noqa: E402  (the timer)
import gpu_graph_resolve as GR  # noqa: E402  (n50)
import gpu_scaffold as GS  # noqa: E402  (the pairs)

STATUS = ("closed", "no_path", "ambiguous", "exhausted")


def torch_search(graph, joins, tolerance, max_fill):
    """-> (hits int64[2 U], states int64[2 U]) at the owner ends: the rule level by level, every candidate of a level at once"""
    import torch
    off, lo, lt = graph["offsets"], graph["link_off"], graph["link_to"].long()
    jn, jg = joins["join"].long(), joins["join_gap"]
    NE = jn.numel()
    L = (off[1:] - off[:-1]).repeat_interleave(2)
    free = ((jn < 0).view(-1, 2).all(1)).repeat_interleave(2)
    e = torch.arange(NE, device=jn.device)
    own = e[(jn >= 0) & (e < (jn ^ 1))]
    hits, states = torch.zeros(NE, dtype=torch.int64, device=jn.device), torch.zeros(NE, dtype=torch.int64, device=jn.device)
    src, owner, d, k = own, own, torch.full_like(own, -22), 0
    while src.numel():
        deg = lo[src + 1] - lo[src]
        first = torch.cumsum(deg, 0) - deg
        rep = torch.repeat_interleave(torch.arange(src.numel(), device=src.device), deg)
        y = lt[lo[src][rep] + torch.arange(rep.numel(), device=src.device) - first[rep]]
        o, dd = owner[rep], d[rep]
        gap = jg[o]
        is_t = y == jn[o]
        hit = is_t & ((dd - gap).abs() <= tolerance)
        mid = ~is_t & free[y] & (dd + L[y] - 22 <= gap + tolerance) & (k < max_fill)
        hits.index_add_(0, o[hit], torch.ones_like(o[hit]))
        states.index_add_(0, o[hit | mid], torch.ones_like(o[hit | mid]))
        src, owner, d, k = y[mid], o[mid], (dd + L[y] - 22)[mid], k + 1
    return hits, states


def noisy(data, rate, seed):
    """substitutions at `rate` per base: a hit base becomes one of the three others"""
    import torch
    gen = torch.Generator(device="cuda").manual_seed(seed)
    hit = torch.rand(data.numel(), device="cuda", generator=gen) < rate
    code = torch.tensor([0] * 256, dtype=torch.uint8, device="cuda")
    for i, c in enumerate(b"ACGT"):
        code[c] = i
    shift = torch.randint(1, 4, (data.numel(),), device="cuda", generator=gen, dtype=torch.uint8)
    letters = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    return torch.where(hit, letters[((code[data.long()] + shift) & 3).long()], data)


def assembly(a, emit, leg):
    import numpy as np
    import torch
    from aindex_amd import _lib, builder, counting, engine
    from aindex_amd.engine import Index
    g = engine.synth_genome_t(61, a.asm_genome)
    rng = np.random.default_rng(62)
    slot = a.asm_genome // (2 * a.asm_repeats)
    for r in range(a.asm_repeats):                                    # copy a piece of slot 2 r into slot 2 r + 1 (as gpu_scaffold.py)
        n = int(rng.integers(200, 351))
        src, dst = 2 * r * slot + int(rng.integers(200, slot - 800)), (2 * r + 1) * slot + int(rng.integers(200, slot - 800))
        g[dst:dst + n] = g[src:src + n]
    n_pairs = 30 * a.asm_genome // 200
    data, offs = GS.pairs_t(g, n_pairs, 100, 500, 30, 63)
    cutoff = 0
    if leg == "exact":
        keys, counts = counting.count_distinct_t(g, 23, _lib.CANON_TRUE_RC)
    else:
        data = noisy(data, a.error_rate, 64)
        keys, counts = counting.count_distinct_t(data, 23, _lib.CANON_TRUE_RC)    # windows across two mates: below the cutoff, like the errors
        cutoff = a.noisy_cutoff
    ix = Index.build_23_codes_t(builder.build_pf_codes_t(keys, 23), keys, counts.clamp(max=2 ** 31 - 1).to(torch.int32))
    graph = ix.thread_graph_t(cutoff, 46, 46, 3)
    steps = ix.seq_thread_t(graph, data, offs)
    key, d, kinds, hist = ix.mate_links_t(graph, steps, offs, 1, 1000)
    insert = ix.insert_size_t(hist)
    sl = ix.mate_bundle_t(key, d, graph["U"])
    joins = ix.scaffold_mark_t(graph, sl, insert, a.min_pairs, a.dominance, a.min_contig_bases)
    sc = ix.scaffold_t(graph, joins, 1)
    cl = ix.gap_close_t(graph, joins, a.tolerance, a.max_fill, a.max_states)
    fl = ix.scaffold_fill_t(graph, joins, sc, cl, 1)
    before = (sc["scaffold_offsets"][1:] - sc["scaffold_offsets"][:-1]).cpu().tolist()
    fo, fm, uses = fl["fmember_off"].cpu().tolist(), fl["fmember"].cpu().tolist(), cl["fill_uses"].cpu().tolist()
    fso, ftext = fl["fscaffold_offsets"].cpu().tolist(), bytes(fl["fscaffold_bases"].cpu().numpy())
    kept = [s for s in range(len(fo) - 1) if not (fo[s + 1] - fo[s] == 1 and uses[fm[fo[s]] >> 1] >= 1)]
    after = [fso[s + 1] - fso[s] for s in kept]
    text = bytes(g.cpu().numpy())
    back = text[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))
    wrong = n_runs = 0
    for s in kept:
        if fo[s + 1] - fo[s] == 1:
            continue                                                  # a contig by itself: nothing was filled
        pieces = [x for x in ftext[fso[s]:fso[s + 1]].split(b"N") if x]
        n_runs += len(pieces) - 1
        wrong += any(text.find(x) < 0 and back.find(x) < 0 for x in pieces)
    st, ns = cl["close_status"].cpu().numpy(), cl["close_states"].cpu().numpy()
    jn = joins["join"].cpu().numpy()
    owners = [e for e in range(jn.shape[0]) if jn[e] >= 0 and e < (jn[e] ^ 1)]
    emit({"leg": leg, "genome": a.asm_genome, "planted_repeats": a.asm_repeats, "pairs": n_pairs, "error_rate": 0.0 if leg == "exact" else a.error_rate, "cutoff": cutoff,
          "keys": int(ix.n), "contigs": graph["U"], "links": graph["E"], "insert_size_median": insert,
          "parameters": {"tolerance": a.tolerance, "max_fill": a.max_fill, "max_states": a.max_states, "min_pairs": a.min_pairs, "dominance": a.dominance,
                         "min_contig_bases": a.min_contig_bases},
          "joins": cl["counts"][4], "joins_by_status": dict(zip(STATUS, cl["counts"][:4])), "path_entries": cl["total"],
          "states_per_join": {"max": int(max([ns[e] for e in owners], default=0)), "mean": float(np.mean([ns[e] for e in owners])) if owners else 0.0},
          "scaffolds_before": len(before), "n50_before": GR.n50(before), "longest_before": max(before), "scaffolds_after_drop_absorbed": len(after),
          "n50_after": GR.n50(after), "longest_after": max(after), "absorbed_scaffolds": len(fo) - 1 - len(kept), "n_runs_left_in_multi_member_scaffolds": n_runs,
          "filled_scaffolds_with_a_piece_not_in_genome": int(wrong),
          "gap_close_t": GD.timed(lambda: ix.gap_close_t(graph, joins, a.tolerance, a.max_fill, a.max_states), a.warmup, a.reps),
          "scaffold_fill_t": GD.timed(lambda: ix.scaffold_fill_t(graph, joins, sc, cl, 1), a.warmup, a.reps)})
    return ix


def search(a, emit, ix):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import gap_close_cases as GC
    g = GC.make_batch(1, a.joins)
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x).view(dt).copy()).cuda()
    graph = {"offsets": t(g["offsets"], np.int64), "link_off": t(g["link_off"], np.int64), "link_to": t(g["link_to"], np.int32)}
    joins = {"join": t(g["join"], np.int32), "join_gap": t(g["join_gap"], np.int64)}
    par = GC.PARAMS
    cl = ix.gap_close_t(graph, joins, **par)
    hits, states = torch_search(graph, joins, par["tolerance"], par["max_fill"])
    st = cl["close_status"].long()
    e = torch.arange(st.numel(), device="cuda")
    jn = joins["join"].long()
    own = (jn >= 0) & (e < (jn ^ 1)) & (st != 4)
    want = torch.where(hits == 0, 2, torch.where(hits > 1, 3, 1))
    res = {"leg": "search", "joins": cl["counts"][4], "contigs": g["U"], "links": g["E"], "parameters": par, "joins_by_status": dict(zip(STATUS, cl["counts"][:4])),
           "path_entries": cl["total"], "states_min": int(cl["close_states"][own].min()), "states_max": int(cl["close_states"].max()),
           "states_total": int(cl["close_states"].sum()) // 2,
           "torch_route_equal_where_not_exhausted": bool(torch.equal(want[own], st[own]) and torch.equal(states[own], cl["close_states"].long()[own]))}
    res["gap_close_t"] = GD.timed(lambda: ix.gap_close_t(graph, joins, **par), a.warmup, a.reps)
    res["gap_close_t_with_cap_hint"] = GD.timed(lambda: ix.gap_close_t(graph, joins, **par, cap_hint=cl["total"]), a.warmup, a.reps)
    res["torch_route"] = GD.timed(lambda: torch_search(graph, joins, par["tolerance"], par["max_fill"]), a.warmup, a.reps)
    res["torch_route_over_gap_close_t"] = res["torch_route"]["median_ms"] / res["gap_close_t"]["median_ms"]
    emit(res)


def child(kind, a):
    import torch
    sys.path.insert(0, ROOT)
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)
        json.dump(lines, open(os.path.join(a.work, f"gapclose_{kind}.json"), "w"), indent=1)

    ix = assembly(a, emit, "exact")
    if not a.skip_search:
        search(a, emit, ix)
    if not a.skip_noisy:
        assembly(a, emit, "noisy")
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default="")
    ap.add_argument("--asm-genome", type=int, default=2_000_000)
    ap.add_argument("--asm-repeats", type=int, default=200)
    ap.add_argument("--min-pairs", type=int, default=3)
    ap.add_argument("--dominance", type=int, default=2)
    ap.add_argument("--min-contig-bases", type=int, default=400, help="above a repeat's own contig (350 + 22 bases at most)")
    ap.add_argument("--tolerance", type=int, default=50)
    ap.add_argument("--max-fill", type=int, default=16)
    ap.add_argument("--max-states", type=int, default=1024)
    ap.add_argument("--error-rate", type=float, default=0.005)
    ap.add_argument("--noisy-cutoff", type=int, default=3)
    ap.add_argument("--joins", type=int, default=100_000)
    ap.add_argument("--skip-search", action="store_true")
    ap.add_argument("--skip-noisy", action="store_true")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--limit", type=int, default=540, help="seconds the child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gapclose"))
    ap.add_argument("--work", default=os.path.join(ROOT, "build", "gapclose"), help="scratch directory of the child's result file")
    a = ap.parse_args()
    os.makedirs(a.work, exist_ok=True)
    if a.child:
        return child(a.child, a)
    os.makedirs(a.out, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", "run"] + sys.argv[1:]
    r = subprocess.run(cmd)
    if r.returncode != 0:
        raise SystemExit(f"the child ended with status {r.returncode}")
    out = json.load(open(os.path.join(a.work, "gapclose_run.json")))
    args, skip = [], 0
    for x in sys.argv[1:]:                                             # where the files went is not part of the measurement
        if skip or x in ("--work", "--out", "--limit"):
            skip = 0 if skip else 1
            continue
        args.append(x)
    with open(os.path.join(a.out, "gapclose.json"), "w") as f:
        json.dump({"command": " ".join(["python scripts/gpu_gap_close.py"] + args), "legs": out}, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
