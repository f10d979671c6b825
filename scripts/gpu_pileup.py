"""The pile-up on the MI355X: Index.pile_place_t, pileup_t and pile_call_t for the 150 bp read sets of scripts/gpu_seqthread.py on their
graphs (cutoff 0, rounds = 0), against a torch route for the pile.

  python scripts/gpu_pileup.py [--genome 50000000] [--reads 800000] [--out profiles/pileup]

The driver starts one child process under a time limit. The child builds the two indexes of gpu_debruijn.build_indexes, makes the thread
graph once per index and threads --reads reads through it (not timed: scripts/gpu_seqthread.py measures that): error-free reads through
the clean index, its own reads through the index of reads with 0.5 % substitutions, and those reads through the clean index. Whole
calls, host clocks around calls that end in a device synchronise: median and range of --reps runs after --warmup. Legs:
  pile_place_t                 the steps merged into placements
  pileup_t                     into a counts array that is kept (accumulating, as a caller piling batch after batch does)
  pile_call_t                  with cap_hint = the total (so nothing is sized first)
  place_pile_call              the three in a row (the counts keep accumulating: where that brings variants, the call sizes them first)
  torch_route                  the pile alone, from the placements pile_place_t wrote (the route gets them for free): repeat_interleave over
                               the placement lengths, gathers of read and contig bytes, index_add_ into the counts, the mismatches per
                               placement by a second index_add_. Its counts are compared with pileup_t's before anything is timed."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gpu_debruijn as GD  # noqa: E402  (the seeded indexes and the timer of the De Bruijn measurements)
import gpu_seqthread as GS  # noqa: E402  (the reads with substitutions, by the same seeds)


def child(kind, a):
    import torch
    sys.path.insert(0, ROOT)
    from aindex_amd import engine
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)
        json.dump(lines, open(os.path.join(a.work, f"pileup_{kind}.json"), "w"), indent=1)

    idx = GD.build_indexes(a)
    emit({"leg": "indexes", **{k: int(v[0].n) for k, v in idx.items()}})
    clean = engine.synth_reads_t(43, idx["clean"][1], a.reads, 150, rc_half=True).view(-1, 151)[:, :150].contiguous().reshape(-1)
    noisy = GS.noisy_reads(idx["reads_0.5pct_substitutions"][1], 6 * a.genome_reads // 150)[: a.reads][:, :150].contiguous().reshape(-1)
    # 150 bases per read, no separators. The third leg lays the reads with substitutions over the graph of the clean genome: the only one
    # where steps merge and bases differ from the contig's (on its own index every k-mer of a read is a stored one)
    for name, ix, flat in (("clean", idx["clean"][0], clean), ("reads_0.5pct_substitutions", idx["reads_0.5pct_substitutions"][0], noisy),
                           ("substituted_reads_on_clean_graph", idx["clean"][0], noisy)):
        M = flat.numel() // 150
        offs = torch.arange(M + 1, dtype=torch.int64, device="cuda") * 150
        graph = ix.thread_graph_t(0)
        steps = ix.seq_thread_t(graph, flat, offs)
        B = graph["bases"].numel()
        res = {"leg": f"pileup_{name}", "keys": int(ix.n), "reads": M, "read_bases": 150 * M, "U": graph["U"], "contig_bases": B, "steps": steps[1].numel()}
        places = ix.pile_place_t(graph, offs, steps)
        piled = ix.pileup_t(graph, flat, offs, places)
        called = ix.pile_call_t(graph, piled["counts"])
        R = places["n_place"]
        res.update(placements=R, circular_steps=places["n_circular_steps"], merged_placements=int((places["place_steps"] > 1).sum()),
                   piled_bases=int(places["place_len"].sum()), stats=piled["stats"], variants=called["total"], changed=called["n_changed"],
                   uncovered_bases=int(called["uncovered"].sum()))
        counts = torch.zeros(4 * B, dtype=torch.int32, device="cuda")
        res["pile_place_t"] = GD.timed(lambda: ix.pile_place_t(graph, offs, steps), a.warmup, a.reps)
        res["pileup_t"] = GD.timed(lambda: ix.pileup_t(graph, flat, offs, places, counts), a.warmup, a.reps)
        res["pile_call_t"] = GD.timed(lambda: ix.pile_call_t(graph, piled["counts"], cap_hint=called["total"]), a.warmup, a.reps)

        def whole():
            p = ix.pile_place_t(graph, offs, steps)
            c = ix.pileup_t(graph, flat, offs, p, counts)
            return ix.pile_call_t(graph, c["counts"], cap_hint=called["total"])
        res["place_pile_call"] = GD.timed(whole, a.warmup, a.reps)
        ms = res["pileup_t"]["median_ms"]
        res.update(piled_bases_per_s=res["piled_bases"] / ms * 1e3, pileup_counts_bytes_per_s=32 * B / ms * 1e3)
        # the torch route of the pile
        spo, pu, pf, pp, pq, pl = (places[k] for k in ix.PLACE_KEYS[:6])
        off, bases = graph["offsets"], graph["bases"]
        rcounts = torch.zeros(4 * B, dtype=torch.int32, device="cuda")

        def route():
            ln = pl.long()
            seq = torch.repeat_interleave(torch.arange(M, device="cuda"), spo[1:] - spo[:-1])
            r = torch.repeat_interleave(torch.arange(R, device="cuda"), ln)
            x = torch.arange(r.numel(), device="cuda") - (torch.cumsum(ln, 0) - ln)[r]
            g0 = off[pu.long()] + pp.long()
            back = (pf[r] & 1).bool()
            gb = torch.where(back, (g0 + ln - 1)[r] - x, g0[r] + x)
            rb = flat[(offs[seq] + pq.long())[r] + x]
            code = (((rb >> 1) ^ (rb >> 2)) & 3).long()
            code = torch.where(back, 3 - code, code)
            ok = (rb == 65) | (rb == 67) | (rb == 71) | (rb == 84)
            cb = bases[gb]
            rcounts.index_add_(0, 4 * gb + code, ok.to(torch.int32))
            mism = torch.zeros(R, dtype=torch.int32, device="cuda")
            mism.index_add_(0, r, (ok & (code != (((cb >> 1) ^ (cb >> 2)) & 3))).to(torch.int32))
            return mism
        mism = route()
        res["torch_route_equal"] = bool(torch.equal(rcounts, piled["counts"]) and torch.equal(mism, piled["place_mism"]))
        res["torch_route"] = GD.timed(route, a.warmup, a.reps)
        res["torch_route_over_pileup_t"] = res["torch_route"]["median_ms"] / ms
        emit(res)
        del graph, steps, places, piled, called, counts, rcounts
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default="")
    ap.add_argument("--genome", type=int, default=50_000_000)
    ap.add_argument("--genome-reads", type=int, default=20_000_000, help="leading part of the genome the reads with substitutions cover (6 x)")
    ap.add_argument("--reads", type=int, default=800_000, help="reads of 150 bp piled per call")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--limit", type=int, default=840, help="seconds the child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pileup"))
    ap.add_argument("--work", default=os.path.join(ROOT, "build", "pileup"), help="scratch directory of the child's result file")
    a = ap.parse_args()
    os.makedirs(a.work, exist_ok=True)
    if a.child:
        return child(a.child, a)
    os.makedirs(a.out, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", "clean"] + sys.argv[1:]
    r = subprocess.run(cmd)
    if r.returncode != 0:
        raise SystemExit(f"the child ended with status {r.returncode}")
    out = json.load(open(os.path.join(a.work, "pileup_clean.json")))
    json.dump(out, open(os.path.join(a.out, "pileup.json"), "w"), indent=1)
    print(json.dumps(out[1:]))


if __name__ == "__main__":
    main()
