"""Threading on the MI355X: Index.seq_thread_t on the two indexes of scripts/gpu_unitigs.py at cutoff 0, against the route that exists
without it and against coverage_t on the same sequences.

  python scripts/gpu_seqthread.py [--genome 50000000] [--reads 800000] [--out profiles/seqthread]

The driver starts one child process under a time limit. The child builds the clean index and the index of reads with 0.5 % substitutions
(gpu_debruijn.build_indexes), makes the thread graph once per index (Index.thread_graph_t, rounds = 0) and threads --reads reads of 150 bp
through it: error-free reads of the genome through the clean index, its own reads (the same seeds, so the same bytes) through the reads
index. Whole calls, host clocks around calls that end in a device synchronise: median and range of --reps runs after --warmup. Legs:
  seq_thread_t                 one call with cap_hint = the total (so nothing is sized first), with and without link_support
  existing_route               the windows materialised as N x 23 bytes, aix_kid_strand_batch_ascii_dev, three torch gathers into the
                               per-kid arrays, a torch run-length pass (diff / nonzero) for the steps. No link search: that favours the route
  coverage_t                   the same sequences
  thread_graph_t               rounds = 0 and rounds = 3 (thresholds 46), on the reads index"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gpu_debruijn as GD  # noqa: E402  (the seeded indexes and the timer of the De Bruijn measurements)


def noisy_reads(g2, n_reads):
    """the reads of build_indexes (the same seeds): 150 bases + a line end each, 0.5 % substitutions"""
    import torch
    from aindex_amd import engine
    reads = engine.synth_reads_t(43, g2, n_reads, 150, rc_half=True).view(-1, 151)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    hit = torch.rand(reads.shape, device="cuda", generator=gen) < 0.005
    hit[:, 150] = False
    lut = torch.tensor([65, 67, 71, 84], dtype=torch.uint8, device="cuda")
    code = ((reads >> 1) ^ (reads >> 2)) & 3
    other = (code + torch.randint(1, 4, reads.shape, device="cuda", generator=gen, dtype=torch.uint8)) & 3
    return torch.where(hit, lut[other.long()], reads)


def child(kind, a):
    import torch
    sys.path.insert(0, ROOT)
    from aindex_amd import engine
    from aindex_amd._lib import check, lib, vp
    from aindex_amd.engine import _stream_ptr
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)
        json.dump(lines, open(os.path.join(a.work, f"seqthread_{kind}.json"), "w"), indent=1)

    idx = GD.build_indexes(a)
    emit({"leg": "indexes", **{k: int(v[0].n) for k, v in idx.items()}})
    for name, (ix, g) in idx.items():
        if name == "clean":
            reads = engine.synth_reads_t(43, g, a.reads, 150, rc_half=True).view(-1, 151)
        else:
            reads = noisy_reads(g, 6 * a.genome_reads // 150)[: a.reads]
        seqs = reads[:, :150].contiguous()                           # 150 bases per read, no separators
        M = seqs.shape[0]
        flat = seqs.reshape(-1)
        offs = torch.arange(M + 1, dtype=torch.int64, device="cuda") * 150
        W = M * 128
        del reads
        res = {"leg": f"seqthread_{name}", "keys": int(ix.n), "reads": M, "windows": W}
        res["thread_graph_t_rounds0"] = GD.timed(lambda: ix.thread_graph_t(0), 1, 3)
        graph = ix.thread_graph_t(0)
        res.update(U=graph["U"], E=graph["E"])
        out = ix.seq_thread_t(graph, flat, offs)
        T = out[1].numel()
        link = out[6]
        res.update(steps=T, junctions=int((link >= 0).sum()), broken=int((link == -2).sum()), nodes=int((out[5] - out[4] + 1).sum()))
        sup = torch.zeros(graph["E"], dtype=torch.int64, device="cuda")
        res["seq_thread_t"] = GD.timed(lambda: ix.seq_thread_t(graph, flat, offs, cap_hint=T), a.warmup, a.reps)
        res["seq_thread_t_with_support"] = GD.timed(lambda: ix.seq_thread_t(graph, flat, offs, link_support=sup, cap_hint=T), a.warmup, a.reps)
        res["seq_thread_t_sized_first"] = GD.timed(lambda: ix.seq_thread_t(graph, flat, offs), a.warmup, a.reps)
        ms = res["seq_thread_t"]["median_ms"]
        res.update(windows_per_s=W / ms * 1e3, steps_per_s=T / ms * 1e3, junctions_per_s=res["junctions"] / res["seq_thread_t_with_support"]["median_ms"] * 1e3)
        # the existing route
        ku, kp, kf = graph["kid_unitig"], graph["kid_pos"], graph["kid_flag"]
        st = _stream_ptr(ix.device)

        def route():
            win = seqs.unfold(1, 23, 1).reshape(-1, 23).contiguous()  # N x 23 bytes
            kid = torch.empty(W, dtype=torch.int64, device="cuda")
            strand = torch.empty(W, dtype=torch.uint8, device="cuda")
            check(lib().aix_kid_strand_batch_ascii_dev(ix._h, vp(win.data_ptr()), W, vp(kid.data_ptr()), vp(strand.data_ptr()), st))
            at = torch.where(strand != 0, kid, torch.zeros_like(kid))
            u, p, f = ku[at], kp[at].to(torch.int64), kf[at]
            live = (strand != 0) & (u >= 0)
            s = (f & 1) ^ (strand == 2).to(torch.uint8)
            step = torch.where(s == 0, 1, -1)
            q = torch.arange(W, device="cuda") % 128
            cont = live[1:] & live[:-1] & (u[1:] == u[:-1]) & (s[1:] == s[:-1]) & (p[1:] == p[:-1] + step[:-1]) & (q[1:] != 0)
            head = live.clone()
            head[1:] &= ~cont
            return torch.nonzero(head).reshape(-1)
        heads = route()
        res["existing_route_steps"] = int(heads.numel())               # (no wrap round circular unitigs: it may count a few more)
        res["existing_route"] = GD.timed(route, a.warmup, a.reps)
        res["existing_route_over_seq_thread_t"] = res["existing_route"]["median_ms"] / ms
        # coverage on the same sequences
        out_offs = torch.arange(M + 1, dtype=torch.int64, device="cuda") * 128
        cov = torch.zeros(W, dtype=torch.int32, device="cuda")
        res["coverage_t"] = GD.timed(lambda: ix.coverage_t(flat, offs, out_offs, W, 0, out_t=cov), a.warmup, a.reps)
        res["present_windows"] = int((cov != 0).sum())
        res["coverage_windows_per_s"] = W / res["coverage_t"]["median_ms"] * 1e3
        res["seq_thread_t_over_coverage_t_rate"] = res["windows_per_s"] / res["coverage_windows_per_s"]
        if name != "clean":
            res["thread_graph_t_rounds3"] = GD.timed(lambda: ix.thread_graph_t(0, 46, 46, 3), 1, 3)
            g3 = ix.thread_graph_t(0, 46, 46, 3)
            o3 = ix.seq_thread_t(g3, flat, offs)
            res["contigs"] = {"rounds": g3["rounds"], "U": g3["U"], "E": g3["E"], "steps": o3[1].numel(), "broken": int((o3[6] == -2).sum())}
            res["seq_thread_t_contigs"] = GD.timed(lambda: ix.seq_thread_t(g3, flat, offs, cap_hint=o3[1].numel()), a.warmup, a.reps)
            del g3, o3
        emit(res)
        del graph, out, sup, cov, heads, seqs, flat
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default="")
    ap.add_argument("--genome", type=int, default=50_000_000)
    ap.add_argument("--genome-reads", type=int, default=20_000_000, help="leading part of the genome the reads with substitutions cover (6 x)")
    ap.add_argument("--reads", type=int, default=800_000, help="reads of 150 bp threaded per call")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--limit", type=int, default=840, help="seconds the child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seqthread"))
    ap.add_argument("--work", default=os.path.join(ROOT, "build", "seqthread"), help="scratch directory of the child's result file")
    a = ap.parse_args()
    os.makedirs(a.work, exist_ok=True)
    if a.child:
        return child(a.child, a)
    os.makedirs(a.out, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", "clean"] + sys.argv[1:]
    r = subprocess.run(cmd)
    if r.returncode != 0:
        raise SystemExit(f"the child ended with status {r.returncode}")
    out = json.load(open(os.path.join(a.work, "seqthread_clean.json")))
    json.dump(out, open(os.path.join(a.out, "seqthread.json"), "w"), indent=1)
    print(json.dumps(out[1:]))


if __name__ == "__main__":
    main()
