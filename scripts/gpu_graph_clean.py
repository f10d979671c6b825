"""Graph cleaning on the MI355X: aix_graph_mark_dev, aix_graph_compact_layout_dev and aix_graph_compact_emit_dev on the two indexes of
scripts/gpu_unitigs.py at cutoff 0, against the route that exists without them.

  python scripts/gpu_graph_clean.py [--genome 50000000] [--out profiles/unitigs]

The driver starts one child process under a time limit. The child builds the clean index and the index of reads with 0.5 % substitutions,
makes unitigs and links once, and times one round with thresholds 46 — mark, compact layout, compact emit — and the three-round
Index.graph_clean_t as whole calls (host clocks around calls that end in a device synchronise: median and range of --reps runs after
--warmup); it reports U and E of every round. In the same process it opens a second index over the k-mers of the unitigs that survive
round one and times unitigs_layout_t + unitigs_t + unitig_links_t on it: the only way to the same graph without this feature. Building
that second index (MPHF and scatter) is NOT in the time."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gpu_debruijn as GD  # noqa: E402  (the seeded indexes and the timer of the De Bruijn measurements)


def child(kind, a):
    import torch
    sys.path.insert(0, ROOT)
    from aindex_amd import builder
    from aindex_amd._lib import check, lib, vp
    from aindex_amd.engine import Index, _stream_ptr
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)
        json.dump(lines, open(os.path.join(a.work, f"graph_clean_{kind}.json"), "w"), indent=1)

    idx = GD.build_indexes(a)
    emit({"leg": "indexes", **{k: int(v[0].n) for k, v in idx.items()}})
    p = lambda t: vp(t.data_ptr())
    for name, (ix, _) in idx.items():
        un = ix.unitigs_t(0)
        lk = ix.unitig_links_t(0, unitigs=un)
        g = {k: (un[k] if k in un else lk[k]) for k in Index.GRAPH_KEYS}
        U, E, s = un["U"], lk["E"], _stream_ptr(ix.device)
        remove, tips, arms = ix.graph_mark_t(g, None, 46, 46)
        out = ix.graph_compact_t(g, None, remove)
        Cn, total, E2 = out["U"], int(out["offsets"][-1]), out["E"]
        nt, na, n4 = C.c_uint64(), C.c_uint64(), [C.c_uint64() for _ in range(4)]
        rm2, m2 = torch.empty_like(remove), [torch.empty_like(out[k]) for k in ("unitig_contig", "unitig_pos", "unitig_flag")]
        o2 = [torch.empty_like(out[k]) for k in Index.GRAPH_KEYS]
        gp = [p(g[k]) for k in Index.GRAPH_KEYS]
        mark = lambda: check(lib().aix_graph_mark_dev(U, gp[0], gp[2], gp[3], gp[6], gp[7], E, None, 46, 46, p(rm2), C.byref(nt), C.byref(na), s))
        mark_given = lambda: check(lib().aix_graph_mark_dev(U, gp[0], gp[2], gp[3], gp[6], gp[7], E, p(lk["bubble_mate"]), 46, 46, p(rm2), C.byref(nt), C.byref(na), s))
        layout = lambda: check(lib().aix_graph_compact_layout_dev(U, gp[0], gp[1], gp[2], gp[6], gp[7], E, p(remove), *[p(t) for t in m2],
                                                                  *[C.byref(x) for x in n4], s))
        emit_ = lambda: check(lib().aix_graph_compact_emit_dev(U, *gp, E, p(remove), *[p(t) for t in m2], Cn, total, E2, *[p(t) for t in o2], s))
        res = {"leg": f"graph_clean_{name}", "keys": int(ix.n), "U": U, "E": E, "bases_in": int(un["offsets"][-1]), "tips": tips, "arms": arms,
               "C": Cn, "E_out": E2, "bases_out": total, "n_circular": out["n_circular"]}
        res["mark"] = GD.timed(mark, a.warmup, a.reps)
        res["mark_given_bubble_mate"] = GD.timed(mark_given, a.warmup, a.reps)
        res["compact_layout"] = GD.timed(layout, a.warmup, a.reps)
        res["compact_emit"] = GD.timed(emit_, a.warmup, a.reps)
        assert torch.equal(rm2, remove) and all(torch.equal(x, out[k]) for x, k in zip(o2, Index.GRAPH_KEYS))
        rounds = []

        def three():
            rounds.clear()
            cur = g
            for _ in range(3):
                r, t_, a_ = ix.graph_mark_t(cur, None, 46, 46)
                rounds.append({"U": cur["offsets"].numel() - 1, "E": cur["link_to"].numel(), "tips": t_, "arms": a_})
                if t_ + a_ == 0:
                    break
                cur = ix.graph_compact_t(cur, None, r)
            rounds.append({"U": cur["offsets"].numel() - 1, "E": cur["link_to"].numel()})
        res["three_rounds"] = GD.timed(three, a.warmup, a.reps)
        res["per_round"] = list(rounds)
        # the route without the feature: a second index over the surviving k-mers (its construction is not timed)
        codes = torch.from_numpy((ix.checker_array() & ((1 << 46) - 1)).astype("int64")).cuda()
        tfs = torch.from_numpy(ix.tf_array().astype("int32")).cuda()
        ku = un["kid_unitig"]
        keep = (ku >= 0) & (remove[ku.clamp(min=0)] == 0)
        k2, order = torch.sort(codes[keep])
        t2 = tfs[keep][order].contiguous()
        second = Index.build_23_codes_t(builder.build_pf_codes_t(k2, 23), k2, t2)
        torch.cuda.synchronize()
        del codes, tfs, keep, order

        def route():
            u2 = second.unitigs_t(0, layout=second.unitigs_layout_t(0))
            return u2, second.unitig_links_t(0, unitigs=u2)
        u2, l2 = route()
        res["second_index"] = {"keys": int(second.n), "U": u2["U"], "E": l2["E"], "bases": int(u2["offsets"][-1])}
        res["second_index"]["same_sizes_as_compaction"] = (u2["U"], l2["E"], int(u2["offsets"][-1])) == (Cn, E2, total)
        res["existing_route_layout_emit_links"] = GD.timed(route, a.warmup, a.reps)
        one = res["mark"]["median_ms"] + res["compact_layout"]["median_ms"] + res["compact_emit"]["median_ms"]
        res["one_round_ms"] = one
        res["existing_route_over_one_round"] = res["existing_route_layout_emit_links"]["median_ms"] / one
        emit(res)
        second.close()
        del un, lk, g, out, o2, m2, u2, l2
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default="")
    ap.add_argument("--genome", type=int, default=50_000_000)
    ap.add_argument("--genome-reads", type=int, default=20_000_000, help="leading part of the genome the reads with substitutions cover (6 x)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--limit", type=int, default=540, help="seconds the child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unitigs"))
    ap.add_argument("--work", default=os.path.join(ROOT, "build", "unitigs"), help="scratch directory of the child's result file")
    a = ap.parse_args()
    os.makedirs(a.work, exist_ok=True)
    if a.child:
        return child(a.child, a)
    os.makedirs(a.out, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", "clean"] + sys.argv[1:]
    r = subprocess.run(cmd)
    if r.returncode != 0:
        raise SystemExit(f"the child ended with status {r.returncode}")
    out = json.load(open(os.path.join(a.work, "graph_clean_clean.json")))
    json.dump(out, open(os.path.join(a.out, "graph_clean.json"), "w"), indent=1)
    print(json.dumps(out[1:]))


if __name__ == "__main__":
    main()
