"""The unitig graph on the MI355X: Index.unitig_links_t (links, then bubbles) on the two indexes of scripts/gpu_unitigs.py.

  python scripts/gpu_unitig_links.py [--genome 50000000] [--out profiles/unitigs]

The driver starts one child process under a time limit. The child builds the clean index and the index of reads with 0.5 % substitutions,
makes the unitigs once, and times aix_unitig_links_dev and aix_unitig_bubbles_dev as whole calls (host clocks around calls that end in a
device synchronise: median and range of --reps runs after --warmup); it reports U, E, the histogram of end degrees and the number of
bubble arms. `--child trace` makes one call of each on every index: the program to put behind `rocprofv3 --kernel-trace --stats --` for
the per-kernel times (k_ug_check, k_ul_ends, k_ul_probe, rocPRIM's scan, k_ul_fill, k_ul_bubbles)."""
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
    from aindex_amd._lib import check, lib, vp
    from aindex_amd.engine import _stream_ptr
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)
        json.dump(lines, open(os.path.join(a.work, f"links_{kind}.json"), "w"), indent=1)

    idx = GD.build_indexes(a)
    emit({"leg": "indexes", **{k: int(v[0].n) for k, v in idx.items()}})
    for name, (ix, _) in idx.items():
        un = ix.unitigs_t(0)
        got = ix.unitig_links_t(0, unitigs=un)
        if kind == "trace":
            continue
        U, E = got["U"], got["E"]
        p = lambda t: vp(t.data_ptr())
        link_off, link_to, mate = torch.empty_like(got["link_off"]), torch.empty(8 * U, dtype=torch.int32, device="cuda"), torch.empty_like(got["bubble_mate"])
        e = C.c_uint64()
        links = lambda: check(lib().aix_unitig_links_dev(ix._h, 0, p(un["kid_unitig"]), p(un["kid_pos"]), p(un["kid_flag"]), U, p(un["offsets"]), p(link_off),
                                                         p(link_to), 8 * U, C.byref(e), _stream_ptr(ix.device)))
        bubbles = lambda: check(lib().aix_unitig_bubbles_dev(U, p(got["link_off"]), p(got["link_to"]), E, p(mate), _stream_ptr(ix.device)))
        tl = GD.timed(links, a.warmup, a.reps)
        tb = GD.timed(bubbles, a.warmup, a.reps)
        assert e.value == E and torch.equal(link_off, got["link_off"]) and torch.equal(link_to[:E], got["link_to"]) and torch.equal(mate, got["bubble_mate"])
        deg = got["link_off"][1:] - got["link_off"][:-1]
        emit({"leg": f"unitig_links_{name}", "keys": int(ix.n), "U": U, "E": E, "end_degree_histogram": torch.bincount(deg, minlength=5).tolist(),
              "bubble_arms": int((got["bubble_mate"] != -1).sum()), "links": tl, "bubbles": tb})
        del un, got, link_off, link_to, mate
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
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", "links"] + sys.argv[1:]
    r = subprocess.run(cmd)
    if r.returncode != 0:
        raise SystemExit(f"the child ended with status {r.returncode}")
    out = json.load(open(os.path.join(a.work, "links_links.json")))
    json.dump(out, open(os.path.join(a.out, "unitig_links.json"), "w"), indent=1)
    print(json.dumps(out[1:]))


if __name__ == "__main__":
    main()
