"""The phasing on the MI355X: Index.phase_observe_t, phase_bundle_t, phase_solve_t and phase_tag_t on reads of a synthetic diploid
genome, against a torch route for the observations.

  python scripts/gpu_phase.py [--genome 4000000] [--reads 800000] [--out profiles/phase]

The driver starts one child process under a time limit. The child draws, with torch on the device and by seed, haplotype A of --genome
bases in --contigs contigs, one site per roughly 200 bases (gaps of 100 to 300) where haplotype B shows another base, and --reads reads
of 150 bp: fragments of 400 bases from either haplotype at a random start, both mates on random strands (sequences 2 i and 2 i + 1),
0.5 % of the read bases substituted. Threading and placing are not timed and not run: a read without indels has one placement, its
own span, which is written down directly (what pile_place_t returns for such a read up to the ends it clips). The sites are what
pile_call_t would write for contigs that carry A's bases: ref = A's base, alt = B's. The handle only supplies the device: the index of
tests/golden/small23 is opened for it. Whole calls, host clocks around calls that end in a device synchronise: median and range of
--reps runs after --warmup. Legs, for group 1 (every read a fragment) and group 2 (pairs):
  phase_observe_t    with cap_hint = the larger total (so nothing is sized first)
  phase_bundle_t, phase_solve_t, phase_tag_t   each on the outputs of the one before
  torch_route        the observations and links alone, from the same placements (the route validates nothing): searchsorted of both
                     placement ends in the site positions, repeat_interleave, gathers of the read bytes, a sort by (fragment, site),
                     unique_consecutive. Its observations and links are compared with phase_observe_t's before anything is timed."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gpu_debruijn as GD  # noqa: E402  (the timer of the De Bruijn measurements)


def make_case(a):
    import torch
    g = torch.Generator(device="cuda").manual_seed(47)
    rnd = lambda hi, n, lo=0: torch.randint(lo, hi, (n,), generator=g, device="cuda")
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    U, Lc = a.contigs, a.genome // a.contigs
    B = U * Lc
    code_a = rnd(4, B)
    gaps = rnd(301, B // 100, 100)
    g_site = torch.cumsum(gaps, 0)
    g_site = g_site[g_site < B]
    code_b = code_a.clone()
    code_b[g_site] = (code_a[g_site] + rnd(4, g_site.numel(), 1)) % 4
    offsets = torch.arange(U + 1, dtype=torch.int64, device="cuda") * Lc
    vu = g_site // Lc
    sites = {"var_unitig": vu.int(), "var_pos": (g_site - vu * Lc).int(), "var_ref": acgt[code_a[g_site]], "var_alt": acgt[code_b[g_site]]}
    F = a.reads // 2
    fu, fx, fh = rnd(U, F), rnd(Lc - 400 + 1, F), rnd(2, F)
    start = (fu * Lc + fx).repeat_interleave(2) + torch.tensor([0, 250], device="cuda").repeat(F)       # the mates: bases 0 .. 149 and 250 .. 399
    hap, back = fh.repeat_interleave(2), rnd(2, 2 * F)
    M = 2 * F
    col = torch.arange(150, device="cuda")
    gb = start[:, None] + torch.where(back[:, None].bool(), 149 - col[None, :], col[None, :])
    code = torch.where(hap[:, None].bool(), code_b[gb], code_a[gb])
    code = torch.where(torch.rand((M, 150), generator=g, device="cuda") < 0.005, (code + rnd(4, M * 150, 1).view(M, 150)) % 4, code)
    code = torch.where(back[:, None].bool(), 3 - code, code)
    flat = acgt[code].reshape(-1).contiguous()
    offs = torch.arange(M + 1, dtype=torch.int64, device="cuda") * 150
    su = start // Lc
    places = {"seq_place_off": torch.arange(M + 1, dtype=torch.int64, device="cuda"), "place_unitig": su.int(), "place_flag": back.to(torch.uint8),
              "place_pos": (start - su * Lc).int(), "place_q0": torch.zeros(M, dtype=torch.int32, device="cuda"),
              "place_len": torch.full((M,), 150, dtype=torch.int32, device="cuda")}
    return {"offsets": offsets}, flat, offs, places, sites, g_site


def route(flat, offs, places, sites, g_site, offsets, group):
    """-> frag_obs_off, obs_site, obs_allele, link_lo, link_hi, link_rel as int64 / uint8 tensors"""
    import torch
    spo, pu, pf, pp, pq, pl = (places[k] for k in ("seq_place_off", "place_unitig", "place_flag", "place_pos", "place_q0", "place_len"))
    M, R, V = offs.numel() - 1, pu.numel(), g_site.numel()
    ln = pl.long()
    g0 = offsets[pu.long()] + pp.long()
    lo, hi = torch.searchsorted(g_site, g0), torch.searchsorted(g_site, g0 + ln)
    cnt = hi - lo
    r = torch.repeat_interleave(torch.arange(R, device="cuda"), cnt)
    v = lo[r] + torch.arange(r.numel(), device="cuda") - (torch.cumsum(cnt, 0) - cnt)[r]
    x = g_site[v] - g0[r]
    back = (pf[r] & 1).bool()
    seq = torch.repeat_interleave(torch.arange(M, device="cuda"), spo[1:] - spo[:-1])
    c = flat[(offs[seq] + pq.long())[r] + torch.where(back, ln[r] - 1 - x, x)]
    comp = torch.arange(256, dtype=torch.uint8, device="cuda")
    comp[[65, 67, 71, 84]] = torch.tensor([84, 71, 67, 65], dtype=torch.uint8, device="cuda")
    c = torch.where(back, comp[c.long()], c)
    allele = torch.where(c == sites["var_ref"][v], 0, torch.where(c == sites["var_alt"][v], 1, 2))
    key, order = torch.sort(((seq[r] // group) << 32) | v)
    ukey, inv = torch.unique_consecutive(key, return_inverse=True)
    has = torch.zeros((ukey.numel(), 3), dtype=torch.bool, device="cuda")
    has[inv, allele[order]] = True
    keep = (has[:, 0] ^ has[:, 1]) & ~has[:, 2]
    okey, oall = ukey[keep], has[keep, 1].to(torch.uint8)
    frag, site = okey >> 32, okey & 0xFFFFFFFF
    foff = torch.searchsorted(frag, torch.arange(M // group + 1, device="cuda"))
    vu = sites["var_unitig"]
    link = (frag[1:] == frag[:-1]) & (vu[site[1:]] == vu[site[:-1]])
    return foff, site, oall, site[:-1][link], site[1:][link], (oall[1:] ^ oall[:-1])[link]


def child(a):
    import torch
    sys.path.insert(0, ROOT)
    from aindex_amd.engine import Index
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)
        json.dump(lines, open(os.path.join(a.work, "phase.json"), "w"), indent=1)

    prefix = os.path.join(ROOT, "tests", "golden", "small23", "small23")
    with Index.open_23(prefix + ".pf", prefix + ".tf.bin", prefix + ".kmers.bin", device=0) as ix:
        graph, flat, offs, places, sites, g_site = make_case(a)
        V = g_site.numel()
        for group in (1, 2):
            obs = ix.phase_observe_t(graph, flat, offs, places, sites, group)
            hint = max(obs["n_obs"], obs["n_links"])
            edges = ix.phase_bundle_t(V, obs)
            solved = ix.phase_solve_t(sites, edges)
            tags = ix.phase_tag_t(obs, solved)
            res = {"leg": f"phase_group{group}", "reads": offs.numel() - 1, "read_bases": flat.numel(), "contigs": a.contigs, "contig_bases": int(graph["offsets"][-1]),
                   "V": V, "stats": obs["stats"], "raw_observations": obs["stats"][0], "observations": obs["n_obs"], "links": obs["n_links"],
                   "edges": edges["n_edges"], "jumping_rounds": max(V - 1, 0).bit_length(), "counts": solved["counts"],
                   "tagged_fragments": int((tags["tag_block"] != -1).sum())}
            got = route(flat, offs, places, sites, g_site, graph["offsets"], group)
            mine = [obs[k].long() if obs[k].dtype != torch.uint8 else obs[k] for k in ("frag_obs_off", "obs_site", "obs_allele", "link_lo", "link_hi", "link_rel")]
            res["torch_route_equal"] = bool(all(torch.equal(x, y) for x, y in zip(got, mine)))
            res["phase_observe_t"] = GD.timed(lambda: ix.phase_observe_t(graph, flat, offs, places, sites, group, hint), a.warmup, a.reps)
            res["phase_bundle_t"] = GD.timed(lambda: ix.phase_bundle_t(V, obs), a.warmup, a.reps)
            res["phase_solve_t"] = GD.timed(lambda: ix.phase_solve_t(sites, edges), a.warmup, a.reps)
            res["phase_tag_t"] = GD.timed(lambda: ix.phase_tag_t(obs, solved), a.warmup, a.reps)
            res["torch_route"] = GD.timed(lambda: route(flat, offs, places, sites, g_site, graph["offsets"], group), a.warmup, a.reps)
            res["torch_route_over_phase_observe_t"] = res["torch_route"]["median_ms"] / res["phase_observe_t"]["median_ms"]
            emit(res)
        torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--genome", type=int, default=4_000_000, help="bases of one haplotype (800 000 reads of 150 bp cover it 30 times)")
    ap.add_argument("--contigs", type=int, default=64)
    ap.add_argument("--reads", type=int, default=800_000, help="reads of 150 bp, two per fragment")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--limit", type=int, default=300, help="seconds the child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "phase"))
    ap.add_argument("--work", default=os.path.join(ROOT, "build", "phase"), help="scratch directory of the child's result file")
    a = ap.parse_args()
    os.makedirs(a.work, exist_ok=True)
    if a.child:
        return child(a)
    os.makedirs(a.out, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:]
    r = subprocess.run(cmd)
    if r.returncode != 0:
        raise SystemExit(f"the child ended with status {r.returncode}")
    out = json.load(open(os.path.join(a.work, "phase.json")))
    json.dump(out, open(os.path.join(a.out, "phase.json"), "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
