"""Read cleaning on the MI355X: Index.fix_reads_t against what a caller could compose before it existed.

  python scripts/gpu_readfix.py [--reads 1000000] [--genome 10000000] [--out profiles/readfix]

Two legs: --reads reads of 150 bases of either strand with 0.5 % and with 2 % substitutions. Per leg the index of the reads' own
23-mers is built on the device (count_distinct_t -> build_pf_codes_t -> build_23_codes_t); then, in one process on the same tensors,
  fused     2 warm-up + 7 timed whole calls of fix_reads_t (t = 1, V = 8, F = 4)
  baseline  composed_fix below, the same number of whole calls: coverage_t for the profile, torch operations for boundaries, cursors and
            counters, tf_codes_t on the 4 V candidate windows of every read that has a boundary, the fixes applied and the profile of the
            changed reads taken again, until no read changes
each on a fresh copy of the reads (the copy is outside the clock). Times are host clocks around a call that ends in a device synchronise:
median (min - max). The script asserts that reads, records and logs of the two are equal by SHA-256, and writes both times, their
ratio and the verdict of the rule "the fused kernel is kept only if its median is below the baseline's minimum on both legs" to
readfix.json, with reads/s, an upper estimate of probes/s (windows cut off by a read's end count as probed), the rate of tf_codes_t on
codes of the reads' own windows of either strand (found and absent alike, as the fused kernel meets them) and the useful share of lane
trips. Not measured: the absence-filter policies 1 and 2 of the fused kernel, hardware counters.

composed_fix works on any torch device through two callables, so tests/test_readfix_baseline_cpu.py checks it on the CPU against
tests/readfix_ref.py. It takes reads of one length that hold upper-case A/C/G/T only (what the legs generate)."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, before, warmup, reps):
    import torch
    ts = []
    for i in range(warmup + reps):
        before()
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append(time.perf_counter() - t)
    ts.sort()
    return {"median_ms": 1e3 * ts[len(ts) // 2], "min_ms": 1e3 * ts[0], "max_ms": 1e3 * ts[-1], "reps": reps}


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(t.cpu().numpy()).tobytes())
    return h.hexdigest()


MASK46 = (1 << 46) - 1


def composed_fix(reads, profile_fn, tf_codes_fn, t, V, F):
    """The rules of aix_reads_fix (include/aindex_hip.h) from calls that existed before it. reads: uint8 [n, L] of upper-case A/C/G/T,
    fixed in place. profile_fn(uint8 [a, L]) -> tf int64 [a, L - 22]; tf_codes_fn(int64 [m] codes) -> tf int64 [m].
    Returns (rec int32 [n, 8], fix_pos int32 [n, F], fix_old uint8 [n, F])."""
    import torch
    dev = reads.device
    n, L = reads.shape
    W = L - 22
    lut = torch.zeros(256, dtype=torch.int64, device=dev)
    letters = torch.tensor([65, 67, 71, 84], dtype=torch.uint8, device=dev)
    lut[letters.long()] = torch.arange(4, device=dev)
    c2 = lut[reads.long()]                                            # 2-bit values [n, L]
    shifts = 2 * (22 - torch.arange(23, device=dev))
    ar = torch.arange(W, device=dev)
    solid = profile_fn(reads) > t
    weak_before = W - solid.sum(1)
    phase = torch.zeros(n, dtype=torch.int64, device=dev)             # 0 = R, 1 = L, 2 = done
    cur = torch.ones(n, dtype=torch.int64, device=dev)
    fixes = torch.zeros(n, dtype=torch.int64, device=dev)
    n0, nM = torch.zeros_like(fixes), torch.zeros_like(fixes)
    fix_pos = torch.zeros((n, F), dtype=torch.int32, device=dev)
    fix_old = torch.zeros((n, F), dtype=torch.uint8, device=dev)
    false_col = torch.zeros((1, 1), dtype=torch.bool, device=dev)
    while True:
        phase[fixes >= F] = 2
        rows = torch.nonzero(phase < 2)[:, 0]
        if rows.numel() == 0:
            break
        S, c, ph = solid[rows], cur[rows], phase[rows]
        pad = false_col.expand(rows.numel(), 1)
        bR = torch.cat([pad, S[:, :-1] & ~S[:, 1:]], 1) & (ar[None, :] >= c[:, None])
        to_l = (ph == 0) & ~bR.any(1)                                  # phase R has no boundary left: phase L from the right end
        ph = torch.where(to_l, torch.ones_like(ph), ph)
        c = torch.where(to_l, torch.full_like(c, W - 2), c)
        bL = torch.cat([~S[:, :-1] & S[:, 1:], pad], 1) & (ar[None, :] <= c[:, None])
        done = (ph == 1) & ~bL.any(1)
        ph = torch.where(done, torch.full_like(ph, 2), ph)
        phase[rows], cur[rows] = ph, c
        i = torch.where(ph == 0, bR.int().argmax(1), W - 1 - bL.flip(1).int().argmax(1))
        go = ph < 2
        rows, i, ph = rows[go], i[go], ph[go]
        if rows.numel() == 0:
            continue
        p = torch.where(ph == 0, i + 22, i)
        lo = torch.where(ph == 0, i, (i - V + 1).clamp(min=0))
        hi = torch.where(ph == 0, (i + V - 1).clamp(max=W - 1), i)
        cnt = hi - lo + 1
        j = torch.arange(V, device=dev)
        w = (lo[:, None] + j[None, :]).clamp(max=W - 1)                # [a, V]; windows at or beyond cnt are masked below
        at = w[:, :, None] + torch.arange(23, device=dev)[None, None, :]
        vals = c2[rows[:, None, None], at]                             # [a, V, 23]
        here = at == p[:, None, None]
        cand = torch.stack([(torch.where(here, torch.full_like(vals, b), vals) << shifts).sum(2) for b in range(4)], 1)   # [a, 4, V]
        tf = tf_codes_fn(cand.reshape(-1)).view(-1, 4, V)
        ok = ((tf > t) | (j[None, None, :] >= cnt[:, None, None])).all(2)
        nok = ok.sum(1)
        fix = nok == 1
        fr, fp_, fb = rows[fix], p[fix], ok[fix].int().argmax(1)
        if fr.numel():
            k = fixes[fr]
            fix_pos[fr, k] = fp_.int()
            fix_old[fr, k] = reads[fr, fp_]
            reads[fr, fp_] = letters[fb]
            c2[fr, fp_] = fb
            fixes[fr] = k + 1
            solid[fr] = profile_fn(reads[fr]) > t                      # the profile of the changed reads, again
        bad = ~fix
        br = rows[bad]
        n0[br] += (nok[bad] == 0).long()
        nM[br] += (nok[bad] > 1).long()
        cur[br] = torch.where(ph[bad] == 0, i[bad] + 1, i[bad] - 1)
    weak_after = W - solid.sum(1)
    last_weak = torch.cummax(torch.where(solid, torch.full_like(ar, -1)[None, :], ar[None, :]), 1)[0]
    run = ar[None, :] - last_weak                                      # length of the solid run that ends at each window
    best, e = run.max(1)                                               # the first of equal maxima: the earliest run
    start = torch.where(best > 0, e - best + 1, torch.zeros_like(e))
    tlen = torch.where(best > 0, best + 22, torch.zeros_like(best))
    status = torch.where(weak_before == 0, 0, torch.where(weak_after == 0, 1, torch.where(fixes > 0, 2, 3)))
    rec = torch.stack([status, weak_before, weak_after, fixes, n0, nM, start, tlen], 1).to(torch.int32)
    return rec, fix_pos, fix_old


def leg(genome, n_reads, rate, seed):
    import torch
    from aindex_amd import _lib, builder, counting
    from aindex_amd.engine import Index, synth_reads_t
    clean = synth_reads_t(seed, genome, n_reads, 150, rc_half=True)                  # the truth, kept
    reads = clean.clone()
    gen = torch.Generator(device="cuda").manual_seed(seed)
    sub = torch.rand((n_reads, 150), device="cuda", generator=gen) < rate
    shift = torch.randint(1, 4, (n_reads, 150), device="cuda", generator=gen)
    code = torch.zeros(256, dtype=torch.int64, device="cuda")
    letters = torch.tensor([65, 67, 71, 84], dtype=torch.uint8, device="cuda")
    code[letters.long()] = torch.arange(4, device="cuda")
    body = reads.view(n_reads, 151)[:, :150]
    assert bool(torch.isin(body, letters).all()), "the legs need reads of upper-case A/C/G/T"
    body[sub] = letters[(code[body[sub].long()] + shift[sub]) % 4]
    keys, counts = counting.count_distinct_t(reads, 23, _lib.CANON_TRUE_RC)
    pf = builder.build_pf_codes_t(keys, 23)
    ix = Index.build_23_codes_t(pf, keys, counts.to(torch.int32))
    start = torch.arange(n_reads, dtype=torch.int64, device="cuda") * 151
    end = start + 150
    work = reads.clone()
    out = {}

    def fused():
        out["fused"] = ix.fix_reads_t(work, start, end, 1, 8, 4)

    res = {"substitution_rate": rate, "reads": n_reads, "planted": int(sub.sum()), "index_keys": int(keys.numel()),
           "fused": timed(fused, lambda: work.copy_(reads), 2, 7)}
    print("leg", rate, "fused", res["fused"], file=sys.stderr, flush=True)
    rec, fp, fo = out["fused"]
    fused_body = work.view(n_reads, 151)[:, :150].contiguous()
    res["sha256_fused"] = sha(fused_body, rec, fp, fo)

    # ---- the composition of the parent commit's public device calls, same process, same tensors ----
    orig_body = body.contiguous()
    bwork = orig_body.clone()

    def profile(x):
        a = x.shape[0]
        x = x.contiguous()
        offs = torch.arange(a + 1, dtype=torch.int64, device="cuda")
        return ix.coverage_t(x.view(-1), offs * 150, offs * 128, a * 128).view(a, 128).to(torch.int64) & 0xFFFFFFFF

    def tf_codes(c):
        return ix.tf_codes_t(c.contiguous()).to(torch.int64) & 0xFFFFFFFF

    def baseline():
        out["base"] = composed_fix(bwork, profile, tf_codes, 1, 8, 4)

    res["baseline"] = timed(baseline, lambda: bwork.copy_(orig_body), 2, 7)
    print("leg", rate, "baseline", res["baseline"], file=sys.stderr, flush=True)
    res["sha256_baseline"] = sha(bwork, *out["base"])
    assert res["sha256_fused"] == res["sha256_baseline"], "the fused call and the composition disagree"
    res["fused_median_over_baseline_min"] = res["fused"]["median_ms"] / res["baseline"]["min_ms"]
    res["fused_kept_by_the_rule"] = res["fused"]["median_ms"] < res["baseline"]["min_ms"]

    res["status"] = dict(zip(_lib.FIX_NAMES, torch.bincount(rec[:, 0].long(), minlength=7).tolist()))
    res["fixes"], res["n0"], res["nM"] = int(rec[:, 3].sum()), int(rec[:, 4].sum()), int(rec[:, 5].sum())
    truth = clean.view(n_reads, 151)[:, :150]
    res["planted_bytes_back_to_truth"] = int((fused_body[sub] == truth[sub]).sum())
    res["bytes_differing_from_truth_after"] = int((fused_body != truth).sum())
    res["reads_per_s"] = n_reads / (1e-3 * res["fused"]["median_ms"])
    # lane trips of the fused call: 2 profile trips per read (128 windows), one per try, one per re-probe (V = 8 < 23: every fix has one)
    tries = res["fixes"] + res["n0"] + res["nM"]
    trips = 2 * n_reads + tries + res["fixes"]
    useful = 128 * n_reads + tries * 3 * 8 + res["fixes"] * 15                # an upper estimate: windows cut by the read's end count as full
    res["lane_trips"], res["useful_lane_share_upper"] = trips, useful / (64 * trips)
    res["probes_per_s_upper"] = useful / (1e-3 * res["fused"]["median_ms"])
    # tf_codes_t on what the fused kernel probes most: the codes of the reads' own windows, as read (either strand, errors included)
    n_codes = 1 << 26
    rr = torch.randint(0, n_reads, (n_codes,), device="cuda", generator=gen)
    ww = torch.randint(0, 128, (n_codes,), device="cuda", generator=gen)
    c2 = code[orig_body.long()]
    codes = torch.zeros(n_codes, dtype=torch.int64, device="cuda")
    for k in range(23):
        codes = (codes << 2) | c2[rr, ww + k]
    tf_out = torch.empty(n_codes, dtype=torch.int32, device="cuda")
    res["tf_codes_t"] = timed(lambda: ix.tf_codes_t(codes, tf_out), lambda: None, 2, 7)
    res["tf_codes_per_s"] = n_codes / (1e-3 * res["tf_codes_t"]["median_ms"])
    res["share_of_tf_codes_rate_upper"] = res["probes_per_s_upper"] / res["tf_codes_per_s"]
    ix.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--genome", type=int, default=10_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "readfix"))
    a = ap.parse_args()
    import torch
    from aindex_amd.engine import synth_genome_t
    genome = synth_genome_t(11, a.genome)
    legs = [leg(genome, a.reads, rate, 100 + i) for i, rate in enumerate((0.005, 0.02))]
    doc = {"device": torch.cuda.get_device_name(0), "params": {"true_errors": 1, "verify": 8, "max_fixes": 4, "read_len": 150, "genome": a.genome},
           "legs": legs, "fused_kept_by_the_rule": all(l["fused_kept_by_the_rule"] for l in legs),
           "not_measured": ["absence-filter policies 1 and 2 of the fused kernel", "hardware counters"]}
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "readfix.json"), "w") as f:
        json.dump(doc, f, indent=1)
    for l in legs:
        print(json.dumps({k: l[k] for k in ("substitution_rate", "fused", "baseline", "fused_median_over_baseline_min", "reads_per_s", "fixes", "n0", "nM",
                                            "status", "tf_codes_per_s", "share_of_tf_codes_rate_upper", "useful_lane_share_upper")}))


if __name__ == "__main__":
    main()
