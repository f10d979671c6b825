// aix_pileup.hip — reads piled onto the contigs they thread through: the steps of aix_seq_thread_dev merged into placements (one per
// run of steps on one diagonal of one contig), the bases of every placement counted per contig base and channel, and the counts read out
// as polished bases, variant sites and per-contig depth. The contract is stated above the declarations in include/aindex_hip.h; DESIGN 5p
// has the derivations and the resources. What the graph files share is in aix_graph.hpp, what this file shares with aix_phase.hip in
// aix_pile.hpp. Integer only, no LDS, no grid-wide barrier, no spin-wait; one plain launch per step:
//   aix_pile_place_dev
//     validate k_pl_place_validate: one lane per sequence, per step and per contig; nothing below runs on arrays that fail it
//     heads    k_pl_heads: one lane per step: head[t] = the step is linear and does not merge with step t - 1; circular steps are counted
//     scan     rank[t] = heads in front of step t; rank[T] = the number of placements; seq_place_off[i] = rank[seq_step_off[i]]
//     write    k_pl_write: the head lane walks to the end of its run, finds its neighbours, extends and writes the record
//   aix_pileup_dev
//     validate k_pl_pile_validate (sequences, CSR, placements, contig offsets), then k_pl_bases_check (the contig bytes)
//     edges    k_pl_edges: one lane per placement: +1 / -1 into the zeroed difference array at its two ends (two atomics), and the
//              placement's first read byte and first contig base for the next pass; a scan of the lengths gives the flat base space
//     bases    k_pl_bases: one lane per read base, consecutive lanes on consecutive bases; only a base that differs from the contig's
//              issues atomics (+1 alternative channel, -1 contig channel; another byte only -1)
//     scan     depth[g] = diff[0] + .. + diff[g]
//     apply    k_pl_apply: one lane per contig base: counts[4 g + code of the contig base] += depth[g], one 16-byte load and store
//   aix_pile_call_dev
//     validate the contig offsets, then k_pl_call_flag: the contig bytes, and vflag[g] = base g is a variant site (scratch only)
//     select   the flagged g in ascending order (rocPRIM), when the caller asked for variants
//     write    k_pl_call_write: polished bases, changed count, depth_sum and uncovered per contig; k_pl_call_vars: one lane per variant
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "aix_pile.hpp"
#include "aix_seqhits.hpp"

namespace aix {

struct PlCounters {                                               // one zeroed record per call
    unsigned long long bad, a, b, c;                              // a, b, c: circular steps | counted, other, mismatches | variants, changed
};

struct PlThr {
    uint32_t min_depth, min_major_permille, min_alt_count, min_alt_permille;
};

// A, C, G, T -> 0 .. 3 (bits 2 .. 1 of the byte are 0, 1, 3, 2)
__device__ __forceinline__ uint32_t pl_code(uint32_t c) { const uint32_t x = (c >> 1) & 3u; return x ^ (x >> 1); }

// ---------------------------------------------------------------------------------------------
// 1. steps -> placements
// ---------------------------------------------------------------------------------------------
struct PlSteps {
    uint64_t M, T, U;
    const uint64_t *offs, *sso;
    const uint32_t *unitig, *pos;
    const uint8_t* flag;
    const uint32_t *q_first, *q_last;
    const uint64_t* offsets;
};

__global__ void __launch_bounds__(kCB) k_pl_place_validate(const PlSteps g, PlCounters* __restrict__ ctr) {
    const uint64_t work = std::max(std::max(g.M, g.U) + 1, g.T), stride = (uint64_t)gridDim.x * kCB;
    unsigned long long bad = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kCB + threadIdx.x; i < work; i += stride) {
        bad += pl_frame_bad(i, g.M, g.offs, g.sso, g.T, g.U, g.offsets);
        if (i >= g.T) continue;
        uint64_t j, lo, hi;
        if (!pl_seq_of(g.sso, g.M, i, j, lo, hi)) { ++bad; continue; }
        const uint64_t sa = g.offs[j], sb = g.offs[j + 1], u = g.unitig[i], p = g.pos[i], a = g.q_first[i], b = g.q_last[i];
        if (sb < sa || u >= g.U || a > b || b + 23 > sb - sa) { ++bad; continue; }
        const uint64_t ulo = g.offsets[u], uhi = g.offsets[u + 1];
        if (span_bad(ulo, uhi)) { ++bad; continue; }
        const uint64_t m = uhi - ulo - 22, f = g.flag[i];
        if (!(f & 2u)) bad += (f & 1u) ? !(b - a <= p && p < m) : !(p + (b - a) < m);
        if (i > lo) bad += a <= (uint64_t)g.q_last[i - 1];
    }
    count_add(bad, &ctr->bad);
}

// the diagonal of linear step t: read base j lies on contig base d + j (forwards) or d - j (backwards)
__device__ __forceinline__ long long pl_diag(const PlSteps& g, uint64_t t) {
    const long long p = g.pos[t], a = g.q_first[t];
    return (g.flag[t] & 1u) ? p + a + 22 : p - a;
}

__global__ void __launch_bounds__(kCB) k_pl_heads(const PlSteps g, uint32_t max_gap, uint8_t* __restrict__ head, PlCounters* __restrict__ ctr) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    unsigned long long circ = 0;
    for (uint64_t t = (uint64_t)blockIdx.x * kCB + threadIdx.x; t <= g.T; t += stride) {
        bool hd = false;
        if (t < g.T) {
            const uint32_t f = g.flag[t];
            if (f & 2u) ++circ;
            else {
                hd = true;
                uint64_t j, lo, hi;
                if (pl_seq_of(g.sso, g.M, t, j, lo, hi) && t > lo) {
                    const uint32_t pf = g.flag[t - 1];
                    if (!(pf & 2u) && ((pf ^ f) & 1u) == 0 && g.unitig[t - 1] == g.unitig[t] && pl_diag(g, t - 1) == pl_diag(g, t) &&
                        (uint64_t)g.q_first[t] - g.q_last[t - 1] - 1 <= max_gap)
                        hd = false;
                }
            }
        }
        head[t] = hd ? 1 : 0;                                     // head[T] = 0: the scan's last entry is the total
    }
    count_add(circ, &ctr->a);
}

__global__ void __launch_bounds__(kCB) k_pl_seqoff(const uint64_t* __restrict__ csr, const uint64_t* __restrict__ rank, uint64_t M, uint64_t* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t i = (uint64_t)blockIdx.x * kCB + threadIdx.x; i <= M; i += stride) out[i] = rank[csr[i]];
}

struct PlPlaceOut {
    uint32_t* unitig;
    uint8_t* flag;
    uint32_t *pos, *q0, *len, *steps;
};

__device__ __forceinline__ long long pl_min(long long a, long long b) { return a < b ? a : b; }

__global__ void __launch_bounds__(kCB) k_pl_write(const PlSteps g, const uint8_t* __restrict__ head, const uint64_t* __restrict__ rank, uint32_t extend,
                                                 const PlPlaceOut o) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t t = (uint64_t)blockIdx.x * kCB + threadIdx.x; t < g.T; t += stride) {
        if (!head[t]) continue;
        uint64_t j, lo, hi;
        if (!pl_seq_of(g.sso, g.M, t, j, lo, hi)) continue;      // (never: the arrays passed the validation)
        uint64_t e = t;                                           // the last step of the run
        while (e + 1 < hi && !head[e + 1] && !(g.flag[e + 1] & 2u)) ++e;
        const uint64_t u = g.unitig[t];
        const uint32_t s = g.flag[t] & 1u;
        const long long d = pl_diag(g, t), a = g.q_first[t], last = (long long)g.q_last[e] + 22;      // the core: read bases [a, last]
        const long long L = (long long)(g.offs[j + 1] - g.offs[j]), Lu = (long long)(g.offsets[u + 1] - g.offsets[u]);
        long long left = pl_min(pl_min(extend, a), s ? Lu - 1 - (d - a) : d + a);
        long long right = pl_min(pl_min(extend, L - 1 - last), s ? d - last : Lu - 1 - (d + last));
        uint64_t p = t;                                           // the placement before: its last step is the last linear step in front of t
        while (p > lo && (g.flag[p - 1] & 2u)) --p;
        if (p > lo) left = pl_min(left, a - ((long long)g.q_last[p - 1] + 22) - 1);
        uint64_t n = e + 1;                                       // the placement after: its first step is the first linear step behind e
        while (n < hi && (g.flag[n] & 2u)) ++n;
        if (n < hi) right = pl_min(right, (long long)g.q_first[n] - last - 1);
        const long long q0 = a - (left > 0 ? left : 0), q1 = last + (right > 0 ? right : 0);
        const uint64_t r = rank[t];
        o.unitig[r] = (uint32_t)u;
        o.flag[r] = (uint8_t)s;
        o.pos[r] = (uint32_t)(s ? d - q1 : d + q0);
        o.q0[r] = (uint32_t)q0;
        o.len[r] = (uint32_t)(q1 - q0 + 1);
        o.steps[r] = (uint32_t)(e - t + 1);
    }
}

// Validation, then the placements. *n_place, *n_circ. Synchronises `s`; AIX_ERR_ARG (as hipErrorInvalidValue -> *bad) before anything is written.
static hipError_t pl_place(const PlSteps& g, uint32_t max_gap, uint32_t extend, uint64_t* d_seq_place_off, const PlPlaceOut& o, uint64_t* n_place, uint64_t* n_circ,
                           bool* bad, hipStream_t s) {
    const uint64_t cap = chain_test_grid();
    const dim3 blk(kCB);
    Counted<PlCounters> ctr(s);
    DevArr head(s), rank(s), tmp(s);
    AIX_TRY(ctr.init());
    AIX_TRY(ctr.run([&]() {
        AIX_TRY_LAUNCH(k_pl_place_validate, dim3(chain_grid(std::max(std::max(g.M, g.U) + 1, g.T), 2 * kCB, cap)), blk, 0, s, g, ctr.dev());
        return hipSuccess;
    }));
    *bad = ctr.host.bad != 0;
    *n_place = *n_circ = 0;
    if (*bad) return hipSuccess;
    if (g.T == 0) return zero_offsets(d_seq_place_off, g.M, s);
    AIX_TRY(sh_alloc(head, g.T + 1, 1));
    AIX_TRY(sh_alloc(rank, g.T + 1, 8));
    uint64_t total = 0;
    AIX_TRY(ctr.run([&]() {
        AIX_TRY_LAUNCH(k_pl_heads, dim3(chain_grid(g.T + 1, 2 * kCB, cap)), blk, 0, s, g, max_gap, (uint8_t*)head.p, ctr.dev());
        AIX_TRY(scan_u64(rocprim::make_transform_iterator((const uint8_t*)head.p, Widen<uint8_t>()), (uint64_t*)rank.p, g.T + 1, tmp, s));
        AIX_TRY_LAUNCH(k_pl_seqoff, dim3(chain_grid(g.M + 1, 4 * kCB, cap)), blk, 0, s, g.sso, (const uint64_t*)rank.p, g.M, d_seq_place_off);
        AIX_TRY_LAUNCH(k_pl_write, dim3(chain_grid(g.T, 2 * kCB, cap)), blk, 0, s, g, (const uint8_t*)head.p, (const uint64_t*)rank.p, extend, o);
        return hipMemcpyAsync(&total, (const uint64_t*)rank.p + g.T, 8, hipMemcpyDeviceToHost, s);
    }));
    *n_place = total;
    *n_circ = ctr.host.a;
    return hipSuccess;
}

// ---------------------------------------------------------------------------------------------
// 2. placements and read bytes -> counts
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kCB) k_pl_pile_validate(const PlPlaces g, PlCounters* __restrict__ ctr) {
    const uint64_t work = std::max(std::max(g.M, g.U) + 1, g.R), stride = (uint64_t)gridDim.x * kCB;
    unsigned long long bad = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kCB + threadIdx.x; i < work; i += stride) bad += pl_places_bad(g, i);
    count_add(bad, &ctr->bad);
}

// every contig byte is an upper-case A, C, G or T
__global__ void __launch_bounds__(kCB) k_pl_bases_check(uint64_t B, const uint8_t* __restrict__ bases, PlCounters* __restrict__ ctr) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    unsigned long long bad = 0;
    for (uint64_t g = (uint64_t)blockIdx.x * kCB + threadIdx.x; g < B; g += stride) bad += !pl_is_base(bases[g]);
    count_add(bad, &ctr->bad);
}

// lane r < R: the two ends of placement r in the difference array; len64[r] for the scan (len64[R] = 0: the scan's last entry is the
// total); rd0[r] the index in seqs of its first read byte; gs[r] = the contig base of that byte << 1 | backwards
__global__ void __launch_bounds__(kCB) k_pl_edges(const PlPlaces g, uint32_t* __restrict__ diff, uint64_t* __restrict__ len64, uint64_t* __restrict__ rd0,
                                                 uint64_t* __restrict__ gs) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t r = (uint64_t)blockIdx.x * kCB + threadIdx.x; r <= g.R; r += stride) {
        if (r == g.R) { len64[r] = 0; continue; }
        uint64_t j, lo, hi;
        if (!pl_seq_of(g.spo, g.M, r, j, lo, hi)) { len64[r] = 0; continue; }      // (never: the arrays passed the validation)
        const uint64_t len = g.len[r], g0 = g.offsets[g.unitig[r]] + g.pos[r], s = g.flag[r] & 1u;
        atomicAdd(diff + g0, 1u);
        atomicAdd(diff + g0 + len, 0xFFFFFFFFu);
        len64[r] = len;
        rd0[r] = g.offs[j] + g.q0[r];
        gs[r] = ((s ? g0 + len - 1 : g0) << 1) | s;
    }
}

// One lane per read base of the flat space poff[R]: base i belongs to the last placement r with poff[r] <= i. The wave's first base is
// searched by bisection (the same addresses in every lane), every lane gallops from there. The cost, not a precondition: a placement that
// aix_pile_place_dev made holds 23 bases or more, so a wave meets at most three and the gallop ends after a step or two. Shorter ones (the
// validation admits len >= 1) only make it longer: poff ascends strictly, so the last r with poff[r] <= i is found whatever the lengths.
__global__ void __launch_bounds__(kCB) k_pl_bases(uint64_t R, const uint64_t* __restrict__ poff, const uint64_t* __restrict__ rd0, const uint64_t* __restrict__ gs,
                                                 const uint8_t* __restrict__ seqs, const uint8_t* __restrict__ bases, uint32_t* __restrict__ counts,
                                                 uint32_t* __restrict__ place_mism, PlCounters* __restrict__ ctr) {
    const uint64_t total = poff[R], stride = (uint64_t)gridDim.x * kCB;
    unsigned long long counted = 0, other = 0, mism = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * kCB + (threadIdx.x & ~63u); base < total; base += stride) {      // wave-uniform
        const uint64_t i = base + (threadIdx.x & 63u);
        if (i >= total) continue;
        const uint64_t r0 = last_le(poff, 0, R, base);
        const uint64_t r = gallop_last_le(poff, R, r0, i);       // poff[R] == total > i; an empty placement is never the last one <= i
        const uint64_t x = i - poff[r], w = gs[r], back = w & 1u, g = back ? (w >> 1) - x : (w >> 1) + x;
        const uint32_t c = seqs[rd0[r] + x], rc = pl_code(bases[g]);
        if (!pl_is_base(c)) {
            ++other;
            atomicSub(counts + 4 * g + rc, 1u);
            continue;
        }
        ++counted;
        const uint32_t code = back ? 3u - pl_code(c) : pl_code(c);
        if (code != rc) {
            ++mism;
            atomicAdd(counts + 4 * g + code, 1u);
            atomicSub(counts + 4 * g + rc, 1u);
            if (place_mism) atomicAdd(place_mism + r, 1u);
        }
    }
    count_add(counted, &ctr->a);
    count_add(other, &ctr->b);
    count_add(mism, &ctr->c);
}

// counts[4 g + code of the contig base] += depth[g]: the cell is one aligned 16-byte word
__global__ void __launch_bounds__(kCB) k_pl_apply(uint64_t B, const uint32_t* __restrict__ depth, const uint8_t* __restrict__ bases, uint4* __restrict__ cells) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t g = (uint64_t)blockIdx.x * kCB + threadIdx.x; g < B; g += stride) {
        const uint32_t d = depth[g];
        if (d == 0) continue;
        const uint32_t rc = pl_code(bases[g]);
        uint4 c = cells[g];
        c.x += rc == 0 ? d : 0;
        c.y += rc == 1 ? d : 0;
        c.z += rc == 2 ? d : 0;
        c.w += rc == 3 ? d : 0;
        cells[g] = c;
    }
}

// the contig offsets of a call without placements (aix_pile_call_dev)
__global__ void __launch_bounds__(kCB) k_pl_offsets_validate(uint64_t U, const uint64_t* __restrict__ offsets, PlCounters* __restrict__ ctr) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    unsigned long long bad = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kCB + threadIdx.x; i <= U; i += stride) bad += pl_frame_bad(i, 0, nullptr, nullptr, 0, U, offsets);
    count_add(bad, &ctr->bad);
}

// ---------------------------------------------------------------------------------------------
// 3. counts -> polished bases, variant sites, depth
// ---------------------------------------------------------------------------------------------
struct PlSite {
    uint32_t r, alt, c_ref, c_alt;
    uint64_t D;
    bool polish, variant;
};

__device__ __forceinline__ PlSite pl_site(const uint4 cell, uint32_t r, const PlThr& th) {
    const uint32_t c[4] = {cell.x, cell.y, cell.z, cell.w};
    PlSite s;
    s.r = r;
    s.D = (uint64_t)c[0] + c[1] + c[2] + c[3];
    s.alt = r == 0 ? 1u : 0u;
#pragma unroll
    for (uint32_t x = 0; x < 4; ++x)
        if (x != r && c[x] > c[s.alt]) s.alt = x;                 // ascending x and a strict comparison: ties go to the smaller code
    s.c_ref = c[r];
    s.c_alt = c[s.alt];
    const uint64_t a1000 = 1000ull * s.c_alt;
    const bool deep = s.D >= th.min_depth;
    s.polish = deep && s.c_alt > s.c_ref && pl_reaches(a1000, th.min_major_permille, s.D);
    s.variant = deep && s.c_alt >= th.min_alt_count && pl_reaches(a1000, th.min_alt_permille, s.D);
    return s;
}

// the contig bytes are checked; vflag (nullable) takes "base g is a variant site". A byte that is no base has no site: the call is refused.
__global__ void __launch_bounds__(kCB) k_pl_call_flag(uint64_t B, const uint8_t* __restrict__ bases, const uint4* __restrict__ cells, const PlThr th,
                                                     uint8_t* __restrict__ vflag, PlCounters* __restrict__ ctr) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    unsigned long long bad = 0, nvar = 0;
    for (uint64_t g = (uint64_t)blockIdx.x * kCB + threadIdx.x; g < B; g += stride) {
        const uint32_t c = bases[g];
        const bool ok = pl_is_base(c);
        bad += !ok;
        if (!vflag) continue;
        const bool v = ok && pl_site(cells[g], pl_code(c), th).variant;
        vflag[g] = v ? 1 : 0;
        nvar += v;
    }
    count_add(bad, &ctr->bad);
    count_add(nvar, &ctr->a);
}

// polished (nullable), the changed count, depth_sum and uncovered (nullable, zeroed by the caller). The contig of base g: bisection for the
// wave's first base, a gallop from there. A wave inside one contig adds its sums with one atomic each.
__global__ void __launch_bounds__(kCB) k_pl_call_write(uint64_t B, uint64_t U, const uint64_t* __restrict__ offsets, const uint8_t* __restrict__ bases,
                                                      const uint4* __restrict__ cells, const PlThr th, uint8_t* __restrict__ polished,
                                                      unsigned long long* __restrict__ depth_sum, uint32_t* __restrict__ uncovered, PlCounters* __restrict__ ctr) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    const bool per_contig = depth_sum || uncovered;
    unsigned long long changed = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * kCB + (threadIdx.x & ~63u); base < B; base += stride) {          // wave-uniform
        const uint64_t g = base + (threadIdx.x & 63u);
        const bool in = g < B;
        unsigned long long D = 0, zero = 0;
        if (in) {
            const uint32_t c = bases[g];
            const PlSite s = pl_site(cells[g], pl_code(c), th);
            if (polished) polished[g] = s.polish ? (uint8_t)"ACGT"[s.alt] : (uint8_t)c;
            changed += s.polish;
            D = s.D;
            zero = s.D == 0;
        }
        if (!per_contig) continue;
        const uint64_t last = base + 63 < B ? base + 63 : B - 1;
        const uint64_t u0 = last_le(offsets, 0, U, base);        // offsets[0] == 0 <= base < B == offsets[U]
        if (offsets[u0 + 1] > last) {                             // the whole wave lies in contig u0
            const unsigned long long sd = wave_sum(D), sz = wave_sum(zero);
            if ((threadIdx.x & 63u) == 0) {
                if (depth_sum && sd) atomicAdd(depth_sum + u0, sd);
                if (uncovered && sz) atomicAdd(uncovered + u0, (uint32_t)sz);
            }
        } else if (in) {
            const uint64_t u = gallop_last_le(offsets, U, u0, g);
            if (depth_sum && D) atomicAdd(depth_sum + u, D);
            if (uncovered && zero) atomicAdd(uncovered + u, 1u);
        }
    }
    count_add(changed, &ctr->b);
}

struct PlVarOut {
    uint32_t *unitig, *pos;
    uint8_t *ref, *alt;
    uint32_t *ref_count, *alt_count, *depth;
    uint64_t cap;
};

__global__ void __launch_bounds__(kCB) k_pl_call_vars(uint64_t n, const uint64_t* __restrict__ sel, uint64_t U, const uint64_t* __restrict__ offsets,
                                                     const uint8_t* __restrict__ bases, const uint4* __restrict__ cells, const PlThr th, const PlVarOut o) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t i = (uint64_t)blockIdx.x * kCB + threadIdx.x; i < n && i < o.cap; i += stride) {
        const uint64_t g = sel[i], u = last_le(offsets, 0, U, g);
        const uint32_t c = bases[g];
        const PlSite s = pl_site(cells[g], pl_code(c), th);
        o.unitig[i] = (uint32_t)u;
        o.pos[i] = (uint32_t)(g - offsets[u]);
        o.ref[i] = (uint8_t)c;
        o.alt[i] = (uint8_t)"ACGT"[s.alt];
        o.ref_count[i] = s.c_ref;
        o.alt_count[i] = s.c_alt;
        o.depth[i] = s.D > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)s.D;
    }
}

}  // namespace aix

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" int aix_pile_place_dev(uint64_t M, const uint64_t* d_offs, const uint64_t* d_seq_step_off, uint64_t T, const uint32_t* d_step_unitig,
                                  const uint32_t* d_step_pos, const uint8_t* d_step_flag, const uint32_t* d_q_first, const uint32_t* d_q_last, uint64_t U,
                                  const uint64_t* d_offsets, uint32_t max_gap, uint32_t extend, uint64_t* d_seq_place_off, uint32_t* d_place_unitig,
                                  uint8_t* d_place_flag, uint32_t* d_place_pos, uint32_t* d_place_q0, uint32_t* d_place_len, uint32_t* d_place_steps,
                                  uint64_t* n_place_out, uint64_t* n_circular_steps_out, void* stream) {
    if (U > kUnitLimit) return AIX_ERR_UNSUPPORTED;
    if (!d_offsets || !d_seq_place_off || !n_place_out || M >= (1ull << 56) || T >= (1ull << 56)) return AIX_ERR_ARG;
    if (M && (!d_offs || !d_seq_step_off)) return AIX_ERR_ARG;
    if (T && (!M || !d_step_unitig || !d_step_pos || !d_step_flag || !d_q_first || !d_q_last)) return AIX_ERR_ARG;
    if (T && (!d_place_unitig || !d_place_flag || !d_place_pos || !d_place_q0 || !d_place_len || !d_place_steps)) return AIX_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    uint64_t n_place = 0, n_circ = 0;
    if (M == 0) {
        AIXCHK(zero_offsets(d_seq_place_off, 0, s));
    } else {
        const PlSteps g{M, T, U, d_offs, d_seq_step_off, d_step_unitig, d_step_pos, d_step_flag, d_q_first, d_q_last, d_offsets};
        const PlPlaceOut o{d_place_unitig, d_place_flag, d_place_pos, d_place_q0, d_place_len, d_place_steps};
        bool bad = false;
        AIXCHK(pl_place(g, max_gap, extend, d_seq_place_off, o, &n_place, &n_circ, &bad, s));
        if (bad) return AIX_ERR_ARG;
    }
    *n_place_out = n_place;
    if (n_circular_steps_out) *n_circular_steps_out = n_circ;
    return AIX_OK;
}

extern "C" int aix_pileup_dev(const char* d_seqs, const uint64_t* d_offs, uint64_t M, const uint64_t* d_seq_place_off, uint64_t R, const uint32_t* d_place_unitig,
                              const uint8_t* d_place_flag, const uint32_t* d_place_pos, const uint32_t* d_place_q0, const uint32_t* d_place_len, uint64_t U,
                              const uint64_t* d_offsets, const uint8_t* d_bases, uint32_t* d_counts, uint32_t* d_place_mism, uint64_t* d_stats, void* stream) {
    if (U > kUnitLimit) return AIX_ERR_UNSUPPORTED;
    if (!d_offsets || M >= (1ull << 56) || R >= (1ull << 56) || ((uintptr_t)d_counts & 15u)) return AIX_ERR_ARG;
    if (M && (!d_offs || !d_seq_place_off)) return AIX_ERR_ARG;
    if (U && (!d_bases || !d_counts)) return AIX_ERR_ARG;
    if (R && (!M || !U || !d_seqs || !d_place_unitig || !d_place_flag || !d_place_pos || !d_place_q0 || !d_place_len)) return AIX_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const uint64_t cap = chain_test_grid();
    const dim3 blk(kCB);
    const PlPlaces g{M, R, U, d_offs, d_seq_place_off, d_place_unitig, d_place_flag, d_place_pos, d_place_q0, d_place_len, d_offsets};
    Counted<PlCounters> ctr(s);
    AIXCHK(ctr.init());
    uint64_t B = 0;
    AIXCHK(ctr.run([&]() {
        AIX_TRY_LAUNCH(k_pl_pile_validate, dim3(chain_grid(std::max(std::max(M, U) + 1, R), 2 * kCB, cap)), blk, 0, s, g, ctr.dev());
        return hipMemcpyAsync(&B, d_offsets + U, 8, hipMemcpyDeviceToHost, s);
    }));
    if (ctr.host.bad || B >= (1ull << 60)) return AIX_ERR_ARG;
    AIXCHK(ctr.run([&]() {
        AIX_TRY_LAUNCH(k_pl_bases_check, dim3(chain_grid(B, 16 * kCB, cap)), blk, 0, s, B, d_bases, ctr.dev());
        return hipSuccess;
    }));
    if (ctr.host.bad) return AIX_ERR_ARG;
    // everything is validated: from here on counts and the outputs are written
    unsigned long long stats[3] = {0, 0, 0};
    if (R) {
        DevArr diff(s), depth(s), len64(s), poff(s), rd0(s), gs(s), tmp(s), tmp2(s);
        AIXCHK(sh_alloc(diff, B + 1, 4));
        AIXCHK(sh_alloc(depth, B, 4));
        AIXCHK(sh_alloc(len64, R + 1, 8));
        AIXCHK(sh_alloc(poff, R + 1, 8));
        AIXCHK(sh_alloc(rd0, R, 8));
        AIXCHK(sh_alloc(gs, R, 8));
        AIXCHK(hipMemsetAsync(diff.p, 0, 4 * (B + 1), s));
        if (d_place_mism) AIXCHK(hipMemsetAsync(d_place_mism, 0, 4 * R, s));
        AIXCHK(ctr.run([&]() {
            AIX_TRY_LAUNCH(k_pl_edges, dim3(chain_grid(R + 1, 2 * kCB, cap)), blk, 0, s, g, (uint32_t*)diff.p, (uint64_t*)len64.p, (uint64_t*)rd0.p, (uint64_t*)gs.p);
            AIX_TRY(scan_u64((const uint64_t*)len64.p, (uint64_t*)poff.p, R + 1, tmp, s));
            // a lane per read base, grid-stride: the total is poff[R] on the device, and 64 bases per placement size the grid without a read-back
            AIX_TRY_LAUNCH(k_pl_bases, dim3(chain_grid(64 * R, kCB, cap)), blk, 0, s, R, (const uint64_t*)poff.p, (const uint64_t*)rd0.p, (const uint64_t*)gs.p,
                           (const uint8_t*)d_seqs, d_bases, d_counts, d_place_mism, ctr.dev());
            AIX_TRY(with_temp(tmp2, [&](void* t, size_t& tb) {
                return rocprim::inclusive_scan(t, tb, (const uint32_t*)diff.p, (uint32_t*)depth.p, (size_t)B, rocprim::plus<uint32_t>(), s);
            }));
            AIX_TRY_LAUNCH(k_pl_apply, dim3(chain_grid(B, 4 * kCB, cap)), blk, 0, s, B, (const uint32_t*)depth.p, d_bases, (uint4*)d_counts);
            return hipSuccess;
        }));
        stats[0] = ctr.host.a; stats[1] = ctr.host.b; stats[2] = ctr.host.c;
    }
    if (d_stats) {
        AIXCHK(hipMemcpyAsync(d_stats, stats, 24, hipMemcpyHostToDevice, s));
        AIXCHK(hipStreamSynchronize(s));
    }
    return AIX_OK;
}

extern "C" int aix_pile_call_dev(uint64_t U, const uint64_t* d_offsets, const uint8_t* d_bases, const uint32_t* d_counts, uint32_t min_depth,
                                 uint32_t min_major_permille, uint32_t min_alt_count, uint32_t min_alt_permille, uint8_t* d_polished, uint64_t* n_changed_out,
                                 uint32_t* d_var_unitig, uint32_t* d_var_pos, uint8_t* d_var_ref, uint8_t* d_var_alt, uint32_t* d_var_ref_count,
                                 uint32_t* d_var_alt_count, uint32_t* d_var_depth, uint64_t cap, uint64_t* total_out, uint64_t* d_depth_sum, uint32_t* d_uncovered,
                                 void* stream) {
    if (U > kUnitLimit) return AIX_ERR_UNSUPPORTED;
    if (!d_offsets || ((uintptr_t)d_counts & 15u) || (U && (!d_bases || !d_counts))) return AIX_ERR_ARG;
    if (cap && (!total_out || !d_var_unitig || !d_var_pos || !d_var_ref || !d_var_alt || !d_var_ref_count || !d_var_alt_count || !d_var_depth)) return AIX_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const uint64_t grid_cap = chain_test_grid();
    const dim3 blk(kCB);
    const PlThr th{min_depth, min_major_permille, min_alt_count, min_alt_permille};
    Counted<PlCounters> ctr(s);
    AIXCHK(ctr.init());
    uint64_t B = 0;
    AIXCHK(ctr.run([&]() {
        AIX_TRY_LAUNCH(k_pl_offsets_validate, dim3(chain_grid(U + 1, 4 * kCB, grid_cap)), blk, 0, s, U, d_offsets, ctr.dev());
        return hipMemcpyAsync(&B, d_offsets + U, 8, hipMemcpyDeviceToHost, s);
    }));
    if (ctr.host.bad || B >= (1ull << 60)) return AIX_ERR_ARG;
    DevArr vflag(s), sel(s), nsel(s), tmp(s);
    if (total_out) AIXCHK(sh_alloc(vflag, B, 1));
    AIXCHK(ctr.run([&]() {
        AIX_TRY_LAUNCH(k_pl_call_flag, dim3(chain_grid(B, 4 * kCB, grid_cap)), blk, 0, s, B, d_bases, (const uint4*)d_counts, th, total_out ? (uint8_t*)vflag.p : nullptr,
                       ctr.dev());
        return hipSuccess;
    }));
    if (ctr.host.bad) return AIX_ERR_ARG;
    // everything is validated: from here on the outputs are written
    const uint64_t total = ctr.host.a;
    if (d_depth_sum) AIXCHK(hipMemsetAsync(d_depth_sum, 0, 8 * U, s));
    if (d_uncovered) AIXCHK(hipMemsetAsync(d_uncovered, 0, 4 * U, s));
    AIXCHK(ctr.run([&]() {
        if (B && (d_polished || n_changed_out || d_depth_sum || d_uncovered))
            AIX_TRY_LAUNCH(k_pl_call_write, dim3(chain_grid(B, 4 * kCB, grid_cap)), blk, 0, s, B, U, d_offsets, d_bases, (const uint4*)d_counts, th, d_polished,
                           (unsigned long long*)d_depth_sum, d_uncovered, ctr.dev());
        if (total && total <= cap) {
            AIX_TRY(sh_alloc(sel, total, 8));
            AIX_TRY(nsel.alloc(8));
            AIX_TRY(with_temp(tmp, [&](void* t, size_t& tb) {
                return rocprim::select(t, tb, rocprim::counting_iterator<uint64_t>(0), (const uint8_t*)vflag.p, (uint64_t*)sel.p, (uint64_t*)nsel.p, (size_t)B, s);
            }));
            const PlVarOut o{d_var_unitig, d_var_pos, d_var_ref, d_var_alt, d_var_ref_count, d_var_alt_count, d_var_depth, cap};
            AIX_TRY_LAUNCH(k_pl_call_vars, dim3(chain_grid(total, kCB, grid_cap)), blk, 0, s, total, (const uint64_t*)sel.p, U, d_offsets, d_bases, (const uint4*)d_counts, th, o);
        }
        return hipSuccess;
    }));
    if (n_changed_out) *n_changed_out = ctr.host.b;
    if (total_out) *total_out = total;
    return AIX_OK;
}

// the refusals of the handle: those of aix_seq_thread
static int pl_check_handle(const aix_index_t* h) {
    if (!h) return AIX_ERR_ARG;
    if (h->k != 23) return AIX_ERR_MODE;
    if (!h->canonical_only) return AIX_ERR_UNSUPPORTED;
    if (h->n == 0) return AIX_ERR_UNSUPPORTED;
    if (2 * h->n > 0xFFFFFFF8ull) return AIX_ERR_UNSUPPORTED;
    return AIX_OK;
}

// Layout, emit, links and nodes at `cutoff` as aix_seq_thread builds them, the threads (sized, then filled), the placements and one
// pile-up from zero, for host memory: every array is malloc'd (aix_free).
extern "C" int aix_pileup(aix_index_t* h, uint32_t cutoff, const char* seqs, const uint64_t* offs, uint64_t M, uint32_t max_gap, uint32_t extend,
                          uint64_t* n_unitigs_out, uint64_t* n_place_out, uint64_t* n_circular_steps_out, uint64_t** offsets_out, uint8_t** bases_out,
                          uint32_t** counts_out, uint64_t** seq_place_off_out, uint32_t** place_unitig_out, uint8_t** place_flag_out, uint32_t** place_pos_out,
                          uint32_t** place_q0_out, uint32_t** place_len_out, uint32_t** place_steps_out, uint32_t** place_mism_out, uint64_t** stats_out) {
    const int st = pl_check_handle(h);
    if (st) return st;
    if (!n_unitigs_out || !n_place_out || !offsets_out || !bases_out || !counts_out || !seq_place_off_out || !place_unitig_out || !place_flag_out || !place_pos_out ||
        !place_q0_out || !place_len_out || !place_steps_out || !offs || M >= (1ull << 56))
        return AIX_ERR_ARG;
    if (M && offs[M] && !seqs) return AIX_ERR_ARG;
    DevGuard guard(h->device);
    const uint64_t n = h->n;
    DevArr ku, kp, kf, off, bs, ci, ts, tn, tx, lo, lt, nd, sso, su, sp, sf, qf, ql, sl, cnt, spo, pu, pf, pp, pq, pl, ps, pm, stt;
    AIXCHK(ku.alloc(8 * n));
    AIXCHK(kp.alloc(4 * n));
    AIXCHK(kf.alloc(n));
    uint64_t U = 0, B = 0, n_live = 0, n_circ = 0, E = 0;
    int r = aix_unitigs_layout_dev(h, cutoff, (uint64_t*)ku.p, (uint32_t*)kp.p, (uint8_t*)kf.p, &U, &B, &n_live, &n_circ, nullptr);
    if (r) return r;
    AIXCHK(off.alloc(8 * (U + 1)));
    AIXCHK(bs.alloc(B));
    AIXCHK(ci.alloc(U));
    AIXCHK(ts.alloc(8 * U));
    AIXCHK(tn.alloc(4 * U));
    AIXCHK(tx.alloc(4 * U));
    r = aix_unitigs_emit_dev(h, cutoff, (const uint64_t*)ku.p, (const uint32_t*)kp.p, (const uint8_t*)kf.p, U, (uint64_t*)off.p, (uint8_t*)bs.p, (uint8_t*)ci.p,
                             (uint64_t*)ts.p, (uint32_t*)tn.p, (uint32_t*)tx.p, nullptr, nullptr);
    if (r) return r;
    ts.drop(); tn.drop(); tx.drop();
    AIXCHK(lo.alloc(8 * (2 * U + 1)));
    AIXCHK(lt.alloc(4 * 8 * U));
    r = aix_unitig_links_dev(h, cutoff, (const uint64_t*)ku.p, (const uint32_t*)kp.p, (const uint8_t*)kf.p, U, (const uint64_t*)off.p, (uint64_t*)lo.p, (uint32_t*)lt.p,
                             8 * U, &E, nullptr);
    if (r) return r;
    AIXCHK(nd.alloc(8 * n));
    r = aix_thread_nodes_dev(n, (const uint64_t*)ku.p, (const uint32_t*)kp.p, (const uint8_t*)kf.p, U, (const uint64_t*)off.p, (uint64_t*)nd.p, nullptr);
    if (r) return r;
    ku.drop(); kp.drop(); kf.drop();
    DevArr ds, dof;
    if (const int su_st = sh_upload(seqs, offs, M, ds, dof)) return su_st;
    AIXCHK(sso.alloc(8 * (M + 1)));
    uint64_t T = 0, R = 0, n_circ_steps = 0;
    for (int pass = 0; pass < 2; ++pass) {                         // sized, then filled
        const uint64_t cap = pass ? T : 0;
        if (pass) {
            AIXCHK(sh_alloc(su, T, 4));
            AIXCHK(sh_alloc(sp, T, 4));
            AIXCHK(sh_alloc(sf, T, 1));
            AIXCHK(sh_alloc(qf, T, 4));
            AIXCHK(sh_alloc(ql, T, 4));
            AIXCHK(sh_alloc(sl, T, 8));
        }
        r = aix_seq_thread_dev(h, (const char*)ds.p, (const uint64_t*)dof.p, M, (const uint64_t*)nd.p, U, (const uint64_t*)off.p, (const uint8_t*)ci.p,
                               (const uint64_t*)lo.p, (const uint32_t*)lt.p, E, nullptr, (uint64_t*)sso.p, (uint32_t*)su.p, (uint32_t*)sp.p, (uint8_t*)sf.p,
                               (uint32_t*)qf.p, (uint32_t*)ql.p, (uint64_t*)sl.p, cap, &T, nullptr);
        if (r) return r;
        if (T == 0) break;
    }
    nd.drop(); lo.drop(); lt.drop(); ci.drop(); sl.drop();
    AIXCHK(spo.alloc(8 * (M + 1)));
    AIXCHK(sh_alloc(pu, T, 4));
    AIXCHK(sh_alloc(pf, T, 1));
    AIXCHK(sh_alloc(pp, T, 4));
    AIXCHK(sh_alloc(pq, T, 4));
    AIXCHK(sh_alloc(pl, T, 4));
    AIXCHK(sh_alloc(ps, T, 4));
    r = aix_pile_place_dev(M, (const uint64_t*)dof.p, (const uint64_t*)sso.p, T, (const uint32_t*)su.p, (const uint32_t*)sp.p, (const uint8_t*)sf.p, (const uint32_t*)qf.p,
                           (const uint32_t*)ql.p, U, (const uint64_t*)off.p, max_gap, extend, (uint64_t*)spo.p, (uint32_t*)pu.p, (uint8_t*)pf.p, (uint32_t*)pp.p,
                           (uint32_t*)pq.p, (uint32_t*)pl.p, (uint32_t*)ps.p, &R, &n_circ_steps, nullptr);
    if (r) return r;
    AIXCHK(sh_alloc(cnt, B, 16));
    AIXCHK(hipMemset(cnt.p, 0, 16 * B));
    AIXCHK(sh_alloc(pm, R, 4));
    AIXCHK(stt.alloc(24));
    r = aix_pileup_dev((const char*)ds.p, (const uint64_t*)dof.p, M, (const uint64_t*)spo.p, R, (const uint32_t*)pu.p, (const uint8_t*)pf.p, (const uint32_t*)pp.p,
                       (const uint32_t*)pq.p, (const uint32_t*)pl.p, U, (const uint64_t*)off.p, (const uint8_t*)bs.p, (uint32_t*)cnt.p, (uint32_t*)pm.p, (uint64_t*)stt.p,
                       nullptr);
    if (r) return r;
    const HostOut outs[] = {{(void**)offsets_out, off.p, 8 * (U + 1)}, {(void**)bases_out, bs.p, B},           {(void**)counts_out, cnt.p, 16 * B},
                            {(void**)seq_place_off_out, spo.p, 8 * (M + 1)}, {(void**)place_unitig_out, pu.p, 4 * R}, {(void**)place_flag_out, pf.p, R},
                            {(void**)place_pos_out, pp.p, 4 * R},      {(void**)place_q0_out, pq.p, 4 * R},    {(void**)place_len_out, pl.p, 4 * R},
                            {(void**)place_steps_out, ps.p, 4 * R},    {(void**)place_mism_out, pm.p, 4 * R},  {(void**)stats_out, stt.p, 24}};
    AIXCHK(copy_out_host(outs, 12));
    *n_unitigs_out = U;
    *n_place_out = R;
    if (n_circular_steps_out) *n_circular_steps_out = n_circ_steps;
    return AIX_OK;
}
