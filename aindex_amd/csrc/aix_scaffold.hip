// aix_scaffold.hip — contigs scaffolded with read pairs, on arrays resident in HBM: one observation per threaded pair (which contig end
// faces which, and how many bases of the fragment lie on the two contigs), the observations bundled into a scaffold graph over contig
// ends, the joins decided per end, the chains of joined contigs ranked by pointer jumping (cycles cut at their weakest join), and the
// gapped scaffolds written. The contract is stated above the aix_mate_links_dev / aix_scaffold_* declarations in include/aindex_hip.h;
// DESIGN 5n has the derivations and the resources. No index handle: the arrays and the current device, like the cleaning. One plain launch
// per step; every call validates with counting kernels that write nothing but their counters and writes only after the host has read
// them as clean; integer only, no LDS, no grid-wide barrier, no spin-wait:
//   links    k_sc_ml_validate (one lane per offset, step and contig), k_sc_ml_pairs (one lane per pair; a u64 atomicAdd per same-contig pair)
//   bundle   k_sc_bd_validate, a radix sort and a reduce by key of the N observations, k_sc_bd_expand (every bundle and its dual), a radix
//            sort of the 2 B directed links, k_sc_bd_off (one lane per end, a bisection), k_sc_bd_emit
//   mark     k_sc_mk_validate, k_sc_mk_join (one lane per end each)
//   layout   k_sc_ly_validate, k_sc_ly_init, k_sc_ly_jump per round (the host loop is chain_rank); on cycles k_sc_cy_init, k_sc_cy_jump per
//            round, k_sc_cy_cut and the ranking again; k_sc_ly_place, a scan of the first members, k_sc_ly_assign
//   emit     k_sc_ly_validate, k_sc_em_keys, a radix sort into member order, k_sc_em_validate, k_sc_em_ends; then a scan into
//            scaffold_offsets, k_sc_em_members and k_graph_em_bases<false> (one lane per output byte, a bisection over the members' first bytes)
// What the graph files share (the counters holder, the predicates of the validate kernels, the written gap, that emit kernel) is in aix_graph.hpp.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "aix_graph.hpp"

namespace aix {

// (kNoEnd is the join of an unjoined end; the constants, the counters holder, the predicates of the validation and k_graph_em_bases: aix_graph.hpp)
static constexpr uint64_t kSFlag = 1ULL << 63;                    // ranking state: terminal reached
static constexpr uint64_t kSNoKey = ~0ULL;                        // obs_key of a pair that is no observation
static constexpr uint64_t kSLow = 0xFFFFFFFFull;

struct ScCounters {                                               // one zeroed record per call
    unsigned long long bad, n, total, cut, kind[4], unflagged[66];
};

struct ScAgg {                                                    // a bundle: its observations and the sum of their d
    unsigned long long count, dsum;
};
struct ScAggOp {
    __host__ __device__ ScAgg operator()(const ScAgg& a, const ScAgg& b) const { return ScAgg{a.count + b.count, a.dsum + b.dsum}; }
};
struct ScAggOf {
    __host__ __device__ ScAgg operator()(uint32_t d) const { return ScAgg{1ull, (unsigned long long)d}; }
};

// ---------------------------------------------------------------------------------------------
// 1. one observation per pair
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kCB) k_sc_ml_validate(uint64_t P, const uint64_t* __restrict__ offs, const uint64_t* __restrict__ sso, uint64_t T,
                                                       const uint32_t* __restrict__ step_unitig, const uint32_t* __restrict__ step_pos,
                                                       const uint32_t* __restrict__ q_first, const uint32_t* __restrict__ q_last, uint64_t U,
                                                       const uint64_t* __restrict__ offsets, ScCounters* __restrict__ ctr) {
    const uint64_t M = 2 * P, mt = M > T ? M : T, work = mt > U ? mt : U, stride = (uint64_t)gridDim.x * kCB;
    unsigned long long bad = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kCB + threadIdx.x; i < work; i += stride) {
        if (i < M) {
            const uint64_t a = sso[i], b = sso[i + 1], x = offs[i], y = offs[i + 1];
            bad += i == 0 && a != 0;
            bad += i == M - 1 && b != T;
            bad += b < a || b > T;
            bad += y < x || y - x > kSLow;
        }
        if (i < T) {
            const uint64_t u = step_unitig[i];
            bad += q_first[i] > q_last[i];
            if (u >= U) ++bad;
            else {
                const uint64_t a = offsets[u], b = offsets[u + 1];
                bad += b >= a && b - a >= 23 && (uint64_t)step_pos[i] >= b - a - 22;      // (offsets that do not ascend: counted below)
            }
        }
        if (i < U) bad += span_bad(offsets[i], offsets[i + 1]);
    }
    count_add(bad, &ctr->bad);
}

struct ScAnchor {
    bool ok;
    uint64_t u, s;
    long long x0;                                                 // the start of the mate on its contig, oriented as the step traverses it
};

// the step of sequence m with the most windows, the earliest on a tie (behind k_sc_ml_validate: every index is in range)
__device__ __forceinline__ ScAnchor sc_anchor(uint64_t m, const uint64_t* __restrict__ sso, const uint32_t* __restrict__ step_unitig,
                                              const uint32_t* __restrict__ step_pos, const uint8_t* __restrict__ step_flag, const uint32_t* __restrict__ q_first,
                                              const uint32_t* __restrict__ q_last, const uint64_t* __restrict__ offsets, const uint8_t* __restrict__ circular,
                                              uint64_t min_windows) {
    uint64_t best = 0, bw = 0;
    for (uint64_t j = sso[m], hi = sso[m + 1]; j < hi; ++j) {
        const uint64_t w = (uint64_t)q_last[j] - q_first[j] + 1;
        if (w > bw) { bw = w; best = j; }
    }
    ScAnchor a{false, 0, 0, 0};
    if (bw == 0 || bw < min_windows) return a;
    a.u = step_unitig[best];
    if (circular[a.u]) return a;
    a.ok = true;
    a.s = step_flag[best] & 1u;
    const long long mu = (long long)(offsets[a.u + 1] - offsets[a.u]) - 22, pos = step_pos[best];
    a.x0 = (a.s ? mu - 1 - pos : pos) - (long long)q_first[best];
    return a;
}

__global__ void __launch_bounds__(kCB) k_sc_ml_pairs(uint64_t P, const uint64_t* __restrict__ offs, const uint64_t* __restrict__ sso,
                                                    const uint32_t* __restrict__ step_unitig, const uint32_t* __restrict__ step_pos,
                                                    const uint8_t* __restrict__ step_flag, const uint32_t* __restrict__ q_first, const uint32_t* __restrict__ q_last,
                                                    const uint64_t* __restrict__ offsets, const uint8_t* __restrict__ circular, uint64_t min_windows,
                                                    long long max_insert, unsigned long long* __restrict__ hist, uint64_t* __restrict__ obs_key,
                                                    uint32_t* __restrict__ obs_d, ScCounters* __restrict__ ctr) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    unsigned long long kind[4] = {0, 0, 0, 0};                   // same contig, link, discordant, unanchored
    for (uint64_t i = (uint64_t)blockIdx.x * kCB + threadIdx.x; i < P; i += stride) {
        const ScAnchor A = sc_anchor(2 * i, sso, step_unitig, step_pos, step_flag, q_first, q_last, offsets, circular, min_windows);
        const ScAnchor B = sc_anchor(2 * i + 1, sso, step_unitig, step_pos, step_flag, q_first, q_last, offsets, circular, min_windows);
        const long long LB = (long long)(offs[2 * i + 2] - offs[2 * i + 1]);
        uint64_t key = kSNoKey;
        uint32_t d = 0;
        int k = 2;
        if (!A.ok || !B.ok) k = 3;
        else if (A.u == B.u) {
            const long long F = B.x0 + LB - A.x0;
            if (A.s == B.s && F >= 1 && F <= max_insert) { k = 0; atomicAdd(hist + F, 1ull); }
        } else {
            const long long dd = ((long long)(offsets[A.u + 1] - offsets[A.u]) - A.x0) + (B.x0 + LB);
            if (dd >= 1 && dd <= max_insert) {
                uint64_t e = 2 * A.u + A.s, t = 2 * B.u + B.s;
                if ((t ^ 1) < e) { const uint64_t e2 = t ^ 1; t = e ^ 1; e = e2; }
                key = e << 32 | t;
                d = (uint32_t)dd;
                k = 1;
            }
        }
        obs_key[i] = key;
        obs_d[i] = d;
        ++kind[k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) count_add(kind[k], &ctr->kind[k]);
}

// ---------------------------------------------------------------------------------------------
// 2. observations into a scaffold graph
// ---------------------------------------------------------------------------------------------
// every key is skipped (all ones) or canonical with both words below 2 U on different contigs and d >= 1; n: the keys that are not skipped
__global__ void __launch_bounds__(kCB) k_sc_bd_validate(uint64_t N, const uint64_t* __restrict__ key, const uint32_t* __restrict__ d, uint64_t U,
                                                       ScCounters* __restrict__ ctr) {
    const uint64_t NE = 2 * U, stride = (uint64_t)gridDim.x * kCB;
    unsigned long long bad = 0, n = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kCB + threadIdx.x; i < N; i += stride) {
        const uint64_t k = key[i];
        if (k == kSNoKey) continue;
        const uint64_t e = k >> 32, t = k & kSLow;
        bad += e >= NE || t >= NE || (e >> 1) == (t >> 1) || e > (t ^ 1) || d[i] == 0;
        ++n;
    }
    count_add(bad, &ctr->bad);
    count_add(n, &ctr->n);
}

// bundle i as e -> t and as its dual; both name bundle i
__global__ void __launch_bounds__(kCB) k_sc_bd_expand(uint64_t B, const uint64_t* __restrict__ uniq, uint64_t* __restrict__ dkey, uint32_t* __restrict__ didx) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t i = (uint64_t)blockIdx.x * kCB + threadIdx.x; i < B; i += stride) {
        const uint64_t k = uniq[i], e = k >> 32, t = k & kSLow;
        dkey[2 * i] = k;
        dkey[2 * i + 1] = (t ^ 1) << 32 | (e ^ 1);
        didx[2 * i] = (uint32_t)i;
        didx[2 * i + 1] = (uint32_t)i;
    }
}

// slink_off[e] = the number of directed links whose source is below e
__global__ void __launch_bounds__(kCB) k_sc_bd_off(uint64_t NE, const uint64_t* __restrict__ dkey, uint64_t S, uint64_t* __restrict__ slink_off) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t e = (uint64_t)blockIdx.x * kCB + threadIdx.x; e <= NE; e += stride) slink_off[e] = first_ge(dkey, 0, S, e << 32);
}

__global__ void __launch_bounds__(kCB) k_sc_bd_emit(uint64_t S, uint64_t B, const uint64_t* __restrict__ dkey, const uint32_t* __restrict__ didx,
                                                   const ScAgg* __restrict__ agg, uint32_t* __restrict__ to, uint64_t* __restrict__ count, uint64_t* __restrict__ dsum) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t j = (uint64_t)blockIdx.x * kCB + threadIdx.x; j < S; j += stride) {
        const uint64_t b = didx[j];
        if (b >= B) continue;                                     // (never: the expansion wrote it)
        const ScAgg a = agg[b];
        to[j] = (uint32_t)(dkey[j] & kSLow);
        count[j] = a.count;
        dsum[j] = a.dsum;
    }
}

// ---------------------------------------------------------------------------------------------
// 3. which ends are joined
// ---------------------------------------------------------------------------------------------
struct ScGraph {                                                  // contigs and the scaffold links over their ends, in HBM
    uint64_t U, S;
    const uint64_t* offsets;
    const uint8_t* circular;
    const uint64_t* off;
    const uint32_t* to;
    const uint64_t* count;
    const uint64_t* dsum;
};

// offsets ascend by 23; slink_off starts at 0, ascends, ends at S; words below 2 U, on another contig, strictly ascending; count >= 1; the
// mean d fits 32 bits; every link has its dual with equal count and dsum
__global__ void __launch_bounds__(kCB) k_sc_mk_validate(const ScGraph g, ScCounters* __restrict__ ctr) {
    const uint64_t NE = 2 * g.U, stride = (uint64_t)gridDim.x * kCB;
    unsigned long long bad = 0;
    for (uint64_t e = (uint64_t)blockIdx.x * kCB + threadIdx.x; e < NE; e += stride) {
        if (!(e & 1)) bad += span_bad(g.offsets[e >> 1], g.offsets[(e >> 1) + 1]);
        const uint64_t lo = g.off[e], hi = g.off[e + 1];
        bad += csr_bad(e, NE, lo, hi, g.S, kAnyDegree);
        if (!csr_in_range(lo, hi, g.S, kAnyDegree)) continue;
        for (uint64_t j = lo; j < hi; ++j) {
            const uint64_t t = g.to[j], c = g.count[j];
            if (t >= NE || (t >> 1) == (e >> 1) || c == 0) { ++bad; continue; }
            bad += j > lo && (uint64_t)g.to[j - 1] >= t;
            bad += g.dsum[j] / c > kSLow;
            const uint64_t lo2 = g.off[t ^ 1], hi2 = g.off[(t ^ 1) + 1];
            if (!csr_in_range(lo2, hi2, g.S, kAnyDegree)) { ++bad; continue; }
            uint64_t a = lo2, b = hi2;                            // a bisection that ends whatever the list holds
            while (a < b) {
                const uint64_t mid = a + ((b - a) >> 1);
                if ((uint64_t)g.to[mid] < (e ^ 1)) a = mid + 1; else b = mid;
            }
            if (a >= hi2 || (uint64_t)g.to[a] != (e ^ 1)) { ++bad; continue; }
            bad += g.count[a] != c || g.dsum[a] != g.dsum[j];
        }
    }
    count_add(bad, &ctr->bad);
}

__device__ __forceinline__ bool sc_eligible(const ScGraph& g, uint64_t u, uint64_t min_bases) {
    return !g.circular[u] && g.offsets[u + 1] - g.offsets[u] >= min_bases;
}

// end e is decided: *best is the index of its best link (behind k_sc_mk_validate)
__device__ __forceinline__ bool sc_best(const ScGraph& g, uint64_t e, uint64_t min_pairs, uint64_t dominance, uint64_t min_bases, uint64_t* best) {
    if (!sc_eligible(g, e >> 1, min_bases)) return false;
    const uint64_t lo = g.off[e], hi = g.off[e + 1];
    uint64_t bj = ~0ULL, bc = 0;
    for (uint64_t j = lo; j < hi; ++j) {
        const uint64_t c = g.count[j];
        if (c >= min_pairs && c > bc && sc_eligible(g, g.to[j] >> 1, min_bases)) { bc = c; bj = j; }   // ascending words: the smaller one stays on a tie
    }
    if (bj == ~0ULL) return false;
    for (uint64_t j = lo; j < hi; ++j) {
        const uint64_t c = g.count[j];
        if (j != bj && c >= min_pairs && sc_eligible(g, g.to[j] >> 1, min_bases) && (unsigned __int128)c * dominance > (unsigned __int128)bc) return false;
    }
    *best = bj;
    return true;
}

__global__ void __launch_bounds__(kCB) k_sc_mk_join(const ScGraph g, uint32_t insert_size, uint64_t min_pairs, uint64_t dominance, uint64_t min_bases,
                                                   uint32_t* __restrict__ join, uint64_t* __restrict__ join_count, long long* __restrict__ join_gap,
                                                   ScCounters* __restrict__ ctr) {
    const uint64_t NE = 2 * g.U, stride = (uint64_t)gridDim.x * kCB;
    unsigned long long n = 0;
    for (uint64_t e = (uint64_t)blockIdx.x * kCB + threadIdx.x; e < NE; e += stride) {
        uint32_t t = kNoEnd;
        uint64_t c = 0, j = 0, j2 = 0;
        long long gap = 0;
        if (sc_best(g, e, min_pairs, dominance, min_bases, &j)) {
            const uint64_t w = g.to[j];
            if (sc_best(g, w ^ 1, min_pairs, dominance, min_bases, &j2) && (uint64_t)g.to[j2] == (e ^ 1)) {
                t = (uint32_t)w;
                c = g.count[j];
                gap = (long long)insert_size - (long long)(g.dsum[j] / c);
                n += e < (w ^ 1);
            }
        }
        join[e] = t;
        join_count[e] = c;
        join_gap[e] = gap;
    }
    count_add(n, &ctr->n);
}

// ---------------------------------------------------------------------------------------------
// 4. layout
// ---------------------------------------------------------------------------------------------
// offsets ascend by 23; a join names an end of another contig whose dual join names this end back, with equal count and gap
__global__ void __launch_bounds__(kCB) k_sc_ly_validate(uint64_t U, const uint64_t* __restrict__ offsets, const uint32_t* __restrict__ join,
                                                       const uint64_t* __restrict__ join_count, const long long* __restrict__ join_gap,
                                                       ScCounters* __restrict__ ctr) {
    const uint64_t NE = 2 * U, stride = (uint64_t)gridDim.x * kCB;
    unsigned long long bad = 0;
    for (uint64_t e = (uint64_t)blockIdx.x * kCB + threadIdx.x; e < NE; e += stride) {
        if (!(e & 1)) bad += span_bad(offsets[e >> 1], offsets[(e >> 1) + 1]);
        const uint64_t t = join[e];
        if (t == kNoEnd) continue;
        if (!join_dual_ok(join, join_gap, NE, e, t)) { ++bad; continue; }
        if (join_count) bad += join_count[t ^ 1] != join_count[e];
    }
    count_add(bad, &ctr->bad);
}

// the state of the ranking per end p: nx = the exit end of the next contig (flagged: p is terminal), dist = the bases from the far side of
// the join to there, hops = the members. cut (nullable): joins taken out of their cycles. total: the written gaps, each join once.
__global__ void __launch_bounds__(kCB) k_sc_ly_init(uint64_t NE, const uint64_t* __restrict__ offsets, const uint32_t* __restrict__ join,
                                                   const long long* __restrict__ join_gap, uint32_t min_gap, const uint8_t* __restrict__ cut,
                                                   uint64_t* __restrict__ nx, uint64_t* __restrict__ dist, uint32_t* __restrict__ hops, ScCounters* __restrict__ ctr) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    unsigned long long open = 0, gaps = 0, ncut = 0;
    for (uint64_t p = (uint64_t)blockIdx.x * kCB + threadIdx.x; p < NE; p += stride) {
        const uint64_t t = join[p];
        const bool is_cut = t != kNoEnd && cut && cut[p];
        const bool linked = t != kNoEnd && !is_cut;
        const uint64_t w = linked ? written_gap(join_gap[p], min_gap) : 0;
        nx[p] = linked ? t : (p | kSFlag);
        dist[p] = linked ? w + unit_len(offsets, t) : 0;
        hops[p] = linked;
        open += linked;
        if (linked && p < (t ^ 1)) gaps += w;
        ncut += is_cut && p < (t ^ 1);
    }
    count_add(open, &ctr->unflagged[0]);
    count_add(gaps, &ctr->total);
    count_add(ncut, &ctr->cut);
}

__global__ void __launch_bounds__(kCB) k_sc_ly_jump(uint64_t NE, const uint64_t* __restrict__ nx_in, const uint64_t* __restrict__ d_in, const uint32_t* __restrict__ h_in,
                                                   uint64_t* __restrict__ nx_out, uint64_t* __restrict__ d_out, uint32_t* __restrict__ h_out,
                                                   unsigned long long* __restrict__ unflagged) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    unsigned long long open = 0;
    for (uint64_t p = (uint64_t)blockIdx.x * kCB + threadIdx.x; p < NE; p += stride) {
        uint64_t s = nx_in[p], d = d_in[p];
        uint32_t h = h_in[p];
        if (!(s & kSFlag)) {
            const uint64_t q = s & kSLow;
            s = nx_in[q];
            d += d_in[q];                                          // on a cycle d and h mean nothing (and may wrap)
            h += h_in[q];
            open += !(s & kSFlag);
        }
        nx_out[p] = s;
        d_out[p] = d;
        h_out[p] = h;
    }
    count_add(open, unflagged);
}

// the key of the join at end p: the weaker join has the smaller key, the end id decides among equals
__device__ __forceinline__ uint64_t sc_cut_key(uint64_t p, uint64_t t, uint64_t count) {
    return (count < kSLow ? count : kSLow) << 32 | (p < (t ^ 1) ? p : (t ^ 1));
}

// cycles (unflagged ends only): succ = the end 2^r joins on, key = the smallest join key on the way
__global__ void __launch_bounds__(kCB) k_sc_cy_init(uint64_t NE, const uint64_t* __restrict__ rank, const uint32_t* __restrict__ join,
                                                   const uint64_t* __restrict__ join_count, uint32_t* __restrict__ succ, uint64_t* __restrict__ key) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t p = (uint64_t)blockIdx.x * kCB + threadIdx.x; p < NE; p += stride) {
        if (rank[p] & kSFlag) continue;
        const uint64_t t = join[p];                                // an unflagged end is joined
        succ[p] = (uint32_t)t;
        key[p] = sc_cut_key(p, t, join_count[p]);
    }
}

__global__ void __launch_bounds__(kCB) k_sc_cy_jump(uint64_t NE, const uint64_t* __restrict__ rank, const uint32_t* __restrict__ s_in, const uint64_t* __restrict__ k_in,
                                                   uint32_t* __restrict__ s_out, uint64_t* __restrict__ k_out) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t p = (uint64_t)blockIdx.x * kCB + threadIdx.x; p < NE; p += stride) {
        if (rank[p] & kSFlag) continue;
        const uint64_t q = s_in[p];
        if (q >= NE || (rank[q] & kSFlag)) { s_out[p] = s_in[p]; k_out[p] = k_in[p]; continue; }   // (never: a successor on a cycle is on it)
        const uint64_t a = k_in[p], b = k_in[q];
        s_out[p] = s_in[q];
        k_out[p] = a < b ? a : b;
    }
}

__global__ void __launch_bounds__(kCB) k_sc_cy_cut(uint64_t NE, const uint64_t* __restrict__ rank, const uint32_t* __restrict__ join,
                                                  const uint64_t* __restrict__ join_count, const uint64_t* __restrict__ key, uint8_t* __restrict__ cut) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t p = (uint64_t)blockIdx.x * kCB + threadIdx.x; p < NE; p += stride)
        cut[p] = !(rank[p] & kSFlag) && sc_cut_key(p, join[p], join_count[p]) == key[p];
}

// Per contig, behind a ranking that left nothing open: a / b = the terminal ends reached through its forward / backward exit. The
// terminal contig with the smaller id is the first member; u is forwards iff the first member lies behind its backward exit.
__global__ void __launch_bounds__(kCB) k_sc_ly_place(uint64_t U, const uint64_t* __restrict__ offsets, const uint64_t* __restrict__ nx, const uint64_t* __restrict__ dist,
                                                    const uint32_t* __restrict__ hops, uint32_t* __restrict__ first_of, uint32_t* __restrict__ rank,
                                                    uint64_t* __restrict__ pos, uint8_t* __restrict__ flag, uint64_t* __restrict__ is_first, ScCounters* __restrict__ ctr) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    unsigned long long n = 0, bases = 0;
    for (uint64_t u = (uint64_t)blockIdx.x * kCB + threadIdx.x; u <= U; u += stride) {
        if (u == U) { is_first[U] = 0; continue; }
        const uint64_t fa = (nx[2 * u] & kSLow) >> 1, fb = (nx[2 * u + 1] & kSLow) >> 1;
        uint64_t first = u, r = 0, x = 0, f = 0;
        if (fa != fb) {
            f = fa < fb;
            first = f ? fa : fb;
            r = hops[2 * u + 1 - f];
            x = dist[2 * u + 1 - f];
        }
        first_of[u] = (uint32_t)first;
        rank[u] = (uint32_t)r;
        pos[u] = x;
        flag[u] = (uint8_t)f;
        is_first[u] = first == u;
        n += first == u;
        bases += offsets[u + 1] - offsets[u];
    }
    count_add(n, &ctr->n);
    count_add(bases, &ctr->total);
}

__global__ void __launch_bounds__(kCB) k_sc_ly_assign(uint64_t U, const uint32_t* __restrict__ first_of, const uint64_t* __restrict__ sid, uint32_t* __restrict__ scaffold) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t u = (uint64_t)blockIdx.x * kCB + threadIdx.x; u < U; u += stride) {
        const uint64_t f = first_of[u];
        scaffold[u] = f < U ? (uint32_t)sid[f] : kNoEnd;
    }
}

// ---------------------------------------------------------------------------------------------
// 5. emit
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kCB) k_sc_em_keys(uint64_t U, uint64_t Sc, const uint32_t* __restrict__ scaffold, const uint32_t* __restrict__ rank,
                                                   const uint8_t* __restrict__ flag, uint64_t* __restrict__ keys, ScCounters* __restrict__ ctr) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    unsigned long long bad = 0;
    for (uint64_t u = (uint64_t)blockIdx.x * kCB + threadIdx.x; u < U; u += stride) {
        bad += (uint64_t)scaffold[u] >= Sc || flag[u] > 1;
        keys[u] = (uint64_t)scaffold[u] << 32 | rank[u];
    }
    count_add(bad, &ctr->bad);
}

struct ScMap {                                                    // the layout's map and what it is checked against
    uint64_t U, Sc;
    const uint64_t* offsets;
    const uint32_t* join;
    const long long* join_gap;
    const uint64_t* pos;
    const uint8_t* flag;
    const uint64_t* keys;                                         // scaffold << 32 | rank, sorted
    const uint32_t* ids;                                          // the contig of every sorted key: the member order
    uint32_t min_gap;
};

// one lane per member in member order: (scaffold, rank) are dense, a member follows its predecessor through a join in matching
// orientation at the distance of its length and the written gap; moff[s] = the index of the first member of scaffold s
__global__ void __launch_bounds__(kCB) k_sc_em_validate(const ScMap m, uint64_t* __restrict__ moff, ScCounters* __restrict__ ctr) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    unsigned long long bad = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kCB + threadIdx.x; i <= m.U; i += stride) {
        if (i == m.U) { moff[m.Sc] = m.U; continue; }
        const uint64_t k = m.keys[i], s = k >> 32, r = k & kSLow, u = m.ids[i];
        if (u >= m.U || s >= m.Sc) { ++bad; continue; }
        const uint64_t f = m.flag[u] & 1u;
        bad += i == m.U - 1 && s != m.Sc - 1;
        const uint64_t pk = i ? m.keys[i - 1] : 0, ps = pk >> 32;
        const bool head = i == 0 || ps != s;
        if (head) {
            bad += r != 0 || (i == 0 ? s != 0 : s != ps + 1) || m.pos[u] != 0;
            moff[s] = i;
            continue;
        }
        const uint64_t w = m.ids[i - 1];
        if (r != (pk & kSLow) + 1 || w >= m.U) { ++bad; continue; }
        const uint64_t e = 2 * w + (m.flag[w] & 1u);
        if ((uint64_t)m.join[e] != 2 * u + f) { ++bad; continue; }
        bad += m.pos[u] != m.pos[w] + (m.offsets[w + 1] - m.offsets[w]) + written_gap(m.join_gap[e], m.min_gap);
    }
    count_add(bad, &ctr->bad);
}

// one lane per scaffold, behind k_sc_em_validate: its two outer ends are unjoined or joined to each other (the cut of a cycle); the
// terminal with the smaller id is first, a single contig is forwards, scaffold ids ascend by first member; slen[s] = its bases
__global__ void __launch_bounds__(kCB) k_sc_em_ends(const ScMap m, const uint64_t* __restrict__ moff, uint64_t* __restrict__ slen, ScCounters* __restrict__ ctr) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    unsigned long long bad = 0, total = 0;
    for (uint64_t s = (uint64_t)blockIdx.x * kCB + threadIdx.x; s <= m.Sc; s += stride) {
        if (s == m.Sc) { slen[s] = 0; continue; }
        const uint64_t i0 = moff[s], i1 = moff[s + 1];
        if (i0 >= i1 || i1 > m.U) { ++bad; slen[s] = 0; continue; }
        const uint64_t u = m.ids[i0], z = m.ids[i1 - 1], fu = m.flag[u] & 1u, fz = m.flag[z] & 1u;
        const uint64_t in = m.join[2 * u + (fu ^ 1)], out = m.join[2 * z + fz];
        if (i1 - i0 == 1) bad += fu != 0 || in != kNoEnd || out != kNoEnd;
        else {
            bad += u >= z;
            bad += !(in == kNoEnd && out == kNoEnd) && !(out == 2 * u + fu && in == ((2 * z + fz) ^ 1));
        }
        if (s) bad += (uint64_t)m.ids[moff[s - 1] < m.U ? moff[s - 1] : 0] >= u;
        const uint64_t len = m.pos[z] + (m.offsets[z + 1] - m.offsets[z]);
        slen[s] = len;
        total += len;
    }
    count_add(bad, &ctr->bad);
    count_add(total, &ctr->total);
}

__global__ void __launch_bounds__(kCB) k_sc_em_members(const ScMap m, const uint64_t* __restrict__ scaffold_offsets, uint32_t* __restrict__ member,
                                                      long long* __restrict__ member_gap, uint64_t* __restrict__ mstart) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t i = (uint64_t)blockIdx.x * kCB + threadIdx.x; i < m.U; i += stride) {
        const uint64_t k = m.keys[i], u = m.ids[i], f = m.flag[u] & 1u;
        member[i] = (uint32_t)(2 * u + f);
        long long gap = 0;
        if (k & kSLow) {
            const uint64_t w = m.ids[i - 1];
            gap = m.join_gap[2 * w + (m.flag[w] & 1u)];
        }
        member_gap[i] = gap;
        mstart[i] = scaffold_offsets[k >> 32] + m.pos[u];
    }
}

// (the bases of the scaffolds: k_graph_em_bases<false>, aix_graph.hpp)

// the ranking of the 2 U ends over `join` less `cut`: nx / dist / hops in the buffers *cn, *cd, *ch on return. ctr.host: the counters of the init.
static hipError_t sc_rank(uint64_t U, const uint64_t* offsets, const uint32_t* join, const long long* join_gap, uint32_t min_gap, const uint8_t* cut,
                          Counted<ScCounters>& ctr, uint64_t** cn, uint64_t** cd, uint32_t** ch, uint64_t** on, uint64_t** od, uint32_t** oh, uint64_t* open, hipStream_t s) {
    const uint64_t NE = 2 * U, cap = chain_test_grid();
    const dim3 blk(kCB), grid(chain_grid(NE, 4 * kCB, cap));
    AIX_TRY(ctr.run([&]() {
        AIX_TRY_LAUNCH(k_sc_ly_init, grid, blk, 0, s, NE, offsets, join, join_gap, min_gap, cut, *cn, *cd, *ch, ctr.dev());
        return hipSuccess;
    }));
    *open = ctr.host.unflagged[0];
    return chain_rank(U, ctr.dev()->unflagged, open, s, [&](int r) {
        AIX_TRY_LAUNCH(k_sc_ly_jump, grid, blk, 0, s, NE, (const uint64_t*)*cn, (const uint64_t*)*cd, (const uint32_t*)*ch, *on, *od, *oh, &ctr.dev()->unflagged[r]);
        std::swap(*cn, *on);
        std::swap(*cd, *od);
        std::swap(*ch, *oh);
        return hipSuccess;
    });
}

}  // namespace aix

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" int aix_mate_links_dev(uint64_t P, const uint64_t* d_offs, const uint64_t* d_seq_step_off, uint64_t T, const uint32_t* d_step_unitig,
                                  const uint32_t* d_step_pos, const uint8_t* d_step_flag, const uint32_t* d_q_first, const uint32_t* d_q_last, uint64_t U,
                                  const uint64_t* d_offsets, const uint8_t* d_circular, uint32_t min_anchor_windows, uint32_t max_insert, uint64_t* d_insert_hist,
                                  uint64_t* d_obs_key, uint32_t* d_obs_d, uint64_t* d_counts, void* stream) {
    if (U > kUnitLimit) return AIX_ERR_UNSUPPORTED;
    if (!d_counts || !d_offsets || !d_insert_hist || min_anchor_windows < 1 || max_insert < 1 || max_insert > (1u << 20) || P >= (1ull << 60) || T >= (1ull << 60))
        return AIX_ERR_ARG;
    if (P && (!d_offs || !d_seq_step_off || !d_obs_key || !d_obs_d)) return AIX_ERR_ARG;
    if (T && (!d_step_unitig || !d_step_pos || !d_step_flag || !d_q_first || !d_q_last)) return AIX_ERR_ARG;
    if (U && !d_circular) return AIX_ERR_ARG;
    if (T && !U) return AIX_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (P == 0) {
        if (T) return AIX_ERR_ARG;
        AIXCHK(hipMemsetAsync(d_counts, 0, 32, s));
        AIXCHK(hipStreamSynchronize(s));
        return AIX_OK;
    }
    const uint64_t cap = chain_test_grid();
    const dim3 blk(kCB);
    Counted<ScCounters> ctr(s);
    AIXCHK(ctr.init());
    const ScCounters& hc = ctr.host;
    AIXCHK(ctr.run([&]() {
        AIX_TRY_LAUNCH(k_sc_ml_validate, dim3(chain_grid(std::max(std::max(2 * P, T), U), 2 * kCB, cap)), blk, 0, s, P, d_offs, d_seq_step_off, T, d_step_unitig, d_step_pos,
                       d_q_first, d_q_last, U, d_offsets, ctr.dev());
        return hipSuccess;
    }));
    if (hc.bad) return AIX_ERR_ARG;
    AIXCHK(ctr.run([&]() {
        AIX_TRY_LAUNCH(k_sc_ml_pairs, dim3(chain_grid(P, kCB, cap)), blk, 0, s, P, d_offs, d_seq_step_off, d_step_unitig, d_step_pos, d_step_flag, d_q_first, d_q_last,
                       d_offsets, d_circular, (uint64_t)min_anchor_windows, (long long)max_insert, (unsigned long long*)d_insert_hist, d_obs_key, d_obs_d, ctr.dev());
        return hipSuccess;
    }));
    const uint64_t kinds[4] = {hc.kind[0], hc.kind[1], hc.kind[2], hc.kind[3]};
    AIXCHK(hipMemcpyAsync(d_counts, kinds, 32, hipMemcpyHostToDevice, s));
    AIXCHK(hipStreamSynchronize(s));
    return AIX_OK;
}

extern "C" int aix_mate_bundle_dev(uint64_t N, const uint64_t* d_obs_key, const uint32_t* d_obs_d, uint64_t U, uint64_t* d_slink_off, uint32_t* d_slink_to,
                                   uint64_t* d_slink_count, uint64_t* d_slink_dsum, uint64_t cap, uint64_t* total_out, void* stream) {
    if (U > kUnitLimit) return AIX_ERR_UNSUPPORTED;
    if (!d_slink_off || !total_out || N >= (1ull << 60)) return AIX_ERR_ARG;
    if (N && (!d_obs_key || !d_obs_d)) return AIX_ERR_ARG;
    if (cap && (!d_slink_to || !d_slink_count || !d_slink_dsum)) return AIX_ERR_ARG;
    if (N > kSLow) return AIX_ERR_UNSUPPORTED;                    // a bundle is named by 32 bits (k_sc_bd_expand)
    hipStream_t s = (hipStream_t)stream;
    const uint64_t NE = 2 * U, grid_cap = chain_test_grid();
    const dim3 blk(kCB);
    Counted<ScCounters> ctr(s);
    DevArr k2(s), d2(s), uniq(s), agg(s), cnt(s), dk(s), di(s), dk2(s), di2(s), tmp(s), tmp2(s), tmp3(s);
    uint64_t B = 0;
    if (N) {
        AIXCHK(ctr.init());
        const ScCounters& hc = ctr.host;
        AIXCHK(ctr.run([&]() {
            AIX_TRY_LAUNCH(k_sc_bd_validate, dim3(chain_grid(N, 4 * kCB, grid_cap)), blk, 0, s, N, d_obs_key, d_obs_d, U, ctr.dev());
            return hipSuccess;
        }));
        if (hc.bad) return AIX_ERR_ARG;
        if (hc.n) {
            AIXCHK(k2.alloc(8 * N));
            AIXCHK(d2.alloc(4 * N));
            AIXCHK(uniq.alloc(8 * N));
            AIXCHK(agg.alloc(sizeof(ScAgg) * N));
            AIXCHK(cnt.alloc(8));
            AIXCHK(sort_pairs(d_obs_key, (uint64_t*)k2.p, d_obs_d, (uint32_t*)d2.p, N, 64u, tmp, s));
            AIXCHK(with_temp(tmp2, [&](void* t, size_t& tb) {
                return rocprim::reduce_by_key(t, tb, (const uint64_t*)k2.p, rocprim::make_transform_iterator((const uint32_t*)d2.p, ScAggOf()), (size_t)N, (uint64_t*)uniq.p,
                                              (ScAgg*)agg.p, (uint64_t*)cnt.p, ScAggOp(), rocprim::equal_to<uint64_t>(), s);
            }));
            uint64_t runs = 0;
            AIXCHK(hipMemcpyAsync(&runs, cnt.p, 8, hipMemcpyDeviceToHost, s));
            AIXCHK(hipStreamSynchronize(s));
            B = std::min(runs, N) - (hc.n < N ? 1 : 0);            // the skipped keys are all ones: the last run
        }
    }
    const uint64_t S = 2 * B;
    if (S) {
        AIXCHK(dk.alloc(8 * S));
        AIXCHK(di.alloc(4 * S));
        AIXCHK(dk2.alloc(8 * S));
        AIXCHK(di2.alloc(4 * S));
        hipLaunchKernelGGL(k_sc_bd_expand, dim3(chain_grid(B, 4 * kCB, grid_cap)), blk, 0, s, B, (const uint64_t*)uniq.p, (uint64_t*)dk.p, (uint32_t*)di.p);
        AIXCHK(hipGetLastError());
        AIXCHK(sort_pairs((const uint64_t*)dk.p, (uint64_t*)dk2.p, (const uint32_t*)di.p, (uint32_t*)di2.p, S, 64u, tmp3, s));
        hipLaunchKernelGGL(k_sc_bd_off, dim3(chain_grid(NE + 1, 4 * kCB, grid_cap)), blk, 0, s, NE, (const uint64_t*)dk2.p, S, d_slink_off);
        AIXCHK(hipGetLastError());
        if (S <= cap) {
            hipLaunchKernelGGL(k_sc_bd_emit, dim3(chain_grid(S, 4 * kCB, grid_cap)), blk, 0, s, S, B, (const uint64_t*)dk2.p, (const uint32_t*)di2.p, (const ScAgg*)agg.p,
                               d_slink_to, d_slink_count, d_slink_dsum);
            AIXCHK(hipGetLastError());
        }
    } else {
        AIXCHK(hipMemsetAsync(d_slink_off, 0, 8 * (NE + 1), s));
    }
    AIXCHK(hipStreamSynchronize(s));
    *total_out = S;
    return AIX_OK;
}

// the refusals the calls over a scaffold graph share, decided before anything is allocated or launched
static int sc_check_sizes(uint64_t U, const void* offsets, const void* circular) {
    if (U > kUnitLimit) return AIX_ERR_UNSUPPORTED;
    if (!offsets || (U && !circular)) return AIX_ERR_ARG;
    return AIX_OK;
}

extern "C" int aix_scaffold_mark_dev(uint64_t U, const uint64_t* d_offsets, const uint8_t* d_circular, const uint64_t* d_slink_off, const uint32_t* d_slink_to,
                                     const uint64_t* d_slink_count, const uint64_t* d_slink_dsum, uint64_t S, uint32_t insert_size, uint64_t min_pairs,
                                     uint64_t dominance, uint64_t min_contig_bases, uint32_t* d_join, uint64_t* d_join_count, int64_t* d_join_gap,
                                     uint64_t* n_joins_out, void* stream) {
    const int st = sc_check_sizes(U, d_offsets, d_circular);
    if (st) return st;
    if (!d_slink_off || !n_joins_out || min_pairs < 1 || dominance < 1 || S >= (1ull << 60) || (S & 1)) return AIX_ERR_ARG;
    if (S && (!d_slink_to || !d_slink_count || !d_slink_dsum || !U)) return AIX_ERR_ARG;
    if (U && (!d_join || !d_join_count || !d_join_gap)) return AIX_ERR_ARG;
    if (U == 0) { *n_joins_out = 0; return AIX_OK; }
    hipStream_t s = (hipStream_t)stream;
    const uint64_t cap = chain_test_grid();
    const dim3 blk(kCB), grid(chain_grid(2 * U, kCB, cap));
    const ScGraph g{U, S, d_offsets, d_circular, d_slink_off, d_slink_to, d_slink_count, d_slink_dsum};
    Counted<ScCounters> ctr(s);
    AIXCHK(ctr.init());
    const ScCounters& hc = ctr.host;
    AIXCHK(ctr.run([&]() {
        AIX_TRY_LAUNCH(k_sc_mk_validate, grid, blk, 0, s, g, ctr.dev());
        return hipSuccess;
    }));
    if (hc.bad) return AIX_ERR_ARG;
    AIXCHK(ctr.run([&]() {
        AIX_TRY_LAUNCH(k_sc_mk_join, grid, blk, 0, s, g, insert_size, min_pairs, dominance, min_contig_bases, d_join, d_join_count, (long long*)d_join_gap, ctr.dev());
        return hipSuccess;
    }));
    *n_joins_out = hc.n;
    return AIX_OK;
}

extern "C" int aix_scaffold_layout_dev(uint64_t U, const uint64_t* d_offsets, const uint32_t* d_join, const uint64_t* d_join_count, const int64_t* d_join_gap,
                                       uint32_t min_gap, uint32_t* d_contig_scaffold, uint32_t* d_contig_rank, uint64_t* d_contig_pos, uint8_t* d_contig_flag,
                                       uint64_t* n_scaffolds_out, uint64_t* total_bases_out, uint64_t* n_cut_out, void* stream) {
    if (U > kUnitLimit) return AIX_ERR_UNSUPPORTED;
    if (!d_offsets || !n_scaffolds_out || !total_bases_out || !n_cut_out || min_gap < 1) return AIX_ERR_ARG;
    if (U && (!d_join || !d_join_count || !d_join_gap || !d_contig_scaffold || !d_contig_rank || !d_contig_pos || !d_contig_flag)) return AIX_ERR_ARG;
    if (U == 0) { *n_scaffolds_out = 0; *total_bases_out = 0; *n_cut_out = 0; return AIX_OK; }
    hipStream_t s = (hipStream_t)stream;
    const uint64_t NE = 2 * U, cap = chain_test_grid();
    const dim3 blk(kCB), grid(chain_grid(NE, 4 * kCB, cap));
    const long long* gap = (const long long*)d_join_gap;
    Counted<ScCounters> ctr(s);
    DevArr n0(s), d0(s), h0(s), n1(s), d1(s), h1(s), cs0(s), ck0(s), cs1(s), ck1(s), cut(s), first(s), isf(s), sid(s), tmp(s);
    AIXCHK(ctr.init());
    const ScCounters& hc = ctr.host;
    AIXCHK(ctr.run([&]() {
        AIX_TRY_LAUNCH(k_sc_ly_validate, grid, blk, 0, s, U, d_offsets, d_join, d_join_count, gap, ctr.dev());
        return hipSuccess;
    }));
    if (hc.bad) return AIX_ERR_ARG;
    AIXCHK(n0.alloc(8 * NE));
    AIXCHK(d0.alloc(8 * NE));
    AIXCHK(h0.alloc(4 * NE));
    AIXCHK(n1.alloc(8 * NE));
    AIXCHK(d1.alloc(8 * NE));
    AIXCHK(h1.alloc(4 * NE));
    uint64_t *cn = (uint64_t*)n0.p, *cd = (uint64_t*)d0.p, *on = (uint64_t*)n1.p, *od = (uint64_t*)d1.p;
    uint32_t *ch = (uint32_t*)h0.p, *oh = (uint32_t*)h1.p;
    uint64_t open = 0;
    AIXCHK(sc_rank(U, d_offsets, d_join, gap, min_gap, nullptr, ctr, &cn, &cd, &ch, &on, &od, &oh, &open, s));
    if (open) {                                                    // only ends on cycles are left: every cycle loses its weakest join
        AIXCHK(cs0.alloc(4 * NE));
        AIXCHK(ck0.alloc(8 * NE));
        AIXCHK(cs1.alloc(4 * NE));
        AIXCHK(ck1.alloc(8 * NE));
        AIXCHK(cut.alloc(NE));
        uint32_t *a = (uint32_t*)cs0.p, *a2 = (uint32_t*)cs1.p;
        uint64_t *k = (uint64_t*)ck0.p, *k2 = (uint64_t*)ck1.p;
        hipLaunchKernelGGL(k_sc_cy_init, grid, blk, 0, s, NE, (const uint64_t*)cn, d_join, d_join_count, a, k);
        AIXCHK(hipGetLastError());
        const int rounds = std::min(64, ceil_log2(open) + 1);
        for (int r = 1; r <= rounds; ++r) {
            hipLaunchKernelGGL(k_sc_cy_jump, grid, blk, 0, s, NE, (const uint64_t*)cn, (const uint32_t*)a, (const uint64_t*)k, a2, k2);
            AIXCHK(hipGetLastError());
            std::swap(a, a2);
            std::swap(k, k2);
        }
        hipLaunchKernelGGL(k_sc_cy_cut, grid, blk, 0, s, NE, (const uint64_t*)cn, d_join, d_join_count, (const uint64_t*)k, (uint8_t*)cut.p);
        AIXCHK(hipGetLastError());
        AIXCHK(sc_rank(U, d_offsets, d_join, gap, min_gap, (const uint8_t*)cut.p, ctr, &cn, &cd, &ch, &on, &od, &oh, &open, s));
        if (open) { set_last_error("aix_scaffold_layout_dev: ends left open behind the cycle cut"); return AIX_ERR_HIP; }
    }
    const uint64_t gaps = hc.total, n_cut = hc.cut;
    AIXCHK(first.alloc(4 * U));
    AIXCHK(isf.alloc(8 * (U + 1)));
    AIXCHK(sid.alloc(8 * (U + 1)));
    AIXCHK(ctr.run([&]() {
        AIX_TRY_LAUNCH(k_sc_ly_place, dim3(chain_grid(U + 1, 4 * kCB, cap)), blk, 0, s, U, d_offsets, (const uint64_t*)cn, (const uint64_t*)cd, (const uint32_t*)ch,
                       (uint32_t*)first.p, d_contig_rank, d_contig_pos, d_contig_flag, (uint64_t*)isf.p, ctr.dev());
        return hipSuccess;
    }));
    AIXCHK(scan_u64((const uint64_t*)isf.p, (uint64_t*)sid.p, U + 1, tmp, s));
    hipLaunchKernelGGL(k_sc_ly_assign, dim3(chain_grid(U, 4 * kCB, cap)), blk, 0, s, U, (const uint32_t*)first.p, (const uint64_t*)sid.p, d_contig_scaffold);
    AIXCHK(hipGetLastError());
    AIXCHK(hipStreamSynchronize(s));
    *n_scaffolds_out = hc.n;
    *total_bases_out = hc.total + gaps;
    *n_cut_out = n_cut;
    return AIX_OK;
}

extern "C" int aix_scaffold_emit_dev(uint64_t U, const uint64_t* d_offsets, const uint8_t* d_bases, const uint32_t* d_join, const int64_t* d_join_gap, uint32_t min_gap,
                                     const uint32_t* d_contig_scaffold, const uint32_t* d_contig_rank, const uint64_t* d_contig_pos, const uint8_t* d_contig_flag,
                                     uint64_t n_scaffolds, uint64_t total_bases, uint64_t* d_scaffold_offsets, uint8_t* d_scaffold_bases, uint64_t* d_member_off,
                                     uint32_t* d_member, int64_t* d_member_gap, void* stream) {
    if (U > kUnitLimit) return AIX_ERR_UNSUPPORTED;
    const uint64_t Sc = n_scaffolds;
    if (!d_offsets || !d_scaffold_offsets || !d_member_off || min_gap < 1 || Sc > U || (U && !Sc)) return AIX_ERR_ARG;
    if (U && (!d_bases || !d_join || !d_join_gap || !d_contig_scaffold || !d_contig_rank || !d_contig_pos || !d_contig_flag || !d_scaffold_bases || !d_member ||
              !d_member_gap))
        return AIX_ERR_ARG;
    if (U ? total_bases < 23 * U : total_bases != 0) return AIX_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (U == 0) {
        AIXCHK(hipMemsetAsync(d_scaffold_offsets, 0, 8, s));
        AIXCHK(hipMemsetAsync(d_member_off, 0, 8, s));
        AIXCHK(hipStreamSynchronize(s));
        return AIX_OK;
    }
    const uint64_t cap = chain_test_grid();
    const dim3 blk(kCB);
    const long long* gap = (const long long*)d_join_gap;
    Counted<ScCounters> ctr(s);
    DevArr keys(s), keys2(s), ids2(s), moff(s), slen(s), mstart(s), tmp(s), tmp2(s);
    AIXCHK(ctr.init());
    const ScCounters& hc = ctr.host;
    AIXCHK(keys.alloc(8 * U));
    AIXCHK(ctr.run([&]() {
        AIX_TRY_LAUNCH(k_sc_ly_validate, dim3(chain_grid(2 * U, 4 * kCB, cap)), blk, 0, s, U, d_offsets, d_join, (const uint64_t*)nullptr, gap, ctr.dev());
        AIX_TRY_LAUNCH(k_sc_em_keys, dim3(chain_grid(U, 4 * kCB, cap)), blk, 0, s, U, Sc, d_contig_scaffold, d_contig_rank, d_contig_flag, (uint64_t*)keys.p, ctr.dev());
        return hipSuccess;
    }));
    if (hc.bad) return AIX_ERR_ARG;
    AIXCHK(keys2.alloc(8 * U));
    AIXCHK(ids2.alloc(4 * U));
    AIXCHK(moff.alloc(8 * (Sc + 1)));
    AIXCHK(slen.alloc(8 * (Sc + 1)));
    AIXCHK(sort_pairs((const uint64_t*)keys.p, (uint64_t*)keys2.p, rocprim::counting_iterator<uint32_t>(0), (uint32_t*)ids2.p, U, 64u, tmp, s));
    const ScMap m{U, Sc, d_offsets, d_join, gap, d_contig_pos, d_contig_flag, (const uint64_t*)keys2.p, (const uint32_t*)ids2.p, min_gap};
    AIXCHK(ctr.run([&]() {
        AIX_TRY_LAUNCH(k_sc_em_validate, dim3(chain_grid(U + 1, 2 * kCB, cap)), blk, 0, s, m, (uint64_t*)moff.p, ctr.dev());
        return hipSuccess;
    }));
    if (hc.bad) return AIX_ERR_ARG;
    AIXCHK(ctr.run([&]() {
        AIX_TRY_LAUNCH(k_sc_em_ends, dim3(chain_grid(Sc + 1, 2 * kCB, cap)), blk, 0, s, m, (const uint64_t*)moff.p, (uint64_t*)slen.p, ctr.dev());
        return hipSuccess;
    }));
    if (hc.bad || hc.total != total_bases) return AIX_ERR_ARG;
    // everything is validated: from here on the outputs are written
    AIXCHK(mstart.alloc(8 * U));
    AIXCHK(scan_u64((const uint64_t*)slen.p, d_scaffold_offsets, Sc + 1, tmp2, s));
    AIXCHK(hipMemcpyAsync(d_member_off, moff.p, 8 * (Sc + 1), hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(k_sc_em_members, dim3(chain_grid(U, 4 * kCB, cap)), blk, 0, s, m, (const uint64_t*)d_scaffold_offsets, d_member, (long long*)d_member_gap,
                       (uint64_t*)mstart.p);
    AIXCHK(hipGetLastError());
    hipLaunchKernelGGL(k_graph_em_bases<false>, dim3(chain_grid(total_bases, 4 * kCB, cap)), blk, 0, s, U, total_bases, d_offsets, d_bases, (const uint32_t*)d_member,
                       (const uint8_t*)nullptr, (const uint64_t*)mstart.p, d_scaffold_bases);
    AIXCHK(hipGetLastError());
    AIXCHK(hipStreamSynchronize(s));
    return AIX_OK;
}

// Bundle, mark, layout, emit for host memory, on the null stream of the current device; every output is malloc'd (aix_free).
extern "C" int aix_scaffold(uint64_t U, const uint64_t* offsets, const uint8_t* bases, const uint8_t* circular, uint64_t N, const uint64_t* obs_key,
                            const uint32_t* obs_d, uint32_t insert_size, uint64_t min_pairs, uint64_t dominance, uint64_t min_contig_bases, uint32_t min_gap,
                            uint64_t* n_scaffolds_out, uint64_t* n_joins_out, uint64_t* n_cut_out, uint64_t* n_slinks_out, uint64_t** scaffold_offsets_out,
                            uint8_t** scaffold_bases_out, uint64_t** member_off_out, uint32_t** member_out, int64_t** member_gap_out, uint32_t** join_out,
                            uint64_t** join_count_out, int64_t** join_gap_out, uint32_t** contig_scaffold_out, uint32_t** contig_rank_out,
                            uint64_t** contig_pos_out, uint8_t** contig_flag_out) {
    const int st = sc_check_sizes(U, offsets, circular);
    if (st) return st;
    if (!n_scaffolds_out || !n_joins_out || !n_cut_out || !n_slinks_out || !scaffold_offsets_out || !scaffold_bases_out || !member_off_out || !member_out ||
        !member_gap_out)
        return AIX_ERR_ARG;
    if ((U && !bases) || (N && (!obs_key || !obs_d)) || min_pairs < 1 || dominance < 1 || min_gap < 1 || N >= (1ull << 60)) return AIX_ERR_ARG;
    if (N > kSLow) return AIX_ERR_UNSUPPORTED;                    // as aix_mate_bundle_dev, before the observations are copied
    // offsets are read on the host for the size of `bases` only; everything else about them is the device's to check
    const uint64_t total_in = offsets[U];
    if (U && (total_in < 23 * U || total_in > (1ULL << 48))) return AIX_ERR_ARG;
    DevArr in[5], lo, lt, lc, ld, jn, jc, jg, cs, cr, cp, cf, so, sb, mo, mm, mg;
    const HostIn ins[5] = {{offsets, 8 * (U + 1)}, {bases, total_in}, {circular, U}, {obs_key, 8 * N}, {obs_d, 4 * N}};
    AIXCHK(copy_in_host(in, ins, 5));
    const uint64_t* d_off = (const uint64_t*)in[0].p;
    uint64_t S = 0, n_joins = 0, Sc = 0, total = 0, n_cut = 0;
    AIXCHK(lo.alloc(8 * (2 * U + 1)));
    AIXCHK(lt.alloc(4 * 2 * N));                                   // S <= 2 N: one call, no sizing pass
    AIXCHK(lc.alloc(8 * 2 * N));
    AIXCHK(ld.alloc(8 * 2 * N));
    int r = aix_mate_bundle_dev(N, (const uint64_t*)in[3].p, (const uint32_t*)in[4].p, U, (uint64_t*)lo.p, (uint32_t*)lt.p, (uint64_t*)lc.p, (uint64_t*)ld.p, 2 * N, &S,
                                nullptr);
    if (r) return r;
    AIXCHK(jn.alloc(4 * 2 * U));
    AIXCHK(jc.alloc(8 * 2 * U));
    AIXCHK(jg.alloc(8 * 2 * U));
    r = aix_scaffold_mark_dev(U, d_off, (const uint8_t*)in[2].p, (const uint64_t*)lo.p, (const uint32_t*)lt.p, (const uint64_t*)lc.p, (const uint64_t*)ld.p, S, insert_size,
                              min_pairs, dominance, min_contig_bases, (uint32_t*)jn.p, (uint64_t*)jc.p, (int64_t*)jg.p, &n_joins, nullptr);
    if (r) return r;
    AIXCHK(cs.alloc(4 * U));
    AIXCHK(cr.alloc(4 * U));
    AIXCHK(cp.alloc(8 * U));
    AIXCHK(cf.alloc(U));
    r = aix_scaffold_layout_dev(U, d_off, (const uint32_t*)jn.p, (const uint64_t*)jc.p, (const int64_t*)jg.p, min_gap, (uint32_t*)cs.p, (uint32_t*)cr.p, (uint64_t*)cp.p,
                                (uint8_t*)cf.p, &Sc, &total, &n_cut, nullptr);
    if (r) return r;
    AIXCHK(so.alloc(8 * (Sc + 1)));
    AIXCHK(sb.alloc(total));
    AIXCHK(mo.alloc(8 * (Sc + 1)));
    AIXCHK(mm.alloc(4 * U));
    AIXCHK(mg.alloc(8 * U));
    r = aix_scaffold_emit_dev(U, d_off, (const uint8_t*)in[1].p, (const uint32_t*)jn.p, (const int64_t*)jg.p, min_gap, (const uint32_t*)cs.p, (const uint32_t*)cr.p,
                              (const uint64_t*)cp.p, (const uint8_t*)cf.p, Sc, total, (uint64_t*)so.p, (uint8_t*)sb.p, (uint64_t*)mo.p, (uint32_t*)mm.p, (int64_t*)mg.p,
                              nullptr);
    if (r) return r;
    const HostOut outs[] = {{(void**)scaffold_offsets_out, so.p, 8 * (Sc + 1)}, {(void**)scaffold_bases_out, sb.p, total}, {(void**)member_off_out, mo.p, 8 * (Sc + 1)},
                            {(void**)member_out, mm.p, 4 * U},                  {(void**)member_gap_out, mg.p, 8 * U},     {(void**)join_out, jn.p, 8 * U},
                            {(void**)join_count_out, jc.p, 16 * U},             {(void**)join_gap_out, jg.p, 16 * U},      {(void**)contig_scaffold_out, cs.p, 4 * U},
                            {(void**)contig_rank_out, cr.p, 4 * U},             {(void**)contig_pos_out, cp.p, 8 * U},     {(void**)contig_flag_out, cf.p, U}};
    AIXCHK(copy_out_host(outs, 12));
    *n_scaffolds_out = Sc; *n_joins_out = n_joins; *n_cut_out = n_cut; *n_slinks_out = S;
    return AIX_OK;
}
