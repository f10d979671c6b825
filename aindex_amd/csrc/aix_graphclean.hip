// aix_graphclean.hip — cleaning of a unitig graph resident in HBM: tips and weaker bubble arms are marked, and the survivors are compacted
// again into contigs, in exactly the format of the input (offsets, bases, circular, tf_*, link_off, link_to), so that the step can be
// applied repeatedly. The contract is stated above the aix_graph_* declarations in include/aindex_hip.h; DESIGN 5k has the derivations
// and the resources. No index handle: the arrays and the current device, like aix_unitig_bubbles_dev.
//
// The compaction is that of aix_unitigs.hip one level up: a node is a unitig, its two ports are its ends 2 u + 0 / 2 u + 1, at most one
// link survives per merged port. What the two levels share is in aix_chains.hpp, and why their kernels are not; what the graph files
// share (the counters holder, the predicates of k_gc_validate, the bisection) is in aix_graph.hpp. The chain (one plain
// launch per step and per round; every host loop is bounded by a count computed on the host; integer only, no LDS, no grid-wide barrier,
// no spin-wait):
//   validate k_gc_validate: one lane per end; offsets, degrees, link words, duality of the surviving links, the mates
//   mark     k_gc_mark: one lane per unitig, the tip and the arm rule over the input graph alone
//   words    k_gc_words: per end the surviving degree and, when it is 1, the end that FACES it (link ^ 1)
//   links    k_gc_links: end p is merged with f = word[p] iff word[f] == p and the two belong to different unitigs (or f == p ^ 1 closes a
//            unitig of two or more k-mers on itself). Ranking state: succ(p) = f ^ 1, d = the k-mers of the unitig jumped to; an end
//            without a merge link is a terminal (bit 63)
//   rank     k_gc_jump: synchronous pointer jumping, double-buffered, distances in k-mers and 64 bits wide; the host reads the number of
//            unflagged ends after every round and stops when it is 0 or did not change (what is left then lies on cycles)
//   cycles   only when ends are left: k_gc_cyc_init / k_gc_cyc_jump carry the minimum END id over a window of 2^r successors, the
//            distance to its first occurrence and the window's own length in k-mers
//   place    k_gc_place: per unitig its contig's start member, position and strand; rocPRIM sorts the starts by (first code, member id)
//            = the contig ids; k_gc_ids / k_gc_assign hand every member its id
//   emit     the map is validated against the graph (k_gc_mapcheck, k_gc_begin, k_gc_ends) before anything is written; members sorted by
//            (contig, position) give the byte range every member contributes; k_gc_emit is a flat grid over 16-byte output chunks that
//            find their member by bisection; k_gc_fill rewrites the links of the contig ends
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "aix_graph.hpp"

namespace aix {

// (kNoEnd, aix_graph.hpp, is here a word without a single surviving link, the contig of a removed unitig and the mate of a unitig without one)
static constexpr uint64_t kGFlag = 1ULL << 63;                    // ranking state: terminal reached
static constexpr uint64_t kGDead = ~0ULL;                         // sort key of a removed unitig / of a unitig that starts no contig
static constexpr uint32_t kGMaxThreshold = 32767;

struct GcCounters {                                               // one zeroed record per call
    unsigned long long bad, n_alive, n_starts, n_circular, total_k, links, max_pos, n_tips, n_arms;
    unsigned long long unflagged[66];                             // [0] after k_gc_links, [r] after round r
};

// (block size kCB, grid sizer, the AIX_UG_TEST_GRID hook of the compaction, wave-reduced counters: aix_chains.hpp)
__device__ __forceinline__ uint64_t gc_m(const uint64_t* __restrict__ offsets, uint64_t u) { return offsets[u + 1] - offsets[u] - 22; }
__device__ __forceinline__ uint32_t gc_base(uint32_t c) { return ((c >> 1) ^ (c >> 2)) & 3u; }               // A 0, C 1, G 2, T 3

// code of the first 23-mer of unitig [lo, hi) as given, or (reversed) of its reverse complement
__device__ __forceinline__ uint64_t gc_first_code(const uint8_t* __restrict__ bases, uint64_t lo, uint64_t hi, bool reversed) {
    uint64_t x = 0;
    if (!reversed) {
#pragma unroll
        for (int i = 0; i < 23; ++i) x = (x << 2) | gc_base(bases[lo + i]);
    } else {
#pragma unroll
        for (int i = 0; i < 23; ++i) x = (x << 2) | (3u - gc_base(bases[hi - 1 - i]));
    }
    return x;
}

__device__ __forceinline__ bool gc_alive(const uint8_t* __restrict__ remove, uint64_t u) { return !remove || remove[u] == 0; }

// ---------------------------------------------------------------------------------------------
// 1. validation of a unitig set (every later kernel relies on it: indices are used unchecked behind it)
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kCB) k_gc_validate(uint64_t U, const uint64_t* __restrict__ offsets, const uint8_t* __restrict__ circular,
                                                    const uint64_t* __restrict__ link_off, const uint32_t* __restrict__ link_to, uint64_t E,
                                                    const uint8_t* __restrict__ remove, const uint32_t* __restrict__ mate, GcCounters* __restrict__ ctr) {
    const uint64_t NE = 2 * U, stride = (uint64_t)gridDim.x * kCB;
    unsigned long long bad = 0;
    for (uint64_t e = (uint64_t)blockIdx.x * kCB + threadIdx.x; e < NE; e += stride) {
        const uint64_t u = e >> 1;
        if (!(e & 1)) {
            bad += span_bad(offsets[u], offsets[u + 1]);
            if (mate) {
                const uint32_t w = mate[u];
                if (w != kNoEnd) bad += w >= U || w == u || mate[w < U ? w : u] != u;
            }
        }
        const uint64_t lo = link_off[e], hi = link_off[e + 1];
        bad += csr_bad(e, NE, lo, hi, E, 4);
        if (!csr_in_range(lo, hi, E, 4)) continue;
        bad += circular[u] && hi > lo;
        for (uint64_t i = lo; i < hi; ++i) {
            const uint64_t t = link_to[i];
            if (t >= NE) { ++bad; continue; }
            bad += circular[t >> 1] != 0;
            if (!gc_alive(remove, u) || !gc_alive(remove, t >> 1)) continue;
            const uint64_t lo2 = link_off[t ^ 1], hi2 = link_off[(t ^ 1) + 1];
            bool dual = false;
            if (csr_in_range(lo2, hi2, E, 4))
                for (uint64_t j = lo2; j < hi2; ++j) dual = dual || link_to[j] == (uint32_t)(e ^ 1);
            bad += !dual;
        }
    }
    count_add(bad, &ctr->bad);
}

// ---------------------------------------------------------------------------------------------
// 2. mark
// ---------------------------------------------------------------------------------------------
// w outranks u: tf_sum_w m_u > tf_sum_u m_w, or equal and w < u (128-bit products: exact whatever the arrays hold)
__device__ __forceinline__ bool gc_outranks(const uint64_t* __restrict__ offsets, const uint64_t* __restrict__ tf_sum, uint64_t w, uint64_t u) {
    const unsigned __int128 a = (unsigned __int128)tf_sum[w] * gc_m(offsets, u), b = (unsigned __int128)tf_sum[u] * gc_m(offsets, w);
    return a > b || (a == b && w < u);
}

// the linked end of tip candidate u, or kNoEnd
__device__ __forceinline__ uint32_t gc_attached(const uint64_t* __restrict__ offsets, const uint8_t* __restrict__ circular, const uint64_t* __restrict__ link_off,
                                                uint64_t u, uint32_t tip_max) {
    if (circular[u] || gc_m(offsets, u) > tip_max) return kNoEnd;
    const uint64_t d0 = link_off[2 * u + 1] - link_off[2 * u], d1 = link_off[2 * u + 2] - link_off[2 * u + 1];
    if (d0 == 0 && d1 == 1) return (uint32_t)(2 * u + 1);
    if (d1 == 0 && d0 == 1) return (uint32_t)(2 * u);
    return kNoEnd;
}

__global__ void __launch_bounds__(kCB) k_gc_mark(uint64_t U, const uint64_t* __restrict__ offsets, const uint8_t* __restrict__ circular,
                                                const uint64_t* __restrict__ tf_sum, const uint64_t* __restrict__ link_off,
                                                const uint32_t* __restrict__ link_to, const uint32_t* __restrict__ mate, uint32_t tip_max, uint32_t bub_max,
                                                uint8_t* __restrict__ remove, GcCounters* __restrict__ ctr) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    unsigned long long tips = 0, arms = 0;
    for (uint64_t u = (uint64_t)blockIdx.x * kCB + threadIdx.x; u < U; u += stride) {
        uint32_t res = 0;
        const uint32_t a = tip_max ? gc_attached(offsets, circular, link_off, u, tip_max) : kNoEnd;
        if (a != kNoEnd) {
            const uint32_t f = link_to[link_off[a]] ^ 1u;           // the fork: the end that faces u
            for (uint64_t i = link_off[f]; i < link_off[f + 1]; ++i) {
                const uint64_t w = link_to[i] >> 1;
                if (w == u) continue;
                if (gc_attached(offsets, circular, link_off, w, tip_max) == kNoEnd || gc_outranks(offsets, tf_sum, w, u)) res = 1;
            }
        }
        const uint32_t w = mate[u];
        if (bub_max && w != kNoEnd && gc_m(offsets, u) <= bub_max && gc_m(offsets, w) <= bub_max && gc_outranks(offsets, tf_sum, w, u)) res = 2;
        remove[u] = (uint8_t)res;
        tips += res == 1;
        arms += res == 2;
    }
    count_add(tips, &ctr->n_tips);
    count_add(arms, &ctr->n_arms);
}

// ---------------------------------------------------------------------------------------------
// 3. surviving degrees, merge links, ranking
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kCB) k_gc_words(uint64_t U, const uint64_t* __restrict__ link_off, const uint32_t* __restrict__ link_to,
                                                 const uint8_t* __restrict__ remove, uint32_t* __restrict__ word, uint8_t* __restrict__ degp) {
    const uint64_t NE = 2 * U, stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t e = (uint64_t)blockIdx.x * kCB + threadIdx.x; e < NE; e += stride) {
        uint32_t d = 0, t1 = kNoEnd;
        if (gc_alive(remove, e >> 1))
            for (uint64_t i = link_off[e]; i < link_off[e + 1]; ++i) {
                const uint32_t t = link_to[i];
                if (gc_alive(remove, t >> 1)) { ++d; t1 = t; }
            }
        word[e] = d == 1 ? (t1 ^ 1u) : kNoEnd;
        degp[e] = (uint8_t)d;
    }
}

__global__ void __launch_bounds__(kCB) k_gc_links(const uint32_t* __restrict__ word, const uint8_t* __restrict__ degp, const uint64_t* __restrict__ offsets,
                                                 uint64_t NE, uint64_t* __restrict__ nx, uint64_t* __restrict__ dist, uint8_t* __restrict__ merged,
                                                 GcCounters* __restrict__ ctr) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    unsigned long long open = 0, links = 0;
    for (uint64_t p = (uint64_t)blockIdx.x * kCB + threadIdx.x; p < NE; p += stride) {
        const uint32_t f = word[p];
        bool linked = false;
        if ((uint64_t)f < NE && (uint64_t)word[f] == p)
            linked = (f >> 1) != (uint32_t)(p >> 1) || ((uint64_t)f == (p ^ 1) && gc_m(offsets, p >> 1) >= 2);
        nx[p] = linked ? (uint64_t)(f ^ 1u) : (p | kGFlag);
        dist[p] = linked ? gc_m(offsets, f >> 1) : 0;
        merged[p] = linked;
        open += linked;
        links += linked ? 0u : degp[p];
    }
    count_add(open, &ctr->unflagged[0]);
    count_add(links, &ctr->links);
}

__global__ void __launch_bounds__(kCB) k_gc_jump(const uint64_t* __restrict__ nx_in, const uint64_t* __restrict__ d_in, uint64_t NE, uint64_t* __restrict__ nx_out,
                                                uint64_t* __restrict__ d_out, unsigned long long* __restrict__ unflagged) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    unsigned long long open = 0;
    for (uint64_t p = (uint64_t)blockIdx.x * kCB + threadIdx.x; p < NE; p += stride) {
        uint64_t s = nx_in[p], d = d_in[p];
        if (!(s & kGFlag)) {
            const uint64_t q = s & 0xFFFFFFFFull;
            s = nx_in[q];
            d += d_in[q];                                          // on a cycle d means nothing (and may wrap)
            open += !(s & kGFlag);
        }
        nx_out[p] = s;
        d_out[p] = d;
    }
    count_add(open, unflagged);
}

// cycles: a = succ | minimum end id << 32, md = k-mers to its first occurrence, w = k-mers of the window; unflagged ends only
__global__ void __launch_bounds__(kCB) k_gc_cyc_init(const uint64_t* __restrict__ rank, const uint32_t* __restrict__ word, const uint64_t* __restrict__ offsets,
                                                    uint64_t NE, uint64_t* __restrict__ a, uint64_t* __restrict__ md, uint64_t* __restrict__ w) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t p = (uint64_t)blockIdx.x * kCB + threadIdx.x; p < NE; p += stride) {
        if (rank[p] & kGFlag) continue;
        const uint32_t succ = word[p] ^ 1u;                        // an unflagged end is merged: its word is its link
        a[p] = (uint64_t)succ | (p << 32);
        md[p] = 0;
        w[p] = gc_m(offsets, succ >> 1);
    }
}

__global__ void __launch_bounds__(kCB) k_gc_cyc_jump(const uint64_t* __restrict__ rank, uint64_t NE, const uint64_t* __restrict__ a_in,
                                                    const uint64_t* __restrict__ md_in, const uint64_t* __restrict__ w_in, uint64_t* __restrict__ a_out,
                                                    uint64_t* __restrict__ md_out, uint64_t* __restrict__ w_out) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t p = (uint64_t)blockIdx.x * kCB + threadIdx.x; p < NE; p += stride) {
        if (rank[p] & kGFlag) continue;
        const uint64_t a = a_in[p], q = a & 0xFFFFFFFFull;
        if (q >= NE || (rank[q] & kGFlag)) { a_out[p] = a; md_out[p] = md_in[p]; w_out[p] = w_in[p]; continue; }   // (never: a successor on a cycle is on it)
        const uint64_t aq = a_in[q];
        uint64_t k = a >> 32, md = md_in[p];
        if ((aq >> 32) < k) { k = aq >> 32; md = w_in[p] + md_in[q]; }   // strictly smaller: the first occurrence stays
        a_out[p] = (aq & 0xFFFFFFFFull) | (k << 32);
        md_out[p] = md;
        w_out[p] = w_in[p] + w_in[q];
    }
}

// ---------------------------------------------------------------------------------------------
// 4. layout
// ---------------------------------------------------------------------------------------------
// Per unitig. Path member: both ends are flagged; spelling A starts at the member reached through the left end (this member: position dL,
// as given), spelling B at the one reached through the right end (position dR, reversed). Cycle member: neither end is flagged.
__global__ void __launch_bounds__(kCB) k_gc_place(uint64_t U, const uint64_t* __restrict__ offsets, const uint8_t* __restrict__ bases,
                                                 const uint8_t* __restrict__ circular, const uint8_t* __restrict__ remove, const uint64_t* __restrict__ rank,
                                                 const uint64_t* __restrict__ dist, const uint64_t* __restrict__ cyc_a, const uint64_t* __restrict__ cyc_md,
                                                 uint32_t* __restrict__ start_of, uint64_t* __restrict__ pos_out, uint8_t* __restrict__ flag_out,
                                                 uint64_t* __restrict__ start_code, uint32_t* __restrict__ start_id, GcCounters* __restrict__ ctr) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    unsigned long long alive = 0, starts = 0, circ = 0, total = 0;
    for (uint64_t u = (uint64_t)blockIdx.x * kCB + threadIdx.x; u < U; u += stride) {
        start_id[u] = (uint32_t)u;
        if (remove[u]) {
            start_of[u] = kNoEnd; pos_out[u] = 0; flag_out[u] = 0; start_code[u] = kGDead;
            continue;
        }
        ++alive;
        total += gc_m(offsets, u);
        const uint64_t sR = rank[2 * u], sL = rank[2 * u + 1];
        uint64_t pos, first = 0;
        uint32_t flag, st;
        bool closed = false;
        if (circular[u]) {
            pos = 0; flag = 0; st = (uint32_t)u; closed = true;
            first = gc_first_code(bases, offsets[u], offsets[u + 1], false);
        } else if ((sR & kGFlag) || (sL & kGFlag) || !cyc_a) {
            const uint32_t eR = (uint32_t)sR, eL = (uint32_t)sL;  // the terminal ends; spelling A leaves its first member through eL ^ 1
            const uint32_t va = eL >> 1, vb = eR >> 1;
            const uint64_t fa = gc_first_code(bases, offsets[va], offsets[va + 1], !(eL & 1u));
            const uint64_t fb = gc_first_code(bases, offsets[vb], offsets[vb + 1], !(eR & 1u));
            const bool A = fa < fb || (fa == fb && va <= vb);
            pos = A ? dist[2 * u + 1] : dist[2 * u];
            flag = A ? 0u : 1u;
            st = A ? va : vb;
            first = A ? fa : fb;
        } else {
            const uint64_t kR = cyc_a[2 * u] >> 32;               // the smallest end of the directed cycle through this member's right end
            const bool keepR = (kR & 1) == 0;                      // it is the right end of the smallest member: this member is traversed forwards
            pos = cyc_md[2 * u + (keepR ? 1 : 0)];
            flag = (keepR ? 0u : 1u) | 2u;
            st = (uint32_t)(kR >> 1);
            closed = true;
            if (pos == 0) first = gc_first_code(bases, offsets[u], offsets[u + 1], false);
        }
        start_of[u] = st;
        pos_out[u] = pos;
        flag_out[u] = (uint8_t)flag;
        start_code[u] = pos == 0 ? first : kGDead;
        starts += pos == 0;
        circ += pos == 0 && closed;
    }
    count_add(alive, &ctr->n_alive);
    count_add(starts, &ctr->n_starts);
    count_add(circ, &ctr->n_circular);
    count_add(total, &ctr->total_k);
}

__global__ void __launch_bounds__(kCB) k_gc_ids(const uint32_t* __restrict__ sorted_id, uint64_t C, uint64_t U, uint32_t* __restrict__ start_cid) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t j = (uint64_t)blockIdx.x * kCB + threadIdx.x; j < C; j += stride) {
        const uint32_t u = sorted_id[j];
        if (u < U) start_cid[u] = (uint32_t)j;
    }
}

__global__ void __launch_bounds__(kCB) k_gc_assign(const uint32_t* __restrict__ start_of, const uint32_t* __restrict__ start_cid, uint64_t U,
                                                  uint32_t* __restrict__ contig) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t u = (uint64_t)blockIdx.x * kCB + threadIdx.x; u < U; u += stride) {
        const uint32_t st = start_of[u];
        contig[u] = (uint64_t)st < U ? start_cid[st] : kNoEnd;
    }
}

// ---------------------------------------------------------------------------------------------
// 5. emit: validation of the map
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kCB) k_gc_mapcheck(uint64_t U, const uint64_t* __restrict__ offsets, const uint8_t* __restrict__ remove,
                                                    const uint32_t* __restrict__ contig, const uint64_t* __restrict__ pos, uint64_t C, GcCounters* __restrict__ ctr) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    unsigned long long alive = 0, starts = 0, bad = 0, total = 0, mx = 0;
    for (uint64_t u = (uint64_t)blockIdx.x * kCB + threadIdx.x; u < U; u += stride) {
        const uint32_t c = contig[u];
        if (remove[u]) { bad += c != kNoEnd; continue; }
        ++alive;
        bad += (uint64_t)c >= C;
        starts += pos[u] == 0;
        total += gc_m(offsets, u);
        mx = pos[u] > mx ? pos[u] : mx;
    }
    count_add(alive, &ctr->n_alive);
    count_add(starts, &ctr->n_starts);
    count_add(bad, &ctr->bad);
    count_add(total, &ctr->total_k);
    count_max(mx, &ctr->max_pos);
}

__global__ void __launch_bounds__(kCB) k_gc_keys(uint64_t U, int pos_bits, const uint8_t* __restrict__ remove, const uint32_t* __restrict__ contig,
                                                const uint64_t* __restrict__ pos, uint64_t* __restrict__ keys, uint32_t* __restrict__ ids) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t u = (uint64_t)blockIdx.x * kCB + threadIdx.x; u < U; u += stride) {
        keys[u] = remove[u] ? kGDead : (((uint64_t)contig[u] << pos_bits) | pos[u]);
        ids[u] = (uint32_t)u;
    }
}

__global__ void __launch_bounds__(kCB) k_gc_mlen(uint64_t S, const uint32_t* __restrict__ ms, uint64_t U, const uint64_t* __restrict__ offsets,
                                                uint64_t* __restrict__ mlen) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t j = (uint64_t)blockIdx.x * kCB + threadIdx.x; j <= S; j += stride) {
        const uint32_t u = j < S ? ms[j] : kNoEnd;
        mlen[j] = (uint64_t)u < U ? gc_m(offsets, u) : 0;
    }
}

// Member j of the sorted members (contig, position): kpre[j] k-mers lie in front of it. Checks that the members of every contig 0 .. C - 1
// follow each other without a gap, and writes begin[j] (the first output byte the member contributes; begin[S] = total) and the new
// offsets (scratch).
__global__ void __launch_bounds__(kCB) k_gc_begin(uint64_t S, uint64_t C, int pos_bits, const uint64_t* __restrict__ keys, const uint64_t* __restrict__ kpre,
                                                 uint64_t total, uint64_t* __restrict__ begin, uint64_t* __restrict__ new_off, GcCounters* __restrict__ ctr) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB, mask = (1ULL << pos_bits) - 1;
    unsigned long long bad = 0;
    for (uint64_t j = (uint64_t)blockIdx.x * kCB + threadIdx.x; j < S; j += stride) {
        const uint64_t key = keys[j], c = key >> pos_bits, p = key & mask;
        if (j == 0) {
            bad += c != 0 || p != 0;
            begin[S] = total;
            new_off[C] = total;
        } else {
            const uint64_t k0 = keys[j - 1], c0 = k0 >> pos_bits, p0 = k0 & mask;
            const bool next = c == c0 && p == p0 + (kpre[j] - kpre[j - 1]);
            bad += !(next || (c == c0 + 1 && p == 0));
        }
        bad += j == S - 1 && c != C - 1;
        if (c >= C) continue;
        begin[j] = kpre[j] + 22 * c + (p ? 22 : 0);
        if (p == 0) new_off[c] = kpre[j] + 22 * c;
    }
    count_add(bad, &ctr->bad);
}

// Per end of every surviving unitig: a merged end has its neighbour next to it in the same contig, in the matching orientation; any
// other end is an end of its contig, and every unitig it links to sits at the end of its own contig. Writes the degrees of the contig ends.
__global__ void __launch_bounds__(kCB) k_gc_ends(uint64_t U, uint64_t C, const uint64_t* __restrict__ offsets, const uint8_t* __restrict__ circular,
                                                const uint64_t* __restrict__ link_off, const uint32_t* __restrict__ link_to, const uint8_t* __restrict__ remove,
                                                const uint32_t* __restrict__ word, const uint8_t* __restrict__ degp, const uint8_t* __restrict__ merged,
                                                const uint32_t* __restrict__ contig, const uint64_t* __restrict__ pos, const uint8_t* __restrict__ flag,
                                                const uint64_t* __restrict__ new_off, uint32_t* __restrict__ ndeg, GcCounters* __restrict__ ctr) {
    const uint64_t NE = 2 * U, stride = (uint64_t)gridDim.x * kCB;
    unsigned long long bad = 0;
    for (uint64_t p = (uint64_t)blockIdx.x * kCB + threadIdx.x; p < NE; p += stride) {
        const uint64_t u = p >> 1;
        if (remove[u]) continue;
        const uint64_t c = contig[u], mc = new_off[c + 1] - new_off[c] - 22, mu = gc_m(offsets, u), pu = pos[u];
        const uint32_t fu = flag[u];
        const uint32_t side = ((uint32_t)p ^ fu) & 1u;             // 0: the right side of u as the contig spells it
        bad += (fu & 2u) && circular[u];
        if (merged[p]) {
            const uint32_t t = word[p] ^ 1u;                        // the link: its unitig is left through end t
            const uint64_t v = t >> 1;
            const uint32_t fv = flag[v];
            if (remove[v] || contig[v] != c || ((fu ^ fv) & 2u) || ((t ^ fv) & 1u) != side) { ++bad; continue; }
            const uint64_t pv = pos[v], mv = gc_m(offsets, v);
            const bool wrap = (fu & 2u) != 0;
            if (side == 0) bad += !(pv == pu + mu || (wrap && pv == 0 && pu + mu == mc));
            else bad += !(pv + mv == pu || (wrap && pu == 0 && pv + mv == mc));
        } else {
            bad += (fu & 2u) != 0;                                  // a member of a merged cycle has two merged ends
            if (circular[u]) { bad += mc != mu || pu != 0; continue; }
            bad += side == 0 ? pu + mu != mc : pu != 0;
            ndeg[2 * c + side] = degp[p];
            for (uint64_t i = link_off[p]; i < link_off[p + 1]; ++i) {
                const uint32_t t = link_to[i];
                const uint64_t v = t >> 1;
                if (remove[v]) continue;
                const uint64_t cv = contig[v];
                if (cv >= C) { ++bad; continue; }
                const uint32_t fv = flag[v];
                const uint64_t mcv = new_off[cv + 1] - new_off[cv] - 22;
                bad += (fv & 2u) || circular[v];
                bad += ((t ^ fv) & 1u) ? pos[v] + gc_m(offsets, v) != mcv : pos[v] != 0;
            }
        }
    }
    count_add(bad, &ctr->bad);
}

__global__ void __launch_bounds__(kCB) k_gc_fill(uint64_t U, const uint8_t* __restrict__ circular, const uint64_t* __restrict__ link_off,
                                                const uint32_t* __restrict__ link_to, const uint8_t* __restrict__ remove, const uint8_t* __restrict__ merged,
                                                const uint32_t* __restrict__ contig, const uint8_t* __restrict__ flag, const uint64_t* __restrict__ new_lo, uint64_t E2,
                                                uint32_t* __restrict__ out_to) {
    const uint64_t NE = 2 * U, stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t p = (uint64_t)blockIdx.x * kCB + threadIdx.x; p < NE; p += stride) {
        const uint64_t u = p >> 1;
        if (remove[u] || merged[p] || circular[u]) continue;
        uint64_t at = new_lo[2 * (uint64_t)contig[u] + (((uint32_t)p ^ flag[u]) & 1u)];
        for (uint64_t i = link_off[p]; i < link_off[p + 1]; ++i) {
            const uint32_t t = link_to[i];
            const uint64_t v = t >> 1;
            if (remove[v]) continue;
            if (at < E2) out_to[at] = 2u * contig[v] + ((t ^ flag[v]) & 1u);
            ++at;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// 6. emit: bases, per output byte
// ---------------------------------------------------------------------------------------------
struct Gc16 {
    uint64_t lo, hi;
};

// the 16 bytes at [src, src + 16) of an 8-byte aligned array of `total` bytes, through aligned words; a word is read only if it holds a byte
// of the array, bytes at or beyond `total` are undefined
__device__ __forceinline__ Gc16 gc_load16(const uint64_t* __restrict__ words, uint64_t src, uint64_t total) {
    const uint64_t a = src >> 3, nw = (total + 7) >> 3;
    const uint32_t sh = (uint32_t)(src & 7) * 8;
    const uint64_t w0 = a < nw ? words[a] : 0, w1 = a + 1 < nw ? words[a + 1] : 0, w2 = (sh && a + 2 < nw) ? words[a + 2] : 0;
    Gc16 r;
    r.lo = sh ? (w0 >> sh) | (w1 << (64 - sh)) : w0;
    r.hi = sh ? (w1 >> sh) | (w2 << (64 - sh)) : w1;
    return r;
}

// A <-> T, C <-> G of eight ASCII bytes: bit 1 of a byte tells C / G (xor 0x04) from A / T (xor 0x15)
__device__ __forceinline__ uint64_t gc_comp8(uint64_t w) {
    const uint64_t cg = ((w >> 1) & 0x0101010101010101ull) * 0xFFull;
    return w ^ ((cg & 0x0404040404040404ull) | (~cg & 0x1515151515151515ull));
}

__global__ void __launch_bounds__(kCB) k_gc_emit(uint64_t S, const uint64_t* __restrict__ begin, const uint32_t* __restrict__ ms, const uint64_t* __restrict__ keys,
                                                int pos_bits, const uint64_t* __restrict__ offsets, const uint8_t* __restrict__ flag,
                                                const uint64_t* __restrict__ words_in, uint64_t total_in, uint8_t* __restrict__ out, uint64_t total) {
    const uint64_t chunks = (total + 15) >> 4, stride = (uint64_t)gridDim.x * kCB, mask = (1ULL << pos_bits) - 1;
    for (uint64_t ch = (uint64_t)blockIdx.x * kCB + threadIdx.x; ch < chunks; ch += stride) {
        const uint64_t o = ch << 4, end = o + 16 < total ? o + 16 : total;
        const uint64_t lo = last_le(begin, 0, S, o);               // the last member with begin <= o (begin[0] == 0)
        unsigned __int128 acc = 0;
        uint64_t cur = o;
        for (uint64_t j = lo; cur < end && j < S; ++j) {           // at most 16 trips: every member contributes a byte
            const uint64_t b0 = begin[j], b1 = begin[j + 1];
            if (b0 > cur || b1 <= cur) break;                      // (never behind k_gc_begin)
            const uint64_t seg_end = b1 < end ? b1 : end, n = seg_end - cur;
            const uint32_t u = ms[j];
            const uint64_t in_lo = offsets[u], len = offsets[u + 1] - in_lo;
            const uint64_t i0 = ((keys[j] & mask) ? 22 : 0) + (cur - b0);      // index into the oriented spelling
            if (i0 + n > len) break;                               // (never)
            unsigned __int128 v;
            if (!(flag[u] & 1u)) {
                const Gc16 g = gc_load16(words_in, in_lo + i0, total_in);
                v = ((unsigned __int128)g.hi << 64) | g.lo;
            } else {
                const Gc16 g = gc_load16(words_in, in_lo + len - i0 - n, total_in);
                v = ((unsigned __int128)gc_comp8(__builtin_bswap64(g.lo)) << 64) | gc_comp8(__builtin_bswap64(g.hi));
                v >>= 8 * (16 - (uint32_t)n);
            }
            if (n < 16) v &= ((unsigned __int128)1 << (8 * (uint32_t)n)) - 1;
            acc |= v << (8 * (uint32_t)(cur - o));
            cur = seg_end;
        }
        const uint64_t a0 = (uint64_t)acc, a1 = (uint64_t)(acc >> 64);
        if (o + 16 <= total) {
            *reinterpret_cast<uint4*>(out + o) = make_uint4((uint32_t)a0, (uint32_t)(a0 >> 32), (uint32_t)a1, (uint32_t)(a1 >> 32));
        } else {
            for (uint64_t i = o; i < end; ++i) out[i] = (uint8_t)((i - o < 8 ? a0 >> (8 * (i - o)) : a1 >> (8 * (i - o - 8))));
        }
    }
}

// ---------------------------------------------------------------------------------------------
// 7. emit: per-contig values
// ---------------------------------------------------------------------------------------------
// (the {sum, min, max} aggregate, its reduction by contig and the kernel that scatters the result: aix_chains.hpp)
__global__ void __launch_bounds__(kCB) k_gc_gather(uint64_t S, const uint32_t* __restrict__ ms, const uint64_t* __restrict__ keys, int pos_bits, uint64_t C,
                                                  const uint8_t* __restrict__ circular, const uint8_t* __restrict__ flag, const uint64_t* __restrict__ tf_sum,
                                                  const uint32_t* __restrict__ tf_min, const uint32_t* __restrict__ tf_max, ChainAgg* __restrict__ agg,
                                                  uint8_t* __restrict__ out_circular) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB, mask = (1ULL << pos_bits) - 1;
    for (uint64_t j = (uint64_t)blockIdx.x * kCB + threadIdx.x; j < S; j += stride) {
        const uint32_t u = ms[j];
        agg[j] = ChainAgg{tf_sum[u], tf_min[u], tf_max[u]};
        const uint64_t c = keys[j] >> pos_bits;
        if ((keys[j] & mask) == 0 && c < C) out_circular[c] = (uint8_t)((circular[u] != 0) | ((flag[u] >> 1) & 1u));
    }
}

struct GcGraph {                                                  // a unitig set in HBM
    uint64_t U, E;
    const uint64_t* offsets;
    const uint8_t* bases;
    const uint8_t* circular;
    const uint64_t *tf_sum;
    const uint32_t *tf_min, *tf_max;
    const uint64_t* link_off;
    const uint32_t* link_to;
};

// *bad: the arrays are no unitig set (with `remove`: one of its surviving links has no dual). Synchronises `s`.
static hipError_t gc_validate(const GcGraph& g, const uint8_t* remove, const uint32_t* mate, Counted<GcCounters>& ctr, bool* bad, hipStream_t s) {
    AIX_TRY(ctr.run([&]() {
        AIX_TRY_LAUNCH(k_gc_validate, dim3(chain_grid(2 * g.U, 2 * kCB, chain_test_grid())), dim3(kCB), 0, s, g.U, g.offsets, g.circular, g.link_off, g.link_to, g.E, remove, mate,
                       ctr.dev());
        return hipSuccess;
    }));
    *bad = ctr.host.bad != 0;
    return hipSuccess;
}

static hipError_t gc_mark(const GcGraph& g, const uint32_t* mate, uint32_t tip_max, uint32_t bub_max, uint8_t* remove, uint64_t out[2], bool* bad, hipStream_t s) {
    Counted<GcCounters> ctr(s);
    AIX_TRY(ctr.init());
    AIX_TRY(gc_validate(g, nullptr, mate, ctr, bad, s));
    if (*bad) return hipSuccess;
    AIX_TRY(ctr.run([&]() {
        AIX_TRY_LAUNCH(k_gc_mark, dim3(chain_grid(g.U, 2 * kCB, chain_test_grid())), dim3(kCB), 0, s, g.U, g.offsets, g.circular, g.tf_sum, g.link_off, g.link_to, mate, tip_max,
                       bub_max, remove, ctr.dev());
        return hipSuccess;
    }));
    out[0] = ctr.host.n_tips;
    out[1] = ctr.host.n_arms;
    return hipSuccess;
}

// surviving degrees and merge links of (g, remove): word[2 U], degp[2 U], merged[2 U], the initial ranking state, and the counters
// unflagged[0] and links. No synchronisation.
static hipError_t gc_merge_links(const GcGraph& g, const uint8_t* remove, uint32_t* word, uint8_t* degp, uint8_t* merged, uint64_t* nx, uint64_t* dist,
                                 GcCounters* ctr, hipStream_t s) {
    const uint64_t NE = 2 * g.U, cap = chain_test_grid();
    AIX_TRY_LAUNCH(k_gc_words, dim3(chain_grid(NE, 4 * kCB, cap)), dim3(kCB), 0, s, g.U, g.link_off, g.link_to, remove, word, degp);
    AIX_TRY_LAUNCH(k_gc_links, dim3(chain_grid(NE, 4 * kCB, cap)), dim3(kCB), 0, s, (const uint32_t*)word, (const uint8_t*)degp, g.offsets, NE, nx, dist, merged, ctr);
    return hipSuccess;
}

// out: C, total bases, links of the contig ends, circular contigs. Synchronises `s`.
static hipError_t gc_layout(const GcGraph& g, const uint8_t* remove, uint32_t* contig, uint64_t* pos, uint8_t* flag, uint64_t out[4], bool* bad, hipStream_t s) {
    const uint64_t U = g.U, NE = 2 * U, cap = chain_test_grid();
    const dim3 blk(kCB);
    Counted<GcCounters> ctr(s);
    DevArr word(s), degp(s), mg(s), n0(s), d0(s), n1(s), d1(s), ca0(s), cm0(s), cw0(s), ca1(s), cm1(s), cw1(s), so(s), sc(s), si(s), sc2(s), si2(s), cid(s), tmp(s);
    AIX_TRY(ctr.init());
    const GcCounters& hc = ctr.host;
    AIX_TRY(gc_validate(g, remove, nullptr, ctr, bad, s));
    if (*bad) return hipSuccess;
    if (U == 0) return hipSuccess;
    AIX_TRY(word.alloc(4 * NE));
    AIX_TRY(degp.alloc(NE));
    AIX_TRY(mg.alloc(NE));
    AIX_TRY(n0.alloc(8 * NE));
    AIX_TRY(d0.alloc(8 * NE));
    AIX_TRY(n1.alloc(8 * NE));
    AIX_TRY(d1.alloc(8 * NE));
    AIX_TRY(ctr.run([&]() { return gc_merge_links(g, remove, (uint32_t*)word.p, (uint8_t*)degp.p, (uint8_t*)mg.p, (uint64_t*)n0.p, (uint64_t*)d0.p, ctr.dev(), s); }));
    const uint64_t links = hc.links;
    uint64_t *cn = (uint64_t*)n0.p, *cd = (uint64_t*)d0.p, *on = (uint64_t*)n1.p, *od = (uint64_t*)d1.p;
    uint64_t open = hc.unflagged[0];
    AIX_TRY(chain_rank(U, ctr.dev()->unflagged, &open, s, [&](int r) {
        AIX_TRY_LAUNCH(k_gc_jump, dim3(chain_grid(NE, 4 * kCB, cap)), blk, 0, s, (const uint64_t*)cn, (const uint64_t*)cd, NE, on, od, &ctr.dev()->unflagged[r]);
        std::swap(cn, on);
        std::swap(cd, od);
        return hipSuccess;
    }));                                                           // open: only ends on cycles are left
    const uint64_t *cyc_a = nullptr, *cyc_md = nullptr;
    if (open) {
        AIX_TRY(ca0.alloc(8 * NE));
        AIX_TRY(cm0.alloc(8 * NE));
        AIX_TRY(cw0.alloc(8 * NE));
        AIX_TRY(ca1.alloc(8 * NE));
        AIX_TRY(cm1.alloc(8 * NE));
        AIX_TRY(cw1.alloc(8 * NE));
        uint64_t *a = (uint64_t*)ca0.p, *m = (uint64_t*)cm0.p, *w = (uint64_t*)cw0.p, *a2 = (uint64_t*)ca1.p, *m2 = (uint64_t*)cm1.p, *w2 = (uint64_t*)cw1.p;
        AIX_TRY_LAUNCH(k_gc_cyc_init, dim3(chain_grid(NE, 4 * kCB, cap)), blk, 0, s, (const uint64_t*)cn, (const uint32_t*)word.p, g.offsets, NE, a, m, w);
        const int rounds = std::min(64, ceil_log2(open) + 1);
        for (int r = 1; r <= rounds; ++r) {
            AIX_TRY_LAUNCH(k_gc_cyc_jump, dim3(chain_grid(NE, 4 * kCB, cap)), blk, 0, s, (const uint64_t*)cn, NE, (const uint64_t*)a, (const uint64_t*)m, (const uint64_t*)w, a2,
                m2, w2);
            std::swap(a, a2);
            std::swap(m, m2);
            std::swap(w, w2);
        }
        cyc_a = a; cyc_md = m;
    }
    AIX_TRY(so.alloc(4 * U));
    AIX_TRY(sc.alloc(8 * U));
    AIX_TRY(si.alloc(4 * U));
    AIX_TRY(ctr.run([&]() {
        AIX_TRY_LAUNCH(k_gc_place, dim3(chain_grid(U, 2 * kCB, cap)), blk, 0, s, U, g.offsets, g.bases, g.circular, remove, (const uint64_t*)cn, (const uint64_t*)cd, cyc_a,
                       cyc_md, (uint32_t*)so.p, pos, flag, (uint64_t*)sc.p, (uint32_t*)si.p, ctr.dev());
        return hipSuccess;
    }));
    const uint64_t C = std::min<uint64_t>(hc.n_starts, U);
    AIX_TRY(sc2.alloc(8 * U));
    AIX_TRY(si2.alloc(4 * U));
    AIX_TRY(cid.alloc(4 * U));
    AIX_TRY(sort_pairs((const uint64_t*)sc.p, (uint64_t*)sc2.p, (const uint32_t*)si.p, (uint32_t*)si2.p, U, 64u, tmp, s));
    AIX_TRY(hipMemsetAsync(cid.p, 0xFF, 4 * U, s));
    AIX_TRY_LAUNCH(k_gc_ids, dim3(chain_grid(C, 4 * kCB, cap)), blk, 0, s, (const uint32_t*)si2.p, C, U, (uint32_t*)cid.p);
    AIX_TRY_LAUNCH(k_gc_assign, dim3(chain_grid(U, 4 * kCB, cap)), blk, 0, s, (const uint32_t*)so.p, (const uint32_t*)cid.p, U, contig);
    out[0] = C;
    out[1] = hc.total_k + 22 * C;
    out[2] = links;
    out[3] = hc.n_circular;
    return hipStreamSynchronize(s);
}

struct GcOut {                                                    // G' in HBM, sized by (C, total, E2)
    uint64_t* offsets;
    uint8_t* bases;
    uint8_t* circular;
    uint64_t* tf_sum;
    uint32_t *tf_min, *tf_max;
    uint64_t* link_off;
    uint32_t* link_to;
};

// *status: AIX_ERR_ARG when the graph, the map or the three sizes disagree (nothing was written then), AIX_ERR_UNSUPPORTED when a sort key
// does not fit 63 bits. Synchronises `s`.
static hipError_t gc_emit(const GcGraph& g, const uint8_t* remove, const uint32_t* contig, const uint64_t* pos, const uint8_t* flag, uint64_t C, uint64_t total,
                          uint64_t E2, const GcOut& o, int* status, hipStream_t s) {
    const uint64_t U = g.U, NE = 2 * U, cap = chain_test_grid();
    const dim3 blk(kCB);
    *status = AIX_ERR_ARG;
    Counted<GcCounters> ctr(s);
    DevArr word(s), degp(s), mg(s), n0(s), d0(s), keys(s), ids(s), keys2(s), ms(s), tmp(s), mlen(s), kpre(s), begin(s), noff(s), ndeg(s), nlo(s), agg(s), uniq(s), ragg(s),
        cnt(s);
    AIX_TRY(ctr.init());
    const GcCounters& hc = ctr.host;
    bool bad = false;
    AIX_TRY(gc_validate(g, remove, nullptr, ctr, &bad, s));
    if (bad) return hipSuccess;
    uint64_t total_in = 0;
    AIX_TRY(hipMemcpyAsync(&total_in, g.offsets + U, 8, hipMemcpyDeviceToHost, s));
    AIX_TRY(ctr.run([&]() {
        AIX_TRY_LAUNCH(k_gc_mapcheck, dim3(chain_grid(U, 2 * kCB, cap)), blk, 0, s, U, g.offsets, remove, contig, pos, C, ctr.dev());
        return hipSuccess;
    }));
    const uint64_t S = hc.n_alive;
    if (hc.bad || hc.n_starts != C || S < C || (C == 0 && S) || hc.total_k + 22 * C != total || (S && hc.max_pos >= hc.total_k)) return hipSuccess;
    if (C == 0) {
        if (E2) return hipSuccess;
        AIX_TRY(hipMemsetAsync(o.offsets, 0, 8, s));
        AIX_TRY(hipMemsetAsync(o.link_off, 0, 8, s));
        *status = AIX_OK;
        return hipStreamSynchronize(s);
    }
    const int pos_bits = bit_length(hc.max_pos);
    if (pos_bits + bit_length(C) > 63) { *status = AIX_ERR_UNSUPPORTED; return hipSuccess; }
    AIX_TRY(word.alloc(4 * NE));
    AIX_TRY(degp.alloc(NE));
    AIX_TRY(mg.alloc(NE));
    AIX_TRY(n0.alloc(8 * NE));
    AIX_TRY(d0.alloc(8 * NE));
    AIX_TRY(hipMemsetAsync(ctr.dev(), 0, sizeof(GcCounters), s));   // (its counters are not read here: no run())
    AIX_TRY(gc_merge_links(g, remove, (uint32_t*)word.p, (uint8_t*)degp.p, (uint8_t*)mg.p, (uint64_t*)n0.p, (uint64_t*)d0.p, ctr.dev(), s));
    AIX_TRY(keys.alloc(8 * U));
    AIX_TRY(ids.alloc(4 * U));
    AIX_TRY(keys2.alloc(8 * U));
    AIX_TRY(ms.alloc(4 * U));
    AIX_TRY_LAUNCH(k_gc_keys, dim3(chain_grid(U, 4 * kCB, cap)), blk, 0, s, U, pos_bits, remove, contig, pos, (uint64_t*)keys.p, (uint32_t*)ids.p);
    AIX_TRY(sort_pairs((const uint64_t*)keys.p, (uint64_t*)keys2.p, (const uint32_t*)ids.p, (uint32_t*)ms.p, U, 64u, tmp, s));
    AIX_TRY(hipStreamSynchronize(s));
    n0.drop(); d0.drop(); keys.drop(); ids.drop();
    AIX_TRY(mlen.alloc(8 * (S + 1)));
    AIX_TRY(kpre.alloc(8 * (S + 1)));
    AIX_TRY(begin.alloc(8 * (S + 1)));
    AIX_TRY(noff.alloc(8 * (C + 1)));
    AIX_TRY_LAUNCH(k_gc_mlen, dim3(chain_grid(S + 1, 4 * kCB, cap)), blk, 0, s, S, (const uint32_t*)ms.p, U, g.offsets, (uint64_t*)mlen.p);
    AIX_TRY(scan_u64((const uint64_t*)mlen.p, (uint64_t*)kpre.p, S + 1, tmp, s));
    AIX_TRY(ctr.run([&]() {
        AIX_TRY(hipMemsetAsync(noff.p, 0, 8 * (C + 1), s));
        AIX_TRY_LAUNCH(k_gc_begin, dim3(chain_grid(S, 4 * kCB, cap)), blk, 0, s, S, C, pos_bits, (const uint64_t*)keys2.p, (const uint64_t*)kpre.p, total, (uint64_t*)begin.p,
                       (uint64_t*)noff.p, ctr.dev());
        return hipSuccess;
    }));
    if (hc.bad) return hipSuccess;
    AIX_TRY(ndeg.alloc(4 * (2 * C + 1)));
    AIX_TRY(nlo.alloc(8 * (2 * C + 1)));
    AIX_TRY(hipMemsetAsync(ndeg.p, 0, 4 * (2 * C + 1), s));
    AIX_TRY_LAUNCH(k_gc_ends, dim3(chain_grid(NE, 2 * kCB, cap)), blk, 0, s, U, C, g.offsets, g.circular, g.link_off, g.link_to, remove, (const uint32_t*)word.p,
        (const uint8_t*)degp.p, (const uint8_t*)mg.p, contig, pos, flag, (const uint64_t*)noff.p, (uint32_t*)ndeg.p, ctr.dev());   // (on top of the zero bad of k_gc_begin: no run())
    AIX_TRY(scan_u64(rocprim::make_transform_iterator((const uint32_t*)ndeg.p, Widen<uint32_t>()), (uint64_t*)nlo.p, 2 * C + 1, tmp, s));
    uint64_t E_new = 0;
    AIX_TRY(hipMemcpyAsync(&E_new, (const uint64_t*)nlo.p + 2 * C, 8, hipMemcpyDeviceToHost, s));
    AIX_TRY(chain_read(&ctr.host, ctr.dev(), s));
    if (hc.bad || E_new != E2) return hipSuccess;
    // everything is validated: from here on the outputs are written
    AIX_TRY(hipMemcpyAsync(o.offsets, noff.p, 8 * (C + 1), hipMemcpyDeviceToDevice, s));
    AIX_TRY(hipMemcpyAsync(o.link_off, nlo.p, 8 * (2 * C + 1), hipMemcpyDeviceToDevice, s));
    if (E2)
        AIX_TRY_LAUNCH(k_gc_fill, dim3(chain_grid(NE, 4 * kCB, cap)), blk, 0, s, U, g.circular, g.link_off, g.link_to, remove, (const uint8_t*)mg.p, contig, flag,
            (const uint64_t*)nlo.p, E2, o.link_to);
    AIX_TRY_LAUNCH(k_gc_emit, dim3(chain_grid((total + 15) >> 4, kCB, cap)), blk, 0, s, S, (const uint64_t*)begin.p, (const uint32_t*)ms.p, (const uint64_t*)keys2.p, pos_bits,
        g.offsets, flag, reinterpret_cast<const uint64_t*>(g.bases), total_in, o.bases, total);
    AIX_TRY(agg.alloc(sizeof(ChainAgg) * S));
    AIX_TRY(uniq.alloc(8 * C));
    AIX_TRY(ragg.alloc(sizeof(ChainAgg) * C));
    AIX_TRY(cnt.alloc(8));
    AIX_TRY_LAUNCH(k_gc_gather, dim3(chain_grid(S, 4 * kCB, cap)), blk, 0, s, S, (const uint32_t*)ms.p, (const uint64_t*)keys2.p, pos_bits, C, g.circular, flag, g.tf_sum, g.tf_min,
        g.tf_max, (ChainAgg*)agg.p, o.circular);
    auto kin = rocprim::make_transform_iterator((const uint64_t*)keys2.p, ChainUnitOf{pos_bits});
    AIX_TRY(with_temp(tmp, [&](void* t, size_t& tb) {
        return rocprim::reduce_by_key(t, tb, kin, (const ChainAgg*)agg.p, (size_t)S, (uint64_t*)uniq.p, (ChainAgg*)ragg.p, (uint64_t*)cnt.p, ChainAggOp(),
                                      rocprim::equal_to<uint64_t>(), s);
    }));
    AIX_TRY_LAUNCH(k_chain_stats<ChainAgg>, dim3(chain_grid(C, 4 * kCB, cap)), blk, 0, s, (const uint64_t*)uniq.p, (const ChainAgg*)ragg.p, (const uint64_t*)cnt.p, C, o.tf_sum,
                   o.tf_min, o.tf_max);
    *status = AIX_OK;
    return hipStreamSynchronize(s);
}

}  // namespace aix

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
// the refusals every entry point shares, decided before anything is allocated or launched
static int gc_check_sizes(uint64_t U, const void* offsets, const void* circular, const void* link_off, const void* link_to, uint64_t E) {
    if (U > kUnitLimit) return AIX_ERR_UNSUPPORTED;
    if (!offsets || !link_off) return AIX_ERR_ARG;
    if (U && !circular) return AIX_ERR_ARG;
    if (E && !link_to) return AIX_ERR_ARG;
    if (E > 8 * U) return AIX_ERR_ARG;
    return AIX_OK;
}

extern "C" int aix_graph_mark_dev(uint64_t U, const uint64_t* d_offsets, const uint8_t* d_circular, const uint64_t* d_tf_sum, const uint64_t* d_link_off,
                                  const uint32_t* d_link_to, uint64_t E, const uint32_t* d_bubble_mate, uint32_t tip_max_kmers, uint32_t bubble_max_kmers,
                                  uint8_t* d_remove, uint64_t* n_tips_out, uint64_t* n_arms_out, void* stream) {
    const int st = gc_check_sizes(U, d_offsets, d_circular, d_link_off, d_link_to, E);
    if (st) return st;
    if (tip_max_kmers > kGMaxThreshold || bubble_max_kmers > kGMaxThreshold) return AIX_ERR_ARG;
    if (!n_tips_out || !n_arms_out || (U && (!d_tf_sum || !d_remove))) return AIX_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    uint64_t out[2] = {0, 0};
    if (U) {
        DevArr bm(s);
        const uint32_t* mate = d_bubble_mate;
        if (!mate) {
            AIXCHK(bm.alloc(4 * U));
            const int r = aix_unitig_bubbles_dev(U, d_link_off, d_link_to, E, (uint32_t*)bm.p, stream);
            if (r) return r;
            mate = (const uint32_t*)bm.p;
        }
        const GcGraph g{U, E, d_offsets, nullptr, d_circular, d_tf_sum, nullptr, nullptr, d_link_off, d_link_to};
        bool bad = false;
        AIXCHK(gc_mark(g, mate, tip_max_kmers, bubble_max_kmers, d_remove, out, &bad, s));
        if (bad) return AIX_ERR_ARG;
    }
    *n_tips_out = out[0];
    *n_arms_out = out[1];
    return AIX_OK;
}

extern "C" int aix_graph_compact_layout_dev(uint64_t U, const uint64_t* d_offsets, const uint8_t* d_bases, const uint8_t* d_circular, const uint64_t* d_link_off,
                                            const uint32_t* d_link_to, uint64_t E, const uint8_t* d_remove, uint32_t* d_unitig_contig, uint64_t* d_unitig_pos,
                                            uint8_t* d_unitig_flag, uint64_t* n_contigs_out, uint64_t* total_bases_out, uint64_t* n_links_out,
                                            uint64_t* n_circular_out, void* stream) {
    const int st = gc_check_sizes(U, d_offsets, d_circular, d_link_off, d_link_to, E);
    if (st) return st;
    if (!n_contigs_out || !total_bases_out || !n_links_out || !n_circular_out) return AIX_ERR_ARG;
    if (U && (!d_bases || !d_remove || !d_unitig_contig || !d_unitig_pos || !d_unitig_flag)) return AIX_ERR_ARG;
    const GcGraph g{U, E, d_offsets, d_bases, d_circular, nullptr, nullptr, nullptr, d_link_off, d_link_to};
    uint64_t out[4] = {0, 0, 0, 0};
    bool bad = false;
    AIXCHK(gc_layout(g, d_remove, d_unitig_contig, d_unitig_pos, d_unitig_flag, out, &bad, (hipStream_t)stream));
    if (bad) return AIX_ERR_ARG;
    *n_contigs_out = out[0]; *total_bases_out = out[1]; *n_links_out = out[2]; *n_circular_out = out[3];
    return AIX_OK;
}

extern "C" int aix_graph_compact_emit_dev(uint64_t U, const uint64_t* d_offsets, const uint8_t* d_bases, const uint8_t* d_circular, const uint64_t* d_tf_sum,
                                          const uint32_t* d_tf_min, const uint32_t* d_tf_max, const uint64_t* d_link_off, const uint32_t* d_link_to, uint64_t E,
                                          const uint8_t* d_remove, const uint32_t* d_unitig_contig, const uint64_t* d_unitig_pos, const uint8_t* d_unitig_flag,
                                          uint64_t C, uint64_t total_bases, uint64_t n_links, uint64_t* d_out_offsets, uint8_t* d_out_bases,
                                          uint8_t* d_out_circular, uint64_t* d_out_tf_sum, uint32_t* d_out_tf_min, uint32_t* d_out_tf_max,
                                          uint64_t* d_out_link_off, uint32_t* d_out_link_to, void* stream) {
    const int st = gc_check_sizes(U, d_offsets, d_circular, d_link_off, d_link_to, E);
    if (st) return st;
    if (!d_out_offsets || !d_out_link_off || C > U || n_links > 8 * C) return AIX_ERR_ARG;
    if (U && (!d_bases || !d_tf_sum || !d_tf_min || !d_tf_max || !d_remove || !d_unitig_contig || !d_unitig_pos || !d_unitig_flag)) return AIX_ERR_ARG;
    if (C && (!d_out_bases || !d_out_circular || !d_out_tf_sum || !d_out_tf_min || !d_out_tf_max)) return AIX_ERR_ARG;
    if (n_links && !d_out_link_to) return AIX_ERR_ARG;
    if (((uintptr_t)d_bases & 7u) || ((uintptr_t)d_out_bases & 15u)) return AIX_ERR_ARG;   // the emission loads 8 and stores 16 aligned bytes
    const GcGraph g{U, E, d_offsets, d_bases, d_circular, d_tf_sum, d_tf_min, d_tf_max, d_link_off, d_link_to};
    const GcOut o{d_out_offsets, d_out_bases, d_out_circular, d_out_tf_sum, d_out_tf_min, d_out_tf_max, d_out_link_off, d_out_link_to};
    int status = AIX_ERR_ARG;
    AIXCHK(gc_emit(g, d_remove, d_unitig_contig, d_unitig_pos, d_unitig_flag, C, total_bases, n_links, o, &status, (hipStream_t)stream));
    return status;
}

// One round for host memory: mark, layout, emit on the null stream of the current device; every output is malloc'd (aix_free).
extern "C" int aix_graph_clean(uint64_t U, const uint64_t* offsets, const uint8_t* bases, const uint8_t* circular, const uint64_t* tf_sum, const uint32_t* tf_min,
                               const uint32_t* tf_max, const uint64_t* link_off, const uint32_t* link_to, uint64_t E, uint32_t tip_max_kmers,
                               uint32_t bubble_max_kmers, uint64_t* n_contigs_out, uint64_t* n_links_out, uint64_t* n_tips_out, uint64_t* n_arms_out,
                               uint64_t** offsets_out, uint8_t** bases_out, uint8_t** circular_out, uint64_t** tf_sum_out, uint32_t** tf_min_out,
                               uint32_t** tf_max_out, uint64_t** link_off_out, uint32_t** link_to_out, uint8_t** remove_out, uint32_t** unitig_contig_out,
                               uint64_t** unitig_pos_out, uint8_t** unitig_flag_out) {
    const int st = gc_check_sizes(U, offsets, circular, link_off, link_to, E);
    if (st) return st;
    if (tip_max_kmers > kGMaxThreshold || bubble_max_kmers > kGMaxThreshold) return AIX_ERR_ARG;
    if (!n_contigs_out || !n_links_out || !n_tips_out || !n_arms_out || !offsets_out || !bases_out || !circular_out || !tf_sum_out || !tf_min_out || !tf_max_out ||
        !link_off_out || !link_to_out)
        return AIX_ERR_ARG;
    if (U && (!bases || !tf_sum || !tf_min || !tf_max)) return AIX_ERR_ARG;
    // offsets are read on the host for the size of `bases` only; everything else about them is the device's to check
    const uint64_t total_in = offsets[U];
    if (U && (total_in < 23 * U || total_in > (1ULL << 48))) return AIX_ERR_ARG;
    DevArr in[8], rm, uc, up, uf, oo, ob, oc, os, on, ox, ol, ot;
    const HostIn ins[8] = {{offsets, 8 * (U + 1)}, {bases, total_in}, {circular, U}, {tf_sum, 8 * U}, {tf_min, 4 * U}, {tf_max, 4 * U}, {link_off, 8 * (2 * U + 1)},
                           {link_to, 4 * E}};
    AIXCHK(copy_in_host(in, ins, 8));
    AIXCHK(rm.alloc(U));
    AIXCHK(uc.alloc(4 * U));
    AIXCHK(up.alloc(8 * U));
    AIXCHK(uf.alloc(U));
    uint64_t tips = 0, arms = 0, C = 0, total = 0, E2 = 0, n_circ = 0;
    int r = aix_graph_mark_dev(U, (const uint64_t*)in[0].p, (const uint8_t*)in[2].p, (const uint64_t*)in[3].p, (const uint64_t*)in[6].p, (const uint32_t*)in[7].p, E,
                               nullptr, tip_max_kmers, bubble_max_kmers, (uint8_t*)rm.p, &tips, &arms, nullptr);
    if (r) return r;
    r = aix_graph_compact_layout_dev(U, (const uint64_t*)in[0].p, (const uint8_t*)in[1].p, (const uint8_t*)in[2].p, (const uint64_t*)in[6].p, (const uint32_t*)in[7].p,
                                     E, (const uint8_t*)rm.p, (uint32_t*)uc.p, (uint64_t*)up.p, (uint8_t*)uf.p, &C, &total, &E2, &n_circ, nullptr);
    if (r) return r;
    AIXCHK(oo.alloc(8 * (C + 1)));
    AIXCHK(ob.alloc(total));
    AIXCHK(oc.alloc(C));
    AIXCHK(os.alloc(8 * C));
    AIXCHK(on.alloc(4 * C));
    AIXCHK(ox.alloc(4 * C));
    AIXCHK(ol.alloc(8 * (2 * C + 1)));
    AIXCHK(ot.alloc(4 * E2));
    r = aix_graph_compact_emit_dev(U, (const uint64_t*)in[0].p, (const uint8_t*)in[1].p, (const uint8_t*)in[2].p, (const uint64_t*)in[3].p, (const uint32_t*)in[4].p,
                                   (const uint32_t*)in[5].p, (const uint64_t*)in[6].p, (const uint32_t*)in[7].p, E, (const uint8_t*)rm.p, (const uint32_t*)uc.p,
                                   (const uint64_t*)up.p, (const uint8_t*)uf.p, C, total, E2, (uint64_t*)oo.p, (uint8_t*)ob.p, (uint8_t*)oc.p, (uint64_t*)os.p,
                                   (uint32_t*)on.p, (uint32_t*)ox.p, (uint64_t*)ol.p, (uint32_t*)ot.p, nullptr);
    if (r) return r;
    // host copies: {destination, device block, bytes}; a NULL destination is an output the caller did not ask for
    const HostOut outs[] = {
        {(void**)offsets_out, oo.p, 8 * (C + 1)}, {(void**)bases_out, ob.p, total}, {(void**)circular_out, oc.p, C}, {(void**)tf_sum_out, os.p, 8 * C},
        {(void**)tf_min_out, on.p, 4 * C}, {(void**)tf_max_out, ox.p, 4 * C}, {(void**)link_off_out, ol.p, 8 * (2 * C + 1)}, {(void**)link_to_out, ot.p, 4 * E2},
        {(void**)remove_out, rm.p, U}, {(void**)unitig_contig_out, uc.p, 4 * U}, {(void**)unitig_pos_out, up.p, 8 * U}, {(void**)unitig_flag_out, uf.p, U}};
    AIXCHK(copy_out_host(outs, 12));
    *n_contigs_out = C; *n_links_out = E2; *n_tips_out = tips; *n_arms_out = arms;
    return AIX_OK;
}
