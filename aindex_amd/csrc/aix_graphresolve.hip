// aix_graphresolve.hip — repeats resolved with threaded sequences, on a unitig graph resident in HBM: the transitions of the step arrays
// through every unitig (which entry link is followed by which exit link), the removal of links that hardly any sequence traverses, and the
// splitting of a repeat unitig into one copy per consistent (entry, exit) pair. The result is a unitig set in exactly the format of the
// input, so aix_graph_compact_* under an all-zero mask merges it into longer contigs. The contract is stated above the
// aix_thread_pairs_dev / aix_graph_resolve_* declarations in include/aindex_hip.h; DESIGN 5m has the derivations and the resources. No
// index handle: the arrays and the current device, like the cleaning. What the graph files share (the counters holder, the predicates
// of the validate kernels, the link search and the bisection) is in aix_graph.hpp. One plain launch per step; every call validates
// with counting kernels that write nothing but their counters and writes only after the host has read them as clean; integer only, no
// LDS, no grid-wide barrier, no spin-wait:
//   pairs    k_gr_linkoff, then k_gr_pairs<check> and k_gr_pairs<add>: one lane per step, a plain device-scope u64 atomicAdd per transition
//   mark     k_gr_validate (one lane per end: the unitig set, duality, symmetric support), k_gr_weak (one lane per end), k_gr_split (one
//            lane per unitig, reads the link_remove of the launch before)
//   layout   k_gr_count (one lane per unitig and per link), a scan of copies - 1, k_gr_copybase
//   emit     k_gr_validate, k_gr_count, the scan, k_gr_checksplit; then k_gr_origin, k_gr_sizes, two scans straight into offsets' and
//            link_off', k_gr_values, k_gr_links (one lane per end of G_r), a device copy of the old bases and k_gr_bases for the copies
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "aix_graph.hpp"

namespace aix {

// (kNoEnd is the copy_base of an unsplit unitig; the constants, the counters holder and the predicates of the validation: aix_graph.hpp)
struct GrCounters {                                               // one zeroed record per call
    unsigned long long bad, n_pairs, removed, n_split, added, extra_bases;
};

struct GrGraph {                                                  // a unitig set in HBM (bases and tf_* only where a call needs them)
    uint64_t U, E;
    const uint64_t* offsets;
    const uint8_t* circular;
    const uint64_t* link_off;
    const uint32_t* link_to;
};

// link_off starts at 0, ascends, ends at E, and no end has more than 4 links
__global__ void __launch_bounds__(kCB) k_gr_linkoff(uint64_t U, uint64_t E, const uint64_t* __restrict__ link_off, GrCounters* __restrict__ ctr) {
    const uint64_t NE = 2 * U, stride = (uint64_t)gridDim.x * kCB;
    unsigned long long bad = 0;
    for (uint64_t e = (uint64_t)blockIdx.x * kCB + threadIdx.x; e < NE; e += stride)
        bad += csr_bad(e, NE, link_off[e], link_off[e + 1], E, 4);
    count_add(bad, &ctr->bad);
}

// ---------------------------------------------------------------------------------------------
// 1. transitions
// ---------------------------------------------------------------------------------------------
// check = true: counts the violations and the transitions, writes nothing; false: adds (the arrays passed the check). Behind k_gr_linkoff.
template <bool kCheck>
__global__ void __launch_bounds__(kCB) k_gr_pairs(uint64_t U, uint64_t E, const uint64_t* __restrict__ link_off, const uint32_t* __restrict__ link_to, uint64_t T,
                                                 const uint32_t* __restrict__ step_unitig, const uint8_t* __restrict__ step_flag,
                                                 const uint64_t* __restrict__ step_link, unsigned long long* __restrict__ pair, GrCounters* __restrict__ ctr) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    unsigned long long bad = 0, n = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kCB + threadIdx.x; i < T; i += stride) {
        const uint64_t u = step_unitig[i], a = step_link[i];
        if (kCheck) {
            bad += u >= U;
            bad += a >= E && a < AIX_THREAD_BROKEN;
            bad += i == 0 && a < E;
        }
        if (i == 0 || i + 1 >= T || a >= E) continue;
        const uint64_t b = step_link[i + 1];
        if (b >= E) continue;
        const uint64_t up = step_unitig[i - 1];
        if (u >= U || up >= U) continue;                          // (counted by the lanes of those steps)
        const uint64_t s = step_flag[i] & 1u, e = 2 * u + s, ep = 2 * up + (step_flag[i - 1] & 1u);
        const bool ok = a >= link_off[ep] && a < link_off[ep + 1] && (uint64_t)link_to[a] == e && b >= link_off[e] && b < link_off[e + 1];
        const uint64_t d = ok ? link_find(link_to, link_off[e ^ 1], link_off[(e ^ 1) + 1], ep ^ 1) : kNoLink;   // (behind k_gr_linkoff: the list lies in [0, E))
        if (d == kNoLink) { ++bad; continue; }
        ++n;
        if (!kCheck) {
            const uint64_t x = (s ? d : b) - link_off[2 * u], y = (s ? b : d) - link_off[2 * u + 1];
            atomicAdd(pair + 16 * u + 4 * x + y, 1ull);
        }
    }
    if (kCheck) {
        count_add(bad, &ctr->bad);
        count_add(n, &ctr->n_pairs);
    }
}

// ---------------------------------------------------------------------------------------------
// 2. validation of a unitig set (every later kernel relies on it: indices are used unchecked behind it)
// ---------------------------------------------------------------------------------------------
// the validation of the cleaning block with the duality of every link; support (nullable) is equal on a link and its dual, link_remove
// (nullable) is set on both or on neither
__global__ void __launch_bounds__(kCB) k_gr_validate(const GrGraph g, const uint64_t* __restrict__ support, const uint8_t* __restrict__ link_remove,
                                                    GrCounters* __restrict__ ctr) {
    const uint64_t NE = 2 * g.U, stride = (uint64_t)gridDim.x * kCB;
    unsigned long long bad = 0;
    for (uint64_t e = (uint64_t)blockIdx.x * kCB + threadIdx.x; e < NE; e += stride) {
        const uint64_t u = e >> 1;
        if (!(e & 1)) bad += span_bad(g.offsets[u], g.offsets[u + 1]);
        const uint64_t lo = g.link_off[e], hi = g.link_off[e + 1];
        bad += csr_bad(e, NE, lo, hi, g.E, 4);
        if (!csr_in_range(lo, hi, g.E, 4)) continue;
        bad += g.circular[u] && hi > lo;
        for (uint64_t i = lo; i < hi; ++i) {
            const uint64_t t = g.link_to[i];
            if (t >= NE) { ++bad; continue; }
            bad += g.circular[t >> 1] != 0;
            const uint64_t lo2 = g.link_off[t ^ 1], hi2 = g.link_off[(t ^ 1) + 1];
            uint64_t dual = kNoLink;
            if (csr_in_range(lo2, hi2, g.E, 4))
                for (uint64_t j = hi2; j > lo2; --j)
                    if (g.link_to[j - 1] == (uint32_t)(e ^ 1)) dual = j - 1;       // the first one
            if (dual == kNoLink) { ++bad; continue; }
            if (support) bad += support[i] != support[dual];
            if (link_remove) bad += (link_remove[i] != 0) != (link_remove[dual] != 0);
        }
    }
    count_add(bad, &ctr->bad);
}

// ---------------------------------------------------------------------------------------------
// 3. mark
// ---------------------------------------------------------------------------------------------
// the end has a link that is not weak
__device__ __forceinline__ bool gr_firm(const uint64_t* __restrict__ link_off, const uint64_t* __restrict__ support, uint64_t e, uint64_t min_link) {
    bool firm = false;
    for (uint64_t j = link_off[e], hi = link_off[e + 1]; j < hi; ++j) firm = firm || support[j] >= min_link;
    return firm;
}

__global__ void __launch_bounds__(kCB) k_gr_weak(const GrGraph g, const uint64_t* __restrict__ support, uint64_t min_link, uint8_t* __restrict__ link_remove,
                                                GrCounters* __restrict__ ctr) {
    const uint64_t NE = 2 * g.U, stride = (uint64_t)gridDim.x * kCB;
    unsigned long long removed = 0;
    for (uint64_t e = (uint64_t)blockIdx.x * kCB + threadIdx.x; e < NE; e += stride) {
        const uint64_t lo = g.link_off[e], hi = g.link_off[e + 1];
        if (lo == hi) continue;
        const bool firm = gr_firm(g.link_off, support, e, min_link);
        for (uint64_t j = lo; j < hi; ++j) {
            const bool rm = support[j] < min_link && (firm || gr_firm(g.link_off, support, (uint64_t)g.link_to[j] ^ 1, min_link));
            link_remove[j] = rm ? 1 : 0;
            removed += rm;
        }
    }
    count_add(removed, &ctr->removed);
}

// the local indices of the surviving links of end e, in list order, four bits each; *n their number
__device__ __forceinline__ uint32_t gr_kept(const uint64_t* __restrict__ link_off, const uint8_t* __restrict__ link_remove, uint64_t e, uint32_t* n) {
    const uint64_t lo = link_off[e], hi = link_off[e + 1];
    uint32_t packed = 0, k = 0;
    for (uint64_t j = lo; j < hi; ++j)
        if (!link_remove[j]) { packed |= (uint32_t)(j - lo) << (4 * k); ++k; }
    *n = k;
    return packed;
}

// a surviving link of u names u itself: a hairpin or a tandem self-link
__device__ __forceinline__ bool gr_self(const uint64_t* __restrict__ link_off, const uint32_t* __restrict__ link_to, const uint8_t* __restrict__ link_remove, uint64_t u) {
    bool self = false;
    for (uint64_t j = link_off[2 * u], hi = link_off[2 * u + 2]; j < hi; ++j) self = self || (!link_remove[j] && (uint64_t)(link_to[j] >> 1) == u);
    return self;
}

struct GrMatch {                                                  // copy r of a split unitig: local index a >> 4 r & 15 at end 2 u, y >> 4 r & 15 at end 2 u + 1
    uint32_t d, a, y;
};

// the strong cells of the surviving links of u are a perfect matching of d >= 2 pairs, and (noise) every other cell is at most max_noise
__device__ __forceinline__ bool gr_match(const uint64_t* __restrict__ link_off, const uint8_t* __restrict__ link_remove, const uint64_t* __restrict__ pair, uint64_t u,
                                         uint64_t min_pair, bool noise, uint64_t max_noise, GrMatch* m) {
    uint32_t na = 0, nb = 0;
    const uint32_t A = gr_kept(link_off, link_remove, 2 * u, &na), B = gr_kept(link_off, link_remove, 2 * u + 1, &nb);
    if (na != nb || na < 2) return false;
    bool ok = true;
    uint32_t Y = 0, ycnt = 0;
    for (uint32_t r = 0; r < na; ++r) {
        const uint32_t x = (A >> (4 * r)) & 15u;
        uint32_t cnt = 0;
        for (uint32_t q = 0; q < nb; ++q) {
            const uint32_t y = (B >> (4 * q)) & 15u;
            const uint64_t c = pair[16 * u + 4 * x + y];
            if (c >= min_pair) { ++cnt; Y |= y << (4 * r); ycnt += 1u << (4 * q); }
            else if (noise && c > max_noise) ok = false;
        }
        ok = ok && cnt == 1;
    }
    for (uint32_t q = 0; q < nb; ++q) ok = ok && ((ycnt >> (4 * q)) & 15u) == 1;
    m->d = na; m->a = A; m->y = Y;
    return ok;
}

__global__ void __launch_bounds__(kCB) k_gr_split(const GrGraph g, const uint8_t* __restrict__ link_remove, const uint64_t* __restrict__ pair, uint64_t min_pair,
                                                 uint64_t max_noise, uint8_t* __restrict__ copies, GrCounters* __restrict__ ctr) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    unsigned long long n_split = 0, added = 0;
    for (uint64_t u = (uint64_t)blockIdx.x * kCB + threadIdx.x; u < g.U; u += stride) {
        uint32_t c = 1;
        GrMatch m;
        if (pair && !g.circular[u] && !gr_self(g.link_off, g.link_to, link_remove, u) && gr_match(g.link_off, link_remove, pair, u, min_pair, true, max_noise, &m)) c = m.d;
        copies[u] = (uint8_t)c;
        n_split += c > 1;
        added += c - 1;
    }
    count_add(n_split, &ctr->n_split);
    count_add(added, &ctr->added);
}

// ---------------------------------------------------------------------------------------------
// 4. layout
// ---------------------------------------------------------------------------------------------
// extra[u] = copies[u] - 1 for the scan (extra[U] = 0), the added unitigs and bases, the removed links; copies outside 1 .. 4 and offsets
// that do not ascend by 23 are counted as bad
__global__ void __launch_bounds__(kCB) k_gr_count(uint64_t U, uint64_t E, const uint64_t* __restrict__ offsets, const uint8_t* __restrict__ copies,
                                                 const uint8_t* __restrict__ link_remove, uint64_t* __restrict__ extra, GrCounters* __restrict__ ctr) {
    const uint64_t work = (U + 1 > E ? U + 1 : E), stride = (uint64_t)gridDim.x * kCB;
    unsigned long long bad = 0, added = 0, bases = 0, removed = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kCB + threadIdx.x; i < work; i += stride) {
        if (i < U) {
            const uint64_t c = copies[i], a = offsets[i], b = offsets[i + 1];
            const bool good = c >= 1 && c <= 4 && !span_bad(a, b);
            bad += !good;
            extra[i] = good ? c - 1 : 0;
            if (good) { added += c - 1; bases += (c - 1) * (b - a); }
        } else if (i == U) extra[U] = 0;
        if (i < E) removed += link_remove[i] != 0;
    }
    count_add(bad, &ctr->bad);
    count_add(added, &ctr->added);
    count_add(bases, &ctr->extra_bases);
    count_add(removed, &ctr->removed);
}

__global__ void __launch_bounds__(kCB) k_gr_copybase(uint64_t U, const uint8_t* __restrict__ copies, const uint64_t* __restrict__ pre, uint32_t* __restrict__ copy_base) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t u = (uint64_t)blockIdx.x * kCB + threadIdx.x; u < U; u += stride) copy_base[u] = copies[u] > 1 ? (uint32_t)(U + pre[u]) : kNoEnd;
}

// ---------------------------------------------------------------------------------------------
// 5. emit
// ---------------------------------------------------------------------------------------------
// copy_base is the scan; every split is one the arrays support (behind k_gr_validate and k_gr_count)
__global__ void __launch_bounds__(kCB) k_gr_checksplit(const GrGraph g, const uint8_t* __restrict__ link_remove, const uint8_t* __restrict__ copies,
                                                      const uint64_t* __restrict__ pre, const uint32_t* __restrict__ copy_base, const uint64_t* __restrict__ pair,
                                                      uint64_t min_pair, GrCounters* __restrict__ ctr) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    unsigned long long bad = 0;
    for (uint64_t u = (uint64_t)blockIdx.x * kCB + threadIdx.x; u < g.U; u += stride) {
        const uint32_t c = copies[u];
        bad += copy_base[u] != (c > 1 ? (uint32_t)(g.U + pre[u]) : kNoEnd);
        if (c == 1) continue;
        GrMatch m;
        const bool ok = pair && min_pair && !g.circular[u] && !gr_self(g.link_off, g.link_to, link_remove, u) &&
                        gr_match(g.link_off, link_remove, pair, u, min_pair, false, 0, &m) && m.d == c;
        bad += !ok;
    }
    count_add(bad, &ctr->bad);
}

__global__ void __launch_bounds__(kCB) k_gr_origin(uint64_t U, const uint8_t* __restrict__ copies, const uint32_t* __restrict__ copy_base, uint64_t U2,
                                                  uint32_t* __restrict__ origin, uint8_t* __restrict__ rank) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t u = (uint64_t)blockIdx.x * kCB + threadIdx.x; u < U; u += stride) {
        origin[u] = (uint32_t)u;
        rank[u] = 0;
        for (uint32_t r = 1; r < copies[u]; ++r) {
            const uint64_t id = (uint64_t)copy_base[u] + r - 1;
            if (id < U2) { origin[id] = (uint32_t)u; rank[id] = (uint8_t)r; }
        }
    }
}

// per unitig of G_r its length in bases and the degrees of its two ends (entry U2 / 2 U2 of the arrays is 0: the scans' totals)
__global__ void __launch_bounds__(kCB) k_gr_sizes(const GrGraph g, const uint8_t* __restrict__ link_remove, const uint8_t* __restrict__ copies, uint64_t U2,
                                                 const uint32_t* __restrict__ origin, uint64_t* __restrict__ len, uint32_t* __restrict__ ndeg) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t i = (uint64_t)blockIdx.x * kCB + threadIdx.x; i <= U2; i += stride) {
        if (i == U2) { len[i] = 0; ndeg[2 * i] = 0; continue; }
        const uint64_t u = origin[i];
        len[i] = g.offsets[u + 1] - g.offsets[u];
        uint32_t d0 = 1, d1 = 1;
        if (copies[u] == 1) { gr_kept(g.link_off, link_remove, 2 * u, &d0); gr_kept(g.link_off, link_remove, 2 * u + 1, &d1); }
        ndeg[2 * i] = d0;
        ndeg[2 * i + 1] = d1;
    }
}

// floor(a * b / den) for b <= den, den != 0: the product and the long division in 128 bits
__device__ __forceinline__ uint64_t gr_muldiv(uint64_t a, uint64_t b, unsigned __int128 den) {
    const unsigned __int128 num = (unsigned __int128)a * b;
    unsigned __int128 rem = 0;
    uint64_t q = 0;
    for (int i = 127; i >= 0; --i) {                               // rem < den < 2^66: the shift does not overflow
        rem = (rem << 1) | (unsigned __int128)((uint64_t)(num >> i) & 1u);
        const bool ge = rem >= den;
        if (ge) rem -= den;
        if (i < 64) q = (q << 1) | (ge ? 1u : 0u);                 // the quotient is at most a: its high half is zero
    }
    return q;
}

__global__ void __launch_bounds__(kCB) k_gr_values(const GrGraph g, const uint64_t* __restrict__ tf_sum, const uint32_t* __restrict__ tf_min, const uint32_t* __restrict__ tf_max,
                                                  const uint8_t* __restrict__ link_remove, const uint8_t* __restrict__ copies, const uint64_t* __restrict__ pair,
                                                  uint64_t min_pair, uint64_t U2, const uint32_t* __restrict__ origin, const uint8_t* __restrict__ rank,
                                                  uint8_t* __restrict__ out_circular, uint64_t* __restrict__ out_sum, uint32_t* __restrict__ out_min,
                                                  uint32_t* __restrict__ out_max) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t i = (uint64_t)blockIdx.x * kCB + threadIdx.x; i < U2; i += stride) {
        const uint64_t u = origin[i];
        uint64_t tf = tf_sum[u];
        GrMatch m;
        if (copies[u] > 1 && gr_match(g.link_off, link_remove, pair, u, min_pair, false, 0, &m)) {
            unsigned __int128 S = 0;
            for (uint32_t r = 0; r < m.d; ++r) S += pair[16 * u + 4 * ((m.a >> (4 * r)) & 15u) + ((m.y >> (4 * r)) & 15u)];
            const uint32_t mine = rank[i];
            uint64_t got = 0, rest = tf;
            for (uint32_t r = 1; r < m.d; ++r) {
                const uint64_t part = gr_muldiv(tf, pair[16 * u + 4 * ((m.a >> (4 * r)) & 15u) + ((m.y >> (4 * r)) & 15u)], S);
                rest -= part;
                if (r == mine) got = part;
            }
            tf = mine ? got : rest;
        }
        out_circular[i] = g.circular[u];
        out_sum[i] = tf;
        out_min[i] = tf_min[u];
        out_max[i] = tf_max[u];
    }
}

// the copy of unitig v that owns the link with local index `local` at end ev of v: its rank, 0 for an unsplit unitig
__device__ __forceinline__ uint32_t gr_owner(const GrGraph& g, const uint8_t* __restrict__ link_remove, const uint8_t* __restrict__ copies,
                                             const uint64_t* __restrict__ pair, uint64_t min_pair, uint64_t ev, uint32_t local) {
    const uint64_t v = ev >> 1;
    GrMatch m;
    if (copies[v] == 1 || !gr_match(g.link_off, link_remove, pair, v, min_pair, false, 0, &m)) return 0;
    const uint32_t side = (ev & 1) ? m.y : m.a;
    for (uint32_t r = 0; r < m.d; ++r)
        if (((side >> (4 * r)) & 15u) == local) return r;
    return 0;                                                      // (never behind k_gr_checksplit: every surviving link of a split end is matched)
}

// one lane per end of G_r: its surviving links, in their order, each word renamed to the copy that owns the dual
__global__ void __launch_bounds__(kCB) k_gr_links(const GrGraph g, const uint8_t* __restrict__ link_remove, const uint8_t* __restrict__ copies,
                                                 const uint32_t* __restrict__ copy_base, const uint64_t* __restrict__ pair, uint64_t min_pair, uint64_t U2,
                                                 const uint32_t* __restrict__ origin, const uint8_t* __restrict__ rank, const uint64_t* __restrict__ new_lo, uint64_t E2,
                                                 uint32_t* __restrict__ out_to) {
    const uint64_t NE2 = 2 * U2, stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t p = (uint64_t)blockIdx.x * kCB + threadIdx.x; p < NE2; p += stride) {
        const uint64_t i = p >> 1, u = origin[i], e = 2 * u + (p & 1), lo = g.link_off[e], hi = g.link_off[e + 1];
        const bool split = copies[u] > 1;
        const uint32_t mine = rank[i];
        uint64_t at = new_lo[p];
        for (uint64_t j = lo; j < hi; ++j) {
            if (link_remove[j]) continue;
            if (split && gr_owner(g, link_remove, copies, pair, min_pair, e, (uint32_t)(j - lo)) != mine) continue;
            const uint64_t t = g.link_to[j], v = t >> 1;
            uint64_t id = v;
            if (copies[v] > 1) {
                const uint64_t dual = link_find(g.link_to, g.link_off[t ^ 1], g.link_off[(t ^ 1) + 1], e ^ 1);
                const uint32_t r = dual == kNoLink ? 0 : gr_owner(g, link_remove, copies, pair, min_pair, t ^ 1, (uint32_t)(dual - g.link_off[t ^ 1]));
                if (r) id = (uint64_t)copy_base[v] + r - 1;
            }
            if (at < E2) out_to[at] = (uint32_t)(2 * id + (t & 1));
            ++at;
        }
    }
}

// the bases of the copies: output byte i in [total_in, total2) belongs to the last id in [U, U2) with new_off[id] <= i
__global__ void __launch_bounds__(kCB) k_gr_bases(uint64_t U, uint64_t U2, const uint64_t* __restrict__ offsets, const uint8_t* __restrict__ bases,
                                                 const uint32_t* __restrict__ origin, const uint64_t* __restrict__ new_off, uint64_t total_in, uint64_t total2,
                                                 uint8_t* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t i = total_in + (uint64_t)blockIdx.x * kCB + threadIdx.x; i < total2; i += stride) {
        const uint64_t lo = last_le(new_off, U, U2, i);            // new_off[U] == total_in <= i < new_off[U2]; at most 32 trips
        const uint64_t u = origin[lo], src = offsets[u] + (i - new_off[lo]);
        if (src < offsets[u + 1]) out[i] = bases[src];
    }
}

static hipError_t gr_validate(const GrGraph& g, const uint64_t* support, const uint8_t* link_remove, Counted<GrCounters>& ctr, bool* bad, hipStream_t s) {
    AIX_TRY(ctr.run([&]() {
        AIX_TRY_LAUNCH(k_gr_validate, dim3(chain_grid(2 * g.U, 2 * kCB, chain_test_grid())), dim3(kCB), 0, s, g, support, link_remove, ctr.dev());
        return hipSuccess;
    }));
    *bad = ctr.host.bad != 0;
    return hipSuccess;
}

// copies and offsets checked, extra[U + 1] scanned into pre[U + 1]; ctr.host: added, extra_bases, removed. Synchronises `s`.
static hipError_t gr_count(const GrGraph& g, const uint8_t* copies, const uint8_t* link_remove, Counted<GrCounters>& ctr, DevArr& extra, DevArr& pre, DevArr& tmp,
                           hipStream_t s) {
    AIX_TRY(extra.alloc(8 * (g.U + 1)));
    AIX_TRY(pre.alloc(8 * (g.U + 1)));
    return ctr.run([&]() {
        AIX_TRY_LAUNCH(k_gr_count, dim3(chain_grid(std::max(g.U + 1, g.E), 4 * kCB, chain_test_grid())), dim3(kCB), 0, s, g.U, g.E, g.offsets, copies, link_remove,
                       (uint64_t*)extra.p, ctr.dev());
        return scan_u64((const uint64_t*)extra.p, (uint64_t*)pre.p, g.U + 1, tmp, s);
    });
}

}  // namespace aix

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
// the refusals every entry point shares, decided before anything is allocated or launched
static int gr_check_sizes(uint64_t U, const void* offsets, const void* circular, const void* link_off, const void* link_to, uint64_t E) {
    if (U > kUnitLimit) return AIX_ERR_UNSUPPORTED;
    if (!offsets || !link_off) return AIX_ERR_ARG;
    if (U && !circular) return AIX_ERR_ARG;
    if (E && !link_to) return AIX_ERR_ARG;
    if (E > 8 * U) return AIX_ERR_ARG;
    return AIX_OK;
}

extern "C" int aix_thread_pairs_dev(uint64_t U, const uint64_t* d_link_off, const uint32_t* d_link_to, uint64_t E, uint64_t T, const uint32_t* d_step_unitig,
                                    const uint8_t* d_step_flag, const uint64_t* d_step_link, uint64_t* d_pair_support, uint64_t* n_pairs_out, void* stream) {
    if (U > kUnitLimit) return AIX_ERR_UNSUPPORTED;
    if (!n_pairs_out || E > 8 * U || T >= (1ull << 60)) return AIX_ERR_ARG;
    if (U && (!d_link_off || !d_pair_support)) return AIX_ERR_ARG;
    if (E && !d_link_to) return AIX_ERR_ARG;
    if (T && (!d_step_unitig || !d_step_flag || !d_step_link)) return AIX_ERR_ARG;
    if (T == 0 || U == 0) { *n_pairs_out = 0; return AIX_OK; }
    hipStream_t s = (hipStream_t)stream;
    const uint64_t cap = chain_test_grid();
    Counted<GrCounters> ctr(s);
    AIXCHK(ctr.init());
    const GrCounters& hc = ctr.host;
    AIXCHK(ctr.run([&]() {
        AIX_TRY_LAUNCH(k_gr_linkoff, dim3(chain_grid(2 * U, 4 * kCB, cap)), dim3(kCB), 0, s, U, E, d_link_off, ctr.dev());
        return hipSuccess;
    }));
    if (hc.bad) return AIX_ERR_ARG;
    const dim3 grid(chain_grid(T, 2 * kCB, cap)), blk(kCB);
    AIXCHK(ctr.run([&]() {
        AIX_TRY_LAUNCH(k_gr_pairs<true>, grid, blk, 0, s, U, E, d_link_off, d_link_to, T, d_step_unitig, d_step_flag, d_step_link, (unsigned long long*)d_pair_support, ctr.dev());
        return hipSuccess;
    }));
    if (hc.bad) return AIX_ERR_ARG;
    if (hc.n_pairs) {
        hipLaunchKernelGGL(k_gr_pairs<false>, grid, blk, 0, s, U, E, d_link_off, d_link_to, T, d_step_unitig, d_step_flag, d_step_link, (unsigned long long*)d_pair_support, ctr.dev());
        AIXCHK(hipGetLastError());
        AIXCHK(hipStreamSynchronize(s));
    }
    *n_pairs_out = hc.n_pairs;
    return AIX_OK;
}

extern "C" int aix_graph_resolve_mark_dev(uint64_t U, const uint64_t* d_offsets, const uint8_t* d_circular, const uint64_t* d_link_off, const uint32_t* d_link_to,
                                          uint64_t E, const uint64_t* d_link_support, const uint64_t* d_pair_support, uint64_t min_link_support,
                                          uint64_t min_pair_support, uint64_t max_pair_noise, uint8_t* d_link_remove, uint8_t* d_copies,
                                          uint64_t* n_links_removed_out, uint64_t* n_split_out, uint64_t* n_copies_added_out, void* stream) {
    const int st = gr_check_sizes(U, d_offsets, d_circular, d_link_off, d_link_to, E);
    if (st) return st;
    if (!n_links_removed_out || !n_split_out || !n_copies_added_out || (U && !d_copies) || (E && !d_link_remove)) return AIX_ERR_ARG;
    const bool weak_on = d_link_support && min_link_support, split_on = d_pair_support && min_pair_support;
    if (split_on && max_pair_noise >= min_pair_support) return AIX_ERR_ARG;
    uint64_t out[3] = {0, 0, 0};
    if (U) {
        hipStream_t s = (hipStream_t)stream;
        const uint64_t cap = chain_test_grid();
        const GrGraph g{U, E, d_offsets, d_circular, d_link_off, d_link_to};
        Counted<GrCounters> ctr(s);
        AIXCHK(ctr.init());
        const GrCounters& hc = ctr.host;
        bool bad = false;
        AIXCHK(gr_validate(g, d_link_support, nullptr, ctr, &bad, s));
        if (bad) return AIX_ERR_ARG;
        AIXCHK(ctr.run([&]() {
            if (weak_on) AIX_TRY_LAUNCH(k_gr_weak, dim3(chain_grid(2 * U, 2 * kCB, cap)), dim3(kCB), 0, s, g, d_link_support, min_link_support, d_link_remove, ctr.dev());
            else if (E) AIX_TRY(hipMemsetAsync(d_link_remove, 0, E, s));
            AIX_TRY_LAUNCH(k_gr_split, dim3(chain_grid(U, 2 * kCB, cap)), dim3(kCB), 0, s, g, (const uint8_t*)d_link_remove, split_on ? d_pair_support : nullptr,
                           min_pair_support, max_pair_noise, d_copies, ctr.dev());
            return hipSuccess;
        }));
        out[0] = hc.removed; out[1] = hc.n_split; out[2] = hc.added;
    }
    *n_links_removed_out = out[0]; *n_split_out = out[1]; *n_copies_added_out = out[2];
    return AIX_OK;
}

extern "C" int aix_graph_resolve_layout_dev(uint64_t U, const uint64_t* d_offsets, uint64_t E, const uint8_t* d_link_remove, const uint8_t* d_copies,
                                            uint32_t* d_copy_base, uint64_t* n_unitigs_out, uint64_t* total_bases_out, uint64_t* n_links_out, void* stream) {
    if (U > kUnitLimit) return AIX_ERR_UNSUPPORTED;
    if (!d_offsets || !n_unitigs_out || !total_bases_out || !n_links_out || E > 8 * U) return AIX_ERR_ARG;
    if ((U && (!d_copies || !d_copy_base)) || (E && !d_link_remove)) return AIX_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (U == 0) {
        *n_unitigs_out = 0; *total_bases_out = 0; *n_links_out = 0;
        return AIX_OK;
    }
    const GrGraph g{U, E, d_offsets, nullptr, nullptr, nullptr};
    Counted<GrCounters> ctr(s);
    DevArr extra(s), pre(s), tmp(s);
    AIXCHK(ctr.init());
    const GrCounters& hc = ctr.host;
    uint64_t total_in = 0;
    AIXCHK(hipMemcpyAsync(&total_in, d_offsets + U, 8, hipMemcpyDeviceToHost, s));
    AIXCHK(gr_count(g, d_copies, d_link_remove, ctr, extra, pre, tmp, s));
    if (hc.bad || hc.removed > E) return AIX_ERR_ARG;
    if (U + hc.added > kUnitLimit) return AIX_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_gr_copybase, dim3(chain_grid(U, 4 * kCB, chain_test_grid())), dim3(kCB), 0, s, U, d_copies, (const uint64_t*)pre.p, d_copy_base);
    AIXCHK(hipGetLastError());
    AIXCHK(hipStreamSynchronize(s));
    *n_unitigs_out = U + hc.added;
    *total_bases_out = total_in + hc.extra_bases;
    *n_links_out = E - hc.removed;
    return AIX_OK;
}

extern "C" int aix_graph_resolve_emit_dev(uint64_t U, const uint64_t* d_offsets, const uint8_t* d_bases, const uint8_t* d_circular, const uint64_t* d_tf_sum,
                                          const uint32_t* d_tf_min, const uint32_t* d_tf_max, const uint64_t* d_link_off, const uint32_t* d_link_to, uint64_t E,
                                          const uint8_t* d_link_remove, const uint8_t* d_copies, const uint32_t* d_copy_base, const uint64_t* d_pair_support,
                                          uint64_t min_pair_support, uint64_t n_unitigs, uint64_t total_bases, uint64_t n_links, uint64_t* d_out_offsets,
                                          uint8_t* d_out_bases, uint8_t* d_out_circular, uint64_t* d_out_tf_sum, uint32_t* d_out_tf_min, uint32_t* d_out_tf_max,
                                          uint64_t* d_out_link_off, uint32_t* d_out_link_to, uint32_t* d_unitig_origin, void* stream) {
    const int st = gr_check_sizes(U, d_offsets, d_circular, d_link_off, d_link_to, E);
    if (st) return st;
    const uint64_t U2 = n_unitigs, E2 = n_links;
    if (U2 > kUnitLimit) return AIX_ERR_UNSUPPORTED;
    if (!d_out_offsets || !d_out_link_off || U2 < U || U2 > 4 * U || E2 > E) return AIX_ERR_ARG;
    if (U && (!d_bases || !d_tf_sum || !d_tf_min || !d_tf_max || !d_copies || !d_copy_base || !d_out_bases || !d_out_circular || !d_out_tf_sum || !d_out_tf_min ||
              !d_out_tf_max || !d_unitig_origin))
        return AIX_ERR_ARG;
    if (E && !d_link_remove) return AIX_ERR_ARG;
    if (E2 && !d_out_link_to) return AIX_ERR_ARG;
    if ((uintptr_t)d_out_bases & 7u) return AIX_ERR_ARG;          // what the compaction asks of its input
    hipStream_t s = (hipStream_t)stream;
    if (U == 0) {
        if (total_bases) return AIX_ERR_ARG;
        AIXCHK(hipMemsetAsync(d_out_offsets, 0, 8, s));
        AIXCHK(hipMemsetAsync(d_out_link_off, 0, 8, s));
        AIXCHK(hipStreamSynchronize(s));
        return AIX_OK;
    }
    const uint64_t cap = chain_test_grid();
    const dim3 blk(kCB);
    const GrGraph g{U, E, d_offsets, d_circular, d_link_off, d_link_to};
    Counted<GrCounters> ctr(s);
    DevArr extra(s), pre(s), tmp(s), tmp2(s), rank(s), len(s), ndeg(s);
    AIXCHK(ctr.init());
    const GrCounters& hc = ctr.host;
    bool bad = false;
    AIXCHK(gr_validate(g, nullptr, d_link_remove, ctr, &bad, s));
    if (bad) return AIX_ERR_ARG;
    uint64_t total_in = 0;
    AIXCHK(hipMemcpyAsync(&total_in, d_offsets + U, 8, hipMemcpyDeviceToHost, s));
    AIXCHK(gr_count(g, d_copies, d_link_remove, ctr, extra, pre, tmp, s));
    if (hc.bad || U + hc.added != U2 || total_in + hc.extra_bases != total_bases || hc.removed > E || E - hc.removed != E2) return AIX_ERR_ARG;
    AIXCHK(ctr.run([&]() {
        AIX_TRY_LAUNCH(k_gr_checksplit, dim3(chain_grid(U, 2 * kCB, cap)), blk, 0, s, g, d_link_remove, d_copies, (const uint64_t*)pre.p, d_copy_base, d_pair_support,
                       min_pair_support, ctr.dev());
        return hipSuccess;
    }));
    if (hc.bad) return AIX_ERR_ARG;
    // everything is validated: from here on the outputs are written
    AIXCHK(rank.alloc(U2));
    AIXCHK(len.alloc(8 * (U2 + 1)));
    AIXCHK(ndeg.alloc(4 * (2 * U2 + 1)));
    hipLaunchKernelGGL(k_gr_origin, dim3(chain_grid(U, 4 * kCB, cap)), blk, 0, s, U, d_copies, d_copy_base, U2, d_unitig_origin, (uint8_t*)rank.p);
    AIXCHK(hipGetLastError());
    hipLaunchKernelGGL(k_gr_sizes, dim3(chain_grid(U2 + 1, 4 * kCB, cap)), blk, 0, s, g, d_link_remove, d_copies, U2, (const uint32_t*)d_unitig_origin, (uint64_t*)len.p,
                       (uint32_t*)ndeg.p);
    AIXCHK(hipGetLastError());
    AIXCHK(scan_u64((const uint64_t*)len.p, d_out_offsets, U2 + 1, tmp, s));
    AIXCHK(scan_u64(rocprim::make_transform_iterator((const uint32_t*)ndeg.p, Widen<uint32_t>()), d_out_link_off, 2 * U2 + 1, tmp2, s));
    hipLaunchKernelGGL(k_gr_values, dim3(chain_grid(U2, 2 * kCB, cap)), blk, 0, s, g, d_tf_sum, d_tf_min, d_tf_max, d_link_remove, d_copies, d_pair_support,
                       min_pair_support, U2, (const uint32_t*)d_unitig_origin, (const uint8_t*)rank.p, d_out_circular, d_out_tf_sum, d_out_tf_min, d_out_tf_max);
    AIXCHK(hipGetLastError());
    if (E2) {
        hipLaunchKernelGGL(k_gr_links, dim3(chain_grid(2 * U2, 2 * kCB, cap)), blk, 0, s, g, d_link_remove, d_copies, d_copy_base, d_pair_support, min_pair_support, U2,
                           (const uint32_t*)d_unitig_origin, (const uint8_t*)rank.p, (const uint64_t*)d_out_link_off, E2, d_out_link_to);
        AIXCHK(hipGetLastError());
    }
    AIXCHK(hipMemcpyAsync(d_out_bases, d_bases, total_in, hipMemcpyDeviceToDevice, s));
    if (total_bases > total_in) {
        hipLaunchKernelGGL(k_gr_bases, dim3(chain_grid(total_bases - total_in, 4 * kCB, cap)), blk, 0, s, U, U2, d_offsets, d_bases, (const uint32_t*)d_unitig_origin,
                           (const uint64_t*)d_out_offsets, total_in, total_bases, d_out_bases);
        AIXCHK(hipGetLastError());
    }
    AIXCHK(hipStreamSynchronize(s));
    return AIX_OK;
}

// Mark, layout, emit for host memory, on the null stream of the current device; every output is malloc'd (aix_free).
extern "C" int aix_graph_resolve(uint64_t U, const uint64_t* offsets, const uint8_t* bases, const uint8_t* circular, const uint64_t* tf_sum, const uint32_t* tf_min,
                                 const uint32_t* tf_max, const uint64_t* link_off, const uint32_t* link_to, uint64_t E, const uint64_t* link_support,
                                 const uint64_t* pair_support, uint64_t min_link_support, uint64_t min_pair_support, uint64_t max_pair_noise,
                                 uint64_t* n_unitigs_out, uint64_t* n_links_out, uint64_t* n_links_removed_out, uint64_t* n_split_out, uint64_t** offsets_out,
                                 uint8_t** bases_out, uint8_t** circular_out, uint64_t** tf_sum_out, uint32_t** tf_min_out, uint32_t** tf_max_out,
                                 uint64_t** link_off_out, uint32_t** link_to_out, uint8_t** link_remove_out, uint8_t** copies_out, uint32_t** unitig_origin_out) {
    const int st = gr_check_sizes(U, offsets, circular, link_off, link_to, E);
    if (st) return st;
    if (!n_unitigs_out || !n_links_out || !n_links_removed_out || !n_split_out || !offsets_out || !bases_out || !circular_out || !tf_sum_out || !tf_min_out ||
        !tf_max_out || !link_off_out || !link_to_out)
        return AIX_ERR_ARG;
    if (U && (!bases || !tf_sum || !tf_min || !tf_max)) return AIX_ERR_ARG;
    // offsets are read on the host for the size of `bases` only; everything else about them is the device's to check
    const uint64_t total_in = offsets[U];
    if (U && (total_in < 23 * U || total_in > (1ULL << 48))) return AIX_ERR_ARG;
    DevArr in[10], rm, cp, cb, oo, ob, oc, os, on, ox, ol, ot, og;
    const HostIn ins[10] = {{offsets, 8 * (U + 1)}, {bases, total_in}, {circular, U}, {tf_sum, 8 * U}, {tf_min, 4 * U}, {tf_max, 4 * U}, {link_off, 8 * (2 * U + 1)},
                            {link_to, 4 * E}, {link_support, 8 * E}, {pair_support, 8 * 16 * U}};
    AIXCHK(copy_in_host(in, ins, 10, true));                       // a null array (U == 0, E == 0, no support given) stays a null block
    AIXCHK(rm.alloc(E));
    AIXCHK(cp.alloc(U));
    AIXCHK(cb.alloc(4 * U));
    const uint64_t* d_sup = link_support ? (const uint64_t*)in[8].p : nullptr;
    const uint64_t* d_pair = pair_support ? (const uint64_t*)in[9].p : nullptr;
    uint64_t removed = 0, n_split = 0, added = 0, U2 = 0, total = 0, E2 = 0;
    int r = aix_graph_resolve_mark_dev(U, (const uint64_t*)in[0].p, (const uint8_t*)in[2].p, (const uint64_t*)in[6].p, (const uint32_t*)in[7].p, E, d_sup, d_pair,
                                       min_link_support, min_pair_support, max_pair_noise, (uint8_t*)rm.p, (uint8_t*)cp.p, &removed, &n_split, &added, nullptr);
    if (r) return r;
    r = aix_graph_resolve_layout_dev(U, (const uint64_t*)in[0].p, E, (const uint8_t*)rm.p, (const uint8_t*)cp.p, (uint32_t*)cb.p, &U2, &total, &E2, nullptr);
    if (r) return r;
    AIXCHK(oo.alloc(8 * (U2 + 1)));
    AIXCHK(ob.alloc(total));
    AIXCHK(oc.alloc(U2));
    AIXCHK(os.alloc(8 * U2));
    AIXCHK(on.alloc(4 * U2));
    AIXCHK(ox.alloc(4 * U2));
    AIXCHK(ol.alloc(8 * (2 * U2 + 1)));
    AIXCHK(ot.alloc(4 * E2));
    AIXCHK(og.alloc(4 * U2));
    r = aix_graph_resolve_emit_dev(U, (const uint64_t*)in[0].p, (const uint8_t*)in[1].p, (const uint8_t*)in[2].p, (const uint64_t*)in[3].p, (const uint32_t*)in[4].p,
                                   (const uint32_t*)in[5].p, (const uint64_t*)in[6].p, (const uint32_t*)in[7].p, E, (const uint8_t*)rm.p, (const uint8_t*)cp.p,
                                   (const uint32_t*)cb.p, d_pair, min_pair_support, U2, total, E2, (uint64_t*)oo.p, (uint8_t*)ob.p, (uint8_t*)oc.p, (uint64_t*)os.p,
                                   (uint32_t*)on.p, (uint32_t*)ox.p, (uint64_t*)ol.p, (uint32_t*)ot.p, (uint32_t*)og.p, nullptr);
    if (r) return r;
    const HostOut outs[] = {{(void**)offsets_out, oo.p, 8 * (U2 + 1)}, {(void**)bases_out, ob.p, total},          {(void**)circular_out, oc.p, U2},
                            {(void**)tf_sum_out, os.p, 8 * U2},        {(void**)tf_min_out, on.p, 4 * U2},        {(void**)tf_max_out, ox.p, 4 * U2},
                            {(void**)link_off_out, ol.p, 8 * (2 * U2 + 1)}, {(void**)link_to_out, ot.p, 4 * E2}, {(void**)link_remove_out, rm.p, E},
                            {(void**)copies_out, cp.p, U},             {(void**)unitig_origin_out, og.p, 4 * U2}};
    AIXCHK(copy_out_host(outs, 11));
    *n_unitigs_out = U2; *n_links_out = E2; *n_links_removed_out = removed; *n_split_out = n_split;
    return AIX_OK;
}
