// aix_gapclose.hip — the gaps of the scaffolds closed through the contig graph, on arrays resident in HBM: per join one bounded search
// for the paths from its exit end to its entry word whose length agrees with the estimated gap, and, where exactly one exists, the
// scaffolds written with the bases of that path in place of the 'N' run. The contract is stated above the aix_gap_close_dev /
// aix_scaffold_fill_* declarations in include/aindex_hip.h; DESIGN 5o has the derivations and the resources. No index handle: the
// arrays and the current device, like the scaffolding. Every call validates with counting kernels that write nothing but their counters
// and scratch, and writes its outputs only after the host has read them as clean; integer only, no grid-wide barrier, no spin-wait, no
// host loop per join:
//   search   k_gp_validate (one lane per end and link; marks the owner ends), a scan and k_gp_list (the join list), k_gp_search (one wave
//            per join at a time, the states of the join in LDS, 64 stored states expanded per round, children counted before any is
//            stored), a scan of the path lengths into path_off, k_gp_gather
//   layout   k_gp_validate, k_gf_members and k_gf_ends (one lane per member / end; a path is walked by the lane of its owner), k_gf_count,
//            two scans (filled members and bytes per member group), k_gf_write
//   emit     k_gf_em_validate (one lane per filled member), k_graph_em_bases<true> (one lane per output byte, a bisection over the first bytes)
// What the graph files share (the counters holder, the predicates of the validate kernels, the unit length, the link search, the
// bisection, the written gap, that emit kernel) is in aix_graph.hpp.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "aix_graph.hpp"

namespace aix {

// (kNoEnd is the join of an unjoined end; the constants, the counters holder, the predicates of the validation, the helpers and k_graph_em_bases: aix_graph.hpp)
static constexpr long long kPMaxGap = 1ll << 30;
static constexpr uint32_t kPMaxTol = 1u << 20, kPMaxFill = 64, kPMaxStates = 4096;
static constexpr int kPW = 64;                                    // the search: one wave per workgroup
static constexpr uint32_t kPRoot = 0xFFFFu, kPHit = 1u << 31;     // packed state: parent (16 bits) | k << 16 | hit

struct GpCounters {                                               // one zeroed record per call
    unsigned long long bad, n, status[4];
};

struct GpGraph {                                                  // contigs, their links and the joins, in HBM
    uint64_t U, E;
    const uint64_t* offsets;
    const uint64_t* link_off;
    const uint32_t* link_to;
    const uint32_t* join;
    const long long* join_gap;
};

// ---------------------------------------------------------------------------------------------
// 1. the search
// ---------------------------------------------------------------------------------------------
// offsets ascend by 23; link_off starts at 0, ascends, ends at E; link words below 2 U; a join names an end of another contig whose
// dual join names this end back, with an equal gap of at most 2^30 in size. own[e] (nullable) = e owns a join; n: the joins
__global__ void __launch_bounds__(kCB) k_gp_validate(const GpGraph g, uint64_t* __restrict__ own, GpCounters* __restrict__ ctr) {
    const uint64_t NE = 2 * g.U, work = (NE + 1 > g.E ? NE + 1 : g.E), stride = (uint64_t)gridDim.x * kCB;
    unsigned long long bad = 0, n = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kCB + threadIdx.x; i < work; i += stride) {
        if (i < g.E) bad += (uint64_t)g.link_to[i] >= NE;
        if (i == NE && own) own[NE] = 0;
        if (i >= NE) continue;
        const uint64_t e = i;
        if (!(e & 1)) bad += span_bad(g.offsets[e >> 1], g.offsets[(e >> 1) + 1]);
        bad += csr_bad(e, NE, g.link_off[e], g.link_off[e + 1], g.E, kAnyDegree);
        const uint64_t t = g.join[e];
        uint64_t mine = 0;
        if (t != kNoEnd) {
            if (!join_dual_ok(g.join, g.join_gap, NE, e, t)) ++bad;
            else {
                const long long gap = g.join_gap[e];
                bad += gap > kPMaxGap || gap < -kPMaxGap;
                mine = e < (t ^ 1);
            }
        }
        if (own) own[e] = mine;
        n += mine;
    }
    count_add(bad, &ctr->bad);
    count_add(n, &ctr->n);
}

__global__ void __launch_bounds__(kCB) k_gp_list(uint64_t NE, uint64_t J, const uint64_t* __restrict__ own, const uint64_t* __restrict__ at, uint32_t* __restrict__ list) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t e = (uint64_t)blockIdx.x * kCB + threadIdx.x; e < NE; e += stride)
        if (own[e] && at[e] < J) list[at[e]] = (uint32_t)e;
}

struct GpRule {                                                   // the join under search and the parameters
    uint64_t t;
    long long gap, lim;                                           // lim = gap + tolerance
    long long tol;
    uint32_t max_fill;
};

// candidate (y, d, k): 0 = dropped, 1 = an intermediate, 2 = a hit (behind k_gp_validate: y < 2 U)
__device__ __forceinline__ int gp_keep(const GpGraph& g, const GpRule& r, uint64_t y, long long d, uint32_t k) {
    if (y == r.t) {
        const long long x = d - r.gap;
        return (x <= r.tol && x >= -r.tol) ? 2 : 0;
    }
    if (k >= r.max_fill || g.join[y & ~1ull] != kNoEnd || g.join[y | 1ull] != kNoEnd) return 0;
    const long long room = r.lim + 22 - d;                        // d + L_y - 22 <= lim, L_y taken as unsigned
    return (room > 0 && unit_len(g.offsets, y) <= (uint64_t)room) ? 1 : 0;
}

// One wave per workgroup, a join at a time. LDS: word, d and packed (parent, k, hit) of the stored states, max_states of each. A round
// takes the next 64 stored states (the first round: the exit end itself), counts the candidates that would be stored, and stores them
// only if the budget holds them all; so the set of stored states, and with it every output, is that of the rule whatever the order.
__global__ void __launch_bounds__(kPW) k_gp_search(const GpGraph g, uint64_t J, const uint32_t* __restrict__ list, long long tol, uint32_t max_fill, uint32_t max_states,
                                                  uint8_t* __restrict__ status, long long* __restrict__ dist, uint32_t* __restrict__ states, uint64_t* __restrict__ path_len,
                                                  uint32_t* __restrict__ slot, uint32_t* __restrict__ fill_uses, GpCounters* __restrict__ ctr) {
    extern __shared__ uint32_t gp_lds[];
    uint32_t* sw = gp_lds;
    int32_t* sd = (int32_t*)(gp_lds + max_states);
    uint32_t* sp = gp_lds + 2 * (size_t)max_states;
    const uint32_t lane = threadIdx.x;
    unsigned long long by_status[4] = {0, 0, 0, 0};
    for (uint64_t j = blockIdx.x; j < J; j += gridDim.x) {
        const uint64_t e = list[j];
        GpRule r;
        r.t = g.join[e];
        r.gap = g.join_gap[e];
        r.tol = tol;
        r.lim = r.gap + tol;
        r.max_fill = max_fill;
        uint32_t n = 0, head = 0, hits = 0, hit_at = 0;
        bool over = false, first = true;
        while (true) {
            bool have = false;
            uint64_t src = 0;
            long long cd = 0;
            uint32_t ck = 0, par = kPRoot, end = head;
            if (first) {
                have = lane == 0;
                src = e;
                cd = -22;
            } else {
                end = n - head > (uint32_t)kPW ? head + kPW : n;
                const uint32_t i = head + lane;
                if (i < end) {
                    const uint32_t p = sp[i];
                    if (!(p & kPHit)) {
                        have = true;
                        src = sw[i];
                        cd = (long long)sd[i] + (long long)unit_len(g.offsets, src) - 22;  // <= lim: the state was stored
                        ck = ((p >> 16) & 0x7Fu) + 1;
                        par = i;
                    }
                }
            }
            const uint64_t lo = have ? g.link_off[src] : 0, hi = have ? g.link_off[src + 1] : 0;
            uint32_t mine = 0;
            for (uint64_t q = lo; q < hi; ++q) mine += gp_keep(g, r, g.link_to[q], cd, ck) != 0;
            uint32_t incl = mine;
#pragma unroll
            for (int s = 1; s < kPW; s <<= 1) {
                const uint32_t o = __shfl_up(incl, s);
                if (lane >= (uint32_t)s) incl += o;
            }
            const uint32_t total = __shfl(incl, kPW - 1);
            if (total > max_states - n) { over = true; break; }  // counted before any is stored: nothing beyond the budget is written
            uint32_t at = n + incl - mine, my_hits = 0, my_hit_at = 0;
            for (uint64_t q = lo; q < hi; ++q) {
                const uint64_t y = g.link_to[q];
                const int c = gp_keep(g, r, y, cd, ck);
                if (!c || at >= max_states) continue;             // (at < n + total <= max_states)
                sw[at] = (uint32_t)y;
                sd[at] = (int32_t)cd;
                sp[at] = par | ck << 16 | (c == 2 ? kPHit : 0u);
                if (c == 2) { ++my_hits; my_hit_at = at; }
                ++at;
            }
            hits += (uint32_t)wave_sum(my_hits);
            const uint32_t h = (uint32_t)wave_max(my_hit_at);
            if (h > hit_at) hit_at = h;
            n += total;
            __syncthreads();
            if (!first) head = end;
            first = false;
            if (head >= n) break;
        }
        const uint32_t st = over ? 4u : hits == 0 ? 2u : hits > 1 ? 3u : 1u;
        if (lane == 0) {
            long long d = 0;
            uint64_t len = 0;
            if (st == 1) {
                const uint32_t p = sp[hit_at];
                d = sd[hit_at];
                len = (p >> 16) & 0x7Fu;
                uint32_t i = p & 0xFFFFu;
                for (uint64_t x = len; x-- > 0 && i < n && x < max_fill;) {
                    const uint32_t w = sw[i];
                    slot[j * max_fill + x] = w;
                    atomicAdd(fill_uses + (w >> 1), 1u);
                    i = sp[i] & 0xFFFFu;
                }
            }
            const uint64_t e2 = r.t ^ 1;
            status[e] = (uint8_t)st; status[e2] = (uint8_t)st;
            dist[e] = d; dist[e2] = d;
            states[e] = over ? max_states : n; states[e2] = states[e];
            path_len[e] = len;
            ++by_status[st - 1];
        }
        __syncthreads();                                          // the next join takes the LDS over
    }
    if (lane == 0)
        for (int k = 0; k < 4; ++k)
            if (by_status[k]) atomicAdd(&ctr->status[k], by_status[k]);
}

__global__ void __launch_bounds__(kCB) k_gp_gather(uint64_t J, uint32_t max_fill, const uint32_t* __restrict__ list, const uint32_t* __restrict__ slot,
                                                  const uint64_t* __restrict__ path_off, uint64_t cap, uint32_t* __restrict__ path) {
    const uint64_t work = J * max_fill, stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t i = (uint64_t)blockIdx.x * kCB + threadIdx.x; i < work; i += stride) {
        const uint64_t e = list[i / max_fill], x = i % max_fill, a = path_off[e], b = path_off[e + 1];
        if (x < b - a && a + x < cap) path[a + x] = slot[i];
    }
}

// ---------------------------------------------------------------------------------------------
// 2. filled member lists
// ---------------------------------------------------------------------------------------------
struct GfIn {                                                     // the member CSR and the closure
    uint64_t Sc, ptotal;
    const uint64_t* member_off;
    const uint32_t* member;
    const uint8_t* status;
    const long long* dist;
    const uint64_t* path_off;
    const uint32_t* path;
    uint32_t min_gap;
};

// member_off starts at 0, ascends strictly and ends at U; a member word is below 2 U and follows its predecessor through `join`;
// seen[u] = the members that name contig u. (The scaffold of member i is last_le(member_off, 0, Sc, i): member_off[0] == 0.)
__global__ void __launch_bounds__(kCB) k_gf_members(const GpGraph g, const GfIn f, uint32_t* __restrict__ seen, GpCounters* __restrict__ ctr) {
    const uint64_t NE = 2 * g.U, work = (g.U > f.Sc + 1 ? g.U : f.Sc + 1), stride = (uint64_t)gridDim.x * kCB;
    unsigned long long bad = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kCB + threadIdx.x; i < work; i += stride) {
        if (i <= f.Sc) {
            const uint64_t a = f.member_off[i];
            bad += i == 0 && a != 0;
            bad += i == f.Sc && a != g.U;
            if (i < f.Sc) { const uint64_t b = f.member_off[i + 1]; bad += b <= a || b > g.U; }
        }
        if (i < g.U) {
            const uint64_t w = f.member[i];
            if (w >= NE) { ++bad; continue; }
            atomicAdd(seen + (w >> 1), 1u);
            if (i == 0 || f.member_off[last_le(f.member_off, 0, f.Sc, i)] == i) continue;
            const uint64_t p = f.member[i - 1];
            bad += p >= NE || (uint64_t)g.join[p < NE ? p : 0] != w;
        }
    }
    count_add(bad, &ctr->bad);
}

__device__ __forceinline__ bool gf_linked(const GpGraph& g, uint64_t a, uint64_t b) { return link_find(g.link_to, g.link_off[a], g.link_off[a + 1], b) != kNoLink; }

// every contig is named once; statuses are 0 .. 4, 0 on an unjoined end, equal at both ends of a join; path_off starts at 0, ascends and
// ends at the total; only the owner of a closed join has a path; every step of it is a link, every intermediate unjoined, and
// close_dist is its length at both ends (behind k_gp_validate: join is symmetric and the link lists are in range)
__global__ void __launch_bounds__(kCB) k_gf_ends(const GpGraph g, const GfIn f, const uint32_t* __restrict__ seen, GpCounters* __restrict__ ctr) {
    const uint64_t NE = 2 * g.U, stride = (uint64_t)gridDim.x * kCB;
    unsigned long long bad = 0;
    for (uint64_t e = (uint64_t)blockIdx.x * kCB + threadIdx.x; e < NE; e += stride) {
        if (!(e & 1)) bad += seen[e >> 1] != 1;
        const uint64_t a = f.path_off[e], b = f.path_off[e + 1];
        bad += csr_bad(e, NE, a, b, f.ptotal, kAnyDegree);
        if (!csr_in_range(a, b, f.ptotal, kAnyDegree)) continue;
        const uint32_t st = f.status[e];
        const uint64_t t = g.join[e];
        bad += st > 4;
        if (t == kNoEnd) { bad += st != 0 || b != a; continue; }
        bad += f.status[t ^ 1] != st;
        if (st != 1 || e > (t ^ 1)) { bad += b != a; continue; }
        uint64_t at = e, d = (uint64_t)-22ll;
        bool ok = true;
        for (uint64_t q = a; q < b && ok; ++q) {
            const uint64_t w = f.path[q];
            ok = w < NE && gf_linked(g, at, w) && g.join[w & ~1ull] == kNoEnd && g.join[w | 1ull] == kNoEnd;
            if (ok) { d += unit_len(g.offsets, w) - 22; at = w; }
        }
        ok = ok && gf_linked(g, at, t);
        bad += !ok || (uint64_t)f.dist[e] != d || (uint64_t)f.dist[t ^ 1] != d;
    }
    count_add(bad, &ctr->bad);
}

// per member i (behind the validation): cnt[i] = the filled members it brings (its path and itself), len[i] = the bytes they write,
// the 'N' run of an unclosed join included: a closed join writes close_dist + L bytes, as close_dist = sum (L_p - 22) - 22
__global__ void __launch_bounds__(kCB) k_gf_count(const GpGraph g, const GfIn f, uint64_t* __restrict__ cnt, uint64_t* __restrict__ len) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t i = (uint64_t)blockIdx.x * kCB + threadIdx.x; i <= g.U; i += stride) {
        if (i == g.U) { cnt[i] = 0; len[i] = 0; continue; }
        const uint64_t w = f.member[i];
        uint64_t c = 1, n = unit_len(g.offsets, w);
        if (i && f.member_off[last_le(f.member_off, 0, f.Sc, i)] != i) {
            const uint64_t e = f.member[i - 1];
            if (f.status[e] == 1) {
                const uint64_t o = e < (w ^ 1) ? e : (w ^ 1);
                c += f.path_off[o + 1] - f.path_off[o];
                n += (uint64_t)f.dist[e];
            } else n += written_gap(g.join_gap[e], f.min_gap);
        }
        cnt[i] = c;
        len[i] = n;
    }
}

struct GfOut {
    uint64_t* fmember_off;
    uint32_t* fmember;
    uint8_t* flag;
    long long* gap;
    uint64_t* pos;
    uint64_t* fscaffold_offsets;
    uint64_t cap;                                                 // U + the path total: what the caller allocated
};

// fo / gs: the exclusive scans of cnt / len
__global__ void __launch_bounds__(kCB) k_gf_write(const GpGraph g, const GfIn f, const uint64_t* __restrict__ fo, const uint64_t* __restrict__ gs, const GfOut o) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t i = (uint64_t)blockIdx.x * kCB + threadIdx.x; i <= g.U; i += stride) {
        if (i == g.U) { o.fmember_off[f.Sc] = fo[i]; o.fscaffold_offsets[f.Sc] = gs[i]; continue; }
        const uint64_t s = last_le(f.member_off, 0, f.Sc, i), i0 = f.member_off[s], base = gs[i0], w = f.member[i];
        uint64_t j = fo[i], x = gs[i] - base;
        uint8_t flag = 0;
        long long gap = 0;
        if (i == i0) {
            o.fmember_off[s] = j;
            o.fscaffold_offsets[s] = base;
        } else {
            const uint64_t e = f.member[i - 1];
            if (f.status[e] == 1) {
                const bool own = e < (w ^ 1);
                const uint64_t ow = own ? e : (w ^ 1), a = f.path_off[ow], n = f.path_off[ow + 1] - a;
                for (uint64_t q = 0; q < n && j < o.cap; ++q, ++j) {
                    const uint64_t p = own ? f.path[a + q] : (f.path[a + n - 1 - q] ^ 1u);
                    o.fmember[j] = (uint32_t)p;
                    o.flag[j] = 3;
                    o.gap[j] = 0;
                    o.pos[j] = x;
                    x += unit_len(g.offsets, p) - 22;
                }
                flag = 1;
                gap = f.dist[e];
            } else {
                gap = g.join_gap[e];
                x += written_gap(gap, f.min_gap);
            }
        }
        if (j >= o.cap) continue;                                 // (never: cap >= U + the path total)
        o.fmember[j] = (uint32_t)w;
        o.flag[j] = flag;
        o.gap[j] = gap;
        o.pos[j] = x;
    }
}

// ---------------------------------------------------------------------------------------------
// 3. filled scaffolds
// ---------------------------------------------------------------------------------------------
struct GfMap {
    uint64_t U, Sc, Mf, total;
    const uint64_t* offsets;
    const uint64_t* fmember_off;
    const uint32_t* fmember;
    const uint8_t* flag;
    const long long* gap;
    const uint64_t* pos;
    const uint64_t* fso;
    uint32_t min_gap;
};

// offsets ascend by 23; fmember_off starts at 0, ascends strictly, ends at Mf; words below 2 U; flags 0, 1 or 3, 0 and position 0 on a
// first member; a member starts where its predecessor's bytes and its own 'N' run end; a scaffold is as long as its last member ends;
// fscaffold_offsets starts at 0 and ends at the total. mstart[j] = the first byte member j writes, over all scaffolds
__global__ void __launch_bounds__(kCB) k_gf_em_validate(const GfMap m, uint64_t* __restrict__ mstart, GpCounters* __restrict__ ctr) {
    const uint64_t NE = 2 * m.U, ms = m.Mf > m.Sc + 1 ? m.Mf : m.Sc + 1, work = ms > m.U ? ms : m.U, stride = (uint64_t)gridDim.x * kCB;
    unsigned long long bad = 0;
    for (uint64_t j = (uint64_t)blockIdx.x * kCB + threadIdx.x; j < work; j += stride) {
        if (j < m.U) bad += span_bad(m.offsets[j], m.offsets[j + 1]);
        if (j <= m.Sc) {
            const uint64_t a = m.fmember_off[j], x = m.fso[j];
            bad += j == 0 && (a != 0 || x != 0);
            bad += j == m.Sc && (a != m.Mf || x != m.total);
            if (j < m.Sc) { const uint64_t b = m.fmember_off[j + 1]; bad += b <= a || b > m.Mf || m.fso[j + 1] < x; }
        }
        if (j >= m.Mf) continue;
        const uint64_t w = m.fmember[j], fl = m.flag[j];
        if (w >= NE || !(fl == 0 || fl == 1 || fl == 3)) { ++bad; continue; }
        const uint64_t s = last_le(m.fmember_off, 0, m.Sc, j), j0 = m.fmember_off[s], j1 = m.fmember_off[s + 1], x = m.pos[j];
        const uint64_t L = unit_len(m.offsets, w);
        if (j == j0) bad += fl != 0 || x != 0;
        else {
            const uint64_t pw = m.fmember[j - 1], pf = m.flag[j - 1];
            if (pw >= NE) { ++bad; continue; }
            const uint64_t pl = unit_len(m.offsets, pw);
            bad += x != m.pos[j - 1] + pl - 22 * (pf & 1) + (fl == 0 ? written_gap(m.gap[j], m.min_gap) : 0);
        }
        if (j + 1 == j1) bad += m.fso[s + 1] - m.fso[s] != x + L - 22 * (fl & 1);
        mstart[j] = m.fso[s] + x;
    }
    count_add(bad, &ctr->bad);
}

// (the bases of the filled scaffolds: k_graph_em_bases<true>, aix_graph.hpp)

// the refusals the calls share, decided before anything is allocated or launched
static int gp_check_graph(uint64_t U, const void* offsets, const void* link_off, const void* link_to, uint64_t E, const void* join, const void* join_gap) {
    if (U > kUnitLimit) return AIX_ERR_UNSUPPORTED;
    if (!offsets || !link_off || E >= (1ull << 60) || (E && (!link_to || !U)) || (U && (!join || !join_gap))) return AIX_ERR_ARG;
    return AIX_OK;
}

}  // namespace aix

using namespace aix;

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" int aix_gap_close_dev(uint64_t U, const uint64_t* d_offsets, const uint64_t* d_link_off, const uint32_t* d_link_to, uint64_t E, const uint32_t* d_join,
                                 const int64_t* d_join_gap, uint32_t tolerance, uint32_t max_fill, uint32_t max_states, uint8_t* d_close_status, int64_t* d_close_dist,
                                 uint32_t* d_close_states, uint64_t* d_path_off, uint32_t* d_path, uint64_t cap, uint64_t* total_out, uint32_t* d_fill_uses,
                                 uint64_t* d_counts, void* stream) {
    const int st = gp_check_graph(U, d_offsets, d_link_off, d_link_to, E, d_join, d_join_gap);
    if (st) return st;
    if (!d_path_off || !total_out || !d_counts || tolerance > kPMaxTol || max_fill > kPMaxFill || max_states < 1 || max_states > kPMaxStates) return AIX_ERR_ARG;
    if (U && (!d_close_status || !d_close_dist || !d_close_states || !d_fill_uses)) return AIX_ERR_ARG;
    if (cap && !d_path) return AIX_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (U == 0) {
        AIXCHK(hipMemsetAsync(d_path_off, 0, 8, s));
        AIXCHK(hipMemsetAsync(d_counts, 0, 40, s));
        AIXCHK(hipStreamSynchronize(s));
        *total_out = 0;
        return AIX_OK;
    }
    const uint64_t NE = 2 * U, grid_cap = chain_test_grid();
    const dim3 blk(kCB);
    const GpGraph g{U, E, d_offsets, d_link_off, d_link_to, d_join, (const long long*)d_join_gap};
    Counted<GpCounters> ctr(s);
    DevArr own(s), at(s), list(s), slot(s), plen(s), tmp(s), tmp2(s);
    AIXCHK(ctr.init());
    AIXCHK(own.alloc(8 * (NE + 1)));
    const GpCounters& hc = ctr.host;
    AIXCHK(ctr.run([&]() {
        AIX_TRY_LAUNCH(k_gp_validate, dim3(chain_grid(std::max(NE + 1, E), 2 * kCB, grid_cap)), blk, 0, s, g, (uint64_t*)own.p, ctr.dev());
        return hipSuccess;
    }));
    if (hc.bad) return AIX_ERR_ARG;
    // everything is validated: from here on the outputs are written
    const uint64_t J = hc.n;
    uint64_t total = 0;
    unsigned long long by_status[4] = {0, 0, 0, 0};
    AIXCHK(hipMemsetAsync(d_close_status, 0, NE, s));
    AIXCHK(hipMemsetAsync(d_close_dist, 0, 8 * NE, s));
    AIXCHK(hipMemsetAsync(d_close_states, 0, 4 * NE, s));
    AIXCHK(hipMemsetAsync(d_fill_uses, 0, 4 * U, s));
    if (J == 0) {
        AIXCHK(hipMemsetAsync(d_path_off, 0, 8 * (NE + 1), s));
    } else {
        AIXCHK(at.alloc(8 * (NE + 1)));
        AIXCHK(list.alloc(4 * J));
        AIXCHK(slot.alloc(4 * J * max_fill));
        AIXCHK(plen.alloc(8 * (NE + 1)));
        AIXCHK(scan_u64((const uint64_t*)own.p, (uint64_t*)at.p, NE + 1, tmp, s));
        hipLaunchKernelGGL(k_gp_list, dim3(chain_grid(NE, 4 * kCB, grid_cap)), blk, 0, s, NE, J, (const uint64_t*)own.p, (const uint64_t*)at.p, (uint32_t*)list.p);
        AIXCHK(hipGetLastError());
        AIXCHK(hipMemsetAsync(plen.p, 0, 8 * (NE + 1), s));
        AIXCHK(ctr.run([&]() {
            AIX_TRY_LAUNCH(k_gp_search, dim3(chain_grid(J, 1, grid_cap)), dim3(kPW), 12 * (size_t)max_states, s, g, J, (const uint32_t*)list.p, (long long)tolerance,
                           max_fill, max_states, d_close_status, (long long*)d_close_dist, d_close_states, (uint64_t*)plen.p, (uint32_t*)slot.p, d_fill_uses, ctr.dev());
            return hipSuccess;
        }));
        for (int k = 0; k < 4; ++k) by_status[k] = hc.status[k];
        AIXCHK(scan_u64((const uint64_t*)plen.p, d_path_off, NE + 1, tmp2, s));
        AIXCHK(hipMemcpyAsync(&total, d_path_off + NE, 8, hipMemcpyDeviceToHost, s));
        AIXCHK(hipStreamSynchronize(s));
        if (total && total <= cap) {
            hipLaunchKernelGGL(k_gp_gather, dim3(chain_grid(J * max_fill, 4 * kCB, grid_cap)), blk, 0, s, J, max_fill, (const uint32_t*)list.p, (const uint32_t*)slot.p,
                               (const uint64_t*)d_path_off, cap, d_path);
            AIXCHK(hipGetLastError());
        }
    }
    const uint64_t counts[5] = {by_status[0], by_status[1], by_status[2], by_status[3], J};
    AIXCHK(hipMemcpyAsync(d_counts, counts, 40, hipMemcpyHostToDevice, s));
    AIXCHK(hipStreamSynchronize(s));
    *total_out = total;
    return AIX_OK;
}

// the refusals of the layout that need no device, and its validation; on AIX_OK the inputs are clean
static int gf_check(uint64_t U, uint64_t n_scaffolds, const void* member_off, const void* member, const void* status, const void* dist, const void* path_off,
                    const void* path, uint64_t path_total, uint32_t min_gap) {
    if (!member_off || !path_off || min_gap < 1 || n_scaffolds > U || (U && !n_scaffolds) || path_total >= (1ull << 60)) return AIX_ERR_ARG;
    if (U && (!member || !status || !dist)) return AIX_ERR_ARG;
    if (path_total && (!path || !U)) return AIX_ERR_ARG;
    return AIX_OK;
}

extern "C" int aix_scaffold_fill_layout_dev(uint64_t U, const uint64_t* d_offsets, const uint64_t* d_link_off, const uint32_t* d_link_to, uint64_t E,
                                            const uint32_t* d_join, const int64_t* d_join_gap, uint32_t min_gap, uint64_t n_scaffolds, const uint64_t* d_member_off,
                                            const uint32_t* d_member, const uint8_t* d_close_status, const int64_t* d_close_dist, const uint64_t* d_path_off,
                                            const uint32_t* d_path, uint64_t path_total, uint64_t* d_fmember_off, uint32_t* d_fmember, uint8_t* d_fmember_flag,
                                            int64_t* d_fmember_gap, uint64_t* d_fmember_pos, uint64_t* d_fscaffold_offsets, uint64_t* n_fmembers_out,
                                            uint64_t* total_bases_out, void* stream) {
    int st = gp_check_graph(U, d_offsets, d_link_off, d_link_to, E, d_join, d_join_gap);
    if (st) return st;
    st = gf_check(U, n_scaffolds, d_member_off, d_member, d_close_status, d_close_dist, d_path_off, d_path, path_total, min_gap);
    if (st) return st;
    if (!d_fmember_off || !d_fscaffold_offsets || !n_fmembers_out || !total_bases_out) return AIX_ERR_ARG;
    if (U && (!d_fmember || !d_fmember_flag || !d_fmember_gap || !d_fmember_pos)) return AIX_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (U == 0) {
        AIXCHK(hipMemsetAsync(d_fmember_off, 0, 8, s));
        AIXCHK(hipMemsetAsync(d_fscaffold_offsets, 0, 8, s));
        AIXCHK(hipStreamSynchronize(s));
        *n_fmembers_out = 0;
        *total_bases_out = 0;
        return AIX_OK;
    }
    const uint64_t NE = 2 * U, Sc = n_scaffolds, grid_cap = chain_test_grid();
    const dim3 blk(kCB);
    const GpGraph g{U, E, d_offsets, d_link_off, d_link_to, d_join, (const long long*)d_join_gap};
    const GfIn f{Sc, path_total, d_member_off, d_member, d_close_status, (const long long*)d_close_dist, d_path_off, d_path, min_gap};
    Counted<GpCounters> ctr(s);
    DevArr seen(s), cnt(s), len(s), fo(s), gs(s), tmp(s), tmp2(s);
    AIXCHK(ctr.init());
    const GpCounters& hc = ctr.host;
    AIXCHK(ctr.run([&]() {
        AIX_TRY_LAUNCH(k_gp_validate, dim3(chain_grid(std::max(NE + 1, E), 2 * kCB, grid_cap)), blk, 0, s, g, (uint64_t*)nullptr, ctr.dev());
        return hipSuccess;
    }));
    if (hc.bad) return AIX_ERR_ARG;
    AIXCHK(seen.alloc(4 * U));
    AIXCHK(ctr.run([&]() {
        AIX_TRY(hipMemsetAsync(seen.p, 0, 4 * U, s));
        AIX_TRY_LAUNCH(k_gf_members, dim3(chain_grid(std::max(U, Sc + 1), 2 * kCB, grid_cap)), blk, 0, s, g, f, (uint32_t*)seen.p, ctr.dev());
        AIX_TRY_LAUNCH(k_gf_ends, dim3(chain_grid(NE, kCB, grid_cap)), blk, 0, s, g, f, (const uint32_t*)seen.p, ctr.dev());
        return hipSuccess;
    }));
    if (hc.bad) return AIX_ERR_ARG;
    AIXCHK(cnt.alloc(8 * (U + 1)));
    AIXCHK(len.alloc(8 * (U + 1)));
    AIXCHK(fo.alloc(8 * (U + 1)));
    AIXCHK(gs.alloc(8 * (U + 1)));
    hipLaunchKernelGGL(k_gf_count, dim3(chain_grid(U + 1, 2 * kCB, grid_cap)), blk, 0, s, g, f, (uint64_t*)cnt.p, (uint64_t*)len.p);
    AIXCHK(hipGetLastError());
    AIXCHK(scan_u64((const uint64_t*)cnt.p, (uint64_t*)fo.p, U + 1, tmp, s));
    AIXCHK(scan_u64((const uint64_t*)len.p, (uint64_t*)gs.p, U + 1, tmp2, s));
    uint64_t Mf = 0, total = 0;
    AIXCHK(hipMemcpyAsync(&Mf, (const uint64_t*)fo.p + U, 8, hipMemcpyDeviceToHost, s));
    AIXCHK(hipMemcpyAsync(&total, (const uint64_t*)gs.p + U, 8, hipMemcpyDeviceToHost, s));
    AIXCHK(hipStreamSynchronize(s));
    if (Mf > U + path_total) { set_last_error("aix_scaffold_fill_layout_dev: more filled members than contigs and path entries"); return AIX_ERR_HIP; }
    // everything is validated: from here on the outputs are written
    const GfOut o{d_fmember_off, d_fmember, d_fmember_flag, (long long*)d_fmember_gap, d_fmember_pos, d_fscaffold_offsets, U + path_total};
    hipLaunchKernelGGL(k_gf_write, dim3(chain_grid(U + 1, 2 * kCB, grid_cap)), blk, 0, s, g, f, (const uint64_t*)fo.p, (const uint64_t*)gs.p, o);
    AIXCHK(hipGetLastError());
    AIXCHK(hipStreamSynchronize(s));
    *n_fmembers_out = Mf;
    *total_bases_out = total;
    return AIX_OK;
}

extern "C" int aix_scaffold_fill_emit_dev(uint64_t U, const uint64_t* d_offsets, const uint8_t* d_bases, uint32_t min_gap, uint64_t n_scaffolds,
                                          const uint64_t* d_fmember_off, uint64_t n_fmembers, const uint32_t* d_fmember, const uint8_t* d_fmember_flag,
                                          const int64_t* d_fmember_gap, const uint64_t* d_fmember_pos, const uint64_t* d_fscaffold_offsets, uint64_t total_bases,
                                          uint8_t* d_fscaffold_bases, void* stream) {
    if (U > kUnitLimit) return AIX_ERR_UNSUPPORTED;
    const uint64_t Sc = n_scaffolds, Mf = n_fmembers;
    if (!d_offsets || !d_fmember_off || !d_fscaffold_offsets || min_gap < 1 || Sc > U || (U && !Sc) || Mf < U || Mf >= (1ull << 60)) return AIX_ERR_ARG;
    if (U && (!d_bases || !d_fmember || !d_fmember_flag || !d_fmember_gap || !d_fmember_pos || !d_fscaffold_bases)) return AIX_ERR_ARG;
    if (U ? total_bases < 23 * Sc : (total_bases != 0 || Mf != 0)) return AIX_ERR_ARG;
    if (U == 0) return AIX_OK;
    hipStream_t s = (hipStream_t)stream;
    const uint64_t grid_cap = chain_test_grid();
    const dim3 blk(kCB);
    const GfMap m{U, Sc, Mf, total_bases, d_offsets, d_fmember_off, d_fmember, d_fmember_flag, (const long long*)d_fmember_gap, d_fmember_pos, d_fscaffold_offsets, min_gap};
    Counted<GpCounters> ctr(s);
    DevArr mstart(s);
    AIXCHK(ctr.init());
    AIXCHK(mstart.alloc(8 * Mf));
    AIXCHK(ctr.run([&]() {
        AIX_TRY_LAUNCH(k_gf_em_validate, dim3(chain_grid(std::max(std::max(Mf, Sc + 1), U), 2 * kCB, grid_cap)), blk, 0, s, m, (uint64_t*)mstart.p, ctr.dev());
        return hipSuccess;
    }));
    if (ctr.host.bad) return AIX_ERR_ARG;
    hipLaunchKernelGGL(k_graph_em_bases<true>, dim3(chain_grid(total_bases, 4 * kCB, grid_cap)), blk, 0, s, Mf, total_bases, d_offsets, d_bases, d_fmember, d_fmember_flag,
                       (const uint64_t*)mstart.p, d_fscaffold_bases);
    AIXCHK(hipGetLastError());
    AIXCHK(hipStreamSynchronize(s));
    return AIX_OK;
}

// Search, layout and emit for host memory, on the null stream of the current device; every output is malloc'd (aix_free).
extern "C" int aix_scaffold_fill(uint64_t U, const uint64_t* offsets, const uint8_t* bases, const uint64_t* link_off, const uint32_t* link_to, uint64_t E,
                                 const uint32_t* join, const int64_t* join_gap, uint64_t n_scaffolds, const uint64_t* member_off, const uint32_t* member,
                                 uint32_t tolerance, uint32_t max_fill, uint32_t max_states, uint32_t min_gap, uint64_t* n_fmembers_out, uint64_t* total_bases_out,
                                 uint64_t* path_total_out, uint64_t** fscaffold_offsets_out, uint8_t** fscaffold_bases_out, uint64_t** fmember_off_out,
                                 uint32_t** fmember_out, uint8_t** fmember_flag_out, int64_t** fmember_gap_out, uint64_t** fmember_pos_out, uint8_t** close_status_out,
                                 int64_t** close_dist_out, uint32_t** close_states_out, uint64_t** path_off_out, uint32_t** path_out, uint32_t** fill_uses_out,
                                 uint64_t** counts_out) {
    const int st = gp_check_graph(U, offsets, link_off, link_to, E, join, join_gap);
    if (st) return st;
    if (!n_fmembers_out || !total_bases_out || !path_total_out || !fscaffold_offsets_out || !fscaffold_bases_out || !fmember_off_out || !fmember_out ||
        !fmember_flag_out || !fmember_gap_out || !fmember_pos_out)
        return AIX_ERR_ARG;
    if ((U && (!bases || !member)) || !member_off || min_gap < 1 || n_scaffolds > U || (U && !n_scaffolds)) return AIX_ERR_ARG;
    if (tolerance > kPMaxTol || max_fill > kPMaxFill || max_states < 1 || max_states > kPMaxStates) return AIX_ERR_ARG;
    // offsets are read on the host for the size of `bases` only; everything else about them is the device's to check
    const uint64_t total_in = offsets[U], Sc = n_scaffolds, NE = 2 * U;
    if (U && (total_in < 23 * U || total_in > (1ULL << 48))) return AIX_ERR_ARG;
    DevArr in[8], cs, cd, cn, po, pa, fu, ct, fo, fm, ff, fg, fp, so, sb;
    const HostIn ins[8] = {{offsets, 8 * (U + 1)}, {bases, total_in}, {link_off, 8 * (NE + 1)}, {link_to, 4 * E}, {join, 4 * NE}, {join_gap, 8 * NE},
                           {member_off, 8 * (Sc + 1)}, {member, 4 * U}};
    AIXCHK(copy_in_host(in, ins, 8));
    const uint64_t* d_off = (const uint64_t*)in[0].p;
    const uint64_t* d_lo = (const uint64_t*)in[2].p;
    const uint32_t* d_lt = (const uint32_t*)in[3].p;
    const uint32_t* d_jn = (const uint32_t*)in[4].p;
    const int64_t* d_jg = (const int64_t*)in[5].p;
    AIXCHK(cs.alloc(NE));
    AIXCHK(cd.alloc(8 * NE));
    AIXCHK(cn.alloc(4 * NE));
    AIXCHK(po.alloc(8 * (NE + 1)));
    AIXCHK(fu.alloc(4 * U));
    AIXCHK(ct.alloc(40));
    uint64_t cap = U, ptotal = 0;
    for (int pass = 0; pass < 2; ++pass) {                         // the sizing protocol: a second pass only when the paths outnumber the contigs
        AIXCHK(pa.alloc(4 * cap));
        const int r = aix_gap_close_dev(U, d_off, d_lo, d_lt, E, d_jn, d_jg, tolerance, max_fill, max_states, (uint8_t*)cs.p, (int64_t*)cd.p, (uint32_t*)cn.p,
                                        (uint64_t*)po.p, cap ? (uint32_t*)pa.p : nullptr, cap, &ptotal, (uint32_t*)fu.p, (uint64_t*)ct.p, nullptr);
        if (r) return r;
        if (ptotal <= cap) break;
        cap = ptotal;
    }
    const uint64_t fcap = U + ptotal;
    uint64_t Mf = 0, total = 0;
    AIXCHK(fo.alloc(8 * (Sc + 1)));
    AIXCHK(so.alloc(8 * (Sc + 1)));
    AIXCHK(fm.alloc(4 * fcap));
    AIXCHK(ff.alloc(fcap));
    AIXCHK(fg.alloc(8 * fcap));
    AIXCHK(fp.alloc(8 * fcap));
    int r = aix_scaffold_fill_layout_dev(U, d_off, d_lo, d_lt, E, d_jn, d_jg, min_gap, Sc, (const uint64_t*)in[6].p, (const uint32_t*)in[7].p, (const uint8_t*)cs.p,
                                         (const int64_t*)cd.p, (const uint64_t*)po.p, ptotal ? (const uint32_t*)pa.p : nullptr, ptotal, (uint64_t*)fo.p, (uint32_t*)fm.p,
                                         (uint8_t*)ff.p, (int64_t*)fg.p, (uint64_t*)fp.p, (uint64_t*)so.p, &Mf, &total, nullptr);
    if (r) return r;
    AIXCHK(sb.alloc(total));
    r = aix_scaffold_fill_emit_dev(U, d_off, (const uint8_t*)in[1].p, min_gap, Sc, (const uint64_t*)fo.p, Mf, (const uint32_t*)fm.p, (const uint8_t*)ff.p,
                                   (const int64_t*)fg.p, (const uint64_t*)fp.p, (const uint64_t*)so.p, total, (uint8_t*)sb.p, nullptr);
    if (r) return r;
    const HostOut outs[] = {{(void**)fscaffold_offsets_out, so.p, 8 * (Sc + 1)}, {(void**)fscaffold_bases_out, sb.p, total}, {(void**)fmember_off_out, fo.p, 8 * (Sc + 1)},
                            {(void**)fmember_out, fm.p, 4 * Mf},                 {(void**)fmember_flag_out, ff.p, Mf},       {(void**)fmember_gap_out, fg.p, 8 * Mf},
                            {(void**)fmember_pos_out, fp.p, 8 * Mf},             {(void**)close_status_out, cs.p, NE},       {(void**)close_dist_out, cd.p, 8 * NE},
                            {(void**)close_states_out, cn.p, 4 * NE},            {(void**)path_off_out, po.p, 8 * (NE + 1)}, {(void**)path_out, pa.p, 4 * ptotal},
                            {(void**)fill_uses_out, fu.p, 4 * U},                {(void**)counts_out, ct.p, 40}};
    AIXCHK(copy_out_host(outs, 14));
    *n_fmembers_out = Mf; *total_bases_out = total; *path_total_out = ptotal;
    return AIX_OK;
}
