// aix_phase.hip — the variant sites of aix_pile_call_dev phased with reads: which alternative bases lie together on one haplotype. The
// placements of aix_pile_place_dev give the read byte at every site a read covers; a fragment (a read, or a read and its mate) that shows
// the contig's base or the alternative base at two sites links them; links are counted per pair of sites; every site hangs itself on its
// best decided edge, and pointer jumping with a parity bit turns that forest into blocks and phases. The contract is stated above the
// declarations in include/aindex_hip.h; DESIGN 5q has the derivations and the resources. What it shares with aix_pileup.hip is in
// aix_pile.hpp. Integer only, no LDS, no grid-wide barrier, no spin-wait; one plain launch per step:
//   aix_phase_observe_dev
//     validate k_ph_obs_validate: the placements as aix_pileup_dev validates them, the sites, and g_site[v] (scratch)
//     count    k_ph_count: one lane per placement: the sites under it by two bisections of g_site; a scan gives the flat space of raws
//     raws     k_ph_raws: one lane per raw observation: key = fragment << 32 | site, value = 1 << allele
//     sort     one radix sort of the keys, then a reduce by key that ORs the values: one mask per (fragment, site) group
//     groups   k_ph_groups: mask 1 or 2 is an observation, a mask with bit 2 is dropped as other, mask 3 as discordant; a scan ranks them
//     compact  k_ph_compact: the observations in key order (scratch), k_ph_frag_off: the CSR over fragments by bisection
//     links    k_ph_link_flag: an observation links to the one before it in the same fragment on the same contig; a scan ranks the links
//     emit     k_ph_emit: the observations and the links, each kind only when it fits its cap
//   aix_phase_bundle_dev
//     validate k_ph_bd_validate, then one radix sort of hi << 32 | lo and a reduce by key of (cis, trans); k_ph_bd_emit, k_ph_bd_off
//   aix_phase_solve_dev
//     validate k_ph_sv_validate: one lane per site and per edge
//     parent   k_ph_parent: one lane per site walks its row: state[w] = parent | sign << 32 (itself | 0 for a root), child[parent] = 1
//     jump     k_ph_jump, ceil_log2(V) rounds: state[w] = (ancestor of the ancestor, parity ^ the ancestor's parity), one word per site
//     write    k_ph_sites and k_ph_edges
//   aix_phase_tag_dev
//     validate k_ph_tag_validate, then k_ph_tag: one lane per fragment walks its observations
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "aix_pile.hpp"
#include "aix_seqhits.hpp"

namespace aix {

static constexpr uint8_t kPhaseNone = AIX_PHASE_NONE;
static constexpr uint64_t kPhLow = 0xFFFFFFFFull;
static constexpr uint64_t kPhParity = 1ULL << 32;                 // the parity bit of a jumping state; the ancestor is the low word
static constexpr uint32_t kPhAllele = 1u << 31;                   // the allele bit of a compacted observation; the site is below it

struct PhCounters {                                               // one zeroed record per call
    unsigned long long bad, a, b, c, d, e, f;
};

struct PhSites {
    uint64_t V;
    const uint32_t *unitig, *pos;
    const uint8_t *ref, *alt;
};

// the global base of site v; false when its contig or its position is out of range. Only entry v of the site arrays is read, and
// offsets only behind the test of u.
__device__ __forceinline__ bool ph_site_g(const PhSites& sv, uint64_t v, uint64_t U, const uint64_t* __restrict__ offsets, uint64_t& g) {
    const uint64_t u = sv.unitig[v];
    if (u >= U) return false;
    const uint64_t lo = offsets[u], hi = offsets[u + 1], p = sv.pos[v];
    if (hi < lo || p >= hi - lo) return false;
    g = lo + p;
    return true;
}

// ---------------------------------------------------------------------------------------------
// 1. placements and read bytes -> observations and links
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kCB) k_ph_obs_validate(const PlPlaces g, const PhSites sv, uint64_t* __restrict__ g_site, PhCounters* __restrict__ ctr) {
    const uint64_t work = std::max(std::max(std::max(g.M, g.U) + 1, g.R), sv.V), stride = (uint64_t)gridDim.x * kCB;
    unsigned long long bad = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kCB + threadIdx.x; i < work; i += stride) {
        bad += pl_places_bad(g, i);
        if (i >= sv.V) continue;
        uint64_t gv = 0, gp = 0;
        if (!ph_site_g(sv, i, g.U, g.offsets, gv)) { ++bad; continue; }
        g_site[i] = gv;
        const uint32_t r = sv.ref[i], a = sv.alt[i];
        bad += !pl_is_base(r) || !pl_is_base(a) || r == a;
        if (i) bad += !ph_site_g(sv, i - 1, g.U, g.offsets, gp) || gp >= gv;
    }
    count_add(bad, &ctr->bad);
}

// lane r < R: first[r], cnt[r] = the sites under placement r; rd0[r] the index in seqs of its first read byte; frag[r] its fragment.
// cnt[R] = 0: the scan's last entry is the total.
__global__ void __launch_bounds__(kCB) k_ph_count(const PlPlaces g, uint64_t V, const uint64_t* __restrict__ g_site, uint32_t gshift, uint32_t* __restrict__ first,
                                                 uint64_t* __restrict__ cnt, uint64_t* __restrict__ rd0, uint32_t* __restrict__ frag) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t r = (uint64_t)blockIdx.x * kCB + threadIdx.x; r <= g.R; r += stride) {
        if (r == g.R) { cnt[r] = 0; continue; }
        uint64_t j, lo, hi;
        if (!pl_seq_of(g.spo, g.M, r, j, lo, hi)) { cnt[r] = 0; continue; }        // (never: the arrays passed the validation)
        const uint64_t g0 = g.offsets[g.unitig[r]] + g.pos[r];
        const uint64_t a = first_ge(g_site, 0, V, g0), b = first_ge(g_site, a, V, g0 + g.len[r]);
        first[r] = (uint32_t)a;
        cnt[r] = b - a;
        rd0[r] = g.offs[j] + g.q0[r];
        frag[r] = (uint32_t)(j >> gshift);
    }
}

// One lane per raw observation of the flat space poff[R]: raw i belongs to the last placement r with poff[r] <= i (a placement without
// sites is never that one), and is its site first[r] + (i - poff[r]). The wave's first raw is searched by bisection (the same addresses
// in every lane), every lane gallops from there, as k_pl_bases does.
__global__ void __launch_bounds__(kCB) k_ph_raws(const PlPlaces g, const PhSites sv, const uint64_t* __restrict__ g_site, const uint64_t* __restrict__ poff,
                                                const uint32_t* __restrict__ first, const uint64_t* __restrict__ rd0, const uint32_t* __restrict__ frag,
                                                const uint8_t* __restrict__ seqs, uint64_t* __restrict__ key, uint8_t* __restrict__ mask) {
    const uint64_t R = g.R, total = poff[R], stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t base = (uint64_t)blockIdx.x * kCB + (threadIdx.x & ~63u); base < total; base += stride) {      // wave-uniform
        const uint64_t i = base + (threadIdx.x & 63u);
        if (i >= total) continue;
        const uint64_t r0 = last_le(poff, 0, R, base);
        const uint64_t r = gallop_last_le(poff, R, r0, i);
        const uint64_t v = first[r] + (i - poff[r]), len = g.len[r];
        const uint64_t x = g_site[v] - (g.offsets[g.unitig[r]] + g.pos[r]);      // < len: the count kernel chose v so
        uint32_t c;
        if (g.flag[r] & 1u) {
            c = seqs[rd0[r] + len - 1 - x];
            if (pl_is_base(c)) c = comp_ascii((uint8_t)c);
        } else {
            c = seqs[rd0[r] + x];
        }
        const uint32_t allele = c == sv.ref[v] ? 0u : c == sv.alt[v] ? 1u : 2u;
        key[i] = (uint64_t)frag[r] << 32 | v;
        mask[i] = (uint8_t)(1u << allele);
    }
}

struct PhOr {
    __host__ __device__ uint8_t operator()(uint8_t a, uint8_t b) const { return a | b; }
};

// keep[j] = group j is an observation (mask 1: the contig's base, mask 2: the alternative); keep[G] = 0: the scan's last entry is the total
__global__ void __launch_bounds__(kCB) k_ph_groups(uint64_t G, const uint8_t* __restrict__ gmask, uint8_t* __restrict__ keep, PhCounters* __restrict__ ctr) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    unsigned long long other = 0, disc = 0;
    for (uint64_t j = (uint64_t)blockIdx.x * kCB + threadIdx.x; j <= G; j += stride) {
        const uint32_t m = j < G ? gmask[j] : 0u;
        keep[j] = m == 1u || m == 2u;
        other += (m & 4u) != 0;
        disc += m == 3u;
    }
    count_add(other, &ctr->a);
    count_add(disc, &ctr->b);
}

// okey[rank] = fragment << 32 | allele << 31 | site of every kept group, in key order
__global__ void __launch_bounds__(kCB) k_ph_compact(uint64_t G, const uint64_t* __restrict__ gkey, const uint8_t* __restrict__ gmask, const uint8_t* __restrict__ keep,
                                                   const uint64_t* __restrict__ rank, uint64_t* __restrict__ okey) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t j = (uint64_t)blockIdx.x * kCB + threadIdx.x; j < G; j += stride)
        if (keep[j]) okey[rank[j]] = gkey[j] | (gmask[j] == 2u ? kPhAllele : 0u);
}

// frag_obs_off[f] = the observations of fragments below f
__global__ void __launch_bounds__(kCB) k_ph_frag_off(uint64_t F, const uint64_t* __restrict__ okey, uint64_t n_obs, uint64_t* __restrict__ frag_obs_off) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t f = (uint64_t)blockIdx.x * kCB + threadIdx.x; f <= F; f += stride) frag_obs_off[f] = first_ge(okey, 0, n_obs, f << 32);
}

// lf[o] = observation o follows one of the same fragment on the same contig; lf[n_obs] = 0
__global__ void __launch_bounds__(kCB) k_ph_link_flag(uint64_t n_obs, const uint64_t* __restrict__ okey, const uint32_t* __restrict__ var_unitig, uint8_t* __restrict__ lf) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t o = (uint64_t)blockIdx.x * kCB + threadIdx.x; o <= n_obs; o += stride) {
        bool link = false;
        if (o && o < n_obs) {
            const uint64_t a = okey[o - 1], b = okey[o];
            link = (a >> 32) == (b >> 32) && var_unitig[a & (kPhAllele - 1)] == var_unitig[b & (kPhAllele - 1)];
        }
        lf[o] = link;
    }
}

struct PhObsOut {
    uint32_t* obs_site;
    uint8_t* obs_allele;
    uint32_t *link_lo, *link_hi;
    uint8_t* link_rel;
    bool obs, links;                                              // the kind fits its cap
};

__global__ void __launch_bounds__(kCB) k_ph_emit(uint64_t n_obs, const uint64_t* __restrict__ okey, const uint8_t* __restrict__ lf, const uint64_t* __restrict__ lrank,
                                                const PhObsOut out) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t o = (uint64_t)blockIdx.x * kCB + threadIdx.x; o < n_obs; o += stride) {
        const uint32_t b = (uint32_t)okey[o];
        if (out.obs) {
            out.obs_site[o] = b & (kPhAllele - 1);
            out.obs_allele[o] = (uint8_t)(b >> 31);
        }
        if (out.links && lf[o]) {
            const uint32_t a = (uint32_t)okey[o - 1];
            const uint64_t l = lrank[o];
            out.link_lo[l] = a & (kPhAllele - 1);
            out.link_hi[l] = b & (kPhAllele - 1);
            out.link_rel[l] = (uint8_t)((a ^ b) >> 31);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// 2. links -> counted edges
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kCB) k_ph_bd_validate(uint64_t N, const uint32_t* __restrict__ lo, const uint32_t* __restrict__ hi, const uint8_t* __restrict__ rel,
                                                       uint64_t V, PhCounters* __restrict__ ctr) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    unsigned long long bad = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kCB + threadIdx.x; i < N; i += stride) {
        const uint64_t a = lo[i], b = hi[i];
        bad += !(a < b && b < V) || rel[i] > 1;
    }
    count_add(bad, &ctr->bad);
}

struct PhKeyOf {                                                  // hi << 32 | lo of link i: ascending (hi, lo)
    const uint32_t *lo, *hi;
    __host__ __device__ uint64_t operator()(uint64_t i) const { return (uint64_t)hi[i] << 32 | lo[i]; }
};
struct PhAgg {
    uint32_t cis, trans;
};
struct PhAggOp {
    __host__ __device__ PhAgg operator()(const PhAgg& a, const PhAgg& b) const { return PhAgg{a.cis + b.cis, a.trans + b.trans}; }
};
struct PhAggOf {
    __host__ __device__ PhAgg operator()(uint8_t rel) const { return PhAgg{rel ? 0u : 1u, rel ? 1u : 0u}; }
};

__global__ void __launch_bounds__(kCB) k_ph_bd_emit(uint64_t E, const uint64_t* __restrict__ uniq, const PhAgg* __restrict__ agg, uint32_t* __restrict__ edge_lo,
                                                   uint32_t* __restrict__ edge_hi, uint32_t* __restrict__ cis, uint32_t* __restrict__ trans) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t e = (uint64_t)blockIdx.x * kCB + threadIdx.x; e < E; e += stride) {
        const uint64_t k = uniq[e];
        const PhAgg a = agg[e];
        edge_lo[e] = (uint32_t)k;
        edge_hi[e] = (uint32_t)(k >> 32);
        cis[e] = a.cis;
        trans[e] = a.trans;
    }
}

// edge_off[w] = the edges whose hi is below w
__global__ void __launch_bounds__(kCB) k_ph_bd_off(uint64_t V, const uint64_t* __restrict__ uniq, uint64_t E, uint64_t* __restrict__ edge_off) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t w = (uint64_t)blockIdx.x * kCB + threadIdx.x; w <= V; w += stride) edge_off[w] = first_ge(uniq, 0, E, w << 32);
}

// ---------------------------------------------------------------------------------------------
// 3. edges -> blocks and phases
// ---------------------------------------------------------------------------------------------
struct PhEdges {
    uint64_t V, E;
    const uint32_t* var_unitig;
    const uint64_t* edge_off;
    const uint32_t *lo, *cis, *trans;
    uint32_t min_reads, permille;
};

__global__ void __launch_bounds__(kCB) k_ph_sv_validate(const PhEdges g, PhCounters* __restrict__ ctr) {
    const uint64_t work = std::max(g.V, g.E), stride = (uint64_t)gridDim.x * kCB;
    unsigned long long bad = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kCB + threadIdx.x; i < work; i += stride) {
        if (i < g.V) {
            bad += csr_bad(i, g.V, g.edge_off[i], g.edge_off[i + 1], g.E, kAnyDegree);
            if (i) bad += g.var_unitig[i - 1] > g.var_unitig[i];
        }
        if (i >= g.E) continue;
        uint64_t w, a, b;
        if (!pl_seq_of(g.edge_off, g.V, i, w, a, b)) { ++bad; continue; }
        const uint64_t l = g.lo[i];
        if (l >= w) { ++bad; continue; }
        bad += g.var_unitig[l] != g.var_unitig[w];
        if (i > a) bad += (uint64_t)g.lo[i - 1] >= l;
    }
    count_add(bad, &ctr->bad);
}

// an edge is decided iff n = cis + trans >= max(min_reads, 1), cis != trans and 1000 max(cis, trans) >= permille n, exactly
__device__ __forceinline__ bool ph_decided(const PhEdges& g, uint64_t j, uint64_t& n, uint64_t& m, uint32_t& sign) {
    const uint64_t c = g.cis[j], t = g.trans[j];
    n = c + t;
    m = c > t ? c : t;
    sign = t > c;
    return n >= (g.min_reads > 1u ? g.min_reads : 1u) && c != t && pl_reaches(1000ull * m, g.permille, n);
}

// state[w] = parent | sign << 32: among the decided edges of row w the one with the largest n, then the largest m, then the largest lo
// (the row ascends in lo: a later edge wins a tie). A root is its own parent with sign 0. child[] was zeroed; every writer stores 1.
__global__ void __launch_bounds__(kCB) k_ph_parent(const PhEdges g, uint64_t* __restrict__ state, uint8_t* __restrict__ child, uint32_t* __restrict__ site_parent) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t w = (uint64_t)blockIdx.x * kCB + threadIdx.x; w < g.V; w += stride) {
        uint64_t bn = 0, bm = 0, word = w;
        bool found = false;
        for (uint64_t j = g.edge_off[w], hi = g.edge_off[w + 1]; j < hi; ++j) {
            uint64_t n, m;
            uint32_t sign;
            if (!ph_decided(g, j, n, m, sign)) continue;
            if (!found || n > bn || (n == bn && m >= bm)) {
                found = true;
                bn = n;
                bm = m;
                word = (uint64_t)g.lo[j] | (sign ? kPhParity : 0);
            }
        }
        state[w] = word;
        if (found) child[word & kPhLow] = 1;
        if (site_parent) site_parent[w] = found ? (uint32_t)word : kNoEnd;
    }
}

// One round: the ancestor's own state is one aligned 8-byte word of the buffer this round only reads, so ancestor and parity are a
// consistent pair. A root points at itself with parity 0 and stays.
__global__ void __launch_bounds__(kCB) k_ph_jump(uint64_t V, const uint64_t* __restrict__ in, uint64_t* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t w = (uint64_t)blockIdx.x * kCB + threadIdx.x; w < V; w += stride) {
        const uint64_t s = in[w], t = in[s & kPhLow];
        out[w] = (t & kPhLow) | ((s ^ t) & kPhParity);
    }
}

__global__ void __launch_bounds__(kCB) k_ph_sites(uint64_t V, const uint64_t* __restrict__ state, const uint8_t* __restrict__ child, uint32_t* __restrict__ site_block,
                                                 uint8_t* __restrict__ site_phase, PhCounters* __restrict__ ctr) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    unsigned long long blocks = 0, phased = 0;
    for (uint64_t w = (uint64_t)blockIdx.x * kCB + threadIdx.x; w < V; w += stride) {
        const uint64_t s = state[w], root = s & kPhLow;
        const bool alone = root == w && !child[w];
        site_block[w] = (uint32_t)root;
        site_phase[w] = alone ? kPhaseNone : (uint8_t)((s & kPhParity) != 0);
        blocks += root == w && !alone;
        phased += !alone;
    }
    count_add(blocks, &ctr->a);
    count_add(phased, &ctr->b);
}

// One lane per edge: its row by bisection of edge_off. The hi end of a decided edge has a parent, so it is phased; the lo end may be a
// root nobody chose, and then the edge lies across blocks like any other whose ends have different roots.
__global__ void __launch_bounds__(kCB) k_ph_edges(const PhEdges g, const uint64_t* __restrict__ state, uint8_t* __restrict__ edge_state, PhCounters* __restrict__ ctr) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    unsigned long long decided = 0, agree = 0, conflict = 0, across = 0;
    for (uint64_t j = (uint64_t)blockIdx.x * kCB + threadIdx.x; j < g.E; j += stride) {
        uint64_t w, a, b, n, m;
        uint32_t sign, st = 0;
        if (!pl_seq_of(g.edge_off, g.V, j, w, a, b)) continue;   // (never: the arrays passed the validation)
        if (ph_decided(g, j, n, m, sign)) {
            const uint64_t sl = state[g.lo[j]], sh = state[w];
            if ((sl & kPhLow) != (sh & kPhLow)) st = 3;
            else st = (uint32_t)(((sl ^ sh) & kPhParity) != 0) == sign ? 1 : 2;
            ++decided;
            agree += st == 1;
            conflict += st == 2;
            across += st == 3;
        }
        if (edge_state) edge_state[j] = (uint8_t)st;
    }
    count_add(decided, &ctr->c);
    count_add(agree, &ctr->d);
    count_add(conflict, &ctr->e);
    count_add(across, &ctr->f);
}

// ---------------------------------------------------------------------------------------------
// 4. fragments -> haplotype tags
// ---------------------------------------------------------------------------------------------
struct PhTagIn {
    uint64_t F, n_obs, V;
    const uint64_t* frag_obs_off;
    const uint32_t* obs_site;
    const uint8_t* obs_allele;
    const uint32_t* site_block;
    const uint8_t* site_phase;
};

__global__ void __launch_bounds__(kCB) k_ph_tag_validate(const PhTagIn g, PhCounters* __restrict__ ctr) {
    const uint64_t work = std::max(std::max(g.F, g.n_obs), g.V), stride = (uint64_t)gridDim.x * kCB;
    unsigned long long bad = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kCB + threadIdx.x; i < work; i += stride) {
        if (i < g.F) bad += csr_bad(i, g.F, g.frag_obs_off[i], g.frag_obs_off[i + 1], g.n_obs, kAnyDegree);
        if (i < g.n_obs) bad += g.obs_site[i] >= g.V || g.obs_allele[i] > 1;
        if (i < g.V) {
            const uint32_t p = g.site_phase[i];
            bad += g.site_block[i] > i || !(p <= 1u || p == kPhaseNone);
        }
    }
    count_add(bad, &ctr->bad);
}

__global__ void __launch_bounds__(kCB) k_ph_tag(const PhTagIn g, uint32_t* __restrict__ tag_block, uint32_t* __restrict__ tag_h0, uint32_t* __restrict__ tag_h1,
                                               uint32_t* __restrict__ tag_other) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t f = (uint64_t)blockIdx.x * kCB + threadIdx.x; f < g.F; f += stride) {
        uint32_t block = kNoEnd, h[2] = {0, 0}, other = 0;
        for (uint64_t o = g.frag_obs_off[f], hi = g.frag_obs_off[f + 1]; o < hi; ++o) {
            const uint32_t v = g.obs_site[o], p = g.site_phase[v];
            if (p == kPhaseNone) continue;
            const uint32_t b = g.site_block[v];
            if (block == kNoEnd) block = b;
            if (b == block) ++h[(g.obs_allele[o] ^ p) & 1u]; else ++other;
        }
        tag_block[f] = block;
        tag_h0[f] = h[0];
        tag_h1[f] = h[1];
        tag_other[f] = other;
    }
}

// u64 words from the host into a nullable device array; synchronises `s`
static hipError_t ph_put(uint64_t* d_dst, const unsigned long long* src, int n, hipStream_t s) {
    if (!d_dst) return hipSuccess;
    AIX_TRY(hipMemcpyAsync(d_dst, src, 8 * n, hipMemcpyHostToDevice, s));
    return hipStreamSynchronize(s);
}

}  // namespace aix

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" int aix_phase_observe_dev(const char* d_seqs, const uint64_t* d_offs, uint64_t M, uint32_t group, const uint64_t* d_seq_place_off, uint64_t R,
                                     const uint32_t* d_place_unitig, const uint8_t* d_place_flag, const uint32_t* d_place_pos, const uint32_t* d_place_q0,
                                     const uint32_t* d_place_len, uint64_t U, const uint64_t* d_offsets, uint64_t V, const uint32_t* d_var_unitig,
                                     const uint32_t* d_var_pos, const uint8_t* d_var_ref, const uint8_t* d_var_alt, uint64_t* d_frag_obs_off, uint32_t* d_obs_site,
                                     uint8_t* d_obs_allele, uint64_t obs_cap, uint64_t* obs_total_out, uint32_t* d_link_lo, uint32_t* d_link_hi, uint8_t* d_link_rel,
                                     uint64_t link_cap, uint64_t* link_total_out, uint64_t* d_stats, void* stream) {
    if (U > kUnitLimit || V > kUnitLimit) return AIX_ERR_UNSUPPORTED;
    if ((group != 1 && group != 2) || M % group) return AIX_ERR_ARG;
    const uint64_t F = M / group;
    if (F > kPhLow) return AIX_ERR_UNSUPPORTED;                   // a fragment is the high word of a sort key
    if (!d_offsets || !d_frag_obs_off || !obs_total_out || !link_total_out || M >= (1ull << 56) || R >= (1ull << 56)) return AIX_ERR_ARG;
    if (M && (!d_offs || !d_seq_place_off)) return AIX_ERR_ARG;
    if (R && (!M || !U || !d_seqs || !d_place_unitig || !d_place_flag || !d_place_pos || !d_place_q0 || !d_place_len)) return AIX_ERR_ARG;
    if (V && (!d_var_unitig || !d_var_pos || !d_var_ref || !d_var_alt)) return AIX_ERR_ARG;
    if (obs_cap && (!d_obs_site || !d_obs_allele)) return AIX_ERR_ARG;
    if (link_cap && (!d_link_lo || !d_link_hi || !d_link_rel)) return AIX_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const uint64_t cap = chain_test_grid();
    const dim3 blk(kCB);
    const PlPlaces g{M, R, U, d_offs, d_seq_place_off, d_place_unitig, d_place_flag, d_place_pos, d_place_q0, d_place_len, d_offsets};
    const PhSites sv{V, d_var_unitig, d_var_pos, d_var_ref, d_var_alt};
    Counted<PhCounters> ctr(s);
    DevArr g_site(s), first(s), cnt(s), poff(s), rd0(s), frag(s), key(s), mask(s), key2(s), mask2(s), gkey(s), gmask(s), ng(s), keep(s), rank(s), okey(s), lf(s), lrank(s);
    DevArr tmp(s), tmp2(s), tmp3(s), tmp4(s), tmp5(s);
    AIXCHK(ctr.init());
    AIXCHK(sh_alloc(g_site, V, 8));
    AIXCHK(ctr.run([&]() {
        AIX_TRY_LAUNCH(k_ph_obs_validate, dim3(chain_grid(std::max(std::max(std::max(M, U) + 1, R), V), 2 * kCB, cap)), blk, 0, s, g, sv, (uint64_t*)g_site.p, ctr.dev());
        return hipSuccess;
    }));
    if (ctr.host.bad) return AIX_ERR_ARG;
    // everything is validated: from here on the outputs are written
    unsigned long long stats[6] = {0, 0, 0, 0, 0, 0};
    uint64_t Nr = 0, G = 0, n_obs = 0, n_links = 0;
    if (R && V) {
        AIXCHK(sh_alloc(first, R, 4));
        AIXCHK(sh_alloc(cnt, R + 1, 8));
        AIXCHK(sh_alloc(poff, R + 1, 8));
        AIXCHK(sh_alloc(rd0, R, 8));
        AIXCHK(sh_alloc(frag, R, 4));
        hipLaunchKernelGGL(k_ph_count, dim3(chain_grid(R + 1, 2 * kCB, cap)), blk, 0, s, g, V, (const uint64_t*)g_site.p, group - 1, (uint32_t*)first.p, (uint64_t*)cnt.p,
                           (uint64_t*)rd0.p, (uint32_t*)frag.p);
        AIXCHK(hipGetLastError());
        AIXCHK(scan_u64((const uint64_t*)cnt.p, (uint64_t*)poff.p, R + 1, tmp, s));
        AIXCHK(hipMemcpyAsync(&Nr, (const uint64_t*)poff.p + R, 8, hipMemcpyDeviceToHost, s));
        AIXCHK(hipStreamSynchronize(s));
    }
    if (Nr) {
        AIXCHK(sh_alloc(key, Nr, 8));
        AIXCHK(sh_alloc(mask, Nr, 1));
        AIXCHK(sh_alloc(key2, Nr, 8));
        AIXCHK(sh_alloc(mask2, Nr, 1));
        AIXCHK(sh_alloc(gkey, Nr, 8));
        AIXCHK(sh_alloc(gmask, Nr, 1));
        AIXCHK(ng.alloc(8));
        hipLaunchKernelGGL(k_ph_raws, dim3(chain_grid(Nr, kCB, cap)), blk, 0, s, g, sv, (const uint64_t*)g_site.p, (const uint64_t*)poff.p, (const uint32_t*)first.p,
                           (const uint64_t*)rd0.p, (const uint32_t*)frag.p, (const uint8_t*)d_seqs, (uint64_t*)key.p, (uint8_t*)mask.p);
        AIXCHK(hipGetLastError());
        AIXCHK(sort_pairs((const uint64_t*)key.p, (uint64_t*)key2.p, (const uint8_t*)mask.p, (uint8_t*)mask2.p, Nr, sort_bits((F - 1) << 32 | (V - 1)), tmp2, s));
        AIXCHK(with_temp(tmp3, [&](void* t, size_t& tb) {
            return rocprim::reduce_by_key(t, tb, (const uint64_t*)key2.p, (const uint8_t*)mask2.p, (size_t)Nr, (uint64_t*)gkey.p, (uint8_t*)gmask.p, (uint64_t*)ng.p, PhOr(),
                                          rocprim::equal_to<uint64_t>(), s);
        }));
        AIXCHK(hipMemcpyAsync(&G, ng.p, 8, hipMemcpyDeviceToHost, s));
        AIXCHK(hipStreamSynchronize(s));
        G = std::min(G, Nr);
        AIXCHK(sh_alloc(keep, G + 1, 1));
        AIXCHK(sh_alloc(rank, G + 1, 8));
        AIXCHK(ctr.run([&]() {
            AIX_TRY_LAUNCH(k_ph_groups, dim3(chain_grid(G + 1, 4 * kCB, cap)), blk, 0, s, G, (const uint8_t*)gmask.p, (uint8_t*)keep.p, ctr.dev());
            AIX_TRY(scan_u64(rocprim::make_transform_iterator((const uint8_t*)keep.p, Widen<uint8_t>()), (uint64_t*)rank.p, G + 1, tmp4, s));
            return hipMemcpyAsync(&n_obs, (const uint64_t*)rank.p + G, 8, hipMemcpyDeviceToHost, s);
        }));
        stats[2] = ctr.host.a;
        stats[3] = ctr.host.b;
    }
    if (n_obs) {
        AIXCHK(sh_alloc(okey, n_obs, 8));
        AIXCHK(sh_alloc(lf, n_obs + 1, 1));
        AIXCHK(sh_alloc(lrank, n_obs + 1, 8));
        hipLaunchKernelGGL(k_ph_compact, dim3(chain_grid(G, 4 * kCB, cap)), blk, 0, s, G, (const uint64_t*)gkey.p, (const uint8_t*)gmask.p, (const uint8_t*)keep.p,
                           (const uint64_t*)rank.p, (uint64_t*)okey.p);
        AIXCHK(hipGetLastError());
        hipLaunchKernelGGL(k_ph_frag_off, dim3(chain_grid(F + 1, 4 * kCB, cap)), blk, 0, s, F, (const uint64_t*)okey.p, n_obs, d_frag_obs_off);
        AIXCHK(hipGetLastError());
        hipLaunchKernelGGL(k_ph_link_flag, dim3(chain_grid(n_obs + 1, 4 * kCB, cap)), blk, 0, s, n_obs, (const uint64_t*)okey.p, d_var_unitig, (uint8_t*)lf.p);
        AIXCHK(hipGetLastError());
        AIXCHK(scan_u64(rocprim::make_transform_iterator((const uint8_t*)lf.p, Widen<uint8_t>()), (uint64_t*)lrank.p, n_obs + 1, tmp5, s));
        AIXCHK(hipMemcpyAsync(&n_links, (const uint64_t*)lrank.p + n_obs, 8, hipMemcpyDeviceToHost, s));
        AIXCHK(hipStreamSynchronize(s));
        const PhObsOut out{d_obs_site, d_obs_allele, d_link_lo, d_link_hi, d_link_rel, n_obs <= obs_cap, n_links && n_links <= link_cap};
        if (out.obs || out.links) {
            hipLaunchKernelGGL(k_ph_emit, dim3(chain_grid(n_obs, 4 * kCB, cap)), blk, 0, s, n_obs, (const uint64_t*)okey.p, (const uint8_t*)lf.p, (const uint64_t*)lrank.p, out);
            AIXCHK(hipGetLastError());
        }
        AIXCHK(hipStreamSynchronize(s));
    } else {
        AIXCHK(zero_offsets(d_frag_obs_off, F, s));
    }
    stats[0] = Nr; stats[1] = G; stats[4] = n_obs; stats[5] = n_links;
    AIXCHK(ph_put(d_stats, stats, 6, s));
    *obs_total_out = n_obs;
    *link_total_out = n_links;
    return AIX_OK;
}

extern "C" int aix_phase_bundle_dev(uint64_t V, uint64_t N, const uint32_t* d_link_lo, const uint32_t* d_link_hi, const uint8_t* d_link_rel, uint32_t* d_edge_lo,
                                    uint32_t* d_edge_hi, uint32_t* d_edge_cis, uint32_t* d_edge_trans, uint64_t* d_edge_off, uint64_t* n_edges_out, void* stream) {
    if (V > kUnitLimit || N > kPhLow) return AIX_ERR_UNSUPPORTED;  // N: the counters of an edge are 32 bits wide
    if (!d_edge_off || !n_edges_out) return AIX_ERR_ARG;
    if (N && (!d_link_lo || !d_link_hi || !d_link_rel || !d_edge_lo || !d_edge_hi || !d_edge_cis || !d_edge_trans)) return AIX_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const uint64_t cap = chain_test_grid();
    const dim3 blk(kCB);
    uint64_t E = 0;
    if (N) {
        Counted<PhCounters> ctr(s);
        DevArr k2(s), r2(s), uniq(s), agg(s), cnt(s), tmp(s), tmp2(s);
        AIXCHK(ctr.init());
        AIXCHK(ctr.run([&]() {
            AIX_TRY_LAUNCH(k_ph_bd_validate, dim3(chain_grid(N, 4 * kCB, cap)), blk, 0, s, N, d_link_lo, d_link_hi, d_link_rel, V, ctr.dev());
            return hipSuccess;
        }));
        if (ctr.host.bad) return AIX_ERR_ARG;
        AIXCHK(sh_alloc(k2, N, 8));
        AIXCHK(sh_alloc(r2, N, 1));
        AIXCHK(sh_alloc(uniq, N, 8));
        AIXCHK(sh_alloc(agg, N, sizeof(PhAgg)));
        AIXCHK(cnt.alloc(8));
        const auto keys = rocprim::make_transform_iterator(rocprim::counting_iterator<uint64_t>(0), PhKeyOf{d_link_lo, d_link_hi});
        AIXCHK(sort_pairs(keys, (uint64_t*)k2.p, d_link_rel, (uint8_t*)r2.p, N, sort_bits((V - 1) << 32 | (V - 1)), tmp, s));
        AIXCHK(with_temp(tmp2, [&](void* t, size_t& tb) {
            return rocprim::reduce_by_key(t, tb, (const uint64_t*)k2.p, rocprim::make_transform_iterator((const uint8_t*)r2.p, PhAggOf()), (size_t)N, (uint64_t*)uniq.p,
                                          (PhAgg*)agg.p, (uint64_t*)cnt.p, PhAggOp(), rocprim::equal_to<uint64_t>(), s);
        }));
        AIXCHK(hipMemcpyAsync(&E, cnt.p, 8, hipMemcpyDeviceToHost, s));
        AIXCHK(hipStreamSynchronize(s));
        E = std::min(E, N);
        hipLaunchKernelGGL(k_ph_bd_emit, dim3(chain_grid(E, 4 * kCB, cap)), blk, 0, s, E, (const uint64_t*)uniq.p, (const PhAgg*)agg.p, d_edge_lo, d_edge_hi, d_edge_cis,
                           d_edge_trans);
        AIXCHK(hipGetLastError());
        hipLaunchKernelGGL(k_ph_bd_off, dim3(chain_grid(V + 1, 4 * kCB, cap)), blk, 0, s, V, (const uint64_t*)uniq.p, E, d_edge_off);
        AIXCHK(hipGetLastError());
        AIXCHK(hipStreamSynchronize(s));
    } else {
        AIXCHK(zero_offsets(d_edge_off, V, s));
    }
    *n_edges_out = E;
    return AIX_OK;
}

extern "C" int aix_phase_solve_dev(uint64_t V, const uint32_t* d_var_unitig, const uint64_t* d_edge_off, uint64_t E, const uint32_t* d_edge_lo, const uint32_t* d_edge_cis,
                                   const uint32_t* d_edge_trans, uint32_t min_link_reads, uint32_t min_link_permille, uint32_t* d_site_block, uint8_t* d_site_phase,
                                   uint32_t* d_site_parent, uint8_t* d_edge_state, uint64_t* d_counts, void* stream) {
    if (V > kUnitLimit) return AIX_ERR_UNSUPPORTED;
    if (!d_edge_off || E >= (1ull << 56)) return AIX_ERR_ARG;
    if (V && (!d_var_unitig || !d_site_block || !d_site_phase)) return AIX_ERR_ARG;
    if (E && (!V || !d_edge_lo || !d_edge_cis || !d_edge_trans)) return AIX_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const uint64_t cap = chain_test_grid();
    const dim3 blk(kCB);
    const PhEdges g{V, E, d_var_unitig, d_edge_off, d_edge_lo, d_edge_cis, d_edge_trans, min_link_reads, min_link_permille};
    Counted<PhCounters> ctr(s);
    AIXCHK(ctr.init());
    uint64_t first = 0;
    AIXCHK(ctr.run([&]() {
        AIX_TRY_LAUNCH(k_ph_sv_validate, dim3(chain_grid(std::max(V, E), 2 * kCB, cap)), blk, 0, s, g, ctr.dev());
        return hipMemcpyAsync(&first, d_edge_off, 8, hipMemcpyDeviceToHost, s);
    }));
    if (ctr.host.bad || (V == 0 && first != 0)) return AIX_ERR_ARG;
    // everything is validated: from here on the outputs are written
    unsigned long long counts[6] = {0, 0, 0, 0, 0, 0};
    if (V) {
        DevArr st_a(s), st_b(s), child(s);
        AIXCHK(sh_alloc(st_a, V, 8));
        AIXCHK(sh_alloc(st_b, V, 8));
        AIXCHK(sh_alloc(child, V, 1));
        AIXCHK(hipMemsetAsync(child.p, 0, V, s));
        uint64_t *cur = (uint64_t*)st_a.p, *nxt = (uint64_t*)st_b.p;
        AIXCHK(ctr.run([&]() {
            const unsigned grid = chain_grid(V, 2 * kCB, cap);
            AIX_TRY_LAUNCH(k_ph_parent, dim3(grid), blk, 0, s, g, cur, (uint8_t*)child.p, d_site_parent);
            for (int r = 0, rounds = ceil_log2(V); r < rounds; ++r) {
                AIX_TRY_LAUNCH(k_ph_jump, dim3(grid), blk, 0, s, V, (const uint64_t*)cur, nxt);
                std::swap(cur, nxt);
            }
            AIX_TRY_LAUNCH(k_ph_sites, dim3(grid), blk, 0, s, V, (const uint64_t*)cur, (const uint8_t*)child.p, d_site_block, d_site_phase, ctr.dev());
            if (E && (d_edge_state || d_counts)) AIX_TRY_LAUNCH(k_ph_edges, dim3(chain_grid(E, 2 * kCB, cap)), blk, 0, s, g, (const uint64_t*)cur, d_edge_state, ctr.dev());
            return hipSuccess;
        }));
        const PhCounters& h = ctr.host;
        counts[0] = h.a; counts[1] = h.b; counts[2] = h.c; counts[3] = h.d; counts[4] = h.e; counts[5] = h.f;
    }
    AIXCHK(ph_put(d_counts, counts, 6, s));
    return AIX_OK;
}

extern "C" int aix_phase_tag_dev(uint64_t F, const uint64_t* d_frag_obs_off, uint64_t n_obs, const uint32_t* d_obs_site, const uint8_t* d_obs_allele, uint64_t V,
                                 const uint32_t* d_site_block, const uint8_t* d_site_phase, uint32_t* d_tag_block, uint32_t* d_tag_h0, uint32_t* d_tag_h1,
                                 uint32_t* d_tag_other, void* stream) {
    if (V > kUnitLimit) return AIX_ERR_UNSUPPORTED;
    if (!d_frag_obs_off || F >= (1ull << 56) || n_obs >= (1ull << 56)) return AIX_ERR_ARG;
    if (F && (!d_tag_block || !d_tag_h0 || !d_tag_h1 || !d_tag_other)) return AIX_ERR_ARG;
    if (n_obs && (!F || !V || !d_obs_site || !d_obs_allele)) return AIX_ERR_ARG;
    if (V && (!d_site_block || !d_site_phase)) return AIX_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const uint64_t cap = chain_test_grid();
    const dim3 blk(kCB);
    const PhTagIn g{F, n_obs, V, d_frag_obs_off, d_obs_site, d_obs_allele, d_site_block, d_site_phase};
    Counted<PhCounters> ctr(s);
    AIXCHK(ctr.init());
    AIXCHK(ctr.run([&]() {
        AIX_TRY_LAUNCH(k_ph_tag_validate, dim3(chain_grid(std::max(std::max(F, n_obs), V), 2 * kCB, cap)), blk, 0, s, g, ctr.dev());
        return hipSuccess;
    }));
    if (ctr.host.bad) return AIX_ERR_ARG;
    if (F) {
        hipLaunchKernelGGL(k_ph_tag, dim3(chain_grid(F, 2 * kCB, cap)), blk, 0, s, g, d_tag_block, d_tag_h0, d_tag_h1, d_tag_other);
        AIXCHK(hipGetLastError());
    }
    AIXCHK(hipStreamSynchronize(s));
    return AIX_OK;
}

// Bundle and solve for host memory, on the null stream of the current device; every output is malloc'd (aix_free).
extern "C" int aix_phase_solve(uint64_t V, const uint32_t* var_unitig, uint64_t N, const uint32_t* link_lo, const uint32_t* link_hi, const uint8_t* link_rel,
                               uint32_t min_link_reads, uint32_t min_link_permille, uint64_t* n_edges_out, uint32_t** edge_lo_out, uint32_t** edge_hi_out,
                               uint32_t** edge_cis_out, uint32_t** edge_trans_out, uint64_t** edge_off_out, uint8_t** edge_state_out, uint32_t** site_block_out,
                               uint8_t** site_phase_out, uint32_t** site_parent_out, uint64_t** counts_out) {
    if (V > kUnitLimit || N > kPhLow) return AIX_ERR_UNSUPPORTED;
    if (!n_edges_out || !edge_lo_out || !edge_hi_out || !edge_cis_out || !edge_trans_out || !edge_off_out || !site_block_out || !site_phase_out) return AIX_ERR_ARG;
    if ((V && !var_unitig) || (N && (!link_lo || !link_hi || !link_rel))) return AIX_ERR_ARG;
    DevArr in[4], el, eh, ec, et, eo, es, sb, sp, spar, cn;
    const HostIn ins[4] = {{var_unitig, 4 * V}, {link_lo, 4 * N}, {link_hi, 4 * N}, {link_rel, N}};
    AIXCHK(copy_in_host(in, ins, 4));
    AIXCHK(sh_alloc(el, N, 4));
    AIXCHK(sh_alloc(eh, N, 4));
    AIXCHK(sh_alloc(ec, N, 4));
    AIXCHK(sh_alloc(et, N, 4));
    AIXCHK(sh_alloc(eo, V + 1, 8));
    uint64_t E = 0;
    int r = aix_phase_bundle_dev(V, N, (const uint32_t*)in[1].p, (const uint32_t*)in[2].p, (const uint8_t*)in[3].p, (uint32_t*)el.p, (uint32_t*)eh.p, (uint32_t*)ec.p,
                                 (uint32_t*)et.p, (uint64_t*)eo.p, &E, nullptr);
    if (r) return r;
    AIXCHK(sh_alloc(es, E, 1));
    AIXCHK(sh_alloc(sb, V, 4));
    AIXCHK(sh_alloc(sp, V, 1));
    AIXCHK(sh_alloc(spar, V, 4));
    AIXCHK(cn.alloc(48));
    r = aix_phase_solve_dev(V, (const uint32_t*)in[0].p, (const uint64_t*)eo.p, E, (const uint32_t*)el.p, (const uint32_t*)ec.p, (const uint32_t*)et.p, min_link_reads,
                            min_link_permille, (uint32_t*)sb.p, (uint8_t*)sp.p, (uint32_t*)spar.p, (uint8_t*)es.p, (uint64_t*)cn.p, nullptr);
    if (r) return r;
    const HostOut outs[] = {{(void**)edge_lo_out, el.p, 4 * E},      {(void**)edge_hi_out, eh.p, 4 * E},     {(void**)edge_cis_out, ec.p, 4 * E},
                            {(void**)edge_trans_out, et.p, 4 * E},   {(void**)edge_off_out, eo.p, 8 * (V + 1)}, {(void**)edge_state_out, es.p, E},
                            {(void**)site_block_out, sb.p, 4 * V},   {(void**)site_phase_out, sp.p, V},      {(void**)site_parent_out, spar.p, 4 * V},
                            {(void**)counts_out, cn.p, 48}};
    AIXCHK(copy_out_host(outs, 10));
    *n_edges_out = E;
    return AIX_OK;
}
