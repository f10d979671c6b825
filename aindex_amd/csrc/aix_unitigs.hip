// aix_unitigs.hip — De Bruijn compaction: every maximal non-branching path (unitig) of a canonical 23-mer index resident in HBM, once,
// with its abundance, and the map from every stored k-mer to its unitig, offset and strand. The contract is stated above the
// declarations in include/aindex_hip.h; DESIGN 5i has the derivations and the resources.
//
// A node (stored key) has two ports: 2 kid + 0 = R (leaving in stored orientation), 2 kid + 1 = L (leaving as the reverse complement).
// The chain (one plain launch per step and per round; every host loop is bounded by a count computed on the host):
//   ports    k_ug_ports: one quad per port, the four lanes probe next(x, b) through the wave-cooperative probe with slots
//            (slot23_wave, aix_probe.hpp); one u32 word per port = the entered port of the only live successor, or a code for
//            "out-degree 0 / 2 / 3 / 4" or "dead node"
//   links    k_ug_links: port p is linked to t = word[p] iff word[t] == p (so both out-degrees are 1, and links are symmetric by
//            construction) and t is a port of another node (self-loops and hairpins are cut). Ranking state: succ(p) = t ^ 1, d = 1;
//            a port without a link is a terminal: d = 0 and an explicit flag (bit 63). A fixed point of succ is NOT the test.
//   rank     k_ug_jump: synchronous pointer jumping, double-buffered: an unflagged port takes over end, flag and distance of the port
//            it points at. After round r every port within 2^(r - 1) hops of its end is flagged; the host reads the number of unflagged
//            ports after every round and stops when it is 0 or did not change (what is left then lies on cycles).
//   cycles   only when ports are left: k_ug_cyc_init / k_ug_cyc_jump carry the minimum of (stored code, port bit) over a window of 2^r
//            successors and the distance to its first occurrence. Of the two directed port cycles of a circle the one through the R port
//            of the smallest node is kept; the position of a node is the distance its OTHER port has to that node in the opposite cycle.
//   place    k_ug_place: per live node the spelling (smaller first oriented k-mer), position and strand; the nodes at position 0 are the
//            starts. rocPRIM sorts the starts by first code = the unitig ids; k_ug_ids / k_ug_assign hand every node its id.
//   emit     k_ug_check validates the layout against the index; rocPRIM sorts the live nodes by (unitig, position), which IS unitig
//            order: k_ug_emit writes offsets, bases, the circular flag and tf along every unitig; tf_sum / min / max come from one
//            reduce-by-key over that array (no atomic on a per-unitig word).
//   graph    section 7 below: the links between unitig ends and the simple bubbles, from a layout and the offsets of its emit.
// What the two compaction levels share is in aix_chains.hpp; the counters holder of a call and the "no end" word are those of the graph
// files, aix_graph.hpp.
// Integer only, no LDS, no grid-wide barrier, no spin-wait. Every index derived from 2 n, from an offset or from the total is 64 bits wide.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "aix_graph.hpp"
#include "aix_probe.hpp"

namespace aix {

static constexpr uint64_t kMask46 = (1ULL << 46) - 1;
static constexpr uint32_t kWNone = 0xFFFFFFF8u;                   // port words from here on: no single live successor; + the out-degree (0, 2, 3, 4)
static constexpr uint32_t kWDead = kWNone + 7u;                   // the node itself is dead
static constexpr uint64_t kFlag = 1ULL << 63;                     // ranking state: nx | (d | terminal flag << 31) << 32
static constexpr uint64_t kCycMark = 1ULL << 63;                  // kid_unitig between k_ug_place and k_ug_assign: this bit + the first code of the circle

struct UgCounters {                                               // one zeroed record per call
    unsigned long long n_live, n_circular, n_starts, bad, max_pos;
    unsigned long long unflagged[66];                             // [0] after k_ug_links, [r] after round r
};

// (block size kCB = four waves = 64 quads per workgroup, grid sizer, AIX_UG_TEST_GRID, wave-reduced counters: aix_chains.hpp)
template <int J>
__device__ __forceinline__ uint32_t ug_quad_bcast(uint32_t v) {   // lane J of the quad to its four lanes (DPP quad_perm [J, J, J, J]); all lanes active
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, J * 0x55, 0xf, 0xf, false);
}

// the oriented k-mer that leaves node `code` through `port`
__device__ __forceinline__ uint64_t ug_orient(uint64_t code, uint32_t port) { return (port & 1u) ? revcomp(code, 23) : code; }

// ---------------------------------------------------------------------------------------------
// 1. ports
// ---------------------------------------------------------------------------------------------
// One quad per (kid, port), 16 per wave, as k_db_neighbours lays its records out. policy: 0 = FilterGauge, 1 = filter always, 2 = never.
__global__ void __launch_bounds__(kCB) k_ug_ports(const IndexDev ix_, uint32_t cutoff, int policy, uint32_t* __restrict__ word) {
    const IndexDev& ix = ix_;
    const uint64_t NP = 2 * ix.n;
    const uint32_t lane = threadIdx.x & 63u, b = lane & 3u;
    FilterGauge fg;
    const uint64_t stride = (uint64_t)gridDim.x * 64;
    for (uint64_t base = (uint64_t)blockIdx.x * 64 + (threadIdx.x >> 6) * 16; base < NP; base += stride) {    // wave-uniform
        const uint64_t p = base + (lane >> 2);
        const bool in = p < NP;
        KeyRec k;
        k.code = 0; k.tf = 0;
        if (in) k = key_at(ix, p >> 1);
        const bool live = in && k.tf > cutoff;
        const uint64_t x = ug_orient(k.code & kMask46, (uint32_t)p);
        const uint64_t y = ((x << 2) | (uint64_t)b) & kMask46;     // next(x, b)
        const bool absence = policy == 1 ? true : (policy == 2 ? false : fg.on);
        const Probe q = slot23_wave(ix, live, y, absence);
        if (policy == 0) fg.seen(live, q.found);
        const bool ylive = live && q.found && q.tf > cutoff && q.slot < ix.n;
        // stored orientation: the successor is entered through its L port and left through R
        const uint32_t ent = 2u * (uint32_t)q.slot + (y <= revcomp(y, 23) ? 1u : 0u);
        const uint32_t l0 = ug_quad_bcast<0>(ylive), l1 = ug_quad_bcast<1>(ylive), l2 = ug_quad_bcast<2>(ylive), l3 = ug_quad_bcast<3>(ylive);
        const uint32_t e0 = ug_quad_bcast<0>(ent), e1 = ug_quad_bcast<1>(ent), e2 = ug_quad_bcast<2>(ent), e3 = ug_quad_bcast<3>(ent);
        const uint32_t deg = l0 + l1 + l2 + l3;
        const uint32_t e = l0 ? e0 : (l1 ? e1 : (l2 ? e2 : e3));
        if (in && b == 0) word[p] = !live ? kWDead : (deg == 1 ? e : kWNone + deg);
    }
}

// ---------------------------------------------------------------------------------------------
// 2. links and 3. ranking
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kCB) k_ug_links(const uint32_t* __restrict__ word, uint64_t NP, uint64_t* __restrict__ st, unsigned long long* __restrict__ unflagged) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    unsigned long long open = 0;
    for (uint64_t p = (uint64_t)blockIdx.x * kCB + threadIdx.x; p < NP; p += stride) {
        const uint32_t t = word[p];
        bool linked = false;
        if (t < kWNone && (uint64_t)t < NP) linked = (uint64_t)word[t] == p && (t >> 1) != (uint32_t)(p >> 1);
        st[p] = linked ? ((uint64_t)(t ^ 1u) | (1ULL << 32)) : (p | kFlag);
        open += linked;
    }
    count_add(open, unflagged);
}

__global__ void __launch_bounds__(kCB) k_ug_jump(const uint64_t* __restrict__ in, uint64_t NP, uint64_t* __restrict__ out, unsigned long long* __restrict__ unflagged) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    unsigned long long open = 0;
    for (uint64_t p = (uint64_t)blockIdx.x * kCB + threadIdx.x; p < NP; p += stride) {
        uint64_t s = in[p];
        if (!(s & kFlag)) {
            const uint64_t q = in[(uint32_t)s];
            // on a cycle d doubles every round and means nothing: it is kept below the flag bit
            const uint64_t d = (((s >> 32) & 0x7FFFFFFFu) + ((q >> 32) & 0x7FFFFFFFu)) & 0x7FFFFFFFu;
            s = (q & (kFlag | 0xFFFFFFFFull)) | (d << 32);
            open += !(s & kFlag);
        }
        out[p] = s;
    }
    count_add(open, unflagged);
}

// ---------------------------------------------------------------------------------------------
// 4. cycles: state a = nx | md << 32 and key = stored code << 1 | port bit, for the unflagged ports only
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kCB) k_ug_cyc_init(const IndexDev ix_, const uint64_t* __restrict__ rank, const uint32_t* __restrict__ word, uint64_t NP,
                                                    uint64_t* __restrict__ a, uint64_t* __restrict__ key) {
    const IndexDev& ix = ix_;
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t p = (uint64_t)blockIdx.x * kCB + threadIdx.x; p < NP; p += stride) {
        if (rank[p] & kFlag) continue;
        a[p] = (uint64_t)(word[p] ^ 1u);                           // an unflagged port is linked: its word is its link
        key[p] = ((key_at(ix, p >> 1).code & kMask46) << 1) | (p & 1);
    }
}

__global__ void __launch_bounds__(kCB) k_ug_cyc_jump(const uint64_t* __restrict__ rank, uint64_t NP, uint64_t span, const uint64_t* __restrict__ a_in,
                                                    const uint64_t* __restrict__ k_in, uint64_t* __restrict__ a_out, uint64_t* __restrict__ k_out) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t p = (uint64_t)blockIdx.x * kCB + threadIdx.x; p < NP; p += stride) {
        if (rank[p] & kFlag) continue;
        const uint64_t a = a_in[p];
        uint64_t k = k_in[p], md = a >> 32;
        const uint32_t q = (uint32_t)a;
        const uint64_t aq = a_in[q], kq = k_in[q];
        if (kq < k) { k = kq; md = span + (aq >> 32); }            // strictly smaller: the first occurrence stays. md < the cycle's length
        a_out[p] = (aq & 0xFFFFFFFFull) | (md << 32);
        k_out[p] = k;
    }
}

// ---------------------------------------------------------------------------------------------
// 5. layout
// ---------------------------------------------------------------------------------------------
// Per kid. Path node: both ports are flagged; spelling A starts at the end reached through L (this node: position dL, stored orientation),
// spelling B at the end reached through R (position dR, reversed); the first oriented k-mer of a spelling leaves its end node through the
// port opposite the unlinked one. Circle node: neither port is flagged. kid_unitig holds, until k_ug_assign, the start's kid (path) or
// kCycMark | first code (circle); a start appends (first code, kid).
__global__ void __launch_bounds__(kCB) k_ug_place(const IndexDev ix_, uint32_t cutoff, const uint64_t* __restrict__ rank, const uint64_t* __restrict__ cyc_a,
                                                 const uint64_t* __restrict__ cyc_k, uint64_t* __restrict__ kid_unitig, uint32_t* __restrict__ kid_pos,
                                                 uint8_t* __restrict__ kid_flag, uint64_t* __restrict__ start_code, uint32_t* __restrict__ start_kid,
                                                 UgCounters* __restrict__ ctr) {
    const IndexDev& ix = ix_;
    const uint64_t n = ix.n, stride = (uint64_t)gridDim.x * kCB;
    unsigned long long live = 0, circ = 0;
    for (uint64_t kid = (uint64_t)blockIdx.x * kCB + threadIdx.x; kid < n; kid += stride) {
        const KeyRec me = key_at(ix, kid);
        if (!(me.tf > cutoff)) {
            kid_unitig[kid] = AIX_UNITIG_NONE; kid_pos[kid] = 0; kid_flag[kid] = 0;
            continue;
        }
        ++live;
        const uint64_t sR = rank[2 * kid], sL = rank[2 * kid + 1];
        uint32_t pos, flag;
        uint64_t first, tmp;
        if ((sR & kFlag) || (sL & kFlag) || !cyc_a) {
            const uint32_t eR = (uint32_t)sR, eL = (uint32_t)sL;
            const uint32_t dR = (uint32_t)(sR >> 32) & 0x7FFFFFFFu, dL = (uint32_t)(sL >> 32) & 0x7FFFFFFFu;
            const uint64_t fa = ug_orient(key_at(ix, eL >> 1).code & kMask46, eL ^ 1u);
            const uint64_t fb = ug_orient(key_at(ix, eR >> 1).code & kMask46, eR ^ 1u);
            const bool A = fa < fb;                                // one node: stored code against its reverse complement
            pos = A ? dL : dR;
            flag = A ? 0u : 1u;
            first = A ? fa : fb;
            tmp = (uint64_t)((A ? eL : eR) >> 1);
        } else {
            const uint64_t kR = cyc_k[2 * kid];
            const bool keepR = (kR & 1) == 0;                      // this node's R port lies on the kept directed cycle
            pos = (uint32_t)(cyc_a[2 * kid + (keepR ? 1 : 0)] >> 32);
            flag = (keepR ? 0u : 1u) | 2u;
            first = kR >> 1;
            tmp = kCycMark | first;
            if (pos == 0) ++circ;
        }
        kid_pos[kid] = pos;
        kid_flag[kid] = (uint8_t)flag;
        if (pos == 0) {
            const unsigned long long j = atomicAdd(&ctr->n_starts, 1ull);
            if (j < n) { start_code[j] = first; start_kid[j] = (uint32_t)kid; }
        } else {
            kid_unitig[kid] = tmp;
        }
    }
    count_add(live, &ctr->n_live);
    count_add(circ, &ctr->n_circular);
}

__global__ void __launch_bounds__(kCB) k_ug_ids(const uint32_t* __restrict__ sorted_kid, uint64_t U, uint64_t n, uint64_t* __restrict__ kid_unitig) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t j = (uint64_t)blockIdx.x * kCB + threadIdx.x; j < U; j += stride) {
        const uint32_t kid = sorted_kid[j];
        if (kid < n) kid_unitig[kid] = j;
    }
}

// every live node that is not a start reads its id at its start (starts are not written here)
__global__ void __launch_bounds__(kCB) k_ug_assign(const uint64_t* __restrict__ sorted_code, uint64_t U, uint64_t n, const uint32_t* __restrict__ kid_pos,
                                                  uint64_t* __restrict__ kid_unitig) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t kid = (uint64_t)blockIdx.x * kCB + threadIdx.x; kid < n; kid += stride) {
        if (kid_pos[kid] == 0) continue;                           // dead, or a start
        const uint64_t t = kid_unitig[kid];
        uint64_t id;
        if (t & kCycMark) {                                        // a circle knows its first code, not its start's kid: lower bound in the sorted codes
            const uint64_t code = t & kMask46;
            uint64_t lo = 0, hi = U;
            while (lo < hi) {                                      // at most 64 trips
                const uint64_t mid = lo + ((hi - lo) >> 1);
                if (sorted_code[mid] < code) lo = mid + 1; else hi = mid;
            }
            id = lo;
        } else {
            id = t < n ? kid_unitig[t] : AIX_UNITIG_NONE;
        }
        kid_unitig[kid] = id;
    }
}

// ---------------------------------------------------------------------------------------------
// 6. emit
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kCB) k_ug_check(const IndexDev ix_, uint32_t cutoff, uint64_t U, const uint64_t* __restrict__ kid_unitig,
                                                 const uint32_t* __restrict__ kid_pos, UgCounters* __restrict__ ctr) {
    const IndexDev& ix = ix_;
    const uint64_t n = ix.n, stride = (uint64_t)gridDim.x * kCB;
    unsigned long long live = 0, starts = 0, bad = 0, mx = 0;
    for (uint64_t kid = (uint64_t)blockIdx.x * kCB + threadIdx.x; kid < n; kid += stride) {
        const uint64_t u = kid_unitig[kid];
        if (u == AIX_UNITIG_NONE) continue;
        const uint32_t pos = kid_pos[kid];
        ++live;
        starts += pos == 0;
        bad += u >= U || !(key_at(ix, kid).tf > cutoff);
        mx = pos > mx ? pos : mx;
    }
    count_add(live, &ctr->n_live);
    count_add(starts, &ctr->n_starts);
    count_add(bad, &ctr->bad);
    count_max(mx, &ctr->max_pos);
}

// sort key of a node: unitig << pos_bits | position; dead nodes behind everything
__global__ void __launch_bounds__(kCB) k_ug_keys(uint64_t n, uint64_t U, int pos_bits, const uint64_t* __restrict__ kid_unitig, const uint32_t* __restrict__ kid_pos,
                                                uint64_t* __restrict__ keys, uint32_t* __restrict__ kids) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t kid = (uint64_t)blockIdx.x * kCB + threadIdx.x; kid < n; kid += stride) {
        const uint64_t u = kid_unitig[kid];
        keys[kid] = u == AIX_UNITIG_NONE ? U << pos_bits : ((u << pos_bits) | kid_pos[kid]);
        kids[kid] = (uint32_t)kid;
    }
}

// Entry j of the sorted nodes is k-mer j in unitig order: its unitig's k-mers start at j - pos, its bases at j - pos + 22 u.
__global__ void __launch_bounds__(kCB) k_ug_emit(const IndexDev ix_, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ kids, uint64_t n_live, uint64_t U,
                                                int pos_bits, const uint8_t* __restrict__ kid_flag, uint64_t total, uint64_t* __restrict__ offsets,
                                                uint8_t* __restrict__ bases, uint8_t* __restrict__ circular, uint32_t* __restrict__ tf_out) {
    const IndexDev& ix = ix_;
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t j = (uint64_t)blockIdx.x * kCB + threadIdx.x; j < n_live; j += stride) {
        const uint64_t key = keys[j], u = key >> pos_bits, pos = key & ((1ULL << pos_bits) - 1);
        const uint32_t kid = kids[j];
        if (u >= U || pos > j || kid >= ix.n) continue;            // (a layout that k_ug_check accepted never gets here)
        const KeyRec rec = key_at(ix, kid);
        const uint32_t flag = kid_flag[kid];
        tf_out[j] = rec.tf;
        const uint64_t x = ug_orient(rec.code & kMask46, flag);
        const uint64_t at = j + 22 * u;                            // the k-mer occupies bases [at, at + 23)
        if (pos == 0) {
            offsets[u] = at;
            circular[u] = (uint8_t)((flag >> 1) & 1u);
            uint64_t w[3];
            ascii23_of_rc(revcomp(x, 23), w[0], w[1], w[2]);
            for (uint32_t c = 0; c < 23; ++c)
                if (at + c < total) bases[at + c] = (uint8_t)(w[c >> 3] >> (8 * (c & 7)));
        } else if (at + 22 < total) {
            bases[at + 22] = (uint8_t)(AIX_LUT_ACGT >> (8 * (uint32_t)(x & 3)));
        }
        if (j == 0) offsets[U] = total;
    }
}

struct UgToAgg {                                                  // (the aggregate, its reduction and k_chain_stats: aix_chains.hpp)
    __host__ __device__ ChainAgg operator()(uint32_t t) const { return ChainAgg{t, t, t}; }
};

// AIX_DBJ_FILTER (A/B switch): the policy of the walks (aix_debruijn.hip), whose probes these are: found keys nearly always
static inline int ug_policy() { return (int)env_int("AIX_DBJ_FILTER", 0, 2, 2); }

// Outputs of the layout call. Synchronises `s`.
static hipError_t ug_layout(const aix_index* h, uint32_t cutoff, uint64_t* kid_unitig, uint32_t* kid_pos, uint8_t* kid_flag, uint64_t out[4], hipStream_t s) {
    const IndexDev ix = h->dev();
    const uint64_t n = ix.n, NP = 2 * n, cap = chain_test_grid();
    const dim3 blk(kCB);
    Counted<UgCounters> ctr(s);
    DevArr word(s), r0(s), r1(s), ca0(s), ck0(s), ca1(s), ck1(s), sc(s), sk(s), sc2(s), sk2(s), tmp(s);
    AIX_TRY(ctr.init());
    AIX_TRY(word.alloc(4 * NP));
    AIX_TRY(r0.alloc(8 * NP));
    AIX_TRY(r1.alloc(8 * NP));
    const UgCounters& hc = ctr.host;
    AIX_TRY(ctr.run([&]() {
        AIX_TRY_LAUNCH(k_ug_ports, dim3((unsigned)std::min<uint64_t>((NP + 63) / 64, cap)), blk, 0, s, ix, cutoff, ug_policy(), (uint32_t*)word.p);
        AIX_TRY_LAUNCH(k_ug_links, dim3(chain_grid(NP, 4 * kCB, cap)), blk, 0, s, (const uint32_t*)word.p, NP, (uint64_t*)r0.p, &ctr.dev()->unflagged[0]);
        return hipSuccess;
    }));
    uint64_t *cur = (uint64_t*)r0.p, *oth = (uint64_t*)r1.p;
    uint64_t open = hc.unflagged[0];
    AIX_TRY(chain_rank(n, ctr.dev()->unflagged, &open, s, [&](int r) {
        AIX_TRY_LAUNCH(k_ug_jump, dim3(chain_grid(NP, 4 * kCB, cap)), blk, 0, s, (const uint64_t*)cur, NP, oth, &ctr.dev()->unflagged[r]);
        std::swap(cur, oth);
        return hipSuccess;
    }));                                                           // open: only cycle ports are left
    (oth == (uint64_t*)r0.p ? r0 : r1).drop();
    const uint64_t *cyc_a = nullptr, *cyc_k = nullptr;
    if (open) {
        AIX_TRY(ca0.alloc(8 * NP));
        AIX_TRY(ck0.alloc(8 * NP));
        AIX_TRY(ca1.alloc(8 * NP));
        AIX_TRY(ck1.alloc(8 * NP));
        uint64_t *a = (uint64_t*)ca0.p, *k = (uint64_t*)ck0.p, *a2 = (uint64_t*)ca1.p, *k2 = (uint64_t*)ck1.p;
        AIX_TRY_LAUNCH(k_ug_cyc_init, dim3(chain_grid(NP, 4 * kCB, cap)), blk, 0, s, ix, (const uint64_t*)cur, (const uint32_t*)word.p, NP, a, k);
        const int rounds = std::min(64, ceil_log2(open) + 1);
        for (int r = 1; r <= rounds; ++r) {
            AIX_TRY_LAUNCH(k_ug_cyc_jump, dim3(chain_grid(NP, 4 * kCB, cap)), blk, 0, s, (const uint64_t*)cur, NP, r <= 63 ? 1ULL << (r - 1) : 0ULL, (const uint64_t*)a,
                (const uint64_t*)k, a2, k2);
            std::swap(a, a2);
            std::swap(k, k2);
        }
        cyc_a = a; cyc_k = k;
        AIX_TRY(hipStreamSynchronize(s));
        (a2 == (uint64_t*)ca0.p ? ca0 : ca1).drop();
        (k2 == (uint64_t*)ck0.p ? ck0 : ck1).drop();
    }
    word.drop();
    AIX_TRY(sc.alloc(8 * n));
    AIX_TRY(sk.alloc(4 * n));
    AIX_TRY_LAUNCH(k_ug_place, dim3(chain_grid(n, 2 * kCB, cap)), blk, 0, s, ix, cutoff, (const uint64_t*)cur, cyc_a, cyc_k, kid_unitig, kid_pos, kid_flag, (uint64_t*)sc.p,
        (uint32_t*)sk.p, ctr.dev());                              // (on top of the counters of the ranking: no run())
    AIX_TRY(chain_read(&ctr.host, ctr.dev(), s));
    const uint64_t U = std::min<uint64_t>(hc.n_starts, n);
    if (U) {
        AIX_TRY(sc2.alloc(8 * U));
        AIX_TRY(sk2.alloc(4 * U));
        AIX_TRY(sort_pairs((const uint64_t*)sc.p, (uint64_t*)sc2.p, (const uint32_t*)sk.p, (uint32_t*)sk2.p, U, 46u, tmp, s));
        AIX_TRY_LAUNCH(k_ug_ids, dim3(chain_grid(U, 4 * kCB, cap)), blk, 0, s, (const uint32_t*)sk2.p, U, n, kid_unitig);
        AIX_TRY_LAUNCH(k_ug_assign, dim3(chain_grid(n, 4 * kCB, cap)), blk, 0, s, (const uint64_t*)sc2.p, U, n, (const uint32_t*)kid_pos, kid_unitig);
    }
    out[0] = U;
    out[1] = hc.n_live + 22 * U;
    out[2] = hc.n_live;
    out[3] = hc.n_circular;
    return hipStreamSynchronize(s);
}

// *bad: the layout does not belong to (index, cutoff, U); nothing was written then. Synchronises `s`.
static hipError_t ug_emit(const aix_index* h, uint32_t cutoff, const uint64_t* kid_unitig, const uint32_t* kid_pos, const uint8_t* kid_flag, uint64_t U,
                          uint64_t* offsets, uint8_t* bases, uint8_t* circular, uint64_t* tf_sum, uint32_t* tf_min, uint32_t* tf_max, uint32_t* kmer_tf, bool* bad,
                          hipStream_t s) {
    const IndexDev ix = h->dev();
    const uint64_t n = ix.n, cap = chain_test_grid();
    const dim3 blk(kCB);
    *bad = false;
    Counted<UgCounters> ctr(s);
    DevArr keys(s), kids(s), keys2(s), kids2(s), tmp(s), tfs(s), uniq(s), agg(s), cnt(s), tmp2(s);
    AIX_TRY(ctr.init());
    const UgCounters& hc = ctr.host;
    AIX_TRY(ctr.run([&]() {
        AIX_TRY_LAUNCH(k_ug_check, dim3(chain_grid(n, 2 * kCB, cap)), blk, 0, s, ix, cutoff, U, kid_unitig, kid_pos, ctr.dev());
        return hipSuccess;
    }));
    if (hc.bad || hc.n_starts != U || hc.n_live < U || (U == 0 && hc.n_live)) { *bad = true; return hipSuccess; }
    const uint64_t n_live = hc.n_live, total = n_live + 22 * U;
    if (U == 0) {
        AIX_TRY(hipMemsetAsync(offsets, 0, 8, s));
        return hipStreamSynchronize(s);
    }
    const int pos_bits = bit_length(hc.max_pos), end_bit = pos_bits + bit_length(U);
    AIX_TRY(keys.alloc(8 * n));
    AIX_TRY(kids.alloc(4 * n));
    AIX_TRY(keys2.alloc(8 * n));
    AIX_TRY(kids2.alloc(4 * n));
    AIX_TRY_LAUNCH(k_ug_keys, dim3(chain_grid(n, 4 * kCB, cap)), blk, 0, s, n, U, pos_bits, kid_unitig, kid_pos, (uint64_t*)keys.p, (uint32_t*)kids.p);
    AIX_TRY(sort_pairs((const uint64_t*)keys.p, (uint64_t*)keys2.p, (const uint32_t*)kids.p, (uint32_t*)kids2.p, n, (unsigned)end_bit, tmp, s));
    AIX_TRY(hipStreamSynchronize(s));
    keys.drop();
    kids.drop();
    uint32_t* tf_seq = kmer_tf;
    if (!tf_seq) {
        AIX_TRY(tfs.alloc(4 * n_live));
        tf_seq = (uint32_t*)tfs.p;
    }
    AIX_TRY_LAUNCH(k_ug_emit, dim3(chain_grid(n_live, 2 * kCB, cap)), blk, 0, s, ix, (const uint64_t*)keys2.p, (const uint32_t*)kids2.p, n_live, U, pos_bits, kid_flag, total,
        offsets, bases, circular, tf_seq);
    AIX_TRY(uniq.alloc(8 * U));
    AIX_TRY(agg.alloc(sizeof(ChainAgg) * U));
    AIX_TRY(cnt.alloc(8));
    auto kin = rocprim::make_transform_iterator((const uint64_t*)keys2.p, ChainUnitOf{pos_bits});
    auto vin = rocprim::make_transform_iterator((const uint32_t*)tf_seq, UgToAgg());
    AIX_TRY(with_temp(tmp2, [&](void* t, size_t& tb) {
        return rocprim::reduce_by_key(t, tb, kin, vin, (size_t)n_live, (uint64_t*)uniq.p, (ChainAgg*)agg.p, (uint64_t*)cnt.p, ChainAggOp(), rocprim::equal_to<uint64_t>(), s);
    }));
    AIX_TRY_LAUNCH(k_chain_stats<ChainAgg>, dim3(chain_grid(U, 4 * kCB, cap)), blk, 0, s, (const uint64_t*)uniq.p, (const ChainAgg*)agg.p, (const uint64_t*)cnt.p, U, tf_sum,
                   tf_min, tf_max);
    return hipStreamSynchronize(s);
}

// ---------------------------------------------------------------------------------------------
// 7. the unitig graph: links between unitig ends, simple bubbles (the contract is the block below the compaction's in aindex_hip.h)
// ---------------------------------------------------------------------------------------------
// End 2 u + 0 leaves the spelling of linear unitig u through its last oriented k-mer, end 2 u + 1 through rc of its first. The chain:
//   ends     k_ul_ends: one lane per kid; the member at position 0 / m - 1 of a linear unitig is the kid of end 2 u + 1 / 2 u + 0
//   probe    k_ul_probe: one quad per end, laid out as k_ug_ports; a live successor y at slot s gives the word 2 kid_unitig[s] + r, and must sit
//            at position 0 (r = 0) or m - 1 (r = 1) of a linear unitig; the quad's words are compacted in base order: cand[4 e ..], deg[e]
//   scan     rocPRIM exclusive scan of deg[2 U + 1] (the last is 0) = link_off; link_off[2 U] = E
//   fill     k_ul_fill: one lane per end copies its words to link_to + link_off[e]
//   bubbles  k_ul_bubbles: one lane per unitig, the chain of gathers of the bubble rule over link_off / link_to; no handle
// (kNoEnd, aix_graph.hpp, is here the end_kid of an end that does not exist (circular unitig), a cand without a word and the bubble_mate of a unitig without one)

struct UlCounters {                                               // one zeroed record per call
    unsigned long long bad, n_ends, n_circular, n_none;
};

__global__ void __launch_bounds__(kCB) k_ul_ends(uint64_t n, uint64_t U, const uint64_t* __restrict__ kid_unitig, const uint32_t* __restrict__ kid_pos,
                                                const uint8_t* __restrict__ kid_flag, const uint64_t* __restrict__ offsets, uint32_t* __restrict__ end_kid,
                                                UlCounters* __restrict__ ctr) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    unsigned long long bad = 0, ends = 0, circ = 0;
    for (uint64_t kid = (uint64_t)blockIdx.x * kCB + threadIdx.x; kid < n; kid += stride) {
        const uint64_t u = kid_unitig[kid];
        if (u == AIX_UNITIG_NONE) continue;
        if (u >= U) { ++bad; continue; }
        const uint64_t lo = offsets[u], hi = offsets[u + 1];
        const uint64_t pos = kid_pos[kid];
        if (hi < lo + 23 || pos >= hi - lo - 22) { ++bad; continue; }
        const uint64_t m = hi - lo - 22;
        if (kid_flag[kid] & 2u) { circ += pos == 0; continue; }
        if (pos == 0) { end_kid[2 * u + 1] = (uint32_t)kid; ++ends; }
        if (pos == m - 1) { end_kid[2 * u] = (uint32_t)kid; ++ends; }
    }
    count_add(bad, &ctr->bad);
    count_add(ends, &ctr->n_ends);
    count_add(circ, &ctr->n_circular);
}

// One quad per end, 16 per wave. policy as k_ug_ports. cand[4 e + j] = the j-th link word of end e in base order (kNoEnd behind the degree).
__global__ void __launch_bounds__(kCB) k_ul_probe(const IndexDev ix_, uint32_t cutoff, int policy, uint64_t U, const uint64_t* __restrict__ kid_unitig,
                                                 const uint32_t* __restrict__ kid_pos, const uint8_t* __restrict__ kid_flag, const uint64_t* __restrict__ offsets,
                                                 const uint32_t* __restrict__ end_kid, uint32_t* __restrict__ cand, uint32_t* __restrict__ deg,
                                                 UlCounters* __restrict__ ctr) {
    const IndexDev& ix = ix_;
    const uint64_t NE = 2 * U;
    const uint32_t lane = threadIdx.x & 63u, b = lane & 3u;
    FilterGauge fg;
    unsigned long long bad = 0, none = 0;
    const uint64_t stride = (uint64_t)gridDim.x * 64;
    for (uint64_t base = (uint64_t)blockIdx.x * 64 + (threadIdx.x >> 6) * 16; base < NE; base += stride) {    // wave-uniform
        const uint64_t e = base + (lane >> 2);
        const bool in = e < NE;
        const uint32_t kid = in ? end_kid[e] : kNoEnd;
        const bool has = in && (uint64_t)kid < ix.n;
        none += in && b == 0 && kid == kNoEnd;
        bad += in && b == 0 && kid != kNoEnd && !has;
        KeyRec k;
        k.code = 0; k.tf = 0;
        uint32_t f = 0;
        if (has) { k = key_at(ix, kid); f = kid_flag[kid]; }
        const bool live = has && k.tf > cutoff;
        const uint64_t x = ug_orient(k.code & kMask46, (f ^ (uint32_t)e) & 1u);
        const uint64_t y = ((x << 2) | (uint64_t)b) & kMask46;     // next(x, b)
        const bool absence = policy == 1 ? true : (policy == 2 ? false : fg.on);
        const Probe q = slot23_wave(ix, live, y, absence);
        if (policy == 0) fg.seen(live, q.found);
        bool ylive = live && q.found && q.tf > cutoff && q.slot < ix.n;
        uint32_t w = kNoEnd;
        if (ylive) {
            const uint64_t v = kid_unitig[q.slot];
            if (v < U) {
                const uint32_t fv = kid_flag[q.slot];
                const uint64_t pos = kid_pos[q.slot], lo = offsets[v], hi = offsets[v + 1];
                const uint32_t r = (y <= revcomp(y, 23) ? 0u : 1u) ^ (fv & 1u);
                // a successor of an end is the first k-mer of a linear unitig in the entering orientation
                const bool ok = !(fv & 2u) && hi >= lo + 23 && (r ? pos + 1 == hi - lo - 22 : pos == 0);
                w = 2u * (uint32_t)v + r;
                bad += !ok;
            } else {
                ++bad;
                ylive = false;
            }
        }
        const uint32_t l0 = ug_quad_bcast<0>(ylive), l1 = ug_quad_bcast<1>(ylive), l2 = ug_quad_bcast<2>(ylive), l3 = ug_quad_bcast<3>(ylive);
        const uint32_t w0 = ug_quad_bcast<0>(w), w1 = ug_quad_bcast<1>(w), w2 = ug_quad_bcast<2>(w), w3 = ug_quad_bcast<3>(w);
        const uint32_t p1 = l0, p2 = l0 + l1, p3 = p2 + l2, d = p3 + l3;
        uint32_t c[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j)
            c[j] = (l0 && j == 0) ? w0 : ((l1 && p1 == j) ? w1 : ((l2 && p2 == j) ? w2 : ((l3 && p3 == j) ? w3 : kNoEnd)));
        if (in && b == 0) {
            *reinterpret_cast<uint4*>(cand + 4 * e) = make_uint4(c[0], c[1], c[2], c[3]);
            deg[e] = d;
        }
    }
    count_add(bad, &ctr->bad);
    count_add(none, &ctr->n_none);
}

__global__ void __launch_bounds__(kCB) k_ul_fill(uint64_t NE, const uint64_t* __restrict__ link_off, const uint32_t* __restrict__ cand, uint64_t E,
                                                uint32_t* __restrict__ link_to) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t e = (uint64_t)blockIdx.x * kCB + threadIdx.x; e < NE; e += stride) {
        const uint64_t o = link_off[e], o1 = link_off[e + 1];
        const uint4 c4 = *reinterpret_cast<const uint4*>(cand + 4 * e);
        const uint32_t c[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j)
            if (o + j < o1 && o + j < E) link_to[o + j] = c[j];
    }
}

// degree and first target of end e; e < NE is the caller's business, every other index is checked here. A degree above 4 reads as 5.
__device__ __forceinline__ uint32_t ul_deg(const uint64_t* __restrict__ link_off, uint64_t E, uint64_t e, uint64_t& at) {
    at = link_off[e];
    const uint64_t hi = link_off[e + 1];
    if (hi < at || hi > E) return 5u;
    return hi - at > 4 ? 5u : (uint32_t)(hi - at);
}

__global__ void __launch_bounds__(kCB) k_ul_bubbles(uint64_t U, const uint64_t* __restrict__ link_off, const uint32_t* __restrict__ link_to, uint64_t E,
                                                   uint32_t* __restrict__ mate) {
    const uint64_t NE = 2 * U, stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t u = (uint64_t)blockIdx.x * kCB + threadIdx.x; u < U; u += stride) {
        uint32_t res = kNoEnd;
        uint64_t aR, aL, aF, aS, aX, aY;
        do {
            if (ul_deg(link_off, E, 2 * u, aR) != 1 || ul_deg(link_off, E, 2 * u + 1, aL) != 1) break;
            const uint64_t tR = link_to[aR], tL = link_to[aL];
            if (tR >= NE || tL >= NE) break;
            if (ul_deg(link_off, E, tL ^ 1, aF) != 2) break;       // the source end
            const uint64_t t0 = link_to[aF], t1 = link_to[aF + 1];
            if (t0 != 2 * u && t1 != 2 * u) break;
            const uint64_t x = t0 == 2 * u ? t1 : t0;
            if (x >= NE || (x >> 1) == u) break;
            if (ul_deg(link_off, E, tR ^ 1, aS) != 2) break;       // the sink: in-degree 2
            if (ul_deg(link_off, E, x, aX) != 1 || link_to[aX] != tR) break;
            if (ul_deg(link_off, E, x ^ 1, aY) != 1 || link_to[aY] != tL) break;
            res = (uint32_t)(x >> 1);
        } while (false);
        mate[u] = res;
    }
}

// *bad: the layout or the offsets do not belong to (index, cutoff, U), nothing was written then; *E is set once link_off is written: if it is
// above link_cap, link_to is untouched. Synchronises `s`.
static hipError_t ul_links(const aix_index* h, uint32_t cutoff, const uint64_t* kid_unitig, const uint32_t* kid_pos, const uint8_t* kid_flag, uint64_t U,
                           const uint64_t* offsets, uint64_t* link_off, uint32_t* link_to, uint64_t link_cap, uint64_t* E_out, bool* bad, hipStream_t s) {
    const IndexDev ix = h->dev();
    const uint64_t n = ix.n, NE = 2 * U, cap = chain_test_grid();
    const dim3 blk(kCB);
    *bad = false;
    Counted<UgCounters> ctr(s);
    DevArr lc_a(s), ek(s), cand(s), deg(s), tmp(s);
    AIX_TRY(ctr.init());
    AIX_TRY(lc_a.alloc(sizeof(UlCounters)));
    UlCounters* lc = (UlCounters*)lc_a.p;                          // zeroed once, read after each of its two kernels: no run()
    const UgCounters& hc = ctr.host;
    UlCounters hl;
    AIX_TRY(ctr.run([&]() {
        AIX_TRY(hipMemsetAsync(lc, 0, sizeof(UlCounters), s));
        AIX_TRY_LAUNCH(k_ug_check, dim3(chain_grid(n, 2 * kCB, cap)), blk, 0, s, ix, cutoff, U, kid_unitig, kid_pos, ctr.dev());
        return hipSuccess;
    }));
    if (hc.bad || hc.n_starts != U || hc.n_live < U || (U == 0 && hc.n_live)) { *bad = true; return hipSuccess; }
    if (U == 0) {
        AIX_TRY(hipMemsetAsync(link_off, 0, 8, s));
        *E_out = 0;
        return hipStreamSynchronize(s);
    }
    AIX_TRY(ek.alloc(4 * NE));
    AIX_TRY(hipMemsetAsync(ek.p, 0xFF, 4 * NE, s));
    AIX_TRY_LAUNCH(k_ul_ends, dim3(chain_grid(n, 4 * kCB, cap)), blk, 0, s, n, U, kid_unitig, kid_pos, kid_flag, offsets, (uint32_t*)ek.p, lc);
    AIX_TRY(hipMemcpyAsync(&hl, lc, sizeof(UlCounters), hipMemcpyDeviceToHost, s));
    AIX_TRY(hipStreamSynchronize(s));
    if (hl.bad || hl.n_circular > U || hl.n_ends != 2 * (U - hl.n_circular)) { *bad = true; return hipSuccess; }
    const uint64_t n_circular = hl.n_circular;
    AIX_TRY(cand.alloc(16 * NE));
    AIX_TRY(deg.alloc(4 * (NE + 1)));
    AIX_TRY(hipMemsetAsync((uint32_t*)deg.p + NE, 0, 4, s));
    AIX_TRY_LAUNCH(k_ul_probe, dim3(chain_grid(NE, 2 * 64, cap)), blk, 0, s, ix, cutoff, ug_policy(), U, kid_unitig, kid_pos, kid_flag, offsets, (const uint32_t*)ek.p,
        (uint32_t*)cand.p, (uint32_t*)deg.p, lc);
    AIX_TRY(hipMemcpyAsync(&hl, lc, sizeof(UlCounters), hipMemcpyDeviceToHost, s));
    AIX_TRY(hipStreamSynchronize(s));
    // every written end was written once: 2 (U - circular) writes, and exactly the two ends of every circular unitig are empty
    if (hl.bad || hl.n_none != 2 * n_circular) { *bad = true; return hipSuccess; }
    ek.drop();
    AIX_TRY(scan_u64(rocprim::make_transform_iterator((const uint32_t*)deg.p, Widen<uint32_t>()), link_off, NE + 1, tmp, s));
    uint64_t E = 0;
    AIX_TRY(hipMemcpyAsync(&E, link_off + NE, 8, hipMemcpyDeviceToHost, s));
    AIX_TRY(hipStreamSynchronize(s));
    *E_out = E;
    if (E > link_cap || E == 0) return hipSuccess;
    AIX_TRY_LAUNCH(k_ul_fill, dim3(chain_grid(NE, 4 * kCB, cap)), blk, 0, s, NE, (const uint64_t*)link_off, (const uint32_t*)cand.p, E, link_to);
    return hipStreamSynchronize(s);
}

}  // namespace aix

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
// the refusals every entry point shares, decided before anything is allocated or launched
static int ug_check_handle(const aix_index_t* h) {
    if (!h) return AIX_ERR_ARG;
    if (h->k != 23) return AIX_ERR_MODE;
    if (!h->canonical_only) return AIX_ERR_UNSUPPORTED;          // freq(x) != freq(rc x): the graph is not strand-symmetric
    if (h->n == 0) return AIX_ERR_UNSUPPORTED;
    if (2 * h->n > (uint64_t)kWNone) return AIX_ERR_UNSUPPORTED;  // a port (2 kid + port) must fit its u32 word below the codes
    return AIX_OK;
}

extern "C" int aix_unitigs_layout_dev(aix_index_t* h, uint32_t cutoff, uint64_t* d_kid_unitig, uint32_t* d_kid_pos, uint8_t* d_kid_flag, uint64_t* n_unitigs_out,
                                      uint64_t* total_bases_out, uint64_t* n_live_out, uint64_t* n_circular_out, void* stream) {
    const int st = ug_check_handle(h);
    if (st) return st;
    if (!d_kid_unitig || !d_kid_pos || !d_kid_flag || !n_unitigs_out || !total_bases_out || !n_live_out || !n_circular_out) return AIX_ERR_ARG;
    DevGuard g(h->device);
    uint64_t out[4] = {0, 0, 0, 0};
    AIXCHK(ug_layout(h, cutoff, d_kid_unitig, d_kid_pos, d_kid_flag, out, (hipStream_t)stream));
    *n_unitigs_out = out[0]; *total_bases_out = out[1]; *n_live_out = out[2]; *n_circular_out = out[3];
    return AIX_OK;
}

extern "C" int aix_unitigs_emit_dev(aix_index_t* h, uint32_t cutoff, const uint64_t* d_kid_unitig, const uint32_t* d_kid_pos, const uint8_t* d_kid_flag, uint64_t U,
                                    uint64_t* d_offsets, uint8_t* d_bases, uint8_t* d_circular, uint64_t* d_tf_sum, uint32_t* d_tf_min, uint32_t* d_tf_max,
                                    uint32_t* d_kmer_tf, void* stream) {
    const int st = ug_check_handle(h);
    if (st) return st;
    if (!d_kid_unitig || !d_kid_pos || !d_kid_flag || !d_offsets) return AIX_ERR_ARG;
    if (U && (!d_bases || !d_circular || !d_tf_sum || !d_tf_min || !d_tf_max)) return AIX_ERR_ARG;
    if (U > h->n) return AIX_ERR_ARG;
    DevGuard g(h->device);
    bool bad = false;
    AIXCHK(ug_emit(h, cutoff, d_kid_unitig, d_kid_pos, d_kid_flag, U, d_offsets, d_bases, d_circular, d_tf_sum, d_tf_min, d_tf_max, d_kmer_tf, &bad,
                  (hipStream_t)stream));
    return bad ? AIX_ERR_ARG : AIX_OK;
}

extern "C" int aix_unitigs(aix_index_t* h, uint32_t cutoff, uint64_t* n_unitigs_out, uint64_t** offsets_out, uint8_t** bases_out, uint8_t** circular_out,
                           uint64_t** tf_sum_out, uint32_t** tf_min_out, uint32_t** tf_max_out, uint32_t** kmer_tf_out, uint64_t** kid_unitig_out,
                           uint32_t** kid_pos_out, uint8_t** kid_flag_out) {
    const int st = ug_check_handle(h);
    if (st) return st;
    if (!n_unitigs_out || !offsets_out || !bases_out || !circular_out || !tf_sum_out || !tf_min_out || !tf_max_out) return AIX_ERR_ARG;
    DevGuard g(h->device);
    const uint64_t n = h->n;
    DevArr ku, kp, kf, off, bs, ci, ts, tn, tx, kt;
    AIXCHK(ku.alloc(8 * n));
    AIXCHK(kp.alloc(4 * n));
    AIXCHK(kf.alloc(n));
    uint64_t U = 0, total = 0, n_live = 0, n_circ = 0;
    int r = aix_unitigs_layout_dev(h, cutoff, (uint64_t*)ku.p, (uint32_t*)kp.p, (uint8_t*)kf.p, &U, &total, &n_live, &n_circ, nullptr);
    if (r) return r;
    AIXCHK(off.alloc(8 * (U + 1)));
    AIXCHK(bs.alloc(total));
    AIXCHK(ci.alloc(U));
    AIXCHK(ts.alloc(8 * U));
    AIXCHK(tn.alloc(4 * U));
    AIXCHK(tx.alloc(4 * U));
    if (kmer_tf_out) AIXCHK(kt.alloc(4 * n_live));
    r = aix_unitigs_emit_dev(h, cutoff, (const uint64_t*)ku.p, (const uint32_t*)kp.p, (const uint8_t*)kf.p, U, (uint64_t*)off.p, (uint8_t*)bs.p, (uint8_t*)ci.p,
                             (uint64_t*)ts.p, (uint32_t*)tn.p, (uint32_t*)tx.p, kmer_tf_out ? (uint32_t*)kt.p : nullptr, nullptr);
    if (r) return r;
    // host copies: {destination, device block, bytes}; a NULL destination is an output the caller did not ask for
    const HostOut outs[] = {
        {(void**)offsets_out, off.p, 8 * (U + 1)}, {(void**)bases_out, bs.p, total}, {(void**)circular_out, ci.p, U}, {(void**)tf_sum_out, ts.p, 8 * U},
        {(void**)tf_min_out, tn.p, 4 * U}, {(void**)tf_max_out, tx.p, 4 * U}, {(void**)kmer_tf_out, kt.p, 4 * n_live}, {(void**)kid_unitig_out, ku.p, 8 * n},
        {(void**)kid_pos_out, kp.p, 4 * n}, {(void**)kid_flag_out, kf.p, n}};
    AIXCHK(copy_out_host(outs, 10));
    *n_unitigs_out = U;
    return AIX_OK;
}

extern "C" int aix_unitig_links_dev(aix_index_t* h, uint32_t cutoff, const uint64_t* d_kid_unitig, const uint32_t* d_kid_pos, const uint8_t* d_kid_flag, uint64_t U,
                                    const uint64_t* d_offsets, uint64_t* d_link_off, uint32_t* d_link_to, uint64_t link_cap, uint64_t* n_links_out, void* stream) {
    const int st = ug_check_handle(h);
    if (st) return st;
    if (!d_kid_unitig || !d_kid_pos || !d_kid_flag || !d_offsets || !d_link_off || !n_links_out) return AIX_ERR_ARG;
    if (link_cap && !d_link_to) return AIX_ERR_ARG;
    if (U > h->n) return AIX_ERR_ARG;
    DevGuard g(h->device);
    bool bad = false;
    uint64_t E = 0;
    AIXCHK(ul_links(h, cutoff, d_kid_unitig, d_kid_pos, d_kid_flag, U, d_offsets, d_link_off, d_link_to, link_cap, &E, &bad, (hipStream_t)stream));
    if (bad) return AIX_ERR_ARG;
    *n_links_out = E;
    return E > link_cap ? AIX_ERR_ARG : AIX_OK;
}

extern "C" int aix_unitig_bubbles_dev(uint64_t U, const uint64_t* d_link_off, const uint32_t* d_link_to, uint64_t E, uint32_t* d_bubble_mate, void* stream) {
    if (!d_link_off) return AIX_ERR_ARG;
    if (U && !d_bubble_mate) return AIX_ERR_ARG;
    if (E && !d_link_to) return AIX_ERR_ARG;
    if (U > (uint64_t)kWNone / 2 || E > 8 * U) return AIX_ERR_ARG;
    if (U == 0) return AIX_OK;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_ul_bubbles, dim3(chain_grid(U, 4 * kCB, chain_test_grid())), dim3(kCB), 0, s, U, d_link_off, d_link_to, E, d_bubble_mate);
    AIXCHK(hipGetLastError());
    AIXCHK(hipStreamSynchronize(s));
    return AIX_OK;
}

extern "C" int aix_unitig_links(aix_index_t* h, uint32_t cutoff, uint64_t* n_unitigs_out, uint64_t* n_links_out, uint64_t** link_off_out, uint32_t** link_to_out,
                                uint32_t** bubble_mate_out) {
    const int st = ug_check_handle(h);
    if (st) return st;
    if (!n_unitigs_out || !n_links_out || !link_off_out || !link_to_out) return AIX_ERR_ARG;
    DevGuard g(h->device);
    const uint64_t n = h->n;
    DevArr ku, kp, kf, off, bs, ci, ts, tn, tx, lo, lt, bm;
    AIXCHK(ku.alloc(8 * n));
    AIXCHK(kp.alloc(4 * n));
    AIXCHK(kf.alloc(n));
    uint64_t U = 0, total = 0, n_live = 0, n_circ = 0, E = 0;
    int r = aix_unitigs_layout_dev(h, cutoff, (uint64_t*)ku.p, (uint32_t*)kp.p, (uint8_t*)kf.p, &U, &total, &n_live, &n_circ, nullptr);
    if (r) return r;
    AIXCHK(off.alloc(8 * (U + 1)));
    AIXCHK(bs.alloc(total));
    AIXCHK(ci.alloc(U));
    AIXCHK(ts.alloc(8 * U));
    AIXCHK(tn.alloc(4 * U));
    AIXCHK(tx.alloc(4 * U));
    r = aix_unitigs_emit_dev(h, cutoff, (const uint64_t*)ku.p, (const uint32_t*)kp.p, (const uint8_t*)kf.p, U, (uint64_t*)off.p, (uint8_t*)bs.p, (uint8_t*)ci.p,
                             (uint64_t*)ts.p, (uint32_t*)tn.p, (uint32_t*)tx.p, nullptr, nullptr);
    if (r) return r;
    bs.drop(); ci.drop(); ts.drop(); tn.drop(); tx.drop();
    AIXCHK(lo.alloc(8 * (2 * U + 1)));
    AIXCHK(lt.alloc(4 * 8 * U));
    r = aix_unitig_links_dev(h, cutoff, (const uint64_t*)ku.p, (const uint32_t*)kp.p, (const uint8_t*)kf.p, U, (const uint64_t*)off.p, (uint64_t*)lo.p,
                             (uint32_t*)lt.p, 8 * U, &E, nullptr);
    if (r) return r;
    if (bubble_mate_out) {
        AIXCHK(bm.alloc(4 * U));
        r = aix_unitig_bubbles_dev(U, (const uint64_t*)lo.p, (const uint32_t*)lt.p, E, (uint32_t*)bm.p, nullptr);
        if (r) return r;
    }
    const HostOut outs[] = {{(void**)link_off_out, lo.p, 8 * (2 * U + 1)}, {(void**)link_to_out, lt.p, 4 * E}, {(void**)bubble_mate_out, bm.p, 4 * U}};
    AIXCHK(copy_out_host(outs, 3));
    *n_unitigs_out = U;
    *n_links_out = E;
    return AIX_OK;
}
