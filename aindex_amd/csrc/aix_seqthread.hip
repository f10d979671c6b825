// aix_seqthread.hip — sequences threaded through a unitig or contig graph resident in HBM: the path of every sequence (one record per
// maximal run of windows that follow each other on one unitig), the link traversed between adjacent records, and the number of sequences
// that traverse every link. Two helpers carry the per-kid map there: aix_graph_kidmap_dev composes it with the map of one compaction
// round, aix_thread_nodes_dev packs it into one word per kid. The contract is stated above the declarations in include/aindex_hip.h;
// DESIGN 5l has the derivations and the resources. What the graph files share (the counters holder, the predicates of the validate
// kernels, the link search and the bisection) is in aix_graph.hpp. The chain of aix_seq_thread_dev (one plain launch per step; integer
// only, no LDS, no grid-wide barrier, no spin-wait):
//   validate k_st_validate: one lane per node word, per unitig and per end; nothing below runs on arrays that fail it
//   windows  k_st_windows: one lane per sequence, its windows max(0, L - 22); a scan gives woff[M + 1], the flat window space of W windows
//   probe    k_st_probe: one lane per window, wave-uniform loop: the 23 bytes at their place in the sequence, the kid by slot23_wave, ONE
//            8-byte gather of node[kid]; word[i] = the node with bit 0 replaced by the strand of the window, qv[i] = its offset
//   heads    k_st_heads: one lane per window compares its word with its predecessor's, read from memory (a run crosses waves, workgroups
//            and grid trips): head[i] = the window has a node and does not follow window i - 1
//   scan     rank[i] = heads in front of window i; rank[W] = the number of steps; seq_step_off[s] = rank[woff[s]]
//   steps    k_st_steps: the head lane of a step writes unitig, pos, flag, q_first, searches the link and adds the support; the tail lane
//            writes q_last
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "aix_graph.hpp"
#include "aix_probe.hpp"
#include "aix_seqhits.hpp"

namespace aix {

static constexpr uint64_t kStDead = ~0ULL;                        // node word of a dead kid, scratch word of a window without a node
static constexpr uint64_t kStPosMask = 0x7FFFFFFFull;

struct StCounters {                                               // one zeroed record per call
    unsigned long long bad, wide;
};

__device__ __forceinline__ uint64_t st_unitig(uint64_t w) { return w >> 33; }
__device__ __forceinline__ uint64_t st_pos(uint64_t w) { return (w >> 2) & kStPosMask; }

// ---------------------------------------------------------------------------------------------
// 1. the k-mer map through one compaction round
// ---------------------------------------------------------------------------------------------
// check = true: counts the violations, writes nothing; false: writes (the arrays passed the check). In place is fine: a lane reads its own
// entry before it writes it.
template <bool kCheck>
__global__ void __launch_bounds__(kCB) k_st_kidmap(uint64_t n, const uint64_t* kid_unitig, const uint32_t* kid_pos, const uint8_t* kid_flag, uint64_t U,
                                                  const uint64_t* __restrict__ offsets, const uint32_t* __restrict__ unitig_contig,
                                                  const uint64_t* __restrict__ unitig_pos, const uint8_t* __restrict__ unitig_flag, uint64_t* out_unitig,
                                                  uint32_t* out_pos, uint8_t* out_flag, StCounters* __restrict__ ctr) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    unsigned long long bad = 0;
    for (uint64_t kid = (uint64_t)blockIdx.x * kCB + threadIdx.x; kid < n; kid += stride) {
        const uint64_t u = kid_unitig[kid];
        uint64_t nu = AIX_UNITIG_NONE;
        uint32_t np = 0, nf = 0;
        if (u != AIX_UNITIG_NONE) {
            if (u >= U) { ++bad; continue; }
            const uint64_t lo = offsets[u], hi = offsets[u + 1], p = kid_pos[kid];
            if (hi < lo + 23 || p >= hi - lo - 22) { ++bad; continue; }
            const uint32_t c = unitig_contig[u];
            if (c != AIX_BUBBLE_NONE) {
                const uint64_t m = hi - lo - 22, base = unitig_pos[u];
                const uint32_t f = kid_flag[kid], uf = unitig_flag[u];
                const uint64_t add = (uf & 1u) ? m - 1 - p : p;
                if ((uint64_t)c >= kUnitLimit || base > 0xFFFFFFFFull - add) { ++bad; continue; }
                nu = c;
                np = (uint32_t)(base + add);
                nf = ((f ^ uf) & 1u) | ((f | uf) & 2u);
            }
        }
        if (!kCheck) { out_unitig[kid] = nu; out_pos[kid] = np; out_flag[kid] = (uint8_t)nf; }
    }
    if (kCheck) count_add(bad, &ctr->bad);
}

// ---------------------------------------------------------------------------------------------
// 2. one word per kid: unitig << 33 | pos << 2 | flag, all ones for a dead kid
// ---------------------------------------------------------------------------------------------
template <bool kCheck>
__global__ void __launch_bounds__(kCB) k_st_nodes(uint64_t n, const uint64_t* __restrict__ kid_unitig, const uint32_t* __restrict__ kid_pos,
                                                 const uint8_t* __restrict__ kid_flag, uint64_t U, const uint64_t* __restrict__ offsets, uint64_t* __restrict__ node,
                                                 StCounters* __restrict__ ctr) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    unsigned long long bad = 0, wide = 0;
    for (uint64_t kid = (uint64_t)blockIdx.x * kCB + threadIdx.x; kid < n; kid += stride) {
        const uint64_t u = kid_unitig[kid];
        uint64_t w = kStDead;
        if (u != AIX_UNITIG_NONE) {
            if (u >= U) { ++bad; continue; }
            const uint64_t lo = offsets[u], hi = offsets[u + 1], p = kid_pos[kid];
            if (hi < lo + 23 || p >= hi - lo - 22) { ++bad; continue; }
            if (p > kStPosMask) { ++wide; continue; }
            w = (u << 33) | (p << 2) | (kid_flag[kid] & 3u);
        }
        if (!kCheck) node[kid] = w;
    }
    if (kCheck) {
        count_add(bad, &ctr->bad);
        count_add(wide, &ctr->wide);
    }
}

// ---------------------------------------------------------------------------------------------
// 3. threading
// ---------------------------------------------------------------------------------------------
struct StGraph {                                                  // node map and graph in HBM
    uint64_t n, U, E;
    const uint64_t* node;
    const uint64_t* offsets;
    const uint8_t* circular;
    const uint64_t* link_off;
    const uint32_t* link_to;
};

// every node word names a unitig below U and a position inside it; offsets ascend by at least 23; link_off starts at 0, ascends, ends at E,
// and no end has more than 4 links
__global__ void __launch_bounds__(kCB) k_st_validate(const StGraph g, StCounters* __restrict__ ctr) {
    const uint64_t NE = 2 * g.U, work = g.n > NE ? g.n : NE, stride = (uint64_t)gridDim.x * kCB;
    unsigned long long bad = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kCB + threadIdx.x; i < work; i += stride) {
        if (i < g.n) {
            const uint64_t w = g.node[i];
            if (w != kStDead) {
                const uint64_t u = st_unitig(w);
                if (u >= g.U) ++bad;
                else {
                    const uint64_t lo = g.offsets[u], hi = g.offsets[u + 1];
                    bad += hi < lo + 23 || st_pos(w) >= hi - lo - 22;
                }
            }
        }
        if (i < g.U) bad += span_bad(g.offsets[i], g.offsets[i + 1]);
        if (i < NE) bad += csr_bad(i, NE, g.link_off[i], g.link_off[i + 1], g.E, 4);
    }
    count_add(bad, &ctr->bad);
}

__global__ void __launch_bounds__(kCB) k_st_windows(const uint64_t* __restrict__ offs, uint64_t M, uint64_t* __restrict__ nwin, StCounters* __restrict__ ctr) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    unsigned long long bad = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kCB + threadIdx.x; i <= M; i += stride) {
        uint64_t w = 0;
        if (i < M) {
            const uint64_t a = offs[i], b = offs[i + 1];
            bad += b < a || b - a >= (1ull << 32);                  // q_first / q_last are u32
            if (b >= a && b - a >= 23) w = b - a - 22;
        }
        nwin[i] = w;                                              // nwin[M] = 0: the scan's last entry is the total
    }
    count_add(bad, &ctr->bad);
}

// Pass 1. word[i]: the node of window i with bit 0 = the strand the window traverses its unitig in (flag bit 0 xor "the window is the
// reverse complement of the stored key"), kStDead without a node. qv[i]: the window's offset in its sequence.
__global__ void __launch_bounds__(kCB) k_st_probe(const IndexDev ix_, const uint8_t* __restrict__ seqs, const uint64_t* __restrict__ offs,
                                                 const uint64_t* __restrict__ woff, uint64_t M, uint64_t W, const uint64_t* __restrict__ node,
                                                 uint64_t* __restrict__ word, uint32_t* __restrict__ qv) {
    const IndexDev& ix = ix_;
    FilterGauge fg;
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t base = (uint64_t)blockIdx.x * kCB + (threadIdx.x & ~63u); base < W; base += stride) {      // wave-uniform
        const uint64_t i = base + (threadIdx.x & 63u);
        const bool in = i < W;
        const uint64_t s0 = wave_count_le(woff, M + 1, base) - 1;            // woff[0] == 0: the last sequence that starts at or before window `base`
        uint64_t w0 = 0, w1 = 0, w2 = 0, q = 0;
        if (in) {
            const uint64_t sq = gallop_last_le(woff, M, s0, i);                  // woff[M] == W > i; a sequence without windows is never the last one <= i
            q = i - woff[sq];
            load23(seqs + offs[sq] + q, w0, w1, w2);
        }
        uint64_t code = 0;
        const bool valid = in && encode23_clean(w0, w1, w2, code);           // upper-case A, C, G, T only
        const Probe pr = slot23_wave(ix, valid, code, fg.on);
        fg.seen(valid, pr.found);
        uint64_t w = kStDead;
        if (valid && pr.found && pr.slot < ix.n) {
            const uint64_t nd = node[pr.slot];
            if (nd != kStDead) w = nd ^ (code > revcomp(code, 23) ? 1ull : 0ull);
        }
        if (in) {
            word[i] = w;
            qv[i] = (uint32_t)q;
        }
    }
}

// window b follows window a of the same sequence on the same unitig
__device__ __forceinline__ bool st_follows(const StGraph& g, uint64_t a, uint64_t b) {
    if (((a ^ b) >> 33) || ((a ^ b) & 1u)) return false;
    const uint64_t pa = st_pos(a), pb = st_pos(b);
    const bool back = (a & 1u) != 0;
    const uint64_t from = back ? pb : pa, to = back ? pa : pb;   // forwards in the spelling: from -> to
    if (to == from + 1) return true;
    if (to != 0) return false;
    const uint64_t u = st_unitig(a);                             // a wrap: only round a circular unitig, from its last k-mer to its first
    if (u >= g.U || !g.circular[u]) return false;
    const uint64_t lo = g.offsets[u], hi = g.offsets[u + 1];
    return hi >= lo + 23 && from == hi - lo - 23;
}

// Pass 2. head[i] for i <= W (head[W] = 0).
__global__ void __launch_bounds__(kCB) k_st_heads(const StGraph g, const uint64_t* __restrict__ word, const uint32_t* __restrict__ qv, uint64_t W,
                                                 uint8_t* __restrict__ head) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t i = (uint64_t)blockIdx.x * kCB + threadIdx.x; i <= W; i += stride) {
        bool hd = false;
        if (i < W) {
            const uint64_t w = word[i];
            hd = w != kStDead;
            if (hd && qv[i] != 0) {                               // i > 0: window i - 1 belongs to the same sequence
                const uint64_t pw = word[i - 1];
                if (pw != kStDead && st_follows(g, pw, w)) hd = false;
            }
        }
        head[i] = hd ? 1 : 0;
    }
}

__global__ void __launch_bounds__(kCB) k_st_seqoff(const uint64_t* __restrict__ woff, const uint64_t* __restrict__ rank, uint64_t M, uint64_t* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t i = (uint64_t)blockIdx.x * kCB + threadIdx.x; i <= M; i += stride) out[i] = rank[woff[i]];
}

// index into link_to of the link e -> t, AIX_THREAD_BROKEN when e has no such link
__device__ __forceinline__ uint64_t st_find_link(const StGraph& g, uint64_t e, uint64_t t) {
    if (e >= 2 * g.U) return AIX_THREAD_BROKEN;
    const uint64_t lo = g.link_off[e], hi = g.link_off[e + 1];
    if (!csr_in_range(lo, hi, g.E, 4)) return AIX_THREAD_BROKEN;
    return link_find(g.link_to, lo, hi, t, AIX_THREAD_BROKEN);
}

struct StOut {
    uint32_t *unitig, *pos;
    uint8_t* flag;
    uint32_t *q_first, *q_last;
    uint64_t* link;
    unsigned long long* support;                                  // nullable
    uint64_t cap;
};

// Pass 3. Window i belongs to step rank[i + 1] - 1.
__global__ void __launch_bounds__(kCB) k_st_steps(const StGraph g, const uint64_t* __restrict__ word, const uint32_t* __restrict__ qv,
                                                 const uint8_t* __restrict__ head, const uint64_t* __restrict__ rank, uint64_t W, const StOut o) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t i = (uint64_t)blockIdx.x * kCB + threadIdx.x; i < W; i += stride) {
        const uint64_t w = word[i];
        if (w == kStDead) continue;
        const uint64_t r = rank[i + 1] - 1;
        if (r >= o.cap) continue;                                 // (never: the caller launches only when the total fits)
        const uint32_t q = qv[i];
        if (head[i]) {
            const uint64_t v = st_unitig(w), pv = st_pos(w), sv = w & 1u;
            uint64_t link = AIX_THREAD_NO_LINK;
            const uint64_t pw = q ? word[i - 1] : kStDead;
            const bool circ = v < g.U && g.circular[v];
            if (pw != kStDead) {                                  // adjacent steps: the junction pw -> w
                link = AIX_THREAD_BROKEN;
                const uint64_t u = st_unitig(pw), pu = st_pos(pw), su = pw & 1u;
                if (u < g.U && v < g.U) {
                    const uint64_t ulo = g.offsets[u], uhi = g.offsets[u + 1], vlo = g.offsets[v], vhi = g.offsets[v + 1];
                    const bool at_exit = uhi >= ulo + 23 && (su ? pu == 0 : pu == uhi - ulo - 23);
                    const bool at_entry = vhi >= vlo + 23 && (sv ? pv == vhi - vlo - 23 : pv == 0);
                    if (at_exit && at_entry) {
                        const uint64_t e = 2 * u + su, t = 2 * v + sv;
                        link = st_find_link(g, e, t);
                        if (link != AIX_THREAD_BROKEN && o.support) {
                            atomicAdd(o.support + link, 1ull);
                            const uint64_t dual = st_find_link(g, t ^ 1, e ^ 1);
                            if (dual != AIX_THREAD_BROKEN && dual != link) atomicAdd(o.support + dual, 1ull);
                        }
                    }
                }
            }
            o.unitig[r] = (uint32_t)v;
            o.pos[r] = (uint32_t)pv;
            o.flag[r] = (uint8_t)(sv | (circ ? 2u : 0u));
            o.q_first[r] = q;
            o.link[r] = link;
        }
        if (i + 1 == W || head[i + 1] || word[i + 1] == kStDead) o.q_last[r] = q;
    }
}

static hipError_t st_validate(const StGraph& g, bool* bad, hipStream_t s) {
    Counted<StCounters> ctr(s);
    AIX_TRY(ctr.init());
    AIX_TRY(ctr.run([&]() {
        AIX_TRY_LAUNCH(k_st_validate, dim3(chain_grid(std::max(g.n, 2 * g.U), 4 * kCB, chain_test_grid())), dim3(kCB), 0, s, g, ctr.dev());
        return hipSuccess;
    }));
    *bad = ctr.host.bad != 0;
    return hipSuccess;
}

struct StRun {                                                    // the scratch of one call between its two halves
    DevArr woff, word, qv, head, rank, tmp, tmp2;
    uint64_t W = 0, total = 0;
    explicit StRun(hipStream_t s) : woff(s), word(s), qv(s), head(s), rank(s), tmp(s), tmp2(s) {}
};

// Passes 1 and 2 and the scans: R.total steps, d_seq_step_off[M + 1] written. *bad: a sequence of 2^32 bytes or more, descending offsets,
// or windows without a byte buffer (nothing is written then). Synchronises `s`.
static hipError_t st_prepare(const aix_index* h, const StGraph& g, const uint8_t* d_seqs, const uint64_t* d_offs, uint64_t M, uint64_t* d_seq_step_off, StRun& R,
                             bool* bad, hipStream_t s) {
    const uint64_t cap = chain_test_grid();
    const dim3 blk(kCB);
    *bad = false;
    R.W = R.total = 0;
    Counted<StCounters> ctr(s);
    DevArr nwin(s);
    AIX_TRY(ctr.init());
    AIX_TRY(sh_alloc(nwin, M + 1, 8));
    AIX_TRY(sh_alloc(R.woff, M + 1, 8));
    uint64_t W = 0;
    AIX_TRY(ctr.run([&]() {
        AIX_TRY_LAUNCH(k_st_windows, dim3(chain_grid(M + 1, 4 * kCB, cap)), blk, 0, s, d_offs, M, (uint64_t*)nwin.p, ctr.dev());
        AIX_TRY(scan_u64((const uint64_t*)nwin.p, (uint64_t*)R.woff.p, M + 1, R.tmp, s));
        return hipMemcpyAsync(&W, (const uint64_t*)R.woff.p + M, 8, hipMemcpyDeviceToHost, s);
    }));
    if (ctr.host.bad || (W && !d_seqs)) { *bad = true; return hipSuccess; }
    R.W = W;
    if (W == 0) {
        AIX_TRY(hipMemsetAsync(d_seq_step_off, 0, 8 * (M + 1), s));
        return hipStreamSynchronize(s);
    }
    AIX_TRY(sh_alloc(R.word, W, 8));
    AIX_TRY(sh_alloc(R.qv, W, 4));
    AIX_TRY(sh_alloc(R.head, W + 1, 1));
    AIX_TRY(sh_alloc(R.rank, W + 1, 8));
    const uint64_t* woff = (const uint64_t*)R.woff.p;
    AIX_TRY_LAUNCH(k_st_probe, dim3(chain_grid(W, kCB, cap)), blk, 0, s, h->dev(), d_seqs, d_offs, woff, M, W, g.node, (uint64_t*)R.word.p, (uint32_t*)R.qv.p);
    AIX_TRY_LAUNCH(k_st_heads, dim3(chain_grid(W + 1, 4 * kCB, cap)), blk, 0, s, g, (const uint64_t*)R.word.p, (const uint32_t*)R.qv.p, W, (uint8_t*)R.head.p);
    AIX_TRY(scan_u64(rocprim::make_transform_iterator((const uint8_t*)R.head.p, Widen<uint8_t>()), (uint64_t*)R.rank.p, W + 1, R.tmp2, s));
    AIX_TRY_LAUNCH(k_st_seqoff, dim3(chain_grid(M + 1, 4 * kCB, cap)), blk, 0, s, woff, (const uint64_t*)R.rank.p, M, d_seq_step_off);
    AIX_TRY(hipMemcpyAsync(&R.total, (const uint64_t*)R.rank.p + W, 8, hipMemcpyDeviceToHost, s));
    return hipStreamSynchronize(s);
}

// Pass 3: the R.total records (o.cap >= R.total) and the support adds. Synchronises `s`.
static hipError_t st_write(const StGraph& g, const StRun& R, const StOut& o, hipStream_t s) {
    if (R.total == 0) return hipSuccess;
    AIX_TRY_LAUNCH(k_st_steps, dim3(chain_grid(R.W, 2 * kCB, chain_test_grid())), dim3(kCB), 0, s, g, (const uint64_t*)R.word.p, (const uint32_t*)R.qv.p,
                   (const uint8_t*)R.head.p, (const uint64_t*)R.rank.p, R.W, o);
    return hipStreamSynchronize(s);
}

}  // namespace aix

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" int aix_graph_kidmap_dev(uint64_t n, const uint64_t* d_kid_unitig, const uint32_t* d_kid_pos, const uint8_t* d_kid_flag, uint64_t U,
                                    const uint64_t* d_offsets, const uint32_t* d_unitig_contig, const uint64_t* d_unitig_pos, const uint8_t* d_unitig_flag,
                                    uint64_t* d_out_unitig, uint32_t* d_out_pos, uint8_t* d_out_flag, void* stream) {
    if (!d_offsets) return AIX_ERR_ARG;
    if (n && (!d_kid_unitig || !d_kid_pos || !d_kid_flag || !d_out_unitig || !d_out_pos || !d_out_flag)) return AIX_ERR_ARG;
    if (U && (!d_unitig_contig || !d_unitig_pos || !d_unitig_flag)) return AIX_ERR_ARG;
    if (n == 0) return AIX_OK;
    hipStream_t s = (hipStream_t)stream;
    Counted<StCounters> ctr(s);
    AIXCHK(ctr.init());
    const dim3 grid(chain_grid(n, 4 * kCB, chain_test_grid())), blk(kCB);
    AIXCHK(ctr.run([&]() {
        AIX_TRY_LAUNCH(k_st_kidmap<true>, grid, blk, 0, s, n, d_kid_unitig, d_kid_pos, d_kid_flag, U, d_offsets, d_unitig_contig, d_unitig_pos, d_unitig_flag, d_out_unitig,
                       d_out_pos, d_out_flag, ctr.dev());
        return hipSuccess;
    }));
    if (ctr.host.bad) return AIX_ERR_ARG;
    hipLaunchKernelGGL(k_st_kidmap<false>, grid, blk, 0, s, n, d_kid_unitig, d_kid_pos, d_kid_flag, U, d_offsets, d_unitig_contig, d_unitig_pos, d_unitig_flag, d_out_unitig,
                       d_out_pos, d_out_flag, ctr.dev());
    AIXCHK(hipGetLastError());
    AIXCHK(hipStreamSynchronize(s));
    return AIX_OK;
}

extern "C" int aix_thread_nodes_dev(uint64_t n, const uint64_t* d_kid_unitig, const uint32_t* d_kid_pos, const uint8_t* d_kid_flag, uint64_t U,
                                    const uint64_t* d_offsets, uint64_t* d_node, void* stream) {
    if (U > kUnitLimit) return AIX_ERR_UNSUPPORTED;
    if (!d_offsets) return AIX_ERR_ARG;
    if (n && (!d_kid_unitig || !d_kid_pos || !d_kid_flag || !d_node)) return AIX_ERR_ARG;
    if (n == 0) return AIX_OK;
    hipStream_t s = (hipStream_t)stream;
    Counted<StCounters> ctr(s);
    AIXCHK(ctr.init());
    const dim3 grid(chain_grid(n, 4 * kCB, chain_test_grid())), blk(kCB);
    AIXCHK(ctr.run([&]() {
        AIX_TRY_LAUNCH(k_st_nodes<true>, grid, blk, 0, s, n, d_kid_unitig, d_kid_pos, d_kid_flag, U, d_offsets, d_node, ctr.dev());
        return hipSuccess;
    }));
    if (ctr.host.bad) return AIX_ERR_ARG;
    if (ctr.host.wide) return AIX_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_st_nodes<false>, grid, blk, 0, s, n, d_kid_unitig, d_kid_pos, d_kid_flag, U, d_offsets, d_node, ctr.dev());
    AIXCHK(hipGetLastError());
    AIXCHK(hipStreamSynchronize(s));
    return AIX_OK;
}

// the refusals of the handle: those of aix_unitigs_layout_dev
static int st_check_handle(const aix_index_t* h) {
    if (!h) return AIX_ERR_ARG;
    if (h->k != 23) return AIX_ERR_MODE;
    if (!h->canonical_only) return AIX_ERR_UNSUPPORTED;
    if (h->n == 0) return AIX_ERR_UNSUPPORTED;
    if (2 * h->n > 0xFFFFFFF8ull) return AIX_ERR_UNSUPPORTED;
    return AIX_OK;
}

extern "C" int aix_seq_thread_dev(aix_index_t* h, const char* d_seqs, const uint64_t* d_offs, uint64_t M, const uint64_t* d_node, uint64_t U,
                                  const uint64_t* d_offsets, const uint8_t* d_circular, const uint64_t* d_link_off, const uint32_t* d_link_to, uint64_t E,
                                  uint64_t* d_link_support, uint64_t* d_seq_step_off, uint32_t* d_step_unitig, uint32_t* d_step_pos, uint8_t* d_step_flag,
                                  uint32_t* d_q_first, uint32_t* d_q_last, uint64_t* d_step_link, uint64_t cap, uint64_t* total_out, void* stream) {
    const int st = st_check_handle(h);
    if (st) return st;
    if (U > kUnitLimit) return AIX_ERR_UNSUPPORTED;
    if (!d_node || !d_offsets || !d_link_off || !d_seq_step_off || !total_out || (M && !d_offs) || M >= (1ull << 56)) return AIX_ERR_ARG;
    if ((U && !d_circular) || (E && !d_link_to) || E > 8 * U) return AIX_ERR_ARG;
    if (cap && (!d_step_unitig || !d_step_pos || !d_step_flag || !d_q_first || !d_q_last || !d_step_link)) return AIX_ERR_ARG;
    DevGuard guard(h->device);
    hipStream_t s = (hipStream_t)stream;
    const StGraph g{h->n, U, E, d_node, d_offsets, d_circular, d_link_off, d_link_to};
    bool bad = false;
    AIXCHK(st_validate(g, &bad, s));
    if (bad) return AIX_ERR_ARG;
    if (M == 0) {
        AIXCHK(hipMemsetAsync(d_seq_step_off, 0, 8, s));
        AIXCHK(hipStreamSynchronize(s));
        *total_out = 0;
        return AIX_OK;
    }
    StRun R(s);
    AIXCHK(st_prepare(h, g, (const uint8_t*)d_seqs, d_offs, M, d_seq_step_off, R, &bad, s));
    if (bad) return AIX_ERR_ARG;
    *total_out = R.total;
    if (R.total > cap) return AIX_OK;                              // sized: the caller repeats with room; nothing was counted
    const StOut o{d_step_unitig, d_step_pos, d_step_flag, d_q_first, d_q_last, d_step_link, (unsigned long long*)d_link_support, cap};
    AIXCHK(st_write(g, R, o, s));
    return AIX_OK;
}

// Layout, emit, links and nodes at `cutoff`, then the threads, for host memory: every array is malloc'd (aix_free).
extern "C" int aix_seq_thread(aix_index_t* h, uint32_t cutoff, const char* seqs, const uint64_t* offs, uint64_t M, uint64_t** seq_step_off_out,
                              uint32_t** step_unitig_out, uint32_t** step_pos_out, uint8_t** step_flag_out, uint32_t** q_first_out, uint32_t** q_last_out,
                              uint64_t** step_link_out, uint64_t** link_support_out, uint64_t* n_unitigs_out, uint64_t* n_links_out) {
    const int st = st_check_handle(h);
    if (st) return st;
    if (!seq_step_off_out || !step_unitig_out || !step_pos_out || !step_flag_out || !q_first_out || !q_last_out || !step_link_out || !offs || M >= (1ull << 56))
        return AIX_ERR_ARG;
    if (M && offs[M] && !seqs) return AIX_ERR_ARG;
    DevGuard guard(h->device);
    const uint64_t n = h->n;
    DevArr ku, kp, kf, off, bs, ci, ts, tn, tx, lo, lt, nd, sup, sso, su, sp, sf, qf, ql, sl;
    AIXCHK(ku.alloc(8 * n));
    AIXCHK(kp.alloc(4 * n));
    AIXCHK(kf.alloc(n));
    uint64_t U = 0, total_bases = 0, n_live = 0, n_circ = 0, E = 0;
    int r = aix_unitigs_layout_dev(h, cutoff, (uint64_t*)ku.p, (uint32_t*)kp.p, (uint8_t*)kf.p, &U, &total_bases, &n_live, &n_circ, nullptr);
    if (r) return r;
    AIXCHK(off.alloc(8 * (U + 1)));
    AIXCHK(bs.alloc(total_bases));
    AIXCHK(ci.alloc(U));
    AIXCHK(ts.alloc(8 * U));
    AIXCHK(tn.alloc(4 * U));
    AIXCHK(tx.alloc(4 * U));
    r = aix_unitigs_emit_dev(h, cutoff, (const uint64_t*)ku.p, (const uint32_t*)kp.p, (const uint8_t*)kf.p, U, (uint64_t*)off.p, (uint8_t*)bs.p, (uint8_t*)ci.p,
                             (uint64_t*)ts.p, (uint32_t*)tn.p, (uint32_t*)tx.p, nullptr, nullptr);
    if (r) return r;
    bs.drop(); ts.drop(); tn.drop(); tx.drop();
    AIXCHK(lo.alloc(8 * (2 * U + 1)));
    AIXCHK(lt.alloc(4 * 8 * U));
    r = aix_unitig_links_dev(h, cutoff, (const uint64_t*)ku.p, (const uint32_t*)kp.p, (const uint8_t*)kf.p, U, (const uint64_t*)off.p, (uint64_t*)lo.p, (uint32_t*)lt.p,
                             8 * U, &E, nullptr);
    if (r) return r;
    AIXCHK(nd.alloc(8 * n));
    r = aix_thread_nodes_dev(n, (const uint64_t*)ku.p, (const uint32_t*)kp.p, (const uint8_t*)kf.p, U, (const uint64_t*)off.p, (uint64_t*)nd.p, nullptr);
    if (r) return r;
    ku.drop(); kp.drop(); kf.drop();
    AIXCHK(sup.alloc(8 * E));
    AIXCHK(hipMemset(sup.p, 0, 8 * E));
    DevArr ds, dof;
    if (const int su_st = sh_upload(seqs, offs, M, ds, dof)) return su_st;
    AIXCHK(sso.alloc(8 * (M + 1)));
    AIXCHK(hipMemset(sso.p, 0, 8 * (M + 1)));
    const StGraph g{n, U, E, (const uint64_t*)nd.p, (const uint64_t*)off.p, (const uint8_t*)ci.p, (const uint64_t*)lo.p, (const uint32_t*)lt.p};
    uint64_t T = 0;
    if (M) {
        StRun R(nullptr);
        bool bad = false;
        AIXCHK(st_prepare(h, g, (const uint8_t*)ds.p, (const uint64_t*)dof.p, M, (uint64_t*)sso.p, R, &bad, nullptr));
        if (bad) return AIX_ERR_ARG;
        T = R.total;
        AIXCHK(sh_alloc(su, T, 4));
        AIXCHK(sh_alloc(sp, T, 4));
        AIXCHK(sh_alloc(sf, T, 1));
        AIXCHK(sh_alloc(qf, T, 4));
        AIXCHK(sh_alloc(ql, T, 4));
        AIXCHK(sh_alloc(sl, T, 8));
        const StOut o{(uint32_t*)su.p, (uint32_t*)sp.p, (uint8_t*)sf.p, (uint32_t*)qf.p, (uint32_t*)ql.p, (uint64_t*)sl.p, (unsigned long long*)sup.p, T};
        AIXCHK(st_write(g, R, o, nullptr));
    }
    const HostOut outs[] = {{(void**)seq_step_off_out, sso.p, 8 * (M + 1)}, {(void**)step_unitig_out, su.p, 4 * T}, {(void**)step_pos_out, sp.p, 4 * T},
                            {(void**)step_flag_out, sf.p, T},               {(void**)q_first_out, qf.p, 4 * T},     {(void**)q_last_out, ql.p, 4 * T},
                            {(void**)step_link_out, sl.p, 8 * T},           {(void**)link_support_out, sup.p, 8 * E}};
    AIXCHK(copy_out_host(outs, 8));
    if (n_unitigs_out) *n_unitigs_out = U;
    if (n_links_out) *n_links_out = E;
    return AIX_OK;
}
