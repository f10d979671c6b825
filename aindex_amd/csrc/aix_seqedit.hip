// aix_seqedit.hip — sequences against the indexed reads with substitutions, insertions and deletions: seed hits -> alignments verified by
// a banded edit-distance programme (include/aindex_hip.h above aix_seq_edit is the contract; tests/seqedit_ref.py restates it).
//   edit_distance beside hamming_distance     aindex/core/aindex.py:22-23   (the reference imports both; it holds no search over either)
// The chain is that of aix_seqfind.hip with another verification:
//   1 sh_run          the seeds of a sequence are its 23-windows at offsets 0, step, ..; their hits (position, window offset, strand flag)
//   2 k_se_verify     THE HOT PATH. Phase 1, one lane per hit: its sequence (bisection of the hit offsets), the anchored diagonal a, the
//                     interval that contains the seed (bisection of the interval starts), the text columns [lo, hi].
//                     Phase 2, kSeLanes lanes per proposal: lane k owns diagonal k - ed of the band. A cell is one word (dist << 4) | start_k,
//                     start_k = start - (a - ed) <= 14, so an integer min is the lexicographic min of (dist, start). Per row: the diagonal
//                     move from the lane's own previous cell, the vertical one from lane k + 1 (one DPP row shift), the horizontal chain as
//                     a min-plus prefix scan over the 16 lanes (four DPP row shifts). Text bytes stream per lane, pattern bytes per group,
//                     a dword per four rows. Out once every cell of a row exceeds ed (costs never fall along a path).
//                     Phase 3, one lane per hit again: coalesced stores of the survivors' keys and columns.
//   3 survivors only  closed up by a scan of the keep flags; two STABLE radix sorts of a permutation, by (start, strand, dist, end) and by
//                     sequence; k_se_heads marks the first entry of every (sequence, start, strand) run — its smallest (dist, end) —, a
//                     scan numbers the records, k_se_seqoff gives the CSR offsets, k_se_write the records.
// Every size, offset and flat index is 64 bits wide. No atomics, no LDS, no scratch; all stores are plain vector stores. Nothing depends on
// the launch geometry.
#include "aix_seqhits.hpp"

namespace aix {

static constexpr uint32_t kSeLanes = 16;                       // lanes that share one proposal: one DPP row
static constexpr uint32_t kSeGroups = 64 / kSeLanes;           // proposals a wave verifies at a time
static constexpr uint32_t kSeInf = 1u << 28;                   // a cell that does not exist or cannot be reached; cells are clamped to it
static_assert(2 * AIX_SEQEDIT_MAX_ED + 1 <= kSeLanes, "the band must fit one group of lanes");
static_assert(2 * AIX_SEQEDIT_MAX_ED <= 15, "start_k lives in four bits");

// The sort key of a survivor: start (54 bits) | strand (1) | dist (3) | w (5), w = (end - start) - L + 2 ed in [0, 28]. For one
// (sequence, start, strand) ascending (dist, w) is ascending (dist, end).
static constexpr unsigned kSeLowBits = 8;

// ---------------------------------------------------------------------------------------------
// 2. verification
// ---------------------------------------------------------------------------------------------
struct SeVerify {
    const uint8_t* seqs;
    const uint64_t* offs;          // [M + 1]
    const uint64_t* soff;          // [M + 1] hits before sequence i
    uint64_t M, T;
    const uint64_t* pos;           // [T] the hits
    const uint32_t* qoff;
    const uint8_t* flag;
    const uint8_t* reads;
    uint64_t reads_len;
    const uint64_t *rs, *re, *rr;  // interval starts / ends / rids
    uint64_t rn;
    uint32_t ed;
    uint8_t* keep;                 // outputs, [T] each: keep for every hit, the others where keep != 0
    uint64_t* key;                 // (start << 9) | (strand << 8) | (dist << 5) | w
    uint64_t* hseq;
    uint64_t* end;
    uint64_t* rid;
    uint64_t* local;
};

// DPP moves inside a row of 16 lanes; a lane without a source keeps `old`
__device__ __forceinline__ int se_from_above(int old, int v) {   // lane k <- lane k + 1 (row_shl:1)
    return __builtin_amdgcn_update_dpp(old, v, 0x101, 0xf, 0xf, false);
}
template <int N>
__device__ __forceinline__ int se_min_below(int v) {             // min(v, lane k - N's v) (row_shr:N)
    return min(v, __builtin_amdgcn_update_dpp(v, v, 0x110 + N, 0xf, 0xf, false));
}

__global__ void __launch_bounds__(kSB) k_se_verify(const SeVerify P) {
    const uint32_t lane = threadIdx.x & 63u, k = lane & (kSeLanes - 1u), grp = lane / kSeLanes;
    const uint64_t stride = (uint64_t)gridDim.x * kSB;
    const uint64_t slen = P.offs[P.M];
    const uint32_t ed = P.ed, live = ((ed + 1u) << 4) - 1u;    // a cell with dist <= ed is <= live
    const int k16 = (int)(k << 4);
    for (uint64_t base = (uint64_t)blockIdx.x * kSB + (threadIdx.x & ~63u); base < P.T; base += stride) {    // wave-uniform
        // phase 1: one lane per hit
        const uint64_t e = base + lane;
        bool ok = false;
        int64_t a = 0;
        uint64_t so = 0, sq = 0, rd = 0, sv = 0, ulo = 0, uhi = 0;             // ulo / uhi: lo / hi as offsets from the band's origin a - ed
        uint32_t L = 0, strand = 2;
        if (e < P.T) strand = P.flag[e] & 3u;
        if (strand < 2) {                                      // so pos + 23 <= reads_len (k_sh_hits compared the bytes)
            uint64_t lo = 0, hi = P.M;                         // soff[lo] <= e < soff[hi]: soff[0] == 0, soff[M] == T
            while (hi - lo > 1) {
                const uint64_t mid = lo + ((hi - lo) >> 1);
                if (P.soff[mid] <= e) lo = mid; else hi = mid;
            }
            sq = lo;
            so = P.offs[sq];
            L = (uint32_t)(P.offs[sq + 1] - so);               // < 2^32 (k_sh_windows)
            const uint64_t p = P.pos[e], q = P.qoff[e];
            a = (int64_t)p - (int64_t)(strand == 0 ? q : (uint64_t)L - 23 - q);        // q <= L - 23; p < reads_len < 2^54
            uint64_t c0 = 0, c1 = P.rn;                        // the intervals with start <= p are [0, c0)
            while (c0 < c1) {
                const uint64_t mid = c0 + ((c1 - c0) >> 1);
                if (P.rs[mid] <= p) c0 = mid + 1; else c1 = mid;
            }
            if (c0) {                                          // sorted and disjoint: only the last of them can hold the seed
                const uint64_t en = P.re[c0 - 1];
                sv = P.rs[c0 - 1];
                if (en >= p && en - p >= 23) {
                    ok = true;
                    rd = P.rr[c0 - 1];
                    const int64_t org = a - (int64_t)ed;
                    const int64_t tlo = max((int64_t)sv, org);                          // >= 0
                    const int64_t thi = min((int64_t)min(en, P.reads_len), a + (int64_t)L + (int64_t)ed);   // >= p + 23 > tlo
                    ulo = (uint64_t)(tlo - org);
                    uhi = (uint64_t)(thi - org);
                }
            }
        }
        // phase 2: round r verifies the proposals of lanes r * kSeGroups .. + kSeGroups - 1, one per group of kSeLanes lanes
        const uint64_t okm = __ballot(ok);
        uint32_t mine = 0xFFFFFFFFu;                           // (cell << 4) | k of the best cell of row L of this lane's own hit
        for (uint32_t r = 0; r < kSeLanes; ++r) {
            if (((okm >> (r * kSeGroups)) & ((1ull << kSeGroups) - 1ull)) == 0) continue;                  // wave-uniform
            const uint32_t src = r * kSeGroups + grp;
            const bool g_ok = (okm >> src) & 1ull;
            const int64_t g_a = (int64_t)sf_shfl64((uint64_t)a, src);
            const uint64_t g_so = sf_shfl64(so, src), g_ulo = sf_shfl64(ulo, src), g_uhi = sf_shfl64(uhi, src);
            const uint32_t g_L = bperm(src, L), g_strand = bperm(src, strand);
            // this lane's cells exist in the rows [ilo, ihi]: ulo <= row + k <= uhi and k <= 2 ed (rows are <= L < 2^32)
            uint32_t ilo = 1, ihi = 0;
            if (g_ok && k <= 2u * ed && g_uhi >= k) {
                ilo = g_ulo > k ? (uint32_t)min(g_ulo - k, (uint64_t)0xFFFFFFFFu) : 0u;
                ihi = (uint32_t)min(g_uhi - k, (uint64_t)0xFFFFFFFFu);
            }
            int c = (ilo == 0 && ilo <= ihi) ? (int)k : (int)kSeInf;             // row 0: dist 0, the start is this column
            const int64_t xat = g_a - (int64_t)ed + (int64_t)k;                  // text byte of the diagonal move into row i + 1: xat + i
            for (uint64_t i0 = 0;; i0 += 4) {                // 64 bits: L may be just below 2^32
                const uint64_t lm = __ballot((uint32_t)c <= live);
                const bool run = g_ok && i0 < g_L && ((lm >> (grp * kSeLanes)) & ((1ull << kSeLanes) - 1ull)) != 0;
                if (__ballot(run) == 0) break;                 // wave-uniform
                if (run) {                                     // uniform in the group: a DPP row is wholly in or wholly out
                    const uint32_t nv = (uint32_t)min((uint64_t)4, (uint64_t)g_L - i0);
                    const uint32_t x = ilo <= ihi ? sf_load4(P.reads, P.reads_len, xat + (int64_t)i0) : 0u;    // lanes outside the band load nothing
                    uint32_t y;
                    if (g_strand == 0) {
                        y = sf_load4(P.seqs, slen, (int64_t)(g_so + i0));
                    } else {                                   // y_b = comp(seq[L - 1 - i0 - b]): the dword that ends at L - 1 - i0, reversed
                        const uint32_t w = __builtin_bswap32(sf_load4(P.seqs, slen, (int64_t)g_so + (int64_t)g_L - 4 - (int64_t)i0));
                        y = sf_comp(w & 0xFFu) | (sf_comp((w >> 8) & 0xFFu) << 8) | (sf_comp((w >> 16) & 0xFFu) << 16) | (sf_comp(w >> 24) << 24);
                    }
#pragma unroll
                    for (uint32_t b = 0; b < 4; ++b) {
                        if (b < nv) {
                            const uint32_t row = (uint32_t)i0 + b + 1;               // <= L
                            const uint32_t xb = (x >> (8 * b)) & 0xFFu, yb = (y >> (8 * b)) & 0xFFu;
                            const int sub = (xb != yb && xb != 'N' && yb != 'N') ? 16 : 0;
                            const bool here = row >= ilo && row <= ihi;
                            const int up = se_from_above((int)kSeInf, c);
                            int v = here ? min(c + sub, up + 16) : (int)kSeInf;
                            v -= k16;                          // h_k = min over m <= k of v_m + 16 (k - m): a prefix min of v_m - 16 m
                            v = se_min_below<1>(v);
                            v = se_min_below<2>(v);
                            v = se_min_below<4>(v);
                            v = se_min_below<8>(v);
                            v += k16;
                            c = here ? min(v, (int)kSeInf) : (int)kSeInf;
                        }
                    }
                }
            }
            // the best cell of row L: min over the group of (cell << 4) | k; a proposal that left early or never started has none <= live
            uint32_t best = (g_ok && (uint32_t)c <= live) ? (((uint32_t)c << 4) | k) : 0xFFFFFFFFu;
#pragma unroll
            for (uint32_t d = 1; d < kSeLanes; d <<= 1) best = min(best, bperm(lane ^ d, best));
            const uint32_t back = bperm((lane % kSeGroups) * kSeLanes, best);  // the group that verified this lane's hit in round lane / kSeGroups
            if (lane / kSeGroups == r) mine = back;
        }
        if (e < P.T) {
            const bool kept = ok && mine != 0xFFFFFFFFu;       // dist <= ed
            P.keep[e] = kept ? 1 : 0;
            if (kept) {
                const uint32_t kend = mine & 15u, sk = (mine >> 4) & 15u, dist = mine >> 8;
                const uint64_t start = (uint64_t)(a - (int64_t)ed + (int64_t)sk);       // >= lo >= 0
                const uint64_t w = kend + 2u * ed - sk;        // (end - start) - L + 2 ed
                P.key[e] = (start << (kSeLowBits + 1)) | ((uint64_t)strand << kSeLowBits) | ((uint64_t)dist << 5) | w;
                P.hseq[e] = sq;
                P.end[e] = (uint64_t)(a - (int64_t)ed + (int64_t)L + (int64_t)kend);
                P.rid[e] = rd;
                P.local[e] = start - sv;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// 3. the survivors: closed up, sorted, made unique, written
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSB) k_se_compact(const uint8_t* __restrict__ keep, const uint64_t* __restrict__ srank, const uint64_t* __restrict__ key, uint64_t T,
                                                   uint64_t* __restrict__ ckey, uint64_t* __restrict__ csrc) {
    const uint64_t stride = (uint64_t)gridDim.x * kSB;
    for (uint64_t e = (uint64_t)blockIdx.x * kSB + threadIdx.x; e < T; e += stride) {
        if (keep[e]) {
            const uint64_t j = srank[e];
            ckey[j] = key[e];
            csrc[j] = e;
        }
    }
}

// head[i] = sorted survivor i opens a (sequence, start, strand) run; head[S] = 0
__global__ void __launch_bounds__(kSB) k_se_heads(const uint64_t* __restrict__ perm, const uint64_t* __restrict__ sseq, const uint64_t* __restrict__ key, uint64_t S,
                                                 uint8_t* __restrict__ head) {
    const uint64_t stride = (uint64_t)gridDim.x * kSB;
    for (uint64_t i = (uint64_t)blockIdx.x * kSB + threadIdx.x; i <= S; i += stride)
        head[i] = (i < S && (i == 0 || sseq[i - 1] != sseq[i] || (key[perm[i - 1]] >> kSeLowBits) != (key[perm[i]] >> kSeLowBits))) ? 1 : 0;
}

// find_offsets[i] = records of the sequences before i: the record that the first sorted survivor of a sequence >= i opens
__global__ void __launch_bounds__(kSB) k_se_seqoff(const uint64_t* __restrict__ sseq, const uint64_t* __restrict__ orank, uint64_t S, uint64_t M,
                                                  uint64_t* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * kSB;
    for (uint64_t i = (uint64_t)blockIdx.x * kSB + threadIdx.x; i <= M; i += stride) {
        uint64_t lo = 0, hi = S;
        while (lo < hi) {
            const uint64_t mid = lo + ((hi - lo) >> 1);
            if (sseq[mid] < i) lo = mid + 1; else hi = mid;
        }
        out[i] = orank[lo];                                    // orank[S] = the number of records
    }
}

struct SeOut {
    uint64_t *start, *end, *rid, *local;
    uint8_t* strand;
    uint32_t* dist;
};
__global__ void __launch_bounds__(kSB) k_se_write(const uint8_t* __restrict__ head, const uint64_t* __restrict__ orank, const uint64_t* __restrict__ perm, uint64_t S,
                                                 const uint64_t* __restrict__ key, const uint64_t* __restrict__ end, const uint64_t* __restrict__ rid,
                                                 const uint64_t* __restrict__ local, const SeOut O) {
    const uint64_t stride = (uint64_t)gridDim.x * kSB;
    for (uint64_t i = (uint64_t)blockIdx.x * kSB + threadIdx.x; i < S; i += stride) {
        if (!head[i]) continue;                                // the head of a run is its smallest (dist, end)
        const uint64_t o = orank[i], e = perm[i], kk = key[e];
        O.start[o] = kk >> (kSeLowBits + 1);
        O.end[o] = end[e];
        O.rid[o] = rid[e];
        O.local[o] = local[e];
        O.strand[o] = (uint8_t)((kk >> kSeLowBits) & 1u);
        O.dist[o] = (uint32_t)((kk >> 5) & 7u);
    }
}

// what a call holds between sizing and writing
struct SeState {
    DevArr key, end, rid, local, perm, head, orank;
    uint64_t S = 0, R = 0;
    explicit SeState(hipStream_t s) : key(s), end(s), rid(s), local(s), perm(s), head(s), orank(s) {}
};

// Steps 1 to 3 up to the number of records: d_find_offsets (M + 1) and F.R are always produced. *bad as sh_run. Synchronises `s`.
static hipError_t se_run(aix_index* h, const uint8_t* d_seqs, const uint64_t* d_offs, uint64_t M, uint32_t ed, uint64_t step, uint64_t m, uint64_t* d_find_offsets,
                         SeState& F, bool* bad, hipStream_t s) {
    F.S = F.R = 0;
    ShBufs B(s);
    DevArr soff(s), keep(s), hseq(s), srank(s), ts(s), ckey(s), csrc(s), kout(s), kin(s), pa(s), tmp(s), ts2(s);
    AIX_TRY(sh_alloc(soff, M + 1, 8));
    AIX_TRY(sh_run(h, d_seqs, d_offs, M, m, (uint64_t*)soff.p, nullptr, false, B, bad, s, step, false));   // the interval is that of the seed: phase 1 finds it
    if (*bad) return hipSuccess;
    const uint64_t T = B.T;
    if (T == 0) return zero_offsets(d_find_offsets, M, s);
    B.koff.drop(); B.woff.drop();
    AIX_TRY(sh_alloc(keep, T + 1, 1));
    AIX_TRY(sh_alloc(F.key, T, 8));
    AIX_TRY(sh_alloc(hseq, T, 8));
    AIX_TRY(sh_alloc(F.end, T, 8));
    AIX_TRY(sh_alloc(F.rid, T, 8));
    AIX_TRY(sh_alloc(F.local, T, 8));
    AIX_TRY(sh_alloc(srank, T + 1, 8));
    AIX_TRY(hipMemsetAsync((uint8_t*)keep.p + T, 0, 1, s));
    SeVerify P{};
    P.seqs = d_seqs; P.offs = d_offs; P.soff = (const uint64_t*)soff.p; P.M = M; P.T = T;
    P.pos = (const uint64_t*)B.pos.p; P.qoff = (const uint32_t*)B.qoff.p; P.flag = (const uint8_t*)B.flag.p;
    P.reads = h->att.rd.as<uint8_t>(); P.reads_len = h->att.rd_len;
    P.rs = h->att.rx.as<uint64_t>(); P.re = P.rs + h->att.rx_n; P.rr = P.rs + 2 * h->att.rx_n; P.rn = h->att.rx_n;
    P.ed = ed;
    P.keep = (uint8_t*)keep.p; P.key = (uint64_t*)F.key.p; P.hseq = (uint64_t*)hseq.p; P.end = (uint64_t*)F.end.p; P.rid = (uint64_t*)F.rid.p;
    P.local = (uint64_t*)F.local.p;
    AIX_TRY_LAUNCH(k_se_verify, dim3(flat_grid(T)), dim3(kSB), 0, s, P);
    AIX_TRY(scan_u64(rocprim::make_transform_iterator((const uint8_t*)keep.p, Widen<uint8_t>()), (uint64_t*)srank.p, T + 1, ts, s));
    uint64_t S = 0;               // read back asynchronously: declared after the DevArrs, whose destructors synchronise `s` before an early return leaves the frame
    AIX_TRY(hipMemcpyAsync(&S, (const uint64_t*)srank.p + T, 8, hipMemcpyDeviceToHost, s));
    AIX_TRY(hipStreamSynchronize(s));
    B.pos.drop(); B.qoff.drop(); B.flag.drop();
    if (S == 0) return zero_offsets(d_find_offsets, M, s);
    F.S = S;
    AIX_TRY(sh_alloc(ckey, S, 8));
    AIX_TRY(sh_alloc(csrc, S, 8));
    AIX_TRY(sh_alloc(kout, S, 8));
    AIX_TRY(sh_alloc(kin, S, 8));
    AIX_TRY(sh_alloc(pa, S, 8));
    AIX_TRY(sh_alloc(F.perm, S, 8));
    AIX_TRY(sh_alloc(F.head, S + 1, 1));
    AIX_TRY(sh_alloc(F.orank, S + 1, 8));
    const dim3 blk(kSB), gS(flat_grid(S));
    AIX_TRY_LAUNCH(k_se_compact, dim3(flat_grid(T)), blk, 0, s, (const uint8_t*)keep.p, (const uint64_t*)srank.p, (const uint64_t*)F.key.p, T, (uint64_t*)ckey.p,
                   (uint64_t*)csrc.p);
    // least significant key first: (start, strand, dist, end), then the sequence; start < reads_len, so the key needs the bits of reads_len << 9
    AIX_TRY(sort_pairs((const uint64_t*)ckey.p, (uint64_t*)kout.p, (const uint64_t*)csrc.p, (uint64_t*)pa.p, S, sort_bits((h->att.rd_len << (kSeLowBits + 1)) | 0x1FFull), tmp, s));
    AIX_TRY_LAUNCH((k_sv_gather<uint64_t, SvSame>), gS, blk, 0, s, (const uint64_t*)hseq.p, (const uint64_t*)pa.p, S, SvSame(), (uint64_t*)kin.p);
    AIX_TRY(sort_pairs((const uint64_t*)kin.p, (uint64_t*)kout.p, (const uint64_t*)pa.p, (uint64_t*)F.perm.p, S, sort_bits(M), tmp, s));
    const uint64_t* sseq = (const uint64_t*)kout.p;
    AIX_TRY_LAUNCH(k_se_heads, dim3(flat_grid(S + 1)), blk, 0, s, (const uint64_t*)F.perm.p, sseq, (const uint64_t*)F.key.p, S, (uint8_t*)F.head.p);
    AIX_TRY(scan_u64(rocprim::make_transform_iterator((const uint8_t*)F.head.p, Widen<uint8_t>()), (uint64_t*)F.orank.p, S + 1, ts2, s));
    AIX_TRY(hipMemcpyAsync(&F.R, (const uint64_t*)F.orank.p + S, 8, hipMemcpyDeviceToHost, s));
    AIX_TRY_LAUNCH(k_se_seqoff, dim3(flat_grid(M + 1)), blk, 0, s, sseq, (const uint64_t*)F.orank.p, S, M, d_find_offsets);
    return hipStreamSynchronize(s);
}

// the F.R records into buffers that hold them. Synchronises `s`.
static hipError_t se_write(const SeState& F, const SeOut& O, hipStream_t s) {
    if (F.R == 0) return hipSuccess;
    AIX_TRY_LAUNCH(k_se_write, dim3(flat_grid(F.S)), dim3(kSB), 0, s, (const uint8_t*)F.head.p, (const uint64_t*)F.orank.p, (const uint64_t*)F.perm.p, F.S,
                   (const uint64_t*)F.key.p, (const uint64_t*)F.end.p, (const uint64_t*)F.rid.p, (const uint64_t*)F.local.p, O);
    return hipStreamSynchronize(s);
}

}  // namespace aix

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
using namespace aix;

extern "C" int aix_seq_edit_dev(aix_index_t* h, const char* d_seqs, const uint64_t* d_offs, uint64_t M, uint32_t ed, uint64_t seed_step, uint64_t max_per_kmer,
                                uint64_t* d_find_offsets, uint64_t* d_start, uint64_t* d_end, uint64_t* d_rid, uint64_t* d_local, uint8_t* d_strand, uint32_t* d_dist,
                                uint64_t cap, uint64_t* total_out, void* stream) {
    if (!h || !d_find_offsets || !total_out || (M && !d_offs) || M >= (1ull << 56) || ed > AIX_SEQEDIT_MAX_ED) return AIX_ERR_ARG;
    if (cap && (!d_start || !d_end || !d_rid || !d_local || !d_strand || !d_dist)) return AIX_ERR_ARG;
    if (const int st = sh_check(h)) return st;
    if (h->att.rd_len >= (1ull << 54)) return AIX_ERR_UNSUPPORTED;                 // start << 9 | .. is the sort key
    DevGuard g(h->device);
    hipStream_t s = (hipStream_t)stream;
    *total_out = 0;
    if (M == 0) { AIXCHK(zero_offsets(d_find_offsets, 0, s)); return AIX_OK; }
    SeState F(s);
    bool bad = false;
    AIXCHK(se_run(h, (const uint8_t*)d_seqs, d_offs, M, ed, seed_step ? seed_step : 23, max_per_kmer, d_find_offsets, F, &bad, s));
    if (bad) return AIX_ERR_ARG;
    *total_out = F.R;
    if (F.R && F.R <= cap) AIXCHK(se_write(F, SeOut{d_start, d_end, d_rid, d_local, d_strand, d_dist}, s));
    return AIX_OK;
}

extern "C" int aix_seq_edit(aix_index_t* h, const char* seqs, const uint64_t* offs, uint64_t M, uint32_t ed, uint64_t seed_step, uint64_t max_per_kmer,
                            uint64_t** find_offsets_out, uint64_t** start_out, uint64_t** end_out, uint64_t** rid_out, uint64_t** local_out, uint8_t** strand_out,
                            uint32_t** dist_out) {
    if (!h || !find_offsets_out || !start_out || !end_out || !rid_out || !local_out || !strand_out || !dist_out || (M && !offs) || M >= (1ull << 56) ||
        ed > AIX_SEQEDIT_MAX_ED)
        return AIX_ERR_ARG;
    *find_offsets_out = *start_out = *end_out = *rid_out = *local_out = nullptr; *strand_out = nullptr; *dist_out = nullptr;
    const uint64_t none = 0;
    if (!offs) offs = &none;                                   // M == 0: find_offsets = {0}
    if (M && offs[M] && !seqs) return AIX_ERR_ARG;
    if (const int st = sh_check(h)) return st;
    if (h->att.rd_len >= (1ull << 54)) return AIX_ERR_UNSUPPORTED;
    DevGuard g(h->device);
    DevArr ds, dof, dfo, dp, de, dr, dl, dst, dd;
    if (const int st = sh_upload(seqs, offs, M, ds, dof)) return st;
    AIXCHK(dfo.alloc(8 * (M + 1)));
    AIXCHK(hipMemset(dfo.p, 0, 8 * (M + 1)));
    SeState F(nullptr);
    bool bad = false;
    if (M) AIXCHK(se_run(h, (const uint8_t*)ds.p, (const uint64_t*)dof.p, M, ed, seed_step ? seed_step : 23, max_per_kmer, (uint64_t*)dfo.p, F, &bad, nullptr));
    if (bad) return AIX_ERR_ARG;
    const uint64_t R = F.R;                                    // <= the survivors, whose blocks were allocated: 8 R cannot overflow
    if (R) {
        AIXCHK(dp.alloc(8 * R)); AIXCHK(de.alloc(8 * R)); AIXCHK(dr.alloc(8 * R)); AIXCHK(dl.alloc(8 * R)); AIXCHK(dst.alloc(R)); AIXCHK(dd.alloc(4 * R));
        AIXCHK(se_write(F, SeOut{(uint64_t*)dp.p, (uint64_t*)de.p, (uint64_t*)dr.p, (uint64_t*)dl.p, (uint8_t*)dst.p, (uint32_t*)dd.p}, nullptr));
    }
    const HostOut outs[] = {{(void**)find_offsets_out, dfo.p, 8 * (M + 1)}, {(void**)start_out, dp.p, 8 * R}, {(void**)end_out, de.p, 8 * R},
                            {(void**)rid_out, dr.p, 8 * R},                 {(void**)local_out, dl.p, 8 * R}, {(void**)strand_out, dst.p, R},
                            {(void**)dist_out, dd.p, 4 * R}};
    AIXCHK(copy_out_host(outs, 7));
    return AIX_OK;
}
