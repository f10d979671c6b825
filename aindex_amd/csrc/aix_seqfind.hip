// aix_seqfind.hip — sequences against the indexed reads with mismatches: seed hits -> Hamming-verified alignments, and strand counts of k-mers.
//   iter_reads_by_sequence(seq, aindex, hd)   API_DOCUMENTATION.md:232-255, 371-382   (documented; the reference holds no code for it)
//   get_srandness(kmer, aindex)               API_DOCUMENTATION.md:232-255, 371-382
//   hamming_distance                          aindex.py:44-46                          mismatches, positions with an N on either side ignored
// The loop a caller writes over get_sequence_hits_array, get_reads_batch and hamming_distance, for M sequences at once. The chain:
//   1 sh_run          steps 1 to 4 of aix_seqhits.hip with a window stride: the seeds of a sequence are its windows at offsets 0, step, ..;
//                     their hits (position, window offset, strand flag), contiguous per sequence
//   2 k_sf_verify     THE HOT PATH. Phase 1, one lane per hit: its sequence (bisection of the hit offsets), the proposed start a of the
//                     alignment, the bounds tests, the read interval that contains [a, a + L) (bisection of the interval starts).
//                     Phase 2, kSfLanes lanes per proposal: kSfTrip bytes of the reads against the pattern (or its reverse complement) per
//                     trip, a dword per lane, mismatches summed over the group with ballot + popcount, out once the count exceeds hd.
//                     Then one lane per hit again: coalesced stores of the survivors' keys and columns.
//   3 survivors only  a scan of the keep flags closes the survivors up (stable: hit order, so sequences ascend); two STABLE radix sorts of a
//                     permutation, by (a, strand) and by sequence, each over the bits its key needs; k_sf_heads marks the first entry of
//                     every (sequence, a, strand) run, a scan numbers the records, k_sf_seqoff gives the CSR offsets, k_sf_write the records.
//   strands: the hits of N k-mers as N sequences of 23 bytes, then two scans of the strand flags; a k-mer's counts are differences of the
//            scans at the ends of its hits — a segmented reduction whose cost does not depend on how skewed the lists are.
// Every size, offset and flat index is 64 bits wide; byte counts are checked for overflow before anything is allocated (sh_alloc). No
// atomics; all stores are plain vector stores. Nothing depends on the launch geometry.
#include "aix_seqhits.hpp"

namespace aix {

static constexpr uint32_t kSfLanes = 16;                       // lanes that share one proposed alignment
static constexpr uint32_t kSfGroups = 64 / kSfLanes;           // proposals a wave verifies at a time
static constexpr uint32_t kSfTrip = 4 * kSfLanes;              // bytes of the pattern per trip of the verification loop
static_assert(kSfTrip == AIX_SEQFIND_TRIP_BYTES, "aix_seqhits.hpp names the trip length; _lib.py repeats it for the tests");

// ---------------------------------------------------------------------------------------------
// 2. verification
// ---------------------------------------------------------------------------------------------
struct SfVerify {
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
    uint32_t hd;
    uint8_t* keep;                 // outputs, [T] each: keep for every hit, the others where keep != 0
    uint64_t* key;                 // (a << 1) | strand
    uint64_t* hseq;
    uint64_t* rid;
    uint64_t* local;
    uint32_t* dist;
};

__global__ void __launch_bounds__(kSB) k_sf_verify(const SfVerify P) {
    const uint32_t lane = threadIdx.x & 63u, sub = lane & (kSfLanes - 1u), grp = lane / kSfLanes;
    const uint64_t stride = (uint64_t)gridDim.x * kSB;
    const uint64_t slen = P.offs[P.M];
    for (uint64_t base = (uint64_t)blockIdx.x * kSB + (threadIdx.x & ~63u); base < P.T; base += stride) {    // wave-uniform
        // phase 1: one lane per hit
        const uint64_t e = base + lane;
        bool ok = false;
        uint64_t a = 0, so = 0, sq = 0, rd = 0, sv = 0;
        uint32_t L = 0, strand = 2;
        if (e < P.T) strand = P.flag[e] & 3u;
        if (strand < 2) {
            uint64_t lo = 0, hi = P.M;                         // soff[lo] <= e < soff[hi]: soff[0] == 0, soff[M] == T
            while (hi - lo > 1) {
                const uint64_t mid = lo + ((hi - lo) >> 1);
                if (P.soff[mid] <= e) lo = mid; else hi = mid;
            }
            sq = lo;
            so = P.offs[sq];
            L = (uint32_t)(P.offs[sq + 1] - so);               // < 2^32 (k_sh_windows)
            const uint64_t p = P.pos[e], q = P.qoff[e];
            const uint64_t back = strand == 0 ? q : (uint64_t)L - 23 - q;      // q <= L - 23
            if (p >= back && p - back <= P.reads_len && P.reads_len - (p - back) >= L) {
                a = p - back;
                uint64_t c0 = 0, c1 = P.rn;                    // the intervals with start <= a are [0, c0)
                while (c0 < c1) {
                    const uint64_t mid = c0 + ((c1 - c0) >> 1);
                    if (P.rs[mid] <= a) c0 = mid + 1; else c1 = mid;
                }
                if (c0) {                                      // sorted and disjoint: only the last of them can hold a
                    const uint64_t en = P.re[c0 - 1];
                    sv = P.rs[c0 - 1];
                    if (en >= a && en - a >= L) { ok = true; rd = P.rr[c0 - 1]; }
                }
            }
        }
        // phase 2: round r verifies the proposals of lanes r * kSfGroups .. + kSfGroups - 1, one per group of kSfLanes lanes
        const uint64_t okm = __ballot(ok);
        uint32_t mine = 0;                                     // the mismatch count of this lane's own hit (exact up to hd)
        for (uint32_t r = 0; r < kSfLanes; ++r) {
            if (((okm >> (r * kSfGroups)) & ((1ull << kSfGroups) - 1ull)) == 0) continue;                  // wave-uniform
            const uint32_t src = r * kSfGroups + grp;
            const bool g_ok = (okm >> src) & 1ull;
            const uint64_t g_a = sf_shfl64(a, src), g_so = sf_shfl64(so, src);
            const uint32_t g_L = bperm(src, L), g_strand = bperm(src, strand);
            uint32_t cnt = 0;
            for (uint32_t t0 = 0;; t0 += kSfTrip) {
                const bool run = g_ok && t0 < g_L && cnt <= P.hd;
                if (__ballot(run) == 0) break;                 // wave-uniform
                uint32_t mm = 0;
                const uint32_t j = t0 + 4u * sub;
                if (run && j < g_L) {
                    const uint32_t nv = min(4u, g_L - j);
                    const uint32_t x = sf_load4(P.reads, P.reads_len, (int64_t)(g_a + j));
                    uint32_t y;
                    if (g_strand == 0) {
                        y = sf_load4(P.seqs, slen, (int64_t)(g_so + j));
                    } else {                                   // y_b = comp(seq[L - 1 - j - b]): the dword that ends at L - 1 - j, reversed
                        const uint32_t w = __builtin_bswap32(sf_load4(P.seqs, slen, (int64_t)g_so + (int64_t)g_L - 4 - (int64_t)j));
                        y = sf_comp(w & 0xFFu) | (sf_comp((w >> 8) & 0xFFu) << 8) | (sf_comp((w >> 16) & 0xFFu) << 16) | (sf_comp(w >> 24) << 24);
                    }
#pragma unroll
                    for (uint32_t b = 0; b < 4; ++b) {
                        const uint32_t xb = (x >> (8 * b)) & 0xFFu, yb = (y >> (8 * b)) & 0xFFu;
                        if (b < nv && xb != yb && xb != 'N' && yb != 'N') mm |= 1u << b;
                    }
                }
#pragma unroll
                for (uint32_t b = 0; b < 4; ++b) {
                    const uint64_t m = __ballot((mm >> b) & 1u);
                    cnt += (uint32_t)__popcll((m >> (grp * kSfLanes)) & ((1ull << kSfLanes) - 1ull));
                }
            }
            const uint32_t back = bperm((lane % kSfGroups) * kSfLanes, cnt);   // the group that verified this lane's hit in round lane / kSfGroups
            if (lane / kSfGroups == r) mine = back;
        }
        if (e < P.T) {
            const bool kept = ok && mine <= P.hd;
            P.keep[e] = kept ? 1 : 0;
            if (kept) {
                P.key[e] = (a << 1) | strand;
                P.hseq[e] = sq;
                P.rid[e] = rd;
                P.local[e] = a - sv;
                P.dist[e] = mine;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// 3. the survivors: closed up, sorted, made unique, written
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSB) k_sf_compact(const uint8_t* __restrict__ keep, const uint64_t* __restrict__ srank, const uint64_t* __restrict__ key, uint64_t T,
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

// head[i] = sorted survivor i opens a (sequence, a, strand) run; head[S] = 0
__global__ void __launch_bounds__(kSB) k_sf_heads(const uint64_t* __restrict__ perm, const uint64_t* __restrict__ sseq, const uint64_t* __restrict__ key, uint64_t S,
                                                 uint8_t* __restrict__ head) {
    const uint64_t stride = (uint64_t)gridDim.x * kSB;
    for (uint64_t i = (uint64_t)blockIdx.x * kSB + threadIdx.x; i <= S; i += stride)
        head[i] = (i < S && (i == 0 || sseq[i - 1] != sseq[i] || key[perm[i - 1]] != key[perm[i]])) ? 1 : 0;
}

// find_offsets[i] = records of the sequences before i: the record that the first sorted survivor of a sequence >= i opens
__global__ void __launch_bounds__(kSB) k_sf_seqoff(const uint64_t* __restrict__ sseq, const uint64_t* __restrict__ orank, uint64_t S, uint64_t M,
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

struct SfOut {
    uint64_t *pos, *rid, *local;
    uint8_t* strand;
    uint32_t* dist;
};
__global__ void __launch_bounds__(kSB) k_sf_write(const uint8_t* __restrict__ head, const uint64_t* __restrict__ orank, const uint64_t* __restrict__ perm, uint64_t S,
                                                 const uint64_t* __restrict__ key, const uint64_t* __restrict__ rid, const uint64_t* __restrict__ local,
                                                 const uint32_t* __restrict__ dist, const SfOut O) {
    const uint64_t stride = (uint64_t)gridDim.x * kSB;
    for (uint64_t i = (uint64_t)blockIdx.x * kSB + threadIdx.x; i < S; i += stride) {
        if (!head[i]) continue;
        const uint64_t o = orank[i], e = perm[i], k = key[e];  // every entry of a run carries the same columns: the first one speaks
        O.pos[o] = k >> 1;
        O.rid[o] = rid[e];
        O.local[o] = local[e];
        O.strand[o] = (uint8_t)(k & 1u);
        O.dist[o] = dist[e];
    }
}

// what a call holds between sizing and writing
struct SfState {
    DevArr key, rid, local, dist, perm, head, orank;
    uint64_t S = 0, R = 0;
    explicit SfState(hipStream_t s) : key(s), rid(s), local(s), dist(s), perm(s), head(s), orank(s) {}
};

// Steps 1 to 3 up to the number of records: d_find_offsets (M + 1) and F.R are always produced. *bad as sh_run. Synchronises `s`.
static hipError_t sf_run(aix_index* h, const uint8_t* d_seqs, const uint64_t* d_offs, uint64_t M, uint32_t hd, uint64_t step, uint64_t m, uint64_t* d_find_offsets,
                         SfState& F, bool* bad, hipStream_t s) {
    F.S = F.R = 0;
    ShBufs B(s);
    DevArr soff(s), keep(s), hseq(s), srank(s), ts(s), ckey(s), csrc(s), kout(s), kin(s), pa(s), tmp(s), ts2(s);
    AIX_TRY(sh_alloc(soff, M + 1, 8));
    AIX_TRY(sh_run(h, d_seqs, d_offs, M, m, (uint64_t*)soff.p, nullptr, false, B, bad, s, step, false));   // containment here is not the interval rule of the hits
    if (*bad) return hipSuccess;
    const uint64_t T = B.T;
    if (T == 0) return zero_offsets(d_find_offsets, M, s);
    B.koff.drop(); B.woff.drop();
    AIX_TRY(sh_alloc(keep, T + 1, 1));
    AIX_TRY(sh_alloc(F.key, T, 8));
    AIX_TRY(sh_alloc(hseq, T, 8));
    AIX_TRY(sh_alloc(F.rid, T, 8));
    AIX_TRY(sh_alloc(F.local, T, 8));
    AIX_TRY(sh_alloc(F.dist, T, 4));
    AIX_TRY(sh_alloc(srank, T + 1, 8));
    AIX_TRY(hipMemsetAsync((uint8_t*)keep.p + T, 0, 1, s));
    SfVerify P{};
    P.seqs = d_seqs; P.offs = d_offs; P.soff = (const uint64_t*)soff.p; P.M = M; P.T = T;
    P.pos = (const uint64_t*)B.pos.p; P.qoff = (const uint32_t*)B.qoff.p; P.flag = (const uint8_t*)B.flag.p;
    P.reads = h->att.rd.as<uint8_t>(); P.reads_len = h->att.rd_len;
    P.rs = h->att.rx.as<uint64_t>(); P.re = P.rs + h->att.rx_n; P.rr = P.rs + 2 * h->att.rx_n; P.rn = h->att.rx_n;
    P.hd = hd;
    P.keep = (uint8_t*)keep.p; P.key = (uint64_t*)F.key.p; P.hseq = (uint64_t*)hseq.p; P.rid = (uint64_t*)F.rid.p; P.local = (uint64_t*)F.local.p;
    P.dist = (uint32_t*)F.dist.p;
    AIX_TRY_LAUNCH(k_sf_verify, dim3(flat_grid(T)), dim3(kSB), 0, s, P);
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
    AIX_TRY_LAUNCH(k_sf_compact, dim3(flat_grid(T)), blk, 0, s, (const uint8_t*)keep.p, (const uint64_t*)srank.p, (const uint64_t*)F.key.p, T, (uint64_t*)ckey.p,
                   (uint64_t*)csrc.p);
    // least significant key first: (a, strand), then the sequence; a <= reads_len, so the key needs the bits of 2 reads_len + 1
    AIX_TRY(sort_pairs((const uint64_t*)ckey.p, (uint64_t*)kout.p, (const uint64_t*)csrc.p, (uint64_t*)pa.p, S, sort_bits((h->att.rd_len << 1) | 1ull), tmp, s));
    AIX_TRY_LAUNCH((k_sv_gather<uint64_t, SvSame>), gS, blk, 0, s, (const uint64_t*)hseq.p, (const uint64_t*)pa.p, S, SvSame(), (uint64_t*)kin.p);
    AIX_TRY(sort_pairs((const uint64_t*)kin.p, (uint64_t*)kout.p, (const uint64_t*)pa.p, (uint64_t*)F.perm.p, S, sort_bits(M), tmp, s));
    const uint64_t* sseq = (const uint64_t*)kout.p;
    AIX_TRY_LAUNCH(k_sf_heads, dim3(flat_grid(S + 1)), blk, 0, s, (const uint64_t*)F.perm.p, sseq, (const uint64_t*)F.key.p, S, (uint8_t*)F.head.p);
    AIX_TRY(scan_u64(rocprim::make_transform_iterator((const uint8_t*)F.head.p, Widen<uint8_t>()), (uint64_t*)F.orank.p, S + 1, ts2, s));
    AIX_TRY(hipMemcpyAsync(&F.R, (const uint64_t*)F.orank.p + S, 8, hipMemcpyDeviceToHost, s));
    AIX_TRY_LAUNCH(k_sf_seqoff, dim3(flat_grid(M + 1)), blk, 0, s, sseq, (const uint64_t*)F.orank.p, S, M, d_find_offsets);
    return hipStreamSynchronize(s);
}

// the F.R records into buffers that hold them. Synchronises `s`.
static hipError_t sf_write(const SfState& F, const SfOut& O, hipStream_t s) {
    if (F.R == 0) return hipSuccess;
    AIX_TRY_LAUNCH(k_sf_write, dim3(flat_grid(F.S)), dim3(kSB), 0, s, (const uint8_t*)F.head.p, (const uint64_t*)F.orank.p, (const uint64_t*)F.perm.p, F.S,
                   (const uint64_t*)F.key.p, (const uint64_t*)F.rid.p, (const uint64_t*)F.local.p, (const uint32_t*)F.dist.p, O);
    return hipStreamSynchronize(s);
}

// ---------------------------------------------------------------------------------------------
// strand counts
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSB) k_ks_offs(uint64_t N, uint64_t* __restrict__ offs) {
    const uint64_t stride = (uint64_t)gridDim.x * kSB;
    for (uint64_t i = (uint64_t)blockIdx.x * kSB + threadIdx.x; i <= N; i += stride) offs[i] = 23 * i;
}

struct KsIsStrand {
    uint8_t want;
    __host__ __device__ uint64_t operator()(uint8_t f) const { return (f & 3u) == want ? 1ull : 0ull; }
};

// sp / sm: [T] hits with strand 0 / 1 before hit e (exclusive scans of the T flags; all three null when T == 0). The count before the end T
// is the last entry plus what the last flag adds.
__global__ void __launch_bounds__(kSB) k_ks_counts(const uint64_t* __restrict__ soff, const uint64_t* __restrict__ sp, const uint64_t* __restrict__ sm,
                                                  const uint8_t* __restrict__ flag, uint64_t T, uint64_t N, uint64_t* __restrict__ plus, uint64_t* __restrict__ minus,
                                                  uint64_t* __restrict__ total) {
    const uint64_t stride = (uint64_t)gridDim.x * kSB;
    for (uint64_t i = (uint64_t)blockIdx.x * kSB + threadIdx.x; i < N; i += stride) {
        const uint64_t a = soff[i], b = soff[i + 1];           // a <= b <= T
        uint64_t p = 0, m = 0;
        if (b > a) {                                           // so T > 0 and a < T
            const uint32_t last = flag[T - 1] & 3u;
            p = (b < T ? sp[b] : sp[T - 1] + (last == 0)) - sp[a];
            m = (b < T ? sm[b] : sm[T - 1] + (last == 1)) - sm[a];
        }
        plus[i] = p;
        minus[i] = m;
        total[i] = b - a;
    }
}

static hipError_t ks_run(aix_index* h, const uint8_t* d_kmers, uint64_t N, uint64_t m, uint64_t* d_plus, uint64_t* d_minus, uint64_t* d_total, hipStream_t s) {
    ShBufs B(s);
    DevArr offs(s), soff(s), sp(s), sm(s), t0(s), t1(s);
    AIX_TRY(sh_alloc(offs, N + 1, 8));
    AIX_TRY(sh_alloc(soff, N + 1, 8));
    AIX_TRY_LAUNCH(k_ks_offs, dim3(flat_grid(N + 1)), dim3(kSB), 0, s, N, (uint64_t*)offs.p);
    bool bad = false;
    AIX_TRY(sh_run(h, d_kmers, (const uint64_t*)offs.p, N, m, (uint64_t*)soff.p, nullptr, false, B, &bad, s, 1, false));
    if (bad) return hipErrorInvalidValue;                      // 23-byte sequences cannot be: kept for the day they can
    const uint64_t T = B.T;
    if (T) {
        B.pos.drop(); B.qoff.drop();
        AIX_TRY(sh_alloc(sp, T, 8));
        AIX_TRY(sh_alloc(sm, T, 8));
        AIX_TRY(scan_u64(rocprim::make_transform_iterator((const uint8_t*)B.flag.p, KsIsStrand{0}), (uint64_t*)sp.p, T, t0, s));
        AIX_TRY(scan_u64(rocprim::make_transform_iterator((const uint8_t*)B.flag.p, KsIsStrand{1}), (uint64_t*)sm.p, T, t1, s));
    }
    AIX_TRY_LAUNCH(k_ks_counts, dim3(flat_grid(N)), dim3(kSB), 0, s, (const uint64_t*)soff.p, (const uint64_t*)sp.p, (const uint64_t*)sm.p,
                   (const uint8_t*)B.flag.p, T, N, d_plus, d_minus, d_total);
    return hipStreamSynchronize(s);
}

}  // namespace aix

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
using namespace aix;

extern "C" int aix_seq_find_dev(aix_index_t* h, const char* d_seqs, const uint64_t* d_offs, uint64_t M, uint32_t hd, uint64_t seed_step, uint64_t max_per_kmer,
                                uint64_t* d_find_offsets, uint64_t* d_pos, uint64_t* d_rid, uint64_t* d_local, uint8_t* d_strand, uint32_t* d_dist, uint64_t cap,
                                uint64_t* total_out, void* stream) {
    if (!h || !d_find_offsets || !total_out || (M && !d_offs) || M >= (1ull << 56)) return AIX_ERR_ARG;
    if (cap && (!d_pos || !d_rid || !d_local || !d_strand || !d_dist)) return AIX_ERR_ARG;
    if (const int st = sh_check(h)) return st;
    if (h->att.rd_len >= (1ull << 62)) return AIX_ERR_UNSUPPORTED;                 // (a << 1) | strand is the sort key
    DevGuard g(h->device);
    hipStream_t s = (hipStream_t)stream;
    *total_out = 0;
    if (M == 0) { AIXCHK(zero_offsets(d_find_offsets, 0, s)); return AIX_OK; }
    SfState F(s);
    bool bad = false;
    AIXCHK(sf_run(h, (const uint8_t*)d_seqs, d_offs, M, hd, seed_step ? seed_step : 23, max_per_kmer, d_find_offsets, F, &bad, s));
    if (bad) return AIX_ERR_ARG;
    *total_out = F.R;
    if (F.R && F.R <= cap) AIXCHK(sf_write(F, SfOut{d_pos, d_rid, d_local, d_strand, d_dist}, s));
    return AIX_OK;
}

extern "C" int aix_seq_find(aix_index_t* h, const char* seqs, const uint64_t* offs, uint64_t M, uint32_t hd, uint64_t seed_step, uint64_t max_per_kmer,
                            uint64_t** find_offsets_out, uint64_t** pos_out, uint64_t** rid_out, uint64_t** local_out, uint8_t** strand_out, uint32_t** dist_out) {
    if (!h || !find_offsets_out || !pos_out || !rid_out || !local_out || !strand_out || !dist_out || !offs || M >= (1ull << 56)) return AIX_ERR_ARG;
    *find_offsets_out = *pos_out = *rid_out = *local_out = nullptr; *strand_out = nullptr; *dist_out = nullptr;
    if (M && offs[M] && !seqs) return AIX_ERR_ARG;
    if (const int st = sh_check(h)) return st;
    if (h->att.rd_len >= (1ull << 62)) return AIX_ERR_UNSUPPORTED;
    DevGuard g(h->device);
    DevArr ds, dof, dfo, dp, dr, dl, dst, dd;
    if (const int st = sh_upload(seqs, offs, M, ds, dof)) return st;
    AIXCHK(dfo.alloc(8 * (M + 1)));
    AIXCHK(hipMemset(dfo.p, 0, 8 * (M + 1)));
    SfState F(nullptr);
    bool bad = false;
    if (M) AIXCHK(sf_run(h, (const uint8_t*)ds.p, (const uint64_t*)dof.p, M, hd, seed_step ? seed_step : 23, max_per_kmer, (uint64_t*)dfo.p, F, &bad, nullptr));
    if (bad) return AIX_ERR_ARG;
    const uint64_t R = F.R;                                    // <= the survivors, whose blocks were allocated: 8 R cannot overflow
    if (R) {
        AIXCHK(dp.alloc(8 * R)); AIXCHK(dr.alloc(8 * R)); AIXCHK(dl.alloc(8 * R)); AIXCHK(dst.alloc(R)); AIXCHK(dd.alloc(4 * R));
        AIXCHK(sf_write(F, SfOut{(uint64_t*)dp.p, (uint64_t*)dr.p, (uint64_t*)dl.p, (uint8_t*)dst.p, (uint32_t*)dd.p}, nullptr));
    }
    const HostOut outs[] = {{(void**)find_offsets_out, dfo.p, 8 * (M + 1)}, {(void**)pos_out, dp.p, 8 * R}, {(void**)rid_out, dr.p, 8 * R},
                            {(void**)local_out, dl.p, 8 * R},               {(void**)strand_out, dst.p, R}, {(void**)dist_out, dd.p, 4 * R}};
    AIXCHK(copy_out_host(outs, 6));
    return AIX_OK;
}

extern "C" int aix_kmer_strands_dev(aix_index_t* h, const char* d_kmers, uint64_t N, uint64_t max_per_kmer, uint64_t* d_plus, uint64_t* d_minus, uint64_t* d_total,
                                    void* stream) {
    if (!h || (N && (!d_kmers || !d_plus || !d_minus || !d_total)) || N >= (1ull << 56)) return AIX_ERR_ARG;
    if (const int st = sh_check(h)) return st;
    if (N == 0) return AIX_OK;
    DevGuard g(h->device);
    AIXCHK(ks_run(h, (const uint8_t*)d_kmers, N, max_per_kmer, d_plus, d_minus, d_total, (hipStream_t)stream));
    return AIX_OK;
}

extern "C" int aix_kmer_strands(aix_index_t* h, const char* kmers, uint64_t N, uint64_t max_per_kmer, uint64_t* plus_out, uint64_t* minus_out, uint64_t* total_out) {
    if (!h || (N && (!kmers || !plus_out || !minus_out || !total_out)) || N >= (1ull << 56)) return AIX_ERR_ARG;
    if (const int st = sh_check(h)) return st;
    if (N == 0) return AIX_OK;
    DevGuard g(h->device);
    DevArr dq, dc;
    AIXCHK(upload_padded(dq, kmers, 23 * N));
    AIXCHK(dc.alloc(24 * N));
    uint64_t* c = (uint64_t*)dc.p;
    AIXCHK(ks_run(h, (const uint8_t*)dq.p, N, max_per_kmer, c, c + N, c + 2 * N, nullptr));
    AIXCHK(hipMemcpy(plus_out, c, 8 * N, hipMemcpyDeviceToHost));
    AIXCHK(hipMemcpy(minus_out, c + N, 8 * N, hipMemcpyDeviceToHost));
    AIXCHK(hipMemcpy(total_out, c + 2 * N, 8 * N, hipMemcpyDeviceToHost));
    return AIX_OK;
}
