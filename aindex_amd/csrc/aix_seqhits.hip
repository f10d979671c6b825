// aix_seqhits.hip — sequences against the indexed reads: seed hits with strand, and votes per (read, strand, diagonal).
//   AindexWrapper::get_positions         python_wrapper.cpp:800-831   one call per 23-window of a sequence
//   AindexWrapper::get_rid / get_start   python_wrapper.cpp:757-789   one call per occurrence
//   AindexWrapper::get_read              python_wrapper.cpp:677-698   23 bytes per occurrence, to tell the strand (a bucket of the positions
//                                                                     index holds both orientations of its k-mer without a strand bit)
// The composition a user of the reference writes as a Python loop over the windows of a sequence, for M sequences at once. The chain:
//   1 k_sh_windows   one lane per sequence: its windows max(0, L - 22) (every `step`-th of them when aix_seqfind.hip asks: offsets 0, step, ..);
//                    a scan gives woff[M + 1], the FLAT window space of W windows
//   2 k_sh_resolve*  one lane per window: the 23 raw bytes at their place in the sequence -> bucket -> (source start, upper bound) through
//                    pq_resolve23_words, the body of k_pq_resolve23 (no N x 23 copy of the windows exists anywhere)
//   3 posquery_lists steps 2 to 5 of aix_posquery.hip, unchanged: W lists -> koff[W + 1] and the positions, windows in sequence order,
//                    so the hits of a sequence are contiguous and ordered by window, then by slot
//   4 k_sh_hits      one lane per hit: its window (wave-wide search for the wave's first hit, then a gallop), the window's bytes again, the
//                    23 bytes of the reads at the position (only when they lie inside the attached buffer), the strand by byte comparison,
//                    the interval by bisection; the votes form also writes the hit's sequence and diagonal
//   votes: 5 a reduction gives the range of the diagonals and the largest read id; four STABLE radix sorts of a permutation of the hits, by
//            diagonal, strand, read id, sequence (least significant first), each over the bits its key needs
//          6 k_sv_heads marks the first hit of every (sequence, read, strand, diagonal) run; a scan numbers the groups, k_sv_starts notes
//            where each begins, k_sv_emit flags those with >= min_votes hits, a scan places them, k_sv_write writes one record per group.
//            The sorts are stable and the hits of a sequence are in window order, so the first and last hit of a run carry q_first / q_last.
// Every size, offset and flat index is 64 bits wide; byte counts are checked for overflow before anything is allocated. No atomics; all
// stores are plain vector stores. Nothing depends on the launch geometry.
#include "aix_seqhits.hpp"

namespace aix {

// ---------------------------------------------------------------------------------------------
// 1 / 2. sequences -> windows -> lists
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSB) k_sh_windows(const uint64_t* __restrict__ offs, uint64_t M, uint64_t step, uint64_t* __restrict__ nwin, uint32_t* __restrict__ flag) {
    const uint64_t stride = (uint64_t)gridDim.x * kSB;
    bool bad = false;
    for (uint64_t i = (uint64_t)blockIdx.x * kSB + threadIdx.x; i <= M; i += stride) {
        uint64_t w = 0;
        if (i < M) {
            const uint64_t a = offs[i], b = offs[i + 1];
            bad |= b < a || b - a >= (1ull << 32);                // query offsets are u32
            if (b >= a && b - a >= 23) w = (b - a - 23) / step + 1;                // windows at offsets 0, step, 2 step, .. <= L - 23
        }
        nwin[i] = w;                                              // nwin[M] = 0: the scan's last entry is the total
    }
    if (bad) *flag = 1u;
}

// the last j in [from, n) with a[j] <= key; a[from] <= key < a[n]. A gallop from `from`, then a bisection.
__device__ __forceinline__ uint64_t sh_last_le(const uint64_t* __restrict__ a, uint64_t n, uint64_t from, uint64_t key) {
    uint64_t lo = from, step = 1, hi;
    for (;;) {
        hi = n - lo > step ? lo + step : n;
        if (hi == n || a[hi] > key) break;
        lo = hi;
        step <<= 1;
    }
    while (hi - lo > 1) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] <= key) lo = mid; else hi = mid;
    }
    return lo;
}

template <int LPP>
__global__ void __launch_bounds__(kSB) k_sh_resolve(const IndexDev ix, const uint8_t* __restrict__ seqs, const uint64_t* __restrict__ offs,
                                                   const uint64_t* __restrict__ woff, uint64_t M, uint64_t W, uint64_t step, const uint64_t* __restrict__ indices,
                                                   uint64_t total, uint64_t* __restrict__ wseq, uint64_t* __restrict__ wsrc, uint64_t* __restrict__ lo_out,
                                                   uint64_t* __restrict__ ub_out) {
    const uint64_t stride = (uint64_t)gridDim.x * kSB;
    for (uint64_t base = (uint64_t)blockIdx.x * kSB + (threadIdx.x & ~63u); base < W; base += stride) {      // wave-uniform
        const uint64_t i = base + (threadIdx.x & 63u);
        const bool in = i < W;
        const uint64_t s0 = wave_count_le(woff, M + 1, base) - 1;            // woff[0] == 0: the last sequence that starts at or before window `base`
        uint64_t w0 = 0, w1 = 0, w2 = 0, sq = 0, src = 0;
        if (in) {
            sq = sh_last_le(woff, M, s0, i);                                 // woff[M] == W > i; a sequence without windows is never the last one <= i
            src = offs[sq] + (i - woff[sq]) * step;
            load23(seqs + src, w0, w1, w2);
        }
        uint64_t lo, ub;
        pq_resolve23_words<LPP>(ix, in, w0, w1, w2, indices, total, lo, ub);
        if (in) {
            wseq[i] = sq;
            wsrc[i] = src;
            lo_out[i] = lo;
            ub_out[i] = ub;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// 4. the hits
// ---------------------------------------------------------------------------------------------
struct ShHits {
    const uint8_t* seqs;
    const uint64_t *woff, *koff, *wseq, *wsrc;     // [M + 1], [W + 1], [W], [W]
    const uint64_t* pos;                           // [T]
    uint64_t M, W, T, step;
    const uint8_t* reads;
    uint64_t reads_len;
    const uint64_t *rs, *re, *rr;                  // interval starts / ends / rids
    uint64_t rn;
    uint32_t* qoff;                                // outputs, [T] each
    uint64_t* rid;
    int64_t* local;
    uint8_t* flag;
    uint64_t* hseq;                                // votes only (else null): the hit's sequence, M when the hit is not kept
    int64_t* diag;                                 // votes only: its diagonal (0 when not kept)
};

// reads[pos .. pos + 23) as the words of load23, or false when the span does not lie inside the buffer. load23 reads whole aligned dwords, up
// to three bytes before and behind the span: near either end of the buffer the bytes are fetched one by one.
__device__ __forceinline__ bool sh_read23(const uint8_t* __restrict__ rd, uint64_t size, uint64_t p, uint64_t& w0, uint64_t& w1, uint64_t& w2) {
    w0 = w1 = w2 = 0;
    if (p > size || size - p < 23) return false;
    if (p >= 3 && size - p >= 26) {
        load23(rd + p, w0, w1, w2);
    } else {
        for (int b = 0; b < 8; ++b) w0 |= (uint64_t)rd[p + b] << (8 * b);
        for (int b = 0; b < 8; ++b) w1 |= (uint64_t)rd[p + 8 + b] << (8 * b);
        for (int b = 0; b < 7; ++b) w2 |= (uint64_t)rd[p + 16 + b] << (8 * b);
    }
    return true;
}

// kLocate false (aix_seqfind.hip, which has an interval rule of its own): no interval search, rid / local not written, flag = the strand alone
template <bool kLocate>
__global__ void __launch_bounds__(kSB) k_sh_hits(const ShHits P) {
    const uint64_t stride = (uint64_t)gridDim.x * kSB;
    for (uint64_t base = (uint64_t)blockIdx.x * kSB + (threadIdx.x & ~63u); base < P.T; base += stride) {    // wave-uniform
        const uint64_t e = base + (threadIdx.x & 63u);
        const uint64_t wv = wave_count_le(P.koff, P.W + 1, base) - 1;        // koff[0] == 0
        if (e >= P.T) continue;
        const uint64_t w = sh_last_le(P.koff, P.W, wv, e);                   // koff[W] == T > e; a window without hits is never the last one <= e
        const uint64_t sq = P.wseq[w], q = (w - P.woff[sq]) * P.step, p = P.pos[e];
        uint64_t w0, w1, w2, r0, r1, r2, t0, t1, t2;
        load23(P.seqs + P.wsrc[w], w0, w1, w2);
        ascii23_of_rc(encode23_words(w0, w1, w2).code, r0, r1, r2);          // decode(reverseDNA(sanitised code))
        uint32_t strand = 2;
        if (sh_read23(P.reads, P.reads_len, p, t0, t1, t2)) {
            if (t0 == w0 && t1 == w1 && t2 == w2) strand = 0;
            else if (t0 == r0 && t1 == r1 && t2 == r2) strand = 1;
        }
        P.qoff[e] = (uint32_t)q;
        if constexpr (!kLocate) {
            P.flag[e] = (uint8_t)strand;
            continue;
        }
        uint64_t rd, sv;
        const bool found = pq_locate(P.rs, P.re, P.rr, P.rn, p, rd, sv);
        const int64_t local = (int64_t)(p - sv);
        P.rid[e] = rd;
        P.local[e] = local;
        P.flag[e] = (uint8_t)(strand | (found ? 4u : 0u));
        if (P.hseq) {
            const bool keep = found && strand < 2;
            P.hseq[e] = keep ? sq : P.M;
            P.diag[e] = keep ? (strand == 0 ? local - (int64_t)q : local + (int64_t)q) : 0;
        }
    }
}

// seq_offsets[i] = hits before the first window of sequence i
__global__ void __launch_bounds__(kSB) k_sh_seqoff(const uint64_t* __restrict__ woff, const uint64_t* __restrict__ koff, uint64_t M, uint64_t* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * kSB;
    for (uint64_t i = (uint64_t)blockIdx.x * kSB + threadIdx.x; i <= M; i += stride) out[i] = koff[woff[i]];
}

// Steps 1 to 4 (declared in aix_seqhits.hpp; aix_seqfind.hip runs them with a window stride). B.woff and (W != 0) B.koff are always produced and d_seq_offsets (M + 1, nullable) filled; the hits go to `user` when
// they fit its cap, or — user == nullptr — to pool blocks of B; votes: hseq / diag as well; locate false (pool blocks, no votes): without rid / local and the located bit of the flag. *bad: a sequence of 2^32 bytes or more,
// descending offsets, or windows without a byte buffer (nothing else is produced then). Synchronises `s`.
hipError_t sh_run(aix_index* h, const uint8_t* d_seqs, const uint64_t* d_offs, uint64_t M, uint64_t m, uint64_t* d_seq_offsets, const ShUser* user, bool votes, ShBufs& B,
                  bool* bad, hipStream_t s, uint64_t step, bool locate) {
    *bad = false;
    B.W = B.T = 0;
    DevArr nwin(s), fl(s), tmp(s), lo(s), ub(s), wseq(s), wsrc(s);
    AIX_TRY(sh_alloc(nwin, M + 1, 8));
    AIX_TRY(sh_alloc(B.woff, M + 1, 8));
    AIX_TRY(fl.alloc(4));
    AIX_TRY(hipMemsetAsync(fl.p, 0, 4, s));
    AIX_TRY_LAUNCH(k_sh_windows, dim3(flat_grid(M + 1)), dim3(kSB), 0, s, d_offs, M, step, (uint64_t*)nwin.p, (uint32_t*)fl.p);
    AIX_TRY(scan_u64((const uint64_t*)nwin.p, (uint64_t*)B.woff.p, M + 1, tmp, s));
    uint64_t W = 0;               // read back asynchronously: declared after the DevArrs, whose destructors synchronise `s` before an early return leaves the frame
    uint32_t flag = 0;
    AIX_TRY(hipMemcpyAsync(&W, (const uint64_t*)B.woff.p + M, 8, hipMemcpyDeviceToHost, s));
    AIX_TRY(hipMemcpyAsync(&flag, fl.p, 4, hipMemcpyDeviceToHost, s));
    AIX_TRY(hipStreamSynchronize(s));
    if (flag || (W && !d_seqs)) { *bad = true; return hipSuccess; }     // (no bytes are needed when no sequence has a window: M empty sequences)
    B.W = W;
    if (W == 0) return d_seq_offsets ? zero_offsets(d_seq_offsets, M, s) : hipStreamSynchronize(s);
    AIX_TRY(sh_alloc(lo, W, 8));
    AIX_TRY(sh_alloc(ub, W + 1, 8));
    AIX_TRY(sh_alloc(wseq, W, 8));
    AIX_TRY(sh_alloc(wsrc, W, 8));
    AIX_TRY(sh_alloc(B.koff, W + 1, 8));
    AIX_TRY(hipMemsetAsync((uint64_t*)ub.p + W, 0, 8, s));
    const IndexDev ix = h->dev();
    const uint64_t* woff = (const uint64_t*)B.woff.p;
#define AIX_SH_RESOLVE(L)                                                                                                                              \
    AIX_TRY_LAUNCH(k_sh_resolve<L>, dim3(flat_grid(W)), dim3(kSB), 0, s, ix, d_seqs, d_offs, woff, M, W, step, h->att.ai_indices.as<uint64_t>(), h->att.ai_total, (uint64_t*)wseq.p, \
                   (uint64_t*)wsrc.p, (uint64_t*)lo.p, (uint64_t*)ub.p)
    if (ix.bk_lpp == 2) AIX_SH_RESOLVE(2);
    else if (ix.bk_lpp == 4) AIX_SH_RESOLVE(4);
    else AIX_SH_RESOLVE(8);
#undef AIX_SH_RESOLVE
    uint64_t T = 0;
    AIX_TRY(posquery_lists(h, (const uint64_t*)lo.p, (const uint64_t*)ub.p, W, m, (uint64_t*)B.koff.p, user ? user->pos : nullptr, nullptr, nullptr, user ? user->cap : 0, &T, s,
                           user ? nullptr : &B.pos));
    B.T = T;
    if (d_seq_offsets) AIX_TRY_LAUNCH(k_sh_seqoff, dim3(flat_grid(M + 1)), dim3(kSB), 0, s, woff, (const uint64_t*)B.koff.p, M, d_seq_offsets);
    if (T && (!user || (T <= user->cap && user->pos))) {
        ShHits P{};
        P.seqs = d_seqs; P.woff = woff; P.koff = (const uint64_t*)B.koff.p; P.wseq = (const uint64_t*)wseq.p; P.wsrc = (const uint64_t*)wsrc.p;
        P.M = M; P.W = W; P.T = T; P.step = step;
        P.reads = h->att.rd.as<uint8_t>(); P.reads_len = h->att.rd_len;
        P.rs = h->att.rx.as<uint64_t>(); P.re = P.rs + h->att.rx_n; P.rr = P.rs + 2 * h->att.rx_n; P.rn = h->att.rx_n;
        if (user) {
            P.pos = user->pos; P.qoff = user->qoff; P.rid = user->rid; P.local = user->local; P.flag = user->flag;
        } else {
            AIX_TRY(sh_alloc(B.qoff, T, 4));
            if (locate) AIX_TRY(sh_alloc(B.rid, T, 8));
            if (locate) AIX_TRY(sh_alloc(B.local, T, 8));
            AIX_TRY(sh_alloc(B.flag, T, 1));
            if (votes) AIX_TRY(sh_alloc(B.hseq, T, 8));
            if (votes) AIX_TRY(sh_alloc(B.diag, T, 8));
            P.pos = (const uint64_t*)B.pos.p; P.qoff = (uint32_t*)B.qoff.p; P.rid = (uint64_t*)B.rid.p; P.local = (int64_t*)B.local.p; P.flag = (uint8_t*)B.flag.p;
            P.hseq = (uint64_t*)B.hseq.p; P.diag = (int64_t*)B.diag.p;
        }
        if (locate) AIX_TRY_LAUNCH(k_sh_hits<true>, dim3(flat_grid(T)), dim3(kSB), 0, s, P);
        else AIX_TRY_LAUNCH(k_sh_hits<false>, dim3(flat_grid(T)), dim3(kSB), 0, s, P);
    }
    return hipStreamSynchronize(s);                            // the scratch blocks go back to the pool idle
}

// ---------------------------------------------------------------------------------------------
// 5 / 6. votes
// ---------------------------------------------------------------------------------------------
struct SvRange {                   // over the kept hits: smallest and largest diagonal, largest read id
    int64_t dlo, dhi;
    uint64_t rmax;
};
struct SvRangeOf {
    const uint64_t* hseq;
    const int64_t* diag;
    const uint64_t* rid;
    uint64_t M;
    __host__ __device__ SvRange operator()(uint64_t e) const {
        if (hseq[e] == M) return SvRange{INT64_MAX, INT64_MIN, 0};
        return SvRange{diag[e], diag[e], rid[e]};
    }
};
struct SvRangeJoin {
    __host__ __device__ SvRange operator()(const SvRange& a, const SvRange& b) const {
        return SvRange{a.dlo < b.dlo ? a.dlo : b.dlo, a.dhi > b.dhi ? a.dhi : b.dhi, a.rmax > b.rmax ? a.rmax : b.rmax};
    }
};
struct SvDiagKey {                 // diagonal - smallest diagonal: ascending as the diagonals are, in as few bits as their range needs
    int64_t dlo;
    __host__ __device__ uint64_t operator()(int64_t d) const { return (uint64_t)d - (uint64_t)dlo; }
};
struct SvStrandOf { __host__ __device__ uint8_t operator()(uint8_t f) const { return (uint8_t)(f & 3u); } };

// head[i] = sorted entry i is a kept hit and the first of its (sequence, read, strand, diagonal) run; head[T] = 0
__global__ void __launch_bounds__(kSB) k_sv_heads(const uint64_t* __restrict__ perm, const uint64_t* __restrict__ sseq, const uint64_t* __restrict__ rid,
                                                 const uint8_t* __restrict__ flag, const int64_t* __restrict__ diag, uint64_t T, uint64_t M,
                                                 uint8_t* __restrict__ head) {
    const uint64_t stride = (uint64_t)gridDim.x * kSB;
    for (uint64_t i = (uint64_t)blockIdx.x * kSB + threadIdx.x; i <= T; i += stride) {
        bool hd = false;
        if (i < T && sseq[i] < M) {
            hd = true;
            if (i && sseq[i - 1] == sseq[i]) {
                const uint64_t a = perm[i - 1], b = perm[i];
                hd = rid[a] != rid[b] || ((flag[a] ^ flag[b]) & 3u) || diag[a] != diag[b];
            }
        }
        head[i] = hd ? 1 : 0;
    }
}

// gstart[g] = sorted index of the first hit of group g; gstart[G] = the number of kept hits (they sort in front of the others)
__global__ void __launch_bounds__(kSB) k_sv_starts(const uint8_t* __restrict__ head, const uint64_t* __restrict__ gid, const uint64_t* __restrict__ sseq, uint64_t T,
                                                  uint64_t M, uint64_t G, uint64_t* __restrict__ gstart) {
    const uint64_t stride = (uint64_t)gridDim.x * kSB;
    for (uint64_t i = (uint64_t)blockIdx.x * kSB + threadIdx.x; i <= T; i += stride) {
        if (head[i]) gstart[gid[i]] = i;
        if ((i == T || sseq[i] == M) && (i == 0 || sseq[i - 1] < M)) gstart[G] = i;
    }
}

__global__ void __launch_bounds__(kSB) k_sv_emit(const uint64_t* __restrict__ gstart, uint64_t G, uint64_t min_votes, uint8_t* __restrict__ emit) {
    const uint64_t stride = (uint64_t)gridDim.x * kSB;
    for (uint64_t g = (uint64_t)blockIdx.x * kSB + threadIdx.x; g <= G; g += stride) emit[g] = (g < G && gstart[g + 1] - gstart[g] >= min_votes) ? 1 : 0;
}

// vote_offsets[i] = records of the sequences before i: the group that the first sorted hit of a sequence >= i opens
__global__ void __launch_bounds__(kSB) k_sv_seqoff(const uint64_t* __restrict__ sseq, const uint64_t* __restrict__ gid, const uint64_t* __restrict__ orank, uint64_t T,
                                                  uint64_t M, uint64_t* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * kSB;
    for (uint64_t i = (uint64_t)blockIdx.x * kSB + threadIdx.x; i <= M; i += stride) {
        uint64_t lo = 0, hi = T;                               // the first sorted index with sseq >= i
        while (lo < hi) {
            const uint64_t mid = lo + ((hi - lo) >> 1);
            if (sseq[mid] < i) lo = mid + 1; else hi = mid;
        }
        out[i] = orank[gid[lo]];
    }
}

struct SvOut {
    uint64_t* rid;
    uint8_t* strand;
    int64_t* diag;
    uint32_t *votes, *qfirst, *qlast;
};
__global__ void __launch_bounds__(kSB) k_sv_write(const uint64_t* __restrict__ gstart, const uint8_t* __restrict__ emit, const uint64_t* __restrict__ orank, uint64_t G,
                                                 const uint64_t* __restrict__ perm, const uint64_t* __restrict__ rid, const uint8_t* __restrict__ flag,
                                                 const int64_t* __restrict__ diag, const uint32_t* __restrict__ qoff, const SvOut O) {
    const uint64_t stride = (uint64_t)gridDim.x * kSB;
    for (uint64_t g = (uint64_t)blockIdx.x * kSB + threadIdx.x; g < G; g += stride) {
        if (!emit[g]) continue;
        const uint64_t i = gstart[g], j = gstart[g + 1], o = orank[g], a = perm[i], b = perm[j - 1];
        O.rid[o] = rid[a];
        O.strand[o] = (uint8_t)(flag[a] & 3u);
        O.diag[o] = diag[a];
        O.votes[o] = j - i < 0xFFFFFFFFull ? (uint32_t)(j - i) : 0xFFFFFFFFu;
        O.qfirst[o] = qoff[a];                                 // stable sorts over hits in window order: the run is ascending in qoff
        O.qlast[o] = qoff[b];
    }
}

// d_vote_offsets (M + 1) and *total_out always; the records only when *total_out <= cap
static hipError_t sv_run(const ShBufs& B, uint64_t M, uint64_t min_votes, uint64_t* d_vote_offsets, const SvOut& O, uint64_t cap, uint64_t* total_out, hipStream_t s) {
    *total_out = 0;
    const uint64_t T = B.T;
    if (T == 0) return zero_offsets(d_vote_offsets, M, s);
    const uint64_t* hseq = (const uint64_t*)B.hseq.p;
    const int64_t* diag = (const int64_t*)B.diag.p;
    const uint64_t* rid = (const uint64_t*)B.rid.p;
    const uint8_t* flag = (const uint8_t*)B.flag.p;
    DevArr rng(s), rt(s), pa(s), pb(s), kin(s), kout(s), k8in(s), k8out(s), tmp(s), head(s), gid(s), ts(s), gstart(s), emit(s), orank(s), ts2(s);
    AIX_TRY(rng.alloc(sizeof(SvRange)));
    AIX_TRY(sh_alloc(pa, T, 8));
    AIX_TRY(sh_alloc(pb, T, 8));
    AIX_TRY(sh_alloc(kin, T + 1, 8));                          // (T + 1: the blocks of kin and k8in fit gid and head afterwards)
    AIX_TRY(sh_alloc(kout, T + 1, 8));
    AIX_TRY(sh_alloc(k8in, T + 1, 1));
    AIX_TRY(sh_alloc(k8out, T + 1, 1));
    const SvRange none{INT64_MAX, INT64_MIN, 0};
    SvRange r = none;
    {
        auto in = rocprim::make_transform_iterator(rocprim::counting_iterator<uint64_t>(0), SvRangeOf{hseq, diag, rid, M});
        AIX_TRY(with_temp(rt, [&](void* t, size_t& tb) { return rocprim::reduce(t, tb, in, (SvRange*)rng.p, none, (size_t)T, SvRangeJoin(), s); }));
        AIX_TRY(hipMemcpyAsync(&r, rng.p, sizeof(SvRange), hipMemcpyDeviceToHost, s));
        AIX_TRY(hipStreamSynchronize(s));
    }
    if (r.dlo > r.dhi) return zero_offsets(d_vote_offsets, M, s);          // no hit is kept
    uint64_t *d_pa = (uint64_t*)pa.p, *d_pb = (uint64_t*)pb.p, *d_kin = (uint64_t*)kin.p, *d_kout = (uint64_t*)kout.p;
    const dim3 gT(flat_grid(T)), blk(kSB);
    // least significant key first: diagonal, strand, read id, sequence
    AIX_TRY(sort_pairs(rocprim::make_transform_iterator(diag, SvDiagKey{r.dlo}), d_kout, rocprim::counting_iterator<uint64_t>(0), d_pa, T,
                       sort_bits((uint64_t)r.dhi - (uint64_t)r.dlo), tmp, s));
    AIX_TRY_LAUNCH((k_sv_gather<uint8_t, SvStrandOf>), gT, blk, 0, s, flag, (const uint64_t*)d_pa, T, SvStrandOf(), (uint8_t*)k8in.p);
    AIX_TRY(sort_pairs((const uint8_t*)k8in.p, (uint8_t*)k8out.p, (const uint64_t*)d_pa, d_pb, T, 2u, tmp, s));
    AIX_TRY_LAUNCH((k_sv_gather<uint64_t, SvSame>), gT, blk, 0, s, rid, (const uint64_t*)d_pb, T, SvSame(), d_kin);
    AIX_TRY(sort_pairs((const uint64_t*)d_kin, d_kout, (const uint64_t*)d_pb, d_pa, T, sort_bits(r.rmax), tmp, s));
    AIX_TRY_LAUNCH((k_sv_gather<uint64_t, SvSame>), gT, blk, 0, s, hseq, (const uint64_t*)d_pa, T, SvSame(), d_kin);
    AIX_TRY(sort_pairs((const uint64_t*)d_kin, d_kout, (const uint64_t*)d_pa, d_pb, T, sort_bits(M), tmp, s));
    const uint64_t *perm = d_pb, *sseq = d_kout;               // the hits by (sequence, read, strand, diagonal, hit number); dropped hits last
    pa.drop(); kin.drop(); k8in.drop(); k8out.drop(); tmp.drop();          // (waits for the sorts) their blocks serve the passes below
    AIX_TRY(sh_alloc(head, T + 1, 1));
    AIX_TRY(sh_alloc(gid, T + 1, 8));
    const dim3 gT1(flat_grid(T + 1));
    AIX_TRY_LAUNCH(k_sv_heads, gT1, blk, 0, s, perm, sseq, rid, flag, diag, T, M, (uint8_t*)head.p);
    AIX_TRY(scan_u64(rocprim::make_transform_iterator((const uint8_t*)head.p, Widen<uint8_t>()), (uint64_t*)gid.p, T + 1, ts, s));
    uint64_t G = 0;
    AIX_TRY(hipMemcpyAsync(&G, (const uint64_t*)gid.p + T, 8, hipMemcpyDeviceToHost, s));
    AIX_TRY(hipStreamSynchronize(s));
    AIX_TRY(sh_alloc(gstart, G + 1, 8));
    AIX_TRY(sh_alloc(emit, G + 1, 1));
    AIX_TRY(sh_alloc(orank, G + 1, 8));
    AIX_TRY_LAUNCH(k_sv_starts, gT1, blk, 0, s, (const uint8_t*)head.p, (const uint64_t*)gid.p, sseq, T, M, G, (uint64_t*)gstart.p);
    AIX_TRY_LAUNCH(k_sv_emit, dim3(flat_grid(G + 1)), blk, 0, s, (const uint64_t*)gstart.p, G, min_votes, (uint8_t*)emit.p);
    AIX_TRY(scan_u64(rocprim::make_transform_iterator((const uint8_t*)emit.p, Widen<uint8_t>()), (uint64_t*)orank.p, G + 1, ts2, s));
    uint64_t R = 0;
    AIX_TRY(hipMemcpyAsync(&R, (const uint64_t*)orank.p + G, 8, hipMemcpyDeviceToHost, s));
    AIX_TRY_LAUNCH(k_sv_seqoff, dim3(flat_grid(M + 1)), blk, 0, s, sseq, (const uint64_t*)gid.p, (const uint64_t*)orank.p, T, M, d_vote_offsets);
    AIX_TRY(hipStreamSynchronize(s));
    *total_out = R;
    if (R == 0 || R > cap || !O.rid) return hipSuccess;
    AIX_TRY_LAUNCH(k_sv_write, dim3(flat_grid(G)), blk, 0, s, (const uint64_t*)gstart.p, (const uint8_t*)emit.p, (const uint64_t*)orank.p, G, perm, rid, flag, diag,
                   (const uint32_t*)B.qoff.p, O);
    return hipStreamSynchronize(s);
}

}  // namespace aix

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" int aix_seq_hits_dev(aix_index_t* h, const char* d_seqs, const uint64_t* d_offs, uint64_t M, uint64_t max_per_kmer, uint64_t* d_seq_offsets,
                                uint32_t* d_qoff, uint64_t* d_pos, uint64_t* d_rid, int64_t* d_local, uint8_t* d_flag, uint64_t cap, uint64_t* total_out, void* stream) {
    if (!h || !d_seq_offsets || !total_out || (M && !d_offs) || M >= (1ull << 56)) return AIX_ERR_ARG;
    if (cap && (!d_qoff || !d_pos || !d_rid || !d_local || !d_flag)) return AIX_ERR_ARG;
    if (const int st = sh_check(h)) return st;
    DevGuard g(h->device);
    hipStream_t s = (hipStream_t)stream;
    *total_out = 0;
    if (M == 0) { AIXCHK(zero_offsets(d_seq_offsets, 0, s)); return AIX_OK; }
    const ShUser u{d_qoff, cap ? d_pos : nullptr, d_rid, d_local, d_flag, cap};
    ShBufs B(s);
    bool bad = false;
    AIXCHK(sh_run(h, (const uint8_t*)d_seqs, d_offs, M, max_per_kmer, d_seq_offsets, &u, false, B, &bad, s));
    if (bad) return AIX_ERR_ARG;
    *total_out = B.T;
    return AIX_OK;
}

extern "C" int aix_seq_votes_dev(aix_index_t* h, const char* d_seqs, const uint64_t* d_offs, uint64_t M, uint64_t max_per_kmer, uint64_t min_votes,
                                 uint64_t* d_vote_offsets, uint64_t* d_rid, uint8_t* d_strand, int64_t* d_diag, uint32_t* d_votes, uint32_t* d_qfirst,
                                 uint32_t* d_qlast, uint64_t cap, uint64_t* total_out, void* stream) {
    if (!h || !d_vote_offsets || !total_out || (M && !d_offs) || M >= (1ull << 56)) return AIX_ERR_ARG;
    if (cap && (!d_rid || !d_strand || !d_diag || !d_votes || !d_qfirst || !d_qlast)) return AIX_ERR_ARG;
    if (const int st = sh_check(h)) return st;
    DevGuard g(h->device);
    hipStream_t s = (hipStream_t)stream;
    *total_out = 0;
    if (M == 0) { AIXCHK(zero_offsets(d_vote_offsets, 0, s)); return AIX_OK; }
    ShBufs B(s);
    bool bad = false;
    AIXCHK(sh_run(h, (const uint8_t*)d_seqs, d_offs, M, max_per_kmer, nullptr, nullptr, true, B, &bad, s));
    if (bad) return AIX_ERR_ARG;
    B.pos.drop(); B.local.drop();                              // the diagonal holds what the grouping needs of them: the sorts take these blocks
    const SvOut O{cap ? d_rid : nullptr, d_strand, d_diag, d_votes, d_qfirst, d_qlast};
    AIXCHK(sv_run(B, M, min_votes, d_vote_offsets, O, cap, total_out, s));
    return AIX_OK;
}

extern "C" int aix_seq_hits(aix_index_t* h, const char* seqs, const uint64_t* offs, uint64_t M, uint64_t max_per_kmer, uint64_t** seq_offsets_out,
                            uint32_t** qoff_out, uint64_t** pos_out, uint64_t** rid_out, int64_t** local_out, uint8_t** flag_out) {
    if (!h || !seq_offsets_out || !qoff_out || !pos_out || !rid_out || !local_out || !flag_out || !offs || M >= (1ull << 56)) return AIX_ERR_ARG;
    *seq_offsets_out = *pos_out = *rid_out = nullptr; *qoff_out = nullptr; *local_out = nullptr; *flag_out = nullptr;
    if (M && offs[M] && !seqs) return AIX_ERR_ARG;
    if (const int st = sh_check(h)) return st;
    DevGuard g(h->device);
    DevArr ds, dof, dso;
    if (const int st = sh_upload(seqs, offs, M, ds, dof)) return st;
    AIXCHK(dso.alloc(8 * (M + 1)));
    AIXCHK(hipMemset(dso.p, 0, 8 * (M + 1)));
    ShBufs B(nullptr);
    bool bad = false;
    if (M) AIXCHK(sh_run(h, (const uint8_t*)ds.p, (const uint64_t*)dof.p, M, max_per_kmer, (uint64_t*)dso.p, nullptr, false, B, &bad, nullptr));
    if (bad) return AIX_ERR_ARG;
    const uint64_t T = B.T;
    const HostOut outs[] = {{(void**)seq_offsets_out, dso.p, 8 * (M + 1)}, {(void**)qoff_out, B.qoff.p, 4 * T}, {(void**)pos_out, B.pos.p, 8 * T},
                            {(void**)rid_out, B.rid.p, 8 * T},             {(void**)local_out, B.local.p, 8 * T}, {(void**)flag_out, B.flag.p, T}};
    AIXCHK(copy_out_host(outs, 6));
    return AIX_OK;
}

extern "C" int aix_seq_votes(aix_index_t* h, const char* seqs, const uint64_t* offs, uint64_t M, uint64_t max_per_kmer, uint64_t min_votes,
                             uint64_t** vote_offsets_out, uint64_t** rid_out, uint8_t** strand_out, int64_t** diag_out, uint32_t** votes_out,
                             uint32_t** qfirst_out, uint32_t** qlast_out) {
    if (!h || !vote_offsets_out || !rid_out || !strand_out || !diag_out || !votes_out || !qfirst_out || !qlast_out || !offs || M >= (1ull << 56)) return AIX_ERR_ARG;
    *vote_offsets_out = *rid_out = nullptr; *strand_out = nullptr; *diag_out = nullptr; *votes_out = *qfirst_out = *qlast_out = nullptr;
    if (M && offs[M] && !seqs) return AIX_ERR_ARG;
    if (const int st = sh_check(h)) return st;
    DevGuard g(h->device);
    DevArr ds, dof, dvo, dr, dst, dd, dv, dqf, dql;
    if (const int st = sh_upload(seqs, offs, M, ds, dof)) return st;
    AIXCHK(dvo.alloc(8 * (M + 1)));
    AIXCHK(hipMemset(dvo.p, 0, 8 * (M + 1)));
    uint64_t R = 0;
    if (M) {
        ShBufs B(nullptr);
        bool bad = false;
        AIXCHK(sh_run(h, (const uint8_t*)ds.p, (const uint64_t*)dof.p, M, max_per_kmer, nullptr, nullptr, true, B, &bad, nullptr));
        if (bad) return AIX_ERR_ARG;
        B.pos.drop(); B.local.drop();
        // a record needs at least one hit: B.T bounds the records, so one grouping pass fills buffers of that size
        uint64_t cap = B.T;
        if (min_votes > 1) cap = B.T / min_votes;
        AIXCHK(dr.alloc(8 * cap)); AIXCHK(dst.alloc(cap)); AIXCHK(dd.alloc(8 * cap)); AIXCHK(dv.alloc(4 * cap)); AIXCHK(dqf.alloc(4 * cap)); AIXCHK(dql.alloc(4 * cap));
        const SvOut O{(uint64_t*)dr.p, (uint8_t*)dst.p, (int64_t*)dd.p, (uint32_t*)dv.p, (uint32_t*)dqf.p, (uint32_t*)dql.p};
        AIXCHK(sv_run(B, M, min_votes, (uint64_t*)dvo.p, O, cap, &R, nullptr));
    }
    const HostOut outs[] = {{(void**)vote_offsets_out, dvo.p, 8 * (M + 1)}, {(void**)rid_out, dr.p, 8 * R},    {(void**)strand_out, dst.p, R},
                            {(void**)diag_out, dd.p, 8 * R},                {(void**)votes_out, dv.p, 4 * R},  {(void**)qfirst_out, dqf.p, 4 * R},
                            {(void**)qlast_out, dql.p, 4 * R}};
    AIXCHK(copy_out_host(outs, 7));
    return AIX_OK;
}
