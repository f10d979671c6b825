// aix_merge.hip — K1 beyond one piece: sorted (key, count) runs are merged, never re-sorted.
//
// The reference merges its per-thread maps once (count_kmers.cpp:334-341). Here a buffer of more than 2^31 windows is counted piece by
// piece (aix_k1.hip: every piece comes out as keys ascending + counts), and across GPUs every rank receives one sorted run per peer
// (aindex_amd/dist.py). Both used to concatenate and run a full-width radix sort + reduce-by-key per merge; what is needed is a TWO-WAY
// MERGE WITH SUMMATION of two runs that are each sorted and distinct:
//   k_merge_split : merge-path split points, one per tile of 2 048 merged entries (binary search on the diagonal, ties = A first);
//                   a split that would separate A[i] == B[j] moves B[j] into the earlier tile, so equal keys always meet in one tile
//   k_merge_tile  : both slices into LDS, every lane merge-path-searches its own 8 entries, merges them in registers, writes the merged
//                   tile back to LDS; an entry equal to its left neighbour is the B half of a pair and folds its count into the A half;
//                   pass 1 counts the survivors per tile, a scan gives the tile bases, pass 2 writes keys and summed counts
// One read of the keys per pass, one of the counts, one write of the result: ~40 B per entry against twelve radix passes of 16 B.
// Sizes are 64-bit throughout (the 2^32 bound of the old path is gone).
#include <algorithm>
#include <cstring>
#include <vector>

#include <new>
#include <string>

#include "aix_env.hpp"
#include "aix_hostkit.hpp"

namespace aix {

static constexpr int kB = 256;
static inline unsigned grid_of(uint64_t work) {
    uint64_t b = (work + kB - 1) / kB;
    if (b > 65536) b = 65536;
    if (b == 0) b = 1;
    return (unsigned)b;
}

static constexpr int MG_TB = 256, MG_IPT = 8, MG_T = MG_TB * MG_IPT;

__global__ void __launch_bounds__(kB) k_merge_split(const uint64_t* __restrict__ A, uint64_t na, const uint64_t* __restrict__ B, uint64_t nb, uint64_t ntiles,
                                                    uint64_t* __restrict__ split /* [ntiles + 1][2] */) {
    const uint64_t t = (uint64_t)blockIdx.x * kB + threadIdx.x;
    if (t > ntiles) return;
    const uint64_t d = std::min<uint64_t>(t * (uint64_t)MG_T, na + nb);
    uint64_t lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
    while (lo < hi) {                                            // entries of A among the first d merged ones, equal keys: A first
        const uint64_t mid = (lo + hi) >> 1;
        if (A[mid] <= B[d - 1 - mid]) lo = mid + 1; else hi = mid;
    }
    uint64_t ai = lo, bi = d - lo;
    if (ai > 0 && bi < nb && A[ai - 1] == B[bi]) ++bi;           // keep the pair in one tile (tiles hold MG_T + 1 entries at most)
    split[2 * t] = ai;
    split[2 * t + 1] = bi;
}

template <bool WRITE>
__global__ void __launch_bounds__(MG_TB) k_merge_tile(const uint64_t* __restrict__ Ak, const uint64_t* __restrict__ Ac, const uint64_t* __restrict__ Bk,
                                                      const uint64_t* __restrict__ Bc, const uint64_t* __restrict__ split, uint64_t ntiles,
                                                      uint64_t* __restrict__ tile_count /* pass 1: out */, const uint64_t* __restrict__ tile_base /* pass 2: in */,
                                                      uint64_t* __restrict__ out_k, uint64_t* __restrict__ out_c) {
    __shared__ uint64_t sk[MG_T + 2];
    __shared__ uint64_t sc[WRITE ? MG_T + 2 : 1];
    __shared__ uint32_t wsum[MG_TB / 64];
    const int tid = threadIdx.x;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t a0 = split[2 * t], b0 = split[2 * t + 1], a1 = split[2 * t + 2], b1 = split[2 * t + 3];
        const uint32_t na_t = (uint32_t)(a1 - a0), nb_t = (uint32_t)(b1 - b0), m = na_t + nb_t;
        for (uint32_t i = tid; i < m; i += MG_TB) {
            sk[i] = i < na_t ? Ak[a0 + i] : Bk[b0 + (i - na_t)];
            if (WRITE) sc[i] = i < na_t ? Ac[a0 + i] : Bc[b0 + (i - na_t)];
        }
        __syncthreads();
        // lane i merges entries [8 i, 8 i + 8); the last lane also takes the 2 049th entry of a tile that was handed a pair's second half
        const uint32_t d0 = std::min<uint32_t>((uint32_t)tid * MG_IPT, m), d1 = tid == MG_TB - 1 ? m : std::min<uint32_t>(d0 + MG_IPT, m);
        uint32_t lo = d0 > nb_t ? d0 - nb_t : 0u, hi = d0 < na_t ? d0 : na_t;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (sk[mid] <= sk[na_t + d0 - 1 - mid]) lo = mid + 1; else hi = mid;
        }
        uint32_t ai = lo, bi = d0 - lo;
        uint64_t rk[MG_IPT + 1], rc[MG_IPT + 1];
#pragma unroll
        for (int j = 0; j <= MG_IPT; ++j) {
            rk[j] = 0; rc[j] = 0;
            if (d0 + j < d1) {
                const bool take_a = ai < na_t && (bi >= nb_t || sk[ai] <= sk[na_t + bi]);
                const uint32_t idx = take_a ? ai : na_t + bi;
                rk[j] = sk[idx];
                if (WRITE) rc[j] = sc[idx];
                if (take_a) ++ai; else ++bi;
            }
        }
        __syncthreads();                                         // the two slices have been read by everybody: the merged tile replaces them
#pragma unroll
        for (int j = 0; j <= MG_IPT; ++j)
            if (d0 + j < d1) { sk[d0 + j] = rk[j]; if (WRITE) sc[d0 + j] = rc[j]; }
        __syncthreads();
        uint32_t kept = 0;
#pragma unroll
        for (int j = 0; j <= MG_IPT; ++j) {
            const uint32_t i = d0 + j;
            if (i < d1 && (i == 0 || sk[i] != sk[i - 1])) ++kept;
        }
        uint32_t incl = kept;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(incl, d);
            if ((tid & 63) >= d) incl += y;
        }
        if ((tid & 63) == 63) wsum[tid >> 6] = incl;
        __syncthreads();
        uint32_t off = 0, all = 0;
#pragma unroll
        for (int w = 0; w < MG_TB / 64; ++w) { const uint32_t x = wsum[w]; if (w < (tid >> 6)) off += x; all += x; }
        if (!WRITE) {
            if (tid == 0) tile_count[t] = all;
        } else {
            uint64_t o = tile_base[t] + off + incl - kept;
#pragma unroll
            for (int j = 0; j <= MG_IPT; ++j) {
                const uint32_t i = d0 + j;
                if (i < d1 && (i == 0 || sk[i] != sk[i - 1])) {
                    out_k[o] = sk[i];
                    out_c[o] = sc[i] + ((i + 1 < m && sk[i + 1] == sk[i]) ? sc[i + 1] : 0ull);
                    ++o;
                }
            }
        }
        __syncthreads();                                         // sk / wsum are reused by the next tile
    }
}

hipError_t merge_sum_runs(RunView a, RunView b, DistinctRun& out, hipStream_t s) {
    out.reset();
    const uint64_t tot = a.n + b.n;
    if (tot == 0) return hipSuccess;
    const uint64_t ntiles = (tot + MG_T - 1) / MG_T;
    DevArr split(s), counts(s), bases(s), tmp(s), ok(s), oc(s);
    AIX_TRY(split.alloc(16 * (ntiles + 1)));
    AIX_TRY(counts.alloc(8 * (ntiles + 1)));
    AIX_TRY(bases.alloc(8 * (ntiles + 1)));
    const unsigned grid = (unsigned)std::min<uint64_t>(ntiles, 1u << 20);
    AIX_TRY_LAUNCH(k_merge_split, dim3((unsigned)((ntiles + 1 + kB - 1) / kB)), dim3(kB), 0, s, a.k, a.n, b.k, b.n, ntiles, (uint64_t*)split.p);
    AIX_TRY(hipMemsetAsync((uint64_t*)counts.p + ntiles, 0, 8, s));   // the scan runs over ntiles + 1 words: its last output is the total
    AIX_TRY_LAUNCH((k_merge_tile<false>), dim3(grid), dim3(MG_TB), 0, s, a.k, a.c, b.k, b.c, (const uint64_t*)split.p, ntiles, (uint64_t*)counts.p,
                   (const uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t*)nullptr);
    AIX_TRY(scan_u64((uint64_t*)counts.p, (uint64_t*)bases.p, ntiles + 1, tmp, s));
    uint64_t total = 0;
    AIX_TRY(hipMemcpyAsync(&total, (uint64_t*)bases.p + ntiles, 8, hipMemcpyDeviceToHost, s));
    AIX_TRY(hipStreamSynchronize(s));
    AIX_TRY(ok.alloc(8 * total));
    AIX_TRY(oc.alloc(8 * total));
    AIX_TRY_LAUNCH((k_merge_tile<true>), dim3(grid), dim3(MG_TB), 0, s, a.k, a.c, b.k, b.c, (const uint64_t*)split.p, ntiles, (uint64_t*)nullptr, (const uint64_t*)bases.p,
                   (uint64_t*)ok.p, (uint64_t*)oc.p);
    AIX_TRY(hipStreamSynchronize(s));
    out.adopt(ok, oc, total);
    return hipSuccess;
}

__global__ void __launch_bounds__(kB) k_widen_counts(const uint32_t* __restrict__ c32, uint64_t n, uint64_t* __restrict__ c64) {
    const uint64_t stride = (uint64_t)gridDim.x * kB;
    for (uint64_t i = (uint64_t)blockIdx.x * kB + threadIdx.x; i < n; i += stride) c64[i] = c32[i];
}
__global__ void __launch_bounds__(kB) k_flag_min64(const uint64_t* __restrict__ counts, uint64_t n, uint64_t min_count, uint8_t* __restrict__ flags) {
    const uint64_t stride = (uint64_t)gridDim.x * kB;
    for (uint64_t i = (uint64_t)blockIdx.x * kB + threadIdx.x; i < n; i += stride) flags[i] = counts[i] >= min_count ? 1 : 0;
}

// keeps the entries of r with count >= min_count (order kept); synchronises `s`. On a failure r is as it was.
static hipError_t filter_min_count(DistinctRun& r, uint64_t min_count, hipStream_t s) {
    if (min_count <= 1 || r.n == 0) return hipSuccess;
    DevArr flags(s), fk(s), fc(s), d_sel(s), tmp_k(s), tmp_c(s);
    AIX_TRY(flags.alloc(r.n));
    AIX_TRY(fk.alloc(8 * r.n));
    AIX_TRY(fc.alloc(8 * r.n));
    AIX_TRY(d_sel.alloc(8));
    AIX_TRY_LAUNCH(k_flag_min64, dim3(grid_of(r.n)), dim3(kB), 0, s, (const uint64_t*)r.c, r.n, min_count, (uint8_t*)flags.p);
    AIX_TRY(with_temp(tmp_k, [&](void* t, size_t& tb) { return rocprim::select(t, tb, r.k, (uint8_t*)flags.p, (uint64_t*)fk.p, (uint64_t*)d_sel.p, (size_t)r.n, s); }));
    AIX_TRY(with_temp(tmp_c, [&](void* t, size_t& tb) { return rocprim::select(t, tb, r.c, (uint8_t*)flags.p, (uint64_t*)fc.p, (uint64_t*)d_sel.p, (size_t)r.n, s); }));
    uint64_t kept = 0;
    AIX_TRY(hipMemcpyAsync(&kept, d_sel.p, 8, hipMemcpyDeviceToHost, s));
    AIX_TRY(hipStreamSynchronize(s));
    r.adopt(fk, fc, kept);
    return hipSuccess;
}

// ---------------------------------------------------------------------------------------------
// DistinctAcc: the distinct set of everything added so far (K1 for buffers / files of any length). A piece = every k-window of one
// PLAIN buffer of at most 2^31 windows; its distinct set (aix_k1.hip: the MSD path, or the radix-sort path) is merged into the accumulated one.
// ---------------------------------------------------------------------------------------------
DistinctAcc::DistinctAcc(int kk, int canon, hipStream_t st) : k(kk), canon_mode(canon), s(st), scratch(st) {}
DistinctAcc::~DistinctAcc() {
    if (acc.k || acc.c) (void)hipStreamSynchronize(s);          // the last merge or the caller's copies may still read the set
}

hipError_t DistinctAcc::add_plain(const uint8_t* d_plain, uint64_t plen) {
    if (plen < (uint64_t)k) return hipSuccess;
    const uint64_t nwin = plen - k + 1;
    if (nwin > (1ull << 31)) return hipErrorInvalidValue;
    ++pieces;
    // the 8 B-per-window staging and the partition workspace stay with the accumulator from piece to piece (K1Scratch)
    AIX_TRY(K1Scratch::need(scratch.codes, scratch.codes_bytes, 8 * nwin));
    uint64_t* codes = (uint64_t*)scratch.codes.p;
    DevArr pk(s), pc(s), pc32(s);
    uint64_t pm = 0;
    bool sorted_path = !k1_msd_eligible(nwin, k);
    // MSD partition + per-bucket LDS hash / sort, windows encoded inside level 1, counts as u64. A bucket too rich for LDS: nothing was
    // produced and the piece takes the sort path
    if (!sorted_path) AIX_TRY(distinct_from_codes_msd(d_plain, plen, nwin, k, canon_mode, codes, scratch, pk, pc, &pm, &sorted_path, s));
    if (sorted_path) {                                                    // counts in 32 bits, widened here
        AIX_TRY(launch_window_codes(d_plain, plen, k, canon_mode, codes, s));
        AIX_TRY(distinct_from_codes(codes, nwin, k, pk, pc32, &pm, s));
        if (pm) {
            AIX_TRY(pc.alloc(8 * pm));
            AIX_TRY_LAUNCH(k_widen_counts, dim3(grid_of(pm)), dim3(kB), 0, s, (const uint32_t*)pc32.p, pm, (uint64_t*)pc.p);
        }
    }
    if (pm == 0) return hipSuccess;
    if (acc.n == 0) {                                                     // the first non-empty piece: sorted, distinct, u64 counts — taken as it is
        (void)hipStreamSynchronize(s);
        acc.adopt(pk, pc, pm);
        return hipSuccess;
    }
    DistinctRun merged;
    AIX_TRY(merge_sum_runs(acc.view(), RunView{(const uint64_t*)pk.p, (const uint64_t*)pc.p, pm}, merged, s));
    ++merges;
    acc = std::move(merged);
    return hipSuccess;
}

hipError_t DistinctAcc::finish(uint64_t min_count, DistinctRun& out) {
    out.reset();
    if (acc.n == 0) return hipSuccess;
    AIX_TRY(filter_min_count(acc, min_count, s));
    out = std::move(acc);
    return hipSuccess;
}

hipError_t distinct_from_plain(const uint8_t* d_plain, uint64_t plen, int k, int canon_mode, uint64_t min_count, uint64_t piece, DistinctRun& out, hipStream_t s) {
    out.reset();
    if (plen < (uint64_t)k) return hipSuccess;
    const uint64_t nwin_all = plen - k + 1;
    // 32-bit window indices inside a piece allow 2^31 windows; the default is 2^30: the two big temporaries of a piece are then 8 and 8.5 GiB
    // and stay in the block cache between calls (16 + 17 GiB did not: every call paid ~0.75 s of hipMalloc / hipFree), at the price of one more
    // 2.4 ms merge per 2^30 windows
    if (piece == 0 || piece > (1ull << 31)) piece = 1ull << 30;
    DistinctAcc acc(k, canon_mode, s);
    for (uint64_t w0 = 0; w0 < nwin_all; w0 += piece) {                      // a window belongs to the piece that holds its first byte
        const uint64_t nwin = std::min(piece, nwin_all - w0);
        AIX_TRY(acc.add_plain(d_plain + w0, nwin + k - 1));
    }
    return acc.finish(min_count, out);
}

// (key, count) pairs in `nruns` runs, run r = entries [offs[r], offs[r + 1]), each run sorted by key and free of repeats (what a rank
// holds after the K1 exchange: one run per peer) -> keys ascending, counts of equal keys summed, counts >= min_count. A tree of
// two-way merges: every entry is read and written log2(nruns) times, nothing is sorted. Inputs are not modified.
hipError_t merge_runs(const uint64_t* d_keys, const uint64_t* d_counts, const uint64_t* offs, uint32_t nruns, uint64_t min_count, DistinctRun& out, hipStream_t s) {
    out.reset();
    struct Run { RunView v; DistinctRun own; };                             // own: empty for a run of the caller's, else what v looks at
    std::vector<Run> cur;
    for (uint32_t r = 0; r < nruns; ++r)
        if (offs[r + 1] > offs[r]) cur.push_back(Run{RunView{d_keys + offs[r], d_counts + offs[r], offs[r + 1] - offs[r]}, DistinctRun{}});
    while (cur.size() > 1) {
        std::vector<Run> nxt;
        for (size_t i = 0; i + 1 < cur.size(); i += 2) {
            Run m;
            AIX_TRY(merge_sum_runs(cur[i].v, cur[i + 1].v, m.own, s));
            m.v = m.own.view();
            nxt.push_back(std::move(m));
        }
        if (cur.size() & 1) nxt.push_back(std::move(cur.back()));
        cur.swap(nxt);                                                      // the merged inputs die here: merge_sum_runs has synchronised
    }
    if (cur.empty()) return hipSuccess;
    DistinctRun res = std::move(cur[0].own);
    if (!res.k) {                                                           // a single run: the result is a copy (inputs stay the caller's)
        const RunView v = cur[0].v;
        DevArr ck(s), cc(s);
        AIX_TRY(ck.alloc(8 * v.n));
        AIX_TRY(cc.alloc(8 * v.n));
        AIX_TRY(hipMemcpyAsync(ck.p, v.k, 8 * v.n, hipMemcpyDeviceToDevice, s));
        AIX_TRY(hipMemcpyAsync(cc.p, v.c, 8 * v.n, hipMemcpyDeviceToDevice, s));
        AIX_TRY(hipStreamSynchronize(s));
        res.adopt(ck, cc, v.n);
    }
    AIX_TRY(filter_min_count(res, min_count, s));
    out = std::move(res);
    return hipSuccess;
}

// the same for pairs in ANY order (repeated keys anywhere): sort by key + reduce-by-key. Kept for callers that cannot name their runs.
hipError_t merge_counts(const uint64_t* d_keys, const uint64_t* d_counts, uint64_t n, uint64_t min_count, DistinctRun& out, hipStream_t s) {
    out.reset();
    if (n == 0) return hipSuccess;
    DevArr srt_k(s), srt_c(s), out_k(s), out_c(s), d_n(s), tmp(s);
    AIX_TRY(srt_k.alloc(8 * n));
    AIX_TRY(srt_c.alloc(8 * n));
    AIX_TRY(sort_pairs(d_keys, (uint64_t*)srt_k.p, d_counts, (uint64_t*)srt_c.p, n, 64u, tmp, s));
    AIX_TRY(out_k.alloc(8 * n));
    AIX_TRY(out_c.alloc(8 * n));
    AIX_TRY(d_n.alloc(8));
    AIX_TRY(with_temp(tmp, [&](void* t, size_t& tb) {                       // tmp is live: its alloc waits for the sort, as before
        return rocprim::reduce_by_key(t, tb, (uint64_t*)srt_k.p, (uint64_t*)srt_c.p, (size_t)n, (uint64_t*)out_k.p, (uint64_t*)out_c.p, (uint64_t*)d_n.p,
                                      rocprim::plus<uint64_t>(), rocprim::equal_to<uint64_t>(), s);
    }));
    uint64_t merged = 0;
    AIX_TRY(hipMemcpyAsync(&merged, d_n.p, 8, hipMemcpyDeviceToHost, s));
    AIX_TRY(hipStreamSynchronize(s));
    DistinctRun res;
    res.adopt(out_k, out_c, merged);
    AIX_TRY(filter_min_count(res, min_count, s));
    out = std::move(res);
    return hipSuccess;
}

}  // namespace aix

// ---------------------------------------------------------------------------------------------
// K1: distinct canonical k-mers of a sequence file (kmer_counter replacement)
// ---------------------------------------------------------------------------------------------
// device-resident twin: the PLAIN buffer is already in HBM; the result stays in HBM inside an opaque object until the caller
// has copied it into arrays of its own (two steps because the number of distinct k-mers is only known afterwards)
struct aix_distinct { DistinctRun r; int device = 0; };

// what the three producers share: device check, guard, the object, and `what` in front of a HIP error. run(result) fills the result.
template <typename F>
static int make_distinct(int device, const char* what, aix_distinct_t** out, F&& run) {
    const int st = check_device(device);
    if (st) return st;
    DevGuard g(device);
    aix_distinct* r = new (std::nothrow) aix_distinct();
    if (!r) return AIX_ERR_NOMEM;
    r->device = device;
    const hipError_t e = run(r->r);
    if (e != hipSuccess) { delete r; set_last_error(std::string(what) + ": " + hipGetErrorString(e)); return AIX_ERR_HIP; }
    *out = r;
    return AIX_OK;
}

extern "C" int aix_count_distinct_dev(const char* d_plain, uint64_t len, int k, int canon_mode, uint64_t min_count, int device, void* stream,
                                      aix_distinct_t** out) {
    if (!out || (len && !d_plain) || k < 1 || k > 31 || canon_mode < 0 || canon_mode > 2) return AIX_ERR_ARG;
    *out = nullptr;
    return make_distinct(device, "count_distinct", out, [&](DistinctRun& r) {
        return distinct_from_plain((const uint8_t*)d_plain, len, k, canon_mode, min_count ? min_count : 1, env_distinct_piece(), r, (hipStream_t)stream);
    });
}
// K1 across GPUs: after the exchange a rank holds (key, count) pairs from every rank; equal keys are summed here
extern "C" int aix_merge_counts_dev(const uint64_t* d_keys, const uint64_t* d_counts, uint64_t n, uint64_t min_count, int device, void* stream,
                                    aix_distinct_t** out) {
    if (!out || (n && (!d_keys || !d_counts))) return AIX_ERR_ARG;
    *out = nullptr;
    return make_distinct(device, "merge_counts", out, [&](DistinctRun& r) {
        return merge_counts(d_keys, d_counts, n, min_count ? min_count : 1, r, (hipStream_t)stream);
    });
}
// the same when the caller knows its runs: run r = entries [run_offsets[r], run_offsets[r + 1]), each sorted by key and free of repeats
// (after the K1 exchange a rank holds one such run per peer): a tree of two-way merges, nothing is sorted
extern "C" int aix_merge_runs_dev(const uint64_t* d_keys, const uint64_t* d_counts, const uint64_t* run_offsets, uint32_t nruns, uint64_t min_count, int device,
                                  void* stream, aix_distinct_t** out) {
    if (!out || !run_offsets || nruns == 0) return AIX_ERR_ARG;
    *out = nullptr;
    for (uint32_t r = 0; r < nruns; ++r) if (run_offsets[r + 1] < run_offsets[r]) return AIX_ERR_ARG;
    if (run_offsets[nruns] > run_offsets[0] && (!d_keys || !d_counts)) return AIX_ERR_ARG;
    return make_distinct(device, "merge_runs", out, [&](DistinctRun& r) {
        return merge_runs(d_keys, d_counts, run_offsets, nruns, min_count ? min_count : 1, r, (hipStream_t)stream);
    });
}
extern "C" int aix_distinct_size(const aix_distinct_t* r, uint64_t* n_out) {
    if (!r || !n_out) return AIX_ERR_ARG;
    *n_out = r->r.n;
    return AIX_OK;
}
extern "C" int aix_distinct_copy_dev(const aix_distinct_t* r, uint64_t* d_keys, uint64_t* d_counts, void* stream) {
    if (!r || (r->r.n && (!d_keys || !d_counts))) return AIX_ERR_ARG;
    DevGuard g(r->device);
    if (r->r.n) {
        HIPCHK(hipMemcpyAsync(d_keys, r->r.k, 8 * r->r.n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
        HIPCHK(hipMemcpyAsync(d_counts, r->r.c, 8 * r->r.n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
        HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    }
    return AIX_OK;
}
extern "C" void aix_distinct_free(aix_distinct_t* r) {
    if (!r) return;
    DevGuard g(r->device);
    delete r;                                                   // a plain free of the two blocks: the copies above have synchronised
}
