// aix_posquery.hip — batch position queries over a positions index ("aindex") resident in HBM.
//   AindexWrapper::get_positions / get_positions_13mer   python_wrapper.cpp:800-831,1070-1100   k-mer -> occurrences
//   PHASH_MAP::get_pfid                                   hash.hpp:150-170                       which strand names the bucket
//   AindexWrapper::get_rid / get_start                    python_wrapper.cpp:757-789 over IntervalTree::query :66-74
//
// The reference answers one k-mer per call. Here N k-mers are one ragged gather: N lists of 0 .. tf_max entries, read in random order from
// the positions array, written back to back (CSR: offsets[N + 1], positions[offsets[N]]). List lengths are heavily skewed (a repeat has
// 10^5 occurrences beside a median of a handful), so no pass gives a list to a wave. The chain:
//   1 k_pq_resolve*   one lane per k-mer: bucket h (wave-cooperative verification-table probe, MPHF for the rest), source start indices[h]
//                     and upper bound ub = min(indices[h + 1], total) - indices[h]
//   2 scans of ub and of (ub != 0); k_pq_compact keeps the non-empty lists only: nfo[j] = start of list j in the FLAT space of T = sum ub
//     candidate entries (strictly ascending), nlo[j] = its source start, ne[j] = the k-mer it belongs to
//   3 k_pq_flat<false>   every wave owns a contiguous tile of 64-entry chunks of the flat space: one wave-wide search of nfo for the tile's
//                        first list, then a chunk's lists lie within 64 entries of nfo (held one per lane, searched with ds_bpermute).
//                        Consecutive lanes read consecutive slots wherever a list is long. Writes the chunk's non-zero mask (ballot) and count.
//   4 scan of the chunk counts = rank of every chunk; k_pq_segrank: kept[i] = min(max_per_kmer, non-zeros of list i) from two rank lookups
//     per list; scan of kept = offsets[]
//   5 k_pq_flat<true>    the same walk; a non-zero entry goes to offsets[i] + (its rank - rank of its list's start) when that is below
//                        max_per_kmer, minus one (0-based); rid / offset in read by per-lane bisection of the interval ends in the same pass
// Step 1 ends in pq_resolve23_words and steps 2 to 5 are posquery_lists (both aix_posquery.hpp): aix_seqhits.hip resolves the windows of
// sequences with the first and runs the second on them.
// Zeros are skipped wherever they sit (the fill leaves them wherever a window was not placed). Every size, offset and flat index is 64 bits wide.
// No atomics; all stores are plain vector stores.
#include <algorithm>
#include <new>
#include <vector>

#include "aix_posquery.hpp"

namespace aix {

static constexpr int kB = kFlatBlock;                             // the grid of the flat kernels: flat_grid (aix_hostkit.hpp)

// ---------------------------------------------------------------------------------------------
// attach: indices[0] == 0, indices[i] <= indices[i + 1], indices[n] <= total
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kB) k_pq_validate(const uint64_t* __restrict__ ind, uint64_t n, uint64_t total, uint32_t* __restrict__ flag) {
    const uint64_t stride = (uint64_t)gridDim.x * kB;
    bool bad = false;
    for (uint64_t i = (uint64_t)blockIdx.x * kB + threadIdx.x; i <= n; i += stride) {
        const uint64_t v = ind[i];
        bad |= (i == 0 && v != 0) || (i < n ? v > ind[i + 1] : v > total);
    }
    if (bad) *flag = 1u;
}

// ---------------------------------------------------------------------------------------------
// 1. k-mer -> bucket -> (source start, upper bound)
// ---------------------------------------------------------------------------------------------
// (pq_emit, the get_pfid strand rule and the probe behind it: pq_resolve23_words, aix_posquery.hpp)
template <int LPP>
__global__ void __launch_bounds__(kB) k_pq_resolve23(const IndexDev ix, const uint8_t* __restrict__ q, uint64_t N, const uint64_t* __restrict__ indices,
                                                    uint64_t total, uint64_t* __restrict__ lo_out, uint64_t* __restrict__ ub_out) {
    const uint64_t stride = (uint64_t)gridDim.x * kB;
    for (uint64_t base = (uint64_t)blockIdx.x * kB + (threadIdx.x & ~63u); base < N; base += stride) {
        const uint64_t i = base + (threadIdx.x & 63u);
        const bool in = i < N;
        uint64_t w0 = 0, w1 = 0, w2 = 0;
        if (in) load23(q + 23 * i, w0, w1, w2);
        uint64_t lo, ub;
        pq_resolve23_words<LPP>(ix, in, w0, w1, w2, indices, total, lo, ub);
        if (in) {
            lo_out[i] = lo;
            ub_out[i] = ub;
        }
    }
}

// get_positions_13mer (:1070-1100): exactly 13 upper-case A/C/G/T, forward strand, bucket = hasher_13mer.lookup(kmer) = perm13[code]
__global__ void __launch_bounds__(kB) k_pq_resolve13(const uint32_t* __restrict__ perm13, const uint8_t* __restrict__ q, uint64_t N,
                                                    const uint64_t* __restrict__ indices, uint64_t total, uint64_t* __restrict__ lo_out,
                                                    uint64_t* __restrict__ ub_out) {
    const uint64_t stride = (uint64_t)gridDim.x * kB;
    for (uint64_t i = (uint64_t)blockIdx.x * kB + threadIdx.x; i < N; i += stride) {
        uint64_t w0, w1;
        load13(q + 13 * i, w0, w1);
        const Enc13 e = encode13_words(w0, w1);
        uint64_t lo, ub;
        pq_emit(indices, total, AIX_TOTAL_13MERS, e.valid ? (uint64_t)perm13[e.code] : AIX_TOTAL_13MERS, lo, ub);
        lo_out[i] = lo;
        ub_out[i] = ub;
    }
}

// ---------------------------------------------------------------------------------------------
// 2. the non-empty lists, closed up. nfo carries 65 entries of padding equal to T behind its J entries.
// ---------------------------------------------------------------------------------------------
static constexpr uint64_t kPad = 65;
__global__ void __launch_bounds__(kB) k_pq_compact(uint64_t N, const uint64_t* __restrict__ ub, const uint64_t* __restrict__ fo, const uint64_t* __restrict__ nj,
                                                  const uint64_t* __restrict__ lo, uint64_t J, uint64_t T, uint64_t* __restrict__ ne,
                                                  uint64_t* __restrict__ nfo, uint64_t* __restrict__ nlo) {
    const uint64_t stride = (uint64_t)gridDim.x * kB;
    const uint64_t M = N > kPad ? N : kPad;
    for (uint64_t i = (uint64_t)blockIdx.x * kB + threadIdx.x; i < M; i += stride) {
        if (i < N && ub[i]) {
            const uint64_t j = nj[i];
            ne[j] = i;
            nfo[j] = fo[i];
            nlo[j] = lo[i];
        }
        if (i < kPad) nfo[J + i] = T;
    }
}

// ---------------------------------------------------------------------------------------------
// 3 / 5. the flat passes
// ---------------------------------------------------------------------------------------------
// (the tile's first list is found with wave_count_le, aix_device.hpp; pq_locate: aix_posquery.hpp)
struct PqFlat {
    const uint64_t* positions;     // the attached array
    const uint64_t* ne;            // [J] k-mer of list j
    const uint64_t* nfo;           // [J + 65] flat start of list j, then T
    const uint64_t* nlo;           // [J] source start of list j
    uint64_t J, T, C;              // lists, flat entries, 64-entry chunks
    uint64_t* bits;                // [C + 1] non-zero mask per chunk (pass 3 writes)
    uint32_t* cnt;                 // [C + 1] its population count
    const uint64_t* wr;            // [C + 1] non-zero entries before chunk c
    const uint64_t* nraw;          // [J] non-zero entries before list j
    const uint64_t* offsets;       // [N + 1]
    uint64_t m;                    // max_per_kmer (0: all)
    uint64_t* out;                 // positions out
    uint64_t* rid_out;             // nullable
    uint64_t* local_out;           // nullable
    const uint64_t *rs, *re, *rr;  // interval starts / ends / rids
    uint64_t rn;
};

template <bool WRITE>
__global__ void __launch_bounds__(kB) k_pq_flat(const PqFlat P) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * kB + threadIdx.x) >> 6, nwaves = (uint64_t)gridDim.x * (kB / 64);
    const uint64_t per = (P.C + nwaves - 1) / nwaves;
    const uint64_t c0 = wave * per, c1 = min(P.C, c0 + per);
    if (c0 >= c1) return;                                      // wave-uniform
    uint64_t j0 = wave_count_le(P.nfo, P.J, c0 * 64) - 1;      // nfo[0] == 0: the list that holds the tile's first entry
    for (uint64_t c = c0; c < c1; ++c) {
        const uint64_t base = c * 64, f = base + lane;
        const uint64_t stv = P.nfo[j0 + lane];                 // the chunk's lists start within the next 64 entries of nfo (lists are non-empty); padding = T
        const uint32_t d = stv <= base ? 0u : (uint32_t)min(stv - base, (uint64_t)64);      // ascending over the lanes, d of lane 0 is 0
        uint32_t k = 0;                                        // the last lane whose list starts at or before f
#pragma unroll
        for (uint32_t s = 32; s; s >>= 1) {
            const uint32_t t = k + s;
            const uint32_t dv = bperm(t & 63u, d);
            if (t < 64u && dv <= lane) k = t;
        }
        const bool active = f < P.T;
        uint64_t v = 0, j = j0 + k;
        if (active) v = P.positions[P.nlo[j] + (f - P.nfo[j])];
        const uint64_t nz = __ballot(v != 0);
        if (!WRITE) {
            if (lane == 0) { P.bits[c] = nz; P.cnt[c] = (uint32_t)__popcll(nz); }
        } else if (v != 0) {
            const uint64_t r = P.wr[c] + (uint64_t)__popcll(nz & ((1ull << lane) - 1ull)) - P.nraw[j];      // rank inside its list
            if (P.m == 0 || r < P.m) {
                const uint64_t dst = P.offsets[P.ne[j]] + r, p = v - 1;
                P.out[dst] = p;
                if (P.rid_out) {
                    uint64_t rd, sv;
                    pq_locate(P.rs, P.re, P.rr, P.rn, p, rd, sv);
                    P.rid_out[dst] = rd;
                    P.local_out[dst] = p - sv;
                }
            }
        }
        const uint64_t jl = j0 + (uint64_t)__shfl(k, 63);      // the list of the chunk's last entry; the next chunk starts there or one further
        j0 = jl + (P.nfo[jl + 1] <= base + 64 ? 1 : 0);
    }
}

// 4. kept[ne[j]] = min(m, non-zeros of list j); nraw[j] = non-zeros before it
__device__ __forceinline__ uint64_t pq_rank(const uint64_t* __restrict__ bits, const uint64_t* __restrict__ wr, uint64_t f) {
    const uint64_t w = f >> 6;
    return wr[w] + (uint64_t)__popcll(bits[w] & ((1ull << (f & 63)) - 1ull));
}
__global__ void __launch_bounds__(kB) k_pq_segrank(const uint64_t* __restrict__ bits, const uint64_t* __restrict__ wr, const uint64_t* __restrict__ nfo,
                                                  const uint64_t* __restrict__ ne, uint64_t J, uint64_t m, uint64_t* __restrict__ nraw,
                                                  uint64_t* __restrict__ kept) {
    const uint64_t stride = (uint64_t)gridDim.x * kB;
    for (uint64_t j = (uint64_t)blockIdx.x * kB + threadIdx.x; j < J; j += stride) {
        const uint64_t r0 = pq_rank(bits, wr, nfo[j]), r1 = pq_rank(bits, wr, nfo[j + 1]);
        nraw[j] = r0;
        const uint64_t nzs = r1 - r0;
        kept[ne[j]] = (m && nzs > m) ? m : nzs;
    }
}

__global__ void __launch_bounds__(kB) k_pq_locate(const uint64_t* __restrict__ pos, uint64_t N, const uint64_t* __restrict__ rs, const uint64_t* __restrict__ re,
                                                 const uint64_t* __restrict__ rr, uint64_t rn, uint64_t* __restrict__ rid_out, uint64_t* __restrict__ start_out) {
    const uint64_t stride = (uint64_t)gridDim.x * kB;
    for (uint64_t i = (uint64_t)blockIdx.x * kB + threadIdx.x; i < N; i += stride) {
        uint64_t r, s;
        pq_locate(rs, re, rr, rn, pos[i], r, s);
        rid_out[i] = r;
        start_out[i] = s;
    }
}

struct PqNonEmpty { __host__ __device__ uint64_t operator()(uint64_t v) const { return v ? 1ull : 0ull; } };

static unsigned pq_flat_grid(uint64_t C) {
    const uint64_t want = (C + 4 * 8 - 1) / (4 * 8);           // at least eight chunks per wave, four waves per workgroup
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(want, 4096));
}

// Steps 2 to 5 (aix_posquery.hpp) for N lists already resolved.
hipError_t posquery_lists(aix_index* h, const uint64_t* d_lo, const uint64_t* d_ub, uint64_t N, uint64_t m, uint64_t* d_offsets, uint64_t* d_positions,
                          uint64_t* d_rid, uint64_t* d_local, uint64_t cap, uint64_t* total_out, hipStream_t s, DevArr* own_pos) {
    *total_out = 0;
    if (N == 0) return hipMemsetAsync(d_offsets, 0, 8, s);
    DevArr fo(s), nj(s), t0(s), t1(s), t2(s), t3(s), ne(s), nfo(s), nlo(s), nraw(s), bits(s), cnt(s), wr(s), kept(s);
    AIX_TRY(fo.alloc(8 * (N + 1)));
    AIX_TRY(nj.alloc(8 * (N + 1)));
    AIX_TRY(scan_u64(d_ub, (uint64_t*)fo.p, N + 1, t0, s));
    AIX_TRY(scan_u64(rocprim::make_transform_iterator(d_ub, PqNonEmpty()), (uint64_t*)nj.p, N + 1, t1, s));
    uint64_t T = 0, J = 0;        // read back asynchronously: declared after the DevArrs, whose destructors synchronise `s` before an early return leaves the frame
    AIX_TRY(hipMemcpyAsync(&T, (const uint64_t*)fo.p + N, 8, hipMemcpyDeviceToHost, s));
    AIX_TRY(hipMemcpyAsync(&J, (const uint64_t*)nj.p + N, 8, hipMemcpyDeviceToHost, s));
    AIX_TRY(hipStreamSynchronize(s));
    if (T == 0) return hipMemsetAsync(d_offsets, 0, 8 * (N + 1), s);
    const uint64_t C = (T + 63) / 64;
    AIX_TRY(ne.alloc(8 * J));
    AIX_TRY(nfo.alloc(8 * (J + kPad)));
    AIX_TRY(nlo.alloc(8 * J));
    AIX_TRY(nraw.alloc(8 * J));
    AIX_TRY(bits.alloc(8 * (C + 1)));
    AIX_TRY(cnt.alloc(4 * (C + 1)));
    AIX_TRY(wr.alloc(8 * (C + 1)));
    AIX_TRY(kept.alloc(8 * (N + 1)));
    AIX_TRY_LAUNCH(k_pq_compact, dim3(flat_grid(std::max(N, kPad))), dim3(kB), 0, s, N, d_ub, (const uint64_t*)fo.p, (const uint64_t*)nj.p, d_lo, J, T,
                   (uint64_t*)ne.p, (uint64_t*)nfo.p, (uint64_t*)nlo.p);
    AIX_TRY(hipMemsetAsync((uint64_t*)bits.p + C, 0, 8, s));
    AIX_TRY(hipMemsetAsync((uint32_t*)cnt.p + C, 0, 4, s));
    AIX_TRY(hipMemsetAsync(kept.p, 0, 8 * (N + 1), s));
    PqFlat P{};
    P.positions = h->att.ai_positions.as<uint64_t>(); P.ne = (const uint64_t*)ne.p; P.nfo = (const uint64_t*)nfo.p; P.nlo = (const uint64_t*)nlo.p;
    P.J = J; P.T = T; P.C = C; P.bits = (uint64_t*)bits.p; P.cnt = (uint32_t*)cnt.p; P.wr = (const uint64_t*)wr.p; P.nraw = (const uint64_t*)nraw.p;
    P.offsets = d_offsets; P.m = m;
    AIX_TRY_LAUNCH(k_pq_flat<false>, dim3(pq_flat_grid(C)), dim3(kB), 0, s, P);
    AIX_TRY(scan_u64(rocprim::make_transform_iterator((const uint32_t*)cnt.p, Widen<uint32_t>()), (uint64_t*)wr.p, C + 1, t2, s));
    AIX_TRY_LAUNCH(k_pq_segrank, dim3(flat_grid(J)), dim3(kB), 0, s, (const uint64_t*)bits.p, (const uint64_t*)wr.p, (const uint64_t*)nfo.p, (const uint64_t*)ne.p, J, m,
                   (uint64_t*)nraw.p, (uint64_t*)kept.p);
    AIX_TRY(scan_u64((const uint64_t*)kept.p, d_offsets, N + 1, t3, s));
    uint64_t total = 0;
    AIX_TRY(hipMemcpyAsync(&total, d_offsets + N, 8, hipMemcpyDeviceToHost, s));
    AIX_TRY(hipStreamSynchronize(s));
    *total_out = total;
    if (own_pos && total) {
        AIX_TRY(own_pos->alloc(8 * total));
        d_positions = (uint64_t*)own_pos->p;
        cap = total;
    }
    if (total == 0 || total > cap || !d_positions) return hipSuccess;
    P.out = d_positions;
    if (d_rid) {
        P.rid_out = d_rid; P.local_out = d_local;
        const uint64_t* const rx = h->att.rx.as<uint64_t>();
        P.rs = rx; P.re = rx + h->att.rx_n; P.rr = rx + 2 * h->att.rx_n; P.rn = h->att.rx_n;
    }
    AIX_TRY_LAUNCH(k_pq_flat<true>, dim3(pq_flat_grid(C)), dim3(kB), 0, s, P);
    return hipStreamSynchronize(s);                            // the scratch blocks go back to the pool idle
}

// The whole chain. d_offsets (N + 1) and *total_out are always produced; entries only when *total_out <= cap.
hipError_t posquery_run(aix_index* h, const uint8_t* d_kmers, uint64_t N, uint64_t m, uint64_t* d_offsets, uint64_t* d_positions, uint64_t* d_rid,
                               uint64_t* d_local, uint64_t cap, uint64_t* total_out, hipStream_t s) {
    *total_out = 0;
    if (N == 0) return hipMemsetAsync(d_offsets, 0, 8, s);
    const IndexDev ix = h->dev();
    const uint64_t* const indices = h->att.ai_indices.as<uint64_t>();
    const uint64_t total = h->att.ai_total;
    DevArr lo(s), ub(s);
    AIX_TRY(lo.alloc(8 * N));
    AIX_TRY(ub.alloc(8 * (N + 1)));
    uint64_t* d_ub = (uint64_t*)ub.p;
    AIX_TRY(hipMemsetAsync(d_ub + N, 0, 8, s));
    if (h->k == 13) AIX_TRY_LAUNCH(k_pq_resolve13, dim3(flat_grid(N)), dim3(kB), 0, s, ix.perm13, d_kmers, N, indices, total, (uint64_t*)lo.p, d_ub);
    else if (ix.bk_lpp == 2) AIX_TRY_LAUNCH(k_pq_resolve23<2>, dim3(flat_grid(N)), dim3(kB), 0, s, ix, d_kmers, N, indices, total, (uint64_t*)lo.p, d_ub);
    else if (ix.bk_lpp == 4) AIX_TRY_LAUNCH(k_pq_resolve23<4>, dim3(flat_grid(N)), dim3(kB), 0, s, ix, d_kmers, N, indices, total, (uint64_t*)lo.p, d_ub);
    else AIX_TRY_LAUNCH(k_pq_resolve23<8>, dim3(flat_grid(N)), dim3(kB), 0, s, ix, d_kmers, N, indices, total, (uint64_t*)lo.p, d_ub);
    return posquery_lists(h, (const uint64_t*)lo.p, d_ub, N, m, d_offsets, d_positions, d_rid, d_local, cap, total_out, s);
}

}  // namespace aix

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
static void pq_detach_aindex(Attachments& a) {
    a.ai_indices.reset();
    a.ai_positions.reset();
    a.ai_total = 0;
}

static int pq_validate(aix_index* h, const uint64_t* d_indices, uint64_t total, hipStream_t s) {
    DevBuf flag(s);
    uint32_t bad = 0;
    AIXCHK(flag.alloc(4));
    AIXCHK(hipMemsetAsync(flag.p, 0, 4, s));
    hipLaunchKernelGGL(k_pq_validate, dim3(flat_grid(h->n + 1)), dim3(kB), 0, s, d_indices, h->n, total, (uint32_t*)flag.p);
    AIXCHK(hipGetLastError());
    AIXCHK(hipMemcpyAsync(&bad, flag.p, 4, hipMemcpyDeviceToHost, s));
    AIXCHK(hipStreamSynchronize(s));
    return bad ? AIX_ERR_FORMAT : AIX_OK;
}

extern "C" int aix_aindex_attach(aix_index_t* h, const uint64_t* indices, const uint64_t* positions, uint64_t total) {
    if (!h || !indices || (total && !positions)) return AIX_ERR_ARG;
    if (total >= (1ull << 60)) return AIX_ERR_NOMEM;
    DevGuard g(h->device);
    HBlock di, dp;                                             // never a partial copy: what is not attached below is freed here
    hipError_t e = di.alloc(8 * (h->n + 1));
    if (e == hipSuccess) e = dp.alloc(total ? 8 * total : 8, 8 * total);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (e == hipErrorOutOfMemory) return AIX_ERR_NOMEM;
        set_last_error(std::string("hipMalloc: ") + hipGetErrorString(e));
        return AIX_ERR_HIP;
    }
    e = hipMemcpy(di.p, indices, 8 * (h->n + 1), hipMemcpyHostToDevice);
    if (e == hipSuccess && total) e = hipMemcpy(dp.p, positions, 8 * total, hipMemcpyHostToDevice);
    if (e != hipSuccess) { set_last_error(std::string("hipMemcpy: ") + hipGetErrorString(e)); return AIX_ERR_HIP; }
    if (const int st = pq_validate(h, di.as<uint64_t>(), total, 0)) return st;
    pq_detach_aindex(h->att);
    h->att.ai_indices.attach_owned(std::move(di));
    h->att.ai_positions.attach_owned(std::move(dp));
    h->att.ai_total = total;
    return AIX_OK;
}

extern "C" int aix_aindex_attach_dev(aix_index_t* h, const uint64_t* d_indices, const uint64_t* d_positions, uint64_t total, void* stream) {
    if (!h || !d_indices || (total && !d_positions)) return AIX_ERR_ARG;
    DevGuard g(h->device);
    const int st = pq_validate(h, d_indices, total, (hipStream_t)stream);
    if (st) return st;
    pq_detach_aindex(h->att);
    h->att.ai_indices.attach_borrowed(d_indices);
    h->att.ai_positions.attach_borrowed(d_positions);
    h->att.ai_total = total;
    return AIX_OK;
}

extern "C" int aix_aindex_detach(aix_index_t* h) {
    if (!h) return AIX_ERR_ARG;
    DevGuard g(h->device);
    (void)hipDeviceSynchronize();
    pq_detach_aindex(h->att);
    h->att.rx.drop();
    h->att.rx_n = 0;
    return AIX_OK;
}

extern "C" int aix_ridx_sorted_disjoint(const uint64_t* triples, uint64_t n_reads) {
    if (n_reads && !triples) return 0;
    for (uint64_t i = 0; i < n_reads; ++i) {
        const uint64_t st = triples[3 * i + 1], en = triples[3 * i + 2];
        if (en < st) return 0;
        if (i && st <= triples[3 * (i - 1) + 2]) return 0;
    }
    return 1;
}

extern "C" int aix_ridx_attach(aix_index_t* h, const uint64_t* triples, uint64_t n_reads) {
    if (!h || (n_reads && !triples)) return AIX_ERR_ARG;
    if (!aix_ridx_sorted_disjoint(triples, n_reads)) return AIX_ERR_UNSUPPORTED;
    DevGuard g(h->device);
    std::vector<uint64_t> soa;
    try { soa.resize(3 * n_reads); } catch (const std::bad_alloc&) { return AIX_ERR_NOMEM; }
    for (uint64_t i = 0; i < n_reads; ++i) {
        soa[i] = triples[3 * i + 1];
        soa[n_reads + i] = triples[3 * i + 2];
        soa[2 * n_reads + i] = triples[3 * i];
    }
    HBlock d;
    AIXCHK(d.alloc(n_reads ? 24 * n_reads : 8, 24 * n_reads));
    if (n_reads) AIXCHK(hipMemcpy(d.p, soa.data(), 24 * n_reads, hipMemcpyHostToDevice));
    if (h->att.rx) (void)hipDeviceSynchronize();
    h->att.rx = std::move(d);
    h->att.rx_n = n_reads;
    return AIX_OK;
}

extern "C" int aix_positions_query_dev(aix_index_t* h, const char* d_kmers, uint64_t N, uint64_t max_per_kmer, uint64_t* d_offsets, uint64_t* d_positions,
                                       uint64_t* d_rid, uint64_t* d_local, uint64_t cap, uint64_t* total_out, void* stream) {
    if (!h || !d_offsets || !total_out || (N && !d_kmers) || ((d_rid == nullptr) != (d_local == nullptr))) return AIX_ERR_ARG;
    if (!h->att.ai_indices.attached || (d_rid && !h->att.rx)) return AIX_ERR_ARG;     // nothing attached: a defined error, never a fault
    if (h->k == 23 && h->n == 0) return AIX_ERR_UNSUPPORTED;
    DevGuard g(h->device);
    AIXCHK(posquery_run(h, (const uint8_t*)d_kmers, N, max_per_kmer, d_offsets, cap ? d_positions : nullptr, d_rid, d_local, cap, total_out, (hipStream_t)stream));
    return AIX_OK;
}

extern "C" int aix_positions_query(aix_index_t* h, const char* kmers, uint64_t N, uint64_t max_per_kmer, uint64_t** offsets_out, uint64_t** positions_out,
                                   uint64_t** rid_out, uint64_t** local_out) {
    if (!h || !offsets_out || !positions_out || (N && !kmers) || ((rid_out == nullptr) != (local_out == nullptr))) return AIX_ERR_ARG;
    *offsets_out = *positions_out = nullptr;
    if (rid_out) *rid_out = *local_out = nullptr;
    if (!h->att.ai_indices.attached || (rid_out && !h->att.rx)) return AIX_ERR_ARG;
    if (h->k == 23 && h->n == 0) return AIX_ERR_UNSUPPORTED;
    DevGuard g(h->device);
    DevArr dq, doff, dpos, drid, dloc;
    AIXCHK(upload_padded(dq, kmers, N * h->k));
    AIXCHK(doff.alloc(8 * (N + 1)));
    uint64_t total = 0;
    AIXCHK(posquery_run(h, (const uint8_t*)dq.p, N, max_per_kmer, (uint64_t*)doff.p, nullptr, nullptr, nullptr, 0, &total, 0));
    if (total) {
        AIXCHK(dpos.alloc(8 * total));
        if (rid_out) { AIXCHK(drid.alloc(8 * total)); AIXCHK(dloc.alloc(8 * total)); }
        uint64_t again = 0;
        AIXCHK(posquery_run(h, (const uint8_t*)dq.p, N, max_per_kmer, (uint64_t*)doff.p, (uint64_t*)dpos.p, (uint64_t*)drid.p, (uint64_t*)dloc.p, total, &again, 0));
        if (again != total) { set_last_error("aix_positions_query: the index changed between the sizing and the filling pass"); return AIX_ERR_HIP; }
    }
    const HostOut outs[] = {{(void**)offsets_out, doff.p, 8 * (N + 1)}, {(void**)positions_out, dpos.p, 8 * total}, {(void**)rid_out, drid.p, 8 * total},
                            {(void**)local_out, dloc.p, 8 * total}};
    AIXCHK(copy_out_host(outs, 4));
    return AIX_OK;
}

extern "C" int aix_positions_locate_dev(aix_index_t* h, const uint64_t* d_pos, uint64_t N, uint64_t* d_rid, uint64_t* d_start, void* stream) {
    if (!h || (N && (!d_pos || !d_rid || !d_start))) return AIX_ERR_ARG;
    if (!h->att.rx) return AIX_ERR_ARG;
    if (N == 0) return AIX_OK;
    DevGuard g(h->device);
    hipLaunchKernelGGL(k_pq_locate, dim3(flat_grid(N)), dim3(kB), 0, (hipStream_t)stream, d_pos, N, h->att.rx.as<uint64_t>(), h->att.rx.as<uint64_t>() + h->att.rx_n, h->att.rx.as<uint64_t>() + 2 * h->att.rx_n, h->att.rx_n, d_rid, d_start);
    AIXCHK(hipGetLastError());
    return AIX_OK;
}

extern "C" int aix_positions_locate(aix_index_t* h, const uint64_t* pos, uint64_t N, uint64_t* rid_out, uint64_t* start_out) {
    if (!h || (N && (!pos || !rid_out || !start_out))) return AIX_ERR_ARG;
    if (!h->att.rx) return AIX_ERR_ARG;
    if (N == 0) return AIX_OK;
    DevGuard g(h->device);
    DevArr dp, dr, ds;
    const HostIn in{pos, 8 * N};
    AIXCHK(copy_in_host(&dp, &in, 1));
    AIXCHK(dr.alloc(8 * N));
    AIXCHK(ds.alloc(8 * N));
    const int st = aix_positions_locate_dev(h, (const uint64_t*)dp.p, N, (uint64_t*)dr.p, (uint64_t*)ds.p, nullptr);
    if (st) return st;
    AIXCHK(hipMemcpy(rid_out, dr.p, 8 * N, hipMemcpyDeviceToHost));
    AIXCHK(hipMemcpy(start_out, ds.p, 8 * N, hipMemcpyDeviceToHost));
    return AIX_OK;
}
