// aix_readsquery.hip — batch read retrieval over a reads file resident in HBM.
//   AindexWrapper::get_read_by_rid       python_wrapper.cpp:666-675   rid -> the read's bytes
//   AindexWrapper::get_read              python_wrapper.cpp:677-698   (start, end, revcomp) -> bytes, reversed and complemented on request
//   AindexWrapper::get_reads_se_by_kmer  python_wrapper.cpp:857-911   k-mer -> the reads that hold it (contract: the project's own
//                                        AindexWrapper.get_reads_se_by_kmer, aindex_amd/wrapper.py; the reference crosses its two arrays)
//
// The reference returns one std::string per call. Here R spans of 0 .. millions of bytes are one ragged byte gather, written back to back
// (CSR: offsets[R + 1], bytes[offsets[R]]). The chain:
//   1 k_rq_spans_*   one lane per item: source start and length of its span (the bounds rules of get_read / get_read_by_rid)
//   2 scan of the lengths = offsets[]
//   3 k_rq_gather    the OUTPUT byte space, seen from the 16-byte alignment of the output pointer, is cut into tiles of 64 chunks of 16 bytes
//                    (one chunk per lane, 1 KiB per wave and step). A wave owns a run of consecutive tiles: one wave-wide search of offsets[]
//                    finds the run's first span; per tile the next 64 offsets sit one per lane and a lane finds its span among them with
//                    ds_bpermute (a tile with more than 63 span starts — empty or tiny spans — falls back to a per-lane bisection). A 100 Mbp
//                    contig is spread over the whole grid and a thousand 100-byte reads are a hundred KiB of tiles, not a thousand waves.
//                    A chunk that lies inside one span is one 16-byte load (the source takes the misalignment) and one aligned 16-byte
//                    store; a chunk that crosses a span boundary, or the ragged first / last chunk, goes byte by byte. The revcomp form reads
//                    the mirrored 16 source bytes, swaps them end to end and complements eight bytes at a time with integer operations.
// aix_reads_by_kmers puts four passes in front: posquery_run (k-mers -> CSR of positions), k_rk_locate (entry -> list and interval),
// first occurrence of every (list, interval) — by comparing with the left neighbour when every list is ascending in its intervals, else
// through two stable radix sorts (by interval, then by list) —, and two scans that rank the first occurrences inside their list for the
// max_reads rule. Every size, offset and byte index is 64 bits wide. No atomics; all stores are plain vector stores.
#include <algorithm>

#include "aix_posquery.hpp"                                       // upload_padded; the rest is aix_hostkit.hpp

namespace aix {

static constexpr int kRB = kFlatBlock;                            // the grid of the flat kernels: flat_grid (aix_hostkit.hpp)

// ---------------------------------------------------------------------------------------------
// 1. spans
// ---------------------------------------------------------------------------------------------
// get_read (:677-698): empty when start >= size || end >= size || start > end, else [start, end)
__global__ void __launch_bounds__(kRB) k_rq_spans_fetch(const uint64_t* __restrict__ start, const uint64_t* __restrict__ end, uint64_t N, uint64_t size,
                                                       uint64_t* __restrict__ src, uint64_t* __restrict__ len) {
    const uint64_t stride = (uint64_t)gridDim.x * kRB;
    for (uint64_t i = (uint64_t)blockIdx.x * kRB + threadIdx.x; i <= N; i += stride) {
        uint64_t s = 0, l = 0;
        if (i < N) {
            const uint64_t a = start[i], b = end[i];
            if (a < size && b < size && a <= b) { s = a; l = b - a; }
        }
        if (i < N) src[i] = s;
        len[i] = l;                                            // len[N] = 0: the scan's last entry is the total
    }
}

// row r of the intervals, clamped to the attached buffer; empty when r >= n_reads (get_read_by_rid, :666-675)
__device__ __forceinline__ void rq_row(const uint64_t* __restrict__ rs, const uint64_t* __restrict__ re, uint64_t rn, uint64_t size, uint64_t r, uint64_t& s,
                                       uint64_t& l) {
    s = 0; l = 0;
    if (r < rn) {
        const uint64_t a = rs[r], b = min(re[r], size);
        if (a < b) { s = a; l = b - a; }
    }
}

__global__ void __launch_bounds__(kRB) k_rq_spans_rid(const uint64_t* __restrict__ rid, uint64_t N, const uint64_t* __restrict__ rs, const uint64_t* __restrict__ re,
                                                     uint64_t rn, uint64_t size, uint64_t* __restrict__ src, uint64_t* __restrict__ len) {
    const uint64_t stride = (uint64_t)gridDim.x * kRB;
    for (uint64_t i = (uint64_t)blockIdx.x * kRB + threadIdx.x; i <= N; i += stride) {
        uint64_t s = 0, l = 0;
        if (i < N) { rq_row(rs, re, rn, size, rid[i], s, l); src[i] = s; }
        len[i] = l;
    }
}

// ---------------------------------------------------------------------------------------------
// 3. the gather
// ---------------------------------------------------------------------------------------------
struct RqGather {
    const uint8_t* reads;          // the attached buffer
    const uint64_t* src;           // [R] source start of span j
    const uint64_t* off;           // [R + 1] output start of span j; off[R] = total
    const uint8_t* rc;             // [R] non-zero: reversed and complemented (RC form only)
    uint64_t R, total;
    uint8_t* out;
};

struct Rq16 { uint64_t lo, hi; };
__device__ __forceinline__ Rq16 rq_load16(const uint8_t* p) {   // any alignment: the compiler emits one 16-byte global load (unaligned access mode)
    Rq16 v;
    __builtin_memcpy(&v, p, 16);
    return v;
}

// bit 7 of every byte of x that equals c
__device__ __forceinline__ uint64_t rq_eq(uint64_t x, uint64_t c) {
    const uint64_t y = x ^ (0x0101010101010101ull * c), l7 = 0x7F7F7F7F7F7F7F7Full;
    return ~(((y & l7) + l7) | y | l7);
}
// A <-> T, C <-> G in eight bytes at once; every other byte stays (python_wrapper.cpp:686-693)
__device__ __forceinline__ uint64_t rq_comp8(uint64_t x) {
    const uint64_t at = (rq_eq(x, 'A') | rq_eq(x, 'T')) >> 7, cg = (rq_eq(x, 'C') | rq_eq(x, 'G')) >> 7;
    return x ^ (at * 0x15u) ^ (cg * 0x04u);                    // 'A' ^ 'T' = 0x15, 'C' ^ 'G' = 0x04
}
__device__ __forceinline__ uint8_t rq_comp1(uint8_t c) {
    return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c;
}

template <bool RC>
__global__ void __launch_bounds__(kRB) k_rq_gather(const RqGather P) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * kRB + threadIdx.x) >> 6, nwaves = (uint64_t)gridDim.x * (kRB / 64);
    const uint64_t head = (uint64_t)(uintptr_t)P.out & 15u;    // output byte o sits in chunk (o + head) / 16 of the aligned space
    const uint64_t nchunks = (P.total + head + 15) >> 4, tiles = (nchunks + 63) >> 6;
    const uint64_t per = (tiles + nwaves - 1) / nwaves;
    const uint64_t t0 = wave * per, t1 = min(tiles, t0 + per);
    if (t0 >= t1) return;                                      // wave-uniform
    const uint64_t b0 = t0 ? t0 * 1024 - head : 0, b1 = min(P.total, t1 * 1024 - head);      // the run's output bytes [b0, b1)
    uint64_t jt = wave_count_le(P.off, P.R + 1, b0) - 1;       // off[0] == 0: the last span that starts at or before b0 (it holds b0)
    const uint64_t jhi = wave_count_le(P.off, P.R + 1, b1 - 1) - 1;
    for (uint64_t t = t0; t < t1; ++t) {
        const uint64_t tb0 = t ? t * 1024 - head : 0, tb1 = min(P.total, (t + 1) * 1024 - head);
        const uint64_t c = t * 64 + lane;
        const uint64_t lo = c ? c * 16 - head : 0, hi = min(P.total, (c + 1) * 16 - head);
        const bool active = lo < hi;
        const uint64_t ov = P.off[min(jt + lane, P.R)];        // the next 64 span starts (ascending); beyond the last span: total
        const uint64_t last = __shfl(ov, 63);
        uint64_t j;
        if (last >= tb1) {                                     // wave-uniform: every span that starts inside the tile is among them
            const uint32_t d = ov <= tb0 ? 0u : (uint32_t)min(ov - tb0, (uint64_t)2048), want = (uint32_t)(lo - tb0);
            uint32_t k = 0;                                    // the last lane whose span starts at or before lo (d of lane 0 is 0)
#pragma unroll
            for (uint32_t s = 32; s; s >>= 1) {
                const uint32_t q = k + s;
                const uint32_t dv = bperm(q & 63u, d);
                if (q < 64u && dv <= want) k = q;
            }
            j = jt + k;
            jt += (uint64_t)__popcll(__ballot(ov <= tb1)) - 1; // the span that holds the next tile's first byte, or an empty one at its start
        } else {
            uint64_t a = jt, b = jhi;                          // the last j in [jt, jhi] with off[j] <= lo
            if (active) {
                while (a < b) {
                    const uint64_t mid = a + ((b - a + 1) >> 1);
                    if (P.off[mid] <= lo) a = mid; else b = mid - 1;
                }
            }
            j = a;
            if (tb1 < P.total) jt = wave_count_le(P.off, P.R + 1, tb1) - 1;
        }
        if (!active) continue;
        uint64_t sj = P.off[j], ej = P.off[j + 1];             // sj <= lo < ej
        if (hi - lo == 16 && ej >= hi) {
            const uint64_t at = lo - sj;
            Rq16 v;
            if (RC && P.rc[j]) {
                const Rq16 m = rq_load16(P.reads + P.src[j] + ((ej - sj) - 16 - at));       // the mirrored 16 bytes
                v.lo = rq_comp8(__builtin_bswap64(m.hi));
                v.hi = rq_comp8(__builtin_bswap64(m.lo));
            } else {
                v = rq_load16(P.reads + P.src[j] + at);
            }
            *reinterpret_cast<ulonglong2*>(P.out + lo) = make_ulonglong2(v.lo, v.hi);       // (out + lo) % 16 == 0
        } else {
            for (uint64_t o = lo; o < hi; ++o) {
                while (o >= ej) { ++j; sj = ej; ej = P.off[j + 1]; }                        // o < total: j stays below R; empty spans are stepped over
                const uint64_t at = o - sj;
                uint8_t ch;
                if (RC && P.rc[j]) ch = rq_comp1(P.reads[P.src[j] + (ej - sj) - 1 - at]);
                else ch = P.reads[P.src[j] + at];
                P.out[o] = ch;
            }
        }
    }
}

static unsigned rq_gather_grid(uint64_t total) {
    const uint64_t tiles = (total + 15 + 1023) / 1024;
    const uint64_t want = (tiles + 4 * 8 - 1) / (4 * 8);       // at least eight tiles per wave, four waves per workgroup
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(want, 4096));
}

// passes 2 and 3: d_len (R + 1, last entry 0) -> d_offsets (R + 1) and *total_out, always; the bytes only when *total_out <= cap
static hipError_t rq_gather_run(aix_index* h, const uint64_t* d_src, const uint64_t* d_len, const uint8_t* d_rc, uint64_t R, uint64_t* d_offsets, uint8_t* d_bytes,
                                uint64_t cap, uint64_t* total_out, hipStream_t s) {
    *total_out = 0;
    DevArr tmp(s);
    AIX_TRY(scan_u64(d_len, d_offsets, R + 1, tmp, s));
    uint64_t total = 0;           // read back asynchronously: declared after the DevArrs, whose destructors synchronise `s` before an early return leaves the frame
    AIX_TRY(hipMemcpyAsync(&total, d_offsets + R, 8, hipMemcpyDeviceToHost, s));
    AIX_TRY(hipStreamSynchronize(s));
    *total_out = total;
    if (total == 0 || total > cap || !d_bytes) return hipSuccess;
    RqGather P{};
    P.reads = h->att.rd.as<uint8_t>(); P.src = d_src; P.off = d_offsets; P.rc = d_rc; P.R = R; P.total = total; P.out = d_bytes;
    if (d_rc) AIX_TRY_LAUNCH(k_rq_gather<true>, dim3(rq_gather_grid(total)), dim3(kRB), 0, s, P);
    else AIX_TRY_LAUNCH(k_rq_gather<false>, dim3(rq_gather_grid(total)), dim3(kRB), 0, s, P);
    return hipStreamSynchronize(s);                            // the scratch blocks go back to the pool idle
}

// ---------------------------------------------------------------------------------------------
// k-mers -> reads: first occurrence of every (list, interval), ranked inside its list
// ---------------------------------------------------------------------------------------------
// IntervalTree::query(pos, pos + 1) of python_wrapper.cpp:66-74 on sorted, disjoint intervals (pq_locate of aix_posquery.hip), as the
// INDEX of the interval; n when there is none
__device__ __forceinline__ uint64_t rk_interval(const uint64_t* __restrict__ st, const uint64_t* __restrict__ en, uint64_t n, uint64_t p) {
    const uint64_t key = p ? p - 1 : 0;
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (en[mid] < key) lo = mid + 1; else hi = mid;
    }
    if (lo < n) {
        const uint64_t sv = st[lo];
        if (sv <= p || sv == p + 1) return lo;
    }
    return n;
}

// entry e of the positions CSR: lst[e] = its k-mer, key[e] = its interval (rn: none)
__global__ void __launch_bounds__(kRB) k_rk_locate(const uint64_t* __restrict__ off, uint64_t N, const uint64_t* __restrict__ pos, uint64_t T,
                                                  const uint64_t* __restrict__ rs, const uint64_t* __restrict__ re, uint64_t rn, uint64_t* __restrict__ lst,
                                                  uint64_t* __restrict__ key) {
    const uint64_t stride = (uint64_t)gridDim.x * kRB;
    for (uint64_t e = (uint64_t)blockIdx.x * kRB + threadIdx.x; e < T; e += stride) {
        uint64_t a = 0, b = N - 1;                             // the last i with off[i] <= e (off[N] = T > e)
        while (a < b) {
            const uint64_t mid = a + ((b - a + 1) >> 1);
            if (off[mid] <= e) a = mid; else b = mid - 1;
        }
        lst[e] = a;
        key[e] = rk_interval(rs, re, rn, pos[e]);
    }
}

// is some list not ascending in its intervals? (then "same interval as my left neighbour" does not find every repeat)
__global__ void __launch_bounds__(kRB) k_rk_ascending(const uint64_t* __restrict__ lst, const uint64_t* __restrict__ key, uint64_t T, uint32_t* __restrict__ flag) {
    const uint64_t stride = (uint64_t)gridDim.x * kRB;
    bool bad = false;
    for (uint64_t e = (uint64_t)blockIdx.x * kRB + threadIdx.x + 1; e < T; e += stride) bad |= lst[e] == lst[e - 1] && key[e] < key[e - 1];
    if (bad) *flag = 1u;
}

__global__ void __launch_bounds__(kRB) k_rk_gather_lst(const uint64_t* __restrict__ lst, const uint64_t* __restrict__ perm, uint64_t T, uint64_t* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * kRB;
    for (uint64_t i = (uint64_t)blockIdx.x * kRB + threadIdx.x; i < T; i += stride) out[i] = lst[perm[i]];
}

// flags of entry e = perm[i] (perm == nullptr: e = i), entries ordered by (list, interval, e): bit 0 = first occurrence of its interval in
// its list, bit 1 = and the read is not empty (row rid of the intervals, clamped to the buffer)
__global__ void __launch_bounds__(kRB) k_rk_first(const uint64_t* __restrict__ perm, const uint64_t* __restrict__ lst, const uint64_t* __restrict__ key, uint64_t T,
                                                 const uint64_t* __restrict__ rs, const uint64_t* __restrict__ re, const uint64_t* __restrict__ rr, uint64_t rn,
                                                 uint64_t size, uint8_t* __restrict__ flags) {
    const uint64_t stride = (uint64_t)gridDim.x * kRB;
    for (uint64_t i = (uint64_t)blockIdx.x * kRB + threadIdx.x; i < T; i += stride) {
        const uint64_t e = perm ? perm[i] : i;
        const uint64_t k = key[e];
        bool first = k < rn;
        if (first && i) {
            const uint64_t p = perm ? perm[i - 1] : i - 1;
            first = lst[p] != lst[e] || key[p] != k;
        }
        uint8_t f = 0;
        if (first) {
            uint64_t s, l;
            rq_row(rs, re, rn, size, rr[k], s, l);
            f = l ? 3 : 1;
        }
        flags[e] = f;
    }
}

// get_reads_se_by_kmer's loop: a first occurrence is appended when its read is not empty, and the limit is tested after every first
// occurrence: m >= 1 keeps the first m non-empty reads, m == 0 looks at the first located occurrence only.
// rank = exclusive scan of bit 1 (m >= 1) or of bit 0 (m == 0)
__global__ void __launch_bounds__(kRB) k_rk_keep(const uint8_t* __restrict__ flags, const uint64_t* __restrict__ rank, const uint64_t* __restrict__ lst,
                                                const uint64_t* __restrict__ off, uint64_t T, uint64_t m, uint8_t* __restrict__ keep) {
    const uint64_t stride = (uint64_t)gridDim.x * kRB;
    for (uint64_t e = (uint64_t)blockIdx.x * kRB + threadIdx.x; e <= T; e += stride) {
        uint8_t k = 0;
        if (e < T && (flags[e] & 2)) k = rank[e] - rank[off[lst[e]]] < (m ? m : 1) ? 1 : 0;
        keep[e] = k;
    }
}

// kmer_offsets[i] = kept entries before list i; per kept entry: the read id, its span
__global__ void __launch_bounds__(kRB) k_rk_emit(const uint8_t* __restrict__ keep, const uint64_t* __restrict__ orank, const uint64_t* __restrict__ key,
                                                const uint64_t* __restrict__ off, uint64_t N, uint64_t T, const uint64_t* __restrict__ rs,
                                                const uint64_t* __restrict__ re, const uint64_t* __restrict__ rr, uint64_t rn, uint64_t size, uint64_t R,
                                                uint64_t* __restrict__ kmer_offsets, uint64_t* __restrict__ rid_out, uint64_t* __restrict__ src,
                                                uint64_t* __restrict__ len) {
    const uint64_t stride = (uint64_t)gridDim.x * kRB;
    const uint64_t M = max(T, N + 1);
    for (uint64_t e = (uint64_t)blockIdx.x * kRB + threadIdx.x; e < M; e += stride) {
        if (e <= N && kmer_offsets) kmer_offsets[e] = orank[off[e]];
        if (rid_out && e < T && keep[e]) {
            const uint64_t o = orank[e], r = rr[key[e]];
            uint64_t s, l;
            rq_row(rs, re, rn, size, r, s, l);
            rid_out[o] = r; src[o] = s; len[o] = l;
        }
        if (rid_out && e == 0) len[R] = 0;
    }
}

struct RkFlagBit {
    uint8_t bit;
    __host__ __device__ uint64_t operator()(uint8_t v) const { return (uint64_t)((v >> bit) & 1u); }
};

// the positions of every k-mer (posquery_run), then the dedup. Outputs in pool blocks the caller owns: d_koff (N + 1), and — R reads —
// rid / src (R) and len (R + 1, last 0).
static hipError_t rk_run(aix_index* h, const uint8_t* d_kmers, uint64_t N, uint64_t m, uint64_t* d_koff, DevArr& rid, DevArr& src, DevArr& len, uint64_t* R_out,
                         hipStream_t s) {
    *R_out = 0;
    if (N == 0) return hipMemsetAsync(d_koff, 0, 8, s);
    DevArr off(s), pos(s), lst(s), key(s), flag(s), perm(s), k2(s), k3(s), p2(s), tmp(s), flags(s), rank(s), keep(s), orank(s), t1(s), t2(s);
    AIX_TRY(off.alloc(8 * (N + 1)));
    uint64_t T = 0, again = 0;
    AIX_TRY(posquery_run(h, d_kmers, N, 0, (uint64_t*)off.p, nullptr, nullptr, nullptr, 0, &T, s));
    if (T == 0) return hipMemsetAsync(d_koff, 0, 8 * (N + 1), s);
    AIX_TRY(pos.alloc(8 * T));
    AIX_TRY(posquery_run(h, d_kmers, N, 0, (uint64_t*)off.p, (uint64_t*)pos.p, nullptr, nullptr, T, &again, s));
    if (again != T) return hipErrorUnknown;
    AIX_TRY(lst.alloc(8 * T));
    AIX_TRY(key.alloc(8 * T));
    AIX_TRY(flag.alloc(4));
    AIX_TRY(flags.alloc(T + 1));
    AIX_TRY(rank.alloc(8 * (T + 1)));
    AIX_TRY(keep.alloc(T + 1));
    AIX_TRY(orank.alloc(8 * (T + 1)));
    AIX_TRY(hipMemsetAsync(flag.p, 0, 4, s));
    const uint64_t rn = h->att.rx_n;
    const uint64_t *rs = h->att.rx.as<uint64_t>(), *re = rs + rn, *rr = rs + 2 * rn;
    const uint64_t *d_off = (const uint64_t*)off.p, *d_lst = (const uint64_t*)lst.p, *d_key = (const uint64_t*)key.p;
    AIX_TRY_LAUNCH(k_rk_locate, dim3(flat_grid(T)), dim3(kRB), 0, s, d_off, N, (const uint64_t*)pos.p, T, rs, re, rn, (uint64_t*)lst.p, (uint64_t*)key.p);
    AIX_TRY_LAUNCH(k_rk_ascending, dim3(flat_grid(T)), dim3(kRB), 0, s, d_lst, d_key, T, (uint32_t*)flag.p);
    uint32_t unsorted = 0;
    AIX_TRY(hipMemcpyAsync(&unsorted, flag.p, 4, hipMemcpyDeviceToHost, s));
    AIX_TRY(hipStreamSynchronize(s));
    const uint64_t* d_perm = nullptr;
    if (unsorted) {
        // some bucket's slots are not in ascending order (files written by a multi-threaded compute_aindex): entries ordered by
        // (list, interval, entry) through two stable radix sorts of the entry numbers, by interval and then by list. Both passes are
        // sized first and share one block of the larger size (so not with_temp, which takes a block per call).
        AIX_TRY(perm.alloc(8 * T));
        AIX_TRY(k2.alloc(8 * T));
        AIX_TRY(p2.alloc(8 * T));
        AIX_TRY(k3.alloc(8 * T));
        size_t tb = 0, tb2 = 0;
        const unsigned kb = sort_bits(rn), lb = sort_bits(N);
        rocprim::counting_iterator<uint64_t> iota(0);
        AIX_TRY(rocprim::radix_sort_pairs(nullptr, tb, d_key, (uint64_t*)k2.p, iota, (uint64_t*)perm.p, (size_t)T, 0u, kb, s));
        AIX_TRY(rocprim::radix_sort_pairs(nullptr, tb2, (const uint64_t*)k3.p, (uint64_t*)k2.p, (const uint64_t*)perm.p, (uint64_t*)p2.p, (size_t)T, 0u, lb, s));
        AIX_TRY(tmp.alloc(std::max<size_t>(std::max(tb, tb2), 1)));
        AIX_TRY(rocprim::radix_sort_pairs(tmp.p, tb, d_key, (uint64_t*)k2.p, iota, (uint64_t*)perm.p, (size_t)T, 0u, kb, s));
        AIX_TRY_LAUNCH(k_rk_gather_lst, dim3(flat_grid(T)), dim3(kRB), 0, s, d_lst, (const uint64_t*)perm.p, T, (uint64_t*)k3.p);
        AIX_TRY(rocprim::radix_sort_pairs(tmp.p, tb2, (const uint64_t*)k3.p, (uint64_t*)k2.p, (const uint64_t*)perm.p, (uint64_t*)p2.p, (size_t)T, 0u, lb, s));
        d_perm = (const uint64_t*)p2.p;
    }
    AIX_TRY_LAUNCH(k_rk_first, dim3(flat_grid(T)), dim3(kRB), 0, s, d_perm, d_lst, d_key, T, rs, re, rr, rn, h->att.rd_len, (uint8_t*)flags.p);
    AIX_TRY(hipMemsetAsync((uint8_t*)flags.p + T, 0, 1, s));
    AIX_TRY(scan_u64(rocprim::make_transform_iterator((const uint8_t*)flags.p, RkFlagBit{(uint8_t)(m ? 1 : 0)}), (uint64_t*)rank.p, T + 1, t1, s));
    AIX_TRY_LAUNCH(k_rk_keep, dim3(flat_grid(T + 1)), dim3(kRB), 0, s, (const uint8_t*)flags.p, (const uint64_t*)rank.p, d_lst, d_off, T, m, (uint8_t*)keep.p);
    AIX_TRY(scan_u64(rocprim::make_transform_iterator((const uint8_t*)keep.p, Widen<uint8_t>()), (uint64_t*)orank.p, T + 1, t2, s));
    uint64_t R = 0;
    AIX_TRY(hipMemcpyAsync(&R, (const uint64_t*)orank.p + T, 8, hipMemcpyDeviceToHost, s));
    AIX_TRY(hipStreamSynchronize(s));
    AIX_TRY(rid.alloc(8 * std::max<uint64_t>(R, 1)));
    AIX_TRY(src.alloc(8 * std::max<uint64_t>(R, 1)));
    AIX_TRY(len.alloc(8 * (R + 1)));
    *R_out = R;
    AIX_TRY_LAUNCH(k_rk_emit, dim3(flat_grid(std::max(T, N + 1))), dim3(kRB), 0, s, (const uint8_t*)keep.p, (const uint64_t*)orank.p, d_key, d_off, N, T, rs, re, rr, rn,
                   h->att.rd_len, R, d_koff, (uint64_t*)rid.p, (uint64_t*)src.p, (uint64_t*)len.p);
    return hipStreamSynchronize(s);
}

}  // namespace aix

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
static void rq_detach(Attachments& a) {
    a.rd.reset();
    a.rd_len = 0;
}

extern "C" int aix_reads_attach(aix_index_t* h, const char* reads, uint64_t len) {
    if (!h || (len && !reads)) return AIX_ERR_ARG;
    if (len >= (1ull << 60)) return AIX_ERR_NOMEM;
    DevGuard g(h->device);
    HBlock d;
    hipError_t e = d.alloc(len ? len : 1, len);
    if (e != hipSuccess) {                                     // nothing is kept; an earlier attachment stays
        (void)hipGetLastError();
        if (e == hipErrorOutOfMemory) return AIX_ERR_NOMEM;
        set_last_error(std::string("hipMalloc: ") + hipGetErrorString(e));
        return AIX_ERR_HIP;
    }
    if (len) AIXCHK(hipMemcpy(d.p, reads, len, hipMemcpyHostToDevice));
    (void)hipDeviceSynchronize();
    h->att.rd.attach_owned(std::move(d));
    h->att.rd_len = len;
    return AIX_OK;
}

extern "C" int aix_reads_attach_dev(aix_index_t* h, const char* d_reads, uint64_t len, void* stream) {
    if (!h || (len && !d_reads)) return AIX_ERR_ARG;
    DevGuard g(h->device);
    AIXCHK(hipStreamSynchronize((hipStream_t)stream));          // what filled the buffer on `stream` has completed before any query reads it
    (void)hipDeviceSynchronize();
    h->att.rd.attach_borrowed(d_reads);
    h->att.rd_len = len;
    return AIX_OK;
}

extern "C" int aix_reads_detach(aix_index_t* h) {
    if (!h) return AIX_ERR_ARG;
    DevGuard g(h->device);
    (void)hipDeviceSynchronize();
    rq_detach(h->att);
    return AIX_OK;
}

extern "C" int aix_reads_info(const aix_index_t* h, uint64_t out[2]) {
    if (!h || !out) return AIX_ERR_ARG;
    out[0] = h->att.rd.attached ? (h->att.rd.owned ? 1 : 2) : 0;
    out[1] = h->att.rd_len;
    return AIX_OK;
}

extern "C" int aix_reads_fetch_dev(aix_index_t* h, const uint64_t* d_start, const uint64_t* d_end, const uint8_t* d_revcomp, uint64_t N, uint64_t* d_offsets,
                                   char* d_bytes, uint64_t cap, uint64_t* total_out, void* stream) {
    if (!h || !d_offsets || !total_out || (N && (!d_start || !d_end))) return AIX_ERR_ARG;
    if (!h->att.rd.attached) return AIX_ERR_ARG;                   // nothing attached: a defined error, never a fault
    DevGuard g(h->device);
    hipStream_t s = (hipStream_t)stream;
    DevArr src(s), len(s);
    AIXCHK(src.alloc(8 * std::max<uint64_t>(N, 1)));
    AIXCHK(len.alloc(8 * (N + 1)));
    hipLaunchKernelGGL(k_rq_spans_fetch, dim3(flat_grid(N + 1)), dim3(kRB), 0, s, d_start, d_end, N, h->att.rd_len, (uint64_t*)src.p, (uint64_t*)len.p);
    AIXCHK(hipGetLastError());
    AIXCHK(rq_gather_run(h, (const uint64_t*)src.p, (const uint64_t*)len.p, d_revcomp, N, d_offsets, cap ? (uint8_t*)d_bytes : nullptr, cap, total_out, s));
    return AIX_OK;
}

extern "C" int aix_reads_fetch_rid_dev(aix_index_t* h, const uint64_t* d_rid, uint64_t N, uint64_t* d_offsets, char* d_bytes, uint64_t cap, uint64_t* total_out,
                                       void* stream) {
    if (!h || !d_offsets || !total_out || (N && !d_rid)) return AIX_ERR_ARG;
    if (!h->att.rd.attached || !h->att.rx) return AIX_ERR_ARG;
    DevGuard g(h->device);
    hipStream_t s = (hipStream_t)stream;
    DevArr src(s), len(s);
    AIXCHK(src.alloc(8 * std::max<uint64_t>(N, 1)));
    AIXCHK(len.alloc(8 * (N + 1)));
    hipLaunchKernelGGL(k_rq_spans_rid, dim3(flat_grid(N + 1)), dim3(kRB), 0, s, d_rid, N, h->att.rx.as<uint64_t>(), h->att.rx.as<uint64_t>() + h->att.rx_n, h->att.rx_n, h->att.rd_len, (uint64_t*)src.p, (uint64_t*)len.p);
    AIXCHK(hipGetLastError());
    AIXCHK(rq_gather_run(h, (const uint64_t*)src.p, (const uint64_t*)len.p, nullptr, N, d_offsets, cap ? (uint8_t*)d_bytes : nullptr, cap, total_out, s));
    return AIX_OK;
}

static int rk_check(const aix_index* h) {
    if (!h->att.rd.attached || !h->att.rx || !h->att.ai_indices.attached) return AIX_ERR_ARG;
    if (h->k == 23 && h->n == 0) return AIX_ERR_UNSUPPORTED;
    return AIX_OK;
}

extern "C" int aix_reads_by_kmers_dev(aix_index_t* h, const char* d_kmers, uint64_t N, uint64_t max_reads, uint64_t* d_kmer_offsets, uint64_t* d_rid,
                                      uint64_t* d_read_offsets, uint64_t cap_reads, char* d_bytes, uint64_t cap_bytes, uint64_t totals_out[2], void* stream) {
    if (!h || !d_kmer_offsets || !totals_out || (N && !d_kmers)) return AIX_ERR_ARG;
    if (const int st = rk_check(h)) return st;
    DevGuard g(h->device);
    hipStream_t s = (hipStream_t)stream;
    totals_out[0] = totals_out[1] = 0;
    DevArr rid(s), src(s), len(s), roff(s);
    uint64_t R = 0, total = 0;
    AIXCHK(rk_run(h, (const uint8_t*)d_kmers, N, max_reads, d_kmer_offsets, rid, src, len, &R, s));
    if (R) {
        AIXCHK(roff.alloc(8 * (R + 1)));
        const bool fits = R <= cap_reads && d_rid && d_read_offsets;
        AIXCHK(rq_gather_run(h, (const uint64_t*)src.p, (const uint64_t*)len.p, nullptr, R, (uint64_t*)roff.p, fits && cap_bytes ? (uint8_t*)d_bytes : nullptr, cap_bytes,
                            &total, s));
        if (fits) {
            AIXCHK(hipMemcpyAsync(d_rid, rid.p, 8 * R, hipMemcpyDeviceToDevice, s));
            AIXCHK(hipMemcpyAsync(d_read_offsets, roff.p, 8 * (R + 1), hipMemcpyDeviceToDevice, s));
            AIXCHK(hipStreamSynchronize(s));
        }
    } else if (d_read_offsets) {
        AIXCHK(zero_offsets(d_read_offsets, 0, s));            // read_offsets = {0}
    }
    totals_out[0] = R; totals_out[1] = total;
    return AIX_OK;
}

template <class Sizer>
static int rq_host_fetch(uint64_t N, uint64_t** offsets_out, char** bytes_out, Sizer run) {
    *offsets_out = nullptr; *bytes_out = nullptr;
    DevArr doff, dby;
    AIXCHK(doff.alloc(8 * (N + 1)));
    uint64_t total = 0, again = 0;
    if (const int st = run((uint64_t*)doff.p, nullptr, 0, &total)) return st;
    if (total) {
        AIXCHK(dby.alloc(total));
        if (const int st = run((uint64_t*)doff.p, (char*)dby.p, total, &again)) return st;
        if (again != total) { set_last_error("aix_reads_fetch: the attachment changed between the sizing and the filling pass"); return AIX_ERR_HIP; }
    }
    const HostOut outs[] = {{(void**)offsets_out, doff.p, 8 * (N + 1)}, {(void**)bytes_out, dby.p, total}};
    AIXCHK(copy_out_host(outs, 2));
    return AIX_OK;
}

extern "C" int aix_reads_fetch(aix_index_t* h, const uint64_t* start, const uint64_t* end, const uint8_t* revcomp, uint64_t N, uint64_t** offsets_out,
                               char** bytes_out) {
    if (!h || !offsets_out || !bytes_out || (N && (!start || !end))) return AIX_ERR_ARG;
    *offsets_out = nullptr; *bytes_out = nullptr;
    if (!h->att.rd.attached) return AIX_ERR_ARG;
    DevGuard g(h->device);
    DevArr in[3];                                              // start, end, revcomp (no block when none is given or N == 0)
    const HostIn ins[3] = {{start, 8 * N}, {end, 8 * N}, {N ? revcomp : nullptr, N}};
    AIXCHK(copy_in_host(in, ins, 2));
    AIXCHK(copy_in_host(in + 2, ins + 2, 1, true));
    return rq_host_fetch(N, offsets_out, bytes_out, [&](uint64_t* off, char* by, uint64_t cap, uint64_t* tot) {
        return aix_reads_fetch_dev(h, (const uint64_t*)in[0].p, (const uint64_t*)in[1].p, (const uint8_t*)in[2].p, N, off, by, cap, tot, nullptr);
    });
}

extern "C" int aix_reads_fetch_rid(aix_index_t* h, const uint64_t* rid, uint64_t N, uint64_t** offsets_out, char** bytes_out) {
    if (!h || !offsets_out || !bytes_out || (N && !rid)) return AIX_ERR_ARG;
    *offsets_out = nullptr; *bytes_out = nullptr;
    if (!h->att.rd.attached || !h->att.rx) return AIX_ERR_ARG;
    DevGuard g(h->device);
    DevArr dr;
    const HostIn in{rid, 8 * N};
    AIXCHK(copy_in_host(&dr, &in, 1));
    return rq_host_fetch(N, offsets_out, bytes_out, [&](uint64_t* off, char* by, uint64_t cap, uint64_t* tot) {
        return aix_reads_fetch_rid_dev(h, (const uint64_t*)dr.p, N, off, by, cap, tot, nullptr);
    });
}

extern "C" int aix_reads_by_kmers(aix_index_t* h, const char* kmers, uint64_t N, uint64_t max_reads, uint64_t** kmer_offsets_out, uint64_t** rid_out,
                                  uint64_t** read_offsets_out, char** bytes_out) {
    if (!h || !kmer_offsets_out || !rid_out || !read_offsets_out || !bytes_out || (N && !kmers)) return AIX_ERR_ARG;
    *kmer_offsets_out = *rid_out = *read_offsets_out = nullptr;
    *bytes_out = nullptr;
    if (const int st = rk_check(h)) return st;
    DevGuard g(h->device);
    DevArr dq, dko, dby, rid, src, len, roff;
    AIXCHK(upload_padded(dq, kmers, N * h->k));
    AIXCHK(dko.alloc(8 * (N + 1)));
    uint64_t R = 0, total = 0, again = 0;
    AIXCHK(rk_run(h, (const uint8_t*)dq.p, N, max_reads, (uint64_t*)dko.p, rid, src, len, &R, nullptr));
    AIXCHK(roff.alloc(8 * (R + 1)));
    if (R) {
        AIXCHK(rq_gather_run(h, (const uint64_t*)src.p, (const uint64_t*)len.p, nullptr, R, (uint64_t*)roff.p, nullptr, 0, &total, nullptr));
        AIXCHK(dby.alloc(total));
        AIXCHK(rq_gather_run(h, (const uint64_t*)src.p, (const uint64_t*)len.p, nullptr, R, (uint64_t*)roff.p, (uint8_t*)dby.p, total, &again, nullptr));
    } else {
        AIXCHK(hipMemset(roff.p, 0, 8));
    }
    const HostOut outs[] = {{(void**)kmer_offsets_out, dko.p, 8 * (N + 1)}, {(void**)rid_out, rid.p, 8 * R}, {(void**)read_offsets_out, roff.p, 8 * (R + 1)},
                            {(void**)bytes_out, dby.p, total}};
    AIXCHK(copy_out_host(outs, 4));
    return AIX_OK;
}
