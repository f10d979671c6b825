// aix_k1.hip — K1 row (kmer_counter: count_kmers.cpp:297-341, distinct canonical k-mers with their counts) without a
// full-width library sort. The window codes (k_window_codes, 2k <= 46 bits) are partitioned most-significant-digit first
// in two levels, and every final bucket is counted and ordered inside LDS:
//
//   k_k1_split    level 1: 16 384-code tiles are counting-sorted in LDS by the top 11 bits (rank = one returning LDS atomic
//                 per code) and each partition's run is appended to the workgroup's current 128-entry chunk of that partition
//                 (chunk ids from a per-workgroup region, as in aix_count13.hip: nothing is sized beforehand)
//   directory     (partition, fill) of every chunk, sorted by partition (a few 10^5 u16 keys)
//   k_k1_count    level 2, pass 1: one workgroup per level-1 partition histograms the next D2 bits -> bucket sizes
//   scan          bucket sizes -> bucket bases (exact: level 2 writes contiguous buckets, no chunk lists)
//   k_k1_scatter  level 2, pass 2: the partition's chunks are tile-sorted in LDS by those D2 bits and written out as runs of
//                 32-bit remainders at the bucket bases
//   k_k1_final    one workgroup per bucket (~10^3 codes): open-addressing hash table in LDS (a k-mer that occurs 10^5 times is
//                 ONE slot and 10^5 LDS adds — heavy hitters cost no capacity), distinct keys compacted and bitonic-sorted in
//                 LDS, (key, count) written at the bucket base
//   k_k1_gather   buckets closed up into the final arrays (bucket order = key order)
//
// D2 is chosen so that a bucket holds ~10^3 codes. A bucket with more than K1_DMAX distinct remainders (possible only when
// the codes are far from uniform in their top 11 + D2 bits) raises a flag and the caller falls back to the radix-sort path
// (distinct_from_codes, at the end of this file): the result never depends on which path ran.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "aix_env.hpp"
#include "aix_msd.hpp"

namespace aix {

// ---------------------------------------------------------------------------------------------
// level 1 source: sixteen codes per lane and tile
// ---------------------------------------------------------------------------------------------
// The windows of a PLAIN buffer, encoded here (count_kmers.cpp:93-136,297-308: A/C/G/T/U either case, canonical form by
// canon_mode): a lane owns 16 consecutive window starts, its 16 + k - 1 bytes are turned ONCE into a 2-bit stream (4 bytes per
// step) and every window is a shift of it — no 8-byte code per window is written to and read back from HBM.
struct K1Plain {
    const uint8_t* buf;
    uint64_t len;         // bytes
    uint64_t n;           // windows = len - k + 1
    int k, canon_mode;
    __device__ __forceinline__ void load(uint64_t tile, int t, uint64_t (&c)[K1_WPT]) const {
        constexpr int ND = 10;                                // 40 bytes >= 16 + 23 - 1
        const uint64_t S = tile * K1_TILE + (uint64_t)t * K1_WPT;
#pragma unroll
        for (int j = 0; j < K1_WPT; ++j) c[j] = K1_INVALID;
        if (S >= n) return;
        uint32_t e[ND];
        {
            const uint32_t o = (uint32_t)((uintptr_t)(buf + S) & 3);
            const uint32_t* q = (const uint32_t*)(buf + S - o);
            const int64_t first = (int64_t)S - o, end = (int64_t)len;
            uint32_t d[ND + 1];
#pragma unroll
            for (int i = 0; i <= ND; ++i) d[i] = (first + 4 * i < end) ? q[i] : 0x0A0A0A0Au;   // never read a dword past the buffer
            const uint32_t sh = o * 8;
#pragma unroll
            for (int i = 0; i < ND; ++i) e[i] = __funnelshift_r(d[i], d[i + 1], sh);
        }
        uint32_t w[3] = {0, 0, 0};
        uint64_t vmask = 0;
#pragma unroll
        for (int i = 0; i < ND; ++i) {
            uint32_t x = e[i] & 0xDFDFDFDFu;
            {   // 'U' -> 'T' (count_kmers.cpp:71-88)
                const uint32_t z = x ^ 0x55555555u;
                const uint32_t nz = (((z & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | z) & 0x80808080u;
                x ^= (~nz & 0x80808080u) >> 7;
            }
            const uint32_t v = ((x >> 1) ^ (x >> 2)) & 0x03030303u;
            const uint32_t diff = x ^ lut4(v, AIX_LUT_ACGT);
            const uint32_t z = ~(((diff & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | diff | 0x7F7F7F7Fu);    // 0x80 in every byte where diff == 0
            const uint32_t f = z >> 7;
            const uint32_t nib = (f | (f >> 7) | (f >> 14) | (f >> 21)) & 0xFu;
            const uint32_t q2 = ((v << 6) & 0xC0u) | ((v >> 4) & 0x30u) | ((v >> 14) & 0x0Cu) | (v >> 24);
            w[i >> 2] |= q2 << (24 - 8 * (i & 3));
            vmask |= (uint64_t)nib << (4 * i);
        }
        const uint64_t avail = len - S;                        // bytes from S to the end of the buffer
        if (avail < 40) vmask &= (1ull << avail) - 1;
        // window j holds a k-mer iff k consecutive mask bits are set
        uint64_t run = vmask;
        for (int i = 1; i < k; ++i) run &= vmask >> i;
        const uint64_t hi = ((uint64_t)w[0] << 32) | w[1], lo = (uint64_t)w[2] << 32;
        const uint64_t kmask = (1ULL << (2 * k)) - 1;
#pragma unroll
        for (int j = 0; j < K1_WPT; ++j) {
            if (!((run >> j) & 1ull) || S + j >= n) continue;
            const int sh = 128 - 2 * j - 2 * k;                // >= 52
            uint64_t code = (sh >= 64 ? (hi >> (sh - 64)) : ((hi << (64 - sh)) | (lo >> sh))) & kmask;
            if (canon_mode == 1) { const uint64_t x = revcomp_refx86(code, k); code = code < x ? code : x; }
            else if (canon_mode == 2) { const uint64_t x = revcomp(code, k); code = code < x ? code : x; }
            c[j] = code;
        }
    }
};


// ---------------------------------------------------------------------------------------------
// per bucket: hash aggregation + sort of the distinct remainders, all in LDS
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(K1_FB) k_k1_final(const uint32_t* __restrict__ in32, const uint32_t* __restrict__ bucket_base, uint32_t nbuckets, uint32_t s2,
                                                   uint64_t* __restrict__ keys_out, uint32_t* __restrict__ cnt_out, uint32_t* __restrict__ distinct_m,
                                                   uint32_t* __restrict__ overflow) {
    __shared__ uint32_t hk[K1_CAP];          // remainder + 1 (0 = empty)
    __shared__ uint32_t hc[K1_CAP];
    __shared__ __attribute__((aligned(16))) uint32_t dk[K1_DMAX + 4];      // + the +infinity padding of the rank pass
    __shared__ uint32_t dc[K1_DMAX];
    __shared__ uint32_t m_out;
    const uint32_t t = threadIdx.x;
    // A bucket is ~10^3 entries: its global loads (two bases, then the entries) are a dependent chain of HBM latencies that
    // would dominate the few microseconds of LDS work. The base pair and the first 1024 entries of the NEXT bucket are therefore
    // fetched into registers while this one is processed.
    uint32_t nlo = 0, nn = 0, pre[K1_PRE];
    auto prefetch = [&](uint32_t b) {
        nn = 0;
        if (b < nbuckets) {
            nlo = bucket_base[b];
            nn = bucket_base[b + 1] - nlo;
#pragma unroll
            for (int q = 0; q < K1_PRE; ++q) { const uint32_t i = t + q * K1_FB; pre[q] = i < nn ? in32[nlo + i] : 0u; }
        }
    };
    prefetch(blockIdx.x);
    // invariant at the top of every bucket: dk[] holds +infinity everywhere, so the rank pass can read whole 16-byte vectors past the
    // last distinct key; the entries a bucket has used are reset when the next one begins (every wave has passed the closing barrier)
    for (uint32_t i = t; i < (uint32_t)K1_DMAX + 4u; i += K1_FB) dk[i] = 0xFFFFFFFFu;
    uint32_t used = 0;                                          // entries of dk the previous bucket wrote (uniform)
    for (uint32_t b = blockIdx.x; b < nbuckets; b += gridDim.x) {
        const uint32_t lo = nlo, n_e = nn;
        uint32_t cur[K1_PRE];
#pragma unroll
        for (int q = 0; q < K1_PRE; ++q) cur[q] = pre[q];
        prefetch(b + gridDim.x);
        if (n_e == 0) { if (t == 0) distinct_m[b] = 0; continue; }
        // table size: a power of two >= 2 x (the most distinct remainders this bucket can be allowed to hold)
        uint32_t cap = 64;
        const uint32_t want = 2u * min(n_e, (uint32_t)K1_DMAX);
        while (cap < want && cap < (uint32_t)K1_CAP) cap <<= 1;
        for (uint32_t i = t; i < cap; i += K1_FB) { hk[i] = 0; hc[i] = 0; }
        for (uint32_t i = t; i < used; i += K1_FB) dk[i] = 0xFFFFFFFFu;
        used = 0;
        if (t == 0) m_out = 0;
        __syncthreads();
        auto insert = [&](uint32_t v) {
            const uint32_t key = v + 1u;                         // remainders are < 2^31 (s2 <= 31): + 1 cannot wrap to the empty marker
            uint32_t h = (key * 0x9E3779B1u) >> 7;
            for (uint32_t probes = 0; probes < cap; ++probes) {
                h &= cap - 1;
                const uint32_t old = atomicCAS(&hk[h], 0u, key);
                if (old == 0u || old == key) { atomicAdd(&hc[h], 1u); break; }
                ++h;
            }
        };
#pragma unroll
        for (int q = 0; q < K1_PRE; ++q) if (t + q * K1_FB < n_e) insert(cur[q]);
        for (uint32_t i = t + K1_PRE * K1_FB; i < n_e; i += K1_FB) insert(in32[lo + i]);      // the tail of an oversized bucket
        __syncthreads();
        // compaction of the occupied slots: one LDS atomic per WAVE (ballot + prefix popcount), not one per distinct key on one address
        for (uint32_t i0 = 0; i0 < cap; i0 += K1_FB) {
            const uint32_t i = i0 + t;
            const uint32_t k = i < cap ? hk[i] : 0u;
            const uint64_t mask = __ballot(k != 0u);
            uint32_t base = 0;
            if ((t & 63u) == 0u && mask) base = atomicAdd(&m_out, (uint32_t)__popcll(mask));
            base = __shfl(base, 0);
            if (k) {
                const uint32_t idx = base + (uint32_t)__popcll(mask & ((1ull << (t & 63u)) - 1ull));
                if (idx < (uint32_t)K1_DMAX) { dk[idx] = k - 1u; dc[idx] = hc[i]; }
            }
        }
        __syncthreads();
        const uint32_t m = m_out;
        used = min(m, (uint32_t)K1_DMAX);
        if (m > (uint32_t)K1_DMAX) {                             // too many distinct remainders for the LDS arrays (or a full table dropped some)
            if (t == 0) { *overflow = 1u; distinct_m[b] = 0; }
            __syncthreads();
            continue;
        }
        const uint64_t prefix = (uint64_t)b << s2;               // bucket id = the top 11 + D2 bits of the code
        if (m <= 384u) {
            // few distinct keys (the usual case: a bucket's ~10^3 entries are ~10^2 distinct k-mers at sequencing depth): every lane
            // ranks its key by counting the smaller ones (broadcast reads, no conflicts) and stores it straight at its place — no
            // further barrier, instead of the dozens a bitonic network needs
            for (uint32_t i = t; i < m; i += K1_FB) {
                const uint32_t key = dk[i];
                uint32_t r = 0;
                const uint32_t m16 = (m + 15u) & ~15u;                  // dk is +infinity past m (at least up to the next multiple of 16: K1_DMAX + 4 entries, m <= 384)
                for (uint32_t j = 0; j < m16; j += 16) {                // four independent 16-byte reads in flight
                    const uint4 v0 = *reinterpret_cast<const uint4*>(&dk[j]), v1 = *reinterpret_cast<const uint4*>(&dk[j + 4]);
                    const uint4 v2 = *reinterpret_cast<const uint4*>(&dk[j + 8]), v3 = *reinterpret_cast<const uint4*>(&dk[j + 12]);
                    r += (v0.x < key ? 1u : 0u) + (v0.y < key ? 1u : 0u) + (v0.z < key ? 1u : 0u) + (v0.w < key ? 1u : 0u);
                    r += (v1.x < key ? 1u : 0u) + (v1.y < key ? 1u : 0u) + (v1.z < key ? 1u : 0u) + (v1.w < key ? 1u : 0u);
                    r += (v2.x < key ? 1u : 0u) + (v2.y < key ? 1u : 0u) + (v2.z < key ? 1u : 0u) + (v2.w < key ? 1u : 0u);
                    r += (v3.x < key ? 1u : 0u) + (v3.y < key ? 1u : 0u) + (v3.z < key ? 1u : 0u) + (v3.w < key ? 1u : 0u);
                }
                keys_out[lo + r] = prefix | key;
                cnt_out[lo + r] = dc[i];
            }
        } else {
            // many distinct keys: bitonic sort of (dk, dc) by dk inside LDS. Every compare-exchange points upwards (the first step of a
            // merge pairs mirror positions), so m needs no rounding up to a power of two: a partner index at or past m is a virtual
            // +infinity that would never move — nothing is read or written past the m entries
            uint32_t half_p = 1;
            while (2 * half_p < m) half_p <<= 1;                 // pairs per step = P / 2, P = the power of two >= m
            auto cmpx = [&](uint32_t a, uint32_t x) {
                if (x < m) {
                    const uint32_t ka = dk[a], kb = dk[x];
                    if (ka > kb) { dk[a] = kb; dk[x] = ka; const uint32_t ca = dc[a]; dc[a] = dc[x]; dc[x] = ca; }
                }
            };
            for (uint32_t k = 2; k <= 2 * half_p; k <<= 1) {
                const uint32_t hk2 = k >> 1;
                for (uint32_t p = t; p < half_p; p += K1_FB) {
                    const uint32_t blk = p / hk2 * k, pos = p & (hk2 - 1);
                    cmpx(blk + pos, blk + k - 1 - pos);
                }
                __syncthreads();
                for (uint32_t j = k >> 2; j > 0; j >>= 1) {
                    for (uint32_t p = t; p < half_p; p += K1_FB) {
                        const uint32_t a = ((p & ~(j - 1)) << 1) | (p & (j - 1));
                        cmpx(a, a + j);
                    }
                    __syncthreads();
                }
            }
            for (uint32_t i = t; i < m; i += K1_FB) {
                keys_out[lo + i] = prefix | dk[i];
                cnt_out[lo + i] = dc[i];
            }
        }
        if (t == 0) distinct_m[b] = m;
        __syncthreads();
    }
}

// buckets closed up: bucket b's m entries move from its base to dm_off[b]; one wave per bucket
// CNT = uint64_t: what the merge of pieces and kmer_counter's output carry is written here, no widening pass
template <typename CNT>
__global__ void __launch_bounds__(256) k_k1_gather(const uint64_t* __restrict__ keys_st, const uint32_t* __restrict__ cnt_st, const uint32_t* __restrict__ bucket_base,
                                                  const uint32_t* __restrict__ dm_off, uint32_t nbuckets, uint64_t* __restrict__ keys, CNT* __restrict__ counts) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t nw = (uint64_t)gridDim.x * 4;
    for (uint64_t b = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); b < nbuckets; b += nw) {
        const uint32_t src = bucket_base[b], dst = dm_off[b], m = dm_off[b + 1] - dst;
        for (uint32_t i = lane; i < m; i += 64) { keys[dst + i] = keys_st[src + i]; counts[dst + i] = (CNT)cnt_st[src + i]; }
    }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
bool k1_msd_eligible(uint64_t nwin, int k) {
    if (env_flag("AIX_K1_ROCPRIM")) return false;      // A/B switch: the radix-sort path
    return k >= 9 && k <= 23 && nwin > 0 && nwin <= (1ull << 31);
}

hipError_t distinct_from_codes_msd(const uint8_t* d_plain, uint64_t plen, uint64_t nwin, int k, int canon_mode, uint64_t* d_staging, K1Scratch& scratch, DevArr& keys,
                                   DevArr& counts, uint64_t* n_out, bool* fell_back, hipStream_t s) {
    *n_out = 0; *fell_back = false;
    const uint32_t B = 2u * (uint32_t)k, s1 = B - K1_PBITS;
    // D2: ~768 codes per bucket on average; the remainder must fit 32 bits
    uint32_t D2 = 3;
    while (D2 < 11 && (nwin >> (K1_PBITS + D2)) > 900) ++D2;
    while (s1 - D2 > 31) ++D2;                                  // remainder + 1 must not wrap (0 marks an empty hash slot)
    if (D2 > s1) D2 = s1;
    const uint32_t s2 = s1 - D2;
    const MsdPlan P(nwin, 1u << D2, (uint32_t)env_int("AIX_K1_TEST_REGION", 1, LONG_MAX, 0), s);   // test hook: an undersized region must fail loudly
    const uint32_t nbuckets = P.nbuckets;
    // behind the head (word 0: region exhausted, word 1: a bucket overflowed): distinct_m (nbuckets + 1) | dm_off | parts
    const uint64_t o_dm = P.head_bytes, o_dmo = o_dm + up256(4ull * (nbuckets + 1)), o_parts = o_dmo + up256(4ull * (nbuckets + 1));
    AIX_TRY(K1Scratch::need(scratch.work, scratch.work_bytes, o_parts + P.parts_bytes()));
    uint8_t* w = (uint8_t*)scratch.work.p;
    uint32_t* overflow = (uint32_t*)w + 1;
    uint32_t* bucket_base = P.bucket_base(w);
    uint32_t* distinct_m = (uint32_t*)(w + o_dm);
    uint32_t* dm_off = (uint32_t*)(w + o_dmo);
    // the staging (8 B per window): its first half takes the 32-bit remainders of level 2, its second half the per-bucket counts;
    // the chunk array (>= 8 B per window) is free after level 2 and takes the per-bucket keys
    uint32_t* out32 = (uint32_t*)d_staging;
    uint32_t* cnt_st = (uint32_t*)d_staging + nwin;
    uint64_t* parts = (uint64_t*)(w + o_parts);
    uint64_t* keys_st = parts;
    AIX_TRY(hipMemsetAsync(distinct_m, 0, 4ull * (nbuckets + 1), s));
    AIX_TRY(msd_partition(P, w, K1Plain{d_plain, plen, nwin, k, canon_mode}, s1, s2, parts, out32, s));
    AIX_TRY_LAUNCH(k_k1_final, dim3(std::min<uint32_t>(nbuckets, 256u * 5u)), dim3(K1_FB), 0, s, (const uint32_t*)out32, (const uint32_t*)bucket_base, nbuckets, s2, keys_st,
                   cnt_st, distinct_m, overflow);
    AIX_TRY(P.scan(w, distinct_m, dm_off, s));
    uint32_t flags[2] = {0, 0}, total_distinct = 0;
    AIX_TRY(hipMemcpyAsync(flags, w, 8, hipMemcpyDeviceToHost, s));
    AIX_TRY(hipMemcpyAsync(&total_distinct, dm_off + nbuckets, 4, hipMemcpyDeviceToHost, s));
    AIX_TRY(hipStreamSynchronize(s));
    if (flags[0]) return hipErrorAssert;                        // chunk region exhausted: never silent (the caller reports it)
    if (flags[1]) { *fell_back = true; return hipSuccess; }
    if (total_distinct == 0) return hipSuccess;
    AIX_TRY(keys.alloc(8ull * total_distinct));
    AIX_TRY(counts.alloc(8ull * total_distinct));
    AIX_TRY_LAUNCH(k_k1_gather<uint64_t>, dim3(std::min<uint32_t>((nbuckets + 3) / 4, 1u << 16)), dim3(256), 0, s, (const uint64_t*)keys_st, (const uint32_t*)cnt_st,
                   (const uint32_t*)bucket_base, (const uint32_t*)dm_off, nbuckets, (uint64_t*)keys.p, (uint64_t*)counts.p);
    AIX_TRY(hipStreamSynchronize(s));
    *n_out = total_distinct;
    return hipSuccess;
}

// ---------------------------------------------------------------------------------------------
// The radix-sort back end: sort + run-length of the window codes (k_window_codes: invalid windows = ~0).
// ---------------------------------------------------------------------------------------------
static constexpr int kB = kFlatBlock;

__global__ void __launch_bounds__(kB) k_mark_invalid(uint64_t* __restrict__ codes, uint64_t nwin, uint64_t sentinel) {
    const uint64_t stride = (uint64_t)gridDim.x * kB;
    for (uint64_t i = (uint64_t)blockIdx.x * kB + threadIdx.x; i < nwin; i += stride)
        if (codes[i] == ~0ULL) codes[i] = sentinel;
}
__global__ void __launch_bounds__(kB) k_flag_min(const uint32_t* __restrict__ counts, uint64_t runs, const uint64_t* __restrict__ keys, uint64_t sentinel,
                                                uint32_t min_count, uint8_t* __restrict__ flags) {
    const uint64_t stride = (uint64_t)gridDim.x * kB;
    for (uint64_t i = (uint64_t)blockIdx.x * kB + threadIdx.x; i < runs; i += stride)
        flags[i] = (keys[i] != sentinel && counts[i] >= min_count) ? 1 : 0;
}

hipError_t distinct_from_codes(uint64_t* d_codes, uint64_t nwin, int k, DevArr& keys, DevArr& counts, uint64_t* n_out, hipStream_t s) {
    *n_out = 0;
    if (nwin == 0) return hipSuccess;
    const uint64_t sentinel = 1ULL << (2 * k);                 // k <= 31: one bit above every valid code
    AIX_TRY_LAUNCH(k_mark_invalid, dim3(flat_grid(nwin)), dim3(kB), 0, s, d_codes, nwin, sentinel);
    DevArr sorted(s), tmp(s), ucnt(s), d_runs(s);
    AIX_TRY(sorted.alloc(8 * nwin));
    AIX_TRY(with_temp(tmp, [&](void* t, size_t& tb) { return rocprim::radix_sort_keys(t, tb, d_codes, (uint64_t*)sorted.p, (size_t)nwin, 0u, (unsigned)(2 * k + 1), s); }));
    tmp.drop();
    // run-length encode into the (now free) input buffer as unique keys, plus counts. rocPRIM takes the input size as unsigned int:
    // nwin < 2^32 here (a piece holds at most 2^31 windows)
    uint64_t* ukeys = d_codes;
    AIX_TRY(ucnt.alloc(4 * nwin));
    AIX_TRY(d_runs.alloc(8));
    AIX_TRY(with_temp(tmp, [&](void* t, size_t& tb) {
        return rocprim::run_length_encode(t, tb, (uint64_t*)sorted.p, (unsigned int)nwin, ukeys, (uint32_t*)ucnt.p, (uint64_t*)d_runs.p, s);
    }));
    uint64_t runs = 0, kept = 0;
    AIX_TRY(hipMemcpyAsync(&runs, d_runs.p, 8, hipMemcpyDeviceToHost, s));
    AIX_TRY(hipStreamSynchronize(s));
    tmp.drop();                                                 // the sorted codes and the temporary go back before the filter's blocks are taken
    sorted.drop();
    if (runs == 0) return hipSuccess;
    // filter: drop the sentinel run (every real run counts at least 1)
    DevArr flags(s), d_sel(s), tmp_c(s);
    AIX_TRY(flags.alloc(runs));
    AIX_TRY(keys.alloc(8 * runs));
    AIX_TRY(counts.alloc(4 * runs));
    AIX_TRY(d_sel.alloc(8));
    AIX_TRY_LAUNCH(k_flag_min, dim3(flat_grid(runs)), dim3(kB), 0, s, (uint32_t*)ucnt.p, runs, ukeys, sentinel, 1u, (uint8_t*)flags.p);
    AIX_TRY(with_temp(tmp, [&](void* t, size_t& tb) { return rocprim::select(t, tb, ukeys, (uint8_t*)flags.p, (uint64_t*)keys.p, (uint64_t*)d_sel.p, (size_t)runs, s); }));
    AIX_TRY(with_temp(tmp_c, [&](void* t, size_t& tb) { return rocprim::select(t, tb, (uint32_t*)ucnt.p, (uint8_t*)flags.p, (uint32_t*)counts.p, (uint64_t*)d_sel.p, (size_t)runs, s); }));
    AIX_TRY(hipMemcpyAsync(&kept, d_sel.p, 8, hipMemcpyDeviceToHost, s));
    AIX_TRY(hipStreamSynchronize(s));
    *n_out = kept;
    return hipSuccess;
}


}  // namespace aix
