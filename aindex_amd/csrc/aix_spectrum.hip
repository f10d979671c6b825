// aix_spectrum.hip — k-mers by frequency over an index resident in HBM: per-kid values, frequency spectrum and statistics, stable top-N /
// threshold selection, and batch kid -> k-mer.
//   AIndex.iter_kmers_by_frequency / get_top_kmers / get_kmer_frequency_stats   aindex/core/aindex.py:594-793   one Python loop over every kid
//   AindexWrapper::get_kmer_by_kid / get_kmer_info                              python_wrapper.cpp:718-755      one kid per call
//   AindexWrapper::get_tf_value_23mer                                           python_wrapper.cpp:610-627      the value of a kid's k-mer
//   AindexWrapper::get_13mer_statistics                                         python_wrapper.cpp:1038-1068
//
// Value of entry i. 23-mer handle: the two-strand probe of checker[i] & (2^46 - 1), forward strand first (the body of k_lookup23_codes) —
// not tf[i]: the two differ where a slot holds a key that is not in its own MPHF slot. 13-mer handle: (uint32_t) tf13[i] in file order.
// Order: descending value, ties in ascending i = ascending by the key ((2^32 - 1 - v) << 32) | i.
//
// The chain (everything streams 4 B per key per pass; nothing sorts n items to return 25):
//   values    k_sp_values23: one lane per kid, key_at() + the wave-cooperative probe; k_sp_narrow: the u32 view of the 13-mer table
//   spectrum  k_sp_hist: one pass; a workgroup keeps bins 0 .. kLdsBins - 1 and the overflow bin in LDS and merges them once, bins between
//             go to memory directly. Real spectra are extremely skewed (most entries are 1 or 2), so lanes of a wave mostly hit the same
//             word: wave_hist_add aggregates equal bins within the wave (leader's bin, ballot, ONE atomic of the population count), at most
//             kAggRounds rounds, then the lanes that are left add on their own (distinct bins by then, or nearly). Statistics ride along
//             in registers and are reduced wave -> workgroup -> memory.
//   select    four passes of k_sp_digits (8-bit digit histograms of the values >= min_v that match the prefix found so far, most
//             significant digit first) with k_sp_pick in between: the value T of the max_items-th entry and r = how many entries equal to
//             T belong to the selection. The state stays on the device; the host reads it once. When everything >= min_v is selected
//             (max_items = 0 or >= total) the later passes return at once (T = min_v, r = all).
//   compact   k_sp_count: per tile of 4096 values the number of v > T and of v == T; two scans; k_sp_emit: every v > T and the first r
//             entries with v == T by kid are written as 64-bit keys (stable: ballot ranks within a wave, wave counts through LDS)
//   sort      rocprim radix sort of the m <= max_items survivors; k_sp_unpack splits the keys into kid and value
//   decode    k_sp_decode: kid -> k ASCII bytes of checker[kid] & mask (13-mer: the base-4 spelling of the index), optionally the reverse
//             complement and tf[kid] read directly (get_kmer_info); kid >= n gives NUL bytes and 0
// All temporaries come from the scratch pool and are sized from n. Every store is bounded by n, nbins or the selection size passed in.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "aix_env.hpp"
#include "aix_hostkit.hpp"
#include "aix_probe.hpp"

namespace aix {

static constexpr int kSB = 256;                                   // four waves per workgroup
static constexpr uint64_t kMask46 = (1ULL << 46) - 1;
static constexpr uint32_t kLdsBins = 2048;                        // spectrum bins a workgroup keeps in LDS (+ 1 word for the overflow bin)
static constexpr int kAggRounds = 4;
static constexpr uint32_t kTile = 16 * kSB;                       // values per workgroup of the compaction

static inline unsigned sp_grid(uint64_t work, uint64_t per_block) {
    uint64_t b = (work + per_block - 1) / per_block;
    if (b > 2048) b = 2048;                                        // grid-stride: one merge of the LDS bins per workgroup
    if (b == 0) b = 1;
    return (unsigned)b;
}

// ---------------------------------------------------------------------------------------------
// values
// ---------------------------------------------------------------------------------------------
// One lane per kid: get_tf_value_23mer (python_wrapper.cpp:610-627) of the slot's code through freq23_wave (aix_probe.hpp). The absence filter
// is not consulted: nearly every probe is a stored key.
template <bool CANON>
__global__ void __launch_bounds__(kSB) k_sp_values23(const IndexDev ix_, uint32_t* __restrict__ out) {
    const IndexDev& ix = ix_;
    const uint64_t n = ix.n, stride = (uint64_t)gridDim.x * kSB;
    for (uint64_t base = (uint64_t)blockIdx.x * kSB + (threadIdx.x & ~63u); base < n; base += stride) {      // wave-uniform
        const uint64_t i = base + (threadIdx.x & 63u);
        const bool in = i < n;
        const uint64_t u = in ? (key_at(ix, i).code & kMask46) : 0ull;
        bool found;
        const uint32_t tf = freq23_wave<CANON>(ix, in, u, false, found);
        if (in) out[i] = tf;
    }
}

// the u32 view of a u64 table (get_13mer_tf_array, python_wrapper.cpp:983-991)
__global__ void __launch_bounds__(kSB) k_sp_narrow(const uint64_t* __restrict__ in, uint64_t n, uint32_t* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * kSB;
    for (uint64_t i = (uint64_t)blockIdx.x * kSB + threadIdx.x; i < n; i += stride) out[i] = (uint32_t)in[i];
}

// ---------------------------------------------------------------------------------------------
// histograms in LDS
// ---------------------------------------------------------------------------------------------
// hist[bin] += 1 for every lane with `on`; every lane of the wave calls it. Equal bins of a wave become one atomic.
__device__ __forceinline__ void wave_hist_add(uint32_t* hist, bool on, uint32_t bin) {
    const uint32_t lane = threadIdx.x & 63u;
    bool mine = on;
#pragma unroll 1
    for (int round = 0; round < kAggRounds; ++round) {
        const uint64_t todo = __ballot(mine);
        if (todo == 0) return;                                    // wave-uniform
        const uint32_t lead = (uint32_t)__ffsll((long long)todo) - 1u;
        const uint32_t lb = (uint32_t)__shfl((int)bin, (int)lead);
        const bool same = mine && bin == lb;
        const uint64_t grp = __ballot(same);
        if (lane == lead) atomicAdd(&hist[lb], (uint32_t)__popcll(grp));
        if (same) mine = false;
    }
    if (mine) atomicAdd(&hist[bin], 1u);
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int s = 32; s; s >>= 1) v += __shfl_xor(v, s);
    return v;
}
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
#pragma unroll
    for (int s = 32; s; s >>= 1) { const unsigned long long o = __shfl_xor(v, s); v = o > v ? o : v; }
    return v;
}

// stats words: n, non-zero, max, min non-zero, sum (of the u32 view), then non-zero, max, sum of the entries at full width
// (get_13mer_statistics, python_wrapper.cpp:1038-1068, reads the u64 table). While the pass runs, word 3 holds max(2^32 - 1 - v) over v != 0.
template <typename T>
__global__ void __launch_bounds__(kSB) k_sp_hist(const T* __restrict__ vals, uint64_t n, uint64_t nbins, unsigned long long* __restrict__ hist,
                                                unsigned long long* __restrict__ stats) {
    __shared__ uint32_t lds[kLdsBins + 1];
    __shared__ unsigned long long red[kSB / 64][7];
    const uint32_t top = nbins - 1 < 0xFFFFFFFFull ? (uint32_t)(nbins - 1) : 0xFFFFFFFFu;       // the overflow bin: v >= top
    const uint32_t nl = top < kLdsBins ? top : kLdsBins;                                 // bins 0 .. nl - 1 in LDS, the overflow bin in lds[nl]
    for (uint32_t j = threadIdx.x; j <= nl; j += kSB) lds[j] = 0;
    __syncthreads();
    unsigned long long nz = 0, mx = 0, inv = 0, sum = 0, nzw = 0, mxw = 0, sumw = 0;
    const uint64_t stride = (uint64_t)gridDim.x * kSB;
    for (uint64_t base = (uint64_t)blockIdx.x * kSB + (threadIdx.x & ~63u); base < n; base += stride) {      // wave-uniform
        const uint64_t i = base + (threadIdx.x & 63u);
        const bool in = i < n;
        const T x = in ? vals[i] : (T)0;
        const uint32_t v = (uint32_t)x;
        if (v) { ++nz; mx = v > mx ? v : mx; const uint64_t q = 0xFFFFFFFFull - v; inv = q > inv ? q : inv; sum += v; }
        if (sizeof(T) == 8 && x) { ++nzw; mxw = (uint64_t)x > mxw ? (uint64_t)x : mxw; sumw += (uint64_t)x; }
        const bool over = v >= top;
        const bool local = over || v < nl;
        wave_hist_add(lds, in && local, over ? nl : v);
        if (in && !local) atomicAdd(&hist[v], 1ull);              // kLdsBins <= v < nbins - 1: the sparse tail of a spectrum
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j <= nl; j += kSB) {
        const uint32_t c = lds[j];
        if (c) atomicAdd(&hist[j == nl ? top : j], (unsigned long long)c);
    }
    nz = wave_sum(nz); sum = wave_sum(sum); mx = wave_max(mx); inv = wave_max(inv);
    nzw = wave_sum(nzw); sumw = wave_sum(sumw); mxw = wave_max(mxw);
    const uint32_t w = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0) { red[w][0] = nz; red[w][1] = mx; red[w][2] = inv; red[w][3] = sum; red[w][4] = nzw; red[w][5] = mxw; red[w][6] = sumw; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kSB / 64; ++k) {
            red[0][0] += red[k][0]; red[0][3] += red[k][3]; red[0][4] += red[k][4]; red[0][6] += red[k][6];
            for (int c : {1, 2, 5}) red[0][c] = red[k][c] > red[0][c] ? red[k][c] : red[0][c];
        }
        if (red[0][0]) {
            atomicAdd(&stats[1], red[0][0]); atomicMax(&stats[2], red[0][1]); atomicMax(&stats[3], red[0][2]); atomicAdd(&stats[4], red[0][3]);
        }
        if (sizeof(T) == 8 && red[0][4]) { atomicAdd(&stats[5], red[0][4]); atomicMax(&stats[6], red[0][5]); atomicAdd(&stats[7], red[0][6]); }
    }
}

__global__ void k_sp_stats_finish(unsigned long long* __restrict__ stats, uint64_t n, int wide) {
    if (threadIdx.x || blockIdx.x) return;
    stats[0] = n;
    stats[3] = stats[1] ? 0xFFFFFFFFull - stats[3] : 0ull;
    if (!wide) { stats[5] = stats[1]; stats[6] = stats[2]; stats[7] = stats[4]; }
}

// ---------------------------------------------------------------------------------------------
// radix select
// ---------------------------------------------------------------------------------------------
struct SelState {
    uint32_t prefix;     // the digits of T found so far
    uint32_t k;          // rank (1-based, from the top) still to be resolved inside the prefix class
    uint32_t total;      // entries with v >= min_v
    uint32_t m;          // entries selected
    uint32_t T, r;       // selected: every v > T, and the first r entries with v == T by index
    uint32_t all;        // everything >= min_v is selected: T = min_v, r = 2^32 - 1
    uint32_t pad;
};

__global__ void __launch_bounds__(kSB) k_sp_digits(const uint32_t* __restrict__ vals, uint64_t n, uint32_t min_v, int pass, const SelState* __restrict__ st,
                                                  uint32_t* __restrict__ ghist) {
    __shared__ uint32_t lds[256];
    uint32_t prefix = 0, himask = 0;
    if (pass) {
        if (st->all) return;                                      // uniform over the grid
        prefix = st->prefix;
        himask = 0xFFFFFFFFu << (32 - 8 * pass);
    }
    const int shift = 24 - 8 * pass;
    lds[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * kSB;
    for (uint64_t base = (uint64_t)blockIdx.x * kSB + (threadIdx.x & ~63u); base < n; base += stride) {      // wave-uniform
        const uint64_t i = base + (threadIdx.x & 63u);
        const bool in = i < n;
        const uint32_t v = in ? vals[i] : 0u;
        wave_hist_add(lds, in && v >= min_v && (v & himask) == prefix, (v >> shift) & 255u);
    }
    __syncthreads();
    const uint32_t c = lds[threadIdx.x];
    if (c) atomicAdd(&ghist[threadIdx.x], c);
}

// one thread: the digit of this pass from the 256 counts (descending), then the counts are cleared for the next pass
__global__ void k_sp_pick(int pass, uint64_t max_items, uint32_t min_v, SelState* __restrict__ st, uint32_t* __restrict__ ghist) {
    if (threadIdx.x || blockIdx.x) return;
    if (pass == 0) {
        uint64_t total = 0;
        for (int d = 0; d < 256; ++d) total += ghist[d];
        const uint64_t m = (max_items && max_items < total) ? max_items : total;
        st->total = (uint32_t)total;
        st->m = (uint32_t)m;
        st->prefix = 0;
        st->k = (uint32_t)m;
        st->all = m == total ? 1u : 0u;
        st->T = min_v;
        st->r = 0xFFFFFFFFu;
    }
    if (!st->all) {
        const int shift = 24 - 8 * pass;
        uint32_t k = st->k, cum = 0, digit = 0;
        for (int d = 255; d >= 0; --d) {
            const uint32_t c = ghist[d];
            if (cum + c >= k) { digit = (uint32_t)d; break; }     // 1 <= k <= the population of the prefix class: always reached
            cum += c;
        }
        st->k = k - cum;
        st->prefix |= digit << shift;
        if (pass == 3) { st->T = st->prefix; st->r = st->k; }
    }
    for (int d = 0; d < 256; ++d) ghist[d] = 0;
}

// ---------------------------------------------------------------------------------------------
// stable compaction
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSB) k_sp_count(const uint32_t* __restrict__ vals, uint64_t n, const SelState* __restrict__ st, uint32_t nblk,
                                                 uint32_t* __restrict__ cgt, uint32_t* __restrict__ ceq) {
    __shared__ uint32_t red[kSB / 64][2];
    const uint32_t T = st->T;
    const uint64_t tile = (uint64_t)blockIdx.x * kTile;
    uint32_t g = 0, e = 0;
#pragma unroll 4
    for (uint32_t j = 0; j < kTile / kSB; ++j) {
        const uint64_t i = tile + j * kSB + threadIdx.x;
        if (i < n) { const uint32_t v = vals[i]; g += v > T; e += v == T; }
    }
    const unsigned long long ge = wave_sum(((unsigned long long)g << 32) | e);
    if ((threadIdx.x & 63u) == 0) { red[threadIdx.x >> 6][0] = (uint32_t)(ge >> 32); red[threadIdx.x >> 6][1] = (uint32_t)ge; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sg = 0, se = 0;
        for (int k = 0; k < kSB / 64; ++k) { sg += red[k][0]; se += red[k][1]; }
        cgt[blockIdx.x] = sg;
        ceq[blockIdx.x] = se;
        if (blockIdx.x == 0) { cgt[nblk] = 0; ceq[nblk] = 0; }    // the scans run over nblk + 1 entries: entry nblk becomes the total
    }
}

__global__ void __launch_bounds__(kSB) k_sp_emit(const uint32_t* __restrict__ vals, uint64_t n, const SelState* __restrict__ st, uint32_t nblk,
                                                const uint32_t* __restrict__ ogt, const uint32_t* __restrict__ oeq, uint64_t m,
                                                unsigned long long* __restrict__ keys) {
    __shared__ uint32_t wc[2][kSB / 64][2];
    const uint32_t T = st->T, r = st->r;
    const uint64_t total_gt = ogt[nblk];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint64_t below = (1ull << lane) - 1ull;
    const uint64_t tile = (uint64_t)blockIdx.x * kTile;
    uint64_t run_g = ogt[blockIdx.x], run_e = oeq[blockIdx.x];
    for (uint32_t j = 0; j < kTile / kSB; ++j) {
        if (tile + (uint64_t)j * kSB >= n) break;                 // uniform over the workgroup
        const uint64_t i = tile + j * kSB + threadIdx.x;
        const uint32_t v = i < n ? vals[i] : 0u;
        const bool g = i < n && v > T, e = i < n && v == T;
        const uint64_t bg = __ballot(g), be = __ballot(e);
        if (lane == 0) { wc[j & 1][w][0] = (uint32_t)__popcll(bg); wc[j & 1][w][1] = (uint32_t)__popcll(be); }
        __syncthreads();
        uint32_t pg = 0, pe = 0, tg = 0, te = 0;
        for (uint32_t k = 0; k < kSB / 64; ++k) {
            const uint32_t a = wc[j & 1][k][0], b = wc[j & 1][k][1];
            if (k < w) { pg += a; pe += b; }
            tg += a; te += b;
        }
        const unsigned long long key = ((unsigned long long)(0xFFFFFFFFu - v) << 32) | (unsigned long long)(uint32_t)i;
        if (g) {
            const uint64_t dst = run_g + pg + (uint64_t)__popcll(bg & below);
            if (dst < m) keys[dst] = key;
        }
        if (e) {
            const uint64_t rank = run_e + pe + (uint64_t)__popcll(be & below);
            if (rank < r && total_gt + rank < m) keys[total_gt + rank] = key;
        }
        run_g += tg;
        run_e += te;
    }
}

__global__ void __launch_bounds__(kSB) k_sp_unpack(const unsigned long long* __restrict__ keys, uint64_t m, uint32_t* __restrict__ idx, uint32_t* __restrict__ val) {
    const uint64_t stride = (uint64_t)gridDim.x * kSB;
    for (uint64_t j = (uint64_t)blockIdx.x * kSB + threadIdx.x; j < m; j += stride) {
        const unsigned long long k = keys[j];
        idx[j] = (uint32_t)k;
        if (val) val[j] = 0xFFFFFFFFu - (uint32_t)(k >> 32);
    }
}

// ---------------------------------------------------------------------------------------------
// decode
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSB) k_sp_decode(const IndexDev ix_, const uint64_t* __restrict__ kid64, const uint32_t* __restrict__ kid32, uint64_t N,
                                                  uint8_t* __restrict__ out, uint8_t* __restrict__ rc_out, uint32_t* __restrict__ tf_out) {
    const IndexDev& ix = ix_;
    const uint32_t k = ix.k;
    const uint64_t stride = (uint64_t)gridDim.x * kSB;
    for (uint64_t j = (uint64_t)blockIdx.x * kSB + threadIdx.x; j < N; j += stride) {
        const uint64_t kid = kid64 ? kid64[j] : (uint64_t)kid32[j];
        const bool ok = kid < ix.n;
        uint64_t f[3] = {0, 0, 0}, b[3] = {0, 0, 0};
        uint32_t tf = 0;
        if (ok && k == 23) {
            const KeyRec rec = key_at(ix, kid);                   // get_kmer_info (python_wrapper.cpp:744-755): tf[kid] itself, not the probe
            const uint64_t u = rec.code & kMask46;
            tf = rec.tf;
            ascii23_of_rc(revcomp(u, 23), f[0], f[1], f[2]);
            ascii23_of_rc(u, b[0], b[1], b[2]);
        } else if (ok) {
            const uint32_t u = (uint32_t)kid;                     // the base-4 spelling of the index (aindex.py:574-592)
            tf = (uint32_t)ix.tf13_mphf[kid];
            ascii13_of_rc((uint32_t)revcomp(u, 13), f[0], f[1]);
            ascii13_of_rc(u, b[0], b[1]);
        }
        for (uint32_t c = 0; c < k; ++c) {
            out[j * k + c] = (uint8_t)(f[c >> 3] >> (8 * (c & 7)));
            if (rc_out) rc_out[j * k + c] = (uint8_t)(b[c >> 3] >> (8 * (c & 7)));
        }
        if (tf_out) tf_out[j] = tf;
    }
}

// ---------------------------------------------------------------------------------------------
// host side of the chain
// ---------------------------------------------------------------------------------------------
static hipError_t sp_values(const aix_index* h, uint32_t* d_out, hipStream_t s) {
    if (h->n == 0) return hipSuccess;
    const IndexDev ix = h->dev();
    if (h->k == 13) hipLaunchKernelGGL(k_sp_narrow, dim3(sp_grid(h->n, 4 * kSB)), dim3(kSB), 0, s, h->tf13_mphf.as<uint64_t>(), h->n, d_out);
    else if (ix.canonical_only) hipLaunchKernelGGL(k_sp_values23<true>, dim3(sp_grid(h->n, kSB) * 8), dim3(kSB), 0, s, ix, d_out);
    else hipLaunchKernelGGL(k_sp_values23<false>, dim3(sp_grid(h->n, kSB) * 8), dim3(kSB), 0, s, ix, d_out);
    return hipGetLastError();
}

template <typename T>
static hipError_t sp_spectrum(const T* d_vals, uint64_t n, uint64_t nbins, uint64_t* d_hist, uint64_t* d_stats, hipStream_t s) {
    hipError_t e = hipMemsetAsync(d_hist, 0, 8 * nbins, s);
    if (e == hipSuccess) e = hipMemsetAsync(d_stats, 0, 8 * AIX_SPECTRUM_STATS, s);
    if (e != hipSuccess) return e;
    if (n) {
        hipLaunchKernelGGL(k_sp_hist<T>, dim3(sp_grid(n, 8 * kSB)), dim3(kSB), 0, s, d_vals, n, nbins, (unsigned long long*)d_hist, (unsigned long long*)d_stats);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_sp_stats_finish, dim3(1), dim3(64), 0, s, (unsigned long long*)d_stats, n, sizeof(T) == 8 ? 1 : 0);
    return hipGetLastError();
}

static hipError_t sp_scan(const uint32_t* in, uint32_t* out, uint64_t n, DevArr& tmp, hipStream_t s) {
    return with_temp(tmp, [&](void* t, size_t& tb) { return rocprim::exclusive_scan(t, tb, in, out, 0u, (size_t)n, rocprim::plus<uint32_t>(), s); });
}

// Selection over d_vals[n], n < 2^32. *m_out / *total_out are always produced; the entries only when they fit `cap` (d_idx / d_val), or
// always into own_idx / own_val when those are given (blocks of exactly m entries). Synchronises `s`.
static hipError_t sp_select(const uint32_t* d_vals, uint64_t n, uint32_t min_v, uint64_t max_items, uint32_t* d_idx, uint32_t* d_val, uint64_t cap,
                            DevArr* own_idx, DevArr* own_val, uint64_t* m_out, uint64_t* total_out, hipStream_t s) {
    *m_out = *total_out = 0;
    if (n == 0) return hipSuccess;
    const uint32_t nblk = (uint32_t)((n + kTile - 1) / kTile);
    DevArr st(s), gh(s), cnt(s), off(s), t0(s), t1(s), keys(s), sorted(s), t2(s);
    hipError_t e = st.alloc(sizeof(SelState));
    if (e == hipSuccess) e = gh.alloc(4 * 256);
    if (e == hipSuccess) e = cnt.alloc(8ull * (nblk + 1));
    if (e == hipSuccess) e = off.alloc(8ull * (nblk + 1));
    if (e == hipSuccess) e = hipMemsetAsync(gh.p, 0, 4 * 256, s);
    if (e == hipSuccess) e = hipMemsetAsync(st.p, 0, sizeof(SelState), s);
    if (e != hipSuccess) return e;
    SelState* d_st = (SelState*)st.p;
    for (int pass = 0; pass < 4; ++pass) {
        hipLaunchKernelGGL(k_sp_digits, dim3(sp_grid(n, 8 * kSB)), dim3(kSB), 0, s, d_vals, n, min_v, pass, (const SelState*)d_st, (uint32_t*)gh.p);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(k_sp_pick, dim3(1), dim3(64), 0, s, pass, max_items, min_v, d_st, (uint32_t*)gh.p);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    SelState hs;
    e = hipMemcpyAsync(&hs, d_st, sizeof(SelState), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return e;
    const uint64_t m = std::min<uint64_t>(hs.m, n);               // m <= total <= n by construction; nothing below is sized beyond n
    *m_out = m;
    *total_out = hs.total;
    if (m == 0) return hipSuccess;
    if (own_idx) {
        if ((e = own_idx->alloc(4 * m)) != hipSuccess) return e;
        if ((e = own_val->alloc(4 * m)) != hipSuccess) return e;
        d_idx = (uint32_t*)own_idx->p; d_val = (uint32_t*)own_val->p; cap = m;
    }
    if (m > cap || !d_idx) return hipSuccess;
    uint32_t *cgt = (uint32_t*)cnt.p, *ceq = cgt + (nblk + 1), *ogt = (uint32_t*)off.p, *oeq = ogt + (nblk + 1);
    if ((e = keys.alloc(8 * m)) != hipSuccess) return e;
    if ((e = sorted.alloc(8 * m)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_sp_count, dim3(nblk), dim3(kSB), 0, s, d_vals, n, (const SelState*)d_st, nblk, cgt, ceq);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = sp_scan(cgt, ogt, (uint64_t)nblk + 1, t0, s)) != hipSuccess) return e;
    if ((e = sp_scan(ceq, oeq, (uint64_t)nblk + 1, t1, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_sp_emit, dim3(nblk), dim3(kSB), 0, s, d_vals, n, (const SelState*)d_st, nblk, (const uint32_t*)ogt, (const uint32_t*)oeq, m,
                       (unsigned long long*)keys.p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    e = with_temp(t2, [&](void* t, size_t& tb) {
        return rocprim::radix_sort_keys(t, tb, (const unsigned long long*)keys.p, (unsigned long long*)sorted.p, (size_t)m, 0u, 64u, s);
    });
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_sp_unpack, dim3(sp_grid(m, 4 * kSB)), dim3(kSB), 0, s, (const unsigned long long*)sorted.p, m, d_idx, d_val);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return hipStreamSynchronize(s);                               // the scratch blocks go back to the pool idle
}

static hipError_t sp_decode(const aix_index* h, const uint64_t* kid64, const uint32_t* kid32, uint64_t N, char* out, char* rc, uint32_t* tf, hipStream_t s) {
    if (N == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sp_decode, dim3(sp_grid(N, kSB) * 8), dim3(kSB), 0, s, h->dev(), kid64, kid32, N, (uint8_t*)out, (uint8_t*)rc, tf);
    return hipGetLastError();
}

}  // namespace aix

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
static constexpr uint64_t kMaxBins = 1ull << 32;                  // a u32 value has no bin beyond 2^32 - 1; more cannot be held by any caller we serve

// ---- array level ----------------------------------------------------------------------------------
extern "C" int aix_values_narrow_dev(const uint64_t* d_in, uint64_t n, uint32_t* d_out, void* stream) {
    if (n && (!d_in || !d_out)) return AIX_ERR_ARG;
    if (n == 0) return AIX_OK;
    hipLaunchKernelGGL(k_sp_narrow, dim3(sp_grid(n, 4 * kSB)), dim3(kSB), 0, (hipStream_t)stream, d_in, n, d_out);
    AIXCHK(hipGetLastError());
    return AIX_OK;
}

extern "C" int aix_spectrum_dev(const void* d_values, int elem_bytes, uint64_t n, uint64_t nbins, uint64_t* d_hist, uint64_t* d_stats, void* stream) {
    if (nbins < 2 || !d_hist || !d_stats || (n && !d_values) || (elem_bytes != 4 && elem_bytes != 8)) return AIX_ERR_ARG;
    if (nbins > kMaxBins || n >= (1ull << 60)) return AIX_ERR_NOMEM;
    if (elem_bytes == 8) AIXCHK(sp_spectrum((const uint64_t*)d_values, n, nbins, d_hist, d_stats, (hipStream_t)stream));
    else AIXCHK(sp_spectrum((const uint32_t*)d_values, n, nbins, d_hist, d_stats, (hipStream_t)stream));
    return AIX_OK;
}

extern "C" int aix_select_dev(const uint32_t* d_values, uint64_t n, uint32_t min_v, uint64_t max_items, uint32_t* d_idx, uint32_t* d_val, uint64_t cap,
                              uint64_t* n_out, uint64_t* total_out, void* stream) {
    if (!n_out || !total_out || (n && !d_values)) return AIX_ERR_ARG;
    if (n >= (1ull << 32)) return AIX_ERR_ARG;                    // an index is 32 bits wide
    AIXCHK(sp_select(d_values, n, min_v, max_items, cap ? d_idx : nullptr, d_val, cap, nullptr, nullptr, n_out, total_out, (hipStream_t)stream));
    return AIX_OK;
}

// ---- handle level ---------------------------------------------------------------------------------
extern "C" int aix_kmer_values_dev(aix_index_t* h, uint32_t* d_out, void* stream) {
    if (!h || (h->n && !d_out)) return AIX_ERR_ARG;
    if (h->n >= (1ull << 32)) return AIX_ERR_UNSUPPORTED;
    DevGuard g(h->device);
    AIXCHK(sp_values(h, d_out, (hipStream_t)stream));
    return AIX_OK;
}

extern "C" int aix_tf_spectrum_dev(aix_index_t* h, uint64_t nbins, uint64_t* d_hist, uint64_t* d_stats, void* stream) {
    if (!h || nbins < 2 || !d_hist || !d_stats) return AIX_ERR_ARG;
    if (nbins > kMaxBins) return AIX_ERR_NOMEM;
    if (h->n >= (1ull << 32)) return AIX_ERR_UNSUPPORTED;
    DevGuard g(h->device);
    hipStream_t s = (hipStream_t)stream;
    if (h->k == 13) {                                             // the table itself: the u32 view and the full-width statistics in one pass
        AIXCHK(sp_spectrum(h->tf13_mphf.as<const uint64_t>(), h->n, nbins, d_hist, d_stats, s));
        return AIX_OK;
    }
    DevArr vals(s);
    AIXCHK(vals.alloc(4 * h->n));
    AIXCHK(sp_values(h, (uint32_t*)vals.p, s));
    AIXCHK(sp_spectrum((const uint32_t*)vals.p, h->n, nbins, d_hist, d_stats, s));
    return AIX_OK;
}

extern "C" int aix_tf_spectrum(aix_index_t* h, uint64_t nbins, uint64_t* hist_out, uint64_t* stats_out) {
    if (!h || nbins < 2 || !hist_out || !stats_out) return AIX_ERR_ARG;
    if (nbins > kMaxBins) return AIX_ERR_NOMEM;
    DevGuard g(h->device);
    DevBuf dh, ds;
    AIXCHK(dh.alloc(8 * nbins));
    AIXCHK(ds.alloc(8 * AIX_SPECTRUM_STATS));
    const int st = aix_tf_spectrum_dev(h, nbins, (uint64_t*)dh.p, (uint64_t*)ds.p, nullptr);
    if (st) return st;
    AIXCHK(hipMemcpy(hist_out, dh.p, 8 * nbins, hipMemcpyDeviceToHost));
    AIXCHK(hipMemcpy(stats_out, ds.p, 8 * AIX_SPECTRUM_STATS, hipMemcpyDeviceToHost));
    return AIX_OK;
}

extern "C" int aix_top_kmers_dev(aix_index_t* h, uint32_t min_tf, uint64_t max_kmers, uint32_t* d_kid, uint32_t* d_tf, char* d_kmers, uint64_t cap,
                                 uint64_t* n_out, uint64_t* total_out, void* stream) {
    if (!h || !n_out || !total_out) return AIX_ERR_ARG;
    if (h->n >= (1ull << 32)) return AIX_ERR_UNSUPPORTED;
    DevGuard g(h->device);
    hipStream_t s = (hipStream_t)stream;
    DevArr vals(s);
    AIXCHK(vals.alloc(4 * h->n));
    AIXCHK(sp_values(h, (uint32_t*)vals.p, s));
    AIXCHK(sp_select((const uint32_t*)vals.p, h->n, min_tf, max_kmers, cap ? d_kid : nullptr, d_tf, cap, nullptr, nullptr, n_out, total_out, s));
    if (*n_out && *n_out <= cap && d_kid && d_kmers) {
        AIXCHK(sp_decode(h, nullptr, d_kid, *n_out, d_kmers, nullptr, nullptr, s));
        AIXCHK(hipStreamSynchronize(s));                           // as the selection: every output is complete on return
    }
    return AIX_OK;
}

extern "C" int aix_top_kmers(aix_index_t* h, uint32_t min_tf, uint64_t max_kmers, uint32_t** kid_out, uint32_t** tf_out, char** kmers_out, uint64_t* n_out,
                             uint64_t* total_out) {
    if (!h || !kid_out || !tf_out || !n_out || !total_out) return AIX_ERR_ARG;
    *kid_out = *tf_out = nullptr;
    if (kmers_out) *kmers_out = nullptr;
    *n_out = *total_out = 0;
    if (h->n >= (1ull << 32)) return AIX_ERR_UNSUPPORTED;
    DevGuard g(h->device);
    DevArr vals, idx, val, km;
    AIXCHK(vals.alloc(4 * h->n));
    AIXCHK(sp_values(h, (uint32_t*)vals.p, nullptr));
    uint64_t m = 0, total = 0;
    AIXCHK(sp_select((const uint32_t*)vals.p, h->n, min_tf, max_kmers, nullptr, nullptr, 0, &idx, &val, &m, &total, nullptr));
    if (m && kmers_out) {
        AIXCHK(km.alloc(m * h->k));
        AIXCHK(sp_decode(h, nullptr, (const uint32_t*)idx.p, m, (char*)km.p, nullptr, nullptr, nullptr));
    }
    uint32_t* hk = (uint32_t*)malloc(m ? 4 * m : 4);
    uint32_t* ht = (uint32_t*)malloc(m ? 4 * m : 4);
    char* hs = kmers_out ? (char*)malloc(m ? m * h->k : 1) : nullptr;
    hipError_t e = (hk && ht && (!kmers_out || hs)) ? hipSuccess : hipErrorOutOfMemory;
    if (e == hipSuccess && m) e = hipMemcpy(hk, idx.p, 4 * m, hipMemcpyDeviceToHost);
    if (e == hipSuccess && m) e = hipMemcpy(ht, val.p, 4 * m, hipMemcpyDeviceToHost);
    if (e == hipSuccess && m && kmers_out) e = hipMemcpy(hs, km.p, m * h->k, hipMemcpyDeviceToHost);
    if (e != hipSuccess) { free(hk); free(ht); free(hs); AIXCHK(e); }
    *kid_out = hk; *tf_out = ht;
    if (kmers_out) *kmers_out = hs;
    *n_out = m; *total_out = total;
    return AIX_OK;
}

extern "C" int aix_kmers_by_kid_dev(aix_index_t* h, const uint64_t* d_kid, uint64_t N, char* d_kmers, char* d_rc, uint32_t* d_tf, void* stream) {
    if (!h || (N && (!d_kid || !d_kmers))) return AIX_ERR_ARG;
    if (N >= (1ull << 56)) return AIX_ERR_NOMEM;
    if (N == 0) return AIX_OK;
    DevGuard g(h->device);
    AIXCHK(sp_decode(h, d_kid, nullptr, N, d_kmers, d_rc, d_tf, (hipStream_t)stream));
    return AIX_OK;
}

extern "C" int aix_kmers_by_kid(aix_index_t* h, const uint64_t* kid, uint64_t N, char* kmers_out, char* rc_out, uint32_t* tf_out) {
    if (!h || (N && (!kid || !kmers_out))) return AIX_ERR_ARG;
    if (N >= (1ull << 56)) return AIX_ERR_NOMEM;
    if (N == 0) return AIX_OK;
    DevGuard g(h->device);
    const uint64_t bytes = N * h->k;
    DevBuf dk, dm, dr, dt;
    AIXCHK(dk.alloc(8 * N));
    AIXCHK(dm.alloc(bytes));
    if (rc_out) AIXCHK(dr.alloc(bytes));
    if (tf_out) AIXCHK(dt.alloc(4 * N));
    AIXCHK(hipMemcpy(dk.p, kid, 8 * N, hipMemcpyHostToDevice));
    const int st = aix_kmers_by_kid_dev(h, (const uint64_t*)dk.p, N, (char*)dm.p, (char*)dr.p, (uint32_t*)dt.p, nullptr);
    if (st) return st;
    AIXCHK(hipMemcpy(kmers_out, dm.p, bytes, hipMemcpyDeviceToHost));
    if (rc_out) AIXCHK(hipMemcpy(rc_out, dr.p, bytes, hipMemcpyDeviceToHost));
    if (tf_out) AIXCHK(hipMemcpy(tf_out, dt.p, 4 * N, hipMemcpyDeviceToHost));
    return AIX_OK;
}
