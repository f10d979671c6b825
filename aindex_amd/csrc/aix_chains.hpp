// aix_chains.hpp — private to the library: what the two compaction levels share. aix_unitigs.hip compacts the stored k-mers of an index
// into unitigs, aix_graphclean.hip compacts the surviving unitigs of a graph into contigs; both link ports, rank them by pointer jumping,
// break what is left (cycles), place, sort and emit. Shared here: the block size, the AIX_UG_TEST_GRID hook and the grid sizer, the
// wave-reduced counters, the {sum, min, max} reduction with its scatter kernel, the counters read-back and the host loop of the ranking.
//
// NOT shared, on purpose: the link, jump, cycle and place kernels. They look alike but carry different state. The unitig level packs a
// 31-bit distance and the terminal flag into ONE u64 per port and keys cycles by the stored code; the contig level needs 64-bit k-mer
// distances in a second array, a window-length array, and end ids as keys. One templated kernel would either widen the unitig level's
// memory traffic or hide two algorithms behind flags. Do not merge them.
#pragma once
#include <algorithm>

#include "aix_env.hpp"
#include "aix_hostkit.hpp"

namespace aix {

static constexpr int kCB = 256;                                   // four waves per workgroup, every kernel of both levels

// AIX_UG_TEST_GRID (test hook, read per call): workgroups of every launch at most, so that small inputs make many trips
static inline uint64_t chain_test_grid() { return env_u64("AIX_UG_TEST_GRID", 1, 65536, 65536); }

static inline unsigned chain_grid(uint64_t work, uint64_t per_block, uint64_t cap) {
    uint64_t b = (work + per_block - 1) / per_block;
    if (b > 4096) b = 4096;                                        // grid-stride: a few atomics per workgroup, not per wave of work
    if (b > cap) b = cap;
    if (b == 0) b = 1;
    return (unsigned)b;
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

// a lane's share of a counter word: one atomic per wave, none when the wave has nothing. Every lane of the wave calls it.
__device__ __forceinline__ void count_add(unsigned long long mine, unsigned long long* dst) {
    const unsigned long long s = wave_sum(mine);
    if ((threadIdx.x & 63u) == 0 && s) atomicAdd(dst, s);
}
__device__ __forceinline__ void count_max(unsigned long long mine, unsigned long long* dst) {
    const unsigned long long m = wave_max(mine);
    if ((threadIdx.x & 63u) == 0 && m) atomicMax(dst, m);
}

// tf_sum / tf_min / tf_max of a unit (unitig, contig) = one reduce-by-key over its members in (unit, position) order
struct ChainAgg {
    unsigned long long sum;
    uint32_t mn, mx;
};
struct ChainAggOp {
    __host__ __device__ ChainAgg operator()(const ChainAgg& a, const ChainAgg& b) const {
        return ChainAgg{a.sum + b.sum, a.mn < b.mn ? a.mn : b.mn, a.mx > b.mx ? a.mx : b.mx};
    }
};
struct ChainUnitOf {                                              // sort key = unit << pos_bits | position
    int pos_bits;
    __host__ __device__ uint64_t operator()(uint64_t key) const { return key >> pos_bits; }
};

// scatters the result of that reduction: unit uniq[i] takes agg[i], for the *count runs found (a template: two translation units include it)
template <class Agg>
__global__ void __launch_bounds__(kCB) k_chain_stats(const uint64_t* __restrict__ uniq, const Agg* __restrict__ agg, const uint64_t* __restrict__ count, uint64_t U,
                                                    uint64_t* __restrict__ tf_sum, uint32_t* __restrict__ tf_min, uint32_t* __restrict__ tf_max) {
    const uint64_t m = *count < U ? *count : U, stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t i = (uint64_t)blockIdx.x * kCB + threadIdx.x; i < m; i += stride) {
        const uint64_t u = uniq[i];
        if (u >= U) continue;
        const Agg a = agg[i];
        tf_sum[u] = a.sum; tf_min[u] = a.mn; tf_max[u] = a.mx;
    }
}

// the counters record of a call, read back. Synchronises `s`.
template <class Counters>
static hipError_t chain_read(Counters* host, const Counters* dev, hipStream_t s) {
    AIX_TRY(hipMemcpyAsync(host, dev, sizeof(Counters), hipMemcpyDeviceToHost, s));
    return hipStreamSynchronize(s);
}

// The host loop of the ranking. step(r) launches round r of the pointer jumping, which counts the ports it leaves unflagged into
// unflagged[r] (device), and swaps its buffers. After round r every port within 2^(r - 1) hops of its end is flagged, so
// min(64, ceil_log2(nodes) + 1) rounds reach every end; the loop stops earlier when nothing is open or a round changed nothing (what is
// left then lies on cycles). *open: the count after the link step on entry, the final count on return. One synchronisation per round.
template <class Step>
static hipError_t chain_rank(uint64_t nodes, const unsigned long long* unflagged, uint64_t* open, hipStream_t s, Step&& step) {
    const int max_rounds = std::min(64, ceil_log2(nodes) + 1);
    for (int r = 1; r <= max_rounds && *open; ++r) {
        AIX_TRY(step(r));
        unsigned long long now = 0;
        AIX_TRY(chain_read(&now, unflagged + r, s));
        const bool same = now == *open;
        *open = now;
        if (same) break;
    }
    return hipSuccess;
}

}  // namespace aix
