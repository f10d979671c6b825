// aix_graph.hpp — private to the library: what the graph files share. The graph layer is everything that works on arrays over the 2 U
// ends of unitigs or contigs: the links half of aix_unitigs.hip, aix_graphclean.hip, aix_seqthread.hip, aix_graphresolve.hip,
// aix_scaffold.hip and aix_gapclose.hip, and aix_pileup.hip on the contigs themselves. Shared here, and only what at least two of them
// use: the two constants, the counters holder of a call, the predicates the validate kernels repeat, a handful of device helpers, and
// the kernel that writes the bases of scaffolds.
//
// THE RULE OF A VALIDATE KERNEL: it runs on arrays that may hold anything, so a value is compared with its bound before it is used as an
// index, and the predicates below read nothing themselves: they take the loaded words. (join_dual_ok is the one that gathers, and it
// tests the word it gathers through first.) The `bad` counters are only ever tested for non-zero; how many a violation counts is free.
//
// NOT shared, on purpose:
//   - the validate kernels as wholes. They differ in what they walk (node words, steps, members, paths); k_gr_validate needs the index of
//     the FIRST dual of a link (support and link_remove are compared there), k_gc_validate skips the links of removed unitigs. Only their
//     predicates are here.
//   - k_gp_search: one wave per join with its states in LDS; nothing else in the layer has that shape.
//   - the ranking and cycle kernels of the scaffold layout: the note in aix_chains.hpp covers them (a third state layout: next end, 64-bit
//     distance in bases and a hop count).
#pragma once
#include "aix_chains.hpp"

namespace aix {

static constexpr uint64_t kUnitLimit = 0x7FFFFFFFull - 4;         // the limit of the graph calls: an end (2 u + side) must fit a 32-bit word
static constexpr uint32_t kNoEnd = 0xFFFFFFFFu;                   // a 32-bit word that names no end, unit or contig (AIX_BUBBLE_NONE)
static constexpr uint64_t kNoLink = ~0ULL;                        // link_find: no such link
static constexpr uint64_t kAnyDegree = ~0ULL;                     // csr_in_range / csr_bad: no cap on the entries of one end

// The counters record of a call: the device block and its host copy. run(launch) zeroes the record, runs the launches, reads it back
// into `host` and synchronises the stream, once. (In an unnamed namespace: internal linkage, like the static functions of the private
// headers, so that the library exports no symbol for it.)
namespace {
template <class Counters>
struct Counted {
    DevArr arr;
    Counters host;
    explicit Counted(hipStream_t s) : arr(s) {}
    hipError_t init() { return arr.alloc(sizeof(Counters)); }
    Counters* dev() const { return (Counters*)arr.p; }
    template <class Launch>
    hipError_t run(Launch&& launch) {
        AIX_TRY(hipMemsetAsync(arr.p, 0, sizeof(Counters), arr.st));
        AIX_TRY(launch());
        return chain_read(&host, dev(), arr.st);
    }
};
}  // namespace

// ---------------------------------------------------------------------------------------------
// predicates of the validate kernels
// ---------------------------------------------------------------------------------------------
// offsets[u] = a, offsets[u + 1] = b: a unit holds a k-mer, so offsets ascend by at least 23
__device__ __forceinline__ bool span_bad(uint64_t a, uint64_t b) { return b < a || b - a < 23; }

// [lo, hi) = off[e], off[e + 1] of a CSR with `total` entries lies inside it and holds at most max_degree entries (4 in the unitig graph,
// kAnyDegree in the contig and scaffold graphs). The guard in front of every walk over the entries of e.
__device__ __forceinline__ bool csr_in_range(uint64_t lo, uint64_t hi, uint64_t total, uint64_t max_degree) {
    return hi >= lo && hi <= total && hi - lo <= max_degree;
}
// the violations entry e of n sees of "the CSR starts at 0, ascends and ends at `total`"
__device__ __forceinline__ unsigned csr_bad(uint64_t e, uint64_t n, uint64_t lo, uint64_t hi, uint64_t total, uint64_t max_degree) {
    return (unsigned)(e == 0 && lo != 0) + (unsigned)(e == n - 1 && hi != total) + (unsigned)!csr_in_range(lo, hi, total, max_degree);
}

// t = join[e] is a join: it names an end of another contig whose dual join names e back, with an equal gap
__device__ __forceinline__ bool join_dual_ok(const uint32_t* __restrict__ join, const long long* __restrict__ join_gap, uint64_t NE, uint64_t e, uint64_t t) {
    return t < NE && (t >> 1) != (e >> 1) && (uint64_t)join[t ^ 1] == (e ^ 1) && join_gap[t ^ 1] == join_gap[e];
}

// ---------------------------------------------------------------------------------------------
// device helpers (behind a validation: indices are in range)
// ---------------------------------------------------------------------------------------------
// the bases of the unit behind end word w
__device__ __forceinline__ uint64_t unit_len(const uint64_t* __restrict__ offsets, uint64_t w) { return offsets[(w >> 1) + 1] - offsets[w >> 1]; }

// index of the first entry of link_to[lo, hi) that is t; `none` without one
__device__ __forceinline__ uint64_t link_find(const uint32_t* __restrict__ link_to, uint64_t lo, uint64_t hi, uint64_t t, uint64_t none = kNoLink) {
    for (uint64_t j = lo; j < hi; ++j)
        if ((uint64_t)link_to[j] == t) return j;
    return none;
}

// the last j in [lo, hi) with a[j] <= key, for a[lo] <= key: a bisection that ends whatever the array holds (at most 64 trips)
__device__ __forceinline__ uint64_t last_le(const uint64_t* __restrict__ a, uint64_t lo, uint64_t hi, uint64_t key) {
    while (hi - lo > 1) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] <= key) lo = mid; else hi = mid;
    }
    return lo;
}

// first index i in [lo, hi) with a[i] >= key (hi without one); a ascends on [lo, hi) (the CSRs cut from sorted keys in aix_scaffold.hip
// and aix_phase.hip, the sites under a placement)
__device__ __forceinline__ uint64_t first_ge(const uint64_t* __restrict__ a, uint64_t lo, uint64_t hi, uint64_t key) {
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the last j in [from, n) with a[j] <= key; a[from] <= key < a[n]. A gallop from `from`, then the bisection above: for keys that ascend
// with the lane, so that the search starts next to the answer (the windows of aix_seqthread.hip, the read bases of aix_pileup.hip).
__device__ __forceinline__ uint64_t gallop_last_le(const uint64_t* __restrict__ a, uint64_t n, uint64_t from, uint64_t key) {
    uint64_t lo = from, step = 1, hi;
    for (;;) {
        hi = n - lo > step ? lo + step : n;
        if (hi == n || a[hi] > key) break;
        lo = hi;
        step <<= 1;
    }
    return last_le(a, lo, hi, key);
}

// the 'N' run written for an estimated gap
__device__ __forceinline__ uint64_t written_gap(long long gap, uint32_t min_gap) { return (uint64_t)(gap > (long long)min_gap ? gap : (long long)min_gap); }

// A <-> T, C <-> G of an ASCII base: bit 1 tells C / G from A / T
__device__ __forceinline__ uint8_t comp_ascii(uint8_t c) { return c ^ ((c & 2) ? 0x04 : 0x15); }

// ---------------------------------------------------------------------------------------------
// the bases of scaffolds (a template: two translation units include it)
// ---------------------------------------------------------------------------------------------
// One lane per output byte. Byte i belongs to the last of the M members whose first byte mstart[j] is at or before it (mstart[0] == 0): a
// base of contig end member[j] in the orientation of the word, or the 'N' run behind it. kOverlap: a member with flag bit 0 (a filled
// one) overlaps its predecessor by 22 bases, which it does not write again; without it no flag array is read.
template <bool kOverlap>
__global__ void __launch_bounds__(kCB) k_graph_em_bases(uint64_t M, uint64_t total, const uint64_t* __restrict__ offsets, const uint8_t* __restrict__ bases,
                                                       const uint32_t* __restrict__ member, const uint8_t* __restrict__ flag, const uint64_t* __restrict__ mstart,
                                                       uint8_t* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * kCB;
    for (uint64_t i = (uint64_t)blockIdx.x * kCB + threadIdx.x; i < total; i += stride) {
        const uint64_t j = last_le(mstart, 0, M, i);
        const uint64_t w = member[j], a = offsets[w >> 1], len = unit_len(offsets, w);
        uint64_t x = i - mstart[j];
        if (kOverlap) x += 22 * (flag[j] & 1u);
        uint8_t c = 'N';
        if (x < len) {
            c = bases[w & 1 ? a + len - 1 - x : a + x];
            if (w & 1) c = comp_ascii(c);
        }
        out[i] = c;
    }
}

}  // namespace aix
