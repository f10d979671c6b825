// aix_posquery.hpp — the device functions of the position queries that more than one translation unit uses (aix_posquery.hip: packed
// k-mer batches; aix_seqhits.hip: the windows of sequences), and the part of the chain behind the resolve step.
#pragma once
#include "aix_hostkit.hpp"

namespace aix {

// load23 (aix_device.hpp) reads whole aligned dwords around a 23-byte window, so its last dword may reach past the final window of a
// batch. Query bytes that a host form uploads therefore sit in a block with kQueryPad spare bytes behind them: `bytes` bytes of src in a
// block of bytes + kQueryPad, on the null stream.
static constexpr uint64_t kQueryPad = 16;
static hipError_t upload_padded(DevArr& d, const void* src, uint64_t bytes) {
    AIX_TRY(d.alloc(bytes + kQueryPad));
    if (bytes) AIX_TRY(hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice));
    return hipSuccess;
}

__device__ __forceinline__ uint64_t pq_bswap(uint64_t x) { return __builtin_bswap64(x); }

__device__ __forceinline__ void pq_emit(const uint64_t* __restrict__ indices, uint64_t total, uint64_t n, uint64_t h, uint64_t& lo, uint64_t& ub) {
    lo = 0; ub = 0;
    if (h < n) {
        lo = indices[h];
        const uint64_t hi = min(indices[h + 1], total);                         // clamped to the positions array, as get_positions_13mer does (:1091)
        ub = hi > lo ? hi - lo : 0;
    }
}

// PHASH_MAP::get_pfid (hash.hpp:150-170): the strand looked up is the query's raw bytes if they compare (byte-wise) <= the decode of the
// reverse complement of their sanitised code, else that decode. Not the rule of k_a2_probe (numeric code <= rc, skip on \n ~ N): the two
// coincide on clean upper-case ACGT only. A forward strand with bytes outside ACGT hashes its RAW bytes, which the verification table
// cannot answer: MPHF path.
// The 23 bytes of a query as the three words of load23 -> source start and upper bound of its list. Wave-cooperative: all 64 lanes call
// it together (in = false: nothing to look up, lo = ub = 0).
template <int LPP>
__device__ __forceinline__ void pq_resolve23_words(const IndexDev& ix, bool in, uint64_t w0, uint64_t w1, uint64_t w2, const uint64_t* __restrict__ indices,
                                                   uint64_t total, uint64_t& lo, uint64_t& ub) {
    const Enc23 e = encode23_words(w0, w1, w2);                             // get_dna23_bitset: non-ACGT -> 0
    const uint64_t r = revcomp(e.code, 23);
    uint64_t r0, r1, r2;
    ascii23_of_rc(e.code, r0, r1, r2);                                      // decode(reverseDNA(code))
    const uint64_t a0 = pq_bswap(w0), b0 = pq_bswap(r0), a1 = pq_bswap(w1), b1 = pq_bswap(r1), a2 = pq_bswap(w2), b2 = pq_bswap(r2);
    const bool fwd = a0 != b0 ? a0 < b0 : (a1 != b1 ? a1 < b1 : a2 <= b2);  // bytes <= rev, first byte most significant
    const uint64_t want = fwd ? e.code : r;
    const uint64_t x0 = fwd ? w0 : r0, x1 = fwd ? w1 : r1, x2 = fwd ? w2 : r2;
    const bool tab = in && (e.valid || !fwd);                               // the hashed bytes are the ASCII of `want`
    uint64_t a = 0, b = 0, c = 0;
    if (in) jenkins23(x0, x1, x2, ix.m.seed, a, b, c);
    bool mphf = in;
    uint64_t h = ix.n;
    if (ix.bk) {
        const BkRes k = bucket_probe_wave<LPP>(ix.bk, ix.nb, tab, a, want);
        if (tab) {
            if (k.found) h = k.slot;
            mphf = !k.found && k.overflow;
        }
    }
    if (mphf) {
        const uint64_t s = mphf_from_hash(ix.m, a, b, c);
        if (s < ix.n && key_at(ix, s).code == want) h = s;                  // h < n and checker[h] == code of the strand looked up
    }
    lo = 0; ub = 0;
    if (in) pq_emit(indices, total, ix.n, h, lo, ub);
}

// IntervalTree::query(pos, pos + 1) of python_wrapper.cpp:66-74 on sorted, disjoint intervals: the first interval with end + 1 >= pos, taken
// if start <= pos + 1; rid = start = 0 otherwise (:757-789). Returns whether an interval was taken.
__device__ __forceinline__ bool pq_locate(const uint64_t* __restrict__ st, const uint64_t* __restrict__ en, const uint64_t* __restrict__ rid, uint64_t n,
                                          uint64_t p, uint64_t& r, uint64_t& s) {
    const uint64_t key = p ? p - 1 : 0;
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (en[mid] < key) lo = mid + 1; else hi = mid;
    }
    r = 0; s = 0;
    if (lo < n) {
        const uint64_t sv = st[lo];
        if (sv <= p || sv == p + 1) { r = rid[lo]; s = sv; return true; }
    }
    return false;
}

// Steps 2 to 5 of the chain of aix_posquery.hip, for N lists already resolved: d_lo[i] = source start of list i, d_ub[i] = its upper bound
// (N + 1 entries, the last one 0). d_offsets (N + 1) and *total_out are always produced; the entries go to d_positions (and d_rid /
// d_local) only when *total_out <= cap. own_pos, when given, takes the place of d_positions / cap: a pool block of *total_out entries is
// allocated there and filled (nothing when the total is 0). Synchronises `s`.
hipError_t posquery_lists(aix_index* h, const uint64_t* d_lo, const uint64_t* d_ub, uint64_t N, uint64_t m, uint64_t* d_offsets, uint64_t* d_positions,
                          uint64_t* d_rid, uint64_t* d_local, uint64_t cap, uint64_t* total_out, hipStream_t s, DevArr* own_pos = nullptr);

}  // namespace aix
