// aix_pile.hpp — private to the library: what the two files that read placements share. aix_pileup.hip counts the read bases of the
// placements per contig base, aix_phase.hip reads them at the variant sites. Shared here: the placement arrays of a batch, their
// validation (one predicate per entry, so that both calls refuse exactly the same arrays), the CSR lookup of an item's sequence, the base
// predicate and the exact permille comparison. The kernels themselves are not shared.
#pragma once
#include "aix_graph.hpp"

namespace aix {

__device__ __forceinline__ bool pl_is_base(uint32_t c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }

// The entry j of a CSR over M sequences that holds item t: csr[j] <= t < csr[j + 1]. Whatever the array holds, j <= M and only entries
// 0 .. M are read; false when no entry holds t (a broken CSR).
__device__ __forceinline__ bool pl_seq_of(const uint64_t* __restrict__ csr, uint64_t M, uint64_t t, uint64_t& j, uint64_t& lo, uint64_t& hi) {
    j = last_le(csr, 0, M + 1, t);
    if (j >= M) return false;
    lo = csr[j];
    hi = csr[j + 1];
    return lo <= t && t < hi;
}

// what the validations repeat for entry i of max(M, U) + 1: sequence offsets ascend by less than 2^32, the CSR starts at 0, ascends and
// ends at `total`, contig offsets start at 0 and ascend by at least 23
__device__ __forceinline__ unsigned pl_frame_bad(uint64_t i, uint64_t M, const uint64_t* __restrict__ offs, const uint64_t* __restrict__ csr, uint64_t total, uint64_t U,
                                                 const uint64_t* __restrict__ offsets) {
    unsigned bad = 0;
    if (i < M) {
        const uint64_t a = offs[i], b = offs[i + 1];
        bad += b < a || b - a >= (1ull << 32);
        bad += csr_bad(i, M, csr[i], csr[i + 1], total, kAnyDegree);
    }
    if (i < U) bad += span_bad(offsets[i], offsets[i + 1]);
    if (i == 0) bad += offsets[0] != 0;
    return bad;
}

struct PlPlaces {                                                 // the placements of a batch of M sequences on U contigs
    uint64_t M, R, U;
    const uint64_t *offs, *spo;
    const uint32_t* unitig;
    const uint8_t* flag;
    const uint32_t *pos, *q0, *len;
    const uint64_t* offsets;
};

// the violations entry i of max(max(M, U) + 1, R) sees: the frame, and placement i inside its read and its contig
__device__ __forceinline__ unsigned pl_places_bad(const PlPlaces& g, uint64_t i) {
    unsigned bad = pl_frame_bad(i, g.M, g.offs, g.spo, g.R, g.U, g.offsets);
    if (i >= g.R) return bad;
    uint64_t j, lo, hi;
    if (!pl_seq_of(g.spo, g.M, i, j, lo, hi)) return bad + 1;
    const uint64_t sa = g.offs[j], sb = g.offs[j + 1], u = g.unitig[i], len = g.len[i];
    if (sb < sa || u >= g.U || len < 1 || (uint64_t)g.q0[i] + len > sb - sa) return bad + 1;
    const uint64_t ulo = g.offsets[u], uhi = g.offsets[u + 1];
    return bad + (uhi < ulo || (uint64_t)g.pos[i] + len > uhi - ulo);
}

// 1000 c >= permille D as a1000 >= permille D, exactly, in 64 bits: a 32-bit threshold times D (up to 2^34 - 4) can pass 2^64 and wrap,
// but c <= D, so above 1000 permille only D == 0 reaches it (0 >= 0), and up to 1000 the product stays below 2^44. The first test is
// wave-uniform.
__device__ __forceinline__ bool pl_reaches(uint64_t a1000, uint32_t permille, uint64_t D) { return (permille <= 1000u || D == 0) && a1000 >= (uint64_t)permille * D; }

}  // namespace aix
