// aix_seqhits.hpp — what more than one translation unit uses of the chain sequences -> windows -> seed hits (aix_seqhits.hip: hits and
// diagonal votes; aix_seqfind.hip: Hamming-verified alignments and strand counts; aix_seqedit.hip: edit-distance alignments): the hit
// buffers, steps 1 to 4 with a window stride, the gather of a permutation, the device helpers of the verification kernels, and of the host
// ends of the C ABI the two steps that are the sequence files' own: sh_check (what must be attached) and sh_upload (ragged sequences into
// HBM). Everything else of a host form — error mapping, scans, the stable sort passes, zero_offsets, the HostOut epilogue — is that of
// aix_hostkit.hpp.
#pragma once
#include <algorithm>

#include "aix_posquery.hpp"

// bytes of a pattern that one trip of the verification loop of aix_seqfind.hip compares (16 lanes x one dword). Not part of the C ABI:
// _lib.SEQFIND_TRIP_BYTES repeats it for the tests that place pattern lengths around its multiples.
#define AIX_SEQFIND_TRIP_BYTES 64u
// the largest edit distance aix_seq_edit accepts: a band of 2 * 7 + 1 = 15 diagonals fits the 16 lanes that share one proposal
// (aix_seqedit.hip). Not part of the C ABI's types; include/aindex_hip.h states the bound and _lib.SEQEDIT_MAX_ED repeats it.
#define AIX_SEQEDIT_MAX_ED 7u

namespace aix {

static constexpr int kSB = kFlatBlock;                            // the grid of the flat kernels: flat_grid (aix_hostkit.hpp)

// n entries of `elem` bytes from the pool; hipErrorOutOfMemory when the byte count does not fit 64 bits
static hipError_t sh_alloc(DevArr& a, uint64_t n, uint64_t elem) {
    uint64_t bytes = 0;
    if (__builtin_mul_overflow(n, elem, &bytes) || bytes >= (1ull << 62)) return hipErrorOutOfMemory;
    return a.alloc(bytes);
}

// what the hits of a call live in: the user's buffers (aix_seq_hits_dev) or pool blocks (everything else)
struct ShBufs {
    DevArr woff, koff, pos, qoff, rid, local, flag, hseq, diag;
    uint64_t W = 0, T = 0;
    explicit ShBufs(hipStream_t s) : woff(s), koff(s), pos(s), qoff(s), rid(s), local(s), flag(s), hseq(s), diag(s) {}
};

struct ShUser {                    // aix_seq_hits_dev: where the entries go when they fit `cap`
    uint32_t* qoff;
    uint64_t* pos;
    uint64_t* rid;
    int64_t* local;
    uint8_t* flag;
    uint64_t cap;
};

// Steps 1 to 4 of aix_seqhits.hip for M sequences: the windows at offsets 0, step, 2 step, .. <= L - 23 of every sequence (step 1: all of
// them, what aix_seq_hits* and aix_seq_votes* ask for), their lists, and the hits with strand and interval; qoff is the window's offset.
// locate false (user == nullptr, votes false): the interval search is left out, B.rid / B.local stay empty and the flag holds the strand alone.
hipError_t sh_run(aix_index* h, const uint8_t* d_seqs, const uint64_t* d_offs, uint64_t M, uint64_t m, uint64_t* d_seq_offsets, const ShUser* user, bool votes, ShBufs& B,
                  bool* bad, hipStream_t s, uint64_t step = 1, bool locate = true);

template <class T, class Map>
__global__ void __launch_bounds__(kSB) k_sv_gather(const T* __restrict__ in, const uint64_t* __restrict__ perm, uint64_t n, Map map, T* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * kSB;
    for (uint64_t i = (uint64_t)blockIdx.x * kSB + threadIdx.x; i < n; i += stride) out[i] = map(in[perm[i]]);
}
struct SvSame { template <class T> __host__ __device__ T operator()(T v) const { return v; } };

// A stable pass of a permutation is sort_pairs over sort_bits(largest key) (aix_hostkit.hpp): keys (any iterator) in the order of perm_in -> perm_out. rocPRIM's temporary
// storage is as large as the keys and values together: the passes of a chain share ONE block (tmp.alloc waits for the pass before it, then
// takes the block back from the pool)

// ---- device helpers of the verification kernels (aix_seqfind.hip: Hamming; aix_seqedit.hip: banded edit distance) ----
// bytes [p, p + 4) of a buffer of `size` bytes, first byte least significant; a byte outside [0, size) reads as 0 and is never touched.
// Inside, two aligned dwords (they reach up to 3 bytes before p and 4 behind p + 4); within 3 bytes of the start or 8 of the end, bytes.
__device__ __forceinline__ uint32_t sf_load4(const uint8_t* __restrict__ buf, uint64_t size, int64_t p) {
    if (p >= 3 && (uint64_t)p < size && size - (uint64_t)p >= 8) {
        const uint8_t* at = buf + p;
        const uint32_t o = (uint32_t)((uintptr_t)at & 3);
        const uint32_t* q = (const uint32_t*)(at - o);         // pointer arithmetic, as load23: the loads stay global_load
        return __funnelshift_r(q[0], q[1], o * 8);
    }
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int64_t at = p + b;
        if (at >= 0 && (uint64_t)at < size) v |= (uint32_t)buf[at] << (8 * b);
    }
    return v;
}

// A <-> T, C <-> G, a <-> t, c <-> g, every other byte as it is
__device__ __forceinline__ uint32_t sf_comp(uint32_t c) {
    const uint32_t u = c & 0xDFu, lower = c & 0x20u;
    const uint32_t r = u == 'A' ? 'T' : u == 'T' ? 'A' : u == 'C' ? 'G' : u == 'G' ? 'C' : 0u;
    return r ? (r | lower) : c;
}

__device__ __forceinline__ uint64_t sf_shfl64(uint64_t v, uint32_t src) {
    return (uint64_t)bperm(src, (uint32_t)v) | ((uint64_t)bperm(src, (uint32_t)(v >> 32)) << 32);
}

}  // namespace aix

static int sh_check(const aix_index* h) {
    if (h->k != 23) return AIX_ERR_MODE;
    if (!h->att.ai_indices.attached || !h->att.rx || !h->att.rd.attached) return AIX_ERR_ARG;     // nothing attached: a defined error, never a fault
    if (h->n == 0) return AIX_ERR_UNSUPPORTED;
    return AIX_OK;
}

// the sequences of a host call in HBM: bytes (upload_padded, aix_posquery.hpp) and offsets
static int sh_upload(const char* seqs, const uint64_t* offs, uint64_t M, DevArr& ds, DevArr& dof) {
    const uint64_t bytes = M ? offs[M] : 0;
    if (bytes >= (1ull << 60)) return AIX_ERR_NOMEM;
    const HostIn in{offs, 8 * (M + 1)};
    AIXCHK(upload_padded(ds, seqs, bytes));
    AIXCHK(copy_in_host(&dof, &in, 1));
    return AIX_OK;
}
