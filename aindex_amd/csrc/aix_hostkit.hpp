// aix_hostkit.hpp — private to the library: the host scaffolding that the subsystem files (one translation unit per subsystem behind the
// C ABI) share. Error mapping, rocPRIM's two-call protocol, the prologue and the epilogue of the host forms (copy_in_host, copy_out_host).
// The query files (aix_posquery, aix_readsquery, aix_seqhits, aix_seqfind, aix_seqedit), the graph files and aix_seqthread use all of it:
// their chains are AIX_TRY / AIX_TRY_LAUNCH, their host forms hold DevArr and publish through one HostOut table. The distinct-k-mer chain
// and the positions fill (aix_k1, aix_merge, aix_positions, aix_a2msd, and aix_msd.hpp between them) use the chain half: AIX_TRY /
// AIX_TRY_LAUNCH over DevArr, with_temp, flat_grid; their extern "C" halves keep HIPCHK and DevBuf. Nothing here is on a hot path, and
// nothing that only one file uses belongs here. The files that work on the index handle (aix_index, aix_count, aix_lookup*, and the
// attach halves of aix_posquery and aix_readsquery) and aix_ingest keep HIPCHK and their own error style, so they do not use this
// header (their kernels are launched through aix_launch.hpp); what they hold lives in the owners of aix_owned.hpp (blocks, streams, events, the two exit guards), through which the handle
// frees itself. aix_normalize and aix_count13 keep raw pool blocks.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>                                                // (rocPRIM's headers use memset without including it)
#include <string>

#include <rocprim/rocprim.hpp>

#include "aix_handle.hpp"

// HIP error -> ABI status, inside a function that returns one: out of memory is AIX_ERR_NOMEM with the sticky error cleared, anything
// else is the text behind aix_strerror and AIX_ERR_HIP. (HIPCHK, aix_handle.hpp, is for calls where out of memory is not expected.)
#define AIXCHK(expr)                                                                             \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e == hipErrorOutOfMemory) { (void)hipGetLastError(); return AIX_ERR_NOMEM; }        \
        if (_e != hipSuccess) {                                                                  \
            set_last_error(std::string(#expr) + ": " + hipGetErrorString(_e));                   \
            return AIX_ERR_HIP;                                                                  \
        }                                                                                        \
    } while (0)

// inside a function that returns hipError_t: pass an error on; a launch is followed by hipGetLastError()
#define AIX_TRY(expr)                            \
    do {                                         \
        const hipError_t e_ = (expr);            \
        if (e_ != hipSuccess) return e_;         \
    } while (0)
#define AIX_TRY_LAUNCH(...)                      \
    do {                                         \
        hipLaunchKernelGGL(__VA_ARGS__);         \
        AIX_TRY(hipGetLastError());              \
    } while (0)

namespace aix {

// Grid of the query files' flat kernels (workgroups of 256, grid-stride): a workgroup per 256 items up to 8192, then a quarter of that
// up to 65536.
static constexpr int kFlatBlock = 256;
static inline unsigned flat_grid(uint64_t work) {
    uint64_t b = (work + kFlatBlock - 1) / kFlatBlock;
    if (b > 8192) b = std::max<uint64_t>(8192, std::min<uint64_t>(b / 4, 65536));
    if (b == 0) b = 1;
    return (unsigned)b;
}

static inline int ceil_log2(uint64_t v) {                         // smallest r with 2^r >= v
    int r = 0;
    while (r < 64 && (1ULL << r) < v) ++r;
    return r;
}
static inline int bit_length(uint64_t v) {
    int r = 0;
    while (v) { ++r; v >>= 1; }
    return r;
}
static inline unsigned sort_bits(uint64_t v) {                    // end_bit of a radix sort whose keys are <= v: at least one bit (v == 0)
    return (unsigned)std::max(1, bit_length(v));
}

template <class T>
struct Widen {                                                    // an integer as the u64 a scan sums
    __host__ __device__ uint64_t operator()(T v) const { return (uint64_t)v; }
};

// rocPRIM's two calls: call(nullptr, bytes) asks for the size of the temporary storage, `tmp` takes a block of that size, call(tmp.p,
// bytes) enqueues the work. THE CONTRACT OF THE BLOCK: `tmp` stays allocated until the caller has synchronised the stream. DevArr::alloc
// on a live block synchronises the stream first, so a DevArr that serves several calls in a row makes each wait for the one before it,
// and one DevArr per call does not.
template <class F>
static hipError_t with_temp(DevArr& tmp, F&& call) {
    size_t tb = 0;
    hipError_t e = call((void*)nullptr, tb);
    if (e == hipSuccess) e = tmp.alloc(tb ? tb : 1);
    if (e == hipSuccess) e = call(tmp.p, tb);
    return e;
}

// out[i] = in[0] + .. + in[i - 1] over n entries, u64 sums
template <class It>
static hipError_t scan_u64(It in, uint64_t* out, uint64_t n, DevArr& tmp, hipStream_t s) {
    return with_temp(tmp, [&](void* t, size_t& tb) { return rocprim::exclusive_scan(t, tb, in, out, (uint64_t)0, (size_t)n, rocprim::plus<uint64_t>(), s); });
}

// stable radix sort of n (key, value) pairs by bits [0, end_bit) of the key; the inputs may be any iterators
template <class KeyIt, class Key, class ValIt, class Val>
static hipError_t sort_pairs(KeyIt keys_in, Key* keys_out, ValIt vals_in, Val* vals_out, uint64_t n, unsigned end_bit, DevArr& tmp, hipStream_t s) {
    return with_temp(tmp, [&](void* t, size_t& tb) { return rocprim::radix_sort_pairs(t, tb, keys_in, keys_out, vals_in, vals_out, (size_t)n, 0u, end_bit, s); });
}

// the answer to a batch without entries: n + 1 offsets, all zero, and `s` synchronised
static hipError_t zero_offsets(uint64_t* d_offsets, uint64_t n, hipStream_t s) {
    AIX_TRY(hipMemsetAsync(d_offsets, 0, 8 * (n + 1), s));
    return hipStreamSynchronize(s);
}

// The prologue of a host form: in[i] becomes a device copy of block i of the table, on the null stream; zero bytes is still a block of its
// own. skip_null: a null src is an input the caller did not give and its in[i] stays empty; without it every src is the caller's to check.
struct HostIn {
    const void* src;
    uint64_t bytes;
};
static hipError_t copy_in_host(DevArr* in, const HostIn* ins, int n, bool skip_null = false) {
    for (int i = 0; i < n; ++i) {
        if (skip_null && !ins[i].src) continue;
        AIX_TRY(in[i].alloc(ins[i].bytes));
        if (ins[i].bytes) AIX_TRY(hipMemcpy(in[i].p, ins[i].src, ins[i].bytes, hipMemcpyHostToDevice));
    }
    return hipSuccess;
}

// The epilogue of a host form: every device block of the table as a malloc'd host copy (aix_free). A null dst is an output the caller
// did not ask for; zero bytes is still a block of its own. On a failure everything is freed and nothing is published.
struct HostOut {
    void** dst;
    const void* src;
    uint64_t bytes;
};
static hipError_t copy_out_host(const HostOut* outs, int n) {
    constexpr int kMax = 16;
    void* host[kMax] = {nullptr};
    if (n > kMax) return hipErrorInvalidValue;
    hipError_t e = hipSuccess;
    for (int i = 0; i < n && e == hipSuccess; ++i) {
        if (!outs[i].dst) continue;
        host[i] = malloc(outs[i].bytes ? outs[i].bytes : 1);
        if (!host[i]) e = hipErrorOutOfMemory;
        else if (outs[i].bytes) e = hipMemcpy(host[i], outs[i].src, outs[i].bytes, hipMemcpyDeviceToHost);
    }
    if (e != hipSuccess) {
        for (void* p : host) free(p);
        return e;
    }
    for (int i = 0; i < n; ++i)
        if (outs[i].dst) *outs[i].dst = host[i];
    return hipSuccess;
}

}  // namespace aix
