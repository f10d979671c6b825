// aix_api.hip — what the C ABI of libaindex_hip.so (include/aindex_hip.h) has outside the subsystems: version and error text, device
// count, pinned host memory, scratch trim, self-test and debug hooks, the synthetic generators and two stand-alone kernels (window codes,
// the random-gather roofline probe), each kernel above its entry point.
// Every subsystem keeps its own entry points: aix_index.hip (handles), aix_lookup.hip, aix_count.hip, aix_normalize.hip,
// aix_positions.hip, aix_posquery.hip, aix_merge.hip (distinct k-mers), aix_ingest.hip (files and host buffers of the counters).
#include <string>

#include "aix_handle.hpp"
#include "aix_ingest.hpp"
#include "aix_launch.hpp"

static thread_local std::string g_last_error;
void set_last_error(const std::string& s) { g_last_error = s; }

// ---------------------------------------------------------------------------------------------
extern "C" const char* aix_version(void) { return "aindex_hip 0.1.0 (gfx950)"; }

extern "C" const char* aix_strerror(int st) {
    switch (st) {
        case AIX_OK: return "ok";
        case AIX_ERR_ARG: return "invalid argument";
        case AIX_ERR_IO: return "file missing, unreadable or short";
        case AIX_ERR_FORMAT: return "malformed index file";
        case AIX_ERR_NOMEM: return "out of memory";
        case AIX_ERR_HIP: return g_last_error.empty() ? "HIP runtime error / no device" : g_last_error.c_str();
        case AIX_ERR_UNSUPPORTED: return "unsupported size or configuration";
        case AIX_ERR_MODE: return "call does not match the handle's k-mer mode";
        case AIX_ERR_CONFLICT: return "hash conflict while scattering (key not in the MPHF set)";
        default: return "unknown status";
    }
}

extern "C" int aix_device_count(int* count) {
    if (!count) return AIX_ERR_ARG;
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess || c <= 0) {
        *count = 0;
        set_last_error(std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
        return AIX_ERR_HIP;
    }
    *count = c;
    return AIX_OK;
}

extern "C" void aix_scratch_trim(void) { pool_trim(); pinned_trim(); }

extern "C" int aix_host_alloc(uint64_t bytes, void** out) {
    if (!out) return AIX_ERR_ARG;
    *out = nullptr;
    if (bytes == 0) return AIX_OK;
    void* p = nullptr;
    const hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
    if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); set_last_error("aix_host_alloc: out of pinned memory"); return AIX_ERR_NOMEM; }
    HIPCHK(e);
    *out = p;
    return AIX_OK;
}
extern "C" int aix_host_free(void* p) {
    if (!p) return AIX_OK;
    HIPCHK(hipHostFree(p));
    return AIX_OK;
}

extern "C" uint64_t aix_selftest_mod(uint64_t h, uint64_t d) { return fastmod(h, make_fastmod(d)); }
extern "C" uint64_t aix_selftest_revcomp(uint64_t code, int k) { return revcomp(code, k); }

// Move the verification table of a 23-mer handle into another block of HBM: d_dst (nb * 128 bytes, caller-owned and kept alive by the caller
// for the life of the handle) or, with d_dst == NULL, a block allocated now. Placement experiments only (scripts/gpu_r3_relocate.py).
extern "C" int aix_debug_relocate_table(aix_index_t* h, void* d_dst) {
    if (!h || h->k != 23 || !h->bk.p) return AIX_ERR_ARG;
    DevGuard g(h->device);
    const uint64_t bytes = (uint64_t)h->nb * 8 * sizeof(BkEntry), counted = h->bk.counted;   // the ledger keeps the table wherever it lives
    HBlock own;
    if (!d_dst) HIPCHK(own.alloc(bytes, counted));
    HIPCHK(hipMemcpy(d_dst ? d_dst : own.p, h->bk.p, bytes, hipMemcpyDeviceToDevice));
    HIPCHK(hipDeviceSynchronize());
    if (d_dst) h->bk.attach_borrowed(d_dst, counted);
    else h->bk.attach_owned(std::move(own));
    return AIX_OK;
}

// the same for the absence filter; the old block is NOT freed (the next candidate must come from other physical pages): experiments only
extern "C" int aix_debug_relocate_bloom(aix_index_t* h, uint64_t pad_bytes) {
    if (!h || h->k != 23 || !h->bloom) return AIX_ERR_ARG;
    DevGuard g(h->device);
    void* pad = nullptr;
    if (pad_bytes) HIPCHK(hipMalloc(&pad, pad_bytes));               // leaked on purpose: shifts where the next block lands
    HBlock nb_;
    HIPCHK(nb_.alloc(8ull * h->nbloom, h->bloom.counted));
    HIPCHK(hipMemcpy(nb_.p, h->bloom.p, 8ull * h->nbloom, hipMemcpyDeviceToDevice));
    HIPCHK(hipDeviceSynchronize());
    (void)h->bloom.leak();
    h->bloom = std::move(nb_);
    return AIX_OK;
}

// Move any subset of a 23-mer handle's device arrays into freshly allocated blocks (mask: 1 MPHF records, 2 side index, 4 unfiled keys, 8 verification
// table, 16 absence filter); the old blocks are NOT freed (the table's only behind the new one's allocation), so that the new ones come
// from other memory. Placement experiments only (scripts/experiments/r3/rehome.py).
extern "C" int aix_debug_rehome(aix_index_t* h, uint32_t mask) {
    if (!h || h->k != 23) return AIX_ERR_ARG;
    DevGuard g(h->device);
    auto copy = [&](const void* from, uint64_t bytes, uint64_t counted, HBlock& to) -> int {
        HIPCHK(to.alloc(bytes, counted));
        HIPCHK(hipMemcpy(to.p, from, bytes, hipMemcpyDeviceToDevice));
        return AIX_OK;
    };
    auto move = [&](HBlock& field, uint64_t bytes) -> int {
        if (!field || !bytes) return AIX_OK;
        HBlock nb_;
        if (const int st = copy(field.p, bytes, field.counted, nb_)) return st;
        (void)field.leak();
        field = std::move(nb_);
        return AIX_OK;
    };
    int st = AIX_OK;
    if (!st && (mask & 1)) st = move(h->mphf.recs, (uint64_t)((h->mphf.B + 15) / 16) * sizeof(BvRec));
    if (!st && (mask & 2)) st = move(h->side, 4ull * h->n);
    if (!st && (mask & 4)) st = move(h->unfiled, (uint64_t)h->n_unfiled * sizeof(KeyRec));
    if (!st && (mask & 8) && h->bk.owned && h->nb) {
        HBlock nb_;
        const uint64_t counted = h->bk.counted;
        st = copy(h->bk.p, (uint64_t)h->nb * 8 * sizeof(BkEntry), counted, nb_);
        if (!st) h->bk.attach_owned(std::move(nb_));          // (the old table goes back only now, behind the new one's allocation)
    }
    if (!st && (mask & 16)) st = move(h->bloom, 8ull * h->nbloom);
    HIPCHK(hipDeviceSynchronize());
    return st;
}

// host copy of the absence filter (nwords must be the handle's absence_filter_words): for the suite, which rebuilds the filter from the keys
extern "C" int aix_debug_filter_words(aix_index_t* h, uint64_t* out, uint64_t nwords) {
    if (!h || !out || !h->bloom || h->nbloom == 0 || nwords != h->nbloom) return AIX_ERR_ARG;
    DevGuard g(h->device);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, h->bloom.p, 8ull * h->nbloom, hipMemcpyDeviceToHost));
    return AIX_OK;
}

namespace aix {
// self-test of wave_lower_bound_pair (aix_device.hpp): wave w of the grid looks up keys[w] and keys[w] + 1 in the sorted array
__global__ void __launch_bounds__(64) k_selftest_lower_bound(const uint16_t* __restrict__ a, uint32_t n, const uint32_t* __restrict__ keys, uint32_t* __restrict__ out) {
    const uint32_t r = wave_lower_bound_pair(a, n, keys[blockIdx.x]);
    if ((threadIdx.x & 31u) == 0) out[2 * blockIdx.x + (threadIdx.x >> 5)] = r;
}
}  // namespace aix
// GPU self-test hook of the suite: lower bounds of keys[i] and keys[i] + 1 in a sorted u16 array, by the wave-wide search the partition kernels
// use to find a partition's chunks (out[2 i], out[2 i + 1]); all pointers are device pointers
extern "C" int aix_selftest_lower_bound_dev(const uint16_t* d_sorted, uint32_t n, const uint32_t* d_keys, uint32_t nkeys, uint32_t* d_out, void* stream) {
    if ((n && !d_sorted) || (nkeys && (!d_keys || !d_out))) return AIX_ERR_ARG;
    if (nkeys == 0) return AIX_OK;
    hipLaunchKernelGGL(k_selftest_lower_bound, dim3(nkeys), dim3(64), 0, (hipStream_t)stream, d_sorted, n, d_keys, d_out);
    HIPCHK(hipGetLastError());
    return AIX_OK;
}

// device addresses of a handle's arrays (same order as the mask bits of aix_debug_rehome): experiments only
extern "C" int aix_debug_pointers(const aix_index_t* h, uint64_t out[5]) {
    if (!h || !out) return AIX_ERR_ARG;
    out[0] = (uint64_t)(uintptr_t)h->mphf.recs.p; out[1] = (uint64_t)(uintptr_t)h->side.p; out[2] = (uint64_t)(uintptr_t)h->unfiled.p;
    out[3] = (uint64_t)(uintptr_t)h->bk.p; out[4] = (uint64_t)(uintptr_t)h->bloom.p;
    return AIX_OK;
}

namespace aix {
// K1 front end (count_kmers.cpp:93-136,297-308): the canonical 2-bit code of every window of a PLAIN
// buffer, ~0 where the window holds a non-base byte. Distinct counting = sort + run-length of this.
template <int K>
__global__ void __launch_bounds__(kBlock) k_window_codes(const uint8_t* __restrict__ buf, uint64_t len, int k, int canon_mode, uint64_t* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    if (len < (uint64_t)k) return;
    const uint64_t nwin = len - k + 1;
    for (uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x; p < nwin; p += stride) {
        uint64_t code = 0;
        bool valid = true;
        if (K == 23) {
            uint64_t w0, w1, w2;
            load23(buf + p, w0, w1, w2);
            w0 = u_to_t(w0 & 0xDFDFDFDFDFDFDFDFULL);
            w1 = u_to_t(w1 & 0xDFDFDFDFDFDFDFDFULL);
            w2 = u_to_t(w2 & 0x00DFDFDFDFDFDFDFULL);
            const Enc23 e = encode23_words(w0, w1, w2);
            code = e.code; valid = e.valid;
        } else if (K == 13) {
            uint64_t w0, w1;
            load13(buf + p, w0, w1);
            w0 = u_to_t(w0 & 0xDFDFDFDFDFDFDFDFULL);
            w1 = u_to_t(w1 & 0x000000DFDFDFDFDFULL);
            const Enc13 e = encode13_words(w0, w1);
            code = e.code; valid = e.valid;
        } else {
            for (int j = 0; j < k; ++j) {
                uint32_t c = buf[p + j] & 0xDFu;
                c = c == 'U' ? 'T' : c;
                const uint32_t v = c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u;
                if (v == 4u) { valid = false; break; }
                code = (code << 2) | v;
            }
        }
        if (valid) {
            if (canon_mode == 1) { const uint64_t x = revcomp_refx86(code, k); code = code < x ? code : x; }
            else if (canon_mode == 2) { const uint64_t x = revcomp(code, k); code = code < x ? code : x; }
        }
        out[p] = valid ? code : ~0ULL;
    }
}
hipError_t launch_window_codes(const uint8_t* buf, uint64_t len, int k, int canon_mode, uint64_t* out, hipStream_t s) {
    if (len < (uint64_t)k) return hipSuccess;
    if (k == 23) return launch_flat(k_window_codes<23>, len - k + 1, s, buf, len, k, canon_mode, out);
    if (k == 13) return launch_flat(k_window_codes<13>, len - k + 1, s, buf, len, k, canon_mode, out);
    return launch_flat(k_window_codes<0>, len - k + 1, s, buf, len, k, canon_mode, out);
}
}  // namespace aix

extern "C" int aix_window_codes_dev(const char* d_plain, uint64_t len, int k, int canon_mode, uint64_t* d_codes, void* stream) {
    if ((len && !d_plain) || k < 1 || k > 32 || canon_mode < 0 || canon_mode > 2) return AIX_ERR_ARG;
    if (len < (uint64_t)k) return AIX_OK;
    if (!d_codes) return AIX_ERR_ARG;
    HIPCHK(launch_window_codes((const uint8_t*)d_plain, len, k, canon_mode, d_codes, (hipStream_t)stream));
    return AIX_OK;
}

namespace aix {
// ---------------------------------------------------------------------------------------------
// synthetic inputs (bit-identical to aindex_amd/synth.py)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t sm64(uint64_t seed, uint64_t idx) {
    uint64_t z = seed + (idx + 1) * 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
__global__ void __launch_bounds__(kBlock) k_synth_genome(uint64_t seed, uint64_t length, uint8_t* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < length; j += stride) {
        const uint64_t v = sm64(seed, j >> 5);
        out[j] = (uint8_t)(AIX_LUT_ACGT >> (8 * ((v >> (2 * (j & 31))) & 3)));
    }
}
__global__ void __launch_bounds__(kBlock) k_synth_kmers(uint64_t seed, uint64_t first, uint64_t N, int k, uint8_t* __restrict__ out) {
    const uint64_t total = N * (uint64_t)k, stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += stride) {
        const uint64_t i = t / (uint64_t)k, j = t - i * (uint64_t)k;
        const uint64_t v = sm64(seed, first + i);
        out[t] = (uint8_t)(AIX_LUT_ACGT >> (8 * ((v >> (2 * (k - 1 - (int)j))) & 3)));
    }
}
__global__ void __launch_bounds__(kBlock) k_synth_reads(uint64_t seed, const uint8_t* __restrict__ genome, uint64_t glen, uint64_t first_read, uint64_t n_reads,
                                                       uint32_t read_len, int rc_half, uint32_t n_ppm, uint8_t* __restrict__ out) {
    const uint64_t rec = (uint64_t)read_len + 1, total = n_reads * rec, stride = (uint64_t)gridDim.x * kBlock;
    const uint64_t span = glen - read_len + 1;
    for (uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += stride) {
        const uint64_t ri = t / rec, j = t - ri * rec;
        if (j == read_len) { out[t] = '\n'; continue; }
        const uint64_t r = first_read + ri;
        const uint64_t v = sm64(seed, 2 * r);
        const uint64_t start = ((v >> 32) * span) >> 32;
        uint8_t ch;
        if (rc_half && (sm64(seed, 2 * r + 1) & 1)) {
            const uint8_t g = genome[start + (read_len - 1 - j)];
            ch = g == 'A' ? 'T' : g == 'C' ? 'G' : g == 'G' ? 'C' : g == 'T' ? 'A' : g;
        } else {
            ch = genome[start + j];
        }
        if (n_ppm) {
            const uint64_t h = sm64(seed ^ 0x5851F42D4C957F2DULL, r * read_len + j);
            if ((((h >> 32) * 1000000ULL) >> 32) < n_ppm) ch = 'N';
        }
        out[t] = ch;
    }
}

// Q_mix of SURVEY §8d: query i is, with probability 1/2, a 23-mer window of the genome at a uniform position on a
// uniform strand, else a uniform-random 23-mer.
__global__ void __launch_bounds__(kBlock) k_synth_mix23(uint64_t seed, const uint8_t* __restrict__ genome, uint64_t glen, uint64_t first, uint64_t N,
                                                       uint8_t* __restrict__ out) {
    const uint64_t total = N * 23, stride = (uint64_t)gridDim.x * kBlock;
    const uint64_t span = glen - 22;
    for (uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += stride) {
        const uint64_t i = t / 23, j = t - i * 23;
        const uint64_t v = sm64(seed, first + i);
        uint8_t ch;
        if (v & 1) {
            const uint64_t r = sm64(seed ^ 0xA5A5A5A5ULL, first + i);
            ch = (uint8_t)(AIX_LUT_ACGT >> (8 * ((r >> (2 * (22 - (int)j))) & 3)));
        } else {
            const uint64_t pos = ((v >> 32) * span) >> 32;
            if (v & 2) {
                const uint8_t g = genome[pos + 22 - j];
                ch = g == 'A' ? 'T' : g == 'C' ? 'G' : g == 'G' ? 'C' : g == 'T' ? 'A' : g;
            } else {
                ch = genome[pos + j];
            }
        }
        out[t] = ch;
    }
}

// ---------------------------------------------------------------------------------------------
// random-gather roofline probe: uniform-random ELEM-byte reads over a large table,
// UNROLL independent reads in flight per lane. The denominator the lookup kernels are judged against.
// ---------------------------------------------------------------------------------------------
template <int ELEM, int UNROLL>
__global__ void __launch_bounds__(kBlock) k_gather(const uint8_t* __restrict__ table, uint64_t n_elems, uint64_t n_access, uint64_t seed, uint64_t* __restrict__ sink) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock * UNROLL;
    uint64_t acc = 0;
    for (uint64_t i = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) * UNROLL; i < n_access; i += stride) {
        uint64_t idx[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) idx[u] = ((sm64(seed, i + u) >> 32) * n_elems) >> 32;
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            if (ELEM >= 32) {                                   // the whole element: ELEM / 16 loads of 16 bytes (a 64-byte half line, a 128-byte line)
                const uint4* p = (const uint4*)(table + idx[u] * (uint64_t)ELEM);
#pragma unroll
                for (int t = 0; t < ELEM / 16; ++t) { const uint4 v = p[t]; acc += (uint64_t)v.x ^ v.w; }
            } else if (ELEM == 16) {
                const BvRec r = ((const BvRec*)table)[idx[u]];
                acc += r.fp ^ r.prefix;
            } else if (ELEM == 8) {
                acc += ((const uint64_t*)table)[idx[u]];
            } else {
                acc += ((const uint32_t*)table)[idx[u]];
            }
        }
    }
    if (acc == 0x1234567887654321ULL) sink[0] = acc;   // keeps the loads alive; practically never taken
}
}  // namespace aix

extern "C" int aix_bench_gather_dev(const void* d_table, uint64_t n_elems, int elem_bytes, int unroll, uint64_t n_access, uint64_t seed, uint64_t* d_sink,
                                    void* stream) {
    if (!d_table || !d_sink || n_elems == 0 || (n_elems >> 32)) return AIX_ERR_ARG;
    if (n_access == 0) return AIX_OK;
    hipError_t gather_launch = hipErrorInvalidValue;                           // an (elem_bytes, unroll) pair that is not instantiated
#define G(E, U) if (elem_bytes == E && unroll == U) gather_launch = launch_flat(k_gather<E, U>, (n_access + U - 1) / U, (hipStream_t)stream, (const uint8_t*)d_table, n_elems, n_access, seed, d_sink)
    G(16, 1); G(16, 4); G(8, 1); G(8, 4); G(4, 1); G(4, 4); G(32, 1); G(64, 1); G(128, 1);
#undef G
    HIPCHK(gather_launch);
    return AIX_OK;
}

extern "C" int aix_synth_genome_dev(uint64_t seed, uint64_t length, char* d_out, void* stream) {
    if (length && !d_out) return AIX_ERR_ARG;
    if (length) HIPCHK(launch_flat(k_synth_genome, length, (hipStream_t)stream, seed, length, (uint8_t*)d_out));
    return AIX_OK;
}
extern "C" int aix_synth_kmers_dev(uint64_t seed, uint64_t first, uint64_t N, int k, char* d_out, void* stream) {
    if ((N && !d_out) || k < 1 || k > 32) return AIX_ERR_ARG;
    if (N) HIPCHK(launch_flat(k_synth_kmers, N * (uint64_t)k, (hipStream_t)stream, seed, first, N, k, (uint8_t*)d_out));
    return AIX_OK;
}
extern "C" int aix_synth_mix23_dev(uint64_t seed, const char* d_genome, uint64_t genome_len, uint64_t first, uint64_t N, char* d_out, void* stream) {
    if (!d_genome || (N && !d_out) || genome_len < 23) return AIX_ERR_ARG;
    if (N) HIPCHK(launch_flat(k_synth_mix23, N * 23, (hipStream_t)stream, seed, (const uint8_t*)d_genome, genome_len, first, N, (uint8_t*)d_out));
    return AIX_OK;
}
extern "C" int aix_synth_reads_dev(uint64_t seed, const char* d_genome, uint64_t genome_len, uint64_t first_read, uint64_t n_reads, uint32_t read_len,
                                   int rc_half, uint32_t n_rate_ppm, char* d_out, void* stream) {
    if (!d_genome || (n_reads && !d_out) || read_len == 0 || genome_len < read_len) return AIX_ERR_ARG;
    if (n_reads) HIPCHK(launch_flat(k_synth_reads, n_reads * ((uint64_t)read_len + 1), (hipStream_t)stream, seed, (const uint8_t*)d_genome, genome_len, first_read, n_reads,
                                    read_len, rc_half, n_rate_ppm, (uint8_t*)d_out));
    return AIX_OK;
}
