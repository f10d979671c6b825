// aix_positions.hip — A1/A2 rows: the positions index ("aindex") of a reads buffer.
//   A1 AIndexCompressed ctor   src/hash.hpp:365-399      indices = exclusive prefix sum of tf
//   A2 lu_compressed_worker    src/hash.cpp:960-1060     positions[indices[h] + slot] = offset + 1, slot < tf[h]
//
// The reference assigns slots with fetch_add in thread-arrival order (ascending offsets with one thread; SURVEY
// §8a-A2). Here every window's bucket is computed in parallel, then a STABLE radix sort by bucket (rocPRIM) of the
// window offsets (a counting iterator, i.e. already ascending) yields each bucket's offsets in ascending order —
// exactly the 1-thread reference result, deterministically — and the first tf[h] of them are placed.
#include <algorithm>
#include <cstring>

#include "aix_env.hpp"
#include "aix_hostkit.hpp"
#include "aix_ingest.hpp"

namespace aix {

static constexpr int kB = kFlatBlock;                             // the grid of the kernels here: flat_grid (aix_hostkit.hpp)

// any byte of x (restricted to `mask` bytes) equal to c ?
__device__ __forceinline__ bool has_byte(uint64_t x, uint8_t c, uint64_t mask) {
    const uint64_t z = (x ^ (0x0101010101010101ULL * c)) | ~mask;
    return (((z - 0x0101010101010101ULL) & ~z) & 0x8080808080808080ULL) != 0;
}

__global__ void __launch_bounds__(kB) k_tf_u64(const IndexDev ix, uint64_t n, uint64_t* __restrict__ tf64) {
    const uint64_t stride = (uint64_t)gridDim.x * kB;
    for (uint64_t i = (uint64_t)blockIdx.x * kB + threadIdx.x; i <= n; i += stride) tf64[i] = i < n ? (uint64_t)key_at(ix, i).tf : 0ull;
}

// bucket of every window (key = n for "no bucket"): hash.cpp:1004-1052. Wave-uniform loop: the verification-table probe is
// wave-cooperative (aix_device.hpp: bucket_probe_wave); a forward-strand window with bytes outside ACGT hashes its RAW bytes
// (:1032-1040), which the table cannot answer, and goes through the MPHF.
template <int LPP>
__global__ void __launch_bounds__(kB) k_a2_probe(const IndexDev ix, const uint8_t* __restrict__ buf, uint64_t nwin, uint64_t start, uint32_t* __restrict__ keys) {
    const uint64_t stride = (uint64_t)gridDim.x * kB;
    const uint64_t FULL = ~0ULL, LAST7 = 0x00FFFFFFFFFFFFFFULL;
    for (uint64_t base = (uint64_t)blockIdx.x * kB + (threadIdx.x & ~63u); base < nwin; base += stride) {
        const uint64_t i = base + (threadIdx.x & 63u);
        const bool in = i < nwin;
        uint32_t key = (uint32_t)ix.n;
        uint64_t w0 = 0, w1 = 0, w2 = 0;
        bool probe = false;
        if (in && i >= start) {
            load23(buf + i, w0, w1, w2);
            const bool skip = has_byte(w0, '\n', FULL) || has_byte(w1, '\n', FULL) || has_byte(w2, '\n', LAST7) ||
                              has_byte(w0, '~', FULL) || has_byte(w1, '~', FULL) || has_byte(w2, '~', LAST7) ||
                              has_byte(w0, 'N', FULL) || has_byte(w1, 'N', FULL) || has_byte(w2, 'N', LAST7);      // :1006-1011
            probe = !skip;
        }
        const Enc23 e = encode23_words(w0, w1, w2);                            // get_dna23_bitset: non-ACGT -> 0
        const uint64_t r = revcomp(e.code, 23);
        const bool fwd = e.code <= r;                                           // :1032: probe the numerically smaller strand only
        const uint64_t want = fwd ? e.code : r;
        uint64_t x0 = w0, x1 = w1, x2 = w2;                                     // forward: the raw bytes of the window
        if (!fwd) ascii23_of_rc(e.code, x0, x1, x2);
        const bool tab = probe && (e.valid || !fwd);                            // the hashed bytes are the ASCII of `want`
        const bool rest = probe;
        uint64_t a = 0, b = 0, c = 0;
        if (rest) jenkins23(x0, x1, x2, ix.m.seed, a, b, c);
        bool mphf = rest;
        if (ix.bk) {
            const bool use = rest && tab;
            const BkRes k = bucket_probe_wave<LPP>(ix.bk, ix.nb, use, a, want);
            if (use) {
                if (k.found) key = k.slot;
                mphf = !k.found && k.overflow;
            }
        }
        if (mphf) {
            const uint64_t h = mphf_from_hash(ix.m, a, b, c);
            if (h < ix.n && key_at(ix, h).code == want) key = (uint32_t)h;
        }
        if (in) keys[i] = key;
    }
}

__global__ void __launch_bounds__(kB) k_a2_first(const uint32_t* __restrict__ skeys, uint64_t nwin, uint32_t n, uint32_t* __restrict__ first) {
    const uint64_t stride = (uint64_t)gridDim.x * kB;
    for (uint64_t j = (uint64_t)blockIdx.x * kB + threadIdx.x; j < nwin; j += stride) {
        const uint32_t h = skeys[j];
        if (h < n && (j == 0 || skeys[j - 1] != h)) first[h] = (uint32_t)j;
    }
}
// `filled[h]` = occurrences of bucket h in the pieces before this one (the reference's ppositions[h] counter, hash.cpp:1037)
__global__ void __launch_bounds__(kB) k_a2_place(const IndexDev ix, const uint32_t* __restrict__ skeys, const uint32_t* __restrict__ svals, uint64_t nwin,
                                                uint64_t piece_first, const uint32_t* __restrict__ first, const uint32_t* __restrict__ filled,
                                                const uint64_t* __restrict__ indices, uint64_t* __restrict__ positions) {
    const uint64_t stride = (uint64_t)gridDim.x * kB;
    const uint32_t n = (uint32_t)ix.n;

    for (uint64_t j = (uint64_t)blockIdx.x * kB + threadIdx.x; j < nwin; j += stride) {
        const uint32_t h = skeys[j];
        if (h >= n) continue;
        const uint64_t rank = (uint64_t)filled[h] + (j - first[h]);
        const uint64_t base = indices[h], tf = indices[h + 1] - base;                             // tf[h] (13-mer: the u64 table of count_kmers13) from its prefix sums
        if (rank < tf) positions[base + rank] = piece_first + svals[j] + 1;                       // :1037-1040 / compute_aindex13.cpp:205-211, 1-based offsets
    }
}
// 13-mer probe (compute_aindex13.cpp:163-204): a window counts iff its 13 bytes are upper-case A/C/G/T; forward strand only;
// bucket = mphf(window) = perm13[code] (the MPHF over all 13-mers, tabulated at open)
__global__ void __launch_bounds__(kB) k_a2_probe13(const uint32_t* __restrict__ perm13, const uint8_t* __restrict__ buf, uint64_t nwin, uint64_t start,
                                                  uint32_t* __restrict__ keys) {
    const uint64_t stride = (uint64_t)gridDim.x * kB;
    for (uint64_t i = (uint64_t)blockIdx.x * kB + threadIdx.x; i < nwin; i += stride) {
        uint32_t key = 67108864u;
        if (i >= start) {
            uint64_t w0, w1;
            load13(buf + i, w0, w1);
            const Enc13 e = encode13_words(w0, w1);
            if (e.valid) { const uint32_t h = perm13[e.code]; if (h < 67108864u) key = h; }
        }
        keys[i] = key;
    }
}
__global__ void __launch_bounds__(kB) k_tf13_copy(const uint64_t* __restrict__ tf, uint64_t n, uint64_t* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * kB;
    for (uint64_t i = (uint64_t)blockIdx.x * kB + threadIdx.x; i <= n; i += stride) out[i] = i < n ? tf[i] : 0ull;
}
// after a piece has been placed: filled[h] += occurrences of h in the piece (saturating). The counters are u32: for 23-mers tf is 32 bits
// (.tf.bin), so a saturated counter can never admit another offset; a 13-mer table is u64, and positions_fill REFUSES a table with an entry
// above 2^32 - 1 (hipErrorNotSupported -> AIX_ERR_UNSUPPORTED) instead of letting a saturated counter overwrite earlier slots.
// One writer per bucket: the lane that holds the last element of h's run.
__global__ void __launch_bounds__(kB) k_tf13_above_u32(const uint64_t* __restrict__ tf, uint64_t n, uint32_t* __restrict__ flag) {
    const uint64_t stride = (uint64_t)gridDim.x * kB;
    bool any = false;
    for (uint64_t i = (uint64_t)blockIdx.x * kB + threadIdx.x; i < n; i += stride) any |= (tf[i] >> 32) != 0;
    if (any) *flag = 1u;
}
__global__ void __launch_bounds__(kB) k_a2_advance(const uint32_t* __restrict__ skeys, uint64_t nwin, uint32_t n, const uint32_t* __restrict__ first,
                                                  uint32_t* __restrict__ filled) {
    const uint64_t stride = (uint64_t)gridDim.x * kB;
    for (uint64_t j = (uint64_t)blockIdx.x * kB + threadIdx.x; j < nwin; j += stride) {
        const uint32_t h = skeys[j];
        if (h >= n || (j + 1 < nwin && skeys[j + 1] == h)) continue;
        const uint64_t tot = (uint64_t)filled[h] + (j - first[h] + 1);
        filled[h] = tot > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)tot;
    }
}

// occurrences per bucket (u64, += ): the shard-local part of the reference's ppositions[h] counters
__global__ void __launch_bounds__(kB) k_a2_tally(const uint32_t* __restrict__ keys, uint64_t nwin, uint32_t n, unsigned long long* __restrict__ counts) {
    const uint64_t stride = (uint64_t)gridDim.x * kB;
    for (uint64_t i = (uint64_t)blockIdx.x * kB + threadIdx.x; i < nwin; i += stride) {
        const uint32_t h = keys[i];
        if (h < n) atomicAdd(&counts[h], 1ull);
    }
}

static hipError_t launch_a2_probe(const IndexDev& ix, const uint8_t* d_reads, uint64_t nwin, uint64_t start, uint32_t* keys, hipStream_t s) {
    if (ix.k == 13) hipLaunchKernelGGL(k_a2_probe13, dim3(flat_grid(nwin)), dim3(kB), 0, s, ix.perm13, d_reads, nwin, start, keys);
    else {
        // lanes that share one bucket line (IndexDev::bk_lpp; the ABI hands in 2 unless the caller chose a width: like count23's slot probe,
        // nothing but a 4-byte slot leaves this kernel, and two lanes per line measured 28.5-29.9 against 29.6-30.7 ms per 5 M reads with eight,
        // three alternating repetitions on one box). AIX_A2_PROBE_LANES: A/B switch
        static const int forced = [] { const long v = env_int("AIX_A2_PROBE_LANES", 2, 8, 0); return v == 2 || v == 4 || v == 8 ? (int)v : 0; }();
        const int lanes = forced ? forced : (int)ix.bk_lpp;
        if (lanes == 2) hipLaunchKernelGGL(k_a2_probe<2>, dim3(flat_grid(nwin)), dim3(kB), 0, s, ix, d_reads, nwin, start, keys);
        else if (lanes == 4) hipLaunchKernelGGL(k_a2_probe<4>, dim3(flat_grid(nwin)), dim3(kB), 0, s, ix, d_reads, nwin, start, keys);
        else hipLaunchKernelGGL(k_a2_probe<8>, dim3(flat_grid(nwin)), dim3(kB), 0, s, ix, d_reads, nwin, start, keys);
    }
    return hipGetLastError();
}

hipError_t exclusive_scan_u32(const uint32_t* d_in, uint32_t* d_out, uint64_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    DevArr tmp(s);
    AIX_TRY(with_temp(tmp, [&](void* t, size_t& tb) { return rocprim::exclusive_scan(t, tb, d_in, d_out, 0u, (size_t)n, rocprim::plus<uint32_t>(), s); }));
    return hipStreamSynchronize(s);
}

// indices (device, n+1 entries); synchronises the stream
hipError_t positions_indices(const IndexDev& ix, uint64_t* d_indices, hipStream_t s) {
    const uint64_t n = ix.n;
    DevArr tf64(s), tmp(s);
    AIX_TRY(tf64.alloc(8 * (n + 1)));
    if (ix.k == 13) AIX_TRY_LAUNCH(k_tf13_copy, dim3(flat_grid(n + 1)), dim3(kB), 0, s, ix.tf13_mphf, n, (uint64_t*)tf64.p);   // compute_aindex13.cpp:57-63
    else AIX_TRY_LAUNCH(k_tf_u64, dim3(flat_grid(n + 1)), dim3(kB), 0, s, ix, n, (uint64_t*)tf64.p);
    AIX_TRY(scan_u64((uint64_t*)tf64.p, d_indices, n + 1, tmp, s));
    return hipStreamSynchronize(s);
}

// positions (device, pre-zeroed, indices[n] entries) for a reads buffer in HBM. Windows are indexed with 32 bits inside a
// piece; longer buffers go piece by piece in ascending order, the per-bucket fill counters carried from piece to piece, which
// keeps every bucket's offsets ascending (the reference's 1-thread order) for any buffer length.
// d_counts (device, u64[n], pre-zeroed): how often every bucket occurs in the buffer under A2's window rules
hipError_t positions_bucket_counts(const IndexDev& ix, const uint8_t* d_reads, uint64_t len, uint64_t start, unsigned long long* d_counts, hipStream_t s) {
    if (len < ix.k || ix.n == 0) return hipSuccess;
    const uint64_t nwin_all = len - (ix.k - 1);
    const uint64_t pw = std::min<uint64_t>(1ull << 30, nwin_all);
    DevArr keys(s);
    AIX_TRY(keys.alloc(4 * pw));
    for (uint64_t w0 = 0; w0 < nwin_all; w0 += pw) {
        const uint64_t nwin = std::min(pw, nwin_all - w0);
        AIX_TRY(launch_a2_probe(ix, d_reads + w0, nwin, start > w0 ? start - w0 : 0, (uint32_t*)keys.p, s));
        AIX_TRY_LAUNCH(k_a2_tally, dim3(flat_grid(nwin)), dim3(kB), 0, s, (uint32_t*)keys.p, nwin, (uint32_t)ix.n, d_counts);
    }
    return hipStreamSynchronize(s);
}

// filled_init (device, u32[n], may be null = zeros): occurrences of every bucket in the shards BEFORE this buffer;
// base_offset: byte offset of this buffer inside the whole reads file (offsets are reported file-relative).
hipError_t positions_fill(const IndexDev& ix, const uint8_t* d_reads, uint64_t len, uint64_t start, const uint64_t* d_indices, uint64_t* d_positions,
                          uint64_t piece, const uint32_t* filled_init, uint64_t base_offset, hipStream_t s, uint32_t* backend_out) {
    if (backend_out) *backend_out = 0;
    if (len < ix.k || ix.n == 0) return hipSuccess;
    const uint64_t nwin_all = len - (ix.k - 1);
    if (piece == 0 || piece > (1ull << 31)) piece = 1ull << 30;
    const uint64_t pw = std::min(piece, nwin_all);
    if (ix.k == 13) {                                                           // the fill counters are 32 bits wide (see k_a2_advance)
        DevArr d_flag(s);
        uint32_t flag = 0;
        AIX_TRY(d_flag.alloc(4));
        AIX_TRY(hipMemsetAsync(d_flag.p, 0, 4, s));
        AIX_TRY_LAUNCH(k_tf13_above_u32, dim3(flat_grid(ix.n)), dim3(kB), 0, s, ix.tf13_mphf, ix.n, (uint32_t*)d_flag.p);
        AIX_TRY(hipMemcpyAsync(&flag, d_flag.p, 4, hipMemcpyDeviceToHost, s));
        AIX_TRY(hipStreamSynchronize(s));
        if (flag) return hipErrorNotSupported;
    }
    DevArr keys_b(s), filled_b(s), skeys_b(s), svals_b(s), first_b(s), tmp(s);
    AIX_TRY(keys_b.alloc(4 * pw));
    AIX_TRY(filled_b.alloc(4 * ix.n));
    uint32_t *keys = (uint32_t*)keys_b.p, *filled = (uint32_t*)filled_b.p, *skeys = nullptr, *svals = nullptr, *first = nullptr;
    AIX_TRY(filled_init ? hipMemcpyAsync(filled, filled_init, 4 * ix.n, hipMemcpyDeviceToDevice, s) : hipMemsetAsync(filled, 0, 4 * ix.n, s));
    unsigned end_bit = 1;
    while (end_bit < 32 && (ix.n >> end_bit)) ++end_bit;                        // keys are in [0, n]
    size_t tmp_bytes = 0;
    rocprim::counting_iterator<uint32_t> iota(0);
    for (uint64_t w0 = 0; w0 < nwin_all; w0 += pw) {
        const uint64_t nwin = std::min(pw, nwin_all - w0);
        const uint64_t rel_start = start > w0 ? start - w0 : 0;               // windows before `start` get no bucket (hash.cpp:973-986)
        const bool more = w0 + pw < nwin_all;
        AIX_TRY(launch_a2_probe(ix, d_reads + w0, nwin, rel_start, keys, s));
        if (a2_msd_eligible(nwin, ix.n)) {                                      // grouping by MSD partition + per-bucket LDS stage (aix_a2msd.hip)
            bool untouched = false;
            const hipError_t e = a2_msd_place(ix, keys, nwin, base_offset + w0, filled, more, d_indices, d_positions, s, &untouched);
            if (e == hipSuccess) { if (backend_out) *backend_out |= 2u; continue; }
            if (!untouched) return e;
            (void)hipGetLastError();                                            // its workspace (16 B per window + chunk slack) did not fit: nothing was written,
        }                                                                       // the sort path below needs about half of that
        if (backend_out) *backend_out |= 1u;
        if (!skeys) {                                                           // short buffers: one stable radix sort of (bucket, offset)
            AIX_TRY(skeys_b.alloc(4 * pw));
            AIX_TRY(svals_b.alloc(4 * pw));
            AIX_TRY(first_b.alloc(4 * ix.n));
            skeys = (uint32_t*)skeys_b.p; svals = (uint32_t*)svals_b.p; first = (uint32_t*)first_b.p;
            // the temporary is sized once, for pw >= nwin elements, and held across the pieces: no piece waits for the one before it
            AIX_TRY(rocprim::radix_sort_pairs(nullptr, tmp_bytes, keys, skeys, iota, svals, (size_t)pw, 0u, end_bit, s));
            AIX_TRY(tmp.alloc(tmp_bytes));
        }
        size_t tb = tmp_bytes;
        AIX_TRY(rocprim::radix_sort_pairs(tmp.p, tb, keys, skeys, iota, svals, (size_t)nwin, 0u, end_bit, s));
        AIX_TRY_LAUNCH(k_a2_first, dim3(flat_grid(nwin)), dim3(kB), 0, s, skeys, nwin, (uint32_t)ix.n, first);
        AIX_TRY_LAUNCH(k_a2_place, dim3(flat_grid(nwin)), dim3(kB), 0, s, ix, skeys, svals, nwin, base_offset + w0, first, filled, d_indices, d_positions);
        if (more) AIX_TRY_LAUNCH(k_a2_advance, dim3(flat_grid(nwin)), dim3(kB), 0, s, skeys, nwin, (uint32_t)ix.n, first, filled);
    }
    return hipStreamSynchronize(s);
}
}  // namespace aix

// ---------------------------------------------------------------------------------------------
// A1/A2: the entry points of the positions index. The host-pointer ones stage through HBM, run the same launch code and copy back.
// ---------------------------------------------------------------------------------------------
// host buffer -> HBM through the pinned, multi-threaded staging pipeline (aix_ingest.hip); returns when the bytes are on the device
static int upload_host(const char* buf, uint64_t len, uint8_t* d_dst, int device) {
    if (len == 0) return AIX_OK;
    ByteSource src;
    src.set_memory(buf, len);
    const int st = upload_pipelined(src, d_dst, device, 0);
    if (st) return st;
    HIPCHK(hipStreamSynchronize(0));
    return AIX_OK;
}

// positions_fill refuses a 13-mer tf table with an entry above 2^32 - 1 (32-bit fill counters, aix_positions.hip): that is a status, not a HIP failure
#define POSCHK(expr)                                                                                                                     \
    do {                                                                                                                                 \
        hipError_t _e = (expr);                                                                                                          \
        if (_e == hipErrorNotSupported) { (void)hipGetLastError(); set_last_error("positions: a 13-mer tf above 2^32 - 1"); return AIX_ERR_UNSUPPORTED; } \
        if (_e != hipSuccess) { set_last_error(std::string(#expr) + ": " + hipGetErrorString(_e)); return AIX_ERR_HIP; }                  \
    } while (0)

// first window the reference's single worker looks at (hash.cpp:973-986): the start is pushed past any
// '\n', '~' or '?' found in the first k bytes, repeatedly
static uint64_t a2_start(const char* c, uint64_t len, uint64_t k = 23) {
    if (len < k) return 0;
    uint64_t start = 0;
    const uint64_t end = len;
    while (start < end - k + 1) {
        bool found = false;
        for (uint64_t i = start; i < start + k; ++i)
            if (c[i] == '\n' || c[i] == '~' || c[i] == '?') { start = i + 1; found = true; break; }
        if (!found) break;
    }
    return start;
}

// the one call of positions_fill behind the four fill entry points: slot-stream lanes, AIX_POSITIONS_PIECE (test hook, read per call:
// exercises the piece logic at small sizes), the back end recorded for aix_index_info
static int fill_positions(aix_index* h, const void* d_reads, uint64_t len, uint64_t start, const void* d_indices, void* d_positions, const void* d_filled_init,
                          uint64_t base_offset, hipStream_t s) {
    POSCHK(positions_fill(h->dev_slots(), (const uint8_t*)d_reads, len, start, (const uint64_t*)d_indices, (uint64_t*)d_positions, env_positions_piece(),
                          (const uint32_t*)d_filled_init, base_offset, s, &h->a2_backend));
    return AIX_OK;
}

extern "C" int aix_positions_fill(aix_index_t* h, const char* reads, uint64_t len, uint64_t* indices_out, uint64_t* positions_out, uint64_t positions_cap,
                                  uint64_t* total_out) {
    if (!h || !indices_out || (len && !reads)) return AIX_ERR_ARG;
    DevGuard g(h->device);
    const uint64_t n = h->n;
    DevBuf dind;
    HIPCHK(dind.alloc(8 * (n + 1)));
    if (n) HIPCHK(positions_indices(h->dev(), (uint64_t*)dind.p, 0));
    else HIPCHK(hipMemset(dind.p, 0, 8));
    { const int ds = download_to_host(indices_out, dind.p, 8 * (n + 1), 0); if (ds) return ds; }
    const uint64_t total = indices_out[n];
    if (total_out) *total_out = total;
    if (!positions_out) return AIX_OK;
    if (positions_cap < total) return AIX_ERR_ARG;
    if (total == 0) return AIX_OK;
    DevBuf dreads, dpos;
    HIPCHK(dreads.alloc(len + 8));
    HIPCHK(dpos.alloc(8 * total));
    HIPCHK(hipMemsetAsync(dpos.p, 0, 8 * total, 0));
    { const int us = upload_host(reads, len, (uint8_t*)dreads.p, h->device); if (us) return us; }
    { const int fs = fill_positions(h, dreads.p, len, a2_start(reads, len, h->k), dind.p, dpos.p, nullptr, 0, 0); if (fs) return fs; }
    return download_to_host(positions_out, dpos.p, 8 * total, 0);
}

// device-resident twin: reads already in HBM, indices (n+1) and positions (indices[n], caller-sized through
// aix_positions_total) written in HBM. `start` = aix_positions_start of the buffer's head (the caller holds the bytes).
extern "C" int aix_positions_total(aix_index_t* h, uint64_t* total_out) {
    if (!h || !total_out) return AIX_ERR_ARG;
    DevGuard g(h->device);
    *total_out = 0;
    if (h->n == 0) return AIX_OK;
    if (h->pos_total_known) { *total_out = h->pos_total; return AIX_OK; }       // sum of tf[]: fixed for the life of a 23-mer handle, reset by aix_index_set_tf_13
    DevBuf dind;
    HIPCHK(dind.alloc(8 * (h->n + 1)));
    HIPCHK(positions_indices(h->dev(), (uint64_t*)dind.p, 0));
    HIPCHK(hipMemcpy(total_out, (const uint64_t*)dind.p + h->n, 8, hipMemcpyDeviceToHost));
    h->pos_total = *total_out;
    h->pos_total_known = true;
    return AIX_OK;
}

extern "C" int aix_positions_fill_dev(aix_index_t* h, const char* d_reads, uint64_t len, uint64_t start, uint64_t* d_indices_out, uint64_t* d_positions_out,
                                      uint64_t positions_cap, void* stream) {
    if (!h || !d_indices_out || (len && !d_reads)) return AIX_ERR_ARG;
    DevGuard g(h->device);
    hipStream_t s = (hipStream_t)stream;
    const uint64_t n = h->n;
    if (n) HIPCHK(positions_indices(h->dev(), d_indices_out, s));           // synchronises the stream
    else HIPCHK(hipMemsetAsync(d_indices_out, 0, 8, s));
    if (n == 0) return AIX_OK;
    uint64_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, d_indices_out + n, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (total == 0) return AIX_OK;
    if (!d_positions_out || positions_cap < total) return AIX_ERR_ARG;
    HIPCHK(hipMemsetAsync(d_positions_out, 0, 8 * total, s));
    return fill_positions(h, d_reads, len, start, d_indices_out, d_positions_out, nullptr, 0, s);
}

extern "C" int aix_positions_start(const char* reads, uint64_t len, uint64_t* start_out) {
    if (!start_out || (len && !reads)) return AIX_ERR_ARG;
    *start_out = a2_start(reads, len);
    return AIX_OK;
}
extern "C" int aix_positions_start_k(const char* reads, uint64_t len, int k, uint64_t* start_out) {
    if (!start_out || (len && !reads) || (k != 13 && k != 23)) return AIX_ERR_ARG;
    *start_out = a2_start(reads, len, (uint64_t)k);
    return AIX_OK;
}

// A2 over shards of the reads file (multi-GPU): tally, then fill with the counters of the earlier shards
extern "C" int aix_positions_bucket_counts(aix_index_t* h, const char* reads, uint64_t len, int first_shard, uint64_t* counts_out) {
    if (!h || !counts_out || (len && !reads)) return AIX_ERR_ARG;
    DevGuard g(h->device);
    const uint64_t n = h->n;
    if (n == 0) return AIX_OK;
    DevBuf dreads, dcnt;
    HIPCHK(dreads.alloc(len + 8));
    HIPCHK(dcnt.alloc(8 * n));
    { const int us = upload_host(reads, len, (uint8_t*)dreads.p, h->device); if (us) return us; }
    HIPCHK(hipMemset(dcnt.p, 0, 8 * n));
    HIPCHK(positions_bucket_counts(h->dev_slots(), (const uint8_t*)dreads.p, len, first_shard ? a2_start(reads, len, h->k) : 0, (unsigned long long*)dcnt.p, 0));
    return download_to_host(counts_out, dcnt.p, 8 * n, 0);
}

extern "C" int aix_positions_fill_shard(aix_index_t* h, const char* reads, uint64_t len, int first_shard, uint64_t base_offset, const uint32_t* filled_init,
                                        uint64_t* positions_out, uint64_t positions_cap) {
    if (!h || !positions_out || (len && !reads)) return AIX_ERR_ARG;
    DevGuard g(h->device);
    const uint64_t n = h->n;
    if (n == 0) return AIX_OK;
    DevBuf dind, dreads, dpos, dfill;
    HIPCHK(dind.alloc(8 * (n + 1)));
    HIPCHK(positions_indices(h->dev(), (uint64_t*)dind.p, 0));
    uint64_t total = 0;
    HIPCHK(hipMemcpy(&total, (const uint64_t*)dind.p + n, 8, hipMemcpyDeviceToHost));
    if (positions_cap < total) return AIX_ERR_ARG;
    if (total == 0) return AIX_OK;
    HIPCHK(dreads.alloc(len + 8));
    HIPCHK(dpos.alloc(8 * total));
    if (filled_init) {
        HIPCHK(dfill.alloc(4 * n));
        HIPCHK(hipMemcpy(dfill.p, filled_init, 4 * n, hipMemcpyHostToDevice));
    }
    { const int us = upload_host(reads, len, (uint8_t*)dreads.p, h->device); if (us) return us; }
    HIPCHK(hipMemset(dpos.p, 0, 8 * total));
    { const int fs = fill_positions(h, dreads.p, len, first_shard ? a2_start(reads, len, h->k) : 0, dind.p, dpos.p, filled_init ? dfill.p : nullptr, base_offset, 0); if (fs) return fs; }
    return download_to_host(positions_out, dpos.p, 8 * total, 0);
}

// device-resident twins of the shard entry points (multi-GPU): a rank's share is already in HBM, the partial results stay in
// HBM for the collectives (RCCL), nothing crosses PCIe
extern "C" int aix_positions_indices_dev(aix_index_t* h, uint64_t* d_indices_out, void* stream) {
    if (!h || !d_indices_out) return AIX_ERR_ARG;
    DevGuard g(h->device);
    if (h->n == 0) { HIPCHK(hipMemsetAsync(d_indices_out, 0, 8, (hipStream_t)stream)); return AIX_OK; }
    HIPCHK(positions_indices(h->dev(), d_indices_out, (hipStream_t)stream));
    return AIX_OK;
}

extern "C" int aix_positions_bucket_counts_dev(aix_index_t* h, const char* d_reads, uint64_t len, uint64_t start, uint64_t* d_counts_out, void* stream) {
    if (!h || !d_counts_out || (len && !d_reads)) return AIX_ERR_ARG;
    DevGuard g(h->device);
    if (h->n == 0) return AIX_OK;
    HIPCHK(hipMemsetAsync(d_counts_out, 0, 8 * h->n, (hipStream_t)stream));
    HIPCHK(positions_bucket_counts(h->dev_slots(), (const uint8_t*)d_reads, len, start, (unsigned long long*)d_counts_out, (hipStream_t)stream));
    return AIX_OK;
}

extern "C" int aix_positions_fill_shard_dev(aix_index_t* h, const char* d_reads, uint64_t len, uint64_t start, uint64_t base_offset, const uint32_t* d_filled_init,
                                            const uint64_t* d_indices, uint64_t* d_positions, void* stream) {
    if (!h || !d_indices || !d_positions || (len && !d_reads)) return AIX_ERR_ARG;
    DevGuard g(h->device);
    if (h->n == 0) return AIX_OK;
    return fill_positions(h, d_reads, len, start, d_indices, d_positions, d_filled_init, base_offset, (hipStream_t)stream);
}
