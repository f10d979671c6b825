// aix_count.hip — the counters' device-pointer entry points: K13 in steps (also driven part by part from aix_ingest.hip) and count23 with
// its three back ends, on the handle's grow-only count workspace. No kernel lives here (aix_count13.hip, aix_kernels.hip, aix_stream23.hip).
#include <algorithm>
#include <mutex>
#include <string>

#include "aix_env.hpp"
#include "aix_handle.hpp"

// What both counters share; every function here is called with h->count_mutex held.
// the scratch table / workspace belong to the handle: counting calls are ordered behind one another even when they come in on
// different streams (the mutex only orders the enqueueing). The caller records h->count_done on `s` when it is through.
static int order_behind_last_count(aix_index* h, hipStream_t s) {
    if (h->count_done) HIPCHK(hipStreamWaitEvent(s, h->count_done, 0));
    else HIPCHK(hipEventCreateWithFlags(&h->count_done, hipEventDisableTiming));
    return AIX_OK;
}

// grow-only per-handle workspace of the counting paths (13-mer partitions; 23-mer slot stream + partitions)
static int ensure_count_workspace(aix_index* h, uint64_t need, hipStream_t s) {
    if (need <= h->count_ws_bytes) return AIX_OK;
    HIPCHK(hipStreamSynchronize(s));
    if (h->count_ws) { (void)hipFree(h->count_ws); h->device_bytes -= h->count_ws_bytes; h->count_ws = nullptr; h->count_ws_bytes = 0; }
    // AIX_COUNT_TEST_WORKSPACE_MAX: test hook, requests above this many bytes "do not fit"
    const hipError_t e = need > env_u64("AIX_COUNT_TEST_WORKSPACE_MAX", 0, ~0ull, ~0ull) ? hipErrorOutOfMemory : hipMalloc(&h->count_ws, need);
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();                                               // the failed request is not a sticky error
        h->count_ws = nullptr;
        set_last_error("count workspace of " + std::to_string(need) + " bytes does not fit in device memory");
        return AIX_ERR_NOMEM;
    }
    HIPCHK(e);
    h->count_ws_bytes = need;
    h->device_bytes += need;
    return AIX_OK;
}

// Buffers are counted in pieces of at most *piece windows, and the workspace grows with the piece (bytes_for(windows)): one that does not
// fit halves the piece instead of failing the call, down to 4096 windows. On AIX_OK *piece is the piece to use (at most nwin).
template <typename F>
static int fit_count_workspace(aix_index* h, uint64_t nwin, uint64_t* piece, hipStream_t s, F&& bytes_for) {
    for (;;) {
        const uint64_t pw = std::min(nwin, *piece);
        const int st = ensure_count_workspace(h, bytes_for(pw), s);
        if (st == AIX_OK) { *piece = pw; return AIX_OK; }
        if (st != AIX_ERR_NOMEM || pw <= 4096) return st;
        *piece = pw / 2;
    }
}

// Word 0 of the workspace is the partition kernels' error word (zeroed by the caller before the first launch): a chunk id outside a
// workgroup's region would have dropped counts, so the kernels raise it instead of staying silent and the call fails (costs one stream
// wait per call; the table is complete when this returns).
static int check_chunk_regions(aix_index* h, const char* who, hipStream_t s) {
    uint32_t dropped = 0;
    HIPCHK(hipMemcpyAsync(&dropped, h->count_ws, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (dropped) { set_last_error(std::string(who) + ": chunk region exhausted (partition workspace undersized)"); return AIX_ERR_UNSUPPORTED; }
    return AIX_OK;
}

// K13 in three steps, so that a file can be counted part by part (aix_ingest.hip) as well as in one call: begin() orders the call behind
// the previous user of the handle's workspace and zeroes the output, add() counts one PLAIN buffer into it (any number of times; every
// window of the concatenated stream must lie inside exactly one of the buffers), end() finishes the table. The caller holds count_mutex
// from begin to end.
int count13_begin_locked(aix_index* h, uint64_t* d_tf_out, hipStream_t s) {
    { const int st = order_behind_last_count(h, s); if (st) return st; }
    h->c13_atomics = env_flag("AIX_COUNT13_ATOMICS") || !h->perm13_bijective;   // env: A/B switch for measurements / tests
    h->c13_added = false;
    if (h->c13_atomics) {
        if (!h->scratch13) {
            HIPCHK(hipMalloc((void**)&h->scratch13, 8 * AIX_TOTAL_13MERS));
            h->device_bytes += 8 * AIX_TOTAL_13MERS;
        }
        HIPCHK(hipMemsetAsync(h->scratch13, 0, 8 * AIX_TOTAL_13MERS, s));
    }
    HIPCHK(hipMemsetAsync(d_tf_out, 0, 8 * AIX_TOTAL_13MERS, s));
    return AIX_OK;
}

int count13_add_locked(aix_index* h, const char* d_plain, uint64_t len, uint64_t* d_tf_out, hipStream_t s) {
    if (h->c13_atomics) {
        // scattered u64 memory-side atomics into the code-ordered table (slower; kept as the independent cross-check)
        HIPCHK(launch_count13_plain((const uint8_t*)d_plain, len, h->scratch13, s));
        h->c13_added = true;
        return AIX_OK;
    }
    // The partitioned path indexes windows and chunks with 32 bits: buffers are cut into pieces of at most `piece` (2^31) window starts.
    // A window belongs to the piece that holds its first byte; a piece is handed its 12 following bytes as well, so the
    // cut needs no record boundary and every window is counted exactly once. Pieces after the first add to the table.
    uint64_t piece = env_count_piece("AIX_COUNT13_PIECE", 1ull << 31);
    const uint64_t nwin = len >= 13 ? len - 12 : 0;
    if (nwin == 0) return AIX_OK;
    { const int st = fit_count_workspace(h, nwin, &piece, s, [](uint64_t pw) { return count13_workspace_bytes(pw + 12); }); if (st) return st; }
    HIPCHK(hipMemsetAsync(h->count_ws, 0, 4, s));                             // the error word of the workspace
    for (uint64_t first = 0; first < nwin; first += piece) {
        const uint64_t w = std::min(piece, nwin - first);
        HIPCHK(launch_count13_partitioned((const uint8_t*)d_plain + first, w + 12, h->count_ws, nullptr, h->perm13, d_tf_out, h->c13_added ? 1 : 0, s));   // fused permutation
        h->c13_added = true;
    }
    return check_chunk_regions(h, "count13", s);
}

int count13_end_locked(aix_index* h, uint64_t* d_tf_out, hipStream_t s) {
    int st = AIX_OK;
    if (h->c13_atomics) {
        const hipError_t e = launch_scatter13_to_mphf(h->perm13, h->scratch13, d_tf_out, h->perm13_bijective ? 0 : 1, s);
        if (e != hipSuccess) { set_last_error(std::string("count13 scatter: ") + hipGetErrorString(e)); st = AIX_ERR_HIP; }
    }
    (void)hipEventRecord(h->count_done, s);
    return st;
}

extern "C" int aix_count13_dev(aix_index_t* h, const char* d_plain, uint64_t len, uint64_t* d_tf_out, void* stream) {
    if (!h || !d_tf_out || (len && !d_plain)) return AIX_ERR_ARG;
    if (h->k != 13) return AIX_ERR_MODE;
    DevGuard g(h->device);
    std::lock_guard<std::mutex> lk(h->count_mutex);
    hipStream_t s = (hipStream_t)stream;
    int st = count13_begin_locked(h, d_tf_out, s);
    if (st) return st;
    st = count13_add_locked(h, d_plain, len, d_tf_out, s);
    const int st2 = count13_end_locked(h, d_tf_out, s);
    return st ? st : st2;
}

// count23: three back ends, same result. Which one ran is reported by aix_index_info (count23_backend / count23_passes). Back ends 1 and 3
// use nothing of the handle but its tables, so they run outside count_mutex and take it for these two stores only.
static void record_count23(aix_index* h, uint32_t backend, uint32_t passes) {
    std::lock_guard<std::mutex> lk(h->count_mutex);
    h->c23_backend = backend; h->c23_passes = passes;
}

// (1) one memory-side atomic per found window: ~23 G scattered atomics/s on MI355X, which bounds the kernel once a probe costs a single line
static int count23_atomics(aix_index* h, const char* d_plain, uint64_t len, int canon_mode, uint32_t* d_tf_out, hipStream_t s) {
    HIPCHK(launch_count23_fixed(h->dev(), (const uint8_t*)d_plain, len, canon_mode, d_tf_out, s));
    record_count23(h, 1, 0);
    return AIX_OK;
}

// (3) counting the distinct k-mers of the reads first (K1: MSD partition + per-bucket LDS hash, pieces merged) and probing each of them ONCE:
// K1's LDS-bound 21 ps per window beat a 128-byte line per window (24 - 27 ps) as soon as the distinct k-mers — at most n — are few against the
// windows: 34.7 / 69.8 / 138 / 272 ms against 43.0 / 85.7 / 171 / 341 ms at 32 / 64 / 128 / 256 windows per key (5e7 keys, one handle), config 4
// 531 against 617 - 679 ms; the extra probe per distinct k-mer (28 ps) is paid back from ~6 windows per key. Same histogram: every window is
// counted under the same canonical form, skipped for the same bytes, and two distinct k-mers never share a slot.
// AIX_ERR_NOMEM: K1's scratch does not fit, nothing was counted and the caller goes on with (2).
static int count23_via_k1(aix_index* h, const char* d_plain, uint64_t len, int canon_mode, uint32_t* d_tf_out, hipStream_t s) {
    DistinctRun d;
    const hipError_t e = distinct_from_plain((const uint8_t*)d_plain, len, 23, canon_mode, 1, env_distinct_piece(), d, s);
    if (e != hipSuccess) (void)hipGetLastError();
    if (e == hipErrorOutOfMemory) return AIX_ERR_NOMEM;
    if (e != hipSuccess) { set_last_error(std::string("count23 through K1: ") + hipGetErrorString(e)); return AIX_ERR_HIP; }
    const hipError_t e2 = launch_add_counts23(h->dev_slots(), d.k, d.c, d.n, d_tf_out, s);
    const hipError_t e3 = hipStreamSynchronize(s);                             // the K1 result goes back to the block cache idle
    HIPCHK(e2);
    HIPCHK(e3);
    record_count23(h, 3, 0);
    return AIX_OK;
}

// The second stream of (2) and the events both ways, made by the first multi-piece call of a handle (under count_mutex).
// AIX_COUNT23_HIST_CUS=n[,style] (A/B switch, read here): the partition + histogram kernels get n of the 256 CUs and the probe the others,
// through CU-masked streams. The split kernel takes a whole CU (152 KiB of LDS, 16 waves of 128 VGPRs), so on shared CUs the two kernels
// alternate workgroup by workgroup instead of running side by side. style 0: the low n bits of the mask, 1: every (256 / n)-th bit.
static int ensure_count23_streams(aix_index* h) {
    if (h->probe_stream) return AIX_OK;
    int hist_cus = 0, style = 0;
    env_int_pair("AIX_COUNT23_HIST_CUS", &hist_cus, &style);
    if (hist_cus >= 8 && hist_cus <= 224) {
        uint32_t mh[8] = {0, 0, 0, 0, 0, 0, 0, 0}, mp[8];
        const int step = style ? 256 / hist_cus : 1;
        for (int i = 0, c = 0; c < hist_cus && i < 256; i += step, ++c) mh[i >> 5] |= 1u << (i & 31);
        for (int w = 0; w < 8; ++w) mp[w] = ~mh[w];
        HIPCHK(hipExtStreamCreateWithCUMask(&h->probe_stream, 8, mp));
        HIPCHK(hipExtStreamCreateWithCUMask(&h->hist_stream, 8, mh));
    } else {
        HIPCHK(hipStreamCreateWithFlags(&h->probe_stream, hipStreamNonBlocking));
    }
    for (int i = 0; i < 2; ++i) {
        HIPCHK(hipEventCreateWithFlags(&h->probe_ev[i], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&h->hist_ev[i], hipEventDisableTiming));
    }
    HIPCHK(hipEventCreateWithFlags(&h->start_ev, hipEventDisableTiming));
    return AIX_OK;
}

namespace {
struct RecordOnExit {                   // the next counting call may touch the workspace once the caller's stream has reached this point
    hipEvent_t ev; hipStream_t st;
    ~RecordOnExit() { (void)hipEventRecord(ev, st); }
};
// an error in the middle of the piece loop would return with the probe stream still writing into the workspace, and the event recorded on
// exit (caller's stream only) would let the next counting call in under it: a failing call waits for the probe stream first
struct ProbeDrainOnError {
    aix_index* h;
    bool armed = true;
    ~ProbeDrainOnError() { if (armed && h->probe_stream) (void)hipStreamSynchronize(h->probe_stream); if (armed && h->hist_stream) (void)hipStreamSynchronize(h->hist_stream); }
};
}  // namespace

// (2) the slots are streamed out (4 B per window) and added into tf[] by the chunked-partition + LDS histogram of the 13-mer counter: no
// global atomics at all. Handles 2^26 slots per pass over the slot stream (2048 partitions of 32 768 bins; a larger key set takes
// ceil(n / 2^26) passes) and pays a fixed cost, so short buffers keep (1).
static int count23_histogram(aix_index* h, const char* d_plain, uint64_t nwin, int canon_mode, uint32_t* d_tf_out, hipStream_t s) {
    const uint32_t range_bits = (uint32_t)env_int("AIX_COUNT23_TEST_RANGE_BITS", 4, 26, 26);   // test hook, several slot ranges on a small key set
    std::lock_guard<std::mutex> lk(h->count_mutex);
    { const int st = order_behind_last_count(h, s); if (st) return st; }
    RecordOnExit record_on_exit{h->count_done, s};
    // windows per pass. Every pass pays for its chunk directory (sort, clears) and leaves one partly filled 512-byte chunk per (workgroup,
    // partition) pair — up to 2^20 of them — for the histogram kernel to read, so long passes win: 200 M reads in 809 / 788 / 775 / 772 ms with
    // 2^28 / 2^29 / 2^30 / 2^31 windows per pass (same box). 2^30: 4 GiB of slots (twice with the second stream) + ~2.6 GiB of partitions.
    uint64_t pw = env_count_piece("AIX_COUNT23_PIECE", 1ull << 30);
    const IndexDev d = h->dev();
    // More than one piece: the probe of piece i + 1 (HBM lines + hash arithmetic, no LDS) runs on a second stream while piece i is
    // partitioned and added on the caller's stream (LDS-bound, one 152 KiB workgroup per CU) — two slot buffers, one partition
    // workspace, events both ways. AIX_COUNT23_OVERLAP=0 keeps everything on the caller's stream (A/B switch).
    // A workspace that does not fit (2^30 windows: ~10.6 GiB) halves the pass.
    const bool may_overlap = !d.mk && env_bool("AIX_COUNT23_OVERLAP", true);
    uint64_t part_bytes = 0, slot_bytes = 0;
    bool overlap = false;
    { const int st = fit_count_workspace(h, nwin, &pw, s, [&](uint64_t w) {
          part_bytes = (count13_workspace_bytes(w + 12) + 255) / 256 * 256;
          slot_bytes = (4 * w + 255) / 256 * 256;
          overlap = may_overlap && nwin > w;
          return part_bytes + (overlap ? 2 : 1) * slot_bytes;
      }); if (st) return st; }
    uint32_t* slot_buf[2] = {(uint32_t*)((uint8_t*)h->count_ws + part_bytes), (uint32_t*)((uint8_t*)h->count_ws + part_bytes + (overlap ? slot_bytes : 0))};
    ProbeDrainOnError probe_drain{h};
    HIPCHK(hipMemsetAsync(h->count_ws, 0, 4, s));                             // the error word of the partition workspace
    hipStream_t hs = s;
    if (overlap) {
        { const int st = ensure_count23_streams(h); if (st) return st; }
        HIPCHK(hipEventRecord(h->start_ev, s));                                // the reads (and whatever else the caller queued) are ready when the first probe starts
        HIPCHK(hipStreamWaitEvent(h->probe_stream, h->start_ev, 0));
        if (h->hist_stream) { hs = h->hist_stream; HIPCHK(hipStreamWaitEvent(hs, h->start_ev, 0)); }
    }
    // the slot-stream probe of the counter runs best with two lanes per bucket line (38.7-40.4 against 42.5-42.7 ms per 10 M reads with
    // eight, same box): nothing but the 4-byte slot leaves the kernel, so fewer, wider reads per probe win; lookups keep eight
    const IndexDev dc = h->dev_slots();
    // probe kernel of the slot stream: one window per lane (k_probe23_slots) or a run of 16 / 32 windows per lane (k_run23_slots: the bytes are
    // encoded once per run). AIX_COUNT23_RUN=0 / 16 / 32 (A/B switch).
    const long run_env = env_int("AIX_COUNT23_RUN", 16, 32, 0);
    const int run_w = (run_env == 16 || run_env == 32) ? (int)run_env : 0;
    auto probe = [&](const uint8_t* p, uint64_t n, uint32_t* out, hipStream_t st) {
        return (run_w && dc.bk) ? launch_run23_slots(dc, p, n, canon_mode, out, run_w, st) : launch_probe23_slots(dc, p, n, canon_mode, out, st);
    };
    uint64_t ip = 0;
    for (uint64_t first = 0; first < nwin; first += pw, ++ip) {
        const uint64_t w = std::min(pw, nwin - first);
        const int b = overlap ? (int)(ip & 1) : 0;
        if (d.mk) {                                                            // 32 consecutive windows per lane; word 1 of the workspace = "undecided windows" flag
            HIPCHK(hipMemsetAsync((uint32_t*)h->count_ws + 1, 0, 4, s));
            HIPCHK(launch_stream23_slots(d, (const uint8_t*)d_plain + first, w + 22, canon_mode, slot_buf[b], (uint32_t*)h->count_ws + 1, s));
        } else if (overlap) {
            if (ip >= 2) HIPCHK(hipStreamWaitEvent(h->probe_stream, h->hist_ev[b], 0));      // piece ip - 2 has been read out of this buffer
            HIPCHK(probe((const uint8_t*)d_plain + first, w + 22, slot_buf[b], h->probe_stream));
            HIPCHK(hipEventRecord(h->probe_ev[b], h->probe_stream));
            HIPCHK(hipStreamWaitEvent(hs, h->probe_ev[b], 0));
        } else {
            HIPCHK(probe((const uint8_t*)d_plain + first, w + 22, slot_buf[b], s));
        }
        uint32_t passes = 0;
        HIPCHK(launch_histogram_slots(slot_buf[b], w, h->count_ws, d_tf_out, h->n, hs, range_bits, &passes));
        h->c23_backend = 2; h->c23_passes = passes;
        if (overlap) HIPCHK(hipEventRecord(h->hist_ev[b], hs));
    }
    if (hs != s && ip) HIPCHK(hipStreamWaitEvent(s, h->hist_ev[(ip - 1) & 1], 0));
    { const int st = check_chunk_regions(h, "count23", s); if (st) return st; }
    probe_drain.armed = false;                                                 // every probe has been waited for by a histogram on the caller's stream
    return AIX_OK;
}

extern "C" int aix_count23_fixed_dev(aix_index_t* h, const char* d_plain, uint64_t len, int canon_mode, uint32_t* d_tf_out, void* stream) {
    if (!h || !d_tf_out || (len && !d_plain)) return AIX_ERR_ARG;
    if (h->k != 23) return AIX_ERR_MODE;
    if (canon_mode < 0 || canon_mode > 2) return AIX_ERR_ARG;
    DevGuard g(h->device);
    hipStream_t s = (hipStream_t)stream;
    const uint64_t nwin = len >= 23 ? len - 22 : 0;
    if (nwin == 0 || h->n == 0) return AIX_OK;
    // (1) below AIX_COUNT23_HIST_MIN windows (tests run the others on small inputs) or when AIX_COUNT23_ATOMICS is set
    if (nwin < env_u64("AIX_COUNT23_HIST_MIN", 0, ~0ull, 1ull << 22) || env_flag("AIX_COUNT23_ATOMICS")) return count23_atomics(h, d_plain, len, canon_mode, d_tf_out, s);
    // (3) from 8 windows per key and 2^29 windows up (AIX_COUNT23_VIA_K1=0 / 1 forces); if K1's scratch does not fit the call goes on with (2)
    if (env_bool("AIX_COUNT23_VIA_K1", nwin >= (1ull << 29) && nwin / 8 >= h->n)) {
        const int st = count23_via_k1(h, d_plain, len, canon_mode, d_tf_out, s);
        if (st != AIX_ERR_NOMEM) return st;
    }
    return count23_histogram(h, d_plain, nwin, canon_mode, d_tf_out, s);
}
