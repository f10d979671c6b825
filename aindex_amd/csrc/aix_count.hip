// aix_count.hip — the counters' device-pointer entry points: K13 in steps (also driven part by part from aix_ingest.hip) and count23 with
// its three back ends, on the handle's grow-only count workspace. The one-window-per-lane kernels come first; the partitioned counter and
// the run / streaming probes are subsystems of their own (aix_count13.hip, aix_stream23.hip).
#include <algorithm>
#include <mutex>
#include <string>

#include "aix_env.hpp"
#include "aix_handle.hpp"
#include "aix_launch.hpp"
#include "aix_probe.hpp"

namespace aix {

// ---------------------------------------------------------------------------------------------
// counting (PLAIN form: any byte that is not a base breaks the window; '\n' separates sequences)
// ---------------------------------------------------------------------------------------------
// count_kmers13.cpp:113-161: upper-case, ACGT only, forward strand; one lane per window start
__global__ void __launch_bounds__(kBlock) k_count13(const uint8_t* __restrict__ buf, uint64_t len, unsigned long long* __restrict__ table) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    if (len < 13) return;
    const uint64_t nwin = len - 12;
    for (uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x; p < nwin; p += stride) {
        uint64_t w0, w1;
        load13(buf + p, w0, w1);
        w0 &= 0xDFDFDFDFDFDFDFDFULL;                            // toupper for letters; nothing else maps onto ACGT
        w1 &= 0xDFDFDFDFDFDFDFDFULL;
        const Enc13 e = encode13_words(w0, w1);
        if (e.valid) atomicAdd(&table[e.code], 1ULL);
    }
}
// the code-ordered table of k_count13 into the mphf-ordered output.
// ADD: the MPHF is not a bijection on the 13-mers (a foreign .pf): several codes may share a slot, and the reference's
// counts[mphf(window)].fetch_add(1) (count_kmers13.cpp:147-152) then sums them; slots >= 4^13 are skipped as there.
template <bool ADD>
__global__ void __launch_bounds__(kBlock) k_scatter13(const uint32_t* __restrict__ perm, const unsigned long long* __restrict__ table_code, uint64_t* __restrict__ out_mphf) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t code = (uint64_t)blockIdx.x * kBlock + threadIdx.x; code < 67108864ull; code += stride) {
        const uint32_t h = perm[code];
        if (h >= 67108864u) continue;
        if (ADD) { const unsigned long long c = table_code[code]; if (c) atomicAdd((unsigned long long*)&out_mphf[h], c); }
        else out_mphf[h] = table_code[code];
    }
}

template <int LPP>
__global__ void __launch_bounds__(kBlock) k_count23_fixed(const IndexDev ix, const uint8_t* __restrict__ buf, uint64_t len, int canon_mode, uint32_t* __restrict__ tf_out) {
    if (len < 23) return;
    const uint64_t nwin = len - 22;
    IndexDev ixn = ix;
    ixn.bloom = nullptr;          // no absence filter in front of the table: it would be one more read for nearly every window
    ixn.early_exit = 0;           // windows of reads drawn from the indexed genome are mostly hits. With the verification table: one line
                                  // per window; without it (and for the overflow fall-back): the parallel three-read evaluation, whose
                                  // fingerprint (same 16 bytes as the pairs) still spares the key-record read of a window that is NOT a key
    AIX_WAVE_LOOP(p, nwin) {
        const bool in = p < nwin;
        uint64_t w0 = 0, w1 = 0, w2 = 0;
        if (in) load23(buf + p, w0, w1, w2);
        w0 = u_to_t(w0 & 0xDFDFDFDFDFDFDFDFULL);
        w1 = u_to_t(w1 & 0xDFDFDFDFDFDFDFDFULL);
        w2 = u_to_t(w2 & 0x00DFDFDFDFDFDFDFULL);
        const Enc23 e = encode23_words(w0, w1, w2);
        uint64_t key = e.code;
        if (canon_mode == 1) { const uint64_t x = revcomp_refx86(e.code, 23); key = e.code < x ? e.code : x; }
        else if (canon_mode == 2) { const uint64_t x = revcomp(e.code, 23); key = e.code < x ? e.code : x; }
        uint64_t s0, s1, s2;
        ascii23_of_rc(revcomp(key, 23), s0, s1, s2);
        const Probe pr = probe23_wave<LPP>(ixn, in && e.valid, s0, s1, s2, key);
        if (pr.found) atomicAdd(&tf_out[pr.slot], 1u);
    }
}

// count23 without global atomics, front end: the MPHF slot of every window (0xFFFFFFFF: not a key / not a clean window) as a
// coalesced 4-byte stream; aix_count13.hip's chunked-partition + LDS histogram then adds the stream into tf[] (1.3e9 scattered
// memory-side atomics per 10 M reads run at ~23 G/s and were what bounded k_count23_fixed once a probe cost one line).
template <int LPP>
__global__ void __launch_bounds__(kBlock) k_probe23_slots(const IndexDev ix, const uint8_t* __restrict__ buf, uint64_t len, int canon_mode, uint32_t* __restrict__ slots) {
    if (len < 23) return;
    const uint64_t nwin = len - 22;
    IndexDev ixn = ix;
    ixn.bloom = nullptr;
    ixn.early_exit = 0;
    AIX_WAVE_LOOP(p, nwin) {
        const bool in = p < nwin;
        uint64_t w0 = 0, w1 = 0, w2 = 0;
        if (in) load23(buf + p, w0, w1, w2);
        w0 = u_to_t(w0 & 0xDFDFDFDFDFDFDFDFULL);
        w1 = u_to_t(w1 & 0xDFDFDFDFDFDFDFDFULL);
        w2 = u_to_t(w2 & 0x00DFDFDFDFDFDFDFULL);
        const Enc23 e = encode23_words(w0, w1, w2);
        uint64_t key = e.code;
        if (canon_mode == 1) { const uint64_t x = revcomp_refx86(e.code, 23); key = e.code < x ? e.code : x; }
        else if (canon_mode == 2) { const uint64_t x = revcomp(e.code, 23); key = e.code < x ? e.code : x; }
        uint64_t s0, s1, s2;
        ascii23_of_rc(revcomp(key, 23), s0, s1, s2);
        const Probe pr = probe23_wave<LPP>(ixn, in && e.valid, s0, s1, s2, key);
        if (in) slots[p] = pr.found ? (uint32_t)pr.slot : 0xFFFFFFFFu;
    }
}

// count23 through K1: the distinct k-mers of the reads (already in the call's canonical form) with their counts; one probe per DISTINCT k-mer, and a plain
// read-modify-write of its slot — two distinct k-mers never share a slot
template <int LPP>
__global__ void __launch_bounds__(kBlock) k_add_counts23(const IndexDev ix, const uint64_t* __restrict__ keys, const uint64_t* __restrict__ counts, uint64_t n,
                                                        uint32_t* __restrict__ tf_out) {
    IndexDev ixn = ix;
    ixn.bloom = nullptr;
    ixn.early_exit = 0;
    AIX_WAVE_LOOP(i, n) {
        const bool in = i < n;
        const uint64_t key = in ? keys[i] : 0ull;
        uint64_t s0, s1, s2;
        ascii23_of_rc(revcomp(key, 23), s0, s1, s2);
        const Probe pr = probe23_wave<LPP>(ixn, in, s0, s1, s2, key);
        if (in && pr.found) tf_out[pr.slot] += (uint32_t)counts[i];          // u32 histogram: wraps like the per-window adds of the other back ends
    }
}

// the slot stream of a PLAIN buffer, one window per lane: slots[p] for p < len - 22; asynchronous on `s`, returns hipGetLastError()
static hipError_t launch_probe23_slots(const IndexDev& ix, const uint8_t* buf, uint64_t len, int canon_mode, uint32_t* slots, hipStream_t s) {
    if (len < 23 || ix.n == 0) return hipSuccess;
    // AIX_PROBE_LDS_PAD=bytes (experiment): unused dynamic LDS per workgroup, to run the probe at a chosen number of waves per CU
    static const unsigned pad = (unsigned)env_int("AIX_PROBE_LDS_PAD", INT_MIN, INT_MAX, 0);
    return with_lpp(ix.bk_lpp, [&](auto L) { return launch_flat_lds(k_probe23_slots<decltype(L)::value>, len - 22, pad, s, ix, buf, len, canon_mode, slots); });
}

}  // namespace aix

// What both counters share (CountState, aix_handle.hpp); every function here is called with c.mutex held.
// the scratch table / workspace belong to the handle: counting calls are ordered behind one another even when they come in on
// different streams (the mutex only orders the enqueueing). The caller records c.done on `s` when it is through.
static int order_behind_last_count(CountState& c, hipStream_t s) {
    if (c.done) HIPCHK(hipStreamWaitEvent(s, c.done, 0));
    else HIPCHK(c.done.create());
    return AIX_OK;
}

// grow-only per-handle workspace of the counting paths (13-mer partitions; 23-mer slot stream + partitions)
static int ensure_count_workspace(CountState& c, uint64_t need, hipStream_t s) {
    // AIX_COUNT_TEST_WORKSPACE_MAX: test hook, requests above this many bytes "do not fit"
    const bool fits = need <= env_u64("AIX_COUNT_TEST_WORKSPACE_MAX", 0, ~0ull, ~0ull);
    const hipError_t e = c.ws.ensure(need, need, [&] { return hipStreamSynchronize(s); }, fits);
    if (e == hipErrorOutOfMemory) {
        set_last_error("count workspace of " + std::to_string(need) + " bytes does not fit in device memory");
        return AIX_ERR_NOMEM;
    }
    HIPCHK(e);
    return AIX_OK;
}

// Buffers are counted in pieces of at most *piece windows, and the workspace grows with the piece (bytes_for(windows)): one that does not
// fit halves the piece instead of failing the call, down to 4096 windows. On AIX_OK *piece is the piece to use (at most nwin).
template <typename F>
static int fit_count_workspace(CountState& c, uint64_t nwin, uint64_t* piece, hipStream_t s, F&& bytes_for) {
    for (;;) {
        const uint64_t pw = std::min(nwin, *piece);
        const int st = ensure_count_workspace(c, bytes_for(pw), s);
        if (st == AIX_OK) { *piece = pw; return AIX_OK; }
        if (st != AIX_ERR_NOMEM || pw <= 4096) return st;
        *piece = pw / 2;
    }
}

// Word 0 of the workspace is the partition kernels' error word (zeroed by the caller before the first launch): a chunk id outside a
// workgroup's region would have dropped counts, so the kernels raise it instead of staying silent and the call fails (costs one stream
// wait per call; the table is complete when this returns).
static int check_chunk_regions(CountState& c, const char* who, hipStream_t s) {
    uint32_t dropped = 0;
    HIPCHK(hipMemcpyAsync(&dropped, c.ws.p, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (dropped) { set_last_error(std::string(who) + ": chunk region exhausted (partition workspace undersized)"); return AIX_ERR_UNSUPPORTED; }
    return AIX_OK;
}

// K13 in three steps, so that a file can be counted part by part (aix_ingest.hip) as well as in one call: begin() orders the call behind
// the previous user of the handle's workspace and zeroes the output, add() counts one PLAIN buffer into it (any number of times; every
// window of the concatenated stream must lie inside exactly one of the buffers), end() finishes the table. The caller holds cnt.mutex
// from begin to end.
int count13_begin_locked(aix_index* h, uint64_t* d_tf_out, hipStream_t s) {
    CountState& c = h->cnt;
    { const int st = order_behind_last_count(c, s); if (st) return st; }
    c.c13_atomics = env_flag("AIX_COUNT13_ATOMICS") || !h->perm13_bijective;   // env: A/B switch for measurements / tests
    c.c13_added = false;
    if (c.c13_atomics) {
        if (!c.scratch13) HIPCHK(c.scratch13.alloc(8 * AIX_TOTAL_13MERS));
        HIPCHK(hipMemsetAsync(c.scratch13.p, 0, 8 * AIX_TOTAL_13MERS, s));
    }
    HIPCHK(hipMemsetAsync(d_tf_out, 0, 8 * AIX_TOTAL_13MERS, s));
    return AIX_OK;
}

int count13_add_locked(aix_index* h, const char* d_plain, uint64_t len, uint64_t* d_tf_out, hipStream_t s) {
    CountState& c = h->cnt;
    if (c.c13_atomics) {
        // scattered u64 memory-side atomics into the code-ordered table (slower; kept as the independent cross-check)
        if (len >= 13) HIPCHK(launch_flat(k_count13, len - 12, s, (const uint8_t*)d_plain, len, c.scratch13.as<unsigned long long>()));
        c.c13_added = true;
        return AIX_OK;
    }
    // The partitioned path indexes windows and chunks with 32 bits: buffers are cut into pieces of at most `piece` (2^31) window starts.
    // A window belongs to the piece that holds its first byte; a piece is handed its 12 following bytes as well, so the
    // cut needs no record boundary and every window is counted exactly once. Pieces after the first add to the table.
    uint64_t piece = env_count_piece("AIX_COUNT13_PIECE", 1ull << 31);
    const uint64_t nwin = len >= 13 ? len - 12 : 0;
    if (nwin == 0) return AIX_OK;
    { const int st = fit_count_workspace(c, nwin, &piece, s, [](uint64_t pw) { return count13_workspace_bytes(pw + 12); }); if (st) return st; }
    HIPCHK(hipMemsetAsync(c.ws.p, 0, 4, s));                                  // the error word of the workspace
    for (uint64_t first = 0; first < nwin; first += piece) {
        const uint64_t w = std::min(piece, nwin - first);
        HIPCHK(launch_count13_partitioned((const uint8_t*)d_plain + first, w + 12, c.ws.p, nullptr, h->perm13.as<uint32_t>(), d_tf_out, c.c13_added ? 1 : 0, s));   // fused permutation
        c.c13_added = true;
    }
    return check_chunk_regions(c, "count13", s);
}

int count13_end_locked(aix_index* h, uint64_t* d_tf_out, hipStream_t s) {
    int st = AIX_OK;
    if (h->cnt.c13_atomics) {
        const uint32_t* perm = h->perm13.as<uint32_t>();
        const unsigned long long* table = h->cnt.scratch13.as<unsigned long long>();
        const hipError_t e = h->perm13_bijective ? launch_flat(k_scatter13<false>, AIX_TOTAL_13MERS, s, perm, table, d_tf_out)
                                                 : launch_flat(k_scatter13<true>, AIX_TOTAL_13MERS, s, perm, table, d_tf_out);
        if (e != hipSuccess) { set_last_error(std::string("count13 scatter: ") + hipGetErrorString(e)); st = AIX_ERR_HIP; }
    }
    (void)hipEventRecord(h->cnt.done, s);
    return st;
}

extern "C" int aix_count13_dev(aix_index_t* h, const char* d_plain, uint64_t len, uint64_t* d_tf_out, void* stream) {
    if (!h || !d_tf_out || (len && !d_plain)) return AIX_ERR_ARG;
    if (h->k != 13) return AIX_ERR_MODE;
    DevGuard g(h->device);
    std::lock_guard<std::mutex> lk(h->cnt.mutex);
    hipStream_t s = (hipStream_t)stream;
    int st = count13_begin_locked(h, d_tf_out, s);
    if (st) return st;
    st = count13_add_locked(h, d_plain, len, d_tf_out, s);
    const int st2 = count13_end_locked(h, d_tf_out, s);
    return st ? st : st2;
}

// count23: three back ends, same result. Which one ran is reported by aix_index_info (count23_backend / count23_passes). Back ends 1 and 3
// use nothing of the handle but its tables, so they run outside cnt.mutex and take it for these two stores only.
static void record_count23(aix_index* h, uint32_t backend, uint32_t passes) {
    std::lock_guard<std::mutex> lk(h->cnt.mutex);
    h->cnt.c23_backend = backend; h->cnt.c23_passes = passes;
}

// (1) one memory-side atomic per found window: ~23 G scattered atomics/s on MI355X, which bounds the kernel once a probe costs a single line
static int count23_atomics(aix_index* h, const char* d_plain, uint64_t len, int canon_mode, uint32_t* d_tf_out, hipStream_t s) {
    const IndexDev d = h->dev();
    if (len >= 23 && d.n) HIPCHK(with_lpp(d.bk_lpp, [&](auto L) { return launch_flat(k_count23_fixed<decltype(L)::value>, len - 22, s, d, (const uint8_t*)d_plain, len, canon_mode, d_tf_out); }));
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
    const hipError_t e2 = d.n ? launch_flat(k_add_counts23<2>, d.n, s, h->dev_slots(), d.k, d.c, d.n, d_tf_out) : hipSuccess;
    const hipError_t e3 = hipStreamSynchronize(s);                             // the K1 result goes back to the block cache idle
    HIPCHK(e2);
    HIPCHK(e3);
    record_count23(h, 3, 0);
    return AIX_OK;
}

// The second stream of (2) and the events both ways, made by the first multi-piece call of a handle (under cnt.mutex).
// AIX_COUNT23_HIST_CUS=n[,style] (A/B switch, read here): the partition + histogram kernels get n of the 256 CUs and the probe the others,
// through CU-masked streams. The split kernel takes a whole CU (152 KiB of LDS, 16 waves of 128 VGPRs), so on shared CUs the two kernels
// alternate workgroup by workgroup instead of running side by side. style 0: the low n bits of the mask, 1: every (256 / n)-th bit.
// They are built into locals and handed to the handle together: a failure on the way leaves the handle without any of them, and the next
// call starts over.
static int ensure_count23_streams(CountState& c) {
    if (c.probe_stream) return AIX_OK;
    Stream probe, hist;
    Event probe_ev[2], hist_ev[2], start_ev;
    int hist_cus = 0, style = 0;
    env_int_pair("AIX_COUNT23_HIST_CUS", &hist_cus, &style);
    if (hist_cus >= 8 && hist_cus <= 224) {
        uint32_t mh[8] = {0, 0, 0, 0, 0, 0, 0, 0}, mp[8];
        const int step = style ? 256 / hist_cus : 1;
        for (int i = 0, n = 0; n < hist_cus && i < 256; i += step, ++n) mh[i >> 5] |= 1u << (i & 31);
        for (int w = 0; w < 8; ++w) mp[w] = ~mh[w];
        HIPCHK(probe.create_cu_mask(8, mp));
        HIPCHK(hist.create_cu_mask(8, mh));
    } else {
        HIPCHK(probe.create());
    }
    for (int i = 0; i < 2; ++i) {
        HIPCHK(probe_ev[i].create());
        HIPCHK(hist_ev[i].create());
    }
    HIPCHK(start_ev.create());
    c.probe_stream = std::move(probe);
    c.hist_stream = std::move(hist);
    for (int i = 0; i < 2; ++i) { c.probe_ev[i] = std::move(probe_ev[i]); c.hist_ev[i] = std::move(hist_ev[i]); }
    c.start_ev = std::move(start_ev);
    return AIX_OK;
}

// (2) the slots are streamed out (4 B per window) and added into tf[] by the chunked-partition + LDS histogram of the 13-mer counter: no
// global atomics at all. Handles 2^26 slots per pass over the slot stream (2048 partitions of 32 768 bins; a larger key set takes
// ceil(n / 2^26) passes) and pays a fixed cost, so short buffers keep (1).
static int count23_histogram(aix_index* h, const char* d_plain, uint64_t nwin, int canon_mode, uint32_t* d_tf_out, hipStream_t s) {
    const uint32_t range_bits = (uint32_t)env_int("AIX_COUNT23_TEST_RANGE_BITS", 4, 26, 26);   // test hook, several slot ranges on a small key set
    CountState& c = h->cnt;
    std::lock_guard<std::mutex> lk(c.mutex);
    { const int st = order_behind_last_count(c, s); if (st) return st; }
    RecordOnExit record_on_exit{c.done, s};                                    // the next counting call may touch the workspace once the caller's stream has reached this point
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
    { const int st = fit_count_workspace(c, nwin, &pw, s, [&](uint64_t w) {
          part_bytes = (count13_workspace_bytes(w + 12) + 255) / 256 * 256;
          slot_bytes = (4 * w + 255) / 256 * 256;
          overlap = may_overlap && nwin > w;
          return part_bytes + (overlap ? 2 : 1) * slot_bytes;
      }); if (st) return st; }
    uint32_t* slot_buf[2] = {(uint32_t*)(c.ws.as<uint8_t>() + part_bytes), (uint32_t*)(c.ws.as<uint8_t>() + part_bytes + (overlap ? slot_bytes : 0))};
    // an error in the middle of the piece loop would return with the probe stream still writing into the workspace, and the event recorded on
    // exit (caller's stream only) would let the next counting call in under it: a failing call waits for the side streams first
    DrainOnError<2> probe_drain{{&c.probe_stream, &c.hist_stream}};
    HIPCHK(hipMemsetAsync(c.ws.p, 0, 4, s));                                  // the error word of the partition workspace
    hipStream_t hs = s;
    if (overlap) {
        { const int st = ensure_count23_streams(c); if (st) return st; }
        HIPCHK(hipEventRecord(c.start_ev, s));                                 // the reads (and whatever else the caller queued) are ready when the first probe starts
        HIPCHK(hipStreamWaitEvent(c.probe_stream, c.start_ev, 0));
        if (c.hist_stream) { hs = c.hist_stream; HIPCHK(hipStreamWaitEvent(hs, c.start_ev, 0)); }
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
            HIPCHK(hipMemsetAsync(c.ws.as<uint32_t>() + 1, 0, 4, s));
            HIPCHK(launch_stream23_slots(d, (const uint8_t*)d_plain + first, w + 22, canon_mode, slot_buf[b], c.ws.as<uint32_t>() + 1, s));
        } else if (overlap) {
            if (ip >= 2) HIPCHK(hipStreamWaitEvent(c.probe_stream, c.hist_ev[b], 0));        // piece ip - 2 has been read out of this buffer
            HIPCHK(probe((const uint8_t*)d_plain + first, w + 22, slot_buf[b], c.probe_stream));
            HIPCHK(hipEventRecord(c.probe_ev[b], c.probe_stream));
            HIPCHK(hipStreamWaitEvent(hs, c.probe_ev[b], 0));
        } else {
            HIPCHK(probe((const uint8_t*)d_plain + first, w + 22, slot_buf[b], s));
        }
        uint32_t passes = 0;
        HIPCHK(launch_histogram_slots(slot_buf[b], w, c.ws.p, d_tf_out, h->n, hs, range_bits, &passes));
        c.c23_backend = 2; c.c23_passes = passes;
        if (overlap) HIPCHK(hipEventRecord(c.hist_ev[b], hs));
    }
    if (hs != s && ip) HIPCHK(hipStreamWaitEvent(s, c.hist_ev[(ip - 1) & 1], 0));
    { const int st = check_chunk_regions(c, "count23", s); if (st) return st; }
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
