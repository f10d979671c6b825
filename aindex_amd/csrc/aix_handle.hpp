// aix_handle.hpp — private to the library: the index handle resident in HBM, the error / device / scratch helpers shared by the
// translation units that implement the C ABI (aix_api.hip and one file per subsystem). The handle frees itself: every block, stream,
// event and pinned block on it is a member of an owner type of aix_owned.hpp, grouped by the subsystem that uses it, and the byte
// ledger device_bytes is kept by those owners. A handle is made and deleted through HandlePtr, whose deleter switches to the handle's
// device; aix_index_close is that plus pool_trim().
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <mutex>
#include <string>

#include "../../include/aindex_hip.h"
#include "aix_internal.hpp"
#include "aix_owned.hpp"

using namespace aix;

void set_last_error(const std::string& s);      // thread-local text behind aix_strerror(AIX_ERR_HIP)

#define HIPCHK(expr)                                                                          \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) {                                                               \
            set_last_error(std::string(#expr) + ": " + hipGetErrorString(_e));                \
            return AIX_ERR_HIP;                                                               \
        }                                                                                     \
    } while (0)


struct DevGuard {   // switch to the handle's device for the duration of a call, then restore
    int prev = -1;
    bool ok = false;
    explicit DevGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = (hipSetDevice(dev) == hipSuccess);
    }
    ~DevGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

struct DevBuf {                     // per-call temporary from the scratch pool, used on ONE stream (default: the null stream)
    void* p = nullptr;
    hipStream_t st = nullptr;
    DevBuf() = default;
    explicit DevBuf(hipStream_t s) : st(s) {}
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    bool pooled = true;
    hipError_t alloc(uint64_t bytes) { return pool_alloc(&p, bytes ? bytes : 1); }
    // one-shot staging (index load): straight from the driver and straight back, never parked in the scratch cache
    hipError_t alloc_once(uint64_t bytes) { pooled = false; return hipMalloc(&p, bytes ? bytes : 1); }
    // a block goes back to the pool idle: wait for the stream it was used on (not for the whole device — other handles and
    // other host threads keep running; error paths leave through here too)
    ~DevBuf() { if (p) { (void)hipStreamSynchronize(st); if (pooled) pool_free(p); else (void)hipFree(p); } }
};

// A .pf image in HBM: the header fields and the BvRec records. upload_mphf (aix_index.hip) fills one; the handle holds one, and so
// does a scatter call that needs the MPHF and nothing else of a handle.
struct MphfImage {
    uint64_t mphf_n = 0, D = 0, seed = 0, B = 0, W = 0;
    HBlock recs;
    explicit MphfImage(uint64_t* ledger = nullptr) : recs(ledger) {}
    MphfDev view() const {                     // without the early-exit table
        MphfDev m{};
        m.recs = recs.as<BvRec>();
        m.D = D;
        m.seed = seed;
        m.nrecs = (B + 15) / 16;
        m.fm = make_fastmod(D);
        return m;
    }
};

// The groups below are the state of one subsystem each; the file named uses the members directly. Members are released in reverse
// order of declaration, and where that order matters the comment says so.

// counting (aix_count.hip; aix_ingest.hip drives K13 part by part): everything here is touched under `mutex`
struct CountState {
    std::mutex mutex;
    // count23's histogram back end: the partition + histogram kernels on their own CUs (hist_stream, AIX_COUNT23_HIST_CUS only) and the slot
    // probe of piece i + 1 (probe_stream) beside piece i on the caller's stream; all of them or none (ensure_count23_streams)
    Stream hist_stream, probe_stream;
    Event probe_ev[2], hist_ev[2], start_ev;
    Event done;                                // recorded behind every counting call: the next one (any stream) waits for it before touching the workspace
    HBlock scratch13;                          // code-ordered count table, lazily allocated
    GrowBlock ws;                              // workspace of both counters: 13-mer partitions; 23-mer slot stream + partitions
    uint32_t c23_backend = 0, c23_passes = 0;  // the last aix_count23_fixed*: 1 = memory-side atomics, 2 = slot stream + LDS histogram, 3 = distinct k-mers first (K1); passes over the slot stream
    bool c13_atomics = false, c13_added = false;   // state of a 13-mer count in progress (between count13_begin_locked and count13_end_locked)
    explicit CountState(uint64_t* ledger) : scratch13(ledger), ws(ledger) {}
};

// binned lookups (aix_lookup_binned.hip): records, survivor list, cursors and header of one piece, and the filter's coarse image (a
// byte per word, slice by slice) that pass B holds in LDS. Grow-only, freed at close; not part of the index, so not on the ledger.
struct BinnedState {
    std::mutex mutex;
    GrowBlock ws, coarse;
    HBlock stats;                              // device: pieces binned, pieces direct, records that overflowed, survivors; records tested against the coarse image, records sent on
    const uint64_t* coarse_src = nullptr;      // what the image was folded from
    uint32_t coarse_nbloom = 0, coarse_wps = 0;
    hipStream_t stream = nullptr;              // the stream of the last call
    bool used = false;
    Event done{true};                          // recorded behind every call: a call on another stream waits for it first. Declared last: it is waited for before the blocks go
};

// what is attached for the position and read queries (aix_posquery.hip, aix_readsquery.hip, the aix_seq* files)
struct Attachments {
    Attached ai_indices, ai_positions;         // the .indices.bin (n + 1 offsets) / .index.bin (ai_total entries, 1-based, 0 = empty slot) images: copied or borrowed together
    uint64_t ai_total = 0;
    HBlock rx;                                 // the .ridx intervals: starts[rx_n], ends[rx_n], rids[rx_n]
    uint64_t rx_n = 0;
    Attached rd;                               // the .reads image
    uint64_t rd_len = 0;
    explicit Attachments(uint64_t* ledger) : ai_indices(ledger), ai_positions(ledger), rx(ledger), rd(ledger) {}
};

// tiny host batches (a Python loop over index[kmer]; aix_lookup.hip): pinned, device-mapped staging so that a call is one memcpy into
// host memory, one launch and one synchronise — no hipMemcpy round trips
struct SmallBatch {
    std::mutex mutex;
    PinnedBlock in, out[3];
    PinnedBlock cov;                           // small coverage requests (kCovPin bytes)
    Stream stream;                             // own stream: no implicit ordering with the null stream
};

// Large host-buffer batches (aix_lookup.hip): three staging sets (pinned host + device buffers + a stream + an event each), built by the
// first large batch. The streams are declared behind the blocks they write: they are synchronised and destroyed first.
struct HostPipe {
    static constexpr int S = 3;
    static constexpr uint64_t kChunkQ = 2ull << 20;          // queries per chunk
    static constexpr uint64_t kInBytes = kChunkQ * 23 + 64, kOutBytes = kChunkQ * 8;
    PinnedBlock hin[S], hout[S][3];
    HBlock din[S], dout[S][3];
    Stream st[S] = {Stream(true), Stream(true), Stream(true)};
    Event ev[S];
};

struct aix_index {
    int device = 0;
    uint32_t k = 0;
    uint64_t n = 0;
    uint64_t device_bytes = 0;                 // the ledger: what the handle holds in HBM for the index (adjusted by the owners bound to it, aix_owned.hpp)
    SmallBatch small;
    CountState cnt{&device_bytes};
    std::unique_ptr<HostPipe> pipe;
    std::mutex pipe_mutex;
    Attachments att{&device_bytes};
    BinnedState lb;
    // the index in HBM
    MphfImage mphf{&device_bytes};
    HBlock ee{&device_bytes};                  // EeRec: early-exit table (23-mer handles with keys)
    HBlock keys{&device_bytes};                // KeyRec: checker[] / tf[] interleaved: while the handle is built, and afterwards only when no verification table was built
    HBlock side{&device_bytes};                // u32: with a table: slot -> table entry | AIX_SIDE_UNFILED + index into `unfiled` (4 B per key instead of 16)
    HBlock unfiled{&device_bytes};             // KeyRec: the keys the table does not hold (~1 %)
    uint64_t n_unfiled = 0;
    Attached bk{&device_bytes};                // BkEntry: verification table, nb buckets of eight {code, tf, slot} entries (one 128-byte line each); borrowed once it lives in a caller's block (aix_debug_relocate_table)
    uint32_t nb = 0;
    uint32_t bk_lpp = 8;                       // lanes that share one bucket read
    bool bk_lpp_set = false;                   // chosen by the caller (AIX_BUCKET_LANES / aix_index_set_bucket_table): then every consumer uses it
    uint64_t bk_unfiled = 0;                   // keys beyond the eighth of their bucket (answered through the MPHF)
    bool bk_enabled = true;
    HBlock mk{&device_bytes};                  // BkEntry: minimizer-keyed copy of the table for the streaming counter: entries grouped by minimizer bucket
    HBlock mk_off{&device_bytes};              // u32: nbm + 1 offsets into mk
    uint32_t mk_cap = 16;                      // entries of a bucket a lane of the streaming counter reads
    uint32_t nbm = 0;
    uint64_t mk_unfiled = 0;
    bool mk_enabled = true;
    HBlock bloom{&device_bytes};               // u64: absence filter in front of the table (lookups / coverage)
    uint32_t nbloom = 0;
    bool bloom_enabled = true;
    HBlock tf13_mphf{&device_bytes}, tf13_code{&device_bytes}, perm13{&device_bytes};   // u64, u64, u32
    bool perm13_bijective = false;             // 13-mer: code -> mphf slot is a bijection of [0, 4^13) (true for the all-13-mers .pf)
    bool canonical_only = false;
    bool canonical_fastpath = true;
    bool has_fp = false;
    bool fp_filter = true;
    bool early_exit = true;                    // (used when the early-exit table exists: built at open only without a verification table, else on request)
    uint64_t pos_total = 0;                    // aix_positions_total, once computed (sum of tf[])
    bool pos_total_known = false;
    uint32_t a2_backend = 0;                   // the last positions fill: bit 0 = stable radix sort, bit 1 = MSD partition (per piece)

    // the slot-stream consumers (count23's histogram path, the positions probe): two lanes per bucket line unless the caller chose a width
    IndexDev dev_slots() const {
        IndexDev d = dev();
        if (!bk_lpp_set) d.bk_lpp = 2;
        return d;
    }
    IndexDev dev() const {
        IndexDev d{};
        d.m = mphf.view();
        d.m.ee = ee.as<EeRec>();
        d.keys = keys.as<KeyRec>();
        d.side = side.as<uint32_t>();
        d.bk_store = bk.as<BkEntry>();
        d.unfiled = unfiled.as<KeyRec>();
        d.n = n;
        d.tf13_code = tf13_code.as<uint64_t>();
        d.tf13_mphf = tf13_mphf.as<uint64_t>();
        d.perm13 = perm13.as<uint32_t>();
        d.canonical_only = (canonical_only && canonical_fastpath) ? 1u : 0u;
        d.k = k;
        d.use_fp = (has_fp && fp_filter) ? 1u : 0u;
        d.early_exit = (has_fp && ee && early_exit) ? 1u : 0u;
        d.bk = bk_enabled ? d.bk_store : nullptr;
        d.nb = nb;
        d.bk_lpp = bk_lpp;
        d.bloom = (d.bk && bloom_enabled) ? bloom.as<uint64_t>() : nullptr;
        d.nbloom = nbloom;
        d.mk = (d.bk && mk_enabled) ? mk.as<BkEntry>() : nullptr;
        d.nbm = nbm;
        d.mk_off = mk_off.as<uint32_t>();
        d.mk_cap = mk_cap;
        return d;
    }
};

// A handle is deleted on its own device (every owner above frees through the runtime's current device)
struct HandleDelete {
    void operator()(aix_index* h) const { DevGuard g(h->device); delete h; }
};
using HandlePtr = std::unique_ptr<aix_index, HandleDelete>;

// the chain of aix_positions_query* (aix_posquery.hip): d_offsets (N + 1) and *total_out are always produced; entries only when
// *total_out <= cap and d_positions is given. Synchronises `s`.
namespace aix {
hipError_t posquery_run(aix_index* h, const uint8_t* d_kmers, uint64_t N, uint64_t m, uint64_t* d_offsets, uint64_t* d_positions, uint64_t* d_rid,
                        uint64_t* d_local, uint64_t cap, uint64_t* total_out, hipStream_t s);
}
// (the parts of that chain shared with aix_seqhits.hip — pq_resolve23_words, pq_locate, and posquery_lists = the chain behind the resolve
// step — are declared in aix_posquery.hpp, which includes this header)

// shared by the files that implement the ABI: device index in range (aix_index.hip)
__attribute__((visibility("hidden"))) int check_device(int device);

// The binned tf lookup of large absent-heavy batches (aix_lookup_binned.hip). AIX_LB_TAKEN: everything is enqueued on `s`;
// AIX_LB_NOT_TAKEN: not a candidate (mode, index, switches, batch size) or no workspace, the caller runs the direct path; < 0: error.
#define AIX_LB_NOT_TAKEN 0
#define AIX_LB_TAKEN 1
static constexpr uint64_t AIX_LB_DEFAULT_MIN = 1ull << 24;      // AIX_LOOKUP_BINNED_MIN (profiles/lookup_binned/README.md)
int lookup23_binned(aix_index* h, const IndexDev& d, const uint8_t* q, uint64_t N, uint32_t* out, hipStream_t s);

// K13 in steps (aix_count.hip); the caller holds h->cnt.mutex from begin to end
int count13_begin_locked(aix_index* h, uint64_t* d_tf_out, hipStream_t s);
int count13_add_locked(aix_index* h, const char* d_plain, uint64_t len, uint64_t* d_tf_out, hipStream_t s);
int count13_end_locked(aix_index* h, uint64_t* d_tf_out, hipStream_t s);
