// aix_internal.hpp — host-side view of an index resident in HBM + the prototypes that cross translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aix_device.hpp"

namespace aix {

// what kernels receive by value
struct IndexDev {
    MphfDev m;
    const KeyRec* keys;       // 23-mer: n records {code, tf} — only while an index is being built, or when no verification table was built
    // 23-mer with a verification table: checker[h] / tf[h] are NOT stored a second time. side[h] says where slot h's key lives: an entry of
    // the table (filed keys: 99 %), or — top bit set — a record of `unfiled` (keys beyond the eighth of their bucket, keys that are not in
    // their own MPHF slot). key_at() below is the one accessor.
    const uint32_t* side;
    const BkEntry* bk_store;  // the table's storage (also when the table is switched off for probing)
    const KeyRec* unfiled;
    uint64_t n;               // 23-mer: number of keys; 13-mer: 4^13
    const uint64_t* tf13_code;  // 13-mer: tf in 2-bit-code order (u64[4^13])
    const uint64_t* tf13_mphf;  // 13-mer: tf in mphf order (the file's order)
    const uint32_t* perm13;     // 13-mer: 2-bit code -> mphf slot
    uint32_t canonical_only;  // 23-mer: every stored code <= its reverse complement
    uint32_t k;
    uint32_t use_fp;          // 23-mer: the fingerprint nibbles of the MPHF records are populated
    uint32_t early_exit;      // 23-mer: presence masks populated and the early-exit walk enabled
    const BkEntry* bk;        // 23-mer: verification table (nb buckets of 8 entries), nullptr when not built / switched off
    uint32_t nb;
    uint32_t bk_lpp;          // lanes that share one bucket read (8, 4, 2 or 1); launch-time choice
    const uint64_t* bloom;    // 23-mer: absence filter in front of the table (nbloom 64-bit words), nullptr when off
    uint32_t nbloom;
    const BkEntry* mk;        // 23-mer: minimizer-keyed copy of the table for the streaming counter: the entries of bucket b are mk[mk_off[b] .. mk_off[b + 1]); nullptr when off
    uint32_t nbm;
    const uint32_t* mk_off;   // nbm + 1 offsets into mk (a bucket = all filed keys whose minimizer hashes to it: no bucket overflows at build time)
    uint32_t mk_cap;          // entries of a bucket a lane reads (<= AIX_MK_ENTRIES); a longer bucket leaves its windows to the hash-keyed table
};

#define AIX_SIDE_UNFILED 0x80000000u
// checker[h] and tf[h] of PHASH_MAP (hash.hpp:82-121) for slot h < n
__device__ __forceinline__ KeyRec key_at(const IndexDev& ix, uint64_t h) {
    if (ix.keys) return ix.keys[h];
    const uint32_t s = ix.side[h];
    if (s & AIX_SIDE_UNFILED) return ix.unfiled[s & ~AIX_SIDE_UNFILED];
    const BkEntry e = ix.bk_store[s];
    KeyRec r;
    r.code = (uint64_t)e.code_lo | ((uint64_t)(e.code_hi & 0x3FFFu) << 32);
    r.tf = e.tf;
    r.pad = 0;
    return r;
}

enum LookupMode { MODE_TF = 0, MODE_HASH = 1, MODE_KIDSTRAND = 2, MODE_BOTH = 3, MODE_TOTAL = 4, MODE_LINES = 5 };

struct LookupOut {
    uint32_t* tf;       // MODE_TF
    uint64_t* u64a;     // HASH: hash; KIDSTRAND: kid; BOTH: fwd; TOTAL: sum
    uint64_t* u64b;     // BOTH: rc
    uint8_t* strand;    // KIDSTRAND
};

// scratch pool (aix_pool.hip): cached device blocks for per-call temporaries; release only after the using stream is synchronised
hipError_t pool_alloc(void** out, size_t bytes);
void pool_free(void* p);
void pool_trim();

// The launchers that cross files (every other one is static beside its kernel). All asynchronous on `stream`; return hipGetLastError().
// aix_lookup.hip, also called by aix_lookup_binned.hip.
// gate (nullable): a device word read at the start of the kernel; non-zero = the binned path answers this batch and the kernel returns at once
hipError_t launch_lookup23_ascii(const IndexDev& ix, const uint8_t* q, uint64_t N, int mode, LookupOut out, hipStream_t s, const uint32_t* gate = nullptr);
// canonical index: out[list[j]] = tf of query list[j] for j < *count (<= max_count, which sizes the grid), when *gate is non-zero; *survivors_stat += *count
hipError_t launch_lookup23_list(const IndexDev& ix, const uint8_t* q, const uint32_t* list, const uint32_t* count, uint64_t max_count, const uint32_t* gate,
                                uint32_t* out, unsigned long long* survivors_stat, hipStream_t s);

// counting (aix_count13.hip)
uint64_t count13_workspace_bytes(uint64_t len);
// perm/out_mphf set: counters are written straight into the (pre-zeroed) mphf-ordered output; else into table_code
hipError_t launch_count13_partitioned(const uint8_t* buf, uint64_t len, void* workspace, unsigned long long* table_code, const uint32_t* perm,
                                      uint64_t* out_mphf, int accumulate, hipStream_t s);
// count23 without global atomics: tf_out[slot] += occurrences of slot in the stream (0xFFFFFFFF = skip); one pass per 2^26 slots of the key set
hipError_t launch_histogram_slots(const uint32_t* d_slots, uint64_t nslots, void* workspace /* count13_workspace_bytes(nslots + 12) */, uint32_t* tf_out,
                                  uint64_t n, hipStream_t s, uint32_t range_bits = 26 /* slots per pass = 2^range_bits <= 2^26 */, uint32_t* passes_out = nullptr);
// the same slot stream from the minimizer-keyed table (aix_stream23.hip): a lane owns 32 consecutive windows; needs ix.mk
hipError_t launch_stream23_slots(const IndexDev& ix, const uint8_t* buf, uint64_t len, int canon_mode, uint32_t* slots /* [len - 22] */,
                                 uint32_t* flag /* zeroed word: set when a window stayed undecided */, hipStream_t s);
// the same slot stream with a run of w (16 / 32) consecutive windows per lane (aix_stream23.hip: the bytes are encoded once per run); needs ix.bk
hipError_t launch_run23_slots(const IndexDev& ix, const uint8_t* buf, uint64_t len, int canon_mode, uint32_t* slots, int w, hipStream_t s);
// K1 front end (aix_api.hip, also called by aix_merge.hip): the canonical code of every k-window of a PLAIN buffer, ~0 where there is none
hipError_t launch_window_codes(const uint8_t* buf, uint64_t len, int k, int canon_mode, uint64_t* out /* [len-k+1] */, hipStream_t s);

// out[i] = in[0] + ... + in[i - 1] (device arrays of n words; synchronises the stream)
hipError_t exclusive_scan_u32(const uint32_t* d_in, uint32_t* d_out, uint64_t n, hipStream_t s);

// positions index (aix_positions.hip)
hipError_t positions_indices(const IndexDev& ix, uint64_t* d_indices /* n+1 */, hipStream_t s);
hipError_t positions_fill(const IndexDev& ix, const uint8_t* d_reads, uint64_t len, uint64_t start, const uint64_t* d_indices, uint64_t* d_positions,
                          uint64_t piece, const uint32_t* filled_init, uint64_t base_offset, hipStream_t s,
                          uint32_t* backend_out = nullptr /* bit 0: a piece went through the stable radix sort, bit 1: through the MSD partition */);
// grouping of the probe's (bucket, offset) pairs without a full-width sort (aix_a2msd.hip): two-level MSD partition + per-bucket LDS stage
bool a2_msd_eligible(uint64_t nwin, uint64_t n);
hipError_t a2_msd_place(const IndexDev& ix, const uint32_t* keys, uint64_t nwin, uint64_t piece_first, uint32_t* filled, bool advance, const uint64_t* d_indices,
                        uint64_t* d_positions, hipStream_t s, bool* untouched = nullptr /* set when the call failed before writing anything (workspace allocation) */);
hipError_t positions_bucket_counts(const IndexDev& ix, const uint8_t* d_reads, uint64_t len, uint64_t start, unsigned long long* d_counts, hipStream_t s);

// RAII holder of a pool block used on stream `st`: the stream is synchronised before the block goes back (also by alloc on a live block)
struct DevArr {
    void* p = nullptr;
    hipStream_t st = nullptr;
    DevArr() = default;
    explicit DevArr(hipStream_t s) : st(s) {}
    DevArr(const DevArr&) = delete;
    DevArr& operator=(const DevArr&) = delete;
    void drop() { if (p) { (void)hipStreamSynchronize(st); pool_free(p); p = nullptr; } }
    ~DevArr() { drop(); }
    hipError_t alloc(size_t bytes) { drop(); return pool_alloc(&p, bytes ? bytes : 1); }
    void* release() { void* q = p; p = nullptr; return q; }
};

// (keys ascending, counts, n) of a distinct-k-mer set in HBM. RunView borrows, DistinctRun owns its two pool blocks.
struct RunView {
    const uint64_t* k;
    const uint64_t* c;
    uint64_t n;
};
// THE CONTRACT: the blocks go back to the pool WITHOUT a synchronise (an aix_distinct_t outlives the stream its producer ran on). So
// every producer synchronises its stream before it returns (all do: n has to be known), and whoever enqueues work that reads the blocks
// synchronises before the holder dies or is assigned to.
struct DistinctRun {
    uint64_t* k = nullptr;
    uint64_t* c = nullptr;
    uint64_t n = 0;
    DistinctRun() = default;
    DistinctRun(const DistinctRun&) = delete;
    DistinctRun& operator=(const DistinctRun&) = delete;
    DistinctRun(DistinctRun&& o) noexcept : k(o.k), c(o.c), n(o.n) { o.k = o.c = nullptr; o.n = 0; }
    DistinctRun& operator=(DistinctRun&& o) noexcept {
        if (this != &o) { reset(); k = o.k; c = o.c; n = o.n; o.k = o.c = nullptr; o.n = 0; }
        return *this;
    }
    ~DistinctRun() { reset(); }
    void reset() {
        if (k) pool_free(k);
        if (c) pool_free(c);
        k = c = nullptr;
        n = 0;
    }
    // takes over two finished blocks (their stream synchronised) of m entries
    void adopt(DevArr& keys, DevArr& counts, uint64_t m) { reset(); k = (uint64_t*)keys.release(); c = (uint64_t*)counts.release(); n = m; }
    RunView view() const { return RunView{k, c, n}; }
};

// K1's two back ends for one piece (aix_k1.hip). Both leave keys ascending in `keys` and one count per key in `counts`, on the blocks'
// stream, synchronised; *n_out = 0 leaves the blocks empty.
// Radix sort + run-length of the nwin window codes in d_codes (~0 = no k-mer), which is clobbered; u32 counts.
hipError_t distinct_from_codes(uint64_t* d_codes, uint64_t nwin, int k, DevArr& keys, DevArr& counts, uint64_t* n_out, hipStream_t s);
bool k1_msd_eligible(uint64_t nwin, int k);
// The two big temporaries of a K1 piece (8 B per window of code / remainder staging, ~8 B per window of partition chunks: 16 + 17 GiB for a
// 2^31-window piece), kept by whoever counts piece after piece: a hipMalloc / hipFree pair of that size costs ~0.2 s, more than the kernels
// of the piece (measured: 60 M reads in 5 pieces took 2.5 s of wall clock around 0.16 s of kernels before the blocks were kept).
struct K1Scratch {
    DevArr codes, work;
    size_t codes_bytes = 0, work_bytes = 0;
    explicit K1Scratch(hipStream_t s) : codes(s), work(s) {}
    static hipError_t need(DevArr& a, size_t& have, size_t bytes) {             // grow only
        if (bytes <= have) return hipSuccess;
        have = 0;
        const hipError_t e = a.alloc(bytes);                    // from the block cache: a process that counts buffer after buffer finds them there again
        if (e == hipSuccess) have = bytes;
        return e;
    }
};
// The same without a full-width sort: MSD partition in two levels + per-bucket LDS hash / sort; u64 counts. The windows of the PLAIN
// buffer are encoded inside level 1; d_staging (8 B per window) is only what the later stages write their remainders and per-bucket
// counts to, and the partition workspace lives in scratch.work, kept for the next piece.
// *fell_back: a bucket held too many distinct remainders; nothing was produced and the caller takes the radix-sort path.
hipError_t distinct_from_codes_msd(const uint8_t* d_plain, uint64_t plen, uint64_t nwin, int k, int canon_mode, uint64_t* d_staging, K1Scratch& scratch, DevArr& keys,
                                   DevArr& counts, uint64_t* n_out, bool* fell_back, hipStream_t s);

// sorted (key, count) runs merged without a sort (aix_merge.hip). Every producer below synchronises `s`; on a failure `out` is empty.
// (A, B) -> keys ascending, equal keys summed. A and B are each sorted and free of repeats.
hipError_t merge_sum_runs(RunView a, RunView b, DistinctRun& out, hipStream_t s);
hipError_t merge_runs(const uint64_t* d_keys, const uint64_t* d_counts, const uint64_t* offs /* host, nruns + 1 */, uint32_t nruns, uint64_t min_count,
                      DistinctRun& out, hipStream_t s);
hipError_t merge_counts(const uint64_t* d_keys, const uint64_t* d_counts, uint64_t n, uint64_t min_count, DistinctRun& out, hipStream_t s);
hipError_t distinct_from_plain(const uint8_t* d_plain, uint64_t plen, int k, int canon_mode, uint64_t min_count, uint64_t piece, DistinctRun& out, hipStream_t s);
// the distinct k-mers of everything added so far; a piece = all k-windows of one PLAIN buffer (<= 2^31 windows)
class DistinctAcc {
public:
    DistinctAcc(int k, int canon_mode, hipStream_t s);
    ~DistinctAcc();
    DistinctAcc(const DistinctAcc&) = delete;
    DistinctAcc& operator=(const DistinctAcc&) = delete;
    hipError_t add_plain(const uint8_t* d_plain, uint64_t plen);
    hipError_t finish(uint64_t min_count, DistinctRun& out);
    uint64_t size() const { return acc.n; }
    uint64_t pieces = 0, merges = 0;
private:
    int k, canon_mode;
    hipStream_t s;
    K1Scratch scratch;
    DistinctRun acc;
};

// record normalisation on the device (aix_normalize.hip); d_out holds len + 1 bytes
hipError_t normalise_device(const uint8_t* d_raw, uint64_t len, int format, int fasta_mode, uint8_t* d_out, uint64_t* out_len, hipStream_t s);
// one part of an input normalised piece by piece: *state_io = reader state handed from part to part (AIX_NORM_START before the first)
static constexpr uint32_t AIX_NORM_START = 0xFFFFFFFFu;
hipError_t normalise_device_part(const uint8_t* d_raw, uint64_t len, int format, int fasta_mode, uint8_t* d_out, uint64_t* out_len, uint32_t* state_io, int last,
                                 hipStream_t s);

}  // namespace aix
