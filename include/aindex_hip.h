/* include/aindex_hip.h — C ABI of libaindex_hip.so (MI355X / gfx950).
 *
 * This is the drop-in boundary for the k-mer count / perfect-hash lookup path of ad3002/aindex.
 * Every entry point names the reference interface it replaces (file:line under /root/reference).
 * Plain pointers and sizes only; no C++/torch types. All functions return an int status
 * (AIX_OK = 0, negative = error, see aix_strerror) and never abort the process — the reference's
 * std::terminate()/exit(10|12) paths (python_wrapper.cpp:265,413,1118; hash.cpp:37,129,153) become
 * error codes. Queries are thread-safe per handle. The library fails loudly (AIX_ERR_HIP) when no
 * HIP device is usable: there is NO CPU fallback behind this ABI.
 *
 * Naming: `*_dev` entry points take DEVICE pointers and a hipStream_t (passed as void*) and are
 * asynchronous on that stream; the un-suffixed twins take HOST pointers, stage through HBM and
 * return when the result is in the caller's buffer.
 */
#ifndef AINDEX_HIP_H
#define AINDEX_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AIX_OK               0
#define AIX_ERR_ARG         -1   /* bad argument / NULL handle                                  */
#define AIX_ERR_IO          -2   /* file missing or short (reference: std::terminate / exit(10)) */
#define AIX_ERR_FORMAT      -3   /* malformed .pf / size mismatch                                */
#define AIX_ERR_NOMEM       -4
#define AIX_ERR_HIP         -5   /* HIP runtime error or no device                               */
#define AIX_ERR_UNSUPPORTED -6   /* e.g. n >= 2^32 keys                                          */
#define AIX_ERR_MODE        -7   /* 13-mer call on a 23-mer handle or vice versa                 */
#define AIX_ERR_CONFLICT   -12   /* index scatter collision (reference: exit(12), hash.cpp:708)  */

#define AIX_TOTAL_13MERS 67108864ull   /* 4^13, python_wrapper.cpp:141 */

/* input formats of the counters (count_kmers13.cpp:187-206) */
#define AIX_FMT_AUTO  -1
#define AIX_FMT_PLAIN  0
#define AIX_FMT_FASTA  1
#define AIX_FMT_FASTQ  2

/* canonical form used when counting 23-mers */
#define AIX_CANON_NONE    0
#define AIX_CANON_REF_X86 1   /* bit-exact with kmer_counter's defective rc, count_kmers.cpp:116-136 */
#define AIX_CANON_TRUE_RC 2   /* true reverse complement (tests/analyze_kmers.py:19-80)              */

typedef struct aix_index aix_index_t;   /* opaque: MPHF + tf/checker resident in HBM */

typedef struct {
    uint32_t k;               /* 23 or 13                                                     */
    uint32_t device;          /* HIP device ordinal                                            */
    uint64_t n;               /* keys: size(.kmers.bin)/8 (23) or 4^13 (13)                    */
    uint64_t mphf_n;          /* n stored in the .pf                                           */
    uint64_t hash_domain;     /* m_hash_domain, mphf.hpp:26                                    */
    uint64_t seed;            /* jenkins64 seed                                                */
    uint64_t bitpairs;        /* 3 * hash_domain                                               */
    uint64_t device_bytes;    /* HBM held by this handle                                       */
    uint32_t canonical_only;  /* 1 if every stored 23-mer code <= its reverse complement       */
    uint32_t bucket_table;    /* 1 if the verification table is built and switched on          */
    uint64_t buckets;         /* its 128-byte buckets (0: not built)                           */
    uint64_t bucket_unfiled_keys; /* keys beyond the eighth of their bucket (MPHF path)        */
    uint32_t bucket_lanes;    /* lanes that share one bucket read (8, 4, 2 or 1)               */
    uint32_t absence_filter_words; /* 64-bit words of the absence filter in front of the table (0: off) */
    uint64_t minimizer_lines;     /* 128-byte lines of the minimizer-keyed copy of the table (0: off)   */
    uint64_t minimizer_unfiled_keys; /* keys whose chain of lines was full (answered by the hash-keyed table) */
    uint32_t count23_backend; /* the last aix_count23_fixed* call on this handle: 0 none yet, 1 memory-side atomics (short buffers,
                                 AIX_COUNT23_ATOMICS=1), 2 slot stream + LDS histogram, 3 distinct k-mers of the reads first (K1), one
                                 probe per distinct k-mer (buffers of >= 2^29 windows holding >= 8 windows per key; AIX_COUNT23_VIA_K1) */
    uint32_t count23_passes;  /* back end 2: passes over the slot stream = ceil(n / 2^26)                                           */
    uint32_t positions_backend; /* the last aix_positions_fill* call: bit 0 = a piece was grouped by the stable radix sort (short buffers, more than
                                   2^30 slots, workspace did not fit), bit 1 = by the MSD partition; 0 none yet                    */
    uint32_t reserved0;
    uint32_t aindex_attached; /* positions index for aix_positions_query*: 0 none, 1 copied by aix_aindex_attach, 2 borrowed by aix_aindex_attach_dev */
    uint32_t ridx_on_device;  /* 1 if aix_ridx_attach found the read intervals sorted and disjoint and put them into HBM                  */
    uint64_t aindex_entries;  /* entries of the attached positions array (8 bytes each, plus 8 * (n + 1) of offsets)                      */
    uint64_t ridx_reads;      /* attached read intervals (24 bytes each)                                                                  */
} aix_info_t;

const char* aix_version(void);
const char* aix_strerror(int status);
int aix_device_count(int* count);
/* Calls that need multi-GB temporaries (K1, A1/A2, I1, host-buffer staging) take them from a per-device cache of device
 * blocks (a hipMalloc of that size costs ~20 ms). AIX_SCRATCH_CACHE_GB (default 40) bounds the cache; this and
 * aix_index_close() return it to the driver. */
void aix_scratch_trim(void);                     /* AIX_ERR_HIP if the runtime is unusable  */
/* Page-locked host memory for the buffers a binding hands to the host-pointer entry points (queries in, answers out): a pinned buffer
 * crosses the link at ~48 GB/s instead of ~32 GB/s through the library's own staging, and one kept between calls is not page-faulted again
 * (a fresh 460 MB buffer written by 32 threads costs more than the lookup it feeds). This is where the reference's binding holds the
 * std::vector<std::string> / std::vector<uint32_t> of get_tf_values (python_wrapper.cpp:653-664). Free with aix_host_free only. */
int aix_host_alloc(uint64_t bytes, void** out);
int aix_host_free(void* p);

/* ------------------------------------------------------------------------------------------
 * Index lifecycle.
 * replaces AindexWrapper::load / load_hash_file / load_from_prefix_23mer
 *          (python_wrapper.cpp:228-258,1103-1132) + load_hash (hash.cpp:367-450)
 *          AindexWrapper::load_13mer_index / load_from_prefix_13mer (python_wrapper.cpp:404-437,1162-1188)
 * File layouts are the reference's: .pf = mphf::save (mphf.hpp:99-105), .kmers.bin = u64[n],
 * .tf.bin = u32[n] (23-mer, compute_index.cpp:59-67) or u64[4^13] (13-mer, count_kmers13.cpp:358-388).
 * ------------------------------------------------------------------------------------------ */
/* Validate a .pf image on the HOST (no device needed): header u64 n, hash_domain, seed, bitpairs (mphf.hpp:99-113,
 * base_hash.hpp:116-119, ranked_bitpair_vector.hpp:78-84), bitpairs == 3 * hash_domain without wrap-around, node ids
 * within 32 bits, n <= bitpairs, and the image long enough for the bit-pair words and block ranks. Every open / create /
 * scatter entry point applies the same check before anything is uploaded: AIX_ERR_FORMAT instead of an out-of-bounds
 * read on the device (the reference trusts the header). hdr_out (nullable) receives the four header words. */
int aix_pf_check(const void* pf_bytes, uint64_t pf_len, uint64_t hdr_out[4]);
int aix_index_open_23(const char* pf_path, const char* tf_bin_path, const char* kmers_bin_path,
                      int device, aix_index_t** out);
int aix_index_open_13(const char* pf_path, const char* tf_bin_path /* NULL: all-zero table */,
                      int device, aix_index_t** out);
/* same, from caller memory (host pointers) */
int aix_index_create_23(const void* pf_bytes, uint64_t pf_len, const uint64_t* checker,
                        const uint32_t* tf, uint64_t n, int device, aix_index_t** out);
int aix_index_create_13(const void* pf_bytes, uint64_t pf_len, const uint64_t* tf /* 4^13 or NULL */,
                        int device, aix_index_t** out);
int aix_index_close(aix_index_t* h);                  /* ~AindexWrapper, python_wrapper.cpp:185-226 */
int aix_index_info(const aix_index_t* h, aix_info_t* info);
/* force the two-probe path even on an all-canonical index (A/B measurements) */
int aix_index_set_canonical_fastpath(aix_index_t* h, int enabled);
/* switch the 4-bit fingerprint filter of the MPHF records off/on (A/B measurements; answers are identical) */
int aix_index_set_fingerprint_filter(aix_index_t* h, int enabled);
/* switch the early-exit MPHF walk (presence masks: an absent key usually costs one record read) off/on */
int aix_index_set_early_exit(aix_index_t* h, int enabled);
/* Verification table of a 23-mer handle (built at open unless AIX_BUCKET_TABLE=0): one 128-byte line per probe holding
 * {code, tf, slot} of the keys filed under it, compared in-line — the hit of get_tf_value_23mer / get_kid_by_kmer
 * (python_wrapper.cpp:610-627, hash.hpp:700-716) and of lu_compressed_worker's probe (hash.cpp:993-1054) in ONE read instead of
 * three MPHF records + a key record; answers are identical with it on or off (A/B measurements, tests).
 * lanes: how many lanes share one bucket read (8, 4, 2, 1; 0 = keep). */
int aix_index_set_bucket_table(aix_index_t* h, int enabled, int lanes);
/* Absence filter in front of the verification table (lookups, coverage): a blocked Bloom filter of the filed keys, one cached
 * 8-byte read that answers most absent keys before the table is touched (AIX_BLOOM_BITS bits per key at open, default 16,
 * 0 = none). Off / on for A/B measurements; answers are identical. */
int aix_index_set_absence_filter(aix_index_t* h, int enabled);
/* Minimizer-keyed copy of the verification table, used by the streaming form of aix_count23_fixed*: every filed key once more,
 * grouped by the bucket of the minimizer of its 23-mer (the 15-mer with the smallest hash over both strands; offsets + entries,
 * 16 B per key + 4 B per bucket), so the ~7 consecutive windows of a read that share a minimizer read ONE bucket. EXPERIMENTAL:
 * built at open only with AIX_MINIMIZER_TABLE=1 (AIX_MINIMIZER_LOAD = mean keys per bucket, default 2); measured 6-12 % faster than
 * the hash-keyed probe at one key per bucket and slower at four, so it is not the default; off / on per handle for
 * A/B measurements; answers are identical (verification in the bucket; undecided windows are settled through the hash-keyed table). */
int aix_index_set_minimizer_table(aix_index_t* h, int enabled);
/* replace the tf table of a 13-mer handle (u64[4^13], mphf order, HOST pointer) */
int aix_index_set_tf_13(aix_index_t* h, const uint64_t* tf);
/* copy tf out (HOST pointer): 23 -> u32[n]; 13 -> u64[4^13] in mphf order
 * replaces get_13mer_tf_array / get_tf_by_index_13mer (python_wrapper.cpp:983-998) */
int aix_index_get_tf(const aix_index_t* h, void* out, uint64_t out_bytes);
/* copy the checker (stored 2-bit codes, u64[n]) out; get_kmer_by_kid / get_kmer_info (:718-755) */
int aix_index_get_checker(const aix_index_t* h, uint64_t* out, uint64_t n);

/* I1: replaces `compute_index <dat> <pf> <prefix> <threads> <mock>` (src/compute_index.cpp:34-72,
 * index_hash_pp / worker_for_fill_index src/hash.cpp:671-723,779-881): for every key i,
 * checker_out[mphf(key_i)] = 2-bit code, tf_out[mphf(key_i)] = counts[i] (counts NULL = mock, tf 0).
 * keys = n*23 ASCII bytes (the first column of the .dat), outputs are the .kmers.bin / .tf.bin images.
 * AIX_ERR_CONFLICT when two keys land in one slot or a slot >= n (reference: exit(12) / OOB write). */
int aix_index_scatter(const void* pf_bytes, uint64_t pf_len, const char* keys, const uint32_t* counts, uint64_t n,
                      int device, uint64_t* checker_out, uint32_t* tf_out);
/* the same for a SHARD of the key set (multi-GPU index construction): n_keys keys scatter into full-size
 * arrays of n_slots entries (zero where this shard wrote nothing); occupied_out = ceil(n_slots/32) words, bit h set
 * <=> slot h was written. The caller merges shards with sum(tf), max(checker) and detects cross-shard collisions as
 * overlapping occupied bits. AIX_ERR_CONFLICT (collision inside the shard) still fills the outputs. */
int aix_index_scatter_shard(const void* pf_bytes, uint64_t pf_len, const char* keys, const uint32_t* counts, uint64_t n_keys,
                            uint64_t n_slots, int device, uint64_t* checker_out, uint32_t* tf_out, uint32_t* occupied_out);
/* the same scatter from 2-bit codes already in HBM, keeping the result resident as a 23-mer handle */
int aix_index_build_23_codes_dev(const void* pf_bytes, uint64_t pf_len, const uint64_t* d_codes,
                                 const uint32_t* d_counts /* nullable */, uint64_t n, int device, void* stream,
                                 aix_index_t** out);

/* ------------------------------------------------------------------------------------------
 * Batch tf queries. `kmers` is N*k contiguous ASCII bytes (k = 23 or 13 per the handle).
 * 23-mer handle: AindexWrapper::get_tf_values / get_tf_values_23mer / get_tf_value_23mer
 *   (python_wrapper.cpp:610-627,653-664,1219-1228) bit-exact incl. the raw-bytes forward probe /
 *   sanitised reverse probe asymmetry for non-ACGT bytes and forward-strand precedence.
 * 13-mer handle: get_tf_values_13mer / get_tf_value_13mer (python_wrapper.cpp:482-503,938-980):
 *   strict upper-case ACGT else 0, forward strand only, u64 -> u32 truncation.
 * ------------------------------------------------------------------------------------------ */
int aix_tf_batch_ascii(aix_index_t* h, const char* kmers, uint64_t N, uint32_t* out);
int aix_tf_batch_ascii_dev(aix_index_t* h, const char* d_kmers, uint64_t N, uint32_t* d_out, void* stream);
/* Tests and profiling: what aix_tf_batch_ascii_dev's binned path (large absent-heavy batches on a canonical index, AIX_LOOKUP_BINNED)
 * has done on this handle so far. Synchronises. out = pieces binned, pieces answered directly, records that overflowed their bin,
 * queries that reached the survivor probe. */
int aix_lookup_binned_stats(aix_index_t* h, uint64_t out[4]);
/* The same for pass B's coarse filter image (AIX_LOOKUP_COARSE): out = records tested against the image of their slice in LDS, records
 * that went on to the filter word. Both stay as they are where pass B runs without the image. Synchronises. */
int aix_lookup_binned_coarse_stats(aix_index_t* h, uint64_t out[2]);
/* pre-encoded 2-bit codes (first base most significant; ACGT only), same answers as the ASCII call */
int aix_tf_batch_codes(aix_index_t* h, const uint64_t* codes, uint64_t N, uint32_t* out);
int aix_tf_batch_codes_dev(aix_index_t* h, const uint64_t* d_codes, uint64_t N, uint32_t* d_out, void* stream);
/* variable-length queries: query i = bytes[offsets[i] .. offsets[i+1]). Mirrors what the reference
 * does with a std::string of any length (hash of ALL bytes, code of the first k); lengths < k give 0
 * (the reference reads past the string there). 23-mer handles only for len != k semantics; a 13-mer
 * handle returns 0 unless len == 13 (python_wrapper.cpp:943-946). */
int aix_tf_batch_ragged(aix_index_t* h, const char* bytes, const uint64_t* offsets, uint64_t N, uint32_t* out);
int aix_tf_batch_ragged_dev(aix_index_t* h, const char* d_bytes, const uint64_t* d_offsets, uint64_t N,
                            uint32_t* d_out, void* stream);

/* instrumentation for the roofline accounting: d_out[i] = MPHF + key records that tf query i reads (23-mer handles) */
int aix_lines_batch_ascii_dev(aix_index_t* h, const char* d_kmers, uint64_t N, uint32_t* d_out, void* stream);
/* get_hash_values / get_hash_value (python_wrapper.cpp:629-642): raw mphf::lookup of the bytes. On a 13-mer handle: the
 * value of hasher_13mer.lookup (:1087, used by get_positions_13mer) — the reference crashes there (hash_map is null). */
int aix_hash_batch_ascii(aix_index_t* h, const char* kmers, uint64_t N, uint64_t* out);
int aix_hash_batch_ascii_dev(aix_index_t* h, const char* d_kmers, uint64_t N, uint64_t* d_out, void* stream);
/* get_kid_by_kmer (:700-716; 0 when absent) and get_strand (:726-742; 0 absent,1 fwd,2 rc) */
int aix_kid_strand_batch_ascii(aix_index_t* h, const char* kmers, uint64_t N, uint64_t* kid_out /* nullable */,
                               uint8_t* strand_out /* nullable */);
int aix_kid_strand_batch_ascii_dev(aix_index_t* h, const char* d_kmers, uint64_t N, uint64_t* d_kid,
                                   uint8_t* d_strand, void* stream);
/* get_tf_both_directions_{23,13}mer_batch (:594-608,1259-1286) and, summed, get_total_tf_values_*
 * (:548-562,1230-1257). Both directions are written as u64; either pointer may be NULL. */
int aix_tf_both_batch_ascii(aix_index_t* h, const char* kmers, uint64_t N, uint64_t* fwd_out, uint64_t* rc_out);
int aix_tf_both_batch_ascii_dev(aix_index_t* h, const char* d_kmers, uint64_t N, uint64_t* d_fwd,
                                uint64_t* d_rc, void* stream);
int aix_tf_total_batch_ascii(aix_index_t* h, const char* kmers, uint64_t N, uint64_t* out);
int aix_tf_total_batch_ascii_dev(aix_index_t* h, const char* d_kmers, uint64_t N, uint64_t* d_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Coverage. replaces AIndex.get_sequence_coverage (aindex/core/aindex.py:314-322) for M sequences:
 * sequence s = seqs[offs[s] .. offs[s+1]); for every window i of length k (k = handle's k):
 * out[out_offs[s] + i] = tf >= cutoff ? tf : 0, tf as aix_tf_batch_ascii would give for that window.
 * out_offs[s+1]-out_offs[s] must be >= max(0, len_s - k + 1).
 * ------------------------------------------------------------------------------------------ */
int aix_coverage_batch(aix_index_t* h, const char* seqs, const uint64_t* offs, uint64_t M, uint32_t cutoff,
                       uint32_t* out, const uint64_t* out_offs);
int aix_coverage_batch_dev(aix_index_t* h, const char* d_seqs, const uint64_t* d_offs, uint64_t M,
                           uint64_t total_bytes, uint32_t cutoff, uint32_t* d_out, const uint64_t* d_out_offs,
                           void* stream);

/* ------------------------------------------------------------------------------------------
 * Counting.
 * aix_count13: replaces Kmer13Counter (count_kmers13.cpp:113-161,194-272,358-388): every length-13
 *   window of upper-cased ACGT in every sequence adds 1 to counts[mphf13(window)] (forward strand).
 *   tf_out = u64[4^13] in mphf order — byte-identical to the reference's output file. The handle's
 *   own tf table is NOT modified. `_dev`: d_buf must be in PLAIN form (one sequence per line, any
 *   non-ACGT byte breaks a window); use aix_normalize_reads for FASTA/FASTQ.
 * aix_count23_fixed: histogram of 23-mer windows against the handle's fixed key set (what
 *   kmer_counter -> compute_index would store for these reads, restricted to keys in the index):
 *   window chars valid per count_kmers.cpp:71-88 (ACGTU any case), key = canonical per canon_mode,
 *   tf_out[slot] += 1 when checker[slot] == key. tf_out = u32[n]. Multi-GPU: each rank counts its
 *   shard, then all-reduce(sum) tf_out (aindex_amd/dist.py).
 * ------------------------------------------------------------------------------------------ */
int aix_count13(aix_index_t* h, const char* buf, uint64_t len, int format, uint64_t* tf_out);
int aix_count13_dev(aix_index_t* h, const char* d_plain, uint64_t len, uint64_t* d_tf_out, void* stream);
int aix_count23_fixed(aix_index_t* h, const char* buf, uint64_t len, int format, int canon_mode, uint32_t* tf_out);
int aix_count23_fixed_dev(aix_index_t* h, const char* d_plain, uint64_t len, int canon_mode,
                          uint32_t* d_tf_out /* accumulated into, caller zeroes */, void* stream);
/* Streaming ingestion: the counters fed from a FILE, as the reference's tools are (count_kmers13.cpp:166-183,211-272,277-350: a reader
 * thread pushes sequences while the workers count). The file is read part by part (AIX_INGEST_PART_MB, default 256) by several host
 * threads into pinned staging, crosses the link on a copy stream while the previous part is normalised (FASTA / FASTQ readers as above,
 * their state handed from part to part, so parts are cut at any byte) and counted; HBM use is O(part), the host never holds the file.
 * Results are identical to the buffer forms. The host-buffer forms above (aix_count13, aix_count23_fixed, aix_count_distinct) run the same
 * pipeline from caller memory.
 * aix_count13_file: tf (u64[4^13], mphf order) is written to out_path (the file `count_kmers13 <in> <pf> <out>` writes,
 *   count_kmers13.cpp:358-388) and / or copied to tf_out (either may be NULL, not both).
 * stats (nullable) reports what the call did. */
typedef struct {
    uint64_t bytes_in;         /* bytes read from the file / buffer                                        */
    uint64_t plain_bytes;      /* bytes of PLAIN form that were counted                                    */
    uint64_t parts;            /* parts the input was cut into                                             */
    uint64_t part_bytes;       /* size of a part                                                           */
    uint64_t pieces;           /* K1: pieces whose distinct sets were merged                               */
    uint64_t pinned_bytes;     /* pinned host staging held by the call                                     */
    uint64_t device_bytes;     /* HBM held by the call: part staging + PLAIN part / piece + result (NOT the index, NOT the workspace)   */
    uint64_t workspace_bytes;  /* the handle's counting workspace after the call (grow-only, sized by the largest part it has seen)      */
    double seconds_total;      /* wall clock of the call                                                   */
    double seconds_read;       /* file / page cache -> pinned staging (sum over parts, overlapped)         */
    double seconds_wait;       /* the consumer waited for a part to arrive                                 */
    double seconds_h2d;        /* the parts on the link (HIP events around every copy, summed; the last three parts are not counted) */
    double seconds_normalise;  /* FASTA / FASTQ parts: the transducer pass (waits for the part to arrive included) */
    double seconds_compute;    /* counting as seen by the host (includes the waits inside)                 */
    double seconds_output;     /* result download + file write                                             */
} aix_ingest_stats_t;
/* Pin the staging blocks of a streaming call in the background and return at once (optional): a process that streams ONE file — a tool run —
 * calls this before it opens its index, so that the ~100 ms of page pinning overlap the index load instead of delaying the first part.
 * Staging blocks are kept between calls (AIX_PINNED_CACHE_MB, default 1024; aix_scratch_trim() frees them). */
int aix_ingest_warm(int device);
int aix_count13_file(aix_index_t* h, const char* path, int format, const char* out_path /* nullable */, uint64_t* tf_out /* nullable */,
                     aix_ingest_stats_t* stats);
int aix_count23_fixed_file(aix_index_t* h, const char* path, int format, int canon_mode, uint32_t* tf_out /* u32[n] */, aix_ingest_stats_t* stats);
/* K1 front end: replaces OptimizedKmerCounter's window loop (count_kmers.cpp:93-136,297-308) on a
 * PLAIN buffer in HBM: d_codes[p] = canonical 2-bit code of the k-window starting at byte p
 * (chars valid per count_kmers.cpp:71-88: ACGTU any case; canon_mode as above), or ~0 when the
 * window contains any other byte. d_codes holds len-k+1 entries. Distinct k-mers and their counts are
 * the sort + run-length of the valid entries (aindex_amd/counting.py). 1 <= k <= 32. */
int aix_window_codes_dev(const char* d_plain, uint64_t len, int k, int canon_mode, uint64_t* d_codes, void* stream);
/* A1 + A2: replaces `compute_aindex <reads> <pf> <prefix> <threads> 23 <tf> <kmers.bin> <kmers.txt>`
 * (src/compute_aindex.cpp:28-116): indices_out[n+1] = exclusive prefix sum of tf (AIndexCompressed ctor,
 * src/hash.hpp:365-399) = the .indices.bin image; positions_out[indices[n]] = the .index.bin image:
 * for every 23-byte window of the `.reads` buffer without '\n', '~', 'N', probing only the numerically smaller
 * strand, positions[indices[h] + slot] = offset + 1 for the first tf[h] occurrences in ascending offset order —
 * the result of the reference run with ONE thread (lu_compressed_worker, src/hash.cpp:960-1060; its multi-thread
 * slot order is schedule dependent). positions_out may be NULL to query *total_out = indices[n] first.
 * Any length: buffers of more than 2^30 windows are filled piece by piece, per-bucket fill counters carried over.
 *
 * 13-mer handles (N3: replaces `compute_aindex13 <reads> <pf> <tf> <prefix> <threads>`, src/compute_aindex13.cpp:36-71,
 * 109-226,298-321): n = 4^13 buckets in MPHF order, tf = the handle's u64[4^13] table (what count_kmers13 writes), a window
 * counts iff its 13 bytes are upper-case A/C/G/T, forward strand only, same slot rule and start adjustment. The reference tool
 * itself reads the u64 tf file as u32[4^13] (compute_aindex13.cpp:46-47) and therefore indexes a scrambled table; handing this
 * entry point that misread view (widened to u64) reproduces the reference's files bit for bit, which is how the path is pinned
 * (tests/golden/aindex13). All positions entry points below accept 13-mer handles in the same way; a 13-mer table with an entry
 * above 2^32 - 1 is AIX_ERR_UNSUPPORTED (the per-bucket fill counters are 32 bits wide; the reference's are u64 fetch_adds). */
int aix_positions_fill(aix_index_t* h, const char* reads, uint64_t len, uint64_t* indices_out, uint64_t* positions_out,
                       uint64_t positions_cap, uint64_t* total_out);
/* device-resident twin (reads, indices and positions in HBM; returns after the fill has completed on `stream`):
 * aix_positions_total gives indices[n] = the size of d_positions_out; `start` is aix_positions_start() of the buffer
 * (only the caller holds its head in host memory). */
int aix_positions_total(aix_index_t* h, uint64_t* total_out);
int aix_positions_fill_dev(aix_index_t* h, const char* d_reads, uint64_t len, uint64_t start, uint64_t* d_indices_out,
                           uint64_t* d_positions_out, uint64_t positions_cap, void* stream);
/* A2 over SHARDS of the reads file (multi-GPU). Shards are cut after '\n' (no window spans a cut).
 * aix_positions_bucket_counts: counts_out[h] (u64[n]) = windows of this shard that fall into bucket h under A2's rules;
 * aix_positions_fill_shard: the fill of this shard alone, with bucket h's slot numbering starting at filled_init[h]
 * (= occurrences in all EARLIER shards, clamped to 2^32-1; NULL = zeros) and offsets reported as base_offset + local
 * offset + 1. positions_out is the FULL-size array (indices[n] entries); entries this shard does not own are zero, so
 * the shards combine by addition. first_shard != 0 applies the reference's start adjustment (hash.cpp:973-986), which
 * only the beginning of the file sees. The union over shards equals aix_positions_fill of the whole file. */
int aix_positions_bucket_counts(aix_index_t* h, const char* reads, uint64_t len, int first_shard, uint64_t* counts_out);
/* the start adjustment itself (host only): first window offset the reference's single worker looks at. A shard whose
 * adjusted start is >= its window count has no clean window, and the adjustment carries on into the next shard. */
int aix_positions_start(const char* reads, uint64_t len, uint64_t* start_out);
int aix_positions_start_k(const char* reads, uint64_t len, int k /* 23 or 13 */, uint64_t* start_out);
int aix_positions_fill_shard(aix_index_t* h, const char* reads, uint64_t len, int first_shard, uint64_t base_offset,
                             const uint32_t* filled_init, uint64_t* positions_out, uint64_t positions_cap);
/* Device-resident twins of the SHARD entry points (one process per GPU; the partial results stay in HBM for the RCCL collectives
 * of aindex_amd/dist.py: scatter_sharded_t, positions_fill_sharded_t). d_* are device pointers; `start` is
 * aix_positions_start_k() of the shard's head (0 unless the shard is the first one that holds a clean window);
 * aix_positions_fill_shard_dev writes into a caller-zeroed FULL-size positions array (indices[n] entries). */
int aix_index_scatter_shard_codes_dev(const void* pf_bytes, uint64_t pf_len, const uint64_t* d_codes, const uint32_t* d_counts /* nullable */,
                                      uint64_t n_keys, uint64_t n_slots, int device, void* stream, uint64_t* d_checker_out, uint32_t* d_tf_out,
                                      uint32_t* d_occupied_out /* ceil(n_slots / 32) words */);
int aix_positions_indices_dev(aix_index_t* h, uint64_t* d_indices_out /* n + 1 */, void* stream);
int aix_positions_bucket_counts_dev(aix_index_t* h, const char* d_reads, uint64_t len, uint64_t start, uint64_t* d_counts_out /* n, zeroed here */,
                                    void* stream);
int aix_positions_fill_shard_dev(aix_index_t* h, const char* d_reads, uint64_t len, uint64_t start, uint64_t base_offset,
                                 const uint32_t* d_filled_init /* n, nullable */, const uint64_t* d_indices /* n + 1 */,
                                 uint64_t* d_positions /* indices[n], zeroed by the caller */, void* stream);
/* K1 complete: replaces `kmer_counter <in.fa> <k> <out> [-t N] [-m min]` (src/count_kmers.cpp:235-382): the set of
 * (canonical k-mer code, count) with count >= min_count, sorted by code ascending (the reference sorts by count with
 * unspecified tie order; parity is on the set). *keys_out / *counts_out are malloc'd (aix_free). format as for the
 * counters (FASTA records follow count_kmers.cpp:250-295). 1 <= k <= 31; any length (buffers of more
 * than 2^30 windows are counted piece by piece and the sorted distinct sets MERGED, never re-sorted — count_kmers.cpp:334-341 merges its
 * per-thread maps once; counts and sizes are 64-bit). */
int aix_count_distinct(const char* buf, uint64_t len, int format, int k, int canon_mode, uint64_t min_count, int device,
                       uint64_t** keys_out, uint64_t** counts_out, uint64_t* n_out);
/* the same from a file, streamed (see aix_count13_file): pieces of 2^30 windows are counted as the parts arrive, their sorted sets merged */
int aix_count_distinct_file(const char* path, int format, int k, int canon_mode, uint64_t min_count, int device, uint64_t** keys_out,
                            uint64_t** counts_out, uint64_t* n_out, aix_ingest_stats_t* stats);
/* device-resident twin: d_plain is a PLAIN buffer in HBM; the (key, count) arrays stay in HBM inside *out until the caller
 * has sized its own arrays (aix_distinct_size) and copied them (aix_distinct_copy_dev: u64 keys ascending, u64 counts). */
typedef struct aix_distinct aix_distinct_t;
int aix_count_distinct_dev(const char* d_plain, uint64_t len, int k, int canon_mode, uint64_t min_count, int device, void* stream,
                           aix_distinct_t** out);
/* K1 across GPUs: (key, count) pairs with repeated keys (what a rank holds after the all-to-all by key owner) -> the same kind
 * of result object: keys ascending, counts of equal keys summed, counts >= min_count. Pairs in any order (sort + reduce-by-key). */
int aix_merge_counts_dev(const uint64_t* d_keys, const uint64_t* d_counts, uint64_t n, uint64_t min_count, int device, void* stream,
                         aix_distinct_t** out);
/* the same when the caller can name its runs: run r = entries [run_offsets[r], run_offsets[r + 1]) (HOST array of nruns + 1 offsets), each run
 * sorted by key and free of repeats — after the exchange a rank holds one such run per peer, as the reference's merge holds one map per
 * thread (count_kmers.cpp:334-341). A tree of two-way merges with summation; nothing is sorted, any size. */
int aix_merge_runs_dev(const uint64_t* d_keys, const uint64_t* d_counts, const uint64_t* run_offsets, uint32_t nruns, uint64_t min_count, int device,
                       void* stream, aix_distinct_t** out);
int aix_distinct_size(const aix_distinct_t* r, uint64_t* n_out);
int aix_distinct_copy_dev(const aix_distinct_t* r, uint64_t* d_keys, uint64_t* d_counts, void* stream);
void aix_distinct_free(aix_distinct_t* r);
/* Host-side record normalisation to PLAIN form (readers of count_kmers13.cpp:211-272 /
 * count_kmers.cpp:250-295): out must hold len+1 bytes; *out_len receives the normalised length.
 * fasta_mode: 0 = count_kmers13 rules, 1 = kmer_counter rules ('>' anywhere starts a record). */
int aix_normalize_reads(const char* buf, uint64_t len, int format, int fasta_mode, char* out, uint64_t* out_len);
int aix_detect_format(const char* buf, uint64_t len);  /* count_kmers13.cpp:194-206 */
/* Replaces the binary `compute_reads <file1> <file2|-> <fastq|fasta|se|reads> <prefix>` (src/compute_reads.cpp:20-216), host side (text
 * reformatting bound by file I/O: no device work, runs without a GPU): writes <prefix>.reads (a pair as R1~revcomp(R2), revcomp =
 * get_revcomp of kmers.cpp:310-330: anything but ACGT becomes N), <prefix>.ridx ("rid\tstart\tend") and, for FASTA, <prefix>.header
 * ("name\tstart\tlength"); mode "reads" only indexes an existing reads file. file2 is read in mode "fastq" only.
 * AIX_ERR_ARG: unknown mode; AIX_ERR_IO: a file cannot be read / written. */
int aix_compute_reads(const char* file1, const char* file2 /* nullable */, const char* mode, const char* prefix);
/* The tools' text files, host side (native: the files hold 10^7..10^9 lines).
 * aix_dat_load: the .dat of compute_index ("kmer<ws>tf" per line; worker_for_fill_index, src/hash.cpp:681-702: a missing or unreadable
 *   count reads as 0, one beyond u32 as its maximum; mock != 0: k-mers only). Every k-mer must be 23 characters (AIX_ERR_FORMAT), empty
 *   lines are skipped. *keys_out = n * 23 bytes, *tf_out = n counts (not written when mock); malloc'd, release with aix_free.
 * aix_pf_build_file: compute_mphf_seq <keys.txt> (compute_mphf_generic.hpp:21-30): one key per line -> aix_pf_build_ragged.
 * aix_kmers_write_text: the list kmer_counter writes (count_kmers.cpp:362-382), "KMER\tcount\n" per entry in the order given. */
int aix_dat_load(const char* path, int mock, uint64_t* n_out, char** keys_out, uint32_t** tf_out /* nullable when mock */);
int aix_pf_build_file(const char* keys_path, void** pf_out, uint64_t* pf_len);
int aix_kmers_write_text(const char* path, const uint64_t* keys, const uint64_t* counts, uint64_t n, int k);
/* A binary image to a file (the .index.bin / .indices.bin / .kmers.bin / .tf.bin the tools write: compute_aindex.cpp hash.hpp:470-486,
 * compute_index.cpp:59-67), through a mapping filled by several host threads. AIX_ERR_IO when the file cannot be created or written. */
int aix_file_write(const char* path, const void* data, uint64_t bytes);
/* The .ridx file ("rid\tstart\tend" per read) that compute_reads writes and AindexWrapper::load_reads_index reads back
 * (python_wrapper.cpp:261-279: `fin >> rid >> start >> end` until it fails). *out = 3 * n values, malloc'd (aix_free). */
int aix_ridx_load(const char* path, uint64_t* n_out, uint64_t** out);

/* ------------------------------------------------------------------------------------------
 * Batch position queries: N k-mers -> every occurrence (CSR), optionally with read id and offset in the read.
 * replaces, N at a time, AindexWrapper::get_positions / get_positions_13mer (python_wrapper.cpp:800-831, 1070-1100) with the
 *          strand rule of PHASH_MAP::get_pfid (hash.hpp:150-170), and get_rid / get_start (python_wrapper.cpp:757-789) over
 *          IntervalTree::query (:66-74); aindex.py:333-341 (get_rid2poses) and :162-166 (get_reads_by_kmer) loop over those.
 * The positions index is attached to the handle first and stays in HBM. All entry points accept 23- and 13-mer handles.
 * ------------------------------------------------------------------------------------------ */
/* The .indices.bin (n + 1 offsets) and .index.bin (`total` entries) images that AindexWrapper::load_aindex maps
 * (python_wrapper.cpp:361-402), copied to HBM. Checked on the device: indices[0] == 0, ascending, indices[n] <= total, else
 * AIX_ERR_FORMAT. AIX_ERR_NOMEM when the copy does not fit (nothing is kept; an earlier attachment stays). Replaces an earlier attachment. */
int aix_aindex_attach(aix_index_t* h, const uint64_t* indices, const uint64_t* positions, uint64_t total);
/* The same (python_wrapper.cpp:361-402) for images already in HBM, e.g. the outputs of aix_positions_fill_dev: borrowed, the caller keeps
 * them alive until detach / close. The same check runs on `stream`; the call returns after it. */
int aix_aindex_attach_dev(aix_index_t* h, const uint64_t* d_indices, const uint64_t* d_positions, uint64_t total, void* stream);
/* Drops the positions index and the read intervals (the reference unmaps in ~AindexWrapper, python_wrapper.cpp:160-226);
 * aix_index_close does the same. */
int aix_aindex_detach(aix_index_t* h);
/* The intervals of a .ridx file (aix_ridx_load layout: rid, start, end per read; AindexWrapper::load_reads_index,
 * python_wrapper.cpp:261-279). Host only, no device needed: 1 if every end >= start and every start > the end before it —
 * what compute_reads writes — so that the first match of IntervalTree::query (:66-74) can be found by bisection; else 0. */
int aix_ridx_sorted_disjoint(const uint64_t* triples, uint64_t n_reads);
/* Puts such intervals (python_wrapper.cpp:261-279) into HBM for aix_positions_query* / aix_positions_locate*: AIX_OK and
 * aix_info_t::ridx_on_device = 1. Intervals that are not sorted and disjoint: AIX_ERR_UNSUPPORTED, nothing attached (the caller resolves
 * reads on the host). */
int aix_ridx_attach(aix_index_t* h, const uint64_t* triples, uint64_t n_reads);
/* get_positions (python_wrapper.cpp:800-831 / 1070-1100) for N k-mers of the handle's k (N * k bytes, host): list i =
 * (*positions_out)[(*offsets_out)[i] .. (*offsets_out)[i + 1]) = the non-zero entries of positions[indices[h] .. min(indices[h + 1], total))
 * minus one, in slot order, cut to the first max_per_kmer entries (0: all). 23-mers: h by get_pfid (hash.hpp:150-170), empty unless
 * h < n and checker[h] is the code of the strand looked up; 13-mers: exactly 13 upper-case A/C/G/T, forward strand. rid_out / local_out
 * (both or neither; need aix_ridx_attach): per entry get_rid(pos) and pos - get_start(pos) (python_wrapper.cpp:757-789; 0 and pos when
 * no interval matches). The outputs are malloc'd (aix_free); N = 0 gives offsets = {0}. AIX_ERR_ARG when nothing is attached. */
int aix_positions_query(aix_index_t* h, const char* kmers, uint64_t N, uint64_t max_per_kmer, uint64_t** offsets_out,
                        uint64_t** positions_out, uint64_t** rid_out /* nullable */, uint64_t** local_out /* nullable */);
/* device-resident twin of the above (python_wrapper.cpp:800-831). d_kmers: N * k bytes; d_offsets (N + 1) and *total_out (host) =
 * offsets[N] are always filled; the entries are written only if *total_out <= cap (entries each of d_positions / d_rid / d_local hold),
 * never at or beyond cap, and the call returns AIX_OK either way: size with cap = 0, then call again (the convention of
 * aix_positions_fill with positions_out == NULL). Returns after the work has completed on `stream`. */
int aix_positions_query_dev(aix_index_t* h, const char* d_kmers, uint64_t N, uint64_t max_per_kmer, uint64_t* d_offsets,
                            uint64_t* d_positions, uint64_t* d_rid /* nullable */, uint64_t* d_local /* nullable */, uint64_t cap,
                            uint64_t* total_out, void* stream);
/* get_rid / get_start (python_wrapper.cpp:757-789) for N arbitrary positions: the first interval in file order with
 * start <= pos + 1 and end + 1 >= pos (:66-74); rid = start = 0 when there is none (also beyond the file). Needs aix_ridx_attach
 * (AIX_ERR_ARG otherwise). The _dev twin is asynchronous on `stream`. */
int aix_positions_locate(aix_index_t* h, const uint64_t* pos, uint64_t N, uint64_t* rid_out, uint64_t* start_out);
int aix_positions_locate_dev(aix_index_t* h, const uint64_t* d_pos, uint64_t N, uint64_t* d_rid_out, uint64_t* d_start_out, void* stream);
/* ------------------------------------------------------------------------------------------
 * Batch read retrieval: the reads file in HBM, spans / read ids / k-mers -> the reads' bytes (CSR).
 * replaces, N at a time, AindexWrapper::get_read_by_rid (python_wrapper.cpp:666-675), get_read (:677-698) and
 *          get_reads_se_by_kmer (:857-911); aindex.py:162-166 (get_reads_by_kmer) and iter_reads loop over those.
 * Outputs are CSR: offsets[N + 1] into bytes laid back to back, no separators. The _dev twins follow the sizing convention of
 * aix_positions_query_dev: offsets and the totals are always produced, the rest only when it fits the caps, nothing is written at or
 * beyond a cap; they return after the work has completed on `stream`. Host outputs are malloc'd (aix_free).
 * ------------------------------------------------------------------------------------------ */
/* The .reads image that AindexWrapper::load_reads maps (python_wrapper.cpp:281-322: reads separated by '\n', mates by '~'), copied to
 * HBM; aix_info_t::device_bytes grows by len. AIX_ERR_NOMEM when it does not fit (nothing is kept; an earlier attachment stays).
 * Replaces an earlier attachment. */
int aix_reads_attach(aix_index_t* h, const char* reads, uint64_t len);
/* The same (python_wrapper.cpp:281-322) for a buffer already in HBM: borrowed, the caller keeps it alive until detach / close. Waits for
 * `stream` first. */
int aix_reads_attach_dev(aix_index_t* h, const char* d_reads, uint64_t len, void* stream);
/* Drops the reads (the reference unmaps in ~AindexWrapper, python_wrapper.cpp:160-226); aix_index_close does the same.
 * aix_aindex_detach leaves the reads attached. */
int aix_reads_detach(aix_index_t* h);
/* out = {0 nothing / 1 copied / 2 borrowed, bytes} of the attached reads (reads_size of python_wrapper.cpp:281-322). */
int aix_reads_info(const aix_index_t* h, uint64_t out[2]);
/* get_read (python_wrapper.cpp:677-698) for N (start, end, revcomp) triples: item i is empty when start >= size || end >= size ||
 * start > end (a span that ends AT the file size is empty, as there), else the bytes [start, end); where revcomp[i] != 0 (revcomp may be
 * NULL: none) reversed with A <-> T and C <-> G, every other byte unchanged. AIX_ERR_ARG when no reads are attached. */
int aix_reads_fetch(aix_index_t* h, const uint64_t* start, const uint64_t* end, const uint8_t* revcomp /* nullable */, uint64_t N,
                    uint64_t** offsets_out, char** bytes_out);
/* device-resident twin (python_wrapper.cpp:677-698): d_offsets (N + 1) and *total_out (host) = offsets[N] always; d_bytes (cap bytes) only
 * when *total_out <= cap. */
int aix_reads_fetch_dev(aix_index_t* h, const uint64_t* d_start, const uint64_t* d_end, const uint8_t* d_revcomp /* nullable */, uint64_t N,
                        uint64_t* d_offsets, char* d_bytes, uint64_t cap, uint64_t* total_out, void* stream);
/* get_read_by_rid (python_wrapper.cpp:666-675) for N read ids: row rid of the intervals of aix_ridx_attach, bytes [start, end) clamped
 * to the attached buffer; empty when rid >= n_reads. Needs reads and intervals attached (AIX_ERR_ARG otherwise). */
int aix_reads_fetch_rid(aix_index_t* h, const uint64_t* rid, uint64_t N, uint64_t** offsets_out, char** bytes_out);
int aix_reads_fetch_rid_dev(aix_index_t* h, const uint64_t* d_rid, uint64_t N, uint64_t* d_offsets, char* d_bytes, uint64_t cap,
                            uint64_t* total_out, void* stream);   /* python_wrapper.cpp:666-675, sizing as aix_reads_fetch_dev */
/* What get_reads_se_by_kmer (python_wrapper.cpp:857-911) intends, for N k-mers of the handle's k: for k-mer i the reads that hold one of
 * its indexed occurrences (aix_positions_query order: slot order), each read once at its first occurrence; occurrences without an interval
 * are skipped, empty reads are skipped and do not count, and the limit is tested after every distinct read met, so max_reads >= 1 keeps the
 * first max_reads reads and max_reads == 0 keeps the read of the first located occurrence. Any slot order inside a bucket is handled.
 * Reads of k-mer i: rid[kmer_offsets[i] .. kmer_offsets[i + 1]), read j's bytes at bytes[read_offsets[j] .. read_offsets[j + 1]).
 * Needs the positions index, the intervals and the reads attached (AIX_ERR_ARG otherwise). */
int aix_reads_by_kmers(aix_index_t* h, const char* kmers, uint64_t N, uint64_t max_reads, uint64_t** kmer_offsets_out, uint64_t** rid_out,
                       uint64_t** read_offsets_out, char** bytes_out);
/* device-resident twin (python_wrapper.cpp:857-911): d_kmer_offsets (N + 1) and totals_out (host) = {reads R, bytes} always; d_rid (cap_reads)
 * and d_read_offsets (cap_reads + 1) only when R <= cap_reads, d_bytes (cap_bytes) only when that holds and bytes <= cap_bytes. */
int aix_reads_by_kmers_dev(aix_index_t* h, const char* d_kmers, uint64_t N, uint64_t max_reads, uint64_t* d_kmer_offsets, uint64_t* d_rid,
                           uint64_t* d_read_offsets, uint64_t cap_reads, char* d_bytes, uint64_t cap_bytes, uint64_t totals_out[2], void* stream);

/* ------------------------------------------------------------------------------------------
 * De Bruijn graph layer: the neighbours of 23-mers with their frequencies, and bounded walks along them.
 * replaces, N at a time, DEBRUJIN::print_next / print_prev (debrujin.cpp:30-75, 121-167) over PHASH_MAP::get_freq(uint64_t)
 *          (hash.hpp:123-140: forward strand, then the reverse complement; the forward strand wins).
 * 23-mer handles only (AIX_ERR_MODE otherwise). A k-mer is given either as a 46-bit code (get_dna23_bitset, first base most
 * significant; higher bits are ignored) or as 23 ASCII bytes sanitised as get_freq(std::string_view) does (hash.hpp:203-206,
 * kmers.cpp:12-40: every byte other than upper-case A/C/G/T contributes 0 bits): exactly one of the two pointers is non-NULL.
 * ------------------------------------------------------------------------------------------ */
#define AIX_DIR_NEXT 0      /* successors:   ((u << 2) | b) & (2^46 - 1), debrujin.cpp:34-37 */
#define AIX_DIR_PREV 1      /* predecessors: (u >> 2) | (b << 44),        debrujin.cpp:125-128 */
#define AIX_DIR_BOTH 2      /* aix_neighbours* only: record 2 i = next, 2 i + 1 = prev of k-mer i */
#define AIX_WALK_GREEDY 0   /* follow the best continuation whatever the degree */
#define AIX_WALK_UNITIG 1   /* stop where the path branches (out-degree > 1) or joins (in-degree of the successor > 1) */
#define AIX_STOP_MAX_STEPS 0
#define AIX_STOP_DEAD_END  1  /* no neighbour above the cutoff */
#define AIX_STOP_BRANCH    2
#define AIX_STOP_JOIN      3
#define AIX_STOP_LOOP      4  /* the next k-mer is the seed again (either strand) */
#define AIX_WALK_MAX_STEPS 1048576ull   /* bound of max_steps */
/* struct CONT (debrujin.hpp, filled by debrujin.cpp:30-75 / 121-167) as one 32-byte record: tf[b] = get_freq of neighbour b
 * (A, C, G, T), set to 0 where tf[b] <= cutoff when cutoff > 0 (:44-49, inclusive); sum in u32 arithmetic (:51); n = non-zero
 * tf[b] (:52-53); best_base (0..3) = the LAST base whose tf is >= the other three (the four overwriting ifs of :55-74: ties go
 * to the later letter, all-zero gives T) and best_tf its tf. best_ukmer is the neighbour code of best_base and is not stored. */
typedef struct {
    uint32_t tf[4];
    uint32_t n, sum, best_tf, best_base;
} aix_cont_t;
/* print_next / print_prev (debrujin.cpp:30-75, 121-167) for N k-mers (host pointers): out holds N records (dirs NEXT or PREV)
 * or 2 N (BOTH: k-mer i, direction d at 2 i + d). N = 0 is AIX_OK. */
int aix_neighbours(aix_index_t* h, const uint64_t* codes /* or NULL */, const char* ascii /* or NULL */, uint64_t N, int dirs,
                   uint32_t cutoff, aix_cont_t* out);
/* device-resident twin (debrujin.cpp:30-75, 121-167), asynchronous on `stream`. d_ascii: N * 23 bytes. */
int aix_neighbours_dev(aix_index_t* h, const uint64_t* d_codes /* or NULL */, const char* d_ascii /* or NULL */, uint64_t N, int dirs,
                       uint32_t cutoff, aix_cont_t* d_out, void* stream);
/* S bounded walks, each a chain of print_next (dir NEXT) or print_prev (dir PREV) steps (debrujin.cpp:30-75, 121-167; the
 * reference has no walk of its own). From cur = seed, at most max_steps (1 .. AIX_WALK_MAX_STEPS, else AIX_ERR_ARG) times:
 * C = CONT(cur, dir, cutoff); C.n == 0 stops with DEAD_END; in UNITIG mode C.n > 1 stops with BRANCH, and
 * CONT(C.best_ukmer, the opposite direction, cutoff).n > 1 with JOIN; min(next, revcomp(next)) == min(seed, revcomp(seed))
 * stops with LOOP; else the base of C.best_base ('A', 'C', 'G', 'T') and C.best_tf are appended and cur = C.best_ukmer.
 * No presence test is made on the seed. Outputs per seed i: out_len[i], out_stop[i] (AIX_STOP_*), out_last[i] = the last
 * cur, and rows of stride max_steps: out_bases[i * max_steps + j], out_tf[i * max_steps + j] for j < out_len[i] in the order
 * found (dir PREV: base 0 is the one left of the seed); a row is left untouched from out_len[i] on. out_tf and out_last may
 * be NULL. S * max_steps that no buffer can hold is AIX_ERR_NOMEM before anything is allocated; S = 0 is AIX_OK. This host form
 * uploads the caller's out_bases / out_tf rows before the kernel runs, so that what lies beyond a row's length comes back as it
 * was: twice the transfer of the padded outputs. */
int aix_walk(aix_index_t* h, const uint64_t* codes /* or NULL */, const char* ascii /* or NULL */, uint64_t S, int dir,
             uint64_t max_steps, uint32_t cutoff, int mode, uint8_t* out_bases, uint32_t* out_len, uint8_t* out_stop,
             uint32_t* out_tf /* nullable */, uint64_t* out_last /* nullable */);
/* device-resident twin (debrujin.cpp:30-75, 121-167), asynchronous on `stream`; the loop of every seed is bounded by max_steps. */
int aix_walk_dev(aix_index_t* h, const uint64_t* d_codes /* or NULL */, const char* d_ascii /* or NULL */, uint64_t S, int dir,
                 uint64_t max_steps, uint32_t cutoff, int mode, uint8_t* d_bases, uint32_t* d_len, uint8_t* d_stop,
                 uint32_t* d_tf /* nullable */, uint64_t* d_last /* nullable */, void* stream);

/* ------------------------------------------------------------------------------------------
 * De Bruijn compaction: all maximal unitigs of an index, once each, with their abundance, and the map k-mer -> (unitig, offset, strand).
 * (The reference has no counterpart; the notation is that of the layer above: next / prev, rc, canon(x) = min(x, rc x).)
 *
 * Handles. 23-mer handles whose every stored code is canonical (aix_info_t::canonical_only == 1). Any other 23-mer handle is
 * AIX_ERR_UNSUPPORTED (freq(x) and freq(rc x) differ there, the graph is not strand-symmetric), a 13-mer handle AIX_ERR_MODE, an empty
 * index AIX_ERR_UNSUPPORTED, as is one whose ports (2 kid + port) do not fit a 32-bit word (n > 2^31 - 4). A NULL pointer where one is
 * needed is AIX_ERR_ARG; AIX_ERR_NOMEM keeps nothing. All of these are decided before anything is allocated or launched.
 *
 * Nodes. The oriented 23-mer x is live iff canon(x) is a stored key with tf > cutoff (for every cutoff >= 0 exactly "non-zero after the
 * CONT cutoff rule"; a stored tf of 0 is dead). out(x) = the live members of {next(x, b)}, in(x) = the live members of {prev(x, b)}
 * = rc(out(rc x)).
 * Edges. x -> y is a unitig edge iff y in out(x), |out(x)| == 1, |in(y)| == 1 and canon(y) != canon(x); the last condition cuts
 * self-loops (a homopolymer is a linear unitig of one node) and hairpins (y == rc x). With x -> y, rc y -> rc x is an edge too. A node has
 * two ports — 0 = R, leaving in stored orientation; 1 = L, leaving as the reverse complement — with at most one link each, so the
 * components are simple paths and simple cycles, and they partition the live keys.
 * Spelling. A unitig of m k-mers is its first oriented k-mer plus the last base of each following one: m + 22 ASCII bases. Path: of its
 * two spellings the one whose first oriented k-mer has the smaller 46-bit code (m == 1: the stored key; m > 1: the two belong to
 * different nodes and never tie). Cycle: it starts at the node with the smallest stored code, in stored orientation, leaves through its R
 * port and spells m k-mers (the first k-mer is not repeated); circular = 1.
 * Order. Unitig ids 0 .. U - 1 ascend by the code of the first oriented k-mer of the spelling. These codes are distinct: the output is a
 * pure function of (key set, tf, cutoff) — not of the MPHF, the launch geometry or any probe switch.
 *
 * Outputs per stored kid (n each): kid_unitig (AIX_UNITIG_NONE if dead), kid_pos (the k-mer occupies bases [offsets[u] + pos,
 * offsets[u] + pos + 23)), kid_flag (bit 0: the stored key appears reverse-complemented in the spelling; bit 1: the unitig is circular);
 * dead kids get pos = 0 and flag = 0. Per unitig: offsets[U + 1], bases[offsets[U]], circular[U], and tf_sum / tf_min / tf_max over the
 * member tf. Optional: kmer_tf[n_live] in unitig order — k-mer j of unitig u sits at offsets[u] - 22 u + j: the coverage profile along
 * every unitig. A cutoff at which nothing is live gives U = 0 and offsets = {0}.
 * ------------------------------------------------------------------------------------------ */
#define AIX_UNITIG_NONE 0xFFFFFFFFFFFFFFFFull
/* The graph is analysed once, here: the three per-kid arrays, and the sizes the second call needs (*total_bases_out = offsets[U],
 * *n_live_out = the length of kmer_tf). Returns after its work on `stream` has completed. Scratch: see DESIGN 5i. */
int aix_unitigs_layout_dev(aix_index_t* h, uint32_t cutoff, uint64_t* d_kid_unitig, uint32_t* d_kid_pos, uint8_t* d_kid_flag,
                           uint64_t* n_unitigs_out, uint64_t* total_bases_out, uint64_t* n_live_out, uint64_t* n_circular_out, void* stream);
/* Spells the unitigs of a layout: d_offsets[U + 1], d_bases[total], d_circular / d_tf_sum / d_tf_min / d_tf_max [U], d_kmer_tf[n_live]
 * (nullable); nothing is written at or beyond these sizes. Member tf are read from the index; `cutoff` is only checked against the
 * layout: a live kid whose tf is <= cutoff — or any other disagreement between the arrays, U and the index — is AIX_ERR_ARG, with
 * nothing written. Returns after its work on `stream` has completed. */
int aix_unitigs_emit_dev(aix_index_t* h, uint32_t cutoff, const uint64_t* d_kid_unitig, const uint32_t* d_kid_pos, const uint8_t* d_kid_flag,
                         uint64_t U, uint64_t* d_offsets, uint8_t* d_bases, uint8_t* d_circular, uint64_t* d_tf_sum, uint32_t* d_tf_min,
                         uint32_t* d_tf_max, uint32_t* d_kmer_tf /* nullable */, void* stream);
/* Both calls for host memory: every array is malloc'd (aix_free). */
int aix_unitigs(aix_index_t* h, uint32_t cutoff, uint64_t* n_unitigs_out, uint64_t** offsets_out, uint8_t** bases_out, uint8_t** circular_out,
                uint64_t** tf_sum_out, uint32_t** tf_min_out, uint32_t** tf_max_out, uint32_t** kmer_tf_out /* nullable */,
                uint64_t** kid_unitig_out /* nullable */, uint32_t** kid_pos_out /* nullable */, uint8_t** kid_flag_out /* nullable */);

/* ------------------------------------------------------------------------------------------
 * The unitig graph: which unitig follows which (links between unitig ends), and simple two-armed bubbles.
 * (The reference has no counterpart; the notation is that of the compaction above.)
 *
 * Handles. Exactly those of aix_unitigs_layout_dev: a 23-mer handle with canonical_only == 1, else AIX_ERR_UNSUPPORTED; a 13-mer handle
 * AIX_ERR_MODE; an empty index AIX_ERR_UNSUPPORTED; NULL where a pointer is needed AIX_ERR_ARG. All of these are decided before anything
 * is allocated or launched. The call takes a layout (kid_unitig, kid_pos, kid_flag, U) and the offsets[U + 1] of the emit and validates
 * them first against the index and the cutoff, as the emit does, and against each other: every linear unitig has exactly one member at
 * position 0 and one at position m - 1, every member's position is below m. Any disagreement is AIX_ERR_ARG with no output array
 * written. No address outside the given sizes is read or written, whatever the arrays hold.
 *
 * Ends. A linear unitig u of m = offsets[u + 1] - offsets[u] - 22 k-mers has two ends: end 2 u + 0 ("u+") leaves the spelling at its
 * right end, through the last oriented k-mer x of the spelling; end 2 u + 1 ("u-") leaves it at its left end, through rc of the first
 * oriented k-mer. A circular unitig has no ends: its two entries have degree 0.
 * Links. The links of end e are the live members of {next(x, b), b = A, C, G, T}, in base order (live as in the layout: canon(y) stored
 * with tf > cutoff). Each link is one u32 word 2 v + r: v is the unitig of y; r = 0 if y appears in v's spelling as given — v is entered
 * at its position 0 and traversed forwards ("v+") — and r = 1 if y appears reverse-complemented — v is entered at position m_v - 1 and
 * traversed backwards ("v-"). Every link overlaps by exactly 22 bases.
 * A live successor y of a path end x is always the first k-mer of its unitig in the entering orientation, and that unitig is never
 * circular: a unitig edge z -> y needs |in(y)| == 1, so z == x, and x -> y would itself be a unitig edge. The call checks this for every
 * link; a violation is an inconsistent layout (AIX_ERR_ARG).
 * Duality. (e -> t) is a link iff (t ^ 1 -> e ^ 1) is one. Self-dual links exist: a hairpin end gives u+ -> u-; a homopolymer gives
 * u+ -> u+ and its dual u- -> u-.
 *
 * Outputs. link_off u64[2 U + 1], the exclusive prefix of the end degrees (0 .. 4 each); link_to u32[E], E = link_off[2 U] <= 8 U.
 * U = 0 gives link_off = {0} and E = 0. A pure function of (key set, tf, cutoff) — not of the MPHF, the launch geometry or any probe
 * switch.
 *
 * Simple bubbles. bubble_mate u32[U], AIX_BUBBLE_NONE for none. Linear unitig u is an arm with mate w iff
 *   deg(2 u) == deg(2 u + 1) == 1, with tR and tL those two link words;
 *   the source end f = tL ^ 1 has degree exactly 2, and its targets are {2 u + 0, x} with w = x >> 1 != u;
 *   the sink has in-degree exactly 2: deg(tR ^ 1) == 2;
 *   the other arm, traversed as x, is attached the same way and nowhere else: deg(x) == 1 and its link is tR, deg(x ^ 1) == 1 and its
 *   link is tL.
 * The relation is symmetric (mate[mate[u]] == u); a circular unitig never qualifies. Length and abundance thresholds ("a tip of at most
 * 2 k bases", "the weaker arm") are the caller's: one line over offsets, tf_sum and the degrees.
 * ------------------------------------------------------------------------------------------ */
#define AIX_BUBBLE_NONE 0xFFFFFFFFu
/* d_link_off[2 U + 1] and d_link_to[link_cap] (NULL allowed when link_cap == 0). If E > link_cap: AIX_ERR_ARG with *n_links_out = E,
 * d_link_off written and d_link_to untouched — a caller may size and repeat; 8 U always suffices. Returns after its work on `stream`
 * has completed. Scratch: see DESIGN 5j. */
int aix_unitig_links_dev(aix_index_t* h, uint32_t cutoff, const uint64_t* d_kid_unitig, const uint32_t* d_kid_pos, const uint8_t* d_kid_flag,
                         uint64_t U, const uint64_t* d_offsets, uint64_t* d_link_off, uint32_t* d_link_to, uint64_t link_cap,
                         uint64_t* n_links_out, void* stream);
/* d_bubble_mate[U] from d_link_off[2 U + 1] and d_link_to[E]; needs no handle (the current device). Every index read from the arrays is
 * checked against 2 U and E before it is used; E > 8 U or a NULL array is AIX_ERR_ARG. Returns after its work on `stream` has completed. */
int aix_unitig_bubbles_dev(uint64_t U, const uint64_t* d_link_off, const uint32_t* d_link_to, uint64_t E, uint32_t* d_bubble_mate, void* stream);
/* Layout, offsets, links and bubbles for host memory: every array is malloc'd (aix_free). */
int aix_unitig_links(aix_index_t* h, uint32_t cutoff, uint64_t* n_unitigs_out, uint64_t* n_links_out, uint64_t** link_off_out,
                     uint32_t** link_to_out, uint32_t** bubble_mate_out /* nullable */);

/* ------------------------------------------------------------------------------------------
 * Graph cleaning: clip tips, pop bubbles, and compact the surviving unitigs again into contigs.
 * (The reference has no counterpart; the notation is that of the two blocks above. tests/graph_clean_ref.py restates this block.)
 *
 * A unitig set G is (U, offsets u64[U + 1], bases u8[offsets[U]], circular u8[U], tf_sum u64[U], tf_min / tf_max u32[U],
 * link_off u64[2 U + 1], link_to u32[E]): what aix_unitigs_emit_dev and aix_unitig_links_dev write, and what the compaction below writes,
 * so the step can be applied to its own output. m_u = offsets[u + 1] - offsets[u] - 22; ends, link words 2 v + r and duality as above.
 * No call takes an index handle: they work on device arrays of the current device. All are asynchronous on `stream` and return after
 * their work on it has completed. Scratch comes from the pool and goes back on every path; AIX_ERR_NOMEM keeps nothing.
 *
 * Validation (every call, before anything is written; a violation is AIX_ERR_ARG with no output touched): offsets ascend by at least 23
 * per unitig; link_off starts at 0, ascends, ends at E, and no end has more than 4 links (so E <= 8 U); every link word is below 2 U; a
 * circular unitig has no link and is no link's target; every surviving link e -> t has its dual t ^ 1 -> e ^ 1 (mark: every link).
 * Every index read from an input array is checked against U, 2 U, E and offsets[U] before it is used. U > 2^31 - 4 is
 * AIX_ERR_UNSUPPORTED (an end must fit a 32-bit word). A NULL pointer where one is needed is AIX_ERR_ARG. The bases are taken to be
 * upper-case A, C, G, T (what the emit writes); this is not checked: a byte c counts as base ((c >> 1) ^ (c >> 2)) & 3 and is
 * complemented as c ^ (c & 2 ? 0x04 : 0x15).
 *
 * 1. Mark. remove u8[U]: 0 keep, 1 tip, 2 bubble arm. All decisions are taken from the input graph alone, in one round; the result does
 *    not depend on launch geometry.
 *    Outranks. w outranks u iff tf_sum_w m_u > tf_sum_u m_w (mean(w) > mean(u), compared exactly in 128-bit products), or the two
 *      products are equal and w < u. A strict total order.
 *    Tip candidate. A linear unitig with m_u <= tip_max_kmers, one end of degree 0 and the other end a of degree exactly 1.
 *    Tip removal. t = the single link of a, f = t ^ 1 (the end that faces u). u is removed iff f has another link x with x >> 1 != u
 *      whose unitig w = x >> 1 is no tip candidate, or is a candidate that outranks u. Where every sibling at a fork is a candidate,
 *      exactly one survives; a candidate whose fork has no other link survives.
 *    Bubble arm. u has the mate w = bubble_mate[u], m_u <= bubble_max_kmers, m_w <= bubble_max_kmers and w outranks u: exactly one arm
 *      of a qualifying bubble is removed. An arm has two ends of degree 1, so it is never a tip candidate. bubble_mate may be NULL (it is
 *      computed inside, aix_unitig_bubbles_dev); a given one must be symmetric with entries below U (AIX_ERR_ARG otherwise).
 *    A threshold of 0 switches its rule off; a threshold above 32767 is AIX_ERR_ARG.
 *
 * 2. Compact. Takes G and any remove u8[U] (non-zero = removed), so callers may OR in masks of their own.
 *    Surviving links. A link survives iff neither of its unitigs is removed; deg'(e) counts the surviving links of end e.
 *    Merge edges. e -> t is a merge edge iff deg'(e) == 1, deg'(t ^ 1) == 1 and t >> 1 != e >> 1 — which cuts hairpins (u+ -> u-) and the
 *      self-loop of a homopolymer — with one exception: the link u+ -> u+ (t == e) of a unitig of m_u >= 2 k-mers is a merge edge and
 *      closes u on itself. (Its last and first k-mer are different nodes, so the k-mer rule of the compaction above links them too;
 *      without the exception property (b) below would fail on a ring whose stem was clipped.) With e -> t, t ^ 1 -> e ^ 1 is a merge edge
 *      too: components are simple paths and simple cycles of surviving unitigs. An input-circular unitig is a contig of its own and is
 *      passed through unchanged.
 *    Spelling. The first member is oriented and copied whole; every following oriented member contributes its bases from offset 22 on; a
 *      backwards member is reverse-complemented. A contig of members m_1 .. m_j has the sum of their k-mers; tf_sum is the sum, tf_min the
 *      minimum, tf_max the maximum of its members' values (there are no junction k-mers).
 *    Path. Of its two spellings the one whose first oriented 23-mer has the smaller 46-bit code (the rule of the compaction above); on a
 *      tie — possible only on input that is no compaction — the one whose first member has the smaller id, then the one that spells the
 *      members as given.
 *    Merged cycle. It starts at its member with the smallest unitig id, traversed forwards, and has circular = 1. This is NOT the
 *      smallest-stored-code rotation of the compaction above: finding that rotation would split a member. A caller who needs that form
 *      rotates on the host (tests/graph_clean_ref.py: canonical_form).
 *    Order. Contig ids 0 .. C - 1 ascend by the code of the first 23-mer of the spelling; ties (same remark) by the id of the first member.
 *    Map. unitig_contig u32[U] (AIX_BUBBLE_NONE if removed); unitig_pos u64[U]: the oriented spelling of the member occupies bases
 *      [offsets'[c] + pos, offsets'[c] + pos + m_u + 22) of its contig, so pos is the number of k-mers in front of it and its first
 *      contributed base is pos (first member) or pos + 22; unitig_flag u8[U]: bit 0 the member is reversed, bit 1 the contig is a merged
 *      cycle (an input-circular unitig keeps flag 0). Removed unitigs get pos 0 and flag 0.
 *    Links of G'. A circular contig has no ends. End 2 c + 0 / 2 c + 1 of a linear contig is the outward end of its last / first
 *      member; its links are the surviving links of that unitig end (none of them is a merge edge), in their original order, each word
 *      2 v + r rewritten to 2 contig(v) + (r ^ flag(v) & 1). That v is the member at that end of its contig is checked (AIX_ERR_ARG).
 *      Duality holds in G'.
 *    Properties. (a) With remove all zero on a G that aix_unitigs_emit_dev + aix_unitig_links_dev wrote, G' == G in every array and the
 *      map is the identity. (b) G' equals — up to the rotation and strand of merged circular contigs and the id order that follows from
 *      them — what those two calls return for an index that holds only the k-mers of the surviving unitigs.
 *    U == 0, or everything removed, gives C = 0, offsets' = {0}, link_off' = {0}.
 * ------------------------------------------------------------------------------------------ */
#define AIX_GRAPH_MAX_THRESHOLD 32767u
/* d_remove[U] and the two counts. d_bubble_mate[U] nullable. */
int aix_graph_mark_dev(uint64_t U, const uint64_t* d_offsets, const uint8_t* d_circular, const uint64_t* d_tf_sum, const uint64_t* d_link_off,
                       const uint32_t* d_link_to, uint64_t E, const uint32_t* d_bubble_mate /* nullable: computed inside when NULL */,
                       uint32_t tip_max_kmers, uint32_t bubble_max_kmers, uint8_t* d_remove, uint64_t* n_tips_out, uint64_t* n_arms_out, void* stream);
/* The graph is analysed once, here: the three map arrays [U], and the sizes the second call needs: C, offsets'[C], E' and the number of
 * circular contigs. Scratch: see DESIGN 5k. */
int aix_graph_compact_layout_dev(uint64_t U, const uint64_t* d_offsets, const uint8_t* d_bases, const uint8_t* d_circular, const uint64_t* d_link_off,
                                 const uint32_t* d_link_to, uint64_t E, const uint8_t* d_remove, uint32_t* d_unitig_contig, uint64_t* d_unitig_pos,
                                 uint8_t* d_unitig_flag, uint64_t* n_contigs_out, uint64_t* total_bases_out, uint64_t* n_links_out,
                                 uint64_t* n_circular_out, void* stream);
/* Writes G': d_out_offsets[C + 1], d_out_bases[total_bases], d_out_circular / tf_sum / tf_min / tf_max [C], d_out_link_off[2 C + 1],
 * d_out_link_to[n_links]; nothing is written at or beyond these sizes. The map is validated against (G, remove) and the three sizes
 * first: members of a contig follow each other without a gap, every merge edge joins neighbours in matching orientation, every other
 * end is a contig end; any disagreement is AIX_ERR_ARG with nothing written. d_bases must be aligned to 8 and d_out_bases to 16 bytes
 * (AIX_ERR_ARG): the emission loads and stores whole words. Input and output arrays must not overlap. */
int aix_graph_compact_emit_dev(uint64_t U, const uint64_t* d_offsets, const uint8_t* d_bases, const uint8_t* d_circular, const uint64_t* d_tf_sum,
                               const uint32_t* d_tf_min, const uint32_t* d_tf_max, const uint64_t* d_link_off, const uint32_t* d_link_to, uint64_t E,
                               const uint8_t* d_remove, const uint32_t* d_unitig_contig, const uint64_t* d_unitig_pos, const uint8_t* d_unitig_flag,
                               uint64_t C, uint64_t total_bases, uint64_t n_links, uint64_t* d_out_offsets, uint8_t* d_out_bases,
                               uint8_t* d_out_circular, uint64_t* d_out_tf_sum, uint32_t* d_out_tf_min, uint32_t* d_out_tf_max,
                               uint64_t* d_out_link_off, uint32_t* d_out_link_to, void* stream);
/* One round — mark, layout, emit — for host memory: G in host arrays, G', remove[U] and the map in malloc'd arrays (aix_free); the last
 * four outputs are nullable. */
int aix_graph_clean(uint64_t U, const uint64_t* offsets, const uint8_t* bases, const uint8_t* circular, const uint64_t* tf_sum, const uint32_t* tf_min,
                    const uint32_t* tf_max, const uint64_t* link_off, const uint32_t* link_to, uint64_t E, uint32_t tip_max_kmers,
                    uint32_t bubble_max_kmers, uint64_t* n_contigs_out, uint64_t* n_links_out, uint64_t* n_tips_out, uint64_t* n_arms_out,
                    uint64_t** offsets_out, uint8_t** bases_out, uint8_t** circular_out, uint64_t** tf_sum_out, uint32_t** tf_min_out,
                    uint32_t** tf_max_out, uint64_t** link_off_out, uint32_t** link_to_out, uint8_t** remove_out /* nullable */,
                    uint32_t** unitig_contig_out /* nullable */, uint64_t** unitig_pos_out /* nullable */, uint8_t** unitig_flag_out /* nullable */);

/* ------------------------------------------------------------------------------------------
 * Threading: the path of every sequence through a unitig or contig graph, and the number of sequences that traverse every link.
 * (The reference has no counterpart; the notation is that of the three blocks above. tests/seqthread_ref.py restates this block.)
 *
 * A k-mer map of a unitig set G is the three per-kid arrays of aix_unitigs_layout_dev read against G's offsets: kid_unitig u64[n]
 * (AIX_UNITIG_NONE: the kid has no place in G), kid_pos u32[n] (the k-mer occupies bases [offsets[u] + pos, offsets[u] + pos + 23)),
 * kid_flag u8[n] (bit 0: the stored key appears reverse-complemented in the spelling; bit 1: circular). m_u = offsets[u + 1] - offsets[u] - 22.
 *
 * 1. aix_graph_kidmap_dev carries a k-mer map of G through one compaction round to G': inputs the map on G, U and offsets[U + 1] of G,
 *    and unitig_contig / unitig_pos / unitig_flag [U] as aix_graph_compact_layout_dev wrote them; outputs the map on G'. The outputs may
 *    be the input arrays (every lane reads its own entry before it writes it). For a kid with (u, p, f):
 *      u == AIX_UNITIG_NONE or unitig_contig[u] == AIX_BUBBLE_NONE: dead — AIX_UNITIG_NONE, pos 0, flag 0;
 *      else unitig' = unitig_contig[u]; pos' = unitig_pos[u] + (unitig_flag[u] & 1 ? m_u - 1 - p : p);
 *           flag' bit 0 = (f ^ unitig_flag[u]) & 1; flag' bit 1 = ((f | unitig_flag[u]) >> 1) & 1.
 *    Validation, before anything is written (a violation is AIX_ERR_ARG with the outputs untouched): u < U; offsets[u + 1] >=
 *    offsets[u] + 23 and p < m_u; unitig_contig[u] is AIX_BUBBLE_NONE or below 2^31 - 4 (the limit of U'); pos' fits 32 bits. A NULL
 *    pointer where one is needed (offsets always; the kid arrays when n > 0; the unitig arrays when U > 0) is AIX_ERR_ARG, decided
 *    before anything is allocated or launched. No handle: the current device. n == 0 is AIX_OK.
 *
 * 2. aix_thread_nodes_dev packs a k-mer map into one word per kid, node u64[n]:
 *      node = unitig << 33 | pos << 2 | (flag & 3)      bits 63 .. 33 the unitig, bits 32 .. 2 the position, bits 1 .. 0 the flag
 *      node = 0xFFFFFFFFFFFFFFFF                          a dead kid (no unitig id reaches 2^31 - 1)
 *    Every entry is checked in the same pass: u < U, offsets[u + 1] >= offsets[u] + 23 and pos < m_u, else AIX_ERR_ARG with nothing
 *    written. U > 2^31 - 4, or a position of 2^31 or more, is AIX_ERR_UNSUPPORTED with nothing written. NULL pointers as in 1.
 *
 * 3. aix_seq_thread_dev. Handle: exactly those of aix_unitigs_layout_dev (23-mer, canonical_only == 1, not empty, n <= 2^31 - 4), with the
 *    same statuses. Sequences as aix_seq_hits_dev takes them: sequence i is the bytes d_seqs[d_offs[i] .. d_offs[i + 1]), offsets
 *    ascending, a sequence of 2^32 bytes or more is AIX_ERR_ARG; d_seqs may be NULL when no sequence is 23 bytes long. Graph: d_node[n]
 *    (n of the handle), U, d_offsets[U + 1], d_circular[U], d_link_off[2 U + 1], d_link_to[E] — a unitig set, or what the cleaning wrote,
 *    with the node words of its k-mer map.
 *    Validation, before anything is written (AIX_ERR_ARG with every output and link_support untouched): every node word is dead or
 *    names a unitig below U and a position below its m_u; offsets ascend by at least 23 per unitig; link_off starts at 0, ascends, ends
 *    at E, and no end has more than 4 links; E <= 8 U. U > 2^31 - 4 is AIX_ERR_UNSUPPORTED. Link words are not validated: they are only
 *    compared. Every index read from node, offsets, link_off and link_to is checked against n, U, 2 U and E before it is used; whatever
 *    the arrays hold, no address outside the given sizes is read or written.
 *    Windows. Sequence i of length L has max(0, L - 22) windows, window q the 23 bytes at offset q. A window has a node iff all 23 bytes
 *    are upper-case A, C, G, T, its canonical code is a stored key (whatever its tf), and node[kid] is not dead. Its node is (u, p, s)
 *    with u and p from the word and s = flag bit 0 xor (the window's code is not the canonical one): s = 0 the window reads the
 *    unitig's spelling forwards, s = 1 backwards. (k is odd: no window equals its own reverse complement.)
 *    Steps. A step is a maximal run of consecutive windows of one sequence that all have nodes and where each follows its predecessor:
 *    same u, same s, and p' = p + 1 (s = 0) or p' = p - 1 (s = 1); on a unitig with circular[u] != 0 the step is taken mod m_u, so a
 *    step may wind round it more than once. A linear unitig of one k-mer never continues. One record per step: step_unitig u32,
 *    step_pos u32 (the position of the first window), step_flag u8 (bit 0: traversed backwards; bit 1: circular[u] != 0), q_first and
 *    q_last u32 (its first and last window), step_link u64. CSR over sequences: the steps of sequence i are
 *    [seq_step_off[i], seq_step_off[i + 1]), ordered by q_first.
 *    step_link. AIX_THREAD_NO_LINK when the step is the first of its sequence or a window without a node lies between it and the step
 *    before. Else the two steps are adjacent (q_first == q_last of the previous step + 1) and the value is the index j into link_to of
 *    the link e -> t traversed: e = 2 u + s of the previous step's last window, which must sit at its exit (p == m_u - 1 for s = 0,
 *    p == 0 for s = 1); t = 2 v + s_v of this step's first window, which must sit at its entry (p == 0 for s_v = 0, p == m_v - 1 for
 *    s_v = 1); j is the first index in [link_off[e], link_off[e + 1]) with link_to[j] == t. Adjacent steps without such a link get
 *    AIX_THREAD_BROKEN: a value, not an error — it cannot occur when node map and links describe the same graph.
 *    Link support (d_link_support u64[E], nullable). For every step with a link index j, support[j] += 1, and support[j'] += 1 for
 *    its dual j' (the link t ^ 1 -> e ^ 1, found the same way) when it exists and j' != j; a hairpin u+ -> u- is its own dual and
 *    counts once. The array is accumulated, never zeroed: a caller adds batch after batch. The adds happen only in the call that writes
 *    the entries, so sizing first does not count twice. Starting from zero on a graph with duality, support[j] == support[dual j], and
 *    a batch and its reverse complement give the same array. Integer adds commute: the result does not depend on the launch geometry.
 *    Sizing, as aix_seq_hits_dev: d_seq_step_off[M + 1] and *total_out are always written; the entries, and the support, only when
 *    *total_out <= cap (entries each of the six step arrays hold; they may be NULL when cap == 0), never at or beyond cap; AIX_OK
 *    either way. M = 0 gives seq_step_off = {0}. The result is a pure function of (sequences, key set, node map, graph) — not of the
 *    MPHF, the launch geometry or any probe switch. Returns after its work on `stream` has completed. Scratch: see DESIGN 5l.
 *
 * The host form builds layout, emit, links and nodes of the unitig graph at `cutoff` inside (as aix_unitig_links does), threads host
 * sequences through it and returns malloc'd arrays (aix_free): seq_step_off[M + 1] and the six step arrays, optionally
 * link_support[E] counted from zero, U and E. Threading through contigs is a device-form feature.
 * ------------------------------------------------------------------------------------------ */
#define AIX_THREAD_NO_LINK 0xFFFFFFFFFFFFFFFFull
#define AIX_THREAD_BROKEN  0xFFFFFFFFFFFFFFFEull
int aix_graph_kidmap_dev(uint64_t n, const uint64_t* d_kid_unitig, const uint32_t* d_kid_pos, const uint8_t* d_kid_flag, uint64_t U,
                         const uint64_t* d_offsets, const uint32_t* d_unitig_contig, const uint64_t* d_unitig_pos, const uint8_t* d_unitig_flag,
                         uint64_t* d_out_unitig, uint32_t* d_out_pos, uint8_t* d_out_flag, void* stream);
int aix_thread_nodes_dev(uint64_t n, const uint64_t* d_kid_unitig, const uint32_t* d_kid_pos, const uint8_t* d_kid_flag, uint64_t U,
                         const uint64_t* d_offsets, uint64_t* d_node, void* stream);
int aix_seq_thread_dev(aix_index_t* h, const char* d_seqs, const uint64_t* d_offs, uint64_t M, const uint64_t* d_node, uint64_t U,
                       const uint64_t* d_offsets, const uint8_t* d_circular, const uint64_t* d_link_off, const uint32_t* d_link_to, uint64_t E,
                       uint64_t* d_link_support /* nullable */, uint64_t* d_seq_step_off, uint32_t* d_step_unitig, uint32_t* d_step_pos,
                       uint8_t* d_step_flag, uint32_t* d_q_first, uint32_t* d_q_last, uint64_t* d_step_link, uint64_t cap, uint64_t* total_out,
                       void* stream);
int aix_seq_thread(aix_index_t* h, uint32_t cutoff, const char* seqs, const uint64_t* offs, uint64_t M, uint64_t** seq_step_off_out,
                   uint32_t** step_unitig_out, uint32_t** step_pos_out, uint8_t** step_flag_out, uint32_t** q_first_out, uint32_t** q_last_out,
                   uint64_t** step_link_out, uint64_t** link_support_out /* nullable */, uint64_t* n_unitigs_out /* nullable */,
                   uint64_t* n_links_out /* nullable */);

/* ------------------------------------------------------------------------------------------
 * Repeat resolution: the transitions of threaded sequences through every unitig, weak-link removal, and repeat splitting.
 * (The reference has no counterpart; the notation is that of the four blocks above. tests/graph_resolve_ref.py restates this block.)
 *
 * Ends, link words and duality as above: end 2 u + 0 is the exit of unitig u traversed forwards, end 2 u + 1 its exit backwards; the
 * links of end e are link_to[link_off[e] .. link_off[e + 1]), and the LOCAL INDEX of link j at e is j - link_off[e], 0 .. 3; the dual of
 * e -> t is t ^ 1 -> e ^ 1, found as the first index in the list of t ^ 1 whose word is e ^ 1. No call takes an index handle: they work on
 * device arrays of the current device, are asynchronous on `stream` and return after their work on it has completed. Every call
 * validates first and writes second: a violation is AIX_ERR_ARG with no output (and no in/out array) touched. Every index read from an
 * input array is checked against U, 2 U, E and T before it is used. U > 2^31 - 4 is AIX_ERR_UNSUPPORTED, E > 8 U and a NULL pointer where
 * one is needed AIX_ERR_ARG, decided before anything is allocated or launched. Scratch comes from the pool and goes back on every path.
 *
 * 1. aix_thread_pairs_dev. Inputs U, link_off[2 U + 1], link_to[E] and the step arrays step_unitig u32[T], step_flag u8[T], step_link
 *    u64[T] as aix_seq_thread_dev wrote them (all sequences of a batch, concatenated). In/out pair_support u64[16 U]: accumulated, never
 *    zeroed, like link_support. Step i (1 <= i < T - 1) is a TRANSITION iff a = step_link[i] and b = step_link[i + 1] are both below E: by
 *    the threading contract step i - 1 is then the adjacent step of the same sequence, and the step enters u = step_unitig[i] at its
 *    entry and leaves it at its exit. With s = step_flag[i] & 1, e_prev = 2 step_unitig[i - 1] + (step_flag[i - 1] & 1) and d the dual of
 *    a (it lies in the list of (2 u + s) ^ 1): s == 0 gives x = the local index of b at end 2 u and y = that of d at end 2 u + 1; s == 1
 *    gives y = the local index of b at end 2 u + 1 and x = that of d at end 2 u. Then pair_support[16 u + 4 x + y] += 1: x names the
 *    link at end 2 u, y the link at end 2 u + 1, whichever way the sequence went. A sequence and its reverse complement hit the same
 *    cell; a sequence that crosses u twice counts twice. *n_pairs_out = the number of transitions. Counted from zero over the same
 *    batches as link_support, the cells of a link sum to at most its support — except at a hairpin u+ -> u-, its own dual, which the
 *    support counts once per traversal while the sequence passes u twice there (into the hairpin and out of it): at most twice.
 *    Validation: link_off starts at 0, ascends, ends at E, at most 4 links per end; step_unitig < U; every step_link is below E or one of
 *    AIX_THREAD_NO_LINK / AIX_THREAD_BROKEN; step_link[0] is no link; for a transition a lies in the list of e_prev and link_to[a] ==
 *    2 u + s, b lies in the list of 2 u + s, and d exists. T == 0 or U == 0 is AIX_OK with nothing done. Integer adds commute: the
 *    result does not depend on the launch geometry.
 *
 * 2. aix_graph_resolve_mark_dev decides, from the input arrays alone, in one round. Inputs U, offsets, circular, link_off, link_to, E,
 *    link_support u64[E] (nullable), pair_support u64[16 U] (nullable) and three thresholds; outputs link_remove u8[E] (1 = removed),
 *    copies u8[U] (1 .. 4) and three counts. Validation: that of the cleaning block with the duality of EVERY link; link_support[j] ==
 *    link_support[dual j] when the array is given; max_pair_noise < min_pair_support when splitting is on.
 *    Weak links (off when link_support is NULL or min_link_support == 0). Link j: e -> t is weak iff support[j] < min_link_support. It is
 *      removed iff it is weak and end e or end t ^ 1 has a link that is not weak: a fork decides, a lone weak link in a thin region
 *      stays. The rule is symmetric under duality, so the surviving links keep duality; a hairpin is its own dual.
 *    Splits (off when pair_support is NULL or min_pair_support == 0). A, B = the surviving links of ends 2 u, 2 u + 1. u is split iff it
 *      is linear; |A| == |B| == d >= 2; no surviving link of u names u itself (no hairpin, no tandem self-link); every cell (x, y) of
 *      A x B is strong (>= min_pair_support) or noise (<= max_pair_noise); every x has exactly one strong y and every y exactly one
 *      strong x. Then copies[u] = d, else 1. Cells of removed links are ignored.
 *
 * 3. aix_graph_resolve_layout_dev / aix_graph_resolve_emit_dev write G_r, a unitig set in exactly the format of the input.
 *    Layout. U' = U + sum(copies - 1); copy_base u32[U] = the id of copy 1 of u (U + the exclusive scan of copies - 1), AIX_BUBBLE_NONE
 *      for an unsplit u; the sizes U', offsets'[U'] and E' = E - removed. copies outside 1 .. 4 is AIX_ERR_ARG, U' > 2^31 - 4
 *      AIX_ERR_UNSUPPORTED.
 *    Emit. The eight arrays of G_r and unitig_origin u32[U']. It validates the unitig set, that link_remove is set on a link and its
 *      dual alike, that copy_base is the layout's, that every copies[u] > 1 is a split the arrays support (linear, no surviving self
 *      link, the strong cells of the surviving links a perfect matching of copies[u] pairs; noise is mark's affair and is not looked at
 *      again) and the three sizes, before anything is written. Ids below U keep offsets, bases, circular, tf_min and tf_max. Copy c of u
 *      is numbered by the rank c of its end-0 link among A, in list order: copy 0 keeps the id u, copy c >= 1 is copy_base[u] + c - 1;
 *      the copies are appended to the bases in id order with the same spelling, circular, tf_min and tf_max. tf_sum: with S the sum of
 *      u's strong cells and p_c the strong cell of copy c, copy c >= 1 gets floor(tf_sum p_c / S), exact in 128 bits, and copy 0 the
 *      rest, so the sum is conserved.
 *      Links. Every surviving link j: e -> t exists exactly once in G_r. Its source is end e & 1 of the copy of e >> 1 that OWNS j: an
 *      unsplit unitig is its own copy 0; at end 0 of a split unitig the rank of j in A; at end 1 the rank of the x matched to j's y. Its
 *      word is 2 id(the copy of t >> 1 that owns dual j) + (t & 1). The links of an end keep their order; every end of a copy has
 *      exactly one link; duality holds in G_r.
 *      Input and output arrays must not overlap. d_out_bases must be aligned to 8 bytes (AIX_ERR_ARG), what the compaction asks of its
 *      input.
 *    Properties. (a) With nothing removed and nothing split, G_r == G in every array and unitig_origin is the identity. (b)
 *      aix_graph_mark_dev and aix_graph_compact_* accept G_r; under an all-zero mask the compaction merges every copy with its two
 *      neighbours. (c) E' = E - removed, sum tf_sum' = sum tf_sum, sum(copies - 1) = U' - U.
 *    K-mer map. Unsplit unitigs keep id and positions, so a k-mer map of G stays valid for them. The k-mers of a split unitig keep
 *      pointing at copy 0: threading through G_r reports AIX_THREAD_BROKEN at the other copies. A second resolution round therefore
 *      needs a map that names several copies, which this block does not provide.
 *    U == 0 gives U' = 0, offsets' = {0}, link_off' = {0}.
 *
 * The host form takes G, link_support and pair_support (both nullable) in host arrays, runs mark, layout and emit, and returns G_r,
 * link_remove[E], copies[U] and unitig_origin[U'] in malloc'd arrays (aix_free); the last three are nullable.
 * ------------------------------------------------------------------------------------------ */
int aix_thread_pairs_dev(uint64_t U, const uint64_t* d_link_off, const uint32_t* d_link_to, uint64_t E, uint64_t T, const uint32_t* d_step_unitig,
                         const uint8_t* d_step_flag, const uint64_t* d_step_link, uint64_t* d_pair_support, uint64_t* n_pairs_out, void* stream);
int aix_graph_resolve_mark_dev(uint64_t U, const uint64_t* d_offsets, const uint8_t* d_circular, const uint64_t* d_link_off, const uint32_t* d_link_to,
                               uint64_t E, const uint64_t* d_link_support /* nullable */, const uint64_t* d_pair_support /* nullable */,
                               uint64_t min_link_support, uint64_t min_pair_support, uint64_t max_pair_noise, uint8_t* d_link_remove, uint8_t* d_copies,
                               uint64_t* n_links_removed_out, uint64_t* n_split_out, uint64_t* n_copies_added_out, void* stream);
int aix_graph_resolve_layout_dev(uint64_t U, const uint64_t* d_offsets, uint64_t E, const uint8_t* d_link_remove, const uint8_t* d_copies,
                                 uint32_t* d_copy_base, uint64_t* n_unitigs_out, uint64_t* total_bases_out, uint64_t* n_links_out, void* stream);
/* Writes G_r: d_out_offsets[U' + 1], d_out_bases[total_bases], d_out_circular / tf_sum / tf_min / tf_max [U'], d_out_link_off[2 U' + 1],
 * d_out_link_to[n_links], d_unitig_origin[U']; nothing is written at or beyond these sizes. d_pair_support may be NULL when nothing is
 * split. Scratch: see DESIGN 5m. */
int aix_graph_resolve_emit_dev(uint64_t U, const uint64_t* d_offsets, const uint8_t* d_bases, const uint8_t* d_circular, const uint64_t* d_tf_sum,
                               const uint32_t* d_tf_min, const uint32_t* d_tf_max, const uint64_t* d_link_off, const uint32_t* d_link_to, uint64_t E,
                               const uint8_t* d_link_remove, const uint8_t* d_copies, const uint32_t* d_copy_base,
                               const uint64_t* d_pair_support /* nullable */, uint64_t min_pair_support, uint64_t n_unitigs, uint64_t total_bases,
                               uint64_t n_links, uint64_t* d_out_offsets, uint8_t* d_out_bases, uint8_t* d_out_circular, uint64_t* d_out_tf_sum,
                               uint32_t* d_out_tf_min, uint32_t* d_out_tf_max, uint64_t* d_out_link_off, uint32_t* d_out_link_to,
                               uint32_t* d_unitig_origin, void* stream);
int aix_graph_resolve(uint64_t U, const uint64_t* offsets, const uint8_t* bases, const uint8_t* circular, const uint64_t* tf_sum, const uint32_t* tf_min,
                      const uint32_t* tf_max, const uint64_t* link_off, const uint32_t* link_to, uint64_t E, const uint64_t* link_support /* nullable */,
                      const uint64_t* pair_support /* nullable */, uint64_t min_link_support, uint64_t min_pair_support, uint64_t max_pair_noise,
                      uint64_t* n_unitigs_out, uint64_t* n_links_out, uint64_t* n_links_removed_out, uint64_t* n_split_out, uint64_t** offsets_out,
                      uint8_t** bases_out, uint8_t** circular_out, uint64_t** tf_sum_out, uint32_t** tf_min_out, uint32_t** tf_max_out,
                      uint64_t** link_off_out, uint32_t** link_to_out, uint8_t** link_remove_out /* nullable */, uint8_t** copies_out /* nullable */,
                      uint32_t** unitig_origin_out /* nullable */);

/* ------------------------------------------------------------------------------------------
 * Scaffolding: read pairs threaded through a contig graph become counted, gap-estimated links between contig ends; the joins are
 * decided per end; chains of joined contigs are written as gapped scaffolds.
 * (The reference has no counterpart; the notation is that of the graph blocks above. tests/scaffold_ref.py restates this block.)
 *
 * L_u = offsets[u + 1] - offsets[u], m_u = L_u - 22. End 2 u + 0 is the exit of contig u traversed forwards, 2 u + 1 its exit backwards; a
 * word 2 v + r names v entered in orientation r; the dual of e -> t is t ^ 1 -> e ^ 1. No call takes an index handle: they work on device
 * arrays of the current device, are asynchronous on `stream` and return after their work on it has completed. Every call validates
 * first and writes second: a violation is AIX_ERR_ARG with no output (and no in/out array) touched. Every index read from an input
 * array is checked against its bound before it is used. U > 2^31 - 4 is AIX_ERR_UNSUPPORTED, a NULL pointer where one is needed
 * AIX_ERR_ARG, decided before anything is allocated or launched. Scratch comes from the pool and goes back on every path. Integer adds
 * and deterministic tie rules only: no result depends on the launch geometry.
 *
 * 1. aix_mate_links_dev: one observation per pair. Inputs P; d_offs[2 P + 1], the sequence offsets of a threaded batch in which sequence
 *    2 i is the left mate A and 2 i + 1 the right mate B of pair i, both in fragment orientation (the line R1~revcomp(R2) of a reads
 *    file); seq_step_off[2 P + 1] and the step arrays step_unitig, step_pos, step_flag, q_first, q_last [T] of aix_seq_thread_dev; U,
 *    offsets[U + 1], circular[U]; min_anchor_windows >= 1 and max_insert in 1 .. 2^20.
 *    Anchor of a mate: its step with the most windows (q_last - q_first + 1), the earliest on a tie; it is an anchor only with at least
 *      min_anchor_windows windows and on a unitig that is not circular. With (u, pos, s = flag & 1) of that step, the start of the mate in
 *      the coordinates of its contig oriented as the step traverses it is, in signed 64 bits, x0 = pos - q_first (s = 0) or
 *      (m_u - 1 - pos) - q_first (s = 1).
 *    Cases, with anchors (u, sA, x0A), (v, sB, x0B) and mate lengths LA, LB. A mate without an anchor: unanchored. u == v, sA == sB:
 *      F = x0B + LB - x0A; 1 <= F <= max_insert gives insert_hist[F] += 1 (u64[max_insert + 1], accumulated, never zeroed), otherwise
 *      discordant. u == v, sA != sB: discordant. u != v: d = (L_u - x0A) + (x0B + LB), the bases of the fragment that lie on the two
 *      contigs if they were abutted; d > max_insert is discordant, and so is d < 1 (only hand-set steps reach it: a q_first beyond the
 *      mate puts its end in front of the contig); otherwise the pair observes the link e -> t, e = 2 u + sA, t = 2 v + sB. Of (e, t) and its dual (t ^ 1, e ^ 1) the one with the smaller first word is stored (the canonical form).
 *    Outputs obs_key u64[P] = e << 32 | t of the canonical form, all ones for a pair that is no observation; obs_d u32[P] (0 there);
 *      counts u64[4] = {same contig, link, discordant, unanchored}, written, not accumulated. A pair and its reverse complement
 *      (rc(B), rc(A)) give the same key and the same d whenever neither mate has two steps tied for the most windows.
 *    Validation: seq_step_off starts at 0, ascends and ends at T; step_unitig < U; step_pos < m_u; q_first <= q_last; offsets ascend by at
 *      least 23; d_offs ascends and every mate is shorter than 2^32 bytes. P == 0 is AIX_OK (counts all zero).
 *
 * 2. aix_mate_bundle_dev: N observations (a caller concatenates its batches) into the scaffold graph, a CSR over the 2 U ends:
 *    slink_off u64[2 U + 1], slink_to u32[S], slink_count u64[S], slink_dsum u64[S]. One bundle per distinct key carries count and the
 *    sum of d; every bundle is written twice, as e -> t in the list of e and as its dual in the list of t ^ 1, with equal count and dsum,
 *    so S is twice the number of bundles. The list of an end ascends by target word and may be of any length. Sizing, as
 *    aix_seq_hits_dev: slink_off and *total_out = S are always written, the entries only when S <= cap, never at or beyond cap (they
 *    may be NULL when cap == 0); AIX_OK either way. Validation: every key is all ones (skipped) or canonical with both words below
 *    2 U, on different contigs, and d >= 1. N == 0 gives slink_off all zero. N >= 2^32 is AIX_ERR_UNSUPPORTED (a bundle is named by
 *    32 bits), in the host form too.
 *
 * 3. aix_scaffold_mark_dev: which ends are joined, one round, from the arrays alone. A link is a CANDIDATE iff count >= min_pairs (>= 1),
 *    both its contigs are linear and both are at least min_contig_bases long. The BEST link of an end is its candidate with the largest
 *    count, the smaller target word on a tie. An end is DECIDED iff it has a best link and every other candidate c at it has
 *    count_c * dominance <= count_best (dominance >= 1; the product in 128 bits). e -> t is a JOIN iff it is the best link of a decided e
 *    and its dual is the best link of a decided t ^ 1. Outputs join u32[2 U] (join[e] = t and join[t ^ 1] = e ^ 1, AIX_BUBBLE_NONE
 *    elsewhere), join_count u64[2 U], join_gap i64[2 U] = insert_size - floor(dsum / count) (equal at both ends of a join, 0 elsewhere)
 *    and the number of joins. Every end takes part in at most one join: the components are simple paths and simple cycles of contigs.
 *    Validation: offsets ascend by at least 23; slink_off starts at 0, ascends and ends at S; words below 2 U; no link within one contig;
 *    lists ascend strictly; count >= 1; floor(dsum / count) fits 32 bits; every link has its dual with equal count and dsum.
 *
 * 4. aix_scaffold_layout_dev ranks the ends by pointer jumping over `join`. What the ranking leaves open lies on cycles; a cycle is cut
 *    at its join with the smallest min(count, 2^32 - 1) << 32 | min(e, t ^ 1) and then ranked as a path. The written gap of a join is
 *    max(join_gap, min_gap), min_gap >= 1. Of a path's two terminal contigs the one with the smaller id comes first, oriented so that the
 *    path leaves it; a single contig is forwards. Scaffold ids ascend by the id of the first member. Every contig belongs to exactly one
 *    scaffold. Outputs contig_scaffold u32[U], contig_rank u32[U] (its index among the members), contig_pos u64[U] (the offset of its
 *    first base in the scaffold), contig_flag u8[U] (bit 0: reversed), the number of scaffolds, their total bases, and the joins cut.
 *    Validation: offsets; a join names an end of another contig below 2 U whose entry names it back, with equal count and gap.
 *
 *    aix_scaffold_emit_dev validates the map against join and the two sizes before anything is written: (scaffold, rank) are dense; a
 *    member follows its predecessor through a join in matching orientation, at the distance of the predecessor's length and written
 *    gap; the two outer ends of a scaffold are unjoined, or joined to each other (the cut of a cycle; that it was the weakest join is
 *    the layout's affair and is not looked at again); first members obey the order rules above; the lengths sum to total_bases. It
 *    writes scaffold_offsets u64[Sc + 1] and scaffold_bases (every member's oriented bases whole, a reversed member reverse-complemented
 *    by the byte rule of the cleaning block, 'N' over the gaps), the member CSR member_off u64[Sc + 1] and member u32[U] (word
 *    2 u + flag) and member_gap i64[U], the raw join_gap in front of the member, 0 for a first member. With no joins the scaffolds are
 *    the contigs: the same bases, the same offsets, the identity map. U == 0 gives {0} for both offset arrays.
 *
 * The host form takes the contigs and N observations in host arrays, runs bundle, mark, layout and emit, and returns malloc'd arrays
 * (aix_free); the last seven are nullable.
 * ------------------------------------------------------------------------------------------ */
int aix_mate_links_dev(uint64_t P, const uint64_t* d_offs, const uint64_t* d_seq_step_off, uint64_t T, const uint32_t* d_step_unitig,
                       const uint32_t* d_step_pos, const uint8_t* d_step_flag, const uint32_t* d_q_first, const uint32_t* d_q_last, uint64_t U,
                       const uint64_t* d_offsets, const uint8_t* d_circular, uint32_t min_anchor_windows, uint32_t max_insert,
                       uint64_t* d_insert_hist, uint64_t* d_obs_key, uint32_t* d_obs_d, uint64_t* d_counts, void* stream);
int aix_mate_bundle_dev(uint64_t N, const uint64_t* d_obs_key, const uint32_t* d_obs_d, uint64_t U, uint64_t* d_slink_off, uint32_t* d_slink_to,
                        uint64_t* d_slink_count, uint64_t* d_slink_dsum, uint64_t cap, uint64_t* total_out, void* stream);
int aix_scaffold_mark_dev(uint64_t U, const uint64_t* d_offsets, const uint8_t* d_circular, const uint64_t* d_slink_off, const uint32_t* d_slink_to,
                          const uint64_t* d_slink_count, const uint64_t* d_slink_dsum, uint64_t S, uint32_t insert_size, uint64_t min_pairs,
                          uint64_t dominance, uint64_t min_contig_bases, uint32_t* d_join, uint64_t* d_join_count, int64_t* d_join_gap,
                          uint64_t* n_joins_out, void* stream);
int aix_scaffold_layout_dev(uint64_t U, const uint64_t* d_offsets, const uint32_t* d_join, const uint64_t* d_join_count, const int64_t* d_join_gap,
                            uint32_t min_gap, uint32_t* d_contig_scaffold, uint32_t* d_contig_rank, uint64_t* d_contig_pos, uint8_t* d_contig_flag,
                            uint64_t* n_scaffolds_out, uint64_t* total_bases_out, uint64_t* n_cut_out, void* stream);
/* Nothing is written at or beyond the sizes given. Input and output arrays must not overlap. Scratch: see DESIGN 5n. */
int aix_scaffold_emit_dev(uint64_t U, const uint64_t* d_offsets, const uint8_t* d_bases, const uint32_t* d_join, const int64_t* d_join_gap,
                          uint32_t min_gap, const uint32_t* d_contig_scaffold, const uint32_t* d_contig_rank, const uint64_t* d_contig_pos,
                          const uint8_t* d_contig_flag, uint64_t n_scaffolds, uint64_t total_bases, uint64_t* d_scaffold_offsets,
                          uint8_t* d_scaffold_bases, uint64_t* d_member_off, uint32_t* d_member, int64_t* d_member_gap, void* stream);
int aix_scaffold(uint64_t U, const uint64_t* offsets, const uint8_t* bases, const uint8_t* circular, uint64_t N, const uint64_t* obs_key,
                 const uint32_t* obs_d, uint32_t insert_size, uint64_t min_pairs, uint64_t dominance, uint64_t min_contig_bases, uint32_t min_gap,
                 uint64_t* n_scaffolds_out, uint64_t* n_joins_out, uint64_t* n_cut_out, uint64_t* n_slinks_out, uint64_t** scaffold_offsets_out,
                 uint8_t** scaffold_bases_out, uint64_t** member_off_out, uint32_t** member_out, int64_t** member_gap_out,
                 uint32_t** join_out /* nullable */, uint64_t** join_count_out /* nullable */, int64_t** join_gap_out /* nullable */,
                 uint32_t** contig_scaffold_out /* nullable */, uint32_t** contig_rank_out /* nullable */, uint64_t** contig_pos_out /* nullable */,
                 uint8_t** contig_flag_out /* nullable */);

/* ------------------------------------------------------------------------------------------
 * Gap closing: the 'N' run of a join is replaced by the bases of a path through the contig graph, where exactly one path of the
 * estimated length exists.
 * (The reference has no counterpart; the notation is that of the scaffolding block. tests/gap_close_ref.py restates this block.)
 *
 * L_w is the length of the contig of word w; the exit end of a contig entered as word w is w itself; the dual of e -> t is
 * t ^ 1 -> e ^ 1. No call takes an index handle: they work on device arrays of the current device, are asynchronous on `stream` and
 * return after their work on it has completed. Every call validates first and writes second: a violation is AIX_ERR_ARG with no
 * output touched. Every index read from an input array is checked against its bound before it is used. U > 2^31 - 4 is
 * AIX_ERR_UNSUPPORTED, a NULL pointer where one is needed AIX_ERR_ARG, decided before anything is allocated or launched. Scratch comes
 * from the pool and goes back on every path. Integer only; no result depends on the launch geometry.
 *
 * 1. aix_gap_close_dev: the search. Inputs U, offsets[U + 1], link_off[2 U + 1], link_to[E] (the graph the pairs were threaded through;
 *    a list may be of any length, and the graph need not be dual-closed), join u32[2 U] and join_gap i64[2 U] of
 *    aix_scaffold_mark_dev, tolerance (0 .. 2^20), max_fill (0 .. 64), max_states (1 .. 4096), and cap for the path array.
 *    The OWNER of a join e -> t is its end e with e < (t ^ 1); the search runs once per join, from the owner, with g = join_gap[e].
 *    Rule. A candidate is (w, d, k): w a word, d (signed) the bases between the last base of e's contig and the first base of w, k the
 *      number of intermediates before w. The first candidates are (x, -22, 0) for every link x of end e. A candidate with w == t becomes
 *      a stored state, a HIT, iff |d - g| <= tolerance; it is never expanded. A candidate with w != t becomes a stored state, an
 *      INTERMEDIATE, iff k < max_fill, both join entries of w's contig are none (a fill goes only through contigs the scaffolder left
 *      single) and d + L_w - 22 <= g + tolerance. The children of an intermediate are (y, d + L_w - 22, k + 1) for every link y of end
 *      w. A contig may recur on a path, so a tandem repeat is counted out by length. The set of states, and therefore every output, is
 *      independent of the order in which candidates are examined.
 *    Status per join, equal at both its ends, 0 on unjoined ends: 4 exhausted (the complete search would store more than max_states
 *      states, whatever hits it saw), else 2 no hit, 3 ambiguous (two or more hits), 1 closed (exactly one hit).
 *    Outputs close_status u8[2 U]; close_dist i64[2 U], the hit's d at both ends when closed, else 0; close_states u32[2 U], the states
 *      stored, max_states when exhausted, at both ends; path_off u64[2 U + 1] and path u32[cap], a CSR keyed by end that is non-empty
 *      only at the owner of a closed join and holds the intermediates in order from e to t; fill_uses u32[U], the closed joins that pass
 *      through each contig, once per occurrence; counts u64[5] = joins of status 1 .. 4 and the number of joins, written, not
 *      accumulated. Sizing, as aix_mate_bundle_dev: path_off and *total_out are always written, the entries only when the total <= cap,
 *      never at or beyond cap (path may be NULL when cap == 0); AIX_OK either way. U == 0 and "no joins" are AIX_OK.
 *    Validation: offsets ascend by at least 23; link_off starts at 0, ascends and ends at E; link words below 2 U; join is symmetric as
 *      the layout requires (the named end is below 2 U, lies on another contig and names the caller back with an equal gap);
 *      |join_gap| <= 2^30 on joined ends.
 *
 * 2. aix_scaffold_fill_layout_dev: the filled member lists, from the graph, the joins, min_gap >= 1, the member CSR of
 *    aix_scaffold_emit_dev (n_scaffolds, member_off, member) and the closure (close_status, close_dist, path_off, path, the path total).
 *    A join between ADJACENT members that is closed contributes its path, then the member; the path is reversed with every word ^ 1 when
 *    the scaffold traverses the join from the non-owner side. A join that is not closed, and the cut join of a cycle, stay as they are.
 *    Outputs fmember_off u64[Sc + 1]; fmember u32[Mf]; fmember_flag u8[Mf] (bit 0: the member overlaps its predecessor by 22 bases,
 *      bit 1: it is a fill contig); fmember_gap i64[Mf], the raw join_gap in front of an unclosed member, close_dist in front of the
 *      member that ends a closed join, 0 elsewhere; fmember_pos u64[Mf], the offset in the filled scaffold of the first byte the member
 *      writes; fscaffold_offsets u64[Sc + 1]; *n_fmembers_out = Mf and *total_bases_out. The caller allocates U + path total entries for
 *      the fmember arrays, which is always enough.
 *    Validation: that of the search for the graph and the joins; the member CSR is dense (member_off starts at 0, ascends strictly, ends
 *      at U) and names every contig once; a member follows its predecessor through join; statuses are 0 .. 4, 0 on an unjoined end and
 *      equal at both ends of a join; path_off starts at 0, ascends and ends at the path total; only owners of closed joins have paths;
 *      every step of a path (e -> p0, p0 -> p1, .., p_last -> t) is a link of the graph; every intermediate has no join; close_dist
 *      equals the path's length, sum (L_p - 22) - 22, at both ends.
 *
 *    aix_scaffold_fill_emit_dev revalidates the fmember arrays against offsets and flags (fmember_off starts at 0, ascends strictly and
 *    ends at n_fmembers; words below 2 U; flags 0, 1 or 3; a first member has flag 0 and position 0; every other member starts where
 *    its predecessor's bytes and its own 'N' run end; a scaffold ends with its last member; fscaffold_offsets starts at 0 and ends at
 *    total_bases), then writes fscaffold_bases: a first or unclosed member whole, an unclosed member preceded by max(gap, min_gap)
 *    bytes of 'N', a member with bit 0 without its first 22 oriented bases; reverse complement by the byte rule of the cleaning block.
 *    The 22 overlapping bases are not compared: a graph the library wrote has them equal. With no closed join the filled scaffolds
 *    equal the scaffolds byte for byte and fmember equals member.
 *
 * aix_scaffold_fill is the host form of search, layout and emit: contigs, links, joins and the member CSR in host arrays, malloc'd
 * arrays out (aix_free); the last seven (the closure) are nullable.
 * ------------------------------------------------------------------------------------------ */
int aix_gap_close_dev(uint64_t U, const uint64_t* d_offsets, const uint64_t* d_link_off, const uint32_t* d_link_to, uint64_t E, const uint32_t* d_join,
                      const int64_t* d_join_gap, uint32_t tolerance, uint32_t max_fill, uint32_t max_states, uint8_t* d_close_status,
                      int64_t* d_close_dist, uint32_t* d_close_states, uint64_t* d_path_off, uint32_t* d_path, uint64_t cap, uint64_t* total_out,
                      uint32_t* d_fill_uses, uint64_t* d_counts, void* stream);
int aix_scaffold_fill_layout_dev(uint64_t U, const uint64_t* d_offsets, const uint64_t* d_link_off, const uint32_t* d_link_to, uint64_t E,
                                 const uint32_t* d_join, const int64_t* d_join_gap, uint32_t min_gap, uint64_t n_scaffolds,
                                 const uint64_t* d_member_off, const uint32_t* d_member, const uint8_t* d_close_status, const int64_t* d_close_dist,
                                 const uint64_t* d_path_off, const uint32_t* d_path, uint64_t path_total, uint64_t* d_fmember_off, uint32_t* d_fmember,
                                 uint8_t* d_fmember_flag, int64_t* d_fmember_gap, uint64_t* d_fmember_pos, uint64_t* d_fscaffold_offsets,
                                 uint64_t* n_fmembers_out, uint64_t* total_bases_out, void* stream);
/* Nothing is written at or beyond the sizes given. Input and output arrays must not overlap. Scratch: see DESIGN 5o. */
int aix_scaffold_fill_emit_dev(uint64_t U, const uint64_t* d_offsets, const uint8_t* d_bases, uint32_t min_gap, uint64_t n_scaffolds,
                               const uint64_t* d_fmember_off, uint64_t n_fmembers, const uint32_t* d_fmember, const uint8_t* d_fmember_flag,
                               const int64_t* d_fmember_gap, const uint64_t* d_fmember_pos, const uint64_t* d_fscaffold_offsets, uint64_t total_bases,
                               uint8_t* d_fscaffold_bases, void* stream);
int aix_scaffold_fill(uint64_t U, const uint64_t* offsets, const uint8_t* bases, const uint64_t* link_off, const uint32_t* link_to, uint64_t E,
                      const uint32_t* join, const int64_t* join_gap, uint64_t n_scaffolds, const uint64_t* member_off, const uint32_t* member,
                      uint32_t tolerance, uint32_t max_fill, uint32_t max_states, uint32_t min_gap, uint64_t* n_fmembers_out, uint64_t* total_bases_out,
                      uint64_t* path_total_out, uint64_t** fscaffold_offsets_out, uint8_t** fscaffold_bases_out, uint64_t** fmember_off_out,
                      uint32_t** fmember_out, uint8_t** fmember_flag_out, int64_t** fmember_gap_out, uint64_t** fmember_pos_out,
                      uint8_t** close_status_out /* nullable */, int64_t** close_dist_out /* nullable */, uint32_t** close_states_out /* nullable */,
                      uint64_t** path_off_out /* nullable */, uint32_t** path_out /* nullable */, uint32_t** fill_uses_out /* nullable */,
                      uint64_t** counts_out /* nullable */);

/* ------------------------------------------------------------------------------------------
 * Pile-up: the reads laid back over the contigs they thread through — per-base A/C/G/T counts, variant sites, a polished consensus.
 * (The reference has no counterpart; the notation is that of the threading block. tests/pileup_ref.py restates this block.)
 *
 * L_u = offsets[u + 1] - offsets[u] and m_u = L_u - 22; B = offsets[U]; global base g of contig u at local position x is offsets[u] + x.
 * Sequences as aix_seq_thread_dev takes them. The three device calls take no index handle: they work on device arrays of the current
 * device, are asynchronous on `stream` and return after their work on it has completed. Every call validates first and writes second: a
 * violation is AIX_ERR_ARG with no output (and no in/out array) touched. Every index read from an input array is compared with its bound
 * before it is used. U > 2^31 - 4 is AIX_ERR_UNSUPPORTED, a NULL pointer where one is needed AIX_ERR_ARG, decided before anything is
 * allocated or launched. In all three, offsets start at 0 and ascend by at least 23, and sequence offsets ascend by less than 2^32.
 * Scratch comes from the pool and goes back on every path; see DESIGN 5p. Integer only; no result depends on the launch geometry.
 *
 * 1. aix_pile_place_dev: steps become placements. Inputs M and d_offs[M + 1] of the threaded batch; d_seq_step_off[M + 1], T and
 *    step_unitig / step_pos / step_flag / q_first / q_last [T] as aix_seq_thread_dev wrote them (step_link is not read); U and
 *    offsets[U + 1]; max_gap and extend.
 *    Diagonal. A step with flag bit 1 (circular) makes no placement, ends a merge and is counted in *n_circular_steps_out. A linear step
 *      (u, p, s, a = q_first, b = q_last) lies on diagonal d = p - a (s = 0: read base j lies on contig base d + j) or d = p + a + 22
 *      (s = 1: read base j lies on contig base d - j, complemented). d is signed.
 *    Merging. Consecutive steps t - 1, t of one sequence belong to one placement iff both are linear, have the same u, s and d, and
 *      a_t - b_{t-1} - 1 <= max_gap (the windows between them: 23 for one substitution).
 *    End extension. The core of a placement is read bases [a_first, b_last + 22]. It grows on each side by at most `extend` bases, and
 *      no further than the end of the read, the end of the contig, and its neighbour among the placements of the same sequence (cores, in
 *      step order): on the left it stays beyond b_last + 22 of the placement before it, on the right below a_first of the placement after
 *      it. A limit that comes out negative is 0. (The windows next to a read's end that hold a substitution have no node; the extension
 *      is what brings that base into the pile. Both rules are measured from the neighbour's core, so read bases between two cores that
 *      did not merge may be claimed from both sides, and then count once per placement.)
 *    Outputs, room for T records each (the count never exceeds T: no sizing pass): seq_place_off u64[M + 1], a CSR over sequences, in
 *      step order; place_unitig u32; place_flag u8 (bit 0: the read lies backwards on the contig); place_pos u32, the leftmost contig
 *      base covered, local to the contig; place_q0 u32, the first read base; place_len u32; place_steps u32, the steps merged;
 *      *n_place_out, and *n_circular_steps_out (nullable). A backward placement covers read base q0 + x at contig base pos + len - 1 - x.
 *    Validation: seq_step_off starts at 0, ascends and ends at T; u < U; q_first <= q_last and q_last + 23 <= the sequence's length; a
 *      linear step fits its contig (s = 0: p + (b - a) < m_u; s = 1: b - a <= p < m_u); within a sequence q_first exceeds the q_last of
 *      the step before. M == 0 or T == 0 is AIX_OK with seq_place_off all zero (the step arrays and the record arrays may be NULL when
 *      T == 0); T > 0 with M == 0 is AIX_ERR_ARG.
 *
 * 2. aix_pileup_dev: placements and read bytes become counts. Inputs d_seqs, d_offs[M + 1], M; seq_place_off[M + 1], R and
 *    place_unitig / place_flag / place_pos / place_q0 / place_len [R]; U, offsets[U + 1], bases[B].
 *    In/out counts u32[4 B], 16-byte aligned: cell 4 g + c counts the read bases showing c (A, C, G, T = 0 .. 3) at global base g. It is
 *      accumulated, never zeroed: a caller adds batch after batch. Counters wrap at 2^32.
 *    Per read base of a placement: only an upper-case A, C, G or T is counted, complemented first when the placement lies backwards; any
 *      other byte counts nowhere and adds to stats[1].
 *    Outputs (nullable): place_mism u32[R], the counted bases of a placement that differ from the contig base; stats u64[3] = bases
 *      counted, other bytes, mismatches of this call (written, not accumulated).
 *    Validation: seq_place_off starts at 0, ascends and ends at R; u < U; len >= 1; pos + len <= L_u; q0 + len <= the read's length;
 *      every contig byte is an upper-case A, C, G or T. R == 0 is AIX_OK with counts untouched (the contig bytes are still checked).
 *    Integer adds commute: the result does not depend on the launch geometry, and a batch and its reverse complement give equal counts.
 *
 * 3. aix_pile_call_dev: counts become consensus, variant sites and depth. Inputs U, offsets, bases, counts (16-byte aligned) and
 *    min_depth, min_major_permille, min_alt_count, min_alt_permille.
 *    Per base g: r = the code of the contig base, c[0 .. 3] its cell, D = c[0] + c[1] + c[2] + c[3], alt = the channel other than r with
 *      the largest count, ties to the smaller code. D is summed in 64 bits, and both permille comparisons are exact whatever the
 *      thresholds are: a product that passes 2^64 (a threshold near 2^32 on a D near 2^34) does not wrap.
 *      polished[g] = ACGT[alt] iff D >= min_depth, c[alt] > c[r] and 1000 c[alt] >= min_major_permille D; else the contig's base.
 *      g is a variant site iff D >= min_depth, c[alt] >= min_alt_count and 1000 c[alt] >= min_alt_permille D.
 *    Outputs, each nullable: polished u8[B] and *n_changed_out; the variant sites in ascending g — var_unitig u32, var_pos u32 (local),
 *      var_ref and var_alt u8 (ASCII), var_ref_count = c[r], var_alt_count = c[alt], var_depth u32 (D, 2^32 - 1 when it does not fit);
 *      depth_sum u64[U] (the sum of D over the contig) and uncovered u32[U] (its bases with D == 0).
 *    Sizing of the variants, as aix_seq_hits_dev: *total_out is always written, the entries only when *total_out <= cap, never at or
 *      beyond cap (the seven arrays may be NULL when cap == 0); AIX_OK either way. total_out == NULL (then cap must be 0): no variants.
 *    Validation: the offsets, and every contig byte an upper-case A, C, G or T.
 *    The polished bases keep the offsets of the input and are an end product: the 22-base overlaps between linked contigs and the
 *    k-mer map are NOT kept consistent with them, so they are not to be fed back into the graph calls.
 *
 * The host form builds layout, emit, links and nodes of the unitig graph at `cutoff` inside (as aix_seq_thread does), threads host
 * sequences through it, places them and piles them once from zero, and returns malloc'd arrays (aix_free): offsets[U + 1], bases[B],
 * counts[4 B], seq_place_off[M + 1] and the six placement arrays, optionally place_mism[R] and stats[3]. Handle and statuses as
 * aix_seq_thread. Piling onto contigs after cleaning is a device-form feature.
 * ------------------------------------------------------------------------------------------ */
int aix_pile_place_dev(uint64_t M, const uint64_t* d_offs, const uint64_t* d_seq_step_off, uint64_t T, const uint32_t* d_step_unitig,
                       const uint32_t* d_step_pos, const uint8_t* d_step_flag, const uint32_t* d_q_first, const uint32_t* d_q_last, uint64_t U,
                       const uint64_t* d_offsets, uint32_t max_gap, uint32_t extend, uint64_t* d_seq_place_off, uint32_t* d_place_unitig,
                       uint8_t* d_place_flag, uint32_t* d_place_pos, uint32_t* d_place_q0, uint32_t* d_place_len, uint32_t* d_place_steps,
                       uint64_t* n_place_out, uint64_t* n_circular_steps_out /* nullable */, void* stream);
int aix_pileup_dev(const char* d_seqs, const uint64_t* d_offs, uint64_t M, const uint64_t* d_seq_place_off, uint64_t R,
                   const uint32_t* d_place_unitig, const uint8_t* d_place_flag, const uint32_t* d_place_pos, const uint32_t* d_place_q0,
                   const uint32_t* d_place_len, uint64_t U, const uint64_t* d_offsets, const uint8_t* d_bases, uint32_t* d_counts,
                   uint32_t* d_place_mism /* nullable */, uint64_t* d_stats /* nullable */, void* stream);
int aix_pile_call_dev(uint64_t U, const uint64_t* d_offsets, const uint8_t* d_bases, const uint32_t* d_counts, uint32_t min_depth,
                      uint32_t min_major_permille, uint32_t min_alt_count, uint32_t min_alt_permille, uint8_t* d_polished /* nullable */,
                      uint64_t* n_changed_out /* nullable */, uint32_t* d_var_unitig, uint32_t* d_var_pos, uint8_t* d_var_ref, uint8_t* d_var_alt,
                      uint32_t* d_var_ref_count, uint32_t* d_var_alt_count, uint32_t* d_var_depth, uint64_t cap, uint64_t* total_out /* nullable */,
                      uint64_t* d_depth_sum /* nullable */, uint32_t* d_uncovered /* nullable */, void* stream);
int aix_pileup(aix_index_t* h, uint32_t cutoff, const char* seqs, const uint64_t* offs, uint64_t M, uint32_t max_gap, uint32_t extend,
               uint64_t* n_unitigs_out, uint64_t* n_place_out, uint64_t* n_circular_steps_out /* nullable */, uint64_t** offsets_out,
               uint8_t** bases_out, uint32_t** counts_out, uint64_t** seq_place_off_out, uint32_t** place_unitig_out, uint8_t** place_flag_out,
               uint32_t** place_pos_out, uint32_t** place_q0_out, uint32_t** place_len_out, uint32_t** place_steps_out,
               uint32_t** place_mism_out /* nullable */, uint64_t** stats_out /* nullable */);

/* ------------------------------------------------------------------------------------------
 * Phasing: the variant sites of aix_pile_call_dev linked by the reads that cover two of them — allele links, phase blocks, haplotype
 * tags. (The reference has no counterpart; notation and conventions are those of the pile-up block. tests/phase_ref.py restates this
 * block.) The four device calls take no index handle, work on device arrays of the current device, are asynchronous on `stream` and
 * return after their work on it has completed. Every call validates first and writes second: a violation is AIX_ERR_ARG with no output
 * touched. Every index read from an input array is compared with its bound before it is used. A NULL pointer where one is needed is
 * AIX_ERR_ARG, decided before anything is allocated or launched. Scratch comes from the pool and goes back on every path; see DESIGN
 * 5q. Integer only; no result depends on the launch geometry.
 *
 * Sites. V sites var_unitig u32[V], var_pos u32[V], var_ref u8[V], var_alt u8[V] as aix_pile_call_dev writes them; site v lies at
 *   global base g_v = offsets[var_unitig[v]] + var_pos[v]. Validation: var_unitig < U and var_pos < L_u; g strictly ascending; ref and
 *   alt are upper-case A, C, G or T and differ. V > 2^31 - 4 is AIX_ERR_UNSUPPORTED (all five calls).
 * Fragments. group is 1 or 2; anything else, or M not a multiple of group, is AIX_ERR_ARG. Fragment f is sequences group f ..
 *   group f + group - 1 (the mate convention of aix_mate_links_dev); F = M / group. F > 2^32 - 1 is AIX_ERR_UNSUPPORTED.
 *
 * 1. aix_phase_observe_dev: placements and read bytes become allele observations and links. Inputs d_seqs, d_offs[M + 1], M, group;
 *    seq_place_off[M + 1], R and place_unitig / place_flag / place_pos / place_q0 / place_len [R], validated exactly as aix_pileup_dev
 *    validates them (contig bytes are not read); U, offsets[U + 1]; the sites.
 *    Raw observation: one for every placement r = (u, pos, len, q0) and every site v with offsets[u] + pos <= g_v < offsets[u] + pos +
 *      len. With x = g_v - (offsets[u] + pos) its byte is seq[q0 + x] when the placement lies forwards and the complement of
 *      seq[q0 + len - 1 - x] when it lies backwards (an upper-case A, C, G, T is complemented, any other byte stays what it is). Its
 *      allele is 0 if the byte equals var_ref[v], 1 if it equals var_alt[v], 2 otherwise (a third base, lower case, N).
 *    Observation: fragment f observes site v with allele a iff it has at least one raw observation of v and all of them have the same
 *      allele a in {0, 1} (both mates, and overlapping placements of one read, may see the site). A (f, v) group that holds an allele 2
 *      is dropped as "other"; one that holds both 0 and 1 and no 2 is dropped as "discordant".
 *    Link: two observations (v, a), (w, b) of one fragment that follow each other in site order, with var_unitig[v] == var_unitig[w],
 *      give the link (lo = v, hi = w, rel = a ^ b). Consecutive observations on different contigs give none.
 *    Outputs: frag_obs_off u64[F + 1], always written; obs_site u32, obs_allele u8, per fragment in ascending site order; link_lo u32,
 *      link_hi u32, link_rel u8, in fragment order, then site order; stats u64[6] (nullable) = raw observations, (f, v) groups, groups
 *      dropped as other, groups dropped as discordant, observations, links.
 *    Sizing, as aix_seq_hits_dev, with two independent caps and totals: *obs_total_out and *link_total_out are always written, the
 *      entries of a kind only when its total <= its cap, never at or beyond the cap (its arrays may be NULL at cap 0); AIX_OK either way.
 *    M == 0 or R == 0 or V == 0 is AIX_OK with frag_obs_off all zero and both totals 0 (what is given is still validated).
 *
 * 2. aix_phase_bundle_dev: links become counted edges. Inputs V, N and link_lo / link_hi / link_rel [N], in any order (the caller
 *    concatenates what the batches wrote). Validation: lo < hi < V and rel <= 1. N > 2^32 - 1 is AIX_ERR_UNSUPPORTED, so the counters
 *    cannot wrap. Outputs, room for N each (the count never exceeds N: no sizing pass): the distinct (lo, hi) in ascending (hi, lo) —
 *    edge_lo u32, edge_hi u32 — with edge_cis u32 (links with rel 0) and edge_trans u32 (rel 1); edge_off u64[V + 1], a CSR over hi;
 *    *n_edges_out. N == 0 gives edge_off all zero.
 *
 * 3. aix_phase_solve_dev: edges become blocks and phases. Inputs V, var_unitig[V]; edge_off[V + 1], E, edge_lo, edge_cis, edge_trans
 *    [E] (edge_hi is the row); min_link_reads, min_link_permille.
 *    Validation: edge_off starts at 0, ascends and ends at E; in row w every lo < w, the lo ascend strictly, and var_unitig[lo] ==
 *      var_unitig[w]; var_unitig does not descend.
 *    Decided. n = cis + trans and m = max(cis, trans), in 64 bits. An edge is decided iff n >= max(min_link_reads, 1), cis != trans and
 *      1000 m >= min_link_permille n, exactly whatever the threshold (above 1000 no edge is decided). Its sign is 1 iff trans > cis.
 *    Parent. The parent of site w is, among the decided edges of its row, the lo of the one with the largest n; ties go to the larger
 *      m, then to the larger lo (the nearest site). A site whose row has no decided edge is a root. Parents have smaller indices.
 *    Block and phase. site_block[w] is the root reached from w, site_phase[w] the XOR of the signs on the way, so a root has phase 0.
 *      A root without children is unphased: its block is itself and its phase AIX_PHASE_NONE. Phase p at site v means: the alternative
 *      base lies on haplotype 1 ^ p and the contig's base on haplotype p; an observation (v, a) lies on haplotype a ^ p.
 *    Outputs: site_block u32[V], site_phase u8[V]; nullable site_parent u32[V] (0xFFFFFFFF for a root); nullable edge_state u8[E]: 0
 *      undecided, 1 decided with both ends in one block and phase[lo] ^ phase[hi] == sign, 2 decided, one block, contradicting the
 *      phases, 3 decided with the ends in different blocks (not used); nullable counts u64[6] = blocks of two or more sites, phased
 *      sites, decided edges, edges of state 1, 2 and 3.
 *
 * 4. aix_phase_tag_dev: fragments get a haplotype. Inputs F, frag_obs_off[F + 1], n_obs, obs_site, obs_allele [n_obs]; V, site_block,
 *    site_phase [V]. Validation: frag_obs_off starts at 0, ascends and ends at n_obs; site < V; allele <= 1; site_block[v] <= v;
 *    site_phase[v] is 0, 1 or AIX_PHASE_NONE. Per fragment the first observation in the order of the arrays whose site is phased names
 *    tag_block (0xFFFFFFFF without one); tag_h0 / tag_h1 count the observations in that block with a ^ p = 0 / 1, tag_other those on
 *    phased sites of other blocks. All four are u32[F].
 *
 * The host form takes host arrays (V, var_unitig, N and the three link arrays, the two thresholds), runs bundle and solve on the null
 * stream of the current device and returns malloc'd arrays (aix_free): the four edge arrays [E], edge_off[V + 1], edge_state[E]
 * (nullable), site_block[V], site_phase[V], site_parent[V] (nullable), counts[6] (nullable); *n_edges_out = E.
 * ------------------------------------------------------------------------------------------ */
#define AIX_PHASE_NONE 0xFFu
int aix_phase_observe_dev(const char* d_seqs, const uint64_t* d_offs, uint64_t M, uint32_t group, const uint64_t* d_seq_place_off, uint64_t R,
                          const uint32_t* d_place_unitig, const uint8_t* d_place_flag, const uint32_t* d_place_pos, const uint32_t* d_place_q0,
                          const uint32_t* d_place_len, uint64_t U, const uint64_t* d_offsets, uint64_t V, const uint32_t* d_var_unitig,
                          const uint32_t* d_var_pos, const uint8_t* d_var_ref, const uint8_t* d_var_alt, uint64_t* d_frag_obs_off,
                          uint32_t* d_obs_site, uint8_t* d_obs_allele, uint64_t obs_cap, uint64_t* obs_total_out, uint32_t* d_link_lo,
                          uint32_t* d_link_hi, uint8_t* d_link_rel, uint64_t link_cap, uint64_t* link_total_out, uint64_t* d_stats /* nullable */,
                          void* stream);
int aix_phase_bundle_dev(uint64_t V, uint64_t N, const uint32_t* d_link_lo, const uint32_t* d_link_hi, const uint8_t* d_link_rel, uint32_t* d_edge_lo,
                         uint32_t* d_edge_hi, uint32_t* d_edge_cis, uint32_t* d_edge_trans, uint64_t* d_edge_off, uint64_t* n_edges_out, void* stream);
int aix_phase_solve_dev(uint64_t V, const uint32_t* d_var_unitig, const uint64_t* d_edge_off, uint64_t E, const uint32_t* d_edge_lo,
                        const uint32_t* d_edge_cis, const uint32_t* d_edge_trans, uint32_t min_link_reads, uint32_t min_link_permille,
                        uint32_t* d_site_block, uint8_t* d_site_phase, uint32_t* d_site_parent /* nullable */, uint8_t* d_edge_state /* nullable */,
                        uint64_t* d_counts /* nullable */, void* stream);
int aix_phase_tag_dev(uint64_t F, const uint64_t* d_frag_obs_off, uint64_t n_obs, const uint32_t* d_obs_site, const uint8_t* d_obs_allele, uint64_t V,
                      const uint32_t* d_site_block, const uint8_t* d_site_phase, uint32_t* d_tag_block, uint32_t* d_tag_h0, uint32_t* d_tag_h1,
                      uint32_t* d_tag_other, void* stream);
int aix_phase_solve(uint64_t V, const uint32_t* var_unitig, uint64_t N, const uint32_t* link_lo, const uint32_t* link_hi, const uint8_t* link_rel,
                    uint32_t min_link_reads, uint32_t min_link_permille, uint64_t* n_edges_out, uint32_t** edge_lo_out, uint32_t** edge_hi_out,
                    uint32_t** edge_cis_out, uint32_t** edge_trans_out, uint64_t** edge_off_out, uint8_t** edge_state_out /* nullable */,
                    uint32_t** site_block_out, uint8_t** site_phase_out, uint32_t** site_parent_out /* nullable */,
                    uint64_t** counts_out /* nullable */);

/* ------------------------------------------------------------------------------------------
 * Read cleaning: the weak-window profile of a read, its longest solid span, and single-base substitution fixes.
 * replaces, M reads at a time, the scaffolding of the reference's read-cleaning layer: READ::set_fm / STUPID_READ::set_fm
 *          (read.hpp:286-307, :392-402: fm[i] = get_freq of 23-window i; an error window iff fm[i] <= Settings::TRUE_ERRORS,
 *          settings.cpp:10, default 1), cut_end_from / cut_start_to (read.hpp:324-343) and the book-keeping of struct Correction /
 *          struct CorrectionErrors (read.hpp:36-117: simple_ok, simple_n0, simple_nM). The reference holds no corrector; the rules
 *          below are this library's. 23-mer handles only (AIX_ERR_MODE otherwise).
 *
 * Read r is the bytes s[0 .. L) = buf[start[r] .. end[r]) (the convention of get_read(start, end) and .ridx); reads are pairwise
 * disjoint. t = true_errors, V = verify (1 .. AIX_READFIX_MAX_VERIFY), F = max_fixes (0 .. AIX_READFIX_MAX_FIXES; 0 = profile and
 * trim only, nothing is written to the reads); V or F out of range is AIX_ERR_ARG.
 *   start > end or end > total_bytes: AIX_FIX_BAD_RANGE; L < 23: AIX_FIX_SHORT; L > AIX_READFIX_MAX_LEN: AIX_FIX_TOO_LONG. Such a
 *   read is left untouched and its other record words are 0. Nothing outside [0, total_bytes) is read whatever the arrays hold.
 *   Otherwise W = L - 22 windows; valid(i): the 23 bytes of window i are upper-case A/C/G/T; fm(i) = valid(i) ? get_freq(code of
 *   window i) : 0 (hash.hpp:123-140: forward strand, then the reverse complement; an invalid window is not probed);
 *   solid(i) = fm(i) > t, weak = !solid (read.hpp:296). weak_before = weak windows of the read as given.
 *   try(p, lo, hi), lo .. hi all containing p and hi - lo + 1 <= V: if s[p] is no ASCII letter there is no candidate (a separator is
 *   never written); else base b of A, C, G, T is a candidate iff every window lo .. hi of the read with s[p] := b is solid. Exactly
 *   one candidate: s[p] := b, log (p, old byte), fixes += 1 (simple_ok). None: n0 += 1 (simple_n0). Several: nM += 1 (simple_nM).
 *   Phase R: c = 1; while fixes < F: i = the smallest i >= c, i < W with solid(i - 1) && weak(i), none = stop; p = i + 22;
 *            try(p, i, min(i + V - 1, W - 1)); after a fix c stays, after a failure c = i + 1.
 *   Phase L: c = W - 2; while fixes < F: i = the largest i <= c, i >= 0 with weak(i) && solid(i + 1), none = stop; p = i;
 *            try(p, max(i - V + 1, 0), i); after a fix c stays, after a failure c = i - 1.
 *   solid() is always that of the read as fixed so far. Then weak_after = weak windows of the final read, and the longest run of
 *   solid windows [a, a + n), the earliest on ties, gives trim_start = a, trim_len = n + 22 in bases (what cut_start_to(a - 1) and
 *   cut_end_from(a + n + 22) keep, read.hpp:324-343); both 0 without a solid window.
 *   status: CLEAN weak_before == 0; FIXED weak_before > 0 && weak_after == 0; PARTIAL fixes > 0 && weak_after > 0; UNFIXED
 *   fixes == 0 && weak_after > 0.
 * Log rows of stride F: fix_pos[r * F + j], fix_old[r * F + j] (the byte that was there) for j < fixes in order of application;
 * nothing is written at or beyond `fixes` in a row, and nothing is written to buf except the fixed bytes.
 * Known limits: two errors closer than V + 22 can defeat both rules (n0); tf is not updated after a fix; indels, quality strings
 * and the 13-mer mode are out of scope.
 * ------------------------------------------------------------------------------------------ */
#define AIX_READFIX_MAX_LEN    4096u  /* longest read: the solid bitmap is 64 lanes x 64 windows, the bytes sit in 4 KiB of LDS */
#define AIX_READFIX_MAX_VERIFY 16u
#define AIX_READFIX_MAX_FIXES  16u
#define AIX_FIX_CLEAN     0
#define AIX_FIX_FIXED     1
#define AIX_FIX_PARTIAL   2
#define AIX_FIX_UNFIXED   3
#define AIX_FIX_SHORT     4
#define AIX_FIX_TOO_LONG  5
#define AIX_FIX_BAD_RANGE 6
/* one 32-byte record per read: the profile of set_fm (read.hpp:286-307), the counters of CorrectionErrors (read.hpp:36-117),
 * the span of cut_start_to / cut_end_from (read.hpp:324-343) */
typedef struct {
    uint32_t status, weak_before, weak_after, fixes, n0, nM, trim_start, trim_len;
} aix_readfix_t;
/* set_fm + cuts + Correction log (read.hpp:286-307, :324-343, :36-117) for M reads of a device buffer, fixed in place, asynchronous
 * on `stream`. M = 0 is AIX_OK; an empty index is AIX_ERR_UNSUPPORTED; a NULL pointer where one is needed is AIX_ERR_ARG. The
 * caller guarantees that the ranges are pairwise disjoint. */
int aix_reads_fix_dev(aix_index_t* h, char* d_buf, uint64_t total_bytes, const uint64_t* d_start, const uint64_t* d_end, uint64_t M,
                      uint32_t true_errors, uint32_t verify, uint32_t max_fixes, aix_readfix_t* d_rec,
                      uint32_t* d_fix_pos /* NULL iff max_fixes == 0 */, uint8_t* d_fix_old /* NULL iff max_fixes == 0 */, void* stream);
/* host twin (read.hpp:286-307, :324-343, :36-117): buf is fixed in place. Ranges that are not ascending and disjoint
 * (end[i] <= start[i + 1]) are refused with AIX_ERR_ARG. The caller's log rows are uploaded before the kernel runs, so that what
 * lies at or beyond `fixes` in a row comes back as it was. */
int aix_reads_fix(aix_index_t* h, char* buf, uint64_t total_bytes, const uint64_t* start, const uint64_t* end, uint64_t M,
                  uint32_t true_errors, uint32_t verify, uint32_t max_fixes, aix_readfix_t* rec, uint32_t* fix_pos /* NULL iff max_fixes == 0 */,
                  uint8_t* fix_old /* NULL iff max_fixes == 0 */);

/* ------------------------------------------------------------------------------------------
 * Sequences against the indexed reads: seed hits with strand, and votes per (read, strand, diagonal).
 * replaces, M sequences at a time, the loop a caller of the reference writes over the 23-windows of a sequence:
 *          AindexWrapper::get_positions per window (python_wrapper.cpp:800-831), get_rid / get_start per occurrence (:757-789) and
 *          get_read of 23 bytes per occurrence (:677-698) to tell the orientation — a bucket of the positions index holds both
 *          orientations of its k-mer without a strand bit (hash.hpp:150-170).
 * 23-mer handles only (AIX_ERR_MODE otherwise). The positions index (aix_aindex_attach*), the read intervals (aix_ridx_attach) and the
 * reads (aix_reads_attach*) must be attached: AIX_ERR_ARG otherwise. Sequences come as aix_coverage_batch takes them: sequence i is the
 * bytes seqs[offs[i] .. offs[i + 1]), offs ascending; a sequence of 2^32 bytes or more is AIX_ERR_ARG (query offsets are u32). seqs may
 * be NULL when no sequence is 23 bytes long (M empty sequences give all-zero offsets).
 * A sequence of length L has max(0, L - 22) windows, window q the 23 raw bytes at offset q. The _dev twins follow the sizing convention
 * of aix_positions_query_dev: offsets and *total_out always, entries only when the total fits `cap`, never at or beyond it, AIX_OK either
 * way; they return after the work on `stream` has completed. Host outputs are malloc'd (aix_free); M = 0 gives offsets = {0}.
 * ------------------------------------------------------------------------------------------ */
#define AIX_HIT_STRAND_MASK 3u   /* aix_seq_hits flag bits 0-1: 0 the reads hold the window's bytes at pos, 1 they hold the reverse
                                    complement of its sanitised code (kmers.cpp:12-40), 2 neither, or pos + 23 lies beyond the reads */
#define AIX_HIT_LOCATED     4u   /* bit 2: an interval was found for pos (python_wrapper.cpp:66-74)                                */
/* Seed hits (python_wrapper.cpp:800-831 per window): the hits of window q are exactly aix_positions_query of its 23 bytes — get_pfid on
 * the raw bytes, slot order, zeros skipped, the first max_per_kmer entries (0: all). CSR over sequences: hits of sequence i =
 * [seq_offsets[i], seq_offsets[i + 1]), ordered by window, then slot. Per hit: qoff (window offset), pos (0-based position in the reads),
 * rid / local (get_rid(pos), pos - get_start(pos), :757-789; 0 and pos without an interval) and flag (above). The reads are never read
 * at or beyond their attached length, whatever the positions array holds. */
int aix_seq_hits(aix_index_t* h, const char* seqs, const uint64_t* offs, uint64_t M, uint64_t max_per_kmer, uint64_t** seq_offsets_out,
                 uint32_t** qoff_out, uint64_t** pos_out, uint64_t** rid_out, int64_t** local_out, uint8_t** flag_out);
int aix_seq_hits_dev(aix_index_t* h, const char* d_seqs, const uint64_t* d_offs, uint64_t M, uint64_t max_per_kmer, uint64_t* d_seq_offsets,
                     uint32_t* d_qoff, uint64_t* d_pos, uint64_t* d_rid, int64_t* d_local, uint8_t* d_flag, uint64_t cap, uint64_t* total_out,
                     void* stream);   /* python_wrapper.cpp:800-831, 757-789, 677-698; d_seq_offsets: M + 1 */
/* Diagonal votes (the grouping a caller does over the hits above; python_wrapper.cpp:800-831, 757-789): of the hits of a sequence, those
 * with strand 0 or 1 and an interval, grouped by (rid, strand, diag), diag = local - qoff (strand 0) or local + qoff (strand 1) —
 * constant along a co-linear match in either orientation. One record per group of at least min_votes hits: rid, strand, diag, votes
 * (hits in the group), q_first / q_last (its smallest / largest qoff). CSR over sequences, records ascending by (rid, strand, diag).
 * Deterministic: independent of launch geometry and of every probe switch. */
int aix_seq_votes(aix_index_t* h, const char* seqs, const uint64_t* offs, uint64_t M, uint64_t max_per_kmer, uint64_t min_votes,
                  uint64_t** vote_offsets_out, uint64_t** rid_out, uint8_t** strand_out, int64_t** diag_out, uint32_t** votes_out,
                  uint32_t** qfirst_out, uint32_t** qlast_out);
int aix_seq_votes_dev(aix_index_t* h, const char* d_seqs, const uint64_t* d_offs, uint64_t M, uint64_t max_per_kmer, uint64_t min_votes,
                      uint64_t* d_vote_offsets, uint64_t* d_rid, uint8_t* d_strand, int64_t* d_diag, uint32_t* d_votes, uint32_t* d_qfirst,
                      uint32_t* d_qlast, uint64_t cap, uint64_t* total_out, void* stream);   /* python_wrapper.cpp:800-831, 757-789 */

/* ------------------------------------------------------------------------------------------
 * Sequences with mismatches against the indexed reads (Hamming seeds), and strand counts of k-mers.
 * replaces, M sequences at a time, the documented "Analysis Functions" iter_reads_by_sequence(seq, aindex, hd) and get_srandness(kmer,
 *          aindex) (API_DOCUMENTATION.md:232-255, 371-382; the reference holds no code for them, so this header is the contract) over
 *          hamming_distance (aindex.py:44-46): the loop a caller writes over aix_seq_hits, aix_reads_fetch and one comparison per candidate.
 * Restrictions and input form are those of aix_seq_hits: 23-mer handles only (AIX_ERR_MODE); positions index, read intervals and reads
 * attached (AIX_ERR_ARG otherwise); M sequences as seqs + offs[M + 1], each shorter than 2^32 bytes (AIX_ERR_ARG otherwise).
 *   hd            the largest distance reported
 *   seed_step     >= 1; 0 means 23
 *   max_per_kmer  as in aix_seq_hits
 * Seeds: the seeds of a sequence of length L >= 23 are its 23-windows at offsets q = 0, seed_step, 2 seed_step, .. <= L - 23; a shorter
 *   sequence has no seeds and no results.
 * Hits: the hits of a seed are exactly the aix_seq_hits hits of that window, cap included; only hits with strand 0 or 1 count.
 * Proposed alignments: a hit (q, pos, strand) proposes the alignment that starts at absolute reads offset a = pos - q (strand 0) or
 *   a = pos - (L - 23 - q) (strand 1). It is dropped when a < 0, when a + L exceeds the attached reads, or when no interval
 *   (rid, start, end) has start <= a and a + L <= end: plain containment in [start, end), not the off-by-one rule of get_rid
 *   (python_wrapper.cpp:757-789).
 * Distance: x_j = reads[a + j]; y_j = seq[j] (strand 0) or comp(seq[L - 1 - j]) (strand 1), comp: A <-> T, C <-> G, a <-> t, c <-> g, every
 *   other byte as it is. d = #{ j : x_j != y_j and x_j != 'N' and y_j != 'N' } on raw bytes: hamming_distance (aindex.py:44-46).
 * Output: an alignment is reported when d <= hd, each (a, strand) of a sequence once however many seeds proposed it. CSR over sequences:
 *   the records of sequence i are [find_offsets[i], find_offsets[i + 1]), ascending by (a, strand). Columns: pos = a, rid,
 *   local = a - start, strand, dist = d. The answer is independent of launch geometry and of every probe switch. The reads are never read
 *   at or beyond their attached length, whatever the positions array holds.
 * Completeness: the answer equals the full Hamming search over the indexed reads whenever the seed set holds hd + 1 pairwise disjoint
 *   windows that the positions index lists in full (max_per_kmer = 0, every occurrence indexed): one of them is free of mismatches. That is
 *   the case when hd < floor(L / 23) and seed_step is 1 or 23. An alignment with an 'N' inside every such window can be missed: the N rule
 *   forgives what the seed lookup does not.
 * The _dev twin follows the sizing convention of aix_seq_hits_dev: find_offsets and *total_out always, records only when the total fits
 * `cap`, never at or beyond it, AIX_OK either way; it returns after the work on `stream` has completed. Host outputs are malloc'd
 * (aix_free); M = 0 gives find_offsets = {0}.
 * ------------------------------------------------------------------------------------------ */
int aix_seq_find(aix_index_t* h, const char* seqs, const uint64_t* offs, uint64_t M, uint32_t hd, uint64_t seed_step, uint64_t max_per_kmer,
                 uint64_t** find_offsets_out, uint64_t** pos_out, uint64_t** rid_out, uint64_t** local_out, uint8_t** strand_out,
                 uint32_t** dist_out);   /* API_DOCUMENTATION.md:232-255, 371-382; aindex.py:44-46 */
int aix_seq_find_dev(aix_index_t* h, const char* d_seqs, const uint64_t* d_offs, uint64_t M, uint32_t hd, uint64_t seed_step,
                     uint64_t max_per_kmer, uint64_t* d_find_offsets, uint64_t* d_pos, uint64_t* d_rid, uint64_t* d_local, uint8_t* d_strand,
                     uint32_t* d_dist, uint64_t cap, uint64_t* total_out, void* stream);   /* API_DOCUMENTATION.md:232-255; d_find_offsets: M + 1 */
/* ------------------------------------------------------------------------------------------
 * Sequences against the indexed reads with substitutions, insertions and deletions (edit distance): indel-tolerant seed verification.
 * replaces the loop a caller writes over aix_seq_hits, aix_reads_fetch and a dynamic programme per candidate on the host; the reference's
 *          public module imports edit_distance beside hamming_distance (aindex/core/aindex.py:22-23) and holds no search over either, so
 *          this header is the contract. tests/seqedit_ref.py restates it.
 * Restrictions, input form, seeds and hits are those of aix_seq_find: 23-mer handles only (AIX_ERR_MODE); positions index, read intervals
 * and reads attached (AIX_ERR_ARG otherwise); M sequences as seqs + offs[M + 1], each shorter than 2^32 bytes; seed_step 0 means 23;
 * max_per_kmer as in aix_seq_hits; only hits with strand 0 or 1 count.
 *   ed            the largest distance reported, 0 <= ed <= 7 (AIX_SEQEDIT_MAX_ED of csrc/aix_seqhits.hpp); AIX_ERR_ARG otherwise
 * Oriented pattern: y_i (0 <= i < L) exactly as in aix_seq_find: seq[i] (strand 0) or comp(seq[L - 1 - i]) (strand 1), the same comp.
 * Proposal: a hit (q, pos, strand) anchors the diagonal a = pos - q (strand 0) or a = pos - (L - 23 - q) (strand 1); a is signed and may
 *   be negative. The hit belongs to the interval (rid, start, end) with start <= pos and pos + 23 <= end: plain containment of the SEED,
 *   found by bisection; without one the proposal is dropped. Text columns: lo = max(start, a - ed), hi = min(end, a + L + ed, attached
 *   length). Bytes of the reads outside [lo, hi) never reach a cell that exists, and nothing is read outside the attached reads,
 *   whatever the positions array holds.
 * Banded programme: cells (i, j) exist for 0 <= i <= L, lo <= j <= hi and |j - i - a| <= ed. Row 0: D[0][j] = 0 with start j (the start
 *   of the text is free). Three moves into (i, j), each from an existing cell: from (i - 1, j - 1) at cost 0 when x_{j-1} == y_{i-1} or
 *   either byte is 'N' (raw bytes: the N rule of hamming_distance), else 1, x_j = reads[j]; from (i - 1, j) at cost 1; from (i, j - 1) at
 *   cost 1. Every cell carries the pair (cost, start); its value is the lexicographic minimum over its incoming moves. The pattern is
 *   consumed whole, the end of the text is free: the proposal's result is the lexicographic minimum (dist, start, end = j) over the
 *   existing cells of row L, and the proposal survives when dist <= ed.
 * Output: one record per (start, strand) of a sequence: the lexicographically smallest (dist, end) among its surviving proposals that share
 *   that (start, strand). CSR over sequences, the records of sequence i = [find_offsets[i], find_offsets[i + 1]), ascending by
 *   (start, strand). Columns: start u64, end u64 (the alignment is reads[start, end)), rid u64, local u64 = start - interval start,
 *   strand u8, dist u32. The answer is independent of launch geometry and of every probe switch.
 * ed = 0: the band is one diagonal, so the records equal those of aix_seq_find(hd = 0) with start = a and end = a + L.
 * Near-duplicates: two seeds on different diagonals (on either side of an indel) can report overlapping records with different start for
 *   one underlying alignment: their bands differ, so their tie-breaks can differ. An alignment with at most ed edits lies inside the
 *   band of each of its untouched seeds, so this needs a second alignment within ed at another start that one band holds and the other
 *   does not: self-similar text (tandem repeats, homopolymers). This array surface keeps both; the list surface
 *   (AIndex.find_reads_by_sequence_edit_batch) merges per read.
 * Completeness: if an alignment of the whole pattern to a substring of one read has at most ed edits, one of ed + 1 pairwise disjoint seed
 *   windows is untouched by them; when it is listed in full its band holds the whole alignment (an alignment with at most ed edits drifts
 *   at most ed diagonals from an untouched seed). So for ed < floor(L / 23), seed_step 1 or 23, max_per_kmer = 0, every occurrence indexed
 *   and no 'N' in the seeds, the smallest distance per (rid, strand) equals that of an unbanded semi-global Levenshtein search (same N rule)
 *   over every read.
 * The _dev twin follows the sizing convention of aix_seq_find_dev: d_find_offsets[M + 1] and *total_out always, records only when the
 * total fits `cap`, never at or beyond it, AIX_OK either way; it returns after the work on `stream` has completed. Host outputs are
 * malloc'd (aix_free); M = 0 gives find_offsets = {0}.
 * ------------------------------------------------------------------------------------------ */
int aix_seq_edit(aix_index_t* h, const char* seqs, const uint64_t* offs, uint64_t M, uint32_t ed, uint64_t seed_step, uint64_t max_per_kmer,
                 uint64_t** find_offsets_out, uint64_t** start_out, uint64_t** end_out, uint64_t** rid_out, uint64_t** local_out,
                 uint8_t** strand_out, uint32_t** dist_out);   /* aindex/core/aindex.py:22-23 */
int aix_seq_edit_dev(aix_index_t* h, const char* d_seqs, const uint64_t* d_offs, uint64_t M, uint32_t ed, uint64_t seed_step,
                     uint64_t max_per_kmer, uint64_t* d_find_offsets, uint64_t* d_start, uint64_t* d_end, uint64_t* d_rid, uint64_t* d_local,
                     uint8_t* d_strand, uint32_t* d_dist, uint64_t cap, uint64_t* total_out, void* stream);   /* d_find_offsets: M + 1 */
/* get_srandness (API_DOCUMENTATION.md:232-255, 371-382) for N 23-mers in the input form of aix_positions_query (N * 23 bytes): per k-mer
 * total = its listed hits (aix_seq_hits of the 23 bytes, cut to max_per_kmer when that is > 0), plus = those whose strand flag is 0 (the
 * reads hold the k-mer as given), minus = those whose strand flag is 1 (they hold its reverse complement); total - plus - minus hits are
 * neither. Outputs hold N entries each (the caller's; device buffers for the _dev twin, which returns after the work on `stream` has
 * completed). N = 0 is AIX_OK. Same restrictions as aix_seq_hits. */
int aix_kmer_strands(aix_index_t* h, const char* kmers, uint64_t N, uint64_t max_per_kmer, uint64_t* plus_out, uint64_t* minus_out,
                     uint64_t* total_out);
int aix_kmer_strands_dev(aix_index_t* h, const char* d_kmers, uint64_t N, uint64_t max_per_kmer, uint64_t* d_plus, uint64_t* d_minus,
                         uint64_t* d_total, void* stream);   /* API_DOCUMENTATION.md:232-255 */

/* ------------------------------------------------------------------------------------------
 * k-mers by frequency: per-kid values, frequency spectrum and statistics, stable top-N / threshold selection, batch kid -> k-mer.
 * replaces AIndex.iter_kmers_by_frequency / get_top_kmers / get_kmer_frequency_stats (aindex/core/aindex.py:594-793: a Python loop over
 *          every kid and a sort of all of them) and, N at a time, AindexWrapper::get_kmer_by_kid / get_kmer_info
 *          (python_wrapper.cpp:718-755).
 * Value of entry i. 23-mer handle, i < n: get_tf_value_23mer(get_kmer_by_kid(i)) (python_wrapper.cpp:610-627, 718-724) = the two-strand
 * probe of checker[i] & (2^46 - 1), forward strand first; NOT tf[i] (they differ where a slot holds a key that is not in its own MPHF
 * slot). 13-mer handle, i < 4^13: (uint32_t) tf13[i] in file order (get_13mer_tf_array, :983-991); the label of entry i is the base-4
 * spelling of i (aindex.py:574-592). Order: descending value, ties in ascending i (Python's stable sort(key = tf, reverse = True),
 * aindex.py:643, 671) = ascending by ((2^32 - 1 - v) << 32) | i. Selection(min_v, max_items): the first max_items (0 = all) entries
 * with v >= min_v in that order; total = the number of entries with v >= min_v before the cut. Spectrum(nbins >= 2): hist[j] = #{i : v_i = j}
 * for j < nbins - 1, hist[nbins - 1] = #{i : v_i >= nbins - 1}. The answers do not depend on any probe switch.
 * Both handle kinds are accepted. AIX_ERR_ARG for nbins < 2 or a NULL output; AIX_ERR_NOMEM, before anything is allocated, for a size
 * that cannot be held (nbins > 2^32, N >= 2^56). The _dev forms of the selection follow aix_positions_query_dev: *n_out / *total_out are
 * always produced, entries only when *n_out <= cap, nothing is written at or beyond *n_out. Stream contract, per entry point:
 * aix_select_dev and aix_top_kmers_dev read the size of the selection back, so they return after all their work on `stream` has completed
 * (d_kmers included); aix_tf_spectrum_dev on a 23-mer handle also returns completed (its values live in pool scratch that goes back idle),
 * on a 13-mer handle it is asynchronous; aix_values_narrow_dev, aix_spectrum_dev, aix_kmer_values_dev and aix_kmers_by_kid_dev are
 * asynchronous on `stream`. Host arrays handed out are malloc'd (aix_free).
 * ------------------------------------------------------------------------------------------ */
#define AIX_SPECTRUM_STATS 8   /* words of a statistics record: n, non-zero entries, max, smallest non-zero value (0 if none), sum — of the
                                  u32 values — then non-zero entries, max and sum at full width (they differ from words 1, 2, 4 only for a
                                  u64 source: get_13mer_statistics, python_wrapper.cpp:1038-1068, reads the u64 table) */
/* Array level (no handle; device pointers of the current device). These also serve the tensors aix_count23_fixed_dev (u32) and
 * aix_count13_dev (u64) leave in HBM. */
/* the u32 view of n u64 entries (get_13mer_tf_array, python_wrapper.cpp:983-991) */
int aix_values_narrow_dev(const uint64_t* d_in, uint64_t n, uint32_t* d_out, void* stream);
/* spectrum (d_hist[nbins]) and statistics (d_stats[AIX_SPECTRUM_STATS]) of n entries of elem_bytes 4 (u32) or 8 (u64, binned by their
 * u32 view); what get_kmer_frequency_stats computes (aindex.py:703-793). Asynchronous on `stream`. */
int aix_spectrum_dev(const void* d_values, int elem_bytes, uint64_t n, uint64_t nbins, uint64_t* d_hist, uint64_t* d_stats, void* stream);
/* Selection(min_v, max_items) over d_values[n], n < 2^32 (aindex.py:636-647): d_idx[j] / d_val[j] = index and value of the j-th entry.
 * d_val may be NULL. */
int aix_select_dev(const uint32_t* d_values, uint64_t n, uint32_t min_v, uint64_t max_items, uint32_t* d_idx, uint32_t* d_val, uint64_t cap,
                   uint64_t* n_out, uint64_t* total_out, void* stream);
/* Handle level. */
/* d_out[i] = value of entry i for every i < n (aindex.py:661-664 for every kid); asynchronous on `stream` */
int aix_kmer_values_dev(aix_index_t* h, uint32_t* d_out, void* stream);
/* spectrum and statistics of the values (aindex.py:703-793); hist_out[nbins], stats_out[AIX_SPECTRUM_STATS] are the caller's */
int aix_tf_spectrum(aix_index_t* h, uint64_t nbins, uint64_t* hist_out, uint64_t* stats_out);
int aix_tf_spectrum_dev(aix_index_t* h, uint64_t nbins, uint64_t* d_hist, uint64_t* d_stats, void* stream);   /* aindex.py:703-793; 23-mer handle: completed on return */
/* iter_kmers_by_frequency(min_tf, max_kmers) (aindex.py:594-681; max_kmers 0 = all): kid, value and — when kmers_out is not NULL — the
 * k ASCII bytes of every selected entry (get_kmer_by_kid, python_wrapper.cpp:718-724; 13-mer: the spelling of the index). */
int aix_top_kmers(aix_index_t* h, uint32_t min_tf, uint64_t max_kmers, uint32_t** kid_out, uint32_t** tf_out, char** kmers_out /* nullable */,
                  uint64_t* n_out, uint64_t* total_out);
int aix_top_kmers_dev(aix_index_t* h, uint32_t min_tf, uint64_t max_kmers, uint32_t* d_kid, uint32_t* d_tf /* nullable */,
                      char* d_kmers /* nullable, cap * k bytes */, uint64_t cap, uint64_t* n_out, uint64_t* total_out, void* stream);   /* aindex.py:594-681 */
/* get_kmer_by_kid / get_kmer_info (python_wrapper.cpp:718-755) for N kids: row i of kmers_out = the k ASCII bytes of checker[kid[i]] &
 * (2^46 - 1), of rc_out (nullable) its reverse complement, tf_out[i] (nullable) = tf[kid[i]] read directly (:753, not the probe). For
 * kid[i] >= n the rows are k NUL bytes and tf 0. 13-mer handle: the base-4 spelling of kid[i] and (uint32_t) tf13[kid[i]]. */
int aix_kmers_by_kid(aix_index_t* h, const uint64_t* kid, uint64_t N, char* kmers_out, char* rc_out /* nullable */, uint32_t* tf_out /* nullable */);
int aix_kmers_by_kid_dev(aix_index_t* h, const uint64_t* d_kid, uint64_t N, char* d_kmers, char* d_rc /* nullable */, uint32_t* d_tf /* nullable */,
                         void* stream);   /* python_wrapper.cpp:718-755; asynchronous on `stream` */

/* The same normalisation for a buffer already in HBM (byte-identical output; the readers are finite-state transducers,
 * resolved with a parallel scan of per-chunk transition functions). format must be PLAIN, FASTA or FASTQ; d_out holds
 * len+1 bytes; *out_len is a HOST pointer; the call synchronises the stream. */
int aix_normalize_reads_dev(const char* d_raw, uint64_t len, int format, int fasta_mode, char* d_out, uint64_t* out_len, void* stream);

/* ------------------------------------------------------------------------------------------
 * Synthetic inputs generated directly in HBM (mirrored by aindex_amd/synth.py).
 * ------------------------------------------------------------------------------------------ */
int aix_synth_genome_dev(uint64_t seed, uint64_t length, char* d_out, void* stream);
int aix_synth_kmers_dev(uint64_t seed, uint64_t first, uint64_t N, int k, char* d_out, void* stream);
int aix_synth_mix23_dev(uint64_t seed, const char* d_genome, uint64_t genome_len, uint64_t first, uint64_t N,
                        char* d_out /* N*23 */, void* stream);   /* Q_mix: 50 % genome windows on a random strand, 50 % random */
int aix_synth_reads_dev(uint64_t seed, const char* d_genome, uint64_t genome_len, uint64_t first_read,
                        uint64_t n_reads, uint32_t read_len, int rc_half, uint32_t n_rate_ppm,
                        char* d_out /* n_reads*(read_len+1) */, void* stream);

/* ------------------------------------------------------------------------------------------
 * MWHC builder (host code, like the reference's). replaces `compute_mphf_seq <keys.txt> <out.pf>`
 * (src/emphf/compute_mphf_generic.hpp:19-61, mphf.hpp:21-67, hypergraph_sorter_seq.hpp:29-102):
 * bit-identical .pf image for the same key list (same mt19937_64(37) seed stream, peeling order
 * and value assignment). *pf_out is malloc'd; release with aix_free. AIX_ERR_CONFLICT when the key
 * list is not peelable after 64 seeds (duplicate keys; the reference would loop forever).
 * ------------------------------------------------------------------------------------------ */
int aix_pf_build(const char* keys /* n*key_len bytes */, uint64_t n, uint32_t key_len, void** pf_out, uint64_t* pf_len);
int aix_pf_build_ragged(const char* bytes, const uint64_t* offsets /* n+1 */, uint64_t n, void** pf_out, uint64_t* pf_len);
int aix_pf_build_codes(const uint64_t* codes, uint64_t n, int k, void** pf_out, uint64_t* pf_len); /* keys = ASCII of 2-bit codes */
int aix_pf_build_all_13mers(void** pf_out, uint64_t* pf_len);   /* generate_all_13mers + build_13mer_hash */
/* The same construction on the GPU for keys (2-bit codes, ASCII-hashed) already in HBM: same seed stream, hash domain
 * and hypergraph, parallel peeling — a valid emphf .pf that the reference loads and evaluates, but NOT byte-identical
 * to compute_mphf_seq's (the bit-pair values depend on the peeling order). n and 3*hash_domain must be < 2^32. */
int aix_pf_build_codes_dev(const uint64_t* d_codes, uint64_t n, int k, int device, void* stream, void** pf_out, uint64_t* pf_len);
void aix_free(void* p);

/* Roofline probe: n_access uniform-random reads of elem_bytes (4, 8, 16; 32, 64, 128 with unroll 1: the whole element) over a table
 * of n_elems elements in HBM, `unroll` (1 or 4) independent reads in flight per lane. Measurement aid only. */
int aix_bench_gather_dev(const void* d_table, uint64_t n_elems, int elem_bytes, int unroll, uint64_t n_access,
                         uint64_t seed, uint64_t* d_sink, void* stream);

/* Diagnostics of the placement experiments (scripts/gpu_r3_relocate.py, gpu_r3_bloomlot.py): move the verification table of a
 * 23-mer handle into d_dst (nb * 128 bytes, caller-owned, kept alive by the caller) or, with NULL, into a block allocated now; move the
 * absence filter into a block allocated now (behind `pad_bytes` of padding; the old block and the padding are deliberately not freed, so
 * that successive moves land on different pages). Answers are unchanged. Not for production use. */
int aix_debug_relocate_table(aix_index_t* h, void* d_dst);
int aix_debug_relocate_bloom(aix_index_t* h, uint64_t pad_bytes);
int aix_debug_pointers(const aix_index_t* h, uint64_t out[5]);   /* device addresses: MPHF records, side index, unfiled keys, table, absence filter */
int aix_debug_rehome(aix_index_t* h, uint32_t mask);   /* 1 MPHF records, 2 side index, 4 unfiled keys, 8 table, 16 absence filter -> fresh blocks */
/* Host copy of the absence filter of a 23-mer handle (nwords = its absence_filter_words; AIX_ERR_ARG on any other size or without a filter).
 * The filter is built when the index is opened and has no file format; only the test-suite reads it. */
int aix_debug_filter_words(aix_index_t* h, uint64_t* out, uint64_t nwords);

/* self-test hook of the GPU suite: lower bounds of keys[i] and keys[i] + 1 in a sorted u16 array of n entries, computed by the wave-wide search with
 * which the partition kernels find a partition's chunks; out[2 i], out[2 i + 1]. Device pointers. */
int aix_selftest_lower_bound_dev(const uint16_t* d_sorted, uint32_t n, const uint32_t* d_keys, uint32_t nkeys, uint32_t* d_out, void* stream);

/* self-test hook for the CPU test-suite: the exact-modulo used by the kernels, run on the host */
uint64_t aix_selftest_mod(uint64_t h, uint64_t d);
uint64_t aix_selftest_revcomp(uint64_t code, int k);

#ifdef __cplusplus
}
#endif
#endif /* AINDEX_HIP_H */
