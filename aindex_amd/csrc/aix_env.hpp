// aix_env.hpp — private: the one place where the library reads its environment. Every switch goes through one of the typed readers
// below; a switch that more than one place reads has a named accessor, so that its range and default are written once. A value out of
// range is ignored (the default holds). WHEN a switch is read belongs to its caller: "once" switches sit behind a function-local
// static there, everything else is read per call (the tests and bench.py flip those between calls of one process).
//
// The switches (T tuning, AB = A/B measurement switch, H = test hook; where read; range; default):
//   at open of a 23-mer handle (aix_index.hip)
//     AIX_BUCKET_TABLE             T   0 / 1                         1      0: no verification table, every probe through the MPHF records
//     AIX_BUCKET_LOAD              T   0.25 .. 8                     4      mean keys per eight-entry bucket
//     AIX_BUCKET_LANES             T   1, 2, 4, 8                    8      lanes that share one bucket read (fixes the width for every consumer)
//     AIX_BLOOM_BITS               T   0, 4 .. 64                    16     absence-filter bits per key, 0 = no filter
//     AIX_MINIMIZER_TABLE          AB  0 / 1                         0      build the minimizer-keyed copy for the streaming counter
//     AIX_MINIMIZER_LOAD           T   0.25 .. 16                    2      mean keys per minimizer bucket
//     AIX_MINIMIZER_CAP            H   1 .. AIX_MK_ENTRIES           max    entries of a minimizer bucket a lane reads
//   per call, the counters (aix_count.hip, aix_count13.hip)
//     AIX_COUNT13_ATOMICS          AB  set / not set                 -      13-mer count through scattered atomics
//     AIX_COUNT13_PIECE            H   1 .. 2^31                     2^31   window starts per piece of the 13-mer counter
//     AIX_COUNT13_TEST_REGION      H   >= 1                          -      chunk ids per workgroup (an undersized region must fail loudly)
//     AIX_C13_PREFETCH             AB  0 / 1                         0      prefetching variant of the split kernel
//     AIX_COUNT_TEST_WORKSPACE_MAX H   bytes                         -      count workspaces above this "do not fit"
//     AIX_COUNT23_ATOMICS          AB  set / not set                 -      count23 back end 1 (memory-side atomics) at every size
//     AIX_COUNT23_HIST_MIN         H   windows                       2^22   from here count23 leaves back end 1
//     AIX_COUNT23_VIA_K1           AB  0 / 1                         auto   count23 back end 3 (distinct k-mers first) forced on / off
//     AIX_COUNT23_PIECE            T   1 .. 2^31                     2^30   windows per pass of the slot stream
//     AIX_COUNT23_OVERLAP          AB  0 / 1                         1      probe of piece i + 1 on a second stream
//     AIX_COUNT23_RUN              AB  0, 16, 32                     0      windows per lane of the slot probe
//     AIX_COUNT23_TEST_RANGE_BITS  H   4 .. 26                       26     slots per histogram pass = 2^bits
//   first multi-piece count23 call of a handle (aix_count.hip)
//     AIX_COUNT23_HIST_CUS         AB  n[,style], n 8 .. 224         -      CU-masked streams for histogram and probe
//   per call, the binned tf lookup (aix_lookup_binned.hip)
//     AIX_LOOKUP_BINNED            AB  0, 1, 2                       1      0 never, 1 auto (candidate batches, the device gate decides per piece), 2 always (no gate, no minimum)
//     AIX_LOOKUP_BINNED_MIN        T   queries                       2^24   smallest batch that is a candidate
//     AIX_LOOKUP_SLICE_BYTES       T/H 8 .. 2 MiB                    1 MiB  filter slice = one bin (small values: many bins on a tiny index)
//     AIX_LOOKUP_PIECE             H   1 .. 2^27                     2^27   queries per piece
//     AIX_LOOKUP_TEST_BIN_CAP      H   records                       -      capacity of a bin's region (forces the overflow route)
//     AIX_LOOKUP_TEST_GRID_A       H   1 .. 768                      768    workgroups of pass A at most (many tiles per workgroup on a small batch)
//     AIX_LOOKUP_TEST_GRID_B       H   1 .. 1024                     1024   workgroups of pass B at most (many tickets per workgroup on a small batch); with the coarse image at most 256
//     AIX_LOOKUP_COARSE            AB  0 / 1                         1      pass B tests the coarse image of its slice in LDS before it reads the filter word
//     AIX_LOOKUP_TEST_COARSE_MAX   H   0 .. 2^17 words               2^17   widest slice whose coarse image pass B takes into LDS (wider: pass B without the image)
//   per call, elsewhere
//     AIX_DISTINCT_PIECE           H   1 .. 2^31                     2^30   windows per K1 piece (aix_merge.hip entry points, aix_count.hip, aix_ingest.hip)
//     AIX_POSITIONS_PIECE          H   1 .. 2^31                     2^30   windows per piece of the positions fill (aix_positions.hip)
//     AIX_A2_MSD                   AB  0 / 1                         auto   positions grouping by MSD partition forced on / off (aix_a2msd.hip)
//     AIX_A2_TARGET                AB  >= 1                          1024   windows per bucket the MSD partition aims at
//     AIX_A2_TEST_CAP              H   1 .. A2_CAP - 1               A2_CAP bucket capacity (forces the set-aside path)
//     AIX_A2_TEST_NOMEM            H   set / not set                 -      the MSD workspace "does not fit"
//     AIX_K1_ROCPRIM               AB  set / not set                 -      K1 through the radix sort (aix_k1.hip)
//     AIX_K1_TEST_REGION           H   >= 1                          -      chunk ids per workgroup of K1
//     AIX_DBJ_FILTER               AB  0, 1, 2                       1/2/0  (neighbours / walks / read fixes) absence filter of those kernels: 0 per-trip gauge, 1 always, 2 never (aix_debruijn.hip, aix_readfix.hip; aix_unitigs.hip takes the walks' default)
//     AIX_UG_TEST_GRID             H   1 .. 65536                    -      workgroups at most of k_ug_ports and of every grid-stride launch of the compaction (many trips on a small index; aix_unitigs.hip, aix_graphclean.hip)
//     AIX_INGEST_PART_MB           T   1 .. 2047                     256    part size of the streaming ingestion (aix_ingest.hip)
//     AIX_INGEST_TEST_PART         H   >= 1 bytes                    -      part size in bytes (cuts everywhere)
//   once per process
//     AIX_HOST_COPY_THREADS        T   1 .. 64                       auto   host threads of the lookup staging (aix_lookup.hip)
//     AIX_PIPE_TEST_FAIL_CHUNK     H   chunk number                  -      the chunk of a large host batch whose launch "fails"
//     AIX_INGEST_THREADS           T   1 .. 64                       auto   host threads of the ingestion (aix_ingest.hip)
//     AIX_PINNED_CACHE_MB          T   MiB                           1024   pinned staging blocks kept between calls
//     AIX_SCRATCH_CACHE_GB         T   GiB (below 0 = 0)             40     device scratch kept between calls (aix_pool.hip)
//     AIX_GRID_PER_CU              AB  1 .. 1024                     256    workgroups per CU of the grid-stride kernels (aix_launch.hpp)
//     AIX_PROBE_LDS_PAD            AB  bytes                         0      unused LDS per workgroup of the slot probe
//     AIX_A2_PROBE_LANES           AB  2, 4, 8                       handle lanes per bucket read of the positions probe (aix_positions.hip)
//     AIX_C13_SHAPE                AB  s...                          -      the small workgroup shape of the split kernel (aix_count13.hip)
//     AIX_C13_GRID                 AB  1 .. 4096                     256    workgroups of the split
//     AIX_C23_SLOTS_REGS           AB  0 / 1                         1      slot source of the histogram keeps its windows in registers
#pragma once
#include <stdint.h>

#include <climits>
#include <cstdlib>
#include <cstring>

namespace aix {

// the readers (static: they stay out of the library's exported symbols)
static inline const char* env_str(const char* name) { return getenv(name); }
static inline bool env_flag(const char* name) { return env_str(name) != nullptr; }                                       // set / not set
static inline bool env_bool(const char* name, bool dflt) { const char* e = env_str(name); return e ? atoi(e) != 0 : dflt; }
template <typename T, typename P>
static inline T env_ranged(const char* name, T lo, T hi, T dflt, P parse) {
    const char* e = env_str(name);
    if (!e) return dflt;
    const T v = parse(e);
    return v >= lo && v <= hi ? v : dflt;
}
static inline long env_int(const char* name, long lo, long hi, long dflt) { return env_ranged(name, lo, hi, dflt, [](const char* e) { return atol(e); }); }
static inline uint64_t env_u64(const char* name, uint64_t lo, uint64_t hi, uint64_t dflt) { return env_ranged(name, lo, hi, dflt, [](const char* e) { return (uint64_t)strtoull(e, nullptr, 10); }); }
static inline double env_double(const char* name, double lo, double hi, double dflt) { return env_ranged(name, lo, hi, dflt, [](const char* e) { return atof(e); }); }
static inline char env_char(const char* name) { const char* e = env_str(name); return e ? e[0] : 0; }                    // first character, 0 when not set
static inline void env_int_pair(const char* name, int* a, int* b) {                                                      // "a[,b]"; what is missing stays as it is
    const char* e = env_str(name);
    if (!e) return;
    *a = atoi(e);
    if (const char* c = strchr(e, ',')) *b = atoi(c + 1);
}

// windows per piece of the counters: 32-bit window indices inside a piece allow 2^31
static inline uint64_t env_count_piece(const char* name, uint64_t dflt) { return env_u64(name, 1, 1ull << 31, dflt); }
static inline uint64_t env_distinct_piece() { return env_u64("AIX_DISTINCT_PIECE", 1, 1ull << 31, 1ull << 30); }
static inline uint64_t env_positions_piece() { return env_u64("AIX_POSITIONS_PIECE", 1, 1ull << 31, 1ull << 30); }
static inline bool env_bucket_table() { return env_bool("AIX_BUCKET_TABLE", true); }

}  // namespace aix
