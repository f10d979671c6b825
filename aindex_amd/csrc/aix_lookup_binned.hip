// aix_lookup_binned.hip — tf lookups of large, absent-heavy 23-mer batches on a canonical index with the absence filter read
// from L2 instead of the fabric. The direct kernel sends one scattered 8-byte filter read per query past L2 (the
// filter is ~100 MB) and runs at the chip's random-line request rate. Here a piece of the batch (<= 2^27 queries) goes through
//   k_lb_gate     ~16 K evenly spaced queries against the filter: the piece is binned iff fewer than a quarter of them pass
//                 (FilterGauge's rule). One flag in the workspace header; every kernel behind it reads the flag first and
//                 the one not chosen returns at once, so there is no host synchronisation.
//   k_lb_bin      pass A: load, encode, strand pick and the filter key of the canonical code (no ASCII of the other strand and no
//                 Jenkins hash: the filter is keyed by the code, aix_device.hpp); one 8-byte record per clean query,
//                 counting-sorted by filter slice in LDS per 4096-query tile and flushed into 256-record chunks of a per-slice
//                 region (chunks come from a per-slice cursor; a workgroup asks for all chunks of a tile and slice at once).
//                 The flush writes whole 128-byte lines (LB_LINE = 16 records): what a slice's run leaves over stays in an LDS carry
//                 (fewer than LB_LINE records per slice, 128 bytes of dynamic shared memory each) and goes in front of the slice's
//                 run of the workgroup's next tile; the last tile writes everything. Chunks are 2 KiB and regions 256-byte
//                 aligned, so a line never straddles chunks. One wave flushes a slice and advances its chunk, fill and counts;
//                 nobody else touches them until the next tile's first barrier, so a tile has five barriers and none at its end.
//                 LDS: 32 KiB of sorted records + 6 KiB of per-slice tables + the carry = 50 KiB at 96 slices (three workgroups
//                 per CU), 70 KiB at 256 (two).
//                 out[i] = 0 for every query. Queries with other bytes, and records whose slice region is full, go onto the
//                 survivor list instead, appended by the wave that flushes them. A lane fetches a query's dwords one query before it encodes them (lb_fetch), encodes with
//                 encode23_clean, finds the slice with a shift where the slice width is a power of two (the shipped 2^17 words is),
//                 and the tile's zeros are written with 16-byte stores behind the query loop: 80 VGPRs, three workgroups per CU.
//   k_lb_filter   pass B: chunks in slice order across the whole grid, so that the chip reads one or two slices (~1 MiB each)
//                 at a time and every XCD holds them in its L2. The chunks are handed out in order through eight ticket counters,
//                 four chunks (1024 records) per ticket to a workgroup of 512 threads: ~107 000 returning atomics per 10^8
//                 queries, 128 workgroups on a counter. A record that passes is appended to the survivor list.
//   k_lb_filter_coarse  pass B as it runs by default (AIX_LOOKUP_COARSE): one workgroup of 1024 threads per CU holds the coarse image
//                 of a slice (bloom_fold: one byte per filter word, 128 KiB at the shipped slice width) in LDS and reads the filter
//                 word only of the records whose image bit is set, about 4 in 10 of an absent-heavy batch. Every ticket counter
//                 owns the slices s with s % 8 == its number. The image is folded once per handle (k_lb_fold). k_lb_filter
//                 remains for slices whose image does not fit (2 MiB slices) and as the A/B switch.
//   k_lookup23_list (aix_lookup.hip) pass C: the survivors through the ordinary probe.
// A record = query index in the piece (27 bits) | filter word inside the slice (18 bits) | the 16 bits of the filter key from which
// bloom_mask takes all four bit positions: 8 bytes, three bits spare. Pass B therefore lets exactly the filter's positives through
// (~0.5 % of absent queries); pass C goes through the ordinary probe, which consults the filter again, so answers do not depend on it.
#include <algorithm>

#include "aix_env.hpp"
#include "aix_handle.hpp"

namespace aix {

static constexpr int LB_TB = 512;                      // threads of pass A
static constexpr int LB_QPL = 8;                       // queries per lane and tile
static constexpr int LB_TILE = LB_TB * LB_QPL;         // 4096 queries per tile: 32 KiB of records in LDS
static constexpr int LB_CH = 256;                      // records per chunk (2 KiB)
static constexpr int LB_LINE = 16;                     // records per 128-byte line: pass A writes whole lines and carries the rest of a slice's run
static constexpr int LB_MAXBINS = 256;
static_assert(LB_CH % LB_LINE == 0 && LB_LINE <= 64, "lines do not straddle chunks; one wave instruction moves a carry");
static constexpr unsigned LB_GRID_A = 768;             // three workgroups of pass A per CU (38 KiB of LDS each + 128 bytes per slice: 50 KiB at 96 slices)
static constexpr int LB_FB = 512;                      // threads of pass B: a lane takes one record of each chunk group of a trip
static constexpr int LB_CPG = LB_FB / LB_CH;           // chunks per chunk group: one record per lane
static constexpr int LB_U = 2;                         // chunk groups per trip of a pass-B workgroup (independent loads)
static constexpr int LB_CPT = LB_U * LB_CPG;           // chunks per ticket = per trip: 1024 records
static constexpr int LB_TICKETS = 8;                   // pass B hands its tickets out in order through these counters (one per XCD under round-robin dispatch)
static constexpr int LB_SURV = 4096;                   // survivors a pass-B workgroup can hold in LDS
static constexpr int LB_FLUSH_AT = LB_SURV - LB_U * LB_FB;   // it appends them once it holds more than this, so that a trip's records always fit
static constexpr unsigned LB_GRID_B = 1024;            // four workgroups per CU: 1024 * 1024 ~ 10^6 records in flight, one slice's worth
static_assert(LB_FB % LB_CH == 0 && LB_FB >= LB_MAXBINS && LB_FB % 64 == 0, "pass B scans the slices' chunk counts with one lane per slice");
static_assert(LB_FLUSH_AT > 0, "LB_SURV holds the flush threshold plus one trip's records");
// pass B with the coarse image of the slice in LDS (k_lb_filter_coarse): one workgroup of 1024 threads per CU
static constexpr int LBC_FB = 1024;                    // threads: a lane takes one record of each chunk group of a ticket
static constexpr int LBC_CPG = LBC_FB / LB_CH;         // chunks per chunk group
static constexpr int LBC_U = 4;                        // chunk groups per ticket (independent loads)
static constexpr int LBC_CPT = LBC_U * LBC_CPG;        // chunks per ticket: 4096 records
static constexpr int LBC_SURV = 6144;                  // survivors a workgroup can hold in LDS
static constexpr int LBC_FLUSH_AT = LBC_SURV - LBC_U * LBC_FB;
static constexpr unsigned LBC_GRID = 256;              // one workgroup per CU
static constexpr uint32_t LBC_MAX_WPS = 1u << 17;      // a slice's coarse image is one byte per filter word: 128 KiB of the CU's 160 KiB of LDS
static_assert(LBC_FB % LB_CH == 0 && LBC_FB >= LB_MAXBINS && LBC_FLUSH_AT > 0, "as for pass B without the image");
static_assert(LBC_MAX_WPS + 4 * (LBC_SURV + 2 * LB_MAXBINS + 1 + LBC_FB / 64 + 5) <= 160u << 10, "image, survivors and tables fit the LDS of a CU");
static constexpr uint32_t LB_SAMPLES = 16384;
static constexpr uint32_t LB_IDX_BITS = 27, LB_WORD_BITS = 18, LB_MASK_BITS = 16;
static_assert(LB_MASK_BITS == 16 && LB_IDX_BITS + LB_WORD_BITS + LB_MASK_BITS <= 64, "the record holds the 16 bits bloom_mask reads");
static constexpr uint32_t LB_NONE = 0xFFFFFFFFu;
static constexpr uint32_t LB_LO_BITS = 32 - LB_IDX_BITS, LB_META_LO = 9;   // pass A's per-query word: slice (9 bits) | the word-field bits of a record's low dword | rank << 16
static_assert(LB_IDX_BITS < 32 && LB_MAXBINS < (1 << LB_META_LO) && LB_META_LO + LB_LO_BITS <= 16 && LB_TILE <= (1 << 13), "that word never equals LB_NONE");
static constexpr uint64_t LB_HDR_BYTES = 4096;         // header (4 words) + cursors (LB_MAXBINS words) + ticket counters (a 128-byte line each), zeroed per piece
static constexpr int LB_NSTATS = 6;                    // counters of a handle (LbWs::stats)
enum { LB_FLAG = 0, LB_PASSED = 1, LB_DONE = 2, LB_NSURV = 3, LB_CURSOR = 16, LB_TICKET = 512 };

static constexpr uint32_t LB_NO_SHIFT = 32;
struct LbGeom {
    uint32_t nbins;        // filter slices
    uint32_t wps;          // filter words per slice (<= 2^18)
    uint32_t inv;          // floor(2^32 / wps), for word / wps
    uint32_t shift;        // log2(wps) where wps is a power of two (the shipped 2^17 is): word / wps is a shift; otherwise LB_NO_SHIFT
    uint32_t cap;          // chunks per slice region
};
struct LbWs {
    uint32_t* hdr;                 // LB_FLAG .. LB_NSURV, cursors from LB_CURSOR
    uint32_t* list;                // survivor list: query indices of the piece
    uint32_t* cnt;                 // [nbins * cap] records in each chunk
    uint64_t* rec;                 // [nbins * cap * LB_CH]
    unsigned long long* stats;     // pieces binned, pieces direct, records that overflowed, survivors; records tested against the coarse image, records sent on to the filter word
};

// the filter key of the code query23 (aix_lookup.hip) probes: that of the canonical strand; false = other bytes
__device__ __forceinline__ bool lb_hash(uint64_t w0, uint64_t w1, uint64_t w2, uint32_t& hw, uint32_t& hb) {
    uint64_t code;
    if (!encode23_clean(w0, w1, w2, code)) return false;
    const uint64_t r = revcomp(code, 23);
    filter_key(code <= r ? code : r, hw, hb);
    return true;
}

// filter word -> its slice and the word inside the slice; the branch is the same for every query of a launch
__device__ __forceinline__ void lb_slice(uint32_t word, const LbGeom& g, uint32_t& bin, uint32_t& wi) {
    if (g.shift != LB_NO_SHIFT) {
        bin = word >> g.shift;
        wi = word & (g.wps - 1);
    } else {
        bin = __umulhi(word, g.inv);                             // word / wps, at most one too small
        wi = word - bin * g.wps;
        if (wi >= g.wps) { wi -= g.wps; ++bin; }
    }
}

__global__ void __launch_bounds__(256) k_lb_gate(const uint64_t* __restrict__ bloom, uint32_t nbloom, const uint8_t* __restrict__ q, uint32_t n,
                                                 uint32_t nsamp, int force, uint32_t* __restrict__ hdr, unsigned long long* __restrict__ stats) {
    if (force) {
        if (blockIdx.x == 0 && threadIdx.x == 0) { hdr[LB_FLAG] = 1u; atomicAdd(&stats[0], 1ull); }
        return;
    }
    __shared__ uint32_t s_pass;
    if (threadIdx.x == 0) s_pass = 0;
    __syncthreads();
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    bool pass = false;
    if (s < nsamp) {
        const uint64_t i = (uint64_t)s * n / nsamp;
        uint64_t w0, w1, w2;
        uint32_t hw, hb;
        load23(q + 23 * i, w0, w1, w2);
        pass = true;                                            // other bytes: the direct probe's business
        if (lb_hash(w0, w1, w2, hw, hb)) {
            const uint64_t m = bloom_mask(hb);
            pass = (bloom[bloom_word(hw, nbloom)] & m) == m;
        }
    }
    const uint32_t wave = (uint32_t)__popcll(__ballot(pass));
    if ((threadIdx.x & 63) == 0 && wave) atomicAdd(&s_pass, wave);
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(&hdr[LB_PASSED], s_pass);
        __threadfence();
        if (atomicAdd(&hdr[LB_DONE], 1u) == gridDim.x - 1) {    // the last workgroup decides
            const uint32_t passed = atomicAdd(&hdr[LB_PASSED], 0u);
            const bool binned = 4ull * passed < nsamp;
            hdr[LB_FLAG] = binned ? 1u : 0u;
            atomicAdd(&stats[binned ? 0 : 1], 1ull);
        }
    }
}

// exclusive scan of one value per lane over the workgroup (T threads); `all` = the total. Two barriers.
template <int T>
__device__ __forceinline__ uint32_t lb_scan_excl(uint32_t mine, uint32_t* wsum, uint32_t& all) {
    const int t = threadIdx.x;
    uint32_t s = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(s, d);
        if ((t & 63) >= d) s += y;
    }
    if ((t & 63) == 63) wsum[t >> 6] = s;
    __syncthreads();
    uint32_t off = 0;
    all = 0;
#pragma unroll
    for (int w = 0; w < T / 64; ++w) {
        const uint32_t x = wsum[w];
        if (w < (t >> 6)) off += x;
        all += x;
    }
    __syncthreads();
    return off + s - mine;
}

// where entry number `r` of slice `bin` in this tile goes: the chunk the workgroup was filling (fill f), then the fresh chunks from nb
__device__ __forceinline__ void lb_place(uint32_t f, uint32_t cur, uint32_t nb, uint32_t r, uint32_t& chunk, uint32_t& o) {
    const uint32_t pos = f + r;
    if (pos < (uint32_t)LB_CH) { chunk = cur; o = pos; }
    else { chunk = nb + (pos - LB_CH) / LB_CH; o = (pos - LB_CH) % LB_CH; }
}

// Pass A fetches a query's dwords LB_AHEAD queries before it encodes them, so that a wave has loads in flight while it computes.
// The queries are addressed from q rounded down to a dword (qa = q - q mod 4) with a 32-bit byte offset (23 * (2^27 + a grid's
// tiles) + 3 < 2^32): one register per address. Tiles and a lane's stride inside a tile (LB_TB queries) are multiples of four
// queries, so every query of a lane starts at the same offset `o` inside its dword, whatever the tile.
// The fetch has no branch in it (a load under `if (i < n)`, or a conditional seventh load as in load23, makes hipcc wait for the
// loads right behind them) and reads no address that load23 does not read for a query of this batch: the offset is clamped to that
// of the batch's last query (n >= 1), which is 23 * 4 k bytes away and so has the lane's `o` too; dwords 0..5 of the window are
// load23's, and the seventh load is dword 6 only where load23 reads it (o >= 2); elsewhere it is dword 5 again, whose value
// lb_words never lets through: for o < 2 the funnel shift puts at most its low byte into the word's 24th byte, which is masked off.
static constexpr int LB_AHEAD = 1;
static_assert(LB_AHEAD >= 1 && LB_QPL % LB_AHEAD == 0, "a query's slot in the ring of fetched queries is the same in every tile");
static_assert(LB_TB % 4 == 0, "one offset inside the dword per lane");
struct LbRaw { uint32_t d[7]; };
// b = the query's first byte counted from qa (clamped by the caller), o = b % 4
__device__ __forceinline__ LbRaw lb_fetch(const uint8_t* __restrict__ qa, uint32_t b, uint32_t o) {
    const uint8_t* const a = qa + (b - o);
    LbRaw r;
#pragma unroll
    for (int k = 0; k < 6; ++k) r.d[k] = *(const uint32_t*)(a + 4 * k);
    r.d[6] = *(const uint32_t*)(qa + (b - o + (o >= 2 ? 24u : 20u)));
    return r;
}
// load23's words from the fetched dwords
__device__ __forceinline__ void lb_words(const LbRaw& r, uint32_t o, uint64_t& w0, uint64_t& w1, uint64_t& w2) {
    uint32_t sh = o * 8;
    asm("" : "+v"(sh));                                          // one register for the six shifts (hipcc otherwise keeps a copy of it per shift, for all of the kernel)
    const uint32_t e0 = __funnelshift_r(r.d[0], r.d[1], sh), e1 = __funnelshift_r(r.d[1], r.d[2], sh);
    const uint32_t e2 = __funnelshift_r(r.d[2], r.d[3], sh), e3 = __funnelshift_r(r.d[3], r.d[4], sh);
    const uint32_t e4 = __funnelshift_r(r.d[4], r.d[5], sh), e5 = __funnelshift_r(r.d[5], r.d[6], sh) & 0x00FFFFFFu;
    w0 = e0 | ((uint64_t)e1 << 32);
    w1 = e2 | ((uint64_t)e3 << 32);
    w2 = e4 | ((uint64_t)e5 << 32);
}

__global__ void __launch_bounds__(LB_TB, 3 * LB_TB / 256) k_lb_bin(uint32_t nbloom, const uint8_t* __restrict__ q, uint32_t n, LbGeom g, LbWs w, uint32_t* __restrict__ out) {
    if (!w.hdr[LB_FLAG]) return;
    __shared__ uint64_t sorted[LB_TILE];
    extern __shared__ __attribute__((aligned(16))) uint64_t carry[];   // [nbins][LB_LINE]: the records of a slice that do not fill a line yet
    // per slice (entry nbins = the queries that go straight onto the survivor list): tile count, its exclusive scan (entry nbins + 1 =
    // the tile's queries), the chunk being filled and its fill (a multiple of LB_LINE before the last tile), the first fresh chunk of
    // this tile, the records carried
    __shared__ uint32_t hist[LB_MAXBINS + 1], loc_off[LB_MAXBINS + 2], cur_chunk[LB_MAXBINS], cur_fill[LB_MAXBINS], fresh[LB_MAXBINS], carry_n[LB_MAXBINS];
    __shared__ uint32_t wsum[LB_TB / 64];
    const uint32_t t = threadIdx.x, NB = g.nbins;
    uint32_t* const cursor = w.hdr + LB_CURSOR;
    if (t <= NB) hist[t] = 0;
    if (t < NB) { cur_chunk[t] = LB_NONE; cur_fill[t] = LB_CH; fresh[t] = 0; carry_n[t] = 0; }
    __syncthreads();
    const uint32_t ntiles = (n + LB_TILE - 1) / LB_TILE;
    const uint32_t qo = (uint32_t)((uintptr_t)q & 3);
    const uint8_t* const qa = q - qo;
    // what a fetch beyond the batch is clamped to: the last query that is one of this lane's modulo 4 (it starts at the lane's offset
    // inside its dword, and every query of the lane beyond it is beyond the batch); a lane that has no query at all (t >= n) fetches the
    // batch's last query every time, and takes its offset
    const uint32_t i_last = t < n ? n - 1 - ((n - 1 - t) & 3u) : n - 1;
    const uint32_t b_last = qo + 23u * i_last, o = b_last & 3u;
    LbRaw ahead[LB_AHEAD];                                       // the lane's next LB_AHEAD queries
#pragma unroll
    for (int j = 0; j < LB_AHEAD; ++j) ahead[j] = lb_fetch(qa, min(qo + 23u * (blockIdx.x * LB_TILE + j * LB_TB + t), b_last), o);
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t base = tile * LB_TILE, in_tile = min((uint32_t)LB_TILE, n - base);
        // a record's high dword; its low dword is the query index, which the lane knows, and LB_LO_BITS bits of the word field, kept in meta
        // (eight registers fewer than whole records: with the fetched queries beside them the kernel would not fit 80 VGPRs without scratch)
        uint32_t rec_hi[LB_QPL];
        uint32_t meta[LB_QPL];                                   // slice | low bits of the word << LB_META_LO | rank inside the tile's slice << 16
#pragma unroll
        for (int j = 0; j < LB_QPL; ++j) {
            const uint32_t i = base + j * LB_TB + t;
            // this query's dwords were fetched LB_AHEAD queries ago; fetch those of the lane's query LB_AHEAD further on (in this tile, or
            // at the start of the workgroup's next one) before this one is encoded
            const LbRaw cur = ahead[j % LB_AHEAD];
            const uint32_t i_next = j + LB_AHEAD < LB_QPL ? i + LB_AHEAD * LB_TB : i + LB_AHEAD * LB_TB + (gridDim.x - 1) * LB_TILE;
            ahead[j % LB_AHEAD] = lb_fetch(qa, min(qo + 23u * i_next, b_last), o);
            meta[j] = LB_NONE;
            rec_hi[j] = 0;
            if (i < n) {
                uint64_t w0, w1, w2;
                uint32_t hw, hb;
                lb_words(cur, o, w0, w1, w2);
                uint32_t bin = NB;
                uint64_t r = i;
                if (lb_hash(w0, w1, w2, hw, hb)) {
                    const uint32_t word = bloom_word(hw, nbloom);
                    uint32_t wi;
                    lb_slice(word, g, bin, wi);
                    r |= ((uint64_t)wi << LB_IDX_BITS) | ((uint64_t)(hb & ((1u << LB_MASK_BITS) - 1)) << (LB_IDX_BITS + LB_WORD_BITS));
                }
                meta[j] = bin | (((uint32_t)r >> LB_IDX_BITS) << LB_META_LO) | (atomicAdd(&hist[bin], 1u) << 16);
                rec_hi[j] = (uint32_t)(r >> 32);
            }
        }
        // out[i] = 0 for the tile's queries, behind the query loop: a store counts in vmcnt like a load, so one store per query would
        // stand in the chain the next query's loads are waited for through. out + base is 4-byte aligned only: up to three single
        // dwords in front of and behind the 16-byte stores.
        {
            uint32_t* const o0 = out + base;
            const uint32_t head = min(in_tile, (0u - (uint32_t)((uintptr_t)o0 >> 2)) & 3u);
            const uint32_t nvec = (in_tile - head) / 4, tail = in_tile - head - 4 * nvec;
            uint4* const ov = (uint4*)(o0 + head);
#pragma unroll
            for (int k = 0; k < LB_TILE / 4 / LB_TB; ++k)
                if (k * LB_TB + t < nvec) ov[k * LB_TB + t] = make_uint4(0u, 0u, 0u, 0u);
            if (t < head) o0[t] = 0;
            if (t < tail) o0[head + 4 * nvec + t] = 0;
        }
        __syncthreads();
        // the workgroup's last tile writes everything; before it only whole lines leave, and the rest of a slice's run stays in `carry`
        const bool last = tile + gridDim.x >= ntiles;
        const uint32_t a = t <= NB ? hist[t] : 0u;
        if (t <= NB) hist[t] = 0;                                // the next tile's counting starts behind four more barriers
        uint32_t all;
        const uint32_t excl = lb_scan_excl<LB_TB>(a, wsum, all);
        if (t <= NB) loc_off[t] = excl;
        if (t == 0) loc_off[NB + 1] = all;
        if (t < NB) {
            const uint32_t tot = carry_n[t] + a, full = last ? tot : tot & ~(uint32_t)(LB_LINE - 1);
            if (cur_fill[t] + full > (uint32_t)LB_CH) fresh[t] = atomicAdd(&cursor[t], (cur_fill[t] + full - 1) / LB_CH);
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < LB_QPL; ++j) {
            if (meta[j] != LB_NONE) {
                const uint32_t bin = meta[j] & ((1u << LB_META_LO) - 1), p = loc_off[bin] + (meta[j] >> 16);
                const uint32_t lo = (base + j * LB_TB + t) | (((meta[j] >> LB_META_LO) & ((1u << LB_LO_BITS) - 1)) << LB_IDX_BITS);
                sorted[p] = lo | ((uint64_t)rec_hi[j] << 32);
            }
        }
        __syncthreads();
        // flush: wave v takes slices v, v + LB_TB / 64, ... A slice's run is its carry followed by its records of this tile (contiguous
        // in `sorted`); it lands contiguously behind the slice's fill, which is a multiple of LB_LINE, so every store instruction
        // writes whole 128-byte lines (a chunk is 2 KiB, a region 256-byte aligned). Only this wave touches the slice's carry, chunk and
        // fill here, and thread `bin` reads them again behind the next tile's first barrier: no barrier at the end of a tile.
        const uint32_t lane = t & 63u;
        for (uint32_t b = __builtin_amdgcn_readfirstlane(t >> 6); b <= NB; b += LB_TB / 64) {
            const uint32_t off = loc_off[b], cnt_b = loc_off[b + 1] - off;
            if (b == NB) {                                       // other bytes (rare): straight onto the survivor list
                if (cnt_b) {
                    uint32_t s0 = 0;
                    if (lane == 0) s0 = atomicAdd(&w.hdr[LB_NSURV], cnt_b);
                    s0 = __shfl(s0, 0);
                    for (uint32_t p = lane; p < cnt_b; p += 64) w.list[s0 + p] = (uint32_t)sorted[off + p] & ((1u << LB_IDX_BITS) - 1);
                }
                break;
            }
            const uint32_t c = carry_n[b], tot = c + cnt_b, full = last ? tot : tot & ~(uint32_t)(LB_LINE - 1);
            const uint32_t f = cur_fill[b], cur = cur_chunk[b], nb = fresh[b];
            uint64_t* const cy = carry + b * LB_LINE;
            for (uint32_t p0 = 0; p0 < full; p0 += 64) {
                const uint32_t p = p0 + lane;
                bool ov = false;
                uint64_t r = 0;
                if (p < full) {
                    r = p < c ? cy[p] : sorted[off + (p - c)];
                    uint32_t chunk, o;
                    lb_place(f, cur, nb, p, chunk, o);
                    if (chunk < g.cap) w.rec[((uint64_t)b * g.cap + chunk) * LB_CH + o] = r;
                    else ov = true;
                }
                const uint64_t m = __ballot(ov);
                if (m) {                                         // rare: the slice's region is full -> survivor list
                    uint32_t s0 = 0;
                    if (lane == 0) {
                        s0 = atomicAdd(&w.hdr[LB_NSURV], (uint32_t)__popcll(m));
                        atomicAdd(&w.stats[2], (unsigned long long)__popcll(m));
                    }
                    s0 = __shfl(s0, 0);
                    if (ov) w.list[s0 + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = (uint32_t)r & ((1u << LB_IDX_BITS) - 1);
                }
            }
            // what is left becomes the carry. full == 0: the old carry stays and the tile's records follow it; otherwise all of it comes
            // from `sorted` (p >= full >= LB_LINE > c), and the wave has read the old carry above
            if (lane < tot - full) {
                const uint32_t p = full + lane;
                if (p >= c) cy[p - full] = sorted[off + (p - c)];
            }
            // advance the slice's chunk; a chunk's count is written when the workgroup leaves it
            uint32_t n_chunk = cur, n_fill = f + full;
            uint32_t* const cnt = w.cnt + (uint64_t)b * g.cap;
            if (n_fill > (uint32_t)LB_CH) {
                const uint32_t k = (n_fill - 1) / LB_CH;
                if (lane == 0 && cur < g.cap) cnt[cur] = LB_CH;
                for (uint32_t u = lane; u + 1 < k; u += 64) if (nb + u < g.cap) cnt[nb + u] = LB_CH;
                n_chunk = nb + k - 1;
                n_fill -= k * LB_CH;
            }
            if (lane == 0) {
                carry_n[b] = tot - full;
                cur_chunk[b] = n_chunk;
                cur_fill[b] = n_fill;
                if (last && n_chunk < g.cap) cnt[n_chunk] = n_fill;
            }
        }
    }
}

__global__ void __launch_bounds__(LB_FB) k_lb_filter(const uint64_t* __restrict__ bloom, uint32_t nbloom, LbGeom g, LbWs w) {
    if (!w.hdr[LB_FLAG]) return;
    __shared__ uint32_t pre[LB_MAXBINS + 1];                    // chunks in the slices before this one
    __shared__ uint32_t surv[LB_SURV];
    __shared__ uint32_t wsum[LB_FB / 64];
    __shared__ uint32_t s_n, s_base, s_ticket;
    const uint32_t t = threadIdx.x, NB = g.nbins;
    const uint32_t mine = t < NB ? min(w.hdr[LB_CURSOR + t], g.cap) : 0u;
    uint32_t total;
    const uint32_t excl = lb_scan_excl<LB_FB>(mine, wsum, total);
    if (t < (uint32_t)LB_MAXBINS) pre[t] = excl;
    if (t == 0) { pre[LB_MAXBINS] = total; s_n = 0; }
    __syncthreads();
    auto flush = [&]() {                                         // every lane of the workgroup calls it
        if (t == 0) s_base = atomicAdd(&w.hdr[LB_NSURV], s_n);
        __syncthreads();
        for (uint32_t i = t; i < s_n; i += LB_FB) w.list[s_base + i] = surv[i];
        __syncthreads();
        if (t == 0) s_n = 0;
        __syncthreads();
    };
    // The chunks are handed out in slice order, a ticket of LB_CPT at a time: what the grid has in flight is then one contiguous
    // window of gridDim.x * LB_CPT chunks (~1 % of the records, so ~1 % of the filter: ~1 MB), however unevenly the workgroups
    // advance. With a static grid stride the window drifted apart and 60 % of the filter reads missed L2; a workgroup that holds a
    // second ticket ahead of the one it filters widens the window too, and lost more than the overlap gained
    // (profiles/lookup_binned/README.md). Ticket k of counter x = chunks (k * nt + x) * LB_CPT onwards; lane t takes record t % LB_CH
    // of chunk u * LB_CPG + t / LB_CH of the ticket, u < LB_U. A lane's chunk numbers only ever increase, and so does `bin`.
    const uint32_t nt = min(gridDim.x, (uint32_t)LB_TICKETS);   // counters in use: each of them has a workgroup that pulls on it
    const uint32_t lane_x = blockIdx.x % nt;
    uint32_t* const ticket = w.hdr + LB_TICKET + 32 * lane_x;
    uint32_t bin = 0;
    for (;;) {
        if (t == 0) s_ticket = atomicAdd(ticket, 1u);
        __syncthreads();
        const uint64_t it64 = ((uint64_t)s_ticket * nt + lane_x) * LB_CPT;
        if (it64 >= total) break;
        const uint32_t it = (uint32_t)it64;
        uint64_t r[LB_U], wd[LB_U];
        uint32_t cn[LB_U], wbase[LB_U];
#pragma unroll
        for (int u = 0; u < LB_U; ++u) {
            const uint32_t item = it + u * LB_CPG + t / LB_CH;
            cn[u] = 0; r[u] = 0; wbase[u] = 0;
            if (item < total) {
                while (bin + 1 < NB && item >= pre[bin + 1]) ++bin;
                const uint64_t ch = (uint64_t)bin * g.cap + (item - pre[bin]);
                cn[u] = w.cnt[ch];
                r[u] = __builtin_nontemporal_load(&w.rec[ch * LB_CH + t % LB_CH]);   // streamed once: keep the slice in L2
                wbase[u] = bin * g.wps;
            }
        }
#pragma unroll
        for (int u = 0; u < LB_U; ++u) {
            const uint32_t word = wbase[u] + ((uint32_t)(r[u] >> LB_IDX_BITS) & ((1u << LB_WORD_BITS) - 1));
            wd[u] = (t % LB_CH < cn[u] && word < nbloom) ? bloom[word] : 0ull;
        }
#pragma unroll
        for (int u = 0; u < LB_U; ++u) {
            const uint64_t mk = bloom_mask((uint32_t)(r[u] >> (LB_IDX_BITS + LB_WORD_BITS)));   // all four positions: the low LB_MASK_BITS bits
            const bool pass = t % LB_CH < cn[u] && (wd[u] & mk) == mk;
            const uint64_t m = __ballot(pass);
            if (m) {
                uint32_t r0 = 0;
                if ((t & 63u) == 0) r0 = atomicAdd(&s_n, (uint32_t)__popcll(m));
                r0 = __shfl(r0, 0);
                if (pass) surv[r0 + (uint32_t)__popcll(m & ((1ull << (t & 63u)) - 1))] = (uint32_t)r[u] & ((1u << LB_IDX_BITS) - 1);
            }
        }
        __syncthreads();
        if (s_n > (uint32_t)LB_FLUSH_AT) flush();
    }
    if (s_n) flush();
}

// the coarse image (bloom_fold, aix_device.hpp) of every filter word, slice by slice: slice s starts at byte s * stride (stride = the
// slice width rounded up to 16 bytes, so that a slice is loaded with aligned 16-byte loads); bytes behind a slice's words are zero
__global__ void __launch_bounds__(256) k_lb_fold(const uint64_t* __restrict__ bloom, uint32_t nbloom, uint32_t wps, uint32_t stride, uint32_t nbins,
                                                 uint8_t* __restrict__ coarse) {
    const uint32_t total = nbins * stride;                      // <= LB_MAXBINS * LBC_MAX_WPS = 2^25
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const uint32_t s = i / stride, wi = i - s * stride;
        const uint64_t word = (uint64_t)s * wps + wi;
        coarse[i] = (wi < wps && word < nbloom) ? (uint8_t)bloom_fold(bloom[word]) : (uint8_t)0;
    }
}

// Pass B with the coarse image of the slice in LDS. A record first tests bit hb & 7 of its word's image byte; only where it is set
// (about 4 records in 10 of an absent-heavy batch at 16 filter bits per key) is the filter word read from L2 and the full mask
// tested, so the survivors are those of k_lb_filter. One workgroup of LBC_FB threads per CU holds one slice's image (<= 128 KiB of
// dynamic LDS). Ticket counter x of the nt in use owns the slices s with s % nt == x and hands their chunks out in slice order, a
// ticket of LBC_CPT chunks at a time; a ticket does not span slices (a slice's chunks are rounded up to whole tickets), and a
// workgroup whose ticket lies in another slice than the one it holds loads that slice's image first. A workgroup sends for the
// records of its next ticket as soon as the current one's survivors are stored, so that they travel across the barriers and the
// next pull; under ownership a ticket held ahead widens no window that matters.
__global__ void __launch_bounds__(LBC_FB) k_lb_filter_coarse(const uint64_t* __restrict__ bloom, uint32_t nbloom, const uint8_t* __restrict__ coarse,
                                                             uint32_t stride, LbGeom g, LbWs w) {
    if (!w.hdr[LB_FLAG]) return;
    extern __shared__ __attribute__((aligned(16))) uint8_t image[];   // [stride]: the coarse image of slice `held`
    __shared__ uint32_t tpre[LB_MAXBINS + 1];                   // this counter's tickets in the slices before this one
    __shared__ uint32_t nch[LB_MAXBINS];                        // chunks of the slice
    __shared__ uint32_t surv[LBC_SURV];
    __shared__ uint32_t wsum[LBC_FB / 64];
    __shared__ uint32_t s_n, s_base, s_ticket, s_cnt[2];
    const uint32_t t = threadIdx.x, NB = g.nbins;
    const uint32_t nt = min(gridDim.x, (uint32_t)LB_TICKETS);   // counters in use: each of them has a workgroup that pulls on it
    const uint32_t lane_x = blockIdx.x % nt;
    uint32_t* const ticket = w.hdr + LB_TICKET + 32 * lane_x;
    const uint32_t mine = t < NB ? min(w.hdr[LB_CURSOR + t], g.cap) : 0u;
    uint32_t total;                                             // tickets of this counter
    const uint32_t excl = lb_scan_excl<LBC_FB>(t % nt == lane_x ? (mine + LBC_CPT - 1) / LBC_CPT : 0u, wsum, total);
    if (t < (uint32_t)LB_MAXBINS) { tpre[t] = excl; nch[t] = mine; }
    if (t == 0) { tpre[LB_MAXBINS] = total; s_n = 0; s_cnt[0] = 0; s_cnt[1] = 0; }
    __syncthreads();
    auto flush = [&]() {                                         // every lane of the workgroup calls it
        if (t == 0) s_base = atomicAdd(&w.hdr[LB_NSURV], s_n);
        __syncthreads();
        for (uint32_t i = t; i < s_n; i += LBC_FB) w.list[s_base + i] = surv[i];
        __syncthreads();
        if (t == 0) s_n = 0;
        __syncthreads();
    };
    // ticket k of this counter -> its slice (`bin`, which only ever increases) and its first chunk there; false = past the end.
    // tpre[s] = total for every s >= NB, so the walk stops at a slice that has tickets of this counter.
    uint32_t bin = 0;
    auto locate = [&](uint32_t k, uint32_t& c0) -> bool {
        if (k >= total) return false;
        while (k >= tpre[bin + 1]) ++bin;
        c0 = (k - tpre[bin]) * LBC_CPT;
        return true;
    };
    // lane t takes record t % LB_CH of chunk c0 + u * LBC_CPG + t / LB_CH of slice b, u < LBC_U. No branch around the loads (behind
    // one, hipcc waits for every load in flight where it needs the oldest, and the records fetched ahead would be waited for with
    // the filter words): a chunk behind the slice's last is clamped to the last and its count set to zero, and so is every chunk
    // of a ticket that is not `live`. The slice has a chunk (the caller has located a ticket in it).
    auto fetch = [&](uint32_t b, uint32_t c0, bool live, uint64_t (&r)[LBC_U], uint32_t (&cn)[LBC_U]) {
        const uint32_t last = nch[b] - 1;
#pragma unroll
        for (int u = 0; u < LBC_U; ++u) {
            const uint32_t ci = c0 + u * LBC_CPG + t / LB_CH;
            const uint64_t ch = (uint64_t)b * g.cap + min(ci, last);
            const uint32_t c = w.cnt[ch];
            r[u] = __builtin_nontemporal_load(&w.rec[ch * LB_CH + t % LB_CH]);       // streamed once: keep the slice in L2
            cn[u] = live && ci <= last ? c : 0u;
        }
    };
    uint64_t rn[LBC_U];                                          // the records of the next ticket, of slice bn
    uint32_t cnn[LBC_U], bn, c0 = 0;
    if (t == 0) s_ticket = atomicAdd(ticket, 1u);
    __syncthreads();
    bool more = locate(s_ticket, c0);
    bn = bin;
    if (more) fetch(bn, c0, true, rn, cnn);
    __syncthreads();                                            // s_ticket is written again below
    uint32_t held = LB_NONE, n_tested = 0, n_on = 0;            // the wave's records tested against the image / sent on to the filter word
    while (more) {
        uint64_t r[LBC_U], wd[LBC_U];
        uint32_t cn[LBC_U];
        bool on[LBC_U];
        const uint32_t b = bn;
#pragma unroll
        for (int u = 0; u < LBC_U; ++u) { r[u] = rn[u]; cn[u] = cnn[u]; }
        if (t == 0) s_ticket = atomicAdd(ticket, 1u);
        if (b != held) {                                         // nobody reads the image between the barrier that ended the last ticket and the one below
            const uint4* const src = (const uint4*)(coarse + (uint64_t)b * stride);
            for (uint32_t i = t; i < stride / 16; i += LBC_FB) ((uint4*)image)[i] = src[i];
            held = b;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < LBC_U; ++u) {
            const uint32_t wi = (uint32_t)(r[u] >> LB_IDX_BITS) & ((1u << LB_WORD_BITS) - 1), word = b * g.wps + wi;
            const bool valid = t % LB_CH < cn[u] && wi < g.wps && word < nbloom;
            on[u] = valid && bloom_fold_test(image[valid ? wi : 0u], (uint32_t)(r[u] >> (LB_IDX_BITS + LB_WORD_BITS)));
            wd[u] = bloom[on[u] ? word : b * g.wps];             // the others read the slice's first word together: one request per wave
            n_tested += (uint32_t)__popcll(__ballot(valid));
            n_on += (uint32_t)__popcll(__ballot(on[u]));
        }
#pragma unroll
        for (int u = 0; u < LBC_U; ++u) {
            const uint64_t mk = bloom_mask((uint32_t)(r[u] >> (LB_IDX_BITS + LB_WORD_BITS)));   // all four positions: the low LB_MASK_BITS bits
            const bool pass = on[u] && (wd[u] & mk) == mk;
            const uint64_t m = __ballot(pass);
            if (m) {
                uint32_t r0 = 0;
                if ((t & 63u) == 0) r0 = atomicAdd(&s_n, (uint32_t)__popcll(m));
                r0 = __shfl(r0, 0);
                if (pass) surv[r0 + (uint32_t)__popcll(m & ((1ull << (t & 63u)) - 1))] = (uint32_t)r[u] & ((1u << LB_IDX_BITS) - 1);
            }
        }
        // the next ticket's records go out behind this ticket's survivors and come back across the barriers, a flush and the next
        // ticket pull. Sent out behind the filter reads instead, before the mask test, they cost 0.05 ms
        // (profiles/lookup_binned/README.md).
        more = locate(s_ticket, c0);
        bn = bin;                                                // past the end: still this ticket's slice
        fetch(bn, more ? c0 : 0u, more, rn, cnn);
        __syncthreads();
        if (s_n > (uint32_t)LBC_FLUSH_AT) flush();
    }
    if ((t & 63u) == 0 && n_tested) { atomicAdd(&s_cnt[0], n_tested); atomicAdd(&s_cnt[1], n_on); }
    if (s_n) flush();                                           // the same for every lane: nobody appends behind the loop's last barrier
    __syncthreads();
    if (t == 0 && s_cnt[0]) {
        atomicAdd(&w.stats[4], (unsigned long long)s_cnt[0]);
        atomicAdd(&w.stats[5], (unsigned long long)s_cnt[1]);
    }
}

}  // namespace aix

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
static uint64_t align_up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }

// AIX_TAKEN: the batch is enqueued (binned kernels and, in auto mode, the gated direct kernel); AIX_NOT_TAKEN: the caller runs the
// direct path; anything else is an error status
int lookup23_binned(aix_index* h, const IndexDev& d, const uint8_t* q, uint64_t N, uint32_t* out, hipStream_t s) {
    const long sw = env_int("AIX_LOOKUP_BINNED", 0, 2, 1);
    if (sw == 0 || d.k != 23 || !d.canonical_only || !d.bk || !d.bloom || d.nbloom == 0) return AIX_LB_NOT_TAKEN;
    if (sw == 1 && N < env_u64("AIX_LOOKUP_BINNED_MIN", 0, ~0ull, AIX_LB_DEFAULT_MIN)) return AIX_LB_NOT_TAKEN;
    const uint64_t slice_bytes = env_u64("AIX_LOOKUP_SLICE_BYTES", 8, 2ull << 20, 1ull << 20);
    LbGeom g;
    g.wps = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(slice_bytes / 8, 1), d.nbloom);
    g.nbins = (d.nbloom + g.wps - 1) / g.wps;
    if (g.nbins > (uint32_t)LB_MAXBINS) return AIX_LB_NOT_TAKEN;   // a filter above ~500 MB: direct
    g.inv = g.wps > 1 ? (uint32_t)((1ull << 32) / g.wps) : 0xFFFFFFFFu;
    g.shift = (g.wps & (g.wps - 1)) == 0 ? (uint32_t)__builtin_ctz(g.wps) : LB_NO_SHIFT;
    const uint64_t piece = std::min<uint64_t>(std::min<uint64_t>(N, 1ull << LB_IDX_BITS), env_u64("AIX_LOOKUP_PIECE", 1, 1ull << LB_IDX_BITS, 1ull << LB_IDX_BITS));
    const uint64_t test_grid_a = env_u64("AIX_LOOKUP_TEST_GRID_A", 1, LB_GRID_A, LB_GRID_A);   // fewer workgroups: many tiles each on a small batch
    const unsigned grid_a = (unsigned)std::min<uint64_t>((piece + LB_TILE - 1) / LB_TILE, test_grid_a);
    const uint32_t carry_bytes = g.nbins * LB_LINE * 8;
    // a slice region: its share of a uniformly hashed piece plus a quarter, plus the chunk every pass-A workgroup leaves partly filled
    const uint64_t test_cap = env_u64("AIX_LOOKUP_TEST_BIN_CAP", 0, ~0ull, ~0ull);
    uint64_t cap = test_cap != ~0ull ? (test_cap + LB_CH - 1) / LB_CH : (piece + piece / 4) / g.nbins / LB_CH + 2 + grid_a;
    cap = std::min<uint64_t>(cap, (piece + LB_CH - 1) / LB_CH + grid_a);
    g.cap = (uint32_t)cap;
    const uint64_t off_list = LB_HDR_BYTES, off_cnt = align_up(off_list + 4 * piece, 256), off_rec = align_up(off_cnt + 4ull * g.nbins * cap, 256);
    const uint64_t need = off_rec + 8ull * g.nbins * cap * LB_CH;
    // pass B tests the coarse image of a slice in LDS first (k_lb_filter_coarse) where a slice's image fits there
    const uint64_t coarse_max = std::min<uint64_t>(env_u64("AIX_LOOKUP_TEST_COARSE_MAX", 0, LBC_MAX_WPS, LBC_MAX_WPS), LBC_MAX_WPS);
    bool coarse = env_int("AIX_LOOKUP_COARSE", 0, 1, 1) == 1 && g.wps <= coarse_max;
    const uint32_t cstride = (uint32_t)align_up(g.wps, 16);
    const uint64_t need_coarse = (uint64_t)g.nbins * cstride;

    BinnedState& lb = h->lb;
    std::lock_guard<std::mutex> lk(lb.mutex);                  // orders the enqueueing; the event orders the streams
    if (lb.done.create() != hipSuccess) { (void)hipGetLastError(); return AIX_LB_NOT_TAKEN; }
    if (!lb.stats) {
        if (lb.stats.alloc(8 * LB_NSTATS) != hipSuccess) { (void)hipGetLastError(); return AIX_LB_NOT_TAKEN; }
        HIPCHK(hipMemset(lb.stats.p, 0, 8 * LB_NSTATS));
    }
    // both blocks grow only, behind the kernels of earlier calls, which may still be using the old block
    hipError_t waited = hipSuccess;                            // a failed wait is an error; a block that cannot be had is not
    auto wait = [&] { return waited = lb.used ? hipEventSynchronize(lb.done) : hipSuccess; };
    if (coarse && need_coarse > lb.coarse.bytes) {
        const hipError_t e = lb.coarse.ensure(need_coarse, 0, wait);
        HIPCHK(waited);
        lb.coarse_src = nullptr;
        if (e != hipSuccess) { (void)hipGetLastError(); coarse = false; }   // no room: pass B without the image
    }
    const hipError_t e_ws = lb.ws.ensure(need, 0, wait);
    HIPCHK(waited);
    if (e_ws != hipSuccess) { (void)hipGetLastError(); return AIX_LB_NOT_TAKEN; }
    if (lb.used && lb.stream != s) HIPCHK(hipStreamWaitEvent(s, lb.done, 0));
    lb.used = true;
    lb.stream = s;
    RecordOnExit record_on_exit{lb.done, s};                    // also behind a failed launch: what was enqueued before it uses the workspace

    // pass A's static LDS is 38 KiB: with the carry of more than 128 slices it may pass 64 KiB (two workgroups per CU then)
    if (carry_bytes > (16u << 10)) HIPCHK(hipFuncSetAttribute((const void*)k_lb_bin, hipFuncAttributeMaxDynamicSharedMemorySize, (int)carry_bytes));
    uint8_t* const base = lb.ws.as<uint8_t>();
    LbWs w;
    w.hdr = (uint32_t*)base;
    w.list = (uint32_t*)(base + off_list);
    w.cnt = (uint32_t*)(base + off_cnt);
    w.rec = (uint64_t*)(base + off_rec);
    w.stats = lb.stats.as<unsigned long long>();
    const uint64_t test_grid_b = env_u64("AIX_LOOKUP_TEST_GRID_B", 1, LB_GRID_B, LB_GRID_B);   // fewer workgroups: many tickets each on a small batch
    const unsigned grid_b = (unsigned)std::min<uint64_t>(std::max<uint64_t>(((uint64_t)g.nbins * cap + LB_CPT - 1) / LB_CPT, 1), test_grid_b);
    const unsigned grid_c = (unsigned)std::min<uint64_t>(std::max<uint64_t>((uint64_t)g.nbins * ((cap + LBC_CPT - 1) / LBC_CPT), 1), std::min<uint64_t>(test_grid_b, LBC_GRID));
    if (coarse) {
        // the image is folded once per filter and slice width, on the stream of the first call that needs it: a handle's filter does not
        // change while it is open (switching it off and on again, or moving it, leaves its words as they were)
        if (lb.coarse_src != d.bloom || lb.coarse_nbloom != d.nbloom || lb.coarse_wps != g.wps) {
            hipLaunchKernelGGL(k_lb_fold, dim3((unsigned)std::min<uint64_t>((need_coarse + 255) / 256, 4096)), dim3(256), 0, s, d.bloom, d.nbloom, g.wps, cstride,
                               g.nbins, lb.coarse.as<uint8_t>());
            HIPCHK(hipGetLastError());
            lb.coarse_src = d.bloom;
            lb.coarse_nbloom = d.nbloom;
            lb.coarse_wps = g.wps;
        }
        // 26 KiB of static LDS beside the image
        if (cstride > (16u << 10)) HIPCHK(hipFuncSetAttribute((const void*)k_lb_filter_coarse, hipFuncAttributeMaxDynamicSharedMemorySize, (int)cstride));
    }
    for (uint64_t lo = 0; lo < N; lo += piece) {
        const uint32_t m = (uint32_t)std::min<uint64_t>(piece, N - lo);
        const uint8_t* qp = q + 23 * lo;
        uint32_t* op = out + lo;
        HIPCHK(hipMemsetAsync(w.hdr, 0, LB_HDR_BYTES, s));
        const uint32_t nsamp = std::min<uint32_t>(m, LB_SAMPLES);
        hipLaunchKernelGGL(k_lb_gate, dim3(sw == 2 ? 1 : (nsamp + 255) / 256), dim3(256), 0, s, d.bloom, d.nbloom, qp, m, nsamp, sw == 2 ? 1 : 0, w.hdr,
                           w.stats);
        HIPCHK(hipGetLastError());
        if (sw != 2) HIPCHK(launch_lookup23_ascii(d, qp, m, MODE_TF, LookupOut{op, nullptr, nullptr, nullptr}, s, w.hdr + LB_FLAG));
        hipLaunchKernelGGL(k_lb_bin, dim3(std::min<unsigned>(grid_a, (m + LB_TILE - 1) / LB_TILE)), dim3(LB_TB), carry_bytes, s, d.nbloom, qp, m, g, w, op);
        HIPCHK(hipGetLastError());
        if (coarse) hipLaunchKernelGGL(k_lb_filter_coarse, dim3(grid_c), dim3(LBC_FB), cstride, s, d.bloom, d.nbloom, lb.coarse.as<const uint8_t>(), cstride, g, w);
        else hipLaunchKernelGGL(k_lb_filter, dim3(grid_b), dim3(LB_FB), 0, s, d.bloom, d.nbloom, g, w);
        HIPCHK(hipGetLastError());
        HIPCHK(launch_lookup23_list(d, qp, w.list, w.hdr + LB_NSURV, m, w.hdr + LB_FLAG, op, w.stats + 3, s));
    }
    return AIX_LB_TAKEN;
}

extern "C" int aix_lookup_binned_stats(aix_index_t* h, uint64_t out[4]) {
    if (!h || !out) return AIX_ERR_ARG;
    DevGuard g(h->device);
    std::lock_guard<std::mutex> lk(h->lb.mutex);
    for (int i = 0; i < 4; ++i) out[i] = 0;
    if (!h->lb.stats) return AIX_OK;
    if (h->lb.used) HIPCHK(hipEventSynchronize(h->lb.done));
    HIPCHK(hipMemcpy(out, h->lb.stats.p, 32, hipMemcpyDeviceToHost));
    return AIX_OK;
}

extern "C" int aix_lookup_binned_coarse_stats(aix_index_t* h, uint64_t out[2]) {
    if (!h || !out) return AIX_ERR_ARG;
    DevGuard g(h->device);
    std::lock_guard<std::mutex> lk(h->lb.mutex);
    out[0] = out[1] = 0;
    if (!h->lb.stats) return AIX_OK;
    if (h->lb.used) HIPCHK(hipEventSynchronize(h->lb.done));
    HIPCHK(hipMemcpy(out, h->lb.stats.as<uint64_t>() + 4, 16, hipMemcpyDeviceToHost));
    return AIX_OK;
}
