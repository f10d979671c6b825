// aix_debruijn.hip — De Bruijn neighbour queries and k-mer walks over a 23-mer index resident in HBM.
//   DEBRUJIN::print_next / print_prev   debrujin.cpp:30-75, 121-167   the four successors / predecessors of a 23-mer with their tf (struct CONT)
//   PHASH_MAP::get_freq(uint64_t)       hash.hpp:123-140             forward strand, then the reverse complement; the forward strand wins
//
// Layout: one lane per (k-mer, base). A wave holds 16 k-mers; the four lanes of a quad probe the four neighbours of their k-mer in ONE
// call of the wave-cooperative probe (aix_probe.hpp: verification table, side index, unfiled keys, MPHF fallback — the probe of
// k_lookup23_codes), and the CONT rule is a reduction inside the quad (DPP quad_perm broadcasts, no LDS). A walk is the same step in a loop
// bounded by max_steps: the state (current code, length, stop reason) stays in registers, a step of a walk costs four independent probes
// (eight in unitig mode: the join test looks back from the successor), and nothing but the chosen base and its tf is written per step.
// Walks differ in length: a wave leaves its loop when its last quad has stopped, a workgroup of 64 seeds is the unit the hardware
// schedules (no work counter, no atomics). Every index derived from S * max_steps is 64 bits wide. Integer only, no scratch.
#include <algorithm>
#include <string>

#include "aix_env.hpp"
#include "aix_hostkit.hpp"
#include "aix_probe.hpp"

namespace aix {

static constexpr int kDB = 256;                                   // four waves = 64 quads per workgroup
static constexpr uint64_t kMask46 = (1ULL << 46) - 1;

// The absence filter of a trip: 0 = FilterGauge (what the lookups do), 1 = always consulted, 2 = never. Wave-uniform.
struct DbFilter {
    int policy;
    FilterGauge fg;
    __device__ __forceinline__ bool on() const { return policy == 1 ? true : (policy == 2 ? false : fg.on); }
    __device__ __forceinline__ void seen(bool active, bool found) { if (policy == 0) fg.seen(active, found); }
};

// debrujin.cpp:34-37 (dir 0) and :125-128 (dir 1)
__device__ __forceinline__ uint64_t db_neigh(uint64_t u, int dir, uint32_t b) {
    return dir == 0 ? (((u << 2) | (uint64_t)b) & kMask46) : ((u >> 2) | ((uint64_t)b << 44));
}

template <int J>
__device__ __forceinline__ uint32_t quad_bcast(uint32_t v) {      // lane J of the quad to its four lanes (DPP quad_perm [J, J, J, J]); all lanes active
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, J * 0x55, 0xf, 0xf, false);
}

struct Cont {
    uint32_t mine;      // this lane's tf after the cutoff
    uint32_t n, sum, best_tf, best;
};
// debrujin.cpp:44-74 / :135-166 from the four tf of a quad: cutoff inclusive, u32 sum, the four overwriting ifs
__device__ __forceinline__ Cont db_cont(uint32_t t, uint32_t cutoff) {
    if (cutoff > 0 && t <= cutoff) t = 0;
    const uint32_t A = quad_bcast<0>(t), C = quad_bcast<1>(t), G = quad_bcast<2>(t), T = quad_bcast<3>(t);
    Cont c;
    c.mine = t;
    c.sum = A + C + G + T;
    c.n = (uint32_t)(A != 0) + (uint32_t)(C != 0) + (uint32_t)(G != 0) + (uint32_t)(T != 0);
    c.best = 3; c.best_tf = T;
    if (A >= C && A >= G && A >= T) { c.best = 0; c.best_tf = A; }
    if (C >= A && C >= G && C >= T) { c.best = 1; c.best_tf = C; }
    if (G >= C && G >= A && G >= T) { c.best = 2; c.best_tf = G; }
    if (T >= C && T >= G && T >= A) { c.best = 3; c.best_tf = T; }
    return c;
}

// the lane's k-mer as a 46-bit code: given, or the sanitised code of its 23 bytes (get_dna23_bitset, kmers.cpp:12-40)
__device__ __forceinline__ uint64_t db_code(const uint64_t* __restrict__ codes, const uint8_t* __restrict__ ascii, uint64_t i, bool in) {
    if (!in) return 0;
    if (codes) return codes[i] & kMask46;
    uint64_t w0, w1, w2;
    load23(ascii + 23 * i, w0, w1, w2);
    return encode23_words(w0, w1, w2).code;
}

// one 32-byte record per (k-mer, direction): tf[4], n, sum, best_tf, best_base; lane b of the quad writes words b and 4 + b
template <bool CANON>
__global__ void __launch_bounds__(kDB) k_db_neighbours(const IndexDev ix_, const uint64_t* __restrict__ codes, const uint8_t* __restrict__ ascii, uint64_t N,
                                                      int dirs, uint32_t cutoff, int policy, uint32_t* __restrict__ out) {
    const IndexDev& ix = ix_;
    const uint64_t NR = dirs == AIX_DIR_BOTH ? 2 * N : N;
    const uint32_t lane = threadIdx.x & 63u, b = lane & 3u;
    DbFilter fl{policy, {}};
    const uint64_t stride = (uint64_t)gridDim.x * 64;
    for (uint64_t base = (uint64_t)blockIdx.x * 64 + (threadIdx.x >> 6) * 16; base < NR; base += stride) {    // wave-uniform
        const uint64_t rec = base + (lane >> 2);
        const bool in = rec < NR;
        const uint64_t i = dirs == AIX_DIR_BOTH ? rec >> 1 : rec;
        const int d = dirs == AIX_DIR_BOTH ? (int)(rec & 1) : dirs;
        const uint64_t u = db_code(codes, ascii, i, in);
        bool found;
        const uint32_t t = freq23_wave<CANON>(ix, in, db_neigh(u, d, b), fl.on(), found);
        fl.seen(in, found);
        const Cont c = db_cont(t, cutoff);
        if (in) {
            out[rec * 8 + b] = c.mine;
            out[rec * 8 + 4 + b] = b == 0 ? c.n : (b == 1 ? c.sum : (b == 2 ? c.best_tf : c.best));
        }
    }
}

template <bool CANON, bool UNITIG>
__global__ void __launch_bounds__(kDB) k_db_walk(const IndexDev ix_, const uint64_t* __restrict__ codes, const uint8_t* __restrict__ ascii, uint64_t S, int dir,
                                                uint32_t L, uint32_t cutoff, int policy, uint8_t* __restrict__ out_bases, uint32_t* __restrict__ out_len,
                                                uint8_t* __restrict__ out_stop, uint32_t* __restrict__ out_tf, uint64_t* __restrict__ out_last) {
    const IndexDev& ix = ix_;
    const uint32_t lane = threadIdx.x & 63u, b = lane & 3u;
    DbFilter fl{policy, {}};
    const uint64_t stride = (uint64_t)gridDim.x * 64;
    for (uint64_t base = (uint64_t)blockIdx.x * 64 + (threadIdx.x >> 6) * 16; base < S; base += stride) {     // wave-uniform
        const uint64_t seed = base + (lane >> 2);
        const bool in = seed < S;
        const uint64_t u = db_code(codes, ascii, seed, in);
        const uint64_t ur = revcomp(u, 23), seedc = u <= ur ? u : ur;
        const uint64_t row = seed * (uint64_t)L;                 // 64 bits: S * L passes 2^32
        uint64_t cur = u;
        uint32_t len = 0, stop = AIX_STOP_MAX_STEPS;
        bool alive = in;
        for (uint32_t step = 0; step < L && __ballot(alive) != 0; ++step) {                                  // wave-uniform, bounded by max_steps
            bool found;
            const uint32_t t = freq23_wave<CANON>(ix, alive, db_neigh(cur, dir, b), fl.on(), found);
            fl.seen(alive, found);
            const Cont c = db_cont(t, cutoff);
            const uint64_t nxt = db_neigh(cur, dir, c.best);
            bool go = alive;
            if (go && c.n == 0) { stop = AIX_STOP_DEAD_END; go = false; }
            if (UNITIG) {
                if (go && c.n > 1) { stop = AIX_STOP_BRANCH; go = false; }
                bool found2;
                const uint32_t t2 = freq23_wave<CANON>(ix, go, db_neigh(nxt, 1 - dir, b), fl.on(), found2);
                fl.seen(go, found2);
                const Cont c2 = db_cont(t2, cutoff);
                if (go && c2.n > 1) { stop = AIX_STOP_JOIN; go = false; }
            }
            if (go) {
                const uint64_t nr = revcomp(nxt, 23);
                if ((nxt <= nr ? nxt : nr) == seedc) { stop = AIX_STOP_LOOP; go = false; }
            }
            if (go) {
                if (b == 0) {
                    out_bases[row + len] = (uint8_t)(AIX_LUT_ACGT >> (8 * c.best));
                    if (out_tf) out_tf[row + len] = c.best_tf;
                }
                ++len;
                cur = nxt;
            }
            alive = go;
        }
        if (in && b == 0) {
            out_len[seed] = len;
            out_stop[seed] = (uint8_t)stop;
            if (out_last) out_last[seed] = cur;
        }
    }
}

static inline unsigned db_grid(uint64_t quads, uint64_t cap) {
    uint64_t g = (quads + 63) / 64;
    if (g > cap) g = cap;
    if (g == 0) g = 1;
    return (unsigned)g;
}

// AIX_DBJ_FILTER (A/B switch): the absence-filter policy of these kernels. Not set: neighbours consult the filter always (8 N probes ran at
// 1.01 .. 1.03 of k_lookup23_codes's rate on the same codes), walks never (10^6 seeds x 256 steps, always / gauge / never: 26.4 / 27.0 / 26.8 and
// 49.1 / 46.6 / 46.6 ms on a clean genome, 24.4 / 22.6 / 22.5 and 11.7 / 12.2 / 12.1 ms on reads with errors)
static inline int db_policy(int dflt) { return (int)env_int("AIX_DBJ_FILTER", 0, 2, dflt); }

hipError_t launch_db_neighbours(const IndexDev& ix, const uint64_t* codes, const uint8_t* ascii, uint64_t N, int dirs, uint32_t cutoff, uint32_t* out, hipStream_t s) {
    if (N == 0) return hipSuccess;
    const dim3 g(db_grid(dirs == AIX_DIR_BOTH ? 2 * N : N, 65536)), blk(kDB);
    const int pol = db_policy(1);
    if (ix.canonical_only) hipLaunchKernelGGL(k_db_neighbours<true>, g, blk, 0, s, ix, codes, ascii, N, dirs, cutoff, pol, out);
    else hipLaunchKernelGGL(k_db_neighbours<false>, g, blk, 0, s, ix, codes, ascii, N, dirs, cutoff, pol, out);
    return hipGetLastError();
}

hipError_t launch_db_walk(const IndexDev& ix, const uint64_t* codes, const uint8_t* ascii, uint64_t S, int dir, uint32_t L, uint32_t cutoff, int mode,
                          uint8_t* bases, uint32_t* len, uint8_t* stop, uint32_t* tf, uint64_t* last, hipStream_t s) {
    if (S == 0) return hipSuccess;
    // a workgroup per 64 seeds while that fits a grid: the hardware hands a finished workgroup's place to the next one
    const dim3 g(db_grid(S, 1u << 22)), blk(kDB);
    const int pol = db_policy(2);
#define AIX_DB_WALK(C, U) hipLaunchKernelGGL((k_db_walk<C, U>), g, blk, 0, s, ix, codes, ascii, S, dir, L, cutoff, pol, bases, len, stop, tf, last)
    if (ix.canonical_only) { if (mode == AIX_WALK_UNITIG) AIX_DB_WALK(true, true); else AIX_DB_WALK(true, false); }
    else { if (mode == AIX_WALK_UNITIG) AIX_DB_WALK(false, true); else AIX_DB_WALK(false, false); }
#undef AIX_DB_WALK
    return hipGetLastError();
}

}  // namespace aix

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
static int db_check_input(const aix_index_t* h, const void* codes, const void* ascii, uint64_t n) {
    if (!h) return AIX_ERR_ARG;
    if (h->k != 23) return AIX_ERR_MODE;
    if (n && ((codes == nullptr) == (ascii == nullptr))) return AIX_ERR_ARG;     // exactly one of the two forms
    if (n >= (1ULL << 56)) return AIX_ERR_ARG;
    return AIX_OK;
}

extern "C" int aix_neighbours_dev(aix_index_t* h, const uint64_t* d_codes, const char* d_ascii, uint64_t N, int dirs, uint32_t cutoff, aix_cont_t* d_out,
                                  void* stream) {
    const int st = db_check_input(h, d_codes, d_ascii, N);
    if (st) return st;
    if (dirs != AIX_DIR_NEXT && dirs != AIX_DIR_PREV && dirs != AIX_DIR_BOTH) return AIX_ERR_ARG;
    if (N && !d_out) return AIX_ERR_ARG;
    if (N == 0) return AIX_OK;
    if (h->n == 0) return AIX_ERR_UNSUPPORTED;
    DevGuard g(h->device);
    HIPCHK(launch_db_neighbours(h->dev(), d_codes, (const uint8_t*)d_ascii, N, dirs, cutoff, (uint32_t*)d_out, (hipStream_t)stream));
    return AIX_OK;
}

extern "C" int aix_neighbours(aix_index_t* h, const uint64_t* codes, const char* ascii, uint64_t N, int dirs, uint32_t cutoff, aix_cont_t* out) {
    const int st = db_check_input(h, codes, ascii, N);
    if (st) return st;
    if (dirs != AIX_DIR_NEXT && dirs != AIX_DIR_PREV && dirs != AIX_DIR_BOTH) return AIX_ERR_ARG;
    if (N && !out) return AIX_ERR_ARG;
    if (N == 0) return AIX_OK;
    if (h->n == 0) return AIX_ERR_UNSUPPORTED;
    DevGuard g(h->device);
    const uint64_t in_bytes = codes ? 8 * N : 23 * N, out_bytes = 32 * N * (dirs == AIX_DIR_BOTH ? 2 : 1);
    DevBuf din, dout;
    AIXCHK(din.alloc(in_bytes + 16));
    AIXCHK(dout.alloc(out_bytes));
    HIPCHK(hipMemcpy(din.p, codes ? (const void*)codes : (const void*)ascii, in_bytes, hipMemcpyHostToDevice));
    const int r = aix_neighbours_dev(h, codes ? (const uint64_t*)din.p : nullptr, codes ? nullptr : (const char*)din.p, N, dirs, cutoff, (aix_cont_t*)dout.p, nullptr);
    if (r) return r;
    HIPCHK(hipMemcpy(out, dout.p, out_bytes, hipMemcpyDeviceToHost));
    return AIX_OK;
}

// the checks both walk forms share; *cells = S * max_steps
static int db_check_walk(const aix_index_t* h, const void* codes, const void* ascii, uint64_t S, int dir, uint64_t max_steps, int mode, const void* bases,
                         const void* len, const void* stop, uint64_t* cells) {
    const int st = db_check_input(h, codes, ascii, S);
    if (st) return st;
    if (dir != AIX_DIR_NEXT && dir != AIX_DIR_PREV) return AIX_ERR_ARG;
    if (mode != AIX_WALK_GREEDY && mode != AIX_WALK_UNITIG) return AIX_ERR_ARG;
    if (max_steps < 1 || max_steps > AIX_WALK_MAX_STEPS) return AIX_ERR_ARG;
    if (S && (!bases || !len || !stop)) return AIX_ERR_ARG;
    if (__builtin_mul_overflow(S, max_steps, cells) || *cells >= (1ULL << 48)) return AIX_ERR_NOMEM;     // no buffer of that size exists (4 bytes per cell of out_tf)
    return AIX_OK;
}

extern "C" int aix_walk_dev(aix_index_t* h, const uint64_t* d_codes, const char* d_ascii, uint64_t S, int dir, uint64_t max_steps, uint32_t cutoff, int mode,
                            uint8_t* d_bases, uint32_t* d_len, uint8_t* d_stop, uint32_t* d_tf, uint64_t* d_last, void* stream) {
    uint64_t cells = 0;
    const int st = db_check_walk(h, d_codes, d_ascii, S, dir, max_steps, mode, d_bases, d_len, d_stop, &cells);
    if (st) return st;
    if (S == 0) return AIX_OK;
    if (h->n == 0) return AIX_ERR_UNSUPPORTED;
    DevGuard g(h->device);
    HIPCHK(launch_db_walk(h->dev(), d_codes, (const uint8_t*)d_ascii, S, dir, (uint32_t)max_steps, cutoff, mode, d_bases, d_len, d_stop, d_tf, d_last, (hipStream_t)stream));
    return AIX_OK;
}

extern "C" int aix_walk(aix_index_t* h, const uint64_t* codes, const char* ascii, uint64_t S, int dir, uint64_t max_steps, uint32_t cutoff, int mode,
                        uint8_t* out_bases, uint32_t* out_len, uint8_t* out_stop, uint32_t* out_tf, uint64_t* out_last) {
    uint64_t cells = 0;
    const int st = db_check_walk(h, codes, ascii, S, dir, max_steps, mode, out_bases, out_len, out_stop, &cells);
    if (st) return st;
    if (S == 0) return AIX_OK;
    if (h->n == 0) return AIX_ERR_UNSUPPORTED;
    DevGuard g(h->device);
    const uint64_t in_bytes = codes ? 8 * S : 23 * S;
    DevBuf din, db, dl, ds, dt, dc;
    AIXCHK(din.alloc(in_bytes + 16));
    AIXCHK(db.alloc(cells));
    AIXCHK(dl.alloc(4 * S));
    AIXCHK(ds.alloc(S));
    if (out_tf) AIXCHK(dt.alloc(4 * cells));
    if (out_last) AIXCHK(dc.alloc(8 * S));
    HIPCHK(hipMemcpy(din.p, codes ? (const void*)codes : (const void*)ascii, in_bytes, hipMemcpyHostToDevice));
    // a row is written up to its length only: the caller's rows go up first, so that what lies beyond comes back as it was
    HIPCHK(hipMemcpy(db.p, out_bases, cells, hipMemcpyHostToDevice));
    if (out_tf) HIPCHK(hipMemcpy(dt.p, out_tf, 4 * cells, hipMemcpyHostToDevice));
    const int r = aix_walk_dev(h, codes ? (const uint64_t*)din.p : nullptr, codes ? nullptr : (const char*)din.p, S, dir, max_steps, cutoff, mode, (uint8_t*)db.p,
                               (uint32_t*)dl.p, (uint8_t*)ds.p, out_tf ? (uint32_t*)dt.p : nullptr, out_last ? (uint64_t*)dc.p : nullptr, nullptr);
    if (r) return r;
    HIPCHK(hipMemcpy(out_bases, db.p, cells, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_len, dl.p, 4 * S, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_stop, ds.p, S, hipMemcpyDeviceToHost));
    if (out_tf) HIPCHK(hipMemcpy(out_tf, dt.p, 4 * cells, hipMemcpyDeviceToHost));
    if (out_last) HIPCHK(hipMemcpy(out_last, dc.p, 8 * S, hipMemcpyDeviceToHost));
    return AIX_OK;
}
