// aix_readfix.hip — read cleaning over a 23-mer index resident in HBM: weak-window profile, longest solid span, single-base fixes.
//   READ::set_fm / STUPID_READ::set_fm   read.hpp:286-307, :392-402   fm[i] = get_freq of window i; an error window iff fm[i] <= TRUE_ERRORS
//   Settings::TRUE_ERRORS                settings.cpp:10              default 1 (the `true_errors` argument)
//   cut_end_from / cut_start_to          read.hpp:324-343             the trim span (trim_start, trim_len) names what they keep
//   Correction / CorrectionErrors        read.hpp:36-117              the log rows (position, old byte) and simple_ok / simple_n0 / simple_nM
//   PHASH_MAP::get_freq(uint64_t)        hash.hpp:123-140             forward strand, then the reverse complement; the forward strand wins
// The reference keeps the profile, the cuts and the counters; it has no corrector, so the two boundary rules (phase R, phase L) are
// the ones written down in include/aindex_hip.h and DESIGN 5f.
//
// Layout: one wave per read, four waves per workgroup. A wave stages its read's bytes in its own 4 KiB of LDS (that is the
// AIX_READFIX_MAX_LEN cap; nothing outside [start, end) is ever read from the buffer), so that a window's code under a substituted base
// is 23 LDS byte reads and no global traffic. The solid bitmap lives in registers: lane l holds windows [64 l, 64 l + 64). Boundaries
// (solid next to weak) are one shift across the lane seam, a mask and a __ballot. Every probe trip is wave-uniform and goes through
// freq23_wave (aix_probe.hpp), all lanes calling it with a `want` flag:
//   profile   lane = window, ceil(W / 64) trips
//   try       lane = (base b = lane >> 4, window j = lane & 15): the <= 16 windows lo .. hi under each of the four bases, ONE trip; the
//             base the read has fails by construction (the weak boundary window is among lo .. hi) and is not probed
//   re-probe  after a fix, ONE trip over the <= 22 windows that contain p and were not among lo .. hi
// Both phase loops strictly advance (a fix raises `fixes`, a failure moves c by at least one window), so they are bounded by
// W + max_fixes trips each; there is no run-until-done form. Offsets into the buffer and the log rows are 64 bits wide. Integer only.
#include "aix_env.hpp"
#include "aix_hostkit.hpp"
#include "aix_probe.hpp"

namespace aix {

static constexpr int kRF = 256;                                   // four waves = four reads per workgroup
static constexpr uint32_t kRFMax = AIX_READFIX_MAX_LEN;

// The absence filter of a trip: 0 = FilterGauge, 1 = always consulted, 2 = never. Wave-uniform. The same struct as DbFilter of
// aix_debruijn.hip (private to that file, which stays as it is); a change to one belongs in the other.
struct RfFilter {
    int policy;
    FilterGauge fg;
    __device__ __forceinline__ bool on() const { return policy == 1 ? true : (policy == 2 ? false : fg.on); }
    __device__ __forceinline__ void seen(bool active, bool found) { if (policy == 0) fg.seen(active, found); }
};

__device__ __forceinline__ uint64_t rf_low_bits(int n) {          // n <= 0: none, n >= 64: all
    return n <= 0 ? 0ull : (n >= 64 ? ~0ull : ((1ull << n) - 1));
}
// bits of the wave-wide range [a, a + cnt) that fall into lane `lane`'s word, and the bits of m (bit j = window a + j) moved there
__device__ __forceinline__ void rf_place(uint32_t lane, int a, int cnt, uint64_t m, uint64_t& range, uint64_t& bits) {
    const int d = a - 64 * (int)lane;                             // position of window a in this lane's word
    const uint64_t r = rf_low_bits(cnt);
    if (d >= 64 || d <= -64) { range = 0; bits = 0; }
    else if (d >= 0) { range = r << d; bits = (m & r) << d; }
    else { range = r >> -d; bits = (m & r) >> -d; }
}

// the 46-bit code of window w of the staged read with byte `p` read as `sub` (p < 0: as staged); valid = all 23 bytes upper-case ACGT
__device__ __forceinline__ uint64_t rf_code(const uint8_t* sh, uint32_t w, int p, uint32_t sub, bool& valid) {
    uint64_t code = 0;
    bool ok = true;
#pragma unroll
    for (uint32_t j = 0; j < 23; ++j) {
        uint32_t c = sh[w + j];
        if ((int)(w + j) == p) c = sub;
        const uint32_t v = c == 'A' ? 0u : (c == 'C' ? 1u : (c == 'G' ? 2u : (c == 'T' ? 3u : 4u)));
        ok = ok && v < 4u;
        code = (code << 2) | (uint64_t)(v & 3u);
    }
    valid = ok;
    return code;
}

__device__ __forceinline__ void rf_lds_fence() {                  // a wave's LDS writes before its other lanes' reads
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

template <bool CANON>
__global__ void __launch_bounds__(kRF) k_reads_fix(const IndexDev ix_, uint8_t* __restrict__ buf, uint64_t total, const uint64_t* __restrict__ starts,
                                                  const uint64_t* __restrict__ ends, uint64_t M, uint32_t t, uint32_t V, uint32_t F, int policy,
                                                  uint32_t* __restrict__ rec, uint32_t* __restrict__ fix_pos, uint8_t* __restrict__ fix_old) {
    const IndexDev& ix = ix_;
    __shared__ uint8_t stage[kRF / 64][kRFMax];
    const uint32_t lane = threadIdx.x & 63u, wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint8_t* sh = stage[wv];
    RfFilter fl_prof{policy, {}}, fl_try{policy, {}};             // profile trips find most windows, try trips miss most candidates
    const uint64_t stride = (uint64_t)gridDim.x * (kRF / 64);
    for (uint64_t r = (uint64_t)blockIdx.x * (kRF / 64) + wv; r < M; r += stride) {                           // wave-uniform
        const uint64_t st = starts[r], en = ends[r];
        uint32_t status = 0xFFFFFFFFu;
        if (st > en || en > total) status = AIX_FIX_BAD_RANGE;
        else if (en - st < 23) status = AIX_FIX_SHORT;
        else if (en - st > kRFMax) status = AIX_FIX_TOO_LONG;
        if (status != 0xFFFFFFFFu) {
            if (lane < 8) rec[r * 8 + lane] = lane == 0 ? status : 0u;
            continue;
        }
        const uint32_t L = (uint32_t)(en - st);
        const int W = (int)L - 22;
        rf_lds_fence();                                           // the previous read's last LDS reads before this one's bytes
        for (uint32_t j = lane; j < L; j += 64) sh[j] = buf[st + j];
        rf_lds_fence();

        // ---- profile (read.hpp:286-307): lane = window ----
        uint64_t sol = 0;                                         // bit k of lane l: window 64 l + k is solid (fm > t); 0 from W on
        for (int base = 0; base < W; base += 64) {
            const int i = base + (int)lane;
            bool valid = false, found;
            uint64_t code = 0;
            if (i < W) code = rf_code(sh, (uint32_t)i, -1, 0, valid);
            const bool want = i < W && valid;                     // an invalid window is not probed: fm = 0
            const uint32_t tf = freq23_wave<CANON>(ix, want, code, fl_prof.on(), found);
            fl_prof.seen(want, found);
            const uint64_t m = __ballot(want && tf > t);          // read.hpp:296: weak iff fm <= TRUE_ERRORS
            if ((int)lane == (base >> 6)) sol = m;
        }
        uint32_t solid_n = (uint32_t)__popcll(sol);
        for (int o = 32; o; o >>= 1) solid_n += __shfl_xor(solid_n, o);
        const uint32_t weak_before = (uint32_t)W - solid_n;
        const uint64_t in_w = rf_low_bits(W - 64 * (int)lane);    // this lane's windows below W

        uint32_t fixes = 0, n0 = 0, nM = 0;
        // ---- phase R (dir 0), then phase L (dir 1) ----
        for (int dir = 0; dir < 2; ++dir) {
            int c = dir == 0 ? 1 : W - 2;
            for (int trip = 0; trip < W + (int)F && fixes < F; ++trip) {                                     // bounded: every trip fixes or moves c
                // the boundary: R the smallest i >= c with solid(i - 1) && weak(i); L the largest i <= c with weak(i) && solid(i + 1)
                uint64_t nb;
                if (dir == 0) {
                    const uint64_t up = __shfl_up(sol, 1);
                    nb = (sol << 1) | (lane == 0 ? 0ull : up >> 63);
                    nb &= ~rf_low_bits(c - 64 * (int)lane);
                } else {
                    const uint64_t dn = __shfl_down(sol, 1);
                    nb = (sol >> 1) | (lane == 63 ? 0ull : dn << 63);
                    nb &= rf_low_bits(c + 1 - 64 * (int)lane);
                }
                nb &= ~sol & in_w;
                const uint64_t lanes = __ballot(nb != 0);
                if (lanes == 0) break;
                const int bl = dir == 0 ? __builtin_ctzll(lanes) : 63 - __builtin_clzll(lanes);
                const uint64_t word = __shfl(nb, bl);
                const int i = __builtin_amdgcn_readfirstlane(64 * bl + (dir == 0 ? __builtin_ctzll(word) : 63 - __builtin_clzll(word)));
                const int p = dir == 0 ? i + 22 : i;
                const int lo = dir == 0 ? i : (i - (int)V + 1 > 0 ? i - (int)V + 1 : 0);
                const int hi = dir == 0 ? (i + (int)V - 1 < W - 1 ? i + (int)V - 1 : W - 1) : i;
                const int n = hi - lo + 1;                        // 1 .. V <= 16
                // ---- try(p, lo, hi): lane = (base, window), one trip ----
                const uint32_t old = sh[p];
                const bool letter = (old | 0x20u) >= 'a' && (old | 0x20u) <= 'z';   // a separator is never written
                const uint32_t b = lane >> 4, j = lane & 15u;
                const uint32_t sub = (uint32_t)(AIX_LUT_ACGT >> (8 * b)) & 0xFFu;
                bool valid = false, found;
                uint64_t code = 0;
                const bool cand = letter && (int)j < n && sub != old;               // the base the read has fails by construction
                if (cand) code = rf_code(sh, (uint32_t)lo + j, p, sub, valid);
                const bool want = cand && valid;
                const uint32_t tf = freq23_wave<CANON>(ix, want, code, fl_try.on(), found);
                fl_try.seen(want, found);
                const uint64_t bad = __ballot((int)j < n && !(want && tf > t));
                uint32_t nok = 0, pick = 0;
                for (uint32_t q = 0; q < 4; ++q)
                    if (((bad >> (16 * q)) & 0xFFFFull) == 0) { ++nok; pick = q; }
                if (nok != 1) {
                    if (nok == 0) ++n0; else ++nM;
                    c = dir == 0 ? i + 1 : i - 1;
                    continue;
                }
                // ---- fix: the byte in LDS and in the buffer, the log row, the windows lo .. hi (all solid now) ----
                const uint32_t nbyte = (uint32_t)(AIX_LUT_ACGT >> (8 * pick)) & 0xFFu;
                rf_lds_fence();
                if (lane == 0) {
                    sh[p] = (uint8_t)nbyte;
                    buf[st + (uint64_t)p] = (uint8_t)nbyte;
                    fix_pos[r * (uint64_t)F + fixes] = (uint32_t)p;
                    fix_old[r * (uint64_t)F + fixes] = (uint8_t)old;
                }
                rf_lds_fence();
                ++fixes;
                uint64_t range, bits;
                rf_place(lane, lo, n, ~0ull, range, bits);
                sol |= range;
                // ---- re-probe the windows that contain p and were not tried: R (hi, min(p, W - 1)], L [max(p - 22, 0), lo) ----
                const int ra = dir == 0 ? hi + 1 : (p - 22 > 0 ? p - 22 : 0);
                const int rb = dir == 0 ? (p < W - 1 ? p : W - 1) : lo - 1;
                const int rn = rb - ra + 1;                       // <= 22
                if (rn > 0) {                                     // wave-uniform
                    bool v2 = false, f2;
                    uint64_t c2 = 0;
                    const bool in = (int)lane < rn;
                    if (in) c2 = rf_code(sh, (uint32_t)ra + lane, -1, 0, v2);
                    const bool w2 = in && v2;
                    const uint32_t tf2 = freq23_wave<CANON>(ix, w2, c2, fl_prof.on(), f2);
                    fl_prof.seen(w2, f2);
                    const uint64_t m2 = __ballot(w2 && tf2 > t);
                    rf_place(lane, ra, rn, m2, range, bits);
                    sol = (sol & ~range) | bits;
                }
                // c stays: window i is solid now, the next boundary lies further on
            }
        }

        // ---- what is left: weak windows, the longest run of solid windows (the earliest on ties) ----
        solid_n = (uint32_t)__popcll(sol);
        for (int o = 32; o; o >>= 1) solid_n += __shfl_xor(solid_n, o);
        const uint32_t weak_after = (uint32_t)W - solid_n;
        uint32_t best = 0, best_at = 0, run = 0, run_at = 0;
        for (int k = 0; 64 * k < W; ++k) {                        // wave-uniform: every lane walks the runs of word k
            uint64_t w = __shfl(sol, k);
            uint32_t pos = 0;
            while (pos < 64) {
                if (w & 1ull) {
                    const uint32_t ones = ~w == 0 ? 64u : (uint32_t)__builtin_ctzll(~w);
                    if (run == 0) run_at = 64u * (uint32_t)k + pos;
                    run += ones;
                    pos += ones;
                    w = ones >= 64 ? 0ull : w >> ones;
                    if (run > best) { best = run; best_at = run_at; }
                } else {
                    run = 0;
                    if (w == 0) break;
                    const uint32_t z = (uint32_t)__builtin_ctzll(w);
                    pos += z;
                    w >>= z;
                }
            }
        }
        status = weak_before == 0 ? AIX_FIX_CLEAN : (weak_after == 0 ? AIX_FIX_FIXED : (fixes > 0 ? AIX_FIX_PARTIAL : AIX_FIX_UNFIXED));
        const uint32_t out[8] = {status, weak_before, weak_after, fixes, n0, nM, best ? best_at : 0u, best ? best + 22u : 0u};
        uint32_t mine = out[0];
#pragma unroll
        for (uint32_t q = 1; q < 8; ++q) mine = lane == q ? out[q] : mine;
        if (lane < 8) rec[r * 8 + lane] = mine;
    }
}

// AIX_DBJ_FILTER (A/B switch, aix_debruijn.hip): the absence-filter policy of the neighbour / walk kernels and of this one. Not set: the
// per-trip gauge, one for the profile trips and one for the try trips. Not measured here.
static inline int rf_policy() { return (int)env_int("AIX_DBJ_FILTER", 0, 2, 0); }

hipError_t launch_reads_fix(const IndexDev& ix, uint8_t* buf, uint64_t total, const uint64_t* starts, const uint64_t* ends, uint64_t M, uint32_t t, uint32_t V,
                            uint32_t F, aix_readfix_t* rec, uint32_t* fix_pos, uint8_t* fix_old, hipStream_t s) {
    if (M == 0) return hipSuccess;
    // a workgroup per four reads while that fits a grid: the hardware hands a finished workgroup's place to the next one
    uint64_t g = (M + 3) / 4;
    if (g > (1u << 22)) g = 1u << 22;
    const dim3 grid((unsigned)g), blk(kRF);
    const int pol = rf_policy();
    if (ix.canonical_only) hipLaunchKernelGGL(k_reads_fix<true>, grid, blk, 0, s, ix, buf, total, starts, ends, M, t, V, F, pol, (uint32_t*)rec, fix_pos, fix_old);
    else hipLaunchKernelGGL(k_reads_fix<false>, grid, blk, 0, s, ix, buf, total, starts, ends, M, t, V, F, pol, (uint32_t*)rec, fix_pos, fix_old);
    return hipGetLastError();
}

}  // namespace aix

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
static_assert(sizeof(aix_readfix_t) == 32, "aix_readfix_t is eight u32 words");

// the checks both forms share
static int rf_check(const aix_index_t* h, const void* buf, const void* start, const void* end, uint64_t M, uint32_t verify, uint32_t max_fixes, const void* rec,
                    const void* fix_pos, const void* fix_old) {
    if (!h) return AIX_ERR_ARG;
    if (h->k != 23) return AIX_ERR_MODE;
    if (verify < 1 || verify > AIX_READFIX_MAX_VERIFY || max_fixes > AIX_READFIX_MAX_FIXES) return AIX_ERR_ARG;
    if (M >= (1ULL << 56)) return AIX_ERR_ARG;
    if (M && (!buf || !start || !end || !rec)) return AIX_ERR_ARG;
    if (M && max_fixes && (!fix_pos || !fix_old)) return AIX_ERR_ARG;
    return AIX_OK;
}

extern "C" int aix_reads_fix_dev(aix_index_t* h, char* d_buf, uint64_t total_bytes, const uint64_t* d_start, const uint64_t* d_end, uint64_t M,
                                 uint32_t true_errors, uint32_t verify, uint32_t max_fixes, aix_readfix_t* d_rec, uint32_t* d_fix_pos, uint8_t* d_fix_old,
                                 void* stream) {
    const int st = rf_check(h, d_buf, d_start, d_end, M, verify, max_fixes, d_rec, d_fix_pos, d_fix_old);
    if (st) return st;
    if (M == 0) return AIX_OK;
    if (h->n == 0) return AIX_ERR_UNSUPPORTED;
    DevGuard g(h->device);
    HIPCHK(launch_reads_fix(h->dev(), (uint8_t*)d_buf, total_bytes, d_start, d_end, M, true_errors, verify, max_fixes, d_rec, d_fix_pos, d_fix_old,
                            (hipStream_t)stream));
    return AIX_OK;
}

extern "C" int aix_reads_fix(aix_index_t* h, char* buf, uint64_t total_bytes, const uint64_t* start, const uint64_t* end, uint64_t M, uint32_t true_errors,
                             uint32_t verify, uint32_t max_fixes, aix_readfix_t* rec, uint32_t* fix_pos, uint8_t* fix_old) {
    const int st = rf_check(h, buf, start, end, M, verify, max_fixes, rec, fix_pos, fix_old);
    if (st) return st;
    if (M == 0) return AIX_OK;
    if (h->n == 0) return AIX_ERR_UNSUPPORTED;
    // ascending and disjoint: end[i] <= start[i + 1], and no range that will be worked on begins before an earlier one of those ended
    uint64_t last_end = 0;
    for (uint64_t i = 0; i < M; ++i) {
        if (i + 1 < M && end[i] > start[i + 1]) return AIX_ERR_ARG;
        if (start[i] > end[i] || end[i] > total_bytes) continue;          // AIX_FIX_BAD_RANGE: never touched
        if (start[i] < last_end) return AIX_ERR_ARG;
        last_end = end[i];
    }
    uint64_t cells = 0;
    if (__builtin_mul_overflow(M, (uint64_t)max_fixes, &cells) || cells >= (1ULL << 48)) return AIX_ERR_NOMEM;
    DevGuard g(h->device);
    DevBuf db, ds, de, dr, dp, dold;
    AIXCHK(db.alloc(total_bytes));
    AIXCHK(ds.alloc(8 * M));
    AIXCHK(de.alloc(8 * M));
    AIXCHK(dr.alloc(sizeof(aix_readfix_t) * M));
    HIPCHK(hipMemcpy(db.p, buf, total_bytes, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ds.p, start, 8 * M, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(de.p, end, 8 * M, hipMemcpyHostToDevice));
    if (max_fixes) {
        AIXCHK(dp.alloc(4 * cells));
        AIXCHK(dold.alloc(cells));
        // a row is written up to `fixes` only: the caller's rows go up first, so that what lies beyond comes back as it was
        HIPCHK(hipMemcpy(dp.p, fix_pos, 4 * cells, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(dold.p, fix_old, cells, hipMemcpyHostToDevice));
    }
    const int r = aix_reads_fix_dev(h, (char*)db.p, total_bytes, (const uint64_t*)ds.p, (const uint64_t*)de.p, M, true_errors, verify, max_fixes,
                                    (aix_readfix_t*)dr.p, max_fixes ? (uint32_t*)dp.p : nullptr, max_fixes ? (uint8_t*)dold.p : nullptr, nullptr);
    if (r) return r;
    HIPCHK(hipMemcpy(rec, dr.p, sizeof(aix_readfix_t) * M, hipMemcpyDeviceToHost));
    if (max_fixes) {
        HIPCHK(hipMemcpy(buf, db.p, total_bytes, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(fix_pos, dp.p, 4 * cells, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(fix_old, dold.p, cells, hipMemcpyDeviceToHost));
    }
    return AIX_OK;
}
