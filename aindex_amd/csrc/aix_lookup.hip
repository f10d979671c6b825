// aix_lookup.hip — lookups and coverage: the device-pointer entry points, and their host-pointer twins with the two staging paths (tiny
// batches through pinned, device-mapped memory of the handle; large ones through a three-deep pipeline of pinned blocks and streams).
// The kernels come first: batch MPHF lookups (23-/13-mer) and per-position coverage, with their launchers.
//
// All kernels are HBM/latency-bound integer work (no MFMA): one query / window per lane, three
// independent 16-byte MPHF record reads + one 16-byte key record read per probe, grid-stride
// launches of >= 8 workgroups per CU so that ~2k probes per CU are in flight.
#include <algorithm>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "aix_env.hpp"
#include "aix_handle.hpp"
#include "aix_launch.hpp"
#include "aix_probe.hpp"

namespace aix {

// Result of get_tf_value_23mer-style probing (python_wrapper.cpp:610-627): strand 0 absent, 1 fwd, 2 rc
struct Q23 {
    uint64_t slot;
    uint32_t tf;
    uint32_t strand;
    uint32_t lines;
};
// wave-cooperative (all lanes call it; `active` = this lane holds a query)
// `reload(a, b, c)` fetches the query's 23 bytes again: the rare lane-by-lane path of a canonical index takes them from memory a second time instead
// of holding the original words, their code and its reverse complement (10 VGPRs) across the wave's probe for a case that almost never comes
template <bool CANON, int LPP, class RELOAD>
__device__ __forceinline__ Q23 query23(const IndexDev& ix, bool active, uint64_t w0, uint64_t w1, uint64_t w2, FilterGauge& fg, RELOAD&& reload) {
    const Enc23 e = encode23_words(w0, w1, w2);
    const uint64_t r = revcomp(e.code, 23);
    Q23 out;
    out.slot = 0; out.tf = 0; out.strand = 0; out.lines = 0;
    if (CANON) {
        // every stored code is canonical: only the canonical strand of a pure-ACGT query can match. ONE probe call site: with the
        // strands chosen per lane first, a wave runs Jenkins + the probe once, not once per strand with half its lanes idle
        const bool fwd = e.code <= r;
        const bool clean = active && e.valid, other = active && !e.valid;
        uint64_t x0 = w0, x1 = w1, x2 = w2;
        if (!fwd) ascii23_of_rc(e.code, x0, x1, x2);
        const Probe p = probe23_wave<LPP>(ix, clean, x0, x1, x2, fwd ? e.code : r, true, fg.on);
        fg.seen(clean, p.found);
        if (clean) {
            out.lines = p.lines;
            if (p.found) { out.slot = p.slot; out.tf = p.tf; out.strand = fwd ? 1u : 2u; }
        }
        if (other) {                                            // other bytes: the reference's two probes, lane by lane (rare)
            uint64_t v0, v1, v2;
            reload(v0, v1, v2);
            const Enc23 e2 = encode23_words(v0, v1, v2);
            uint64_t a, b, c;
            jenkins23(v0, v1, v2, ix.m.seed, a, b, c);
            const Probe f = probe23_mphf(ix, a, b, c, e2.code, false);   // raw bytes hashed, sanitised code compared
            out.lines = f.lines;
            if (f.found) { out.slot = f.slot; out.tf = f.tf; out.strand = 1; }
            else {
                uint64_t r0, r1, r2;
                ascii23_of_rc(e2.code, r0, r1, r2);             // decode(reverseDNA(u)), :615-616
                const Probe g = probe23(ix, r0, r1, r2, revcomp(e2.code, 23));
                out.lines += g.lines;
                if (g.found) { out.slot = g.slot; out.tf = g.tf; out.strand = 2; }
            }
        }
        return out;
    }
    const Probe f = probe23_wave<LPP>(ix, active, w0, w1, w2, e.code, e.valid, fg.on);   // raw bytes hashed, sanitised code compared
    uint64_t r0, r1, r2;
    ascii23_of_rc(e.code, r0, r1, r2);                          // decode(reverseDNA(u)), :615-616
    const Probe g = probe23_wave<LPP>(ix, active && !f.found, r0, r1, r2, r, true, fg.on);
    fg.seen(active, f.found || g.found);
    if (active) {
        out.lines = f.lines;
        if (f.found) { out.slot = f.slot; out.tf = f.tf; out.strand = 1; }
        else {
            out.lines += g.lines;
            if (g.found) { out.slot = g.slot; out.tf = g.tf; out.strand = 2; }
        }
    }
    return out;
}
template <bool CANON, int LPP>
__device__ __forceinline__ Q23 query23(const IndexDev& ix, bool active, uint64_t w0, uint64_t w1, uint64_t w2, FilterGauge& fg) {
    return query23<CANON, LPP>(ix, active, w0, w1, w2, fg, [&](uint64_t& a, uint64_t& b, uint64_t& c) { a = w0; b = w1; c = w2; });
}

// get_tf_both_directions_23mer (python_wrapper.cpp:1259-1275): Q1(q) and Q1(decode(rc(q))); wave-cooperative like query23
template <bool CANON, int LPP>
__device__ __forceinline__ void both23(const IndexDev& ix, bool active, uint64_t w0, uint64_t w1, uint64_t w2, uint32_t& fwd, uint32_t& rc, FilterGauge& fg) {
    const Enc23 e = encode23_words(w0, w1, w2);
    const uint64_t r = revcomp(e.code, 23);
    fwd = 0; rc = 0;
    const bool fast = CANON && e.valid;                         // canonical index, pure-ACGT query: both directions see the one canonical key
    const Q23 q = query23<CANON, LPP>(ix, active && fast, w0, w1, w2, fg);
    if (active && fast) { fwd = q.tf; rc = q.tf; }
    const bool slow = active && !fast;
    if (CANON) {
        if (slow) {                                             // non-ACGT bytes on a canonical index: lane by lane, MPHF path
            uint64_t r0, r1, r2, s0, s1, s2;
            ascii23_of_rc(e.code, r0, r1, r2);
            ascii23_of_rc(r, s0, s1, s2);
            uint64_t a, b, c;
            jenkins23(w0, w1, w2, ix.m.seed, a, b, c);
            const Probe F = probe23_mphf(ix, a, b, c, e.code, false);
            const Probe R = probe23(ix, r0, r1, r2, r);
            const Probe S = probe23(ix, s0, s1, s2, e.code);    // second call's fallback decodes the sanitised code
            fwd = F.found ? F.tf : (R.found ? R.tf : 0u);
            rc = R.found ? R.tf : (S.found ? S.tf : 0u);
        }
        return;
    }
    uint64_t r0, r1, r2, s0, s1, s2;
    ascii23_of_rc(e.code, r0, r1, r2);
    ascii23_of_rc(r, s0, s1, s2);
    const Probe F = probe23_wave<LPP>(ix, slow, w0, w1, w2, e.code, e.valid, fg.on);
    const Probe R = probe23_wave<LPP>(ix, slow, r0, r1, r2, r, true, fg.on);
    const Probe S2 = probe23_wave<LPP>(ix, slow && !e.valid, s0, s1, s2, e.code, true, fg.on);
    fg.seen(slow, F.found || R.found);
    if (slow) {
        const Probe S = e.valid ? F : S2;
        fwd = F.found ? F.tf : (R.found ? R.tf : 0u);
        rc = R.found ? R.tf : (S.found ? S.tf : 0u);
    }
}

template <int MODE, bool CANON, int LPP>
__global__ void __launch_bounds__(kBlock) k_lookup23_ascii(const IndexDev ix_, const uint8_t* __restrict__ q, uint64_t N, LookupOut out,
                                                          const uint32_t* __restrict__ gate /* nullable: non-zero = the binned path answers this batch */) {
    if (gate && *gate) return;
    const IndexDev& ix = ix_;
    FilterGauge fg;
    AIX_WAVE_LOOP(i, N) {
        const bool in = i < N;
        uint64_t w0 = 0, w1 = 0, w2 = 0;
        if (in) load23(q + 23 * i, w0, w1, w2);
        auto again = [&](uint64_t& a, uint64_t& b, uint64_t& c) { load23(q + 23 * i, a, b, c); };
        if (MODE == MODE_TF) {
            const uint32_t v = query23<CANON, LPP>(ix, in, w0, w1, w2, fg, again).tf;
            if (in) out.tf[i] = v;
        } else if (MODE == MODE_LINES) {
            const uint32_t v = query23<CANON, LPP>(ix, in, w0, w1, w2, fg).lines;   // instrumentation: records read for this query
            if (in) out.tf[i] = v;
        } else if (MODE == MODE_HASH) {
            if (in) {
                uint64_t a, b, c;
                jenkins23(w0, w1, w2, ix.m.seed, a, b, c);
                out.u64a[i] = mphf_from_hash(ix.m, a, b, c);
            }
        } else if (MODE == MODE_KIDSTRAND) {
            const Q23 r = query23<CANON, LPP>(ix, in, w0, w1, w2, fg, again);
            if (in) {
                if (out.u64a) out.u64a[i] = r.slot;             // get_kid_by_kmer: 0 when absent (:700-716)
                if (out.strand) out.strand[i] = (uint8_t)r.strand;
            }
        } else {
            uint32_t f, r;
            both23<CANON, LPP>(ix, in, w0, w1, w2, f, r, fg);
            if (in) {
                if (MODE == MODE_TOTAL) {
                    out.u64a[i] = (uint64_t)f + (uint64_t)r;
                } else {
                    if (out.u64a) out.u64a[i] = f;
                    if (out.u64b) out.u64b[i] = r;
                }
            }
        }
    }
}

// pass C of the binned lookup (aix_lookup_binned.hip): the queries list[0 .. *count) of a canonical index through the same probe
// as above. The grid is sized for the worst case; *count and the gate word are read on the device.
template <int LPP>
__global__ void __launch_bounds__(kBlock) k_lookup23_list(const IndexDev ix_, const uint8_t* __restrict__ q, const uint32_t* __restrict__ list,
                                                         const uint32_t* __restrict__ count, const uint32_t* __restrict__ gate, uint32_t* __restrict__ out,
                                                         unsigned long long* __restrict__ survivors_stat) {
    if (!*gate) return;
    const IndexDev& ix = ix_;
    const uint64_t n = *count;
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(survivors_stat, (unsigned long long)n);
    FilterGauge fg;
    AIX_WAVE_LOOP(j, n) {
        const bool in = j < n;
        const uint64_t i = in ? list[j] : 0;
        uint64_t w0 = 0, w1 = 0, w2 = 0;
        if (in) load23(q + 23 * i, w0, w1, w2);
        auto again = [&](uint64_t& a, uint64_t& b, uint64_t& c) { load23(q + 23 * i, a, b, c); };
        const uint32_t v = query23<true, LPP>(ix, in, w0, w1, w2, fg, again).tf;
        if (in) out[i] = v;
    }
}

template <bool CANON, int LPP>
__global__ void __launch_bounds__(kBlock) k_lookup23_codes(const IndexDev ix_, const uint64_t* __restrict__ codes, uint64_t N, uint32_t* __restrict__ out) {
    const IndexDev& ix = ix_;
    FilterGauge fg;
    AIX_WAVE_LOOP(i, N) {
        const bool in = i < N;
        const uint64_t u = in ? (codes[i] & ((1ULL << 46) - 1)) : 0ull;
        const uint64_t r = revcomp(u, 23);
        uint64_t w0, w1, w2;
        uint32_t tf = 0;
        if (CANON) {
            const uint64_t key = u <= r ? u : r;
            ascii23_of_rc(u <= r ? r : u, w0, w1, w2);           // string of `key`
            const Probe p = probe23_wave<LPP>(ix, in, w0, w1, w2, key, true, fg.on);
            fg.seen(in, p.found);
            tf = p.found ? p.tf : 0u;
        } else {
            ascii23_of_rc(r, w0, w1, w2);
            const Probe f = probe23_wave<LPP>(ix, in, w0, w1, w2, u, true, fg.on);
            ascii23_of_rc(u, w0, w1, w2);
            const Probe g = probe23_wave<LPP>(ix, in && !f.found, w0, w1, w2, r, true, fg.on);
            fg.seen(in, f.found || g.found);
            tf = f.found ? f.tf : (g.found ? g.tf : 0u);
        }
        if (in) out[i] = tf;
    }
}

// variable-length queries: the reference hashes ALL bytes of the std::string but encodes the first 23
__global__ void __launch_bounds__(kBlock) k_lookup23_ragged(const IndexDev ix, const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ offs,
                                                           uint64_t N, uint32_t* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < N; i += stride) {
        const uint64_t lo = offs[i], len = offs[i + 1] - lo;
        uint32_t tf = 0;
        if (len >= 23) {
            uint64_t w0, w1, w2;
            load23(bytes + lo, w0, w1, w2);
            if (len == 23) {                                     // lane by lane (lengths differ inside a wave): the MPHF path, both probes
                const Enc23 e = encode23_words(w0, w1, w2);
                const Probe f = probe23(ix, w0, w1, w2, e.code, e.valid);
                if (f.found) tf = f.tf;
                else {
                    uint64_t r0, r1, r2;
                    ascii23_of_rc(e.code, r0, r1, r2);
                    const Probe g = probe23(ix, r0, r1, r2, revcomp(e.code, 23));
                    tf = g.found ? g.tf : 0u;
                }
            } else {
                const Enc23 e = encode23_words(w0, w1, w2);
                uint64_t a, b, c;
                jenkins_bytes(bytes + lo, len, ix.m.seed, a, b, c);
                const Probe f = probe23_hashed(ix, a, b, c, e.code);
                if (f.found) tf = f.tf;
                else {
                    uint64_t r0, r1, r2;
                    ascii23_of_rc(e.code, r0, r1, r2);
                    const Probe g = probe23(ix, r0, r1, r2, revcomp(e.code, 23));
                    tf = g.found ? g.tf : 0u;
                }
            }
        }
        out[i] = tf;
    }
}

// ---------------------------------------------------------------------------------------------
// 13-mer mode: the MPHF over all 4^13 13-mers is a bijection code -> slot, so the table is kept in
// 2-bit-code order in HBM (tf13_code) and a valid query is one 8-byte read. Queries with bytes
// outside ACGT take the reference's raw-bytes MPHF path against the mphf-ordered copy.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t tf13_raw(const IndexDev& ix, uint64_t w0, uint64_t w1) {
    uint64_t a, b, c;
    jenkins13(w0, w1, ix.m.seed, a, b, c);
    const uint64_t h = mphf_from_hash(ix.m, a, b, c);
    return h < 67108864ull ? ix.tf13_mphf[h] : 0ull;            // reference indexes unguarded (:534); OOB -> 0
}
// get_reverse_complement_13mer (python_wrapper.cpp:505-517) on raw bytes: reverse; A<->T, C<->G; others kept
__device__ __forceinline__ void rc13_raw(uint64_t w0, uint64_t w1, uint64_t& r0, uint64_t& r1) {
    r0 = 0; r1 = 0;
#pragma unroll
    for (int i = 0; i < 13; ++i) {
        const int j = 12 - i;
        uint32_t ch = (uint32_t)((j < 8 ? (w0 >> (8 * j)) : (w1 >> (8 * (j - 8)))) & 0xff);
        ch = ch == 'A' ? 'T' : ch == 'T' ? 'A' : ch == 'G' ? 'C' : ch == 'C' ? 'G' : ch;
        if (i < 8) r0 |= (uint64_t)ch << (8 * i);
        else r1 |= (uint64_t)ch << (8 * (i - 8));
    }
}

template <int MODE>
__global__ void __launch_bounds__(kBlock) k_lookup13_ascii(const IndexDev ix, const uint8_t* __restrict__ q, uint64_t N, LookupOut out) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < N; i += stride) {
        uint64_t w0, w1;
        load13(q + 13 * i, w0, w1);
        const Enc13 e = encode13_words(w0, w1);
        if (MODE == MODE_TF) {                                  // get_tf_values_13mer :938-980: strict, u32 truncation
            out.tf[i] = e.valid ? (uint32_t)ix.tf13_code[e.code] : 0u;
        } else if (MODE == MODE_HASH) {                         // hasher_13mer.lookup(kmer) (:1087): the tabulated slot, or the MPHF of the raw bytes
            uint64_t hval;
            if (e.valid) hval = ix.perm13[e.code];
            else { uint64_t a, b, c; jenkins13(w0, w1, ix.m.seed, a, b, c); hval = mphf_from_hash(ix.m, a, b, c); }
            out.u64a[i] = hval;
        } else {
            uint64_t f, r;
            if (e.valid) {
                f = ix.tf13_code[e.code];
                r = ix.tf13_code[(uint32_t)revcomp(e.code, 13)];
            } else {                                            // :522-543 has no validation: raw bytes are hashed
                uint64_t r0, r1;
                rc13_raw(w0, w1, r0, r1);
                f = tf13_raw(ix, w0, w1);
                r = tf13_raw(ix, r0, r1);
            }
            if (MODE == MODE_TOTAL) out.u64a[i] = f + r;
            else {
                if (out.u64a) out.u64a[i] = f;
                if (out.u64b) out.u64b[i] = r;
            }
        }
    }
}

__global__ void __launch_bounds__(kBlock) k_lookup13_ragged(const IndexDev ix, const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ offs,
                                                           uint64_t N, uint32_t* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < N; i += stride) {
        const uint64_t lo = offs[i], len = offs[i + 1] - lo;
        uint32_t tf = 0;
        if (len == 13) {                                        // is_13mer(): length check first (:943)
            uint64_t w0, w1;
            load13(bytes + lo, w0, w1);
            const Enc13 e = encode13_words(w0, w1);
            if (e.valid) tf = (uint32_t)ix.tf13_code[e.code];
        }
        out[i] = tf;
    }
}

// ---------------------------------------------------------------------------------------------
// coverage: one lane per byte position of the concatenated sequences (aindex.py:314-322)
// ---------------------------------------------------------------------------------------------
// (eight waves per SIMD: 64 VGPRs with two spilled words instead of 69 and seven waves — 268-270 against 280-282 ms per 10^10 positions on one box;
// the same limit on k_lookup23_ascii costs 5-7 %, so it is set here only)
template <bool CANON, int LPP>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(8, 8))) k_coverage(const IndexDev ix_, const uint8_t* __restrict__ seqs, const uint64_t* __restrict__ offs, uint64_t M,
                                                    uint64_t total, double seqs_per_byte, uint32_t cutoff, uint32_t* __restrict__ out,
                                                    const uint64_t* __restrict__ out_offs) {
    const IndexDev& ix = ix_;
    const uint32_t k = ix.k;
    FilterGauge fg;
    AIX_WAVE_LOOP(p, total) {
        // sequence containing byte p: largest s with offs[s] <= p. The lanes of a wave hold consecutive p, so the binary search
        // runs once per wave for its first position (wave-uniform: scalar loads), and a lane then walks forward from there —
        // zero or one step unless the sequences are shorter than a wave is wide (then a bounded walk, then its own search).
        // (the builtin returns int: without the cast a low half with bit 31 set sign-extends over the high half, the search lands on the last
        // sequence and the positions [2^31, 2^32) mod 2^32 of a batch come back 0 — rounds 1 and 2 did that to 43 % of config 5 at full size)
        const uint64_t p0 = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(p_base >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)p_base);
        // the window's bytes are requested before anything is known about the sequence they belong to (a window inside the buffer can be read
        // whether or not it lies inside ONE sequence): the loads fly while the search below waits for its offsets
        const bool inb = p + k <= total;
        uint64_t w0 = 0, w1 = 0, w2 = 0;
        if (inb) { if (k == 23) load23(seqs + p, w0, w1, w2); else load13(seqs + p, w0, w1); }     // (k = 13, same box: 185 against 198 ms per 10^10 positions; k = 23 within noise)
        // The search starts from where p0 would lie if all sequences had the mean length — exact for equal lengths, the usual batch — and
        // gallops from there: two independent loads instead of log2(M) dependent ones per trip of every wave (20 round trips at 10^6 sequences,
        // several times the latency of the probe itself). Any guess gives the same s.
        uint64_t lo, hi;                                        // invariant offs[lo] <= p0 < offs[hi] (or lo == 0)
        {
            uint64_t g = (uint64_t)((double)p0 * seqs_per_byte);
            if (g >= M) g = M - 1;
            const uint64_t og = offs[g], og1 = offs[g + 1];
            if (og <= p0) {
                lo = g; hi = g + 1;
                if (og1 <= p0) {
                    uint64_t step = 1;
                    while (hi < M && offs[hi] <= p0) { lo = hi; step <<= 1; hi = (M - lo > step) ? lo + step : M; }
                }
            } else {
                hi = g; lo = g ? g - 1 : 0;
                uint64_t step = 1;
                while (lo > 0 && offs[lo] > p0) { hi = lo; step <<= 1; lo = lo > step ? lo - step : 0; }
            }
        }
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) >> 1;
            if (offs[mid] <= p0) lo = mid; else hi = mid;
        }
        const uint64_t begin0 = offs[lo], end0 = offs[lo + 1];
        // one probe per lane either way; the two cases are kept apart so that the usual one carries nothing per lane across the probe but the
        // window words (its output address is a wave-uniform base plus the lane number)
        auto answer = [&](bool active) -> uint32_t {
            if (k == 23) return query23<CANON, LPP>(ix, active, w0, w1, w2, fg, [&](uint64_t& a, uint64_t& b, uint64_t& c) { load23(seqs + p, a, b, c); }).tf;
            if (!active) return 0u;
            const Enc13 e = encode13_words(w0, w1);
            return e.valid ? (uint32_t)ix.tf13_code[e.code] : 0u;
        };
        if (begin0 <= p0 && end0 > p0 + 63) {                   // all 64 positions of the wave lie in sequence lo (the usual case): nothing is looked up per lane
            uint32_t* const wdst = out + (out_offs[lo] + (p0 - begin0));      // wave-uniform
            const bool active = inb && p + k <= end0;
            const uint32_t tf = answer(active);
            if (active) wdst[threadIdx.x & 63u] = tf >= cutoff ? tf : 0u;
        } else {
            bool active = inb;
            uint64_t s = lo;
            uint32_t* dst = out;
            if (active) {
                for (int step = 0; step < 4 && s + 1 < M && offs[s + 1] <= p; ++step) ++s;
                if (s + 1 < M && offs[s + 1] <= p) {
                    uint64_t l2 = s + 1, h2 = M;                // offs[l2] <= p < offs[h2]
                    while (h2 - l2 > 1) {
                        const uint64_t mid = (l2 + h2) >> 1;
                        if (offs[mid] <= p) l2 = mid; else h2 = mid;
                    }
                    s = l2;
                }
                const uint64_t begin = offs[s], end = offs[s + 1];
                if (p < begin || p + k > end) active = false;   // p < begin: gaps between sequences are allowed
                dst = out + (out_offs[s] + (p - begin));
            }
            const uint32_t tf = answer(active);
            if (active) *dst = tf >= cutoff ? tf : 0u;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// launchers: all asynchronous on `s`, return hipGetLastError(). The two that aix_lookup_binned.hip calls too are in aix_internal.hpp.
// ---------------------------------------------------------------------------------------------
template <bool CANON>
static hipError_t lookup23_ascii_mode(const IndexDev& ix, const uint8_t* q, uint64_t N, int mode, LookupOut out, const uint32_t* gate, hipStream_t s) {
    switch (mode) {
        case MODE_TF: return with_lpp(ix.bk_lpp, [&](auto L) { return launch_flat(k_lookup23_ascii<MODE_TF, CANON, decltype(L)::value>, N, s, ix, q, N, out, gate); });
        case MODE_LINES: return launch_flat(k_lookup23_ascii<MODE_LINES, CANON, 8>, N, s, ix, q, N, out, gate);
        case MODE_HASH: return launch_flat(k_lookup23_ascii<MODE_HASH, CANON, 8>, N, s, ix, q, N, out, gate);
        case MODE_KIDSTRAND: return launch_flat(k_lookup23_ascii<MODE_KIDSTRAND, CANON, 8>, N, s, ix, q, N, out, gate);
        case MODE_BOTH: return launch_flat(k_lookup23_ascii<MODE_BOTH, CANON, 8>, N, s, ix, q, N, out, gate);
        case MODE_TOTAL: return launch_flat(k_lookup23_ascii<MODE_TOTAL, CANON, 8>, N, s, ix, q, N, out, gate);
    }
    return hipErrorInvalidValue;
}
hipError_t launch_lookup23_ascii(const IndexDev& ix, const uint8_t* q, uint64_t N, int mode, LookupOut out, hipStream_t s, const uint32_t* gate) {
    if (N == 0) return hipSuccess;
    return ix.canonical_only ? lookup23_ascii_mode<true>(ix, q, N, mode, out, gate, s) : lookup23_ascii_mode<false>(ix, q, N, mode, out, gate, s);
}
hipError_t launch_lookup23_list(const IndexDev& ix, const uint8_t* q, const uint32_t* list, const uint32_t* count, uint64_t max_count, const uint32_t* gate,
                                uint32_t* out, unsigned long long* survivors_stat, hipStream_t s) {
    return with_lpp(ix.bk_lpp, [&](auto L) { return launch_flat(k_lookup23_list<decltype(L)::value>, max_count, s, ix, q, list, count, gate, out, survivors_stat); });
}
static hipError_t launch_lookup23_codes(const IndexDev& ix, const uint64_t* codes, uint64_t N, uint32_t* out, hipStream_t s) {
    if (N == 0) return hipSuccess;
    return ix.canonical_only ? launch_flat(k_lookup23_codes<true, 8>, N, s, ix, codes, N, out) : launch_flat(k_lookup23_codes<false, 8>, N, s, ix, codes, N, out);
}
static hipError_t launch_lookup23_ragged(const IndexDev& ix, const uint8_t* bytes, const uint64_t* offs, uint64_t N, uint32_t* out, hipStream_t s) {
    if (N == 0) return hipSuccess;
    return launch_flat(k_lookup23_ragged, N, s, ix, bytes, offs, N, out);
}
static hipError_t launch_lookup13_ascii(const IndexDev& ix, const uint8_t* q, uint64_t N, int mode, LookupOut out, hipStream_t s) {
    if (N == 0) return hipSuccess;
    switch (mode) {
        case MODE_TF: return launch_flat(k_lookup13_ascii<MODE_TF>, N, s, ix, q, N, out);
        case MODE_HASH: return launch_flat(k_lookup13_ascii<MODE_HASH>, N, s, ix, q, N, out);
        case MODE_BOTH: return launch_flat(k_lookup13_ascii<MODE_BOTH>, N, s, ix, q, N, out);
        case MODE_TOTAL: return launch_flat(k_lookup13_ascii<MODE_TOTAL>, N, s, ix, q, N, out);
    }
    return hipErrorInvalidValue;
}
static hipError_t launch_lookup13_ragged(const IndexDev& ix, const uint8_t* bytes, const uint64_t* offs, uint64_t N, uint32_t* out, hipStream_t s) {
    if (N == 0) return hipSuccess;
    return launch_flat(k_lookup13_ragged, N, s, ix, bytes, offs, N, out);
}
static hipError_t launch_coverage(const IndexDev& ix, const uint8_t* seqs, const uint64_t* offs, uint64_t M, uint64_t total, uint32_t cutoff, uint32_t* out,
                                  const uint64_t* out_offs, hipStream_t s) {
    if (M == 0 || total == 0) return hipSuccess;
    const double seqs_per_byte = (double)M / (double)total;
    if (ix.k == 23 && ix.canonical_only)
        return with_lpp(ix.bk_lpp, [&](auto L) { return launch_flat(k_coverage<true, decltype(L)::value>, total, s, ix, seqs, offs, M, total, seqs_per_byte, cutoff, out, out_offs); });
    return launch_flat(k_coverage<false, 8>, total, s, ix, seqs, offs, M, total, seqs_per_byte, cutoff, out, out_offs);
}

}  // namespace aix

// ---------------------------------------------------------------------------------------------
// device-pointer entry points
// ---------------------------------------------------------------------------------------------
static int lookup_ascii_dev(aix_index_t* h, const char* d_kmers, uint64_t N, int mode, LookupOut o, void* stream) {
    if (!h || (N && !d_kmers)) return AIX_ERR_ARG;
    if (N == 0) return AIX_OK;
    DevGuard g(h->device);
    const IndexDev d = h->dev();
    if (h->k == 23) {
        if (h->n == 0) return AIX_ERR_UNSUPPORTED;             // empty index: the host twins answer 0 without a launch
        if (mode == MODE_TF) {                                 // large absent-heavy batches on a canonical index: filter read from L2
            const int st = lookup23_binned(h, d, (const uint8_t*)d_kmers, N, o.tf, (hipStream_t)stream);
            if (st != AIX_LB_NOT_TAKEN) return st == AIX_LB_TAKEN ? AIX_OK : st;
        }
        HIPCHK(launch_lookup23_ascii(d, (const uint8_t*)d_kmers, N, mode, o, (hipStream_t)stream));
    } else {
        if (mode == MODE_KIDSTRAND) return AIX_ERR_MODE;       // hash_map is null in 13-mer mode (kid / strand need the checker)
        HIPCHK(launch_lookup13_ascii(d, (const uint8_t*)d_kmers, N, mode, o, (hipStream_t)stream));
    }
    return AIX_OK;
}

extern "C" int aix_tf_batch_ascii_dev(aix_index_t* h, const char* d_kmers, uint64_t N, uint32_t* d_out, void* stream) {
    if (N && !d_out) return AIX_ERR_ARG;
    return lookup_ascii_dev(h, d_kmers, N, MODE_TF, LookupOut{d_out, nullptr, nullptr, nullptr}, stream);
}
// instrumentation: d_out[i] = number of MPHF + key records the tf query i reads under the handle's current settings
extern "C" int aix_lines_batch_ascii_dev(aix_index_t* h, const char* d_kmers, uint64_t N, uint32_t* d_out, void* stream) {
    if (N && !d_out) return AIX_ERR_ARG;
    if (h && h->k != 23) return AIX_ERR_MODE;
    return lookup_ascii_dev(h, d_kmers, N, MODE_LINES, LookupOut{d_out, nullptr, nullptr, nullptr}, stream);
}
extern "C" int aix_hash_batch_ascii_dev(aix_index_t* h, const char* d_kmers, uint64_t N, uint64_t* d_out, void* stream) {
    if (N && !d_out) return AIX_ERR_ARG;
    return lookup_ascii_dev(h, d_kmers, N, MODE_HASH, LookupOut{nullptr, d_out, nullptr, nullptr}, stream);
}
extern "C" int aix_kid_strand_batch_ascii_dev(aix_index_t* h, const char* d_kmers, uint64_t N, uint64_t* d_kid, uint8_t* d_strand, void* stream) {
    return lookup_ascii_dev(h, d_kmers, N, MODE_KIDSTRAND, LookupOut{nullptr, d_kid, nullptr, d_strand}, stream);
}
extern "C" int aix_tf_both_batch_ascii_dev(aix_index_t* h, const char* d_kmers, uint64_t N, uint64_t* d_fwd, uint64_t* d_rc, void* stream) {
    return lookup_ascii_dev(h, d_kmers, N, MODE_BOTH, LookupOut{nullptr, d_fwd, d_rc, nullptr}, stream);
}
extern "C" int aix_tf_total_batch_ascii_dev(aix_index_t* h, const char* d_kmers, uint64_t N, uint64_t* d_out, void* stream) {
    if (N && !d_out) return AIX_ERR_ARG;
    return lookup_ascii_dev(h, d_kmers, N, MODE_TOTAL, LookupOut{nullptr, d_out, nullptr, nullptr}, stream);
}
extern "C" int aix_tf_batch_codes_dev(aix_index_t* h, const uint64_t* d_codes, uint64_t N, uint32_t* d_out, void* stream) {
    if (!h || (N && (!d_codes || !d_out))) return AIX_ERR_ARG;
    if (h->k != 23) return AIX_ERR_MODE;
    if (N == 0) return AIX_OK;
    if (h->n == 0) return AIX_ERR_UNSUPPORTED;
    DevGuard g(h->device);
    HIPCHK(launch_lookup23_codes(h->dev(), d_codes, N, d_out, (hipStream_t)stream));
    return AIX_OK;
}
extern "C" int aix_tf_batch_ragged_dev(aix_index_t* h, const char* d_bytes, const uint64_t* d_offs, uint64_t N, uint32_t* d_out, void* stream) {
    if (!h || (N && (!d_offs || !d_out))) return AIX_ERR_ARG;
    if (N == 0) return AIX_OK;
    DevGuard g(h->device);
    if (h->k == 23) {
        if (h->n == 0) return AIX_ERR_UNSUPPORTED;
        HIPCHK(launch_lookup23_ragged(h->dev(), (const uint8_t*)d_bytes, d_offs, N, d_out, (hipStream_t)stream));
    } else {
        HIPCHK(launch_lookup13_ragged(h->dev(), (const uint8_t*)d_bytes, d_offs, N, d_out, (hipStream_t)stream));
    }
    return AIX_OK;
}
extern "C" int aix_coverage_batch_dev(aix_index_t* h, const char* d_seqs, const uint64_t* d_offs, uint64_t M, uint64_t total_bytes, uint32_t cutoff,
                                      uint32_t* d_out, const uint64_t* d_out_offs, void* stream) {
    if (!h || (M && (!d_seqs || !d_offs || !d_out || !d_out_offs))) return AIX_ERR_ARG;
    if (M == 0 || total_bytes == 0) return AIX_OK;
    if (h->k == 23 && h->n == 0) return AIX_ERR_UNSUPPORTED;
    DevGuard g(h->device);
    HIPCHK(launch_coverage(h->dev(), (const uint8_t*)d_seqs, d_offs, M, total_bytes, cutoff, d_out, d_out_offs, (hipStream_t)stream));
    return AIX_OK;
}

// ---------------------------------------------------------------------------------------------
// host memory <-> pinned staging with several threads (one thread moves ~10 GB/s; PCIe 5 x16 wants ~50)
// ---------------------------------------------------------------------------------------------
namespace {
class CopyPool {
    struct Job { char* dst; const char* src; size_t bytes; };
    std::vector<std::thread> workers;
    std::mutex mu;
    std::condition_variable cv_work, cv_done;
    std::vector<Job> jobs;
    size_t pending = 0;
    bool stop = false;
    void run() {
        for (;;) {
            Job j;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv_work.wait(lk, [&] { return stop || !jobs.empty(); });
                if (stop && jobs.empty()) return;
                j = jobs.back();
                jobs.pop_back();
            }
            memcpy(j.dst, j.src, j.bytes);
            std::lock_guard<std::mutex> lk(mu);
            if (--pending == 0) cv_done.notify_all();
        }
    }

public:
    explicit CopyPool(unsigned n) { for (unsigned i = 0; i < n; ++i) workers.emplace_back([this] { run(); }); }
    ~CopyPool() {
        { std::lock_guard<std::mutex> lk(mu); stop = true; }
        cv_work.notify_all();
        for (auto& t : workers) t.join();
    }
    unsigned size() const { return (unsigned)workers.size(); }
    // one copy at a time per pool user (callers hold their handle's pipe mutex; the pool itself serialises with `busy`)
    std::mutex busy;
    void copy(void* dst, const void* src, size_t bytes) {
        const size_t parts = workers.size() + 1;
        if (bytes < (4u << 20) || parts == 1) { memcpy(dst, src, bytes); return; }
        std::lock_guard<std::mutex> only(busy);
        const size_t slice = ((bytes + parts - 1) / parts + 4095) & ~(size_t)4095;
        size_t off = slice;                                  // the caller takes the first slice itself
        {
            std::lock_guard<std::mutex> lk(mu);
            for (; off < bytes; off += slice) { jobs.push_back(Job{(char*)dst + off, (const char*)src + off, std::min(slice, bytes - off)}); ++pending; }
        }
        cv_work.notify_all();
        memcpy(dst, src, std::min(slice, bytes));
        std::unique_lock<std::mutex> lk(mu);
        cv_done.wait(lk, [&] { return pending == 0; });
    }
};
CopyPool& copy_pool() {
    static CopyPool pool([] {
        unsigned n = std::thread::hardware_concurrency();
        n = n ? std::min(8u, std::max(1u, n / 2)) : 4u;          // measured on the MI355X host: 8 threads feed ~45 GB/s, more only contend
        return (unsigned)env_int("AIX_HOST_COPY_THREADS", 1, 64, n) - 1;   // + the calling thread
    }());
    return pool;
}
}  // namespace

// Large host-buffer batches: the three staging sets of HostPipe (aix_handle.hpp). While set b's
// chunk is on the wire / in the kernel, the host threads fill the next set and drain the one before: H2D, kernel, D2H and the
// two host copies of different chunks overlap. (Round 1 staged synchronously from pageable memory: 25-35 GB/s in.)
static int pipe_init(HostPipe& P) {
    for (int b = 0; b < HostPipe::S; ++b) {
        if (P.hin[b].alloc(HostPipe::kInBytes, hipHostMallocDefault) != hipSuccess) return AIX_ERR_NOMEM;
        if (P.din[b].alloc(HostPipe::kInBytes) != hipSuccess) return AIX_ERR_NOMEM;
        if (P.st[b].create() != hipSuccess) return AIX_ERR_HIP;
        if (P.ev[b].create() != hipSuccess) return AIX_ERR_HIP;
    }
    return AIX_OK;
}
static int pipe_need_out(HostPipe& P, int j) {
    for (int b = 0; b < HostPipe::S; ++b) {
        if (P.hout[b][j].p) continue;
        if (P.hout[b][j].alloc(HostPipe::kOutBytes, hipHostMallocDefault) != hipSuccess) return AIX_ERR_NOMEM;
        if (P.dout[b][j].alloc(HostPipe::kOutBytes) != hipSuccess) return AIX_ERR_NOMEM;
    }
    return AIX_OK;
}

static uint64_t pipe_fail_chunk() {                       // test hook, read once: the chunk of a large host batch whose launch "fails"
    static const uint64_t c = env_u64("AIX_PIPE_TEST_FAIL_CHUNK", 0, ~0ull, ~0ull);
    return c;
}

// in: N elements of in_elem bytes each (host); outs[j]: N elements of out_elem[j] bytes (host, nullable). call(d_in, m, d_out0..2, stream).
template <typename F>
static int pipelined_host_batch(aix_index_t* h, const char* in, uint32_t in_elem, uint64_t N, const uint32_t out_elem[3], void* const outs[3], F&& call) {
    std::lock_guard<std::mutex> lk(h->pipe_mutex);          // one large host batch per handle at a time (they would share the wire anyway)
    if (!h->pipe) {
        std::unique_ptr<HostPipe> fresh(new (std::nothrow) HostPipe());
        if (!fresh) return AIX_ERR_NOMEM;
        const int st = pipe_init(*fresh);
        if (st) { fresh.reset(); (void)hipGetLastError(); return st; }
        h->pipe = std::move(fresh);
    }
    HostPipe& P = *h->pipe;
    for (int j = 0; j < 3; ++j)
        if (outs[j]) { const int st = pipe_need_out(P, j); if (st) { (void)hipGetLastError(); return st; } }
    // every exit but the last one leaves with copies / kernels possibly queued on the pipe's streams; they touch the handle's staging
    // buffers (and caller-pinned outputs), which the next call reuses at once: a failing call drains the streams before it returns
    static_assert(HostPipe::S == 3, "the guard names every stream of the pipe");
    DrainOnError<3> drain_on_error{{&P.st[0], &P.st[1], &P.st[2]}};
    CopyPool& pool = copy_pool();
    // buffers the caller has already pinned (hipHostMalloc / hipHostRegister, e.g. torch pinned tensors) go over the wire as they
    // are; only pageable memory is staged through the pipe's own pinned buffers
    auto pinned = [](const void* p) {
        hipPointerAttribute_t a;
        if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
        return a.type == hipMemoryTypeHost;
    };
    const bool in_pinned = pinned(in);
    bool out_pinned[3] = {false, false, false};
    for (int j = 0; j < 3; ++j) out_pinned[j] = outs[j] && pinned(outs[j]);
    const uint64_t chunk = HostPipe::kChunkQ;
    const uint64_t nchunks = (N + chunk - 1) / chunk;
    auto drain = [&](uint64_t c) -> int {                    // chunk c has completed on the device: hand its answers to the caller
        const int b = (int)(c % HostPipe::S);
        HIPCHK(hipEventSynchronize(P.ev[b]));
        const uint64_t lo = c * chunk, m = std::min(chunk, N - lo);
        for (int j = 0; j < 3; ++j)
            if (outs[j] && !out_pinned[j]) pool.copy((char*)outs[j] + lo * out_elem[j], P.hout[b][j].p, m * out_elem[j]);
        return AIX_OK;
    };
    for (uint64_t c = 0; c < nchunks; ++c) {
        const int b = (int)(c % HostPipe::S);
        if (c >= (uint64_t)HostPipe::S) { const int st = drain(c - HostPipe::S); if (st) return st; }
        const uint64_t lo = c * chunk, m = std::min(chunk, N - lo);
        if (in_pinned) {
            HIPCHK(hipMemcpyAsync(P.din[b].p, in + lo * in_elem, m * in_elem, hipMemcpyHostToDevice, P.st[b]));
        } else {
            pool.copy(P.hin[b].p, in + lo * in_elem, m * in_elem);
            HIPCHK(hipMemcpyAsync(P.din[b].p, P.hin[b].p, m * in_elem, hipMemcpyHostToDevice, P.st[b]));
        }
        int st = call((const char*)P.din[b].p, m, P.dout[b][0].p, P.dout[b][1].p, P.dout[b][2].p, (void*)P.st[b].s);
        if (!st && c == pipe_fail_chunk()) st = AIX_ERR_HIP;                  // AIX_PIPE_TEST_FAIL_CHUNK: fault injection (tests)
        if (st) return st;
        for (int j = 0; j < 3; ++j)
            if (outs[j]) HIPCHK(hipMemcpyAsync(out_pinned[j] ? (void*)((char*)outs[j] + lo * out_elem[j]) : P.hout[b][j].p, P.dout[b][j].p, m * out_elem[j],
                                               hipMemcpyDeviceToHost, P.st[b]));
        HIPCHK(hipEventRecord(P.ev[b], P.st[b]));
    }
    for (uint64_t c = nchunks > (uint64_t)HostPipe::S ? nchunks - HostPipe::S : 0; c < nchunks; ++c) { const int st = drain(c); if (st) return st; }
    drain_on_error.armed = false;
    return AIX_OK;
}

// ---------------------------------------------------------------------------------------------
// host-pointer twins: stage through HBM in bounded chunks, run the same kernels, copy back
// ---------------------------------------------------------------------------------------------
static constexpr uint64_t kSmall = 4096;         // up to here a host batch goes through the pinned, device-mapped staging of the handle

static int ensure_pinned(SmallBatch& sm) {
    if (sm.out[2].p) return AIX_OK;                        // the last one taken: all four are there
    hipError_t e = sm.in.alloc(kSmall * 23 + 64, hipHostMallocMapped);
    for (int j = 0; j < 3 && e == hipSuccess; ++j) e = sm.out[j].alloc(kSmall * 8, hipHostMallocMapped);
    if (e != hipSuccess) { (void)hipGetLastError(); return AIX_ERR_NOMEM; }   // what was taken stays with the handle; the next call asks for the rest
    memset(sm.in.p, '\n', kSmall * 23 + 64);
    return AIX_OK;
}

template <typename F>
static int chunked_ascii(aix_index_t* h, const char* kmers, uint64_t N, const uint32_t out_elem_bytes[3], void* const outs[3], F&& call) {
    if (!h || (N && !kmers)) return AIX_ERR_ARG;
    if (N == 0) return AIX_OK;
    DevGuard g(h->device);
    if (N <= kSmall) {                                     // latency path: the kernel reads the queries from, and writes the answers to, host memory
        SmallBatch& sm = h->small;
        std::lock_guard<std::mutex> lk(sm.mutex);
        if (ensure_pinned(sm) == AIX_OK) {
            void *din = nullptr, *dout[3] = {nullptr, nullptr, nullptr};
            hipError_t e = hipHostGetDevicePointer(&din, sm.in.p, 0);
            for (int j = 0; j < 3 && e == hipSuccess; ++j) e = hipHostGetDevicePointer(&dout[j], sm.out[j].p, 0);
            if (e == hipSuccess) {
                memcpy(sm.in.p, kmers, N * h->k);
                if (sm.stream.create() != hipSuccess) (void)hipGetLastError();                 // (then the null stream)
                int st = call((const char*)din, N, dout[0], dout[1], dout[2], (void*)sm.stream.s);   // own stream: no implicit ordering with the null stream
                if (st) return st;
                HIPCHK(hipStreamSynchronize(sm.stream));
                for (int j = 0; j < 3; ++j)
                    if (outs[j]) memcpy(outs[j], sm.out[j].p, N * out_elem_bytes[j]);
                return AIX_OK;
            }
            (void)hipGetLastError();
        }
    }
    return pipelined_host_batch(h, kmers, h->k, N, out_elem_bytes, outs, call);
}

static bool empty23(const aix_index_t* h) { return h && h->k == 23 && h->n == 0; }

// a host lookup over ASCII k-mers: outs[j] (nullable) takes N elements of eb[j] bytes; an empty 23-mer index answers zeros without the device
template <typename F>
static int host_ascii(aix_index_t* h, const char* kmers, uint64_t N, const uint32_t (&eb)[3], void* const (&outs)[3], F&& call) {
    if (empty23(h)) {
        for (int j = 0; j < 3; ++j) if (outs[j]) memset(outs[j], 0, (uint64_t)eb[j] * N);
        return AIX_OK;
    }
    return chunked_ascii(h, kmers, N, eb, outs, call);
}

extern "C" int aix_tf_batch_ascii(aix_index_t* h, const char* kmers, uint64_t N, uint32_t* out) {
    if (N && !out) return AIX_ERR_ARG;
    return host_ascii(h, kmers, N, {4, 0, 0}, {out, nullptr, nullptr}, [&](const char* dq, uint64_t m, void* a, void*, void*, void* st) {
        return aix_tf_batch_ascii_dev(h, dq, m, (uint32_t*)a, st);
    });
}
extern "C" int aix_hash_batch_ascii(aix_index_t* h, const char* kmers, uint64_t N, uint64_t* out) {
    if (N && !out) return AIX_ERR_ARG;
    if (empty23(h)) return AIX_ERR_UNSUPPORTED;                // no key, no slot: there is no answer to give
    return host_ascii(h, kmers, N, {8, 0, 0}, {out, nullptr, nullptr}, [&](const char* dq, uint64_t m, void* a, void*, void*, void* st) {
        return aix_hash_batch_ascii_dev(h, dq, m, (uint64_t*)a, st);
    });
}
extern "C" int aix_kid_strand_batch_ascii(aix_index_t* h, const char* kmers, uint64_t N, uint64_t* kid_out, uint8_t* strand_out) {
    if (h && h->k != 23) return AIX_ERR_MODE;
    return host_ascii(h, kmers, N, {8, 1, 0}, {kid_out, strand_out, nullptr}, [&](const char* dq, uint64_t m, void* a, void* b, void*, void* st) {
        return aix_kid_strand_batch_ascii_dev(h, dq, m, kid_out ? (uint64_t*)a : nullptr, strand_out ? (uint8_t*)b : nullptr, st);
    });
}
extern "C" int aix_tf_both_batch_ascii(aix_index_t* h, const char* kmers, uint64_t N, uint64_t* fwd_out, uint64_t* rc_out) {
    return host_ascii(h, kmers, N, {8, 8, 0}, {fwd_out, rc_out, nullptr}, [&](const char* dq, uint64_t m, void* a, void* b, void*, void* st) {
        return aix_tf_both_batch_ascii_dev(h, dq, m, fwd_out ? (uint64_t*)a : nullptr, rc_out ? (uint64_t*)b : nullptr, st);
    });
}
extern "C" int aix_tf_total_batch_ascii(aix_index_t* h, const char* kmers, uint64_t N, uint64_t* out) {
    if (N && !out) return AIX_ERR_ARG;
    return host_ascii(h, kmers, N, {8, 0, 0}, {out, nullptr, nullptr}, [&](const char* dq, uint64_t m, void* a, void*, void*, void* st) {
        return aix_tf_total_batch_ascii_dev(h, dq, m, (uint64_t*)a, st);
    });
}

extern "C" int aix_tf_batch_codes(aix_index_t* h, const uint64_t* codes, uint64_t N, uint32_t* out) {
    if (!h || (N && (!codes || !out))) return AIX_ERR_ARG;
    if (h->k != 23) return AIX_ERR_MODE;
    if (N == 0) return AIX_OK;
    if (h->n == 0) { memset(out, 0, 4 * N); return AIX_OK; }
    DevGuard g(h->device);
    const uint32_t eb[3] = {4, 0, 0};
    void* const outs[3] = {out, nullptr, nullptr};
    return pipelined_host_batch(h, (const char*)codes, 8, N, eb, outs, [&](const char* dq, uint64_t m, void* a, void*, void*, void* st) {
        return aix_tf_batch_codes_dev(h, (const uint64_t*)dq, m, (uint32_t*)a, st);
    });
}

extern "C" int aix_tf_batch_ragged(aix_index_t* h, const char* bytes, const uint64_t* offsets, uint64_t N, uint32_t* out) {
    if (!h || (N && (!offsets || !out))) return AIX_ERR_ARG;
    if (N == 0) return AIX_OK;
    if (empty23(h)) { memset(out, 0, 4 * N); return AIX_OK; }
    const uint64_t base = offsets[0], total = offsets[N] - base;
    if (total && !bytes) return AIX_ERR_ARG;
    DevGuard g(h->device);
    DevBuf db, doffs, dout;
    HIPCHK(db.alloc(total + 8));
    HIPCHK(doffs.alloc((N + 1) * 8));
    HIPCHK(dout.alloc(N * 4));
    std::vector<uint64_t> rel(N + 1);
    for (uint64_t i = 0; i <= N; ++i) rel[i] = offsets[i] - base;
    if (total) HIPCHK(hipMemcpy(db.p, bytes + base, total, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(doffs.p, rel.data(), (N + 1) * 8, hipMemcpyHostToDevice));
    int st = aix_tf_batch_ragged_dev(h, (const char*)db.p, (const uint64_t*)doffs.p, N, (uint32_t*)dout.p, nullptr);
    if (st) return st;
    HIPCHK(hipStreamSynchronize(0));
    HIPCHK(hipMemcpy(out, dout.p, N * 4, hipMemcpyDeviceToHost));
    return AIX_OK;
}

extern "C" int aix_coverage_batch(aix_index_t* h, const char* seqs, const uint64_t* offs, uint64_t M, uint32_t cutoff, uint32_t* out,
                                  const uint64_t* out_offs) {
    if (!h || (M && (!seqs || !offs || !out || !out_offs))) return AIX_ERR_ARG;
    if (M == 0) return AIX_OK;
    const uint64_t base = offs[0], total = offs[M] - base, obase = out_offs[0], ototal = out_offs[M] - obase;
    if (ototal == 0) return AIX_OK;
    if (empty23(h)) { memset(out + obase, 0, 4 * ototal); return AIX_OK; }
    DevGuard g(h->device);
    // latency path (one read, one contig window...): sequences, offsets and the profile live in pinned, device-mapped memory
    constexpr uint64_t kCovSeq = 128u << 10, kCovM = 1024, kCovPin = kCovSeq + 64 + 2 * 8 * (kCovM + 1) + 4 * kCovSeq;
    if (total <= kCovSeq && M <= kCovM && ototal <= kCovSeq) {
        SmallBatch& sm = h->small;
        std::lock_guard<std::mutex> lk(sm.mutex);
        if (sm.cov.alloc(kCovPin, hipHostMallocMapped) != hipSuccess) (void)hipGetLastError();
        void* dbase = nullptr;
        if (sm.cov.p && hipHostGetDevicePointer(&dbase, sm.cov.p, 0) == hipSuccess) {
            if (sm.stream.create() != hipSuccess) (void)hipGetLastError();                     // (then the null stream)
            char* hp = (char*)sm.cov.p;
            uint64_t* hoffs = (uint64_t*)(hp + kCovSeq + 64);
            uint64_t* hooffs = hoffs + (kCovM + 1);
            uint32_t* hout = (uint32_t*)(hooffs + (kCovM + 1));
            memcpy(hp, seqs + base, total);
            memset(hp + total, '\n', 8);
            for (uint64_t i = 0; i <= M; ++i) { hoffs[i] = offs[i] - base; hooffs[i] = out_offs[i] - obase; }
            memset(hout, 0, 4 * ototal);
            char* dp = (char*)dbase;
            int st = aix_coverage_batch_dev(h, dp, (const uint64_t*)(dp + ((char*)hoffs - hp)), M, total, cutoff, (uint32_t*)(dp + ((char*)hout - hp)),
                                            (const uint64_t*)(dp + ((char*)hooffs - hp)), (void*)sm.stream.s);
            if (st) return st;
            HIPCHK(hipStreamSynchronize(sm.stream));
            memcpy(out + obase, hout, 4 * ototal);
            return AIX_OK;
        }
        (void)hipGetLastError();
    }
    DevBuf ds, doffs, dooffs, dout;
    HIPCHK(ds.alloc(total + 8));
    HIPCHK(doffs.alloc((M + 1) * 8));
    HIPCHK(dooffs.alloc((M + 1) * 8));
    HIPCHK(dout.alloc(ototal * 4));
    std::vector<uint64_t> rel(M + 1), orel(M + 1);
    for (uint64_t i = 0; i <= M; ++i) { rel[i] = offs[i] - base; orel[i] = out_offs[i] - obase; }
    if (total) HIPCHK(hipMemcpy(ds.p, seqs + base, total, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(doffs.p, rel.data(), (M + 1) * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dooffs.p, orel.data(), (M + 1) * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(dout.p, 0, ototal * 4));
    int st = aix_coverage_batch_dev(h, (const char*)ds.p, (const uint64_t*)doffs.p, M, total, cutoff, (uint32_t*)dout.p, (const uint64_t*)dooffs.p, nullptr);
    if (st) return st;
    HIPCHK(hipStreamSynchronize(0));
    HIPCHK(hipMemcpy(out + obase, dout.p, ototal * 4, hipMemcpyDeviceToHost));
    return AIX_OK;
}
