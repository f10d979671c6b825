// aix_probe.hpp — private: the probe of the batch kernels (verification table, side index, unfiled keys, MPHF fallback) and the
// absence-filter gauge, shared by the translation units whose kernels look 23-mers up (aix_lookup.hip, aix_count.hip, aix_debruijn.hip, aix_unitigs.hip).
#pragma once
#include "aix_internal.hpp"

namespace aix {

// ---------------------------------------------------------------------------------------------
// probes
// ---------------------------------------------------------------------------------------------
struct Probe {
    uint64_t slot;
    uint32_t tf;
    uint32_t lines;     // instrumentation for MODE_LINES: MPHF records read | 16 per key record read | 256 per completed evaluation | 4096 per filter word | 65536 per bucket line
    bool found;
};
// MPHF path: evaluate the MPHF on the hash (a, b, c) of the probed bytes, verify against the stored code.
// `filters`: the hashed bytes are exactly the ASCII of `code`. Only then do a stored key's fingerprint / presence
// bits (computed from ITS ASCII) say anything about this probe; the reference's forward probe of a query with
// non-ACGT bytes hashes the raw bytes but compares the sanitised code (python_wrapper.cpp:611-613) and can — by a
// 1-in-n coincidence of slots — match a stored key whose hash is different, so that probe runs unfiltered.
__device__ __forceinline__ Probe probe23_mphf(const IndexDev& ix, uint64_t a, uint64_t b, uint64_t c, uint64_t code, bool filters) {
    Probe r;
    r.found = false;
    r.tf = 0;
    r.slot = 0;
    r.lines = 3;
    if (!filters) {
        r.lines += 256;
        r.slot = mphf_from_hash(ix.m, a, b, c);
    } else if (ix.early_exit) {
        if (!mphf_probe_early_exit(ix.m, a, b, c, r.slot, r.lines)) return r;   // a node lacks one of the key's presence bits
        r.lines += 256;
    } else if (ix.use_fp) {
        r.lines += 256;
        uint32_t fps;
        uint64_t node;
        r.slot = mphf_from_hash_fp(ix.m, a, b, c, fps, node);
        if (fps != fp_of_hash(a, b, c)) return r;  // the key assigned to this node (if any) is a different key
    } else {
        r.lines += 256;
        r.slot = mphf_from_hash(ix.m, a, b, c);
    }
    if (r.slot < ix.n) {                           // python_wrapper.cpp:613 `h1 >= n ||`
        const KeyRec k = key_at(ix, r.slot);
        r.lines += 16;
        if (k.code == code) { r.found = true; r.tf = k.tf; }
    }
    return r;
}
// one lane on its own (ragged lengths, index construction): hash the 23 ASCII bytes in (w0,w1,w2), MPHF path
__device__ __forceinline__ Probe probe23(const IndexDev& ix, uint64_t w0, uint64_t w1, uint64_t w2, uint64_t code, bool filters = true) {
    uint64_t a, b, c;
    jenkins23(w0, w1, w2, ix.m.seed, a, b, c);
    return probe23_mphf(ix, a, b, c, code, filters);
}
// same, but the forward hash (a,b,c) was computed elsewhere (ragged lengths)
__device__ __forceinline__ Probe probe23_hashed(const IndexDev& ix, uint64_t a, uint64_t b, uint64_t c, uint64_t code) {
    return probe23_mphf(ix, a, b, c, code, false);
}

// The probe of the batch kernels. EVERY lane of the wave calls it (want = false: this lane has nothing to probe); with the
// verification table on, a probe whose hashed bytes are the ASCII of `code` (filters) is answered from its bucket line, all
// others — and an unmatched probe of an overflowed bucket — by the MPHF path.
// `absence`: consult the absence filter first (wave-uniform; the callers switch it per loop trip, see FilterGauge).
template <int LPP>
__device__ __forceinline__ Probe probe23_wave(const IndexDev& ix, bool want, uint64_t w0, uint64_t w1, uint64_t w2, uint64_t code, bool filters = true,
                                              bool absence = true) {
    Probe r;
    r.found = false; r.tf = 0; r.slot = 0; r.lines = 0;
    bool use = want && filters && ix.bk, mphf = want;
    if (ix.bk && ix.bloom && absence && use) {                  // absent from the filter = not a filed key; an unfiled key (overflow) is in it too
        r.lines += 4096;
        uint32_t hw, hb;
        filter_key(code, hw, hb);                               // filters: the hashed bytes are the ASCII of `code`, so the code is the key
        const uint64_t m = bloom_mask(hb);
        if ((ix.bloom[bloom_word(hw, ix.nbloom)] & m) != m) { use = false; mphf = false; }
    }
    uint64_t a = 0, b = 0, c = 0;
    if (use || mphf) jenkins23(w0, w1, w2, ix.m.seed, a, b, c); // only the lanes that go on to the bucket or the MPHF path
    if (ix.bk) {
        const BkRes k = bucket_probe_wave<LPP>(ix.bk, ix.nb, use, a, code);
        if (use) {
            r.lines += 65536;
            if (k.found) { r.found = true; r.tf = k.tf; r.slot = k.slot; }
            mphf = !k.found && k.overflow;
        }
    }
    if (mphf) {
        const Probe q = probe23_mphf(ix, a, b, c, code, filters);
        r.found = q.found; r.tf = q.tf; r.slot = q.slot; r.lines += q.lines;
    }
    return r;
}

// get_freq(uint64_t) (hash.hpp:123-140) = get_tf_value_23mer (python_wrapper.cpp:610-627) of the lane's code: the two-strand probe, forward
// strand first. Wave-cooperative: every lane calls it (want = false: nothing to probe). The body of k_lookup23_codes at 8 lanes per probe.
template <bool CANON>
__device__ __forceinline__ uint32_t freq23_wave(const IndexDev& ix, bool want, uint64_t u, bool absence, bool& found) {
    const uint64_t r = revcomp(u, 23);
    uint64_t w0, w1, w2;
    if (CANON) {
        const uint64_t key = u <= r ? u : r;
        ascii23_of_rc(u <= r ? r : u, w0, w1, w2);               // string of `key`
        const Probe p = probe23_wave<8>(ix, want, w0, w1, w2, key, true, absence);
        found = p.found;
        return p.found ? p.tf : 0u;
    }
    ascii23_of_rc(r, w0, w1, w2);
    const Probe f = probe23_wave<8>(ix, want, w0, w1, w2, u, true, absence);
    ascii23_of_rc(u, w0, w1, w2);
    const Probe g = probe23_wave<8>(ix, want && !f.found, w0, w1, w2, r, true, absence);
    found = f.found || g.found;
    return f.found ? f.tf : (g.found ? g.tf : 0u);
}

// The sibling of freq23_wave<true> that also says WHERE the key is stored: the probe of min(u, revcomp u), whose `slot` is the kid of a
// found key (key_at(ix, slot).code is that canonical code). Wave-cooperative like freq23_wave; the compaction (aix_unitigs.hip) links
// k-mers to their neighbours through it.
__device__ __forceinline__ Probe slot23_wave(const IndexDev& ix, bool want, uint64_t u, bool absence) {
    const uint64_t r = revcomp(u, 23);
    uint64_t w0, w1, w2;
    ascii23_of_rc(u <= r ? r : u, w0, w1, w2);                   // string of min(u, r)
    return probe23_wave<8>(ix, want, w0, w1, w2, u <= r ? u : r, true, absence);
}

// The absence filter pays when most probes are absent keys (one cached 8-byte read instead of a 128-byte line from HBM) and
// costs when most are present (one more read each). A wave decides trip by trip from what it has just seen: the filter is
// consulted in the next trip iff fewer than a quarter of this trip's queries were found. The answers do not depend on it.
struct FilterGauge {
    bool on = true;
    __device__ __forceinline__ void seen(bool active, bool found) {
        const uint32_t a = (uint32_t)__popcll(__ballot(active)), f = (uint32_t)__popcll(__ballot(active && found));
        if (a) on = 4u * f < a;
    }
};

}  // namespace aix
