// aix_index.hip — the index handle's life in HBM: .pf parsing and upload, the tables built at open (verification table, absence
// filter, minimizer-keyed copy, early-exit masks, 13-mer permutation), scatter, create / open / close / info and the setters.
// The kernels of index construction and re-layout come first; each is launched from the one host function below that needs it.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "aix_env.hpp"
#include "aix_handle.hpp"
#include "aix_launch.hpp"

namespace aix {

// ---------------------------------------------------------------------------------------------
// index re-layout
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) k_build_keyrecs(const uint64_t* __restrict__ checker, const uint32_t* __restrict__ tf, uint64_t n, KeyRec* __restrict__ recs,
                                                         uint32_t* __restrict__ noncanon) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    uint32_t bad = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        KeyRec r;
        r.code = checker[i];
        r.tf = tf[i];
        r.pad = 0;
        recs[i] = r;
        bad |= (r.code > revcomp(r.code & ((1ULL << 46) - 1), 23)) || (r.code >> 46);
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicAdd(noncanon, 1u);
}
__global__ void __launch_bounds__(kBlock) k_extract(const IndexDev ix, uint32_t* __restrict__ tf, uint64_t* __restrict__ checker) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < ix.n; i += stride) {
        const KeyRec r = key_at(ix, i);
        if (tf) tf[i] = r.tf;
        if (checker) checker[i] = r.code;
    }
}
// Fingerprints: for every stored code that sits in its own MPHF slot, write its 4-bit fingerprint into the nibble
// of its assigned node. Entries that are not where the MPHF puts them (corrupt / foreign index) are skipped, so a
// fingerprint mismatch always implies checker[rank] != query.
__global__ void __launch_bounds__(kBlock) k_init_ee(const BvRec* __restrict__ recs, uint64_t nrecs, EeRec* __restrict__ ee) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < nrecs; i += stride) {
        EeRec e;
        e.pairs = recs[i].pairs;
        e.prefix = recs[i].prefix;
#pragma unroll
        for (int k = 0; k < 6; ++k) e.mask[k] = 0;
        ee[i] = e;
    }
}
__global__ void __launch_bounds__(kBlock) k_set_fp(const IndexDev ix, BvRec* __restrict__ recs, EeRec* __restrict__ ee, int do_fp) {
    const MphfDev& m = ix.m;
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < ix.n; i += stride) {
        const uint64_t code = key_at(ix, i).code;
        if (code >> 46) continue;
        uint64_t w0, w1, w2, a, b, c, node;
        uint32_t fps;
        ascii23_of_rc(revcomp(code, 23), w0, w1, w2);
        jenkins23(w0, w1, w2, m.seed, a, b, c);
        if (mphf_from_hash_fp(m, a, b, c, fps, node) != i) continue;
        if (do_fp) atomicOr((unsigned long long*)&recs[node >> 4].fp, (unsigned long long)fp_of_hash(a, b, c) << (4 * (uint32_t)(node & 15)));
        if (!ee) continue;
        const uint64_t nd[3] = {fastmod(a, m.fm), m.D + fastmod(b, m.fm), 2 * m.D + fastmod(c, m.fm)};
#pragma unroll
        for (int t = 0; t < 3; ++t) {                     // the key's two presence bits at each of its three nodes
            const uint32_t bit = (uint32_t)(nd[t] & 15) * 12u, sh = bit & 31u;
            const uint32_t q = present_mask(a, b, c, t);
            uint32_t* w = ee[nd[t] >> 4].mask + (bit >> 5);
            atomicOr(w, q << sh);
            if (sh > 20u) atomicOr(w + 1, q >> (32u - sh));
        }
    }
}

// Verification table (aix_device.hpp: BkEntry). Filed: every stored code that sits in its own MPHF slot, under the bucket its
// Jenkins hash selects; the first eight arrivals of a bucket get an entry, the rest are left to the MPHF path (pass 2 raises
// the bucket's overflow bit). Which eight is decided by the order of the atomics — the answers do not depend on it.
__global__ void __launch_bounds__(kBlock) k_bk_init(BkEntry* __restrict__ bk, uint64_t nent) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < nent; i += stride) {
        BkEntry e;
        e.code_lo = 0xFFFFFFFFu; e.code_hi = AIX_BK_EMPTY_HI; e.tf = 0; e.slot = 0;
        bk[i] = e;
    }
}
__global__ void __launch_bounds__(kBlock) k_bk_fill(const MphfDev m, const KeyRec* __restrict__ keys, uint64_t n, BkEntry* __restrict__ bk, uint32_t nb,
                                                   uint32_t* __restrict__ fill, uint64_t* __restrict__ bloom, uint32_t nbloom, uint32_t nbm, uint32_t* __restrict__ mfill,
                                                   uint32_t* __restrict__ side) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const KeyRec kr = keys[i];
        side[i] = 0xFFFFFFFFu;                                   // not filed until the entry has been written below
        if (kr.code >> 46) continue;
        uint64_t w0, w1, w2, a, b, c;
        ascii23_of_rc(revcomp(kr.code, 23), w0, w1, w2);
        jenkins23(w0, w1, w2, m.seed, a, b, c);
        if (mphf_from_hash(m, a, b, c) != i) continue;         // not where the MPHF puts it: the reference cannot find it, neither can a probe
        if (bloom) {                                           // keyed by the code itself (aix_device.hpp: filter_key)
            uint32_t hw, hb;
            filter_key(kr.code, hw, hb);
            atomicOr((unsigned long long*)&bloom[bloom_word(hw, nbloom)], (unsigned long long)bloom_mask(hb));
        }
        const uint32_t bi = bucket_of(a, nb);
        const uint32_t pos = atomicAdd(&fill[bi], 1u);
        BkEntry e;
        e.code_lo = (uint32_t)kr.code; e.code_hi = (uint32_t)(kr.code >> 32); e.tf = kr.tf; e.slot = (uint32_t)i;
        if (pos < 8u) { bk[(uint64_t)bi * 8 + pos] = e; side[i] = bi * 8u + pos; }      // (nb * 8 < 2^31: nb = n / load + 1 with n < 2^32 ... checked by the caller)
        if (nbm) atomicAdd(&mfill[mk_home(minimizer23(kr.code, revcomp(kr.code, 23)), nbm)], 1u);    // the minimizer-keyed copy: sized here, written by k_mk_fill
    }
}
// The same entries once more, grouped by the bucket of their minimizer: bucket b = mk[off[b], off[b + 1]) holds EVERY filed key whose
// minimizer hashes to b (the keys of one minimizer arrive together, ~8 at a time, so fixed-size buckets overflowed for 15-30 % of the
// windows; a bucket sized by its content never does). Same filing condition as k_bk_fill.
__global__ void __launch_bounds__(kBlock) k_mk_fill(const MphfDev m, const KeyRec* __restrict__ keys, uint64_t n, BkEntry* __restrict__ mk, const uint32_t* __restrict__ off,
                                                   uint32_t nbm, uint32_t* __restrict__ mcur) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const KeyRec kr = keys[i];
        if (kr.code >> 46) continue;
        uint64_t w0, w1, w2, a, b, c;
        ascii23_of_rc(revcomp(kr.code, 23), w0, w1, w2);
        jenkins23(w0, w1, w2, m.seed, a, b, c);
        if (mphf_from_hash(m, a, b, c) != i) continue;
        const uint32_t home = mk_home(minimizer23(kr.code, revcomp(kr.code, 23)), nbm);
        BkEntry e;
        e.code_lo = (uint32_t)kr.code; e.code_hi = (uint32_t)(kr.code >> 32); e.tf = kr.tf; e.slot = (uint32_t)i;
        mk[(uint64_t)off[home] + atomicAdd(&mcur[home], 1u)] = e;
    }
}
__global__ void __launch_bounds__(kBlock) k_side_count(const uint32_t* __restrict__ side, uint64_t n, uint32_t* __restrict__ counter) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    uint32_t c = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) c += side[i] == 0xFFFFFFFFu ? 1u : 0u;
    if (c) atomicAdd(counter, c);
}
__global__ void __launch_bounds__(kBlock) k_side_unfiled(const KeyRec* __restrict__ keys, uint64_t n, uint32_t* __restrict__ side, KeyRec* __restrict__ unfiled,
                                                        uint32_t* __restrict__ counter) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        if (side[i] != 0xFFFFFFFFu) continue;
        const uint32_t idx = atomicAdd(counter, 1u);
        unfiled[idx] = keys[i];
        side[i] = AIX_SIDE_UNFILED | idx;
    }
}
__global__ void __launch_bounds__(kBlock) k_bk_flag(BkEntry* __restrict__ bk, uint32_t nb, const uint32_t* __restrict__ fill) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t bi = (uint64_t)blockIdx.x * kBlock + threadIdx.x; bi < nb; bi += stride)
        if (fill[bi] > 8u) bk[bi * 8 + 7].code_hi |= AIX_BK_OVERFLOW;
}

// I1 (hash.cpp:671-723): checker[h] = code, tf[h] = count with h = mphf(key). Keys arrive either as
// n x 23 ASCII bytes (the .dat lines) or as 2-bit codes. A slot hit twice raises `conflict`
// (the reference detects it only when the earlier tf was non-zero, then exit(12)).
template <bool ASCII>
__global__ void __launch_bounds__(kBlock) k_scatter23(const MphfDev m, uint64_t n, uint64_t nslots, const uint8_t* __restrict__ keys, const uint64_t* __restrict__ codes,
                                                     const uint32_t* __restrict__ counts, uint64_t* __restrict__ checker, uint32_t* __restrict__ tf,
                                                     uint32_t* __restrict__ occupied, uint32_t* __restrict__ conflict) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        uint64_t w0, w1, w2, code;
        if (ASCII) {
            load23(keys + 23 * i, w0, w1, w2);
            code = encode23_words(w0, w1, w2).code;                 // get_dna23_bitset(kmer), hash.cpp:715
        } else {
            code = codes[i] & ((1ULL << 46) - 1);
            ascii23_of_rc(revcomp(code, 23), w0, w1, w2);
        }
        uint64_t a, b, c;
        jenkins23(w0, w1, w2, m.seed, a, b, c);
        const uint64_t h = mphf_from_hash(m, a, b, c);
        if (h >= nslots) { atomicAdd(conflict, 1u); continue; }
        const uint32_t bit = 1u << (h & 31);
        if (atomicOr(&occupied[h >> 5], bit) & bit) { atomicAdd(conflict, 1u); continue; }
        checker[h] = code;
        tf[h] = counts ? counts[i] : 0u;
    }
}

// perm[code] = mphf13(ASCII(code)) for all 4^13 codes
__global__ void __launch_bounds__(kBlock) k_perm13(const MphfDev m, uint32_t* __restrict__ perm) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t code = (uint64_t)blockIdx.x * kBlock + threadIdx.x; code < 67108864ull; code += stride) {
        uint64_t w0, w1, a, b, c;
        ascii13_of_rc((uint32_t)revcomp(code, 13), w0, w1);
        jenkins13(w0, w1, m.seed, a, b, c);
        perm[code] = (uint32_t)mphf_from_hash(m, a, b, c);
    }
}
__global__ void __launch_bounds__(kBlock) k_tf13_to_code(const uint32_t* __restrict__ perm, const uint64_t* __restrict__ tf_mphf, uint64_t* __restrict__ tf_code) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t code = (uint64_t)blockIdx.x * kBlock + threadIdx.x; code < 67108864ull; code += stride) {
        const uint32_t h = perm[code];
        tf_code[code] = h < 67108864u ? tf_mphf[h] : 0ull;
    }
}
// is code -> slot a bijection of [0, 4^13)? every slot in range and claimed once (bits: 4^13 / 32 zeroed words)
__global__ void __launch_bounds__(kBlock) k_perm13_check(const uint32_t* __restrict__ perm, uint32_t* __restrict__ bits, uint32_t* __restrict__ bad) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    uint32_t b = 0;
    for (uint64_t code = (uint64_t)blockIdx.x * kBlock + threadIdx.x; code < 67108864ull; code += stride) {
        const uint32_t h = perm[code];
        if (h >= 67108864u) { b = 1; continue; }
        const uint32_t bit = 1u << (h & 31);
        if (atomicOr(&bits[h >> 5], bit) & bit) b = 1;
    }
    if (__any(b) && (threadIdx.x & 63) == 0) atomicAdd(bad, 1u);
}

// The two launchers that enqueue more than one kernel: asynchronous on `s`, one hipGetLastError() at the end.
// fp nibbles of the MPHF records (do_fp) and / or the presence masks of the early-exit table (ee_rw non-null, initialised here); keys through key_at(ix, .)
static hipError_t launch_set_fingerprints(const IndexDev& ix, BvRec* recs_rw, EeRec* ee_rw, bool do_fp, hipStream_t s) {
    if (ix.n == 0) return hipSuccess;
    if (ee_rw) hipLaunchKernelGGL(k_init_ee, dim3(grid_for(ix.m.nrecs)), dim3(kBlock), 0, s, (const BvRec*)recs_rw, ix.m.nrecs, ee_rw);
    return launch_flat(k_set_fp, ix.n, s, ix, recs_rw, ee_rw, do_fp ? 1 : 0);
}
// verification table: bk (nb * 8 entries) is initialised and filled from the keys that sit in their own MPHF slot; fill = nb zeroed u32 counters
// (scratch); bloom = zeroed, nullable; nbm = 0: no minimizer-keyed copy, else mfill = nbm zeroed words that take the keys per minimizer bucket;
// side = n words: entry index of every filed key, 0xFFFFFFFF for the others
static hipError_t launch_build_buckets(const MphfDev& m, const KeyRec* keys, uint64_t n, BkEntry* bk, uint32_t nb, uint32_t* fill, uint64_t* bloom, uint32_t nbloom, uint32_t nbm,
                                       uint32_t* mfill, uint32_t* side, hipStream_t s) {
    if (n == 0 || nb == 0) return hipSuccess;
    hipLaunchKernelGGL(k_bk_init, dim3(grid_for((uint64_t)nb * 8)), dim3(kBlock), 0, s, bk, (uint64_t)nb * 8);
    hipLaunchKernelGGL(k_bk_fill, dim3(grid_for(n)), dim3(kBlock), 0, s, m, keys, n, bk, nb, fill, bloom, nbloom, nbm, mfill, side);
    return launch_flat(k_bk_flag, nb, s, bk, nb, (const uint32_t*)fill);
}

}  // namespace aix

// ---------------------------------------------------------------------------------------------
// files
// ---------------------------------------------------------------------------------------------
struct MappedFile {
    const uint8_t* p = nullptr;
    uint64_t len = 0;
    int open(const char* path) {
        int fd = ::open(path, O_RDONLY);
        if (fd < 0) return AIX_ERR_IO;
        struct stat st;
        if (fstat(fd, &st) != 0) { ::close(fd); return AIX_ERR_IO; }
        len = (uint64_t)st.st_size;
        if (len) {
            void* m = mmap(nullptr, len, PROT_READ, MAP_PRIVATE, fd, 0);
            if (m == MAP_FAILED) { ::close(fd); return AIX_ERR_IO; }
            p = (const uint8_t*)m;
        }
        ::close(fd);
        return AIX_OK;
    }
    ~MappedFile() { if (p) munmap((void*)p, len); }
};

// .pf header checks shared by every entry point that takes a .pf image (host only)
extern "C" int aix_pf_check(const void* pf_bytes, uint64_t pf_len, uint64_t hdr_out[4]) {
    if (!pf_bytes) return AIX_ERR_ARG;
    if (pf_len < 32) return AIX_ERR_FORMAT;
    uint64_t hdr[4];
    memcpy(hdr, pf_bytes, 32);
    const uint64_t n = hdr[0], D = hdr[1], B = hdr[3];
    // mphf.hpp:26,99-113: B = 3 * hash_domain bit-pairs. A header whose product wraps (D = 0x5555555555555556, B = 2) or whose
    // domain needs more than 32-bit node ids (the builder's own limit) would index the record table far out of bounds on the
    // device, so it is refused here, before anything is uploaded.
    // (D = 0 is the MPHF of an empty key set: mphf.hpp:26 gives (ceil(0 * 1.23) + 2) / 3 = 0; nothing is ever evaluated on it.)
    if (D > 0xFFFFFFFFull / 3) return AIX_ERR_FORMAT;
    if (B != 3 * D) return AIX_ERR_FORMAT;
    if (n > B) return AIX_ERR_FORMAT;
    const uint64_t W = (B + 31) / 32, R = (B + 511) / 512;
    if (pf_len < 32 + 8 * (W + R)) return AIX_ERR_FORMAT;
    if (hdr_out) memcpy(hdr_out, hdr, 32);
    return AIX_OK;
}

// parse a .pf image (mphf.hpp:99-113) and lay it out as BvRec records in HBM
static int upload_mphf(MphfImage* img, const uint8_t* pf, uint64_t len) {
    uint64_t hdr[4];
    const int chk = aix_pf_check(pf, len, hdr);
    if (chk) return chk;
    img->mphf_n = hdr[0]; img->D = hdr[1]; img->seed = hdr[2]; img->B = hdr[3];
    img->W = (img->B + 31) / 32;
    if (img->mphf_n >> 32) return AIX_ERR_UNSUPPORTED;        // 32-bit rank prefixes
    const uint64_t* words = (const uint64_t*)(pf + 32);
    const uint64_t nrec = (img->B + 15) / 16;                    // two records per 64-bit word
    std::vector<BvRec> recs;
    try { recs.resize(nrec ? nrec : 1); } catch (const std::bad_alloc&) { return AIX_ERR_NOMEM; }
    uint64_t run = 0;
    for (uint64_t i = 0; i < nrec; ++i) {
        uint64_t w;
        memcpy(&w, words + (i >> 1), 8);
        const uint32_t half = (uint32_t)(w >> (32 * (i & 1)));
        recs[i].pairs = half;
        recs[i].prefix = (uint32_t)run;
        recs[i].fp = 0;
        run += (uint32_t)__builtin_popcount((half | (half >> 1)) & 0x55555555u);
    }
    if (run >> 32) return AIX_ERR_UNSUPPORTED;
    const uint64_t bytes = sizeof(BvRec) * recs.size();
    HIPCHK(img->recs.alloc(bytes));
    HIPCHK(hipMemcpy(img->recs.p, recs.data(), bytes, hipMemcpyHostToDevice));
    return AIX_OK;
}

int check_device(int device) {
    int c = 0;
    int st = aix_device_count(&c);
    if (st) return st;
    if (device < 0 || device >= c) return AIX_ERR_ARG;
    return AIX_OK;
}

// Verification table: n / load buckets of one 128-byte line. AIX_BUCKET_LOAD = mean keys per 8-entry bucket
// (default 4: 32 B of HBM per key, 2 % of the buckets overflow and 0.4 % of the keys stay with the MPHF path);
// AIX_BUCKET_TABLE=0 skips it (every probe through the MPHF records + key records, as in round 1).
static int build_bucket_table(aix_index* h, hipStream_t s) {
    if (h->n == 0) return AIX_OK;
    if (!env_bucket_table()) return AIX_OK;
    const double load = env_double("AIX_BUCKET_LOAD", 0.25, 8.0, 4.0);
    const long lanes = env_int("AIX_BUCKET_LANES", 1, 8, 0);
    if (lanes == 1 || lanes == 2 || lanes == 4 || lanes == 8) { h->bk_lpp = (uint32_t)lanes; h->bk_lpp_set = true; }
    uint64_t nb = (uint64_t)((double)h->n / load) + 1;
    if (nb > 0x0FFFFFF0ull) nb = 0x0FFFFFF0ull;                                // entry indices (8 per bucket) share a word with the "unfiled" flag of the side index
    const uint64_t bytes = nb * 8 * sizeof(BkEntry);
    DevBuf fill(s);
    HIPCHK(fill.alloc_once(4 * nb));
    {
        HBlock table;
        HIPCHK(table.alloc(bytes));
        h->bk.attach_owned(std::move(table));
    }
    h->nb = (uint32_t)nb;
    HIPCHK(hipMemsetAsync(fill.p, 0, 4 * nb, s));
    // absence filter: AIX_BLOOM_BITS bits per key (default 16: 2 B of Infinity-Cache-resident filter per key, < 1 % of the absent
    // keys pass; 0 = no filter)
    double bloom_bits = env_double("AIX_BLOOM_BITS", 0.0, 64.0, 16.0);
    if (bloom_bits > 0.0 && bloom_bits < 4.0) bloom_bits = 16.0;
    if (bloom_bits > 0) {
        uint64_t nw = (uint64_t)((double)h->n * bloom_bits / 64.0) + 1;
        if (nw > 0xFFFFFFF0ull) nw = 0xFFFFFFF0ull;
        HIPCHK(h->bloom.alloc(8 * nw));
        h->nbloom = (uint32_t)nw;
        HIPCHK(hipMemsetAsync(h->bloom.p, 0, 8 * nw, s));
    }
    // minimizer-keyed copy for the streaming counter (aix_stream23.hip): built only on request (AIX_MINIMIZER_TABLE=1). Every filed key
    // once more, grouped by the bucket of its minimizer (offsets + entries: a bucket is as long as its content, 16 B per key + 4 B per
    // bucket); AIX_MINIMIZER_LOAD = mean keys per bucket (default 2: the offsets of 5e7 keys are 100 MB, Infinity-Cache sized).
    const bool want_mk = env_bool("AIX_MINIMIZER_TABLE", false);
    uint64_t nbm = 0;
    if (want_mk) {
        const double mload = env_double("AIX_MINIMIZER_LOAD", 0.25, 16.0, 2.0);
        nbm = (uint64_t)((double)h->n / mload) + 1;
        if (nbm > 0xFFFFFFF0ull) nbm = 0xFFFFFFF0ull;
    }
    DevBuf mfill(s);
    HIPCHK(mfill.alloc_once(4 * (nbm + 1)));
    HIPCHK(hipMemsetAsync(mfill.p, 0, 4 * (nbm + 1), s));
    HIPCHK(h->side.alloc(4 * h->n));
    HIPCHK(launch_build_buckets(h->dev().m, h->keys.as<KeyRec>(), h->n, h->bk.as<BkEntry>(), h->nb, (uint32_t*)fill.p, h->bloom.as<uint64_t>(), h->nbloom, (uint32_t)nbm,
                                (uint32_t*)mfill.p, h->side.as<uint32_t>(), s));
    h->mk_cap = (uint32_t)env_int("AIX_MINIMIZER_CAP", 1, AIX_MK_ENTRIES, AIX_MK_ENTRIES);   // test hook: short buckets -> many undecided windows
    if (want_mk) {
        // offsets = exclusive scan of the bucket sizes (a bucket holds < 2^32 keys in total: n < 2^32), then the entries
        HIPCHK(h->mk_off.alloc(4 * (nbm + 1)));
        HIPCHK(exclusive_scan_u32((const uint32_t*)mfill.p, h->mk_off.as<uint32_t>(), nbm + 1, s));
        uint32_t filed = 0;
        HIPCHK(hipMemcpyAsync(&filed, h->mk_off.as<uint32_t>() + nbm, 4, hipMemcpyDeviceToHost, s));
        // keys the streaming counter cannot answer from their bucket (longer than the cap): host side, once per open
        std::vector<uint32_t> mf;
        try { mf.resize(nbm); } catch (const std::bad_alloc&) { return AIX_ERR_NOMEM; }
        HIPCHK(hipMemcpyAsync(mf.data(), mfill.p, 4 * nbm, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        uint64_t left = 0;
        for (uint64_t i = 0; i < nbm; ++i) if (mf[i] > h->mk_cap) left += mf[i];
        h->mk_unfiled = left;
        HIPCHK(h->mk.alloc((uint64_t)(filed ? filed : 1) * sizeof(BkEntry), (uint64_t)filed * sizeof(BkEntry)));
        h->nbm = (uint32_t)nbm;
        HIPCHK(hipMemsetAsync(mfill.p, 0, 4 * (nbm + 1), s));
        // second pass of the minimizer-keyed copy: entries written at mk[off[bucket] + arrival]; mfill = nbm zeroed words again (n and nbm are not 0 here)
        HIPCHK(launch_flat(k_mk_fill, h->n, s, h->dev().m, h->keys.as<KeyRec>(), h->n, h->mk.as<BkEntry>(), h->mk_off.as<uint32_t>(), h->nbm, (uint32_t*)mfill.p));
        HIPCHK(hipStreamSynchronize(s));
    }
    // keys left to the MPHF path: sum over buckets of max(fill - 8, 0) (host side: once per open, nb words)
    std::vector<uint32_t> f;
    try { f.resize(nb); } catch (const std::bad_alloc&) { return AIX_ERR_NOMEM; }
    HIPCHK(hipMemcpyAsync(f.data(), fill.p, 4 * nb, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    uint64_t unfiled = 0;
    for (uint64_t i = 0; i < nb; ++i) if (f[i] > 8) unfiled += f[i] - 8;
    h->bk_unfiled = unfiled;
    // The keys the table does not hold (beyond the eighth of their bucket, or not in their own MPHF slot) are closed up into `unfiled`; with
    // the side index every slot's {code, tf} is then reachable without the 16 B-per-key record array, which goes back to the driver.
    {
        DevBuf cnt(s);
        HIPCHK(cnt.alloc_once(8));
        HIPCHK(hipMemsetAsync(cnt.p, 0, 8, s));
        HIPCHK(launch_flat(k_side_count, h->n, s, h->side.as<uint32_t>(), h->n, (uint32_t*)cnt.p));
        uint32_t nu = 0;
        HIPCHK(hipMemcpyAsync(&nu, cnt.p, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        HIPCHK(h->unfiled.alloc(sizeof(KeyRec) * (uint64_t)(nu ? nu : 1), sizeof(KeyRec) * (uint64_t)nu));
        h->n_unfiled = nu;
        // unfiled[idx] = keys[i], side[i] = AIX_SIDE_UNFILED | idx for every side[i] == 0xFFFFFFFF; the counter is the second, still zeroed word
        HIPCHK(launch_flat(k_side_unfiled, h->n, s, h->keys.as<KeyRec>(), h->n, h->side.as<uint32_t>(), h->unfiled.as<KeyRec>(), (uint32_t*)cnt.p + 1));
        HIPCHK(hipStreamSynchronize(s));
    }
    return AIX_OK;
}

// presence masks of the early-exit MPHF walk (aix_device.hpp: EeRec), from the handle's keys
static int build_early_exit_table(aix_index* h, hipStream_t s) {
    if (h->ee || h->n == 0) return AIX_OK;
    const uint64_t nrec = (h->mphf.B + 15) / 16;
    HBlock ee;                                                                  // not visible to dev() until it is complete
    HIPCHK(ee.alloc(sizeof(EeRec) * (nrec ? nrec : 1), sizeof(EeRec) * nrec));
    const hipError_t e = launch_set_fingerprints(h->dev(), h->mphf.recs.as<BvRec>(), ee.as<EeRec>(), false, s);
    const hipError_t e2 = hipStreamSynchronize(s);
    h->ee = std::move(ee);
    HIPCHK(e);
    HIPCHK(e2);
    return AIX_OK;
}

// interleave device-resident checker[]/tf[] into KeyRec records and detect an all-canonical key set
static int adopt_device_arrays(aix_index* h, const uint64_t* d_checker, const uint32_t* d_tf, uint64_t n, hipStream_t s) {
    if (n == 0) return AIX_OK;
    HIPCHK(h->keys.alloc(sizeof(KeyRec) * n));
    uint32_t flag = 1;
    {
        DevBuf d_flag(s);
        HIPCHK(d_flag.alloc_once(4));
        HIPCHK(hipMemsetAsync(d_flag.p, 0, 4, s));
        HIPCHK(launch_flat(k_build_keyrecs, n, s, d_checker, d_tf, n, h->keys.as<KeyRec>(), (uint32_t*)d_flag.p));
        HIPCHK(hipMemcpyAsync(&flag, d_flag.p, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    h->canonical_only = (flag == 0);
    // The early-exit table (32 B per 16 bit-pairs: 2.5 B per key) serves the MPHF walk; with a verification table in front that walk only runs
    // behind overflowed buckets, so the table is then built on request (aix_index_set_early_exit) instead of at every open.
    if (!env_bucket_table()) { const int st = build_early_exit_table(h, s); if (st) return st; }
    HIPCHK(launch_set_fingerprints(h->dev(), h->mphf.recs.as<BvRec>(), nullptr, true, s));
    HIPCHK(hipStreamSynchronize(s));
    h->has_fp = true;
    const int st = build_bucket_table(h, s);
    if (st) return st;
    if (h->bk.p && h->side) h->keys.drop();                                     // every key is reachable through the table / the unfiled list: drop the duplicate
    return AIX_OK;
}

extern "C" int aix_index_create_23(const void* pf_bytes, uint64_t pf_len, const uint64_t* checker, const uint32_t* tf, uint64_t n, int device,
                                   aix_index_t** out) {
    if (!pf_bytes || !out || (n && (!checker || !tf))) return AIX_ERR_ARG;
    *out = nullptr;
    int st = check_device(device);
    if (st) return st;
    if (n >> 32) return AIX_ERR_UNSUPPORTED;
    HandlePtr h(new (std::nothrow) aix_index());
    if (!h) return AIX_ERR_NOMEM;
    h->device = device; h->k = 23; h->n = n;
    DevGuard g(device);
    st = upload_mphf(&h->mphf, (const uint8_t*)pf_bytes, pf_len);
    if (!st && n) {
        DevBuf dc, dt;
        hipError_t e = dc.alloc_once(8 * n);
        if (e == hipSuccess) e = dt.alloc_once(4 * n);
        if (e == hipSuccess) e = hipMemcpy(dc.p, checker, 8 * n, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(dt.p, tf, 4 * n, hipMemcpyHostToDevice);
        if (e != hipSuccess) { set_last_error(std::string("index upload: ") + hipGetErrorString(e)); st = AIX_ERR_HIP; }
        else st = adopt_device_arrays(h.get(), (const uint64_t*)dc.p, (const uint32_t*)dt.p, n, 0);
    }
    if (st) return st;
    *out = h.release();
    return AIX_OK;
}

// I1 on the device: scatter (key, count) pairs through the MPHF. Exactly one of d_keys / d_codes is set.
// n keys into nslots slots (nslots == n for a whole key set; a shard of the keys scatters into the full-size arrays).
// occ_out (optional, device, ceil(nslots/32) words): bit h set <=> slot h was written by this call.
static int scatter_device(const MphfImage& mphf, uint64_t n, uint64_t nslots, const uint8_t* d_keys, const uint64_t* d_codes, const uint32_t* d_counts,
                          uint64_t* d_checker, uint32_t* d_tf, uint32_t* occ_out, hipStream_t s) {
    DevBuf occ(s), flag(s);
    const uint64_t occ_bytes = 4 * ((nslots + 31) / 32);
    HIPCHK(occ.alloc(occ_bytes));
    HIPCHK(flag.alloc(4));
    HIPCHK(hipMemsetAsync(occ.p, 0, occ_bytes, s));
    HIPCHK(hipMemsetAsync(flag.p, 0, 4, s));
    HIPCHK(hipMemsetAsync(d_checker, 0, 8 * nslots, s));       // hash.cpp:836-844: arrays start zeroed
    HIPCHK(hipMemsetAsync(d_tf, 0, 4 * nslots, s));
    if (n) HIPCHK(d_keys ? launch_flat(k_scatter23<true>, n, s, mphf.view(), n, nslots, d_keys, d_codes, d_counts, d_checker, d_tf, (uint32_t*)occ.p, (uint32_t*)flag.p)
                         : launch_flat(k_scatter23<false>, n, s, mphf.view(), n, nslots, d_keys, d_codes, d_counts, d_checker, d_tf, (uint32_t*)occ.p, (uint32_t*)flag.p));
    uint32_t conflicts = 0;
    HIPCHK(hipMemcpyAsync(&conflicts, flag.p, 4, hipMemcpyDeviceToHost, s));
    if (occ_out) HIPCHK(hipMemcpyAsync(occ_out, occ.p, occ_bytes, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    return conflicts ? AIX_ERR_CONFLICT : AIX_OK;
}

static int scatter_host(const void* pf_bytes, uint64_t pf_len, const char* keys, const uint32_t* counts, uint64_t n, uint64_t nslots, int device,
                        uint64_t* checker_out, uint32_t* tf_out, uint32_t* occupied_out) {
    int st = check_device(device);
    if (st) return st;
    DevGuard g(device);
    MphfImage mphf;                                                // declared behind the guard: freed on `device`
    st = upload_mphf(&mphf, (const uint8_t*)pf_bytes, pf_len);
    if (!st) {
        DevBuf dk, dcnt, dc, dt, docc;
        const uint64_t occ_bytes = 4 * ((nslots + 31) / 32);
        hipError_t e = dk.alloc(23 * n + 8);
        if (e == hipSuccess) e = dc.alloc(8 * nslots);
        if (e == hipSuccess) e = dt.alloc(4 * nslots);
        if (e == hipSuccess && occupied_out) e = docc.alloc(occ_bytes);
        if (e == hipSuccess && counts && n) e = dcnt.alloc(4 * n);
        if (e == hipSuccess && n) e = hipMemcpy(dk.p, keys, 23 * n, hipMemcpyHostToDevice);
        if (e == hipSuccess && counts && n) e = hipMemcpy(dcnt.p, counts, 4 * n, hipMemcpyHostToDevice);
        if (e != hipSuccess) { set_last_error(std::string("scatter staging: ") + hipGetErrorString(e)); st = AIX_ERR_HIP; }
        if (!st) st = scatter_device(mphf, n, nslots, (const uint8_t*)dk.p, nullptr, (counts && n) ? (const uint32_t*)dcnt.p : nullptr, (uint64_t*)dc.p,
                                     (uint32_t*)dt.p, occupied_out ? (uint32_t*)docc.p : nullptr, 0);
        if (!st || st == AIX_ERR_CONFLICT) {                       // a shard reports its conflict AND hands back what it wrote
            const int keep = st;
            e = hipMemcpy(checker_out, dc.p, 8 * nslots, hipMemcpyDeviceToHost);
            if (e == hipSuccess) e = hipMemcpy(tf_out, dt.p, 4 * nslots, hipMemcpyDeviceToHost);
            if (e == hipSuccess && occupied_out) e = hipMemcpy(occupied_out, docc.p, occ_bytes, hipMemcpyDeviceToHost);
            if (e != hipSuccess) { set_last_error(std::string("scatter readback: ") + hipGetErrorString(e)); st = AIX_ERR_HIP; }
            else st = keep;
        }
    }
    return st;
}

extern "C" int aix_index_scatter(const void* pf_bytes, uint64_t pf_len, const char* keys, const uint32_t* counts, uint64_t n, int device,
                                 uint64_t* checker_out, uint32_t* tf_out) {
    if (!pf_bytes || !keys || !checker_out || !tf_out || n == 0) return AIX_ERR_ARG;
    return scatter_host(pf_bytes, pf_len, keys, counts, n, n, device, checker_out, tf_out, nullptr);
}

extern "C" int aix_index_scatter_shard(const void* pf_bytes, uint64_t pf_len, const char* keys, const uint32_t* counts, uint64_t n_keys, uint64_t n_slots,
                                       int device, uint64_t* checker_out, uint32_t* tf_out, uint32_t* occupied_out) {
    if (!pf_bytes || (n_keys && !keys) || !checker_out || !tf_out || !occupied_out || n_slots == 0 || n_keys > n_slots) return AIX_ERR_ARG;
    if (n_slots >> 32) return AIX_ERR_UNSUPPORTED;
    return scatter_host(pf_bytes, pf_len, keys, counts, n_keys, n_slots, device, checker_out, tf_out, occupied_out);
}

extern "C" int aix_index_build_23_codes_dev(const void* pf_bytes, uint64_t pf_len, const uint64_t* d_codes, const uint32_t* d_counts, uint64_t n,
                                            int device, void* stream, aix_index_t** out) {
    if (!pf_bytes || !d_codes || !out || n == 0) return AIX_ERR_ARG;
    *out = nullptr;
    int st = check_device(device);
    if (st) return st;
    if (n >> 32) return AIX_ERR_UNSUPPORTED;
    HandlePtr h(new (std::nothrow) aix_index());
    if (!h) return AIX_ERR_NOMEM;
    h->device = device; h->k = 23; h->n = n;
    DevGuard g(device);
    st = upload_mphf(&h->mphf, (const uint8_t*)pf_bytes, pf_len);
    if (!st) {
        DevBuf dc((hipStream_t)stream), dt((hipStream_t)stream);
        hipError_t e = dc.alloc(8 * n);
        if (e == hipSuccess) e = dt.alloc(4 * n);
        if (e != hipSuccess) { set_last_error(std::string("index build: ") + hipGetErrorString(e)); st = AIX_ERR_HIP; }
        if (!st) st = scatter_device(h->mphf, n, n, nullptr, d_codes, d_counts, (uint64_t*)dc.p, (uint32_t*)dt.p, nullptr, (hipStream_t)stream);
        if (!st) st = adopt_device_arrays(h.get(), (const uint64_t*)dc.p, (const uint32_t*)dt.p, n, (hipStream_t)stream);
    }
    if (st) return st;
    *out = h.release();
    return AIX_OK;
}

extern "C" int aix_index_open_23(const char* pf, const char* tf_bin, const char* kmers_bin, int device, aix_index_t** out) {
    if (!pf || !tf_bin || !kmers_bin || !out) return AIX_ERR_ARG;
    MappedFile fpf, ftf, fk;
    if (fpf.open(pf) || ftf.open(tf_bin) || fk.open(kmers_bin)) return AIX_ERR_IO;
    const uint64_t n = fk.len / 8;                              // hash.cpp:393-397: n = size(.kmers.bin)/8
    std::vector<uint32_t> tfpad;
    const uint32_t* tfp = (const uint32_t*)ftf.p;
    if (ftf.len / 4 < n) {                                      // hash.cpp:431-444 reads until EOF; rest stays 0
        tfpad.assign(n, 0);
        memcpy(tfpad.data(), ftf.p, (ftf.len / 4) * 4);
        tfp = tfpad.data();
    }
    return aix_index_create_23(fpf.p, fpf.len, (const uint64_t*)fk.p, tfp, n, device, out);
}

static int build_13_tables(aix_index* h, const uint64_t* tf_host) {
    const uint64_t N13 = AIX_TOTAL_13MERS;
    HIPCHK(h->tf13_mphf.alloc(8 * N13));
    HIPCHK(h->tf13_code.alloc(8 * N13));
    HIPCHK(h->perm13.alloc(4 * N13));
    const IndexDev d = h->dev();
    if (tf_host) HIPCHK(hipMemcpy(h->tf13_mphf.p, tf_host, 8 * N13, hipMemcpyHostToDevice));
    else HIPCHK(hipMemset(h->tf13_mphf.p, 0, 8 * N13));
    HIPCHK(launch_flat(k_perm13, N13, 0, d.m, h->perm13.as<uint32_t>()));              // perm[code] = mphf slot
    HIPCHK(launch_flat(k_tf13_to_code, N13, 0, d.perm13, d.tf13_mphf, h->tf13_code.as<uint64_t>()));
    // The streaming counter writes each bin's total to out[perm[code]] with a plain store: right only when code -> slot is a
    // bijection, which holds for the all-13-mers .pf and not for a foreign one. Checked once here; a handle that fails the check
    // counts through the atomics path, which adds (the reference's fetch_add at mphf(window), count_kmers13.cpp:147-152).
    {
        DevBuf bits, bad;
        HIPCHK(bits.alloc_once(AIX_TOTAL_13MERS / 8));
        HIPCHK(bad.alloc_once(4));
        HIPCHK(hipMemsetAsync(bits.p, 0, AIX_TOTAL_13MERS / 8, 0));
        HIPCHK(hipMemsetAsync(bad.p, 0, 4, 0));
        HIPCHK(launch_flat(k_perm13_check, N13, 0, d.perm13, (uint32_t*)bits.p, (uint32_t*)bad.p));
        uint32_t nbad = 1;
        HIPCHK(hipMemcpy(&nbad, bad.p, 4, hipMemcpyDeviceToHost));
        h->perm13_bijective = (nbad == 0);
    }
    HIPCHK(hipStreamSynchronize(0));
    return AIX_OK;
}

extern "C" int aix_index_create_13(const void* pf_bytes, uint64_t pf_len, const uint64_t* tf, int device, aix_index_t** out) {
    if (!pf_bytes || !out) return AIX_ERR_ARG;
    *out = nullptr;
    int st = check_device(device);
    if (st) return st;
    HandlePtr h(new (std::nothrow) aix_index());
    if (!h) return AIX_ERR_NOMEM;
    h->device = device; h->k = 13; h->n = AIX_TOTAL_13MERS;
    DevGuard g(device);
    st = upload_mphf(&h->mphf, (const uint8_t*)pf_bytes, pf_len);
    if (!st) st = build_13_tables(h.get(), tf);
    if (st) return st;
    *out = h.release();
    return AIX_OK;
}

extern "C" int aix_index_open_13(const char* pf, const char* tf_bin, int device, aix_index_t** out) {
    if (!pf || !out) return AIX_ERR_ARG;
    MappedFile fpf, ftf;
    if (fpf.open(pf)) return AIX_ERR_IO;
    const uint64_t* tf = nullptr;
    if (tf_bin) {
        if (ftf.open(tf_bin)) return AIX_ERR_IO;
        if (ftf.len < 8 * AIX_TOTAL_13MERS) return AIX_ERR_FORMAT;   // reference mmaps 4^13*8 bytes (:425)
        tf = (const uint64_t*)ftf.p;
    }
    return aix_index_create_13(fpf.p, fpf.len, tf, device, out);
}

extern "C" int aix_index_close(aix_index_t* h) {
    if (!h) return AIX_ERR_ARG;
    HandleDelete()(h);                // every owner on the handle releases what it holds, on the handle's device
    pool_trim();                      // scratch blocks cached for this handle's calls go back to the driver with it
    return AIX_OK;
}

extern "C" int aix_index_info(const aix_index_t* h, aix_info_t* info) {
    if (!h || !info) return AIX_ERR_ARG;
    memset(info, 0, sizeof(*info));
    info->k = h->k; info->device = (uint32_t)h->device; info->n = h->n; info->mphf_n = h->mphf.mphf_n;
    info->hash_domain = h->mphf.D; info->seed = h->mphf.seed; info->bitpairs = h->mphf.B; info->device_bytes = h->device_bytes;
    info->canonical_only = h->canonical_only ? 1 : 0;
    info->bucket_table = (h->bk.p && h->bk_enabled) ? 1 : 0;
    info->bucket_lanes = h->bk_lpp;
    info->buckets = h->bk.p ? h->nb : 0;
    info->bucket_unfiled_keys = h->bk_unfiled;
    info->absence_filter_words = (h->bk.p && h->bk_enabled && h->bloom && h->bloom_enabled) ? h->nbloom : 0;
    info->minimizer_lines = (h->bk.p && h->bk_enabled && h->mk && h->mk_enabled) ? h->nbm : 0;
    info->minimizer_unfiled_keys = h->mk_unfiled;
    info->count23_backend = h->cnt.c23_backend;
    info->count23_passes = h->cnt.c23_passes;
    info->positions_backend = h->a2_backend;
    info->aindex_attached = h->att.ai_indices.attached ? (h->att.ai_indices.owned ? 1u : 2u) : 0u;
    info->ridx_on_device = h->att.rx ? 1u : 0u;
    info->aindex_entries = h->att.ai_indices.attached ? h->att.ai_total : 0;
    info->ridx_reads = h->att.rx ? h->att.rx_n : 0;
    return AIX_OK;
}

extern "C" int aix_index_set_canonical_fastpath(aix_index_t* h, int enabled) {
    if (!h) return AIX_ERR_ARG;
    h->canonical_fastpath = enabled != 0;
    return AIX_OK;
}

extern "C" int aix_index_set_fingerprint_filter(aix_index_t* h, int enabled) {
    if (!h) return AIX_ERR_ARG;
    h->fp_filter = enabled != 0;
    return AIX_OK;
}

extern "C" int aix_index_set_early_exit(aix_index_t* h, int enabled) {
    if (!h) return AIX_ERR_ARG;
    h->early_exit = enabled != 0;
    if (enabled && h->k == 23 && h->has_fp && !h->ee) {                         // first request on a handle that was opened with a verification table
        DevGuard g(h->device);
        const int st = build_early_exit_table(h, 0);
        if (st) return st;
    }
    return AIX_OK;
}

extern "C" int aix_index_set_minimizer_table(aix_index_t* h, int enabled) {
    if (!h) return AIX_ERR_ARG;
    h->mk_enabled = enabled != 0;
    return AIX_OK;
}

extern "C" int aix_index_set_absence_filter(aix_index_t* h, int enabled) {
    if (!h) return AIX_ERR_ARG;
    h->bloom_enabled = enabled != 0;
    return AIX_OK;
}

extern "C" int aix_index_set_bucket_table(aix_index_t* h, int enabled, int lanes) {
    if (!h) return AIX_ERR_ARG;
    if (lanes != 0 && lanes != 1 && lanes != 2 && lanes != 4 && lanes != 8) return AIX_ERR_ARG;
    h->bk_enabled = enabled != 0;
    if (lanes) { h->bk_lpp = (uint32_t)lanes; h->bk_lpp_set = true; }
    return AIX_OK;
}

extern "C" int aix_index_set_tf_13(aix_index_t* h, const uint64_t* tf) {
    if (!h || !tf) return AIX_ERR_ARG;
    if (h->k != 13) return AIX_ERR_MODE;
    DevGuard g(h->device);
    HIPCHK(hipMemcpy(h->tf13_mphf.p, tf, 8 * AIX_TOTAL_13MERS, hipMemcpyHostToDevice));
    h->pos_total_known = false;
    HIPCHK(launch_flat(k_tf13_to_code, AIX_TOTAL_13MERS, 0, h->perm13.as<uint32_t>(), h->tf13_mphf.as<uint64_t>(), h->tf13_code.as<uint64_t>()));
    HIPCHK(hipStreamSynchronize(0));
    return AIX_OK;
}

extern "C" int aix_index_get_tf(const aix_index_t* h, void* out, uint64_t out_bytes) {
    if (!h || !out) return AIX_ERR_ARG;
    DevGuard g(h->device);
    if (h->k == 13) {
        if (out_bytes < 8 * AIX_TOTAL_13MERS) return AIX_ERR_ARG;
        HIPCHK(hipMemcpy(out, h->tf13_mphf.p, 8 * AIX_TOTAL_13MERS, hipMemcpyDeviceToHost));
        return AIX_OK;
    }
    if (out_bytes < 4 * h->n) return AIX_ERR_ARG;
    if (h->n == 0) return AIX_OK;
    DevBuf d;
    HIPCHK(d.alloc_once(4 * h->n));
    HIPCHK(launch_flat(k_extract, h->n, 0, h->dev(), (uint32_t*)d.p, (uint64_t*)nullptr));
    HIPCHK(hipMemcpy(out, d.p, 4 * h->n, hipMemcpyDeviceToHost));
    return AIX_OK;
}

extern "C" int aix_index_get_checker(const aix_index_t* h, uint64_t* out, uint64_t n) {
    if (!h || !out) return AIX_ERR_ARG;
    if (h->k != 23) return AIX_ERR_MODE;
    if (n < h->n) return AIX_ERR_ARG;
    if (h->n == 0) return AIX_OK;
    DevGuard g(h->device);
    DevBuf d;
    HIPCHK(d.alloc_once(8 * h->n));
    HIPCHK(launch_flat(k_extract, h->n, 0, h->dev(), (uint32_t*)nullptr, (uint64_t*)d.p));
    HIPCHK(hipMemcpy(out, d.p, 8 * h->n, hipMemcpyDeviceToHost));
    return AIX_OK;
}

// device-resident twin of aix_index_scatter_shard (multi-GPU): a rank's share of the keys is already in HBM, the partial
// arrays stay in HBM for the collectives (RCCL), nothing crosses PCIe
extern "C" int aix_index_scatter_shard_codes_dev(const void* pf_bytes, uint64_t pf_len, const uint64_t* d_codes, const uint32_t* d_counts, uint64_t n_keys,
                                                 uint64_t n_slots, int device, void* stream, uint64_t* d_checker_out, uint32_t* d_tf_out, uint32_t* d_occupied_out) {
    if (!pf_bytes || (n_keys && !d_codes) || !d_checker_out || !d_tf_out || !d_occupied_out || n_slots == 0 || n_keys > n_slots) return AIX_ERR_ARG;
    if (n_slots >> 32) return AIX_ERR_UNSUPPORTED;
    int st = check_device(device);
    if (st) return st;
    DevGuard g(device);
    MphfImage mphf;
    st = upload_mphf(&mphf, (const uint8_t*)pf_bytes, pf_len);
    if (!st) st = scatter_device(mphf, n_keys, n_slots, nullptr, d_codes, d_counts, d_checker_out, d_tf_out, d_occupied_out, (hipStream_t)stream);
    if (mphf.recs) (void)hipStreamSynchronize((hipStream_t)stream);          // the records are freed idle
    return st;
}
