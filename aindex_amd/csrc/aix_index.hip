// aix_index.hip — the index handle's life in HBM: .pf parsing and upload, the tables built at open (verification table, absence
// filter, minimizer-keyed copy, early-exit masks, 13-mer permutation), scatter, create / open / close / info and the setters.
// No kernel lives here (aix_kernels.hip has them).
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
        HIPCHK(launch_fill_minimizer_table(h->dev().m, h->keys.as<KeyRec>(), h->n, h->mk.as<BkEntry>(), h->mk_off.as<uint32_t>(), h->nbm, (uint32_t*)mfill.p, s));
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
        HIPCHK(launch_count_unfiled(h->side.as<uint32_t>(), h->n, (uint32_t*)cnt.p, s));
        uint32_t nu = 0;
        HIPCHK(hipMemcpyAsync(&nu, cnt.p, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        HIPCHK(h->unfiled.alloc(sizeof(KeyRec) * (uint64_t)(nu ? nu : 1), sizeof(KeyRec) * (uint64_t)nu));
        h->n_unfiled = nu;
        HIPCHK(launch_side_unfiled(h->keys.as<KeyRec>(), h->n, h->side.as<uint32_t>(), h->unfiled.as<KeyRec>(), (uint32_t*)cnt.p + 1, s));
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
        HIPCHK(launch_build_keyrecs(d_checker, d_tf, n, h->keys.as<KeyRec>(), (uint32_t*)d_flag.p, s));
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
    HIPCHK(launch_scatter23(mphf.view(), n, nslots, d_keys, d_codes, d_counts, d_checker, d_tf, (uint32_t*)occ.p, (uint32_t*)flag.p, s));
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
    HIPCHK(launch_perm13(d.m, h->perm13.as<uint32_t>(), 0));
    HIPCHK(launch_tf13_to_code_order(d.perm13, d.tf13_mphf, h->tf13_code.as<uint64_t>(), 0));
    // The streaming counter writes each bin's total to out[perm[code]] with a plain store: right only when code -> slot is a
    // bijection, which holds for the all-13-mers .pf and not for a foreign one. Checked once here; a handle that fails the check
    // counts through the atomics path, which adds (the reference's fetch_add at mphf(window), count_kmers13.cpp:147-152).
    {
        DevBuf bits, bad;
        HIPCHK(bits.alloc_once(AIX_TOTAL_13MERS / 8));
        HIPCHK(bad.alloc_once(4));
        HIPCHK(hipMemsetAsync(bits.p, 0, AIX_TOTAL_13MERS / 8, 0));
        HIPCHK(hipMemsetAsync(bad.p, 0, 4, 0));
        HIPCHK(launch_perm13_check(d.perm13, (uint32_t*)bits.p, (uint32_t*)bad.p, 0));
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
    HIPCHK(launch_tf13_to_code_order(h->perm13.as<uint32_t>(), h->tf13_mphf.as<uint64_t>(), h->tf13_code.as<uint64_t>(), 0));
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
    HIPCHK(launch_extract_tf(h->dev(), (uint32_t*)d.p, nullptr, 0));
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
    HIPCHK(launch_extract_tf(h->dev(), nullptr, (uint64_t*)d.p, 0));
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
