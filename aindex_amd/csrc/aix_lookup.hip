// aix_lookup.hip — lookups and coverage: the device-pointer entry points, and their host-pointer twins with the two staging paths (tiny
// batches through pinned, device-mapped memory of the handle; large ones through a three-deep pipeline of pinned blocks and streams).
// No kernel lives here (aix_kernels.hip has them).
#include <algorithm>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "aix_env.hpp"
#include "aix_handle.hpp"

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
