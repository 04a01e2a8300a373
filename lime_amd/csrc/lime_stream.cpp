// lime_stream.cpp -- the host-pointer entry points: host arrays (or mapped files) go through HBM in position-range chunks.  The two-stream
// pipeline (Pipe), the registered files, the pinned staging ring and its threads (IoPool, Feeder), lime_internal_upload, the walks of
// lime_fused_stream / lime_detect* / lime_score, and d2h_pageable for large results on their way back.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <stdio.h>
#include <errno.h>
#include <fcntl.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <sched.h>
#include <sys/stat.h>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "lime_ctx.h"

using namespace lime;
using namespace lime_host;

// ---- streaming from host memory: the collection goes through HBM in position-range chunks ------
// Chunk k owns positions [k*chunk, (k+1)*chunk) and carries a read-ahead halo, exactly like a shard of
// the multi-GPU partition (ClusterLCP.cpp:150-161,246-264); two device buffers alternate so that the
// copy of chunk k+1 runs while chunk k is scanned; all chunks add into one table in HBM.
namespace {
struct Pipe {
    hipStream_t copy = nullptr, comp = nullptr;
    hipEvent_t copied[2] = {nullptr, nullptr}, consumed[2] = {nullptr, nullptr};
    ~Pipe() {
        for (int b = 0; b < 2; ++b) { if (copied[b]) (void)hipEventDestroy(copied[b]); if (consumed[b]) (void)hipEventDestroy(consumed[b]); }
        if (copy) (void)hipStreamDestroy(copy);
        if (comp) (void)hipStreamDestroy(comp);
    }
    int init() {
        HIP_TRY(hipStreamCreateWithFlags(&copy, hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithFlags(&comp, hipStreamNonBlocking));
        for (int b = 0; b < 2; ++b) {
            HIP_TRY(hipEventCreateWithFlags(&copied[b], hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&consumed[b], hipEventDisableTiming));
        }
        return LIME_OK;
    }
};
const uint64_t STREAM_HALO = (uint64_t)LIME_MAX_CLUSTER + LIME_TILE;   // a run the reference accepts closes inside it
const uint64_t STREAM_CHUNK = 64ull << 20;                              // default symbols per chunk, sources pinned (or small)
const uint64_t STAGED_CHUNK = 4ull << 20;                               // through the pinned ring: short chunks fill the pipeline sooner and the
                                                                        // three slots stay small (measured best of 4 / 16 / 64 Mi on 10^9 symbols)
}

// ---- host arrays -> HBM, chunk by chunk ---------------------------------------------------------
// The callers' arrays are usually pageable (the drop-in programs hand over mmap-ed files): a copy straight from
// them is synchronous and staged by the runtime in small pieces.  The Feeder moves chunk k through a ring of three
// pinned slots instead: a producer thread (with LIME_IO_THREADS helpers) copies the chunk's pieces into slot k % 3
// while the copy engine empties slot (k-1) % 3 into one device buffer set and the kernels work on the other.
// Sources that are already pinned (hipHostMalloc / hipHostRegister) skip the ring.
// ---- mapped files the callers hand over as arrays (the drop-in programs): lime_register_file tells the library which file a mapping shows, and
// the staging threads then fill the pinned slots with pread() from the file -- the page cache copied by the kernel at several GB/s per thread --
// instead of memcpy from the mapping, which takes a page fault per 4 KB (16-page fault-around) of every first touch: 10.6 GB/s with 8 threads in
// round 4, a fifth of what the link takes from pinned memory.  Reference: the per-thread FILE* reads of ClusterLCP.cpp:100-123, 206-212.
namespace {
struct FileMap { const char *base; size_t bytes; int fd; };
std::mutex g_files_mu;
std::vector<FileMap> g_files;
// bytes [src, src + len) from the registered file that holds them (false: not in one -- the caller copies from memory)
bool read_from_file(void *dst, const void *src, size_t len)
{
    FileMap m{nullptr, 0, -1};
    {
        std::lock_guard<std::mutex> g(g_files_mu);
        for (const FileMap &f : g_files)
            if ((const char *)src >= f.base && (const char *)src + len <= f.base + f.bytes) { m = f; break; }
    }
    if (m.fd < 0) return false;
    size_t done = 0;
    const off_t at = (off_t)((const char *)src - m.base);
    while (done < len) {
        const ssize_t k = pread(m.fd, (char *)dst + done, len - done, at + (off_t)done);
        if (k <= 0) { if (k < 0 && errno == EINTR) continue; return false; }
        done += (size_t)k;
    }
    return true;
}
}
extern "C" int lime_register_file(const void *base, size_t bytes, int fd)
{
    if (!base || fd < 0) return fail(LIME_ERR_ARG, "lime_register_file: bad argument");
    // (the contract is in include/lime_hip.h: the mapping shows the file from offset 0, read-only; what can be checked is)
    struct stat sb;
    if (fstat(fd, &sb) != 0) return fail(LIME_ERR_IO, "lime_register_file: fstat failed");
    if ((uint64_t)bytes > (uint64_t)sb.st_size) return fail(LIME_ERR_ARG, "lime_register_file: %zu bytes registered, the file has %lld", bytes, (long long)sb.st_size);
    std::lock_guard<std::mutex> g(g_files_mu);
    for (const FileMap &f : g_files)
        if ((const char *)base < f.base + f.bytes && f.base < (const char *)base + bytes)
            return fail(LIME_ERR_ARG, "lime_register_file: the range overlaps a registered one (unregister before unmapping)");
    const int own = dup(fd);                               // the caller may close its descriptor
    if (own < 0) return fail(LIME_ERR_IO, "lime_register_file: dup failed");
    g_files.push_back(FileMap{(const char *)base, bytes, own});
    return LIME_OK;
}
extern "C" void lime_unregister_file(const void *base)
{
    std::lock_guard<std::mutex> g(g_files_mu);
    for (size_t i = 0; i < g_files.size(); ++i)
        if (g_files[i].base == (const char *)base) { close(g_files[i].fd); g_files.erase(g_files.begin() + (long)i); return; }
}

namespace {
struct Piece { const void *src; size_t bytes; void *dst; };

// a few host threads that copy (or pread) pieces of 1 MB: created once per walk, not per piece
struct IoPool {
    struct Task { void *dst; const void *src; size_t len; };
    std::vector<std::thread> th;
    std::mutex mu; std::condition_variable cv_go, cv_done;
    std::vector<Task> tasks; size_t next = 0, left = 0; bool stop = false;
    void start(int n)
    {
        for (int t = 0; t < n; ++t)
            th.emplace_back([this]() {
                for (;;) {
                    Task k;
                    {
                        std::unique_lock<std::mutex> lk(mu);
                        cv_go.wait(lk, [&] { return stop || next < tasks.size(); });
                        if (stop) return;
                        k = tasks[next++];
                    }
                    if (!read_from_file(k.dst, k.src, k.len)) memcpy(k.dst, k.src, k.len);
                    { std::lock_guard<std::mutex> g(mu); if (--left == 0) cv_done.notify_all(); }
                }
            });
    }
    void run(std::vector<Task> &&t)                        // returns when every task is done
    {
        if (t.empty()) return;
        if (th.empty()) { for (const Task &k : t) if (!read_from_file(k.dst, k.src, k.len)) memcpy(k.dst, k.src, k.len); return; }
        std::unique_lock<std::mutex> lk(mu);
        tasks = std::move(t); next = 0; left = tasks.size();
        cv_go.notify_all();
        cv_done.wait(lk, [&] { return left == 0; });
        tasks.clear(); next = 0;
    }
    ~IoPool()
    {
        { std::lock_guard<std::mutex> g(mu); stop = true; }
        cv_go.notify_all();
        for (auto &t : th) t.join();
    }
};

// host threads that move pageable sources into the pinned ring: what the ctx says (lime_set_option "io_threads": the drop-in programs pass the
// reference's `threads` argument, LIME_IO_THREADS overrides at lime_init), else 8; never more than the CPUs this process may run on (its
// affinity mask: a cgroup- or taskset-limited job must not be oversubscribed -- ADVICE r5)
static int staging_threads(const lime_ctx *c)
{
    int t = c && c->io_threads > 0 ? c->io_threads : 8;
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0) { const int n = CPU_COUNT(&set); if (n >= 1 && t > n) t = n; }
    else { const unsigned hw = std::thread::hardware_concurrency(); if (hw && (unsigned)t > hw) t = (int)hw; }
    return t < 1 ? 1 : t;
}

struct Feeder {
    static constexpr int NS = 3, MAXP = 3;
    void *slot[NS] = {nullptr, nullptr, nullptr};
    hipEvent_t h2d_done[NS] = {nullptr, nullptr, nullptr};
    size_t slot_bytes = 0;
    bool staged = false;
    int io_threads = 1, device = 0;
    uint64_t n_chunks = 0;
    std::function<int(uint64_t, Piece *)> describe;       // pieces of chunk k (at most MAXP); returns their number
    std::thread producer;
    std::mutex mu; std::condition_variable cv;
    uint64_t filled = 0, issued = 0; bool stop = false, failed = false;

    // would a walk over `total_bytes` of these sources go through the ring?  (the caller picks its chunk size by it)
    static bool will_stage(const lime_ctx *c, bool all_sources_pinned, size_t total_bytes)
    {
        return !all_sources_pinned && !(c && c->no_staging) && (total_bytes >= ((size_t)8 << 20) || (c && c->force_staging));
    }
    static bool pinned(const void *p)
    {
        if (!p) return true;
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
        return at.type == hipMemoryTypeHost;
    }
    IoPool pool;
    int init(const lime_ctx *c, size_t bytes_per_chunk, uint64_t chunks, bool all_sources_pinned, std::function<int(uint64_t, Piece *)> d)
    {
        describe = std::move(d); n_chunks = chunks; slot_bytes = bytes_per_chunk;
        // small collections: the ring's set-up (pinned allocations, a thread) costs more than it hides
        staged = will_stage(c, all_sources_pinned, bytes_per_chunk * chunks);
        if (!staged) return LIME_OK;
        HIP_TRY(hipGetDevice(&device));
        // staging threads: the ctx's io_threads (the drop-in programs pass their `threads` argument; LIME_IO_THREADS at lime_init), else 8 -- never more
        // than the CPUs this process may run on
        io_threads = staging_threads(c);
        if (io_threads > 1) pool.start(io_threads);
        for (int i = 0; i < NS; ++i) {
            HIP_TRY(hipHostMalloc(&slot[i], slot_bytes + 64, hipHostMallocDefault));
            HIP_TRY(hipEventCreateWithFlags(&h2d_done[i], hipEventDisableTiming));
        }
        producer = std::thread([this]() {
            (void)hipSetDevice(device);
            Piece pc[MAXP];
            for (uint64_t k = 0; k < n_chunks; ++k) {
                if (k >= NS) {                               // slot k % NS: its previous content must have left for the device
                    std::unique_lock<std::mutex> lk(mu);
                    cv.wait(lk, [&] { return issued > k - NS || stop; });
                    if (stop) return;
                    lk.unlock();
                    if (hipEventSynchronize(h2d_done[k % NS]) != hipSuccess) { std::lock_guard<std::mutex> g(mu); failed = true; cv.notify_all(); return; }
                }
                { std::lock_guard<std::mutex> g(mu); if (stop) return; }
                const int np = describe(k, pc);
                size_t off = 0;
                std::vector<IoPool::Task> tk;
                for (int i = 0; i < np; ++i) {
                    for (size_t o = 0; o < pc[i].bytes; o += (size_t)1 << 20)
                        tk.push_back(IoPool::Task{(char *)slot[k % NS] + off + o, (const char *)pc[i].src + o, pc[i].bytes - o < ((size_t)1 << 20) ? pc[i].bytes - o : (size_t)1 << 20});
                    off += (pc[i].bytes + 15) & ~(size_t)15;
                }
                pool.run(std::move(tk));
                { std::lock_guard<std::mutex> g(mu); filled = k + 1; }
                cv.notify_all();
            }
        });
        return LIME_OK;
    }
    // the copies of chunk k, asynchronous on `copy` (chunks must be fed in order)
    int feed(uint64_t k, hipStream_t copy)
    {
        Piece pc[MAXP];
        const int np = describe(k, pc);
        if (!staged) {
            for (int i = 0; i < np; ++i) HIP_TRY(hipMemcpyAsync(pc[i].dst, pc[i].src, pc[i].bytes, hipMemcpyHostToDevice, copy));
            return LIME_OK;
        }
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return filled > k || failed; });
            if (failed) return fail(LIME_ERR_HIP, "staging thread failed");
        }
        size_t off = 0;
        for (int i = 0; i < np; ++i) {
            HIP_TRY(hipMemcpyAsync(pc[i].dst, (char *)slot[k % NS] + off, pc[i].bytes, hipMemcpyHostToDevice, copy));
            off += (pc[i].bytes + 15) & ~(size_t)15;
        }
        HIP_TRY(hipEventRecord(h2d_done[k % NS], copy));
        { std::lock_guard<std::mutex> g(mu); issued = k + 1; }
        cv.notify_all();
        return LIME_OK;
    }
    ~Feeder()
    {
        { std::lock_guard<std::mutex> g(mu); stop = true; }
        cv.notify_all();
        if (producer.joinable()) producer.join();
        for (int i = 0; i < NS; ++i) { if (h2d_done[i]) { (void)hipEventSynchronize(h2d_done[i]); (void)hipEventDestroy(h2d_done[i]); } if (slot[i]) (void)hipHostFree(slot[i]); }
    }
};
}

// Host arrays -> device buffers through the pinned staging ring, asynchronous pieces on `st`, complete on return
// (lime_fused_multi: one host thread per device calls this, so k devices upload at k times the rate of one).
int lime_internal_upload(int n_arr, const void *const *src, void *const *dst, const size_t *bytes, hipStream_t st)
{
    const size_t CH = (size_t)32 << 20;                   // bytes per array and chunk
    size_t total = 0, longest = 0;
    bool pinned = true;
    for (int i = 0; i < n_arr; ++i) { total += bytes[i]; if (bytes[i] > longest) longest = bytes[i]; pinned = pinned && Feeder::pinned(src[i]); }
    if (!total) return LIME_OK;
    if (n_arr > Feeder::MAXP) return fail(LIME_ERR_ARG, "lime_internal_upload: too many arrays");
    const uint64_t n_chunks = (longest + CH - 1) / CH;
    Feeder feeder;
    int rc = feeder.init(nullptr, (size_t)n_arr * (CH + 16), n_chunks, pinned, [&](uint64_t k, Piece *pc) {
        int np = 0;
        for (int i = 0; i < n_arr; ++i) {
            const size_t off = (size_t)k * CH;
            if (off >= bytes[i]) continue;
            pc[np++] = Piece{(const char *)src[i] + off, bytes[i] - off < CH ? bytes[i] - off : CH, (char *)dst[i] + off};
        }
        return np;
    });
    if (rc) return rc;
    for (uint64_t k = 0; k < n_chunks; ++k) if ((rc = feeder.feed(k, st))) { (void)hipStreamSynchronize(st); return rc; }
    HIP_TRY(hipStreamSynchronize(st));
    return LIME_OK;
}

extern "C" int lime_fused_stream(lime_ctx *c, const uint32_t *lcp, const uint32_t *da, const uint8_t *ebwt, uint64_t n,
                                 uint32_t n_reads, uint32_t n_refs, uint32_t alpha, uint64_t chunk, uint8_t *sim,
                                 uint64_t *n_clusters, uint64_t *max_len)
{
    int rc = check_ctx(c, "lime_fused_stream"); if (rc) return rc;
    if (!sim || (n && (!lcp || !da))) return fail(LIME_ERR_ARG, "lime_fused_stream: NULL array");
    if (!n_reads || !n_refs) return fail(LIME_ERR_ARG, "lime_fused_stream: n_reads and n_refs must be > 0");
    const bool src_pinned = Feeder::pinned(lcp) && Feeder::pinned(da) && Feeder::pinned(ebwt);
    if (!chunk) chunk = Feeder::will_stage(c, src_pinned, (size_t)n * 9) ? STAGED_CHUNK : STREAM_CHUNK;
    chunk = (chunk + LIME_TILE - 1) / LIME_TILE * LIME_TILE;
    const uint64_t cap = (chunk < n ? chunk : n) + STREAM_HALO;         // elements per device buffer
    Pipe pp;
    if ((rc = pp.init())) return rc;
    DevBuf dl[2], dd[2], de[2], ds;
    const int nbuf = n > chunk ? 2 : 1;
    for (int b = 0; b < nbuf; ++b) {
        if ((rc = dl[b].alloc(cap * 4 + 16))) return rc;
        if ((rc = dd[b].alloc(cap * 4 + 16))) return rc;
        if (ebwt && (rc = de[b].alloc(cap + 16))) return rc;
    }
    if ((rc = ds.alloc(lime_sim_bytes(n_reads, n_refs)))) return rc;
    if (!n) HIP_TRY(hipMemsetAsync(ds.p, 0, lime_sim_bytes(n_reads, n_refs), pp.comp));
    const uint64_t n_chunks = (n + chunk - 1) / chunk;
    DevBuf dedge;                                          // one edge word per chunk (runs longer than the halo across chunk borders)
    if ((rc = dedge.alloc((size_t)(n_chunks + 1) * 4))) return rc;
    HIP_TRY(hipMemsetAsync(dedge.p, 0, (size_t)(n_chunks + 1) * 4, pp.comp));
    Feeder feeder;
    if ((rc = feeder.init(c, cap * 9 + 64, n_chunks, src_pinned,
                          [&](uint64_t kk, Piece *pc) {
                              const uint64_t lo = kk * chunk, own = n - lo < chunk ? n - lo : chunk;
                              const uint64_t avail = n - lo < own + STREAM_HALO ? n - lo : own + STREAM_HALO;
                              const int b = (int)(kk & 1);
                              pc[0] = Piece{lcp + lo, (size_t)avail * 4, dl[b].p}; pc[1] = Piece{da + lo, (size_t)avail * 4, dd[b].p};
                              if (ebwt) pc[2] = Piece{ebwt + lo, (size_t)avail, de[b].p};
                              return ebwt ? 3 : 2;
                          }))) return rc;
    uint64_t k = 0;
    for (uint64_t lo = 0; lo < n; lo += chunk, ++k) {
        const int b = (int)(k & 1);
        const uint64_t own = n - lo < chunk ? n - lo : chunk;
        const uint64_t avail = n - lo < own + STREAM_HALO ? n - lo : own + STREAM_HALO;
        const int eof = lo + avail == n;
        if (k >= 2) HIP_TRY(hipStreamWaitEvent(pp.copy, pp.consumed[b], 0));        // the buffer is free again
        if ((rc = feeder.feed(k, pp.copy))) { (void)hipDeviceSynchronize(); return rc; }
        HIP_TRY(hipEventRecord(pp.copied[b], pp.copy));
        HIP_TRY(hipStreamWaitEvent(pp.comp, pp.copied[b], 0));
        rc = fused_dev_impl(c, (const uint32_t *)dl[b].p, (const uint32_t *)dd[b].p, ebwt ? (const uint8_t *)de[b].p : nullptr,
                            own, avail, eof, n_reads, n_refs, alpha, (uint8_t *)ds.p, k == 0, k != 0, pp.comp, (uint32_t *)dedge.p + k,
                            n_chunks > 1);
        if (rc) { (void)hipDeviceSynchronize(); return rc; }
        HIP_TRY(hipEventRecord(pp.consumed[b], pp.comp));
    }
    lime_stats_t s;
    rc = lime_get_stats(c, &s, pp.comp);
    if (n_clusters) *n_clusters = n ? s.n_clusters : 0;
    if (max_len) *max_len = n ? s.max_len : 0;
    if (rc) { (void)hipDeviceSynchronize(); return rc; }
    if (n_chunks > 1) {
        std::vector<uint32_t> edges(n_chunks);
        HIP_TRY(hipMemcpyAsync(edges.data(), dedge.p, (size_t)n_chunks * 4, hipMemcpyDeviceToHost, pp.comp));
        HIP_TRY(hipStreamSynchronize(pp.comp));
        if ((rc = lime_combine_edges(edges.data(), (uint32_t)n_chunks))) { (void)hipDeviceSynchronize(); return rc; }
    }
    if ((rc = d2h_pageable(c, sim, ds.p, (size_t)n_reads * n_refs, pp.comp))) return rc;
    HIP_TRY(hipStreamSynchronize(pp.comp));
    HIP_TRY(hipStreamSynchronize(pp.copy));
    return LIME_OK;
}

// The walk of lime_detect / lime_detect_to_file: position-range chunks with a read-ahead halo (see lime_fused_stream); records of chunk k follow
// those of chunk k-1, so the list stays in ascending pStart = the reference's 1-thread order.  The copy of chunk k+1 (through the pinned ring
// when the arrays are pageable) is under way while chunk k is scanned.  sink(device records, count, stream): takes a chunk's records (the list
// of the ctx is reused by the next chunk: the walk waits for the stream after every sink call).
static int detect_walk(lime_ctx *c, const uint32_t *lcp, const uint32_t *da, uint64_t n, uint32_t n_reads, uint32_t alpha, uint64_t chunk,
                       uint64_t *max_len, const std::function<int(const lime_cluster_t *, uint64_t, hipStream_t)> &sink)
{
    chunk = (chunk + LIME_TILE - 1) / LIME_TILE * LIME_TILE;
    const uint64_t cap = (chunk < n ? chunk : n) + STREAM_HALO, n_chunks = (n + chunk - 1) / chunk;
    int rc;
    uint64_t ml = 0;
    Pipe pp;
    if ((rc = pp.init())) return rc;
    DevBuf dl[2], dd[2];
    for (int b = 0; b < (n_chunks > 1 ? 2 : 1); ++b) { if ((rc = dl[b].alloc(cap * 4 + 16))) return rc; if ((rc = dd[b].alloc(cap * 4 + 16))) return rc; }
    Feeder feeder;
    if ((rc = feeder.init(c, cap * 8 + 64, n_chunks, Feeder::pinned(lcp) && Feeder::pinned(da), [&](uint64_t kk, Piece *pc) {
            const uint64_t lo = kk * chunk, own = n - lo < chunk ? n - lo : chunk;
            const uint64_t avail = n - lo < own + STREAM_HALO ? n - lo : own + STREAM_HALO;
            pc[0] = Piece{lcp + lo, (size_t)avail * 4, dl[kk & 1].p}; pc[1] = Piece{da + lo, (size_t)avail * 4, dd[kk & 1].p};
            return 2;
        }))) return rc;
    if ((rc = feeder.feed(0, pp.copy))) return rc;
    HIP_TRY(hipEventRecord(pp.copied[0], pp.copy));
    for (uint64_t k = 0; k < n_chunks; ++k) {
        const int b = (int)(k & 1);
        const uint64_t lo = k * chunk, own = n - lo < chunk ? n - lo : chunk;
        const uint64_t avail = n - lo < own + STREAM_HALO ? n - lo : own + STREAM_HALO;
        if (k + 1 < n_chunks) {                       // the next chunk's copy goes out before this chunk's scan is waited for
            const int nb = (int)((k + 1) & 1);
            if (k + 1 >= 2) HIP_TRY(hipStreamWaitEvent(pp.copy, pp.consumed[nb], 0));
            if ((rc = feeder.feed(k + 1, pp.copy))) { (void)hipDeviceSynchronize(); return rc; }
            HIP_TRY(hipEventRecord(pp.copied[nb], pp.copy));
        }
        HIP_TRY(hipStreamWaitEvent(pp.comp, pp.copied[b], 0));
        const lime_cluster_t *dc = nullptr;
        uint64_t cnt = 0, m = 0;
        rc = lime_detect_dev(c, (const uint32_t *)dl[b].p, (const uint32_t *)dd[b].p, own, avail, lo + avail == n, lo, n_reads,
                             alpha, &dc, &cnt, &m, pp.comp);
        if (rc) { (void)hipDeviceSynchronize(); return rc; }
        if (m > ml) ml = m;
        HIP_TRY(hipEventRecord(pp.consumed[b], pp.comp));   // (the arrays of the chunk have been read: lime_detect_dev waited for its count)
        if (cnt && (rc = sink(dc, cnt, pp.comp))) { (void)hipDeviceSynchronize(); return rc; }
        HIP_TRY(hipStreamSynchronize(pp.comp));           // the record list of the ctx is reused by the next chunk
    }
    HIP_TRY(hipStreamSynchronize(pp.copy));
    *max_len = ml;
    return LIME_OK;
}

static uint64_t detect_chunk(const lime_ctx *c, const uint32_t *lcp, const uint32_t *da, uint64_t n)
{
    if (c->detect_chunk) return c->detect_chunk;
    return Feeder::will_stage(c, Feeder::pinned(lcp) && Feeder::pinned(da), (size_t)n * 8) ? STAGED_CHUNK : STREAM_CHUNK;
}

// one walk with chunks of `chunk` symbols, the records gathered in host memory (*clusters: malloc'ed, the caller's)
static int detect_to_host(lime_ctx *c, const uint32_t *lcp, const uint32_t *da, uint64_t n, uint32_t n_reads, uint32_t alpha, uint64_t chunk,
                          lime_cluster_t **clusters, uint64_t *n_clusters, uint64_t *max_len)
{
    lime_cluster_t *h = nullptr;
    uint64_t have = 0, room = 0, ml = 0;
    auto sink = [&](const lime_cluster_t *dc, uint64_t cnt, hipStream_t st) -> int {
        if (have + cnt > room) {
            room = (have + cnt) + (have + cnt) / 2 + 1024;
            lime_cluster_t *g = (lime_cluster_t *)realloc(h, (size_t)room * sizeof(lime_cluster_t));
            if (!g) return fail(LIME_ERR_NOMEM, "lime_detect: out of host memory");
            h = g;
        }
        HIP_TRY(hipMemcpyAsync(h + have, dc, (size_t)cnt * sizeof(lime_cluster_t), hipMemcpyDeviceToHost, st));
        have += cnt;
        return LIME_OK;
    };
    const int rc = detect_walk(c, lcp, da, n, n_reads, alpha, chunk, &ml, sink);
    if (rc) { free(h); return rc; }
    *clusters = h; *n_clusters = have; *max_len = ml;
    return LIME_OK;
}

extern "C" int lime_detect(lime_ctx *c, const uint32_t *lcp, const uint32_t *da, uint64_t n, uint32_t n_reads,
                           uint32_t alpha, lime_cluster_t **clusters, uint64_t *n_clusters, uint64_t *max_len)
{
    int rc = check_ctx(c, "lime_detect"); if (rc) return rc;
    if (!clusters || !n_clusters || !max_len) return fail(LIME_ERR_ARG, "lime_detect: NULL output");
    *clusters = nullptr; *n_clusters = 0; *max_len = 0;
    if (n && (!lcp || !da)) return fail(LIME_ERR_ARG, "lime_detect: NULL array");
    if (!n) return LIME_OK;
    const uint64_t chunk0 = detect_chunk(c, lcp, da, n);
    rc = detect_to_host(c, lcp, da, n, n_reads, alpha, chunk0, clusters, n_clusters, max_len);
    if (rc == LIME_ERR_HALO && chunk0 < n)
        // a run longer than the halo crosses a chunk border.  ClusterLCP itself has no length limit (only
        // ClusterBWT_DA refuses such a cluster later): redo the whole collection as one chunk
        rc = detect_to_host(c, lcp, da, n, n_reads, alpha, n, clusters, n_clusters, max_len);
    return rc;
}

// lime_detect with the records written to `path` as they come (the .clrs file of ClusterLCP.cpp:229-235, ascending pStart): every chunk's
// records land in one of two pinned buffers and a writer thread appends them to the file while the next chunk is scanned -- no list of the
// whole collection on the host (10^9 symbols: 0.9 GB that round 4 grew by realloc, copied through a pageable buffer and wrote at the end).
extern "C" int lime_detect_to_file(lime_ctx *c, const uint32_t *lcp, const uint32_t *da, uint64_t n, uint32_t n_reads,
                                   uint32_t alpha, const char *path, uint64_t *n_clusters, uint64_t *max_len)
{
    int rc = check_ctx(c, "lime_detect_to_file"); if (rc) return rc;
    if (!path || !n_clusters || !max_len) return fail(LIME_ERR_ARG, "lime_detect_to_file: NULL argument");
    *n_clusters = 0; *max_len = 0;
    if (n && (!lcp || !da)) return fail(LIME_ERR_ARG, "lime_detect_to_file: NULL array");
    // The records go to a temporary file next to `path` that takes its name only when the scan has succeeded: a failure on the way (pinned
    // memory, a HIP error, a full disk) leaves no truncated .clrs behind for ClusterBWT_DA to read (the reference's fopen "w" +
    // exit(1) does leave one, ClusterLCP.cpp:95-98 -- not a behaviour to keep)
    const std::string tmp = std::string(path) + ".tmp." + std::to_string((long)getpid());
    const int fd = open(tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) return fail(LIME_ERR_IO, "lime_detect_to_file: cannot create %s", path);
    if (!n) { close(fd); if (rename(tmp.c_str(), path)) { (void)unlink(tmp.c_str()); return fail(LIME_ERR_IO, "lime_detect_to_file: cannot create %s", path); } return LIME_OK; }
    const uint64_t chunk0 = detect_chunk(c, lcp, da, n);
    const size_t buf_records = (size_t)((chunk0 < n ? chunk0 : n) / 2 + 4096);      // a chunk has at most half as many clusters as positions
    void *pin[2] = {nullptr, nullptr};
    struct Job { int b; uint64_t cnt, at; };
    std::mutex mu; std::condition_variable cv;
    std::vector<Job> jobs; size_t taken = 0, written = 0; bool stop = false, io_failed = false;
    uint64_t have = 0, ml = 0;
    std::thread writer;
    auto finish = [&]() {
        { std::lock_guard<std::mutex> g(mu); stop = true; }
        cv.notify_all();
        if (writer.joinable()) writer.join();
        for (int b = 0; b < 2; ++b) if (pin[b]) (void)hipHostFree(pin[b]);
        close(fd);
    };
    if (hipHostMalloc(&pin[0], buf_records * sizeof(lime_cluster_t), hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc(&pin[1], buf_records * sizeof(lime_cluster_t), hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError(); finish(); (void)unlink(tmp.c_str());
        return fail(LIME_ERR_NOMEM, "lime_detect_to_file: no pinned memory for the record buffers");
    }
    writer = std::thread([&]() {
        for (;;) {
            Job j;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return stop || taken < jobs.size(); });
                if (taken >= jobs.size()) return;
                j = jobs[taken++];
            }
            size_t done = 0; const size_t len = (size_t)j.cnt * sizeof(lime_cluster_t);
            while (done < len) {
                const ssize_t k = pwrite(fd, (const char *)pin[j.b] + done, len - done, (off_t)(j.at * sizeof(lime_cluster_t) + done));
                if (k <= 0) { if (k < 0 && errno == EINTR) continue; std::lock_guard<std::mutex> g(mu); io_failed = true; break; }
                done += (size_t)k;
            }
            { std::lock_guard<std::mutex> g(mu); ++written; }
            cv.notify_all();
        }
    });
    uint64_t n_jobs = 0;
    auto sink = [&](const lime_cluster_t *dc, uint64_t cnt, hipStream_t st) -> int {
        if (cnt > buf_records) return fail(LIME_ERR_HIP, "internal: %llu records in one chunk", (unsigned long long)cnt);
        const int b = (int)(n_jobs & 1);
        {   // the buffer's previous content (two jobs ago) must be in the file
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return n_jobs < 2 || written + 2 > n_jobs || io_failed; });
            if (io_failed) return fail(LIME_ERR_IO, "lime_detect_to_file: write to %s failed", path);
        }
        HIP_TRY(hipMemcpyAsync(pin[b], dc, (size_t)cnt * sizeof(lime_cluster_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        { std::lock_guard<std::mutex> g(mu); jobs.push_back(Job{b, cnt, have}); }
        cv.notify_all();
        have += cnt; ++n_jobs;
        return LIME_OK;
    };
    rc = detect_walk(c, lcp, da, n, n_reads, alpha, chunk0, &ml, sink);
    {   // everything handed over is in the file
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return written == jobs.size() || io_failed; });
    }
    const bool bad_io = io_failed;
    finish();
    if (!rc && bad_io) rc = fail(LIME_ERR_IO, "lime_detect_to_file: write to %s failed", path);
    if (rc == LIME_ERR_HALO && chunk0 < n) {
        // (a run longer than the halo across a chunk border: the whole collection as ONE chunk, through memory -- directly, not through
        // lime_detect, whose first walk would repeat the chunked scan that has just failed)
        lime_cluster_t *h = nullptr;
        if ((rc = detect_to_host(c, lcp, da, n, n_reads, alpha, n, &h, &have, &ml))) { (void)unlink(tmp.c_str()); return rc; }
        rc = lime_write_clrs(tmp.c_str(), h, have);
        free(h);
        if (rc) { (void)unlink(tmp.c_str()); return fail(LIME_ERR_IO, "lime_detect_to_file: write to %s failed", path); }
    }
    if (rc) { (void)unlink(tmp.c_str()); return rc; }
    if (rename(tmp.c_str(), path)) { (void)unlink(tmp.c_str()); return fail(LIME_ERR_IO, "lime_detect_to_file: cannot create %s", path); }
    *n_clusters = have; *max_len = ml;
    return LIME_OK;
}

// clusterAnalyze of a host cluster list into the device table d_sim, the arrays going through HBM
// in position-range chunks: a chunk takes the clusters that START in it (any input order: an index
// sorted by pStart is built when needed) and the arrays up to the end of the last of them.
int lime_host::score_in_chunks(lime_ctx *c, const uint32_t *da, const uint8_t *ebwt, uint64_t n,
                           const lime_cluster_t *clusters, uint64_t n_clusters, uint32_t n_reads, uint32_t n_refs,
                           uint8_t *d_sim)
{
    int rc;
    HIP_TRY(hipMemset(d_sim, 0, lime_sim_bytes(n_reads, n_refs)));
    HIP_TRY(hipDeviceSynchronize());                      // the chunks below run on streams of their own
    if (!n_clusters) return LIME_OK;
    uint64_t chunk = c->score_chunk ? c->score_chunk : Feeder::will_stage(c, Feeder::pinned(da) && Feeder::pinned(ebwt), (size_t)n * 5) ? STAGED_CHUNK : STREAM_CHUNK;
    bool sorted = true;
    for (uint64_t i = 0; i < n_clusters; ++i) {
        const lime_cluster_t &q = clusters[i];
        if (q.len > LIME_MAX_CLUSTER) return fail(LIME_ERR_MAXLEN, "a cluster is longer than %u symbols", LIME_MAX_CLUSTER);
        if (q.pStart > n || q.len > n - q.pStart) return fail(LIME_ERR_ARG, "a cluster record lies outside the arrays");
        if (i && q.pStart < clusters[i - 1].pStart) sorted = false;
    }
    std::vector<lime_cluster_t> order;
    const lime_cluster_t *cl = clusters;
    if (!sorted) {
        order.assign(clusters, clusters + n_clusters);
        std::sort(order.begin(), order.end(), [](const lime_cluster_t &x, const lime_cluster_t &y) { return x.pStart < y.pStart; });
        cl = order.data();
    }
    // the plan: chunk k = clusters [i, j) that start in [lo, lo + chunk), arrays [lo, end) up to the end of the last of them
    struct Plan { uint64_t i, j, lo, end; };
    std::vector<Plan> plan;
    size_t max_el = 0, max_cl = 0;
    for (uint64_t i = 0; i < n_clusters;) {
        const uint64_t lo = cl[i].pStart, hi = lo + chunk;
        uint64_t j = i, end = lo;
        while (j < n_clusters && cl[j].pStart < hi) { if (cl[j].pStart + cl[j].len > end) end = cl[j].pStart + cl[j].len; ++j; }
        plan.push_back(Plan{i, j, lo, end});
        if (end - lo > max_el) max_el = (size_t)(end - lo);
        if (j - i > max_cl) max_cl = (size_t)(j - i);
        i = j;
    }
    Pipe pp;
    if ((rc = pp.init())) return rc;
    DevBuf dd[2], de[2], dc[2];
    for (int b = 0; b < (plan.size() > 1 ? 2 : 1); ++b) {
        if ((rc = dd[b].alloc(max_el * 4 + 16))) return rc;
        if (ebwt && (rc = de[b].alloc(max_el + 16))) return rc;
        if ((rc = dc[b].alloc(max_cl * sizeof(lime_cluster_t)))) return rc;
    }
    Feeder feeder;
    if ((rc = feeder.init(c, max_el * 5 + max_cl * sizeof(lime_cluster_t) + 64, plan.size(),
                          Feeder::pinned(da) && Feeder::pinned(ebwt) && Feeder::pinned(cl), [&](uint64_t k, Piece *pc) {
            const Plan &q = plan[k];
            const int b = (int)(k & 1);
            int np = 0;
            pc[np++] = Piece{da + q.lo, (size_t)(q.end - q.lo) * 4, dd[b].p};
            if (ebwt) pc[np++] = Piece{ebwt + q.lo, (size_t)(q.end - q.lo), de[b].p};
            pc[np++] = Piece{cl + q.i, (size_t)(q.j - q.i) * sizeof(lime_cluster_t), dc[b].p};
            return np;
        }))) return rc;
    if ((rc = feeder.feed(0, pp.copy))) return rc;
    HIP_TRY(hipEventRecord(pp.copied[0], pp.copy));
    for (uint64_t k = 0; k < plan.size(); ++k) {
        const int b = (int)(k & 1);
        const Plan &q = plan[k];
        if (k + 1 < plan.size()) {                        // the next chunk's copy goes out before this chunk's scoring is waited for
            const int nb = (int)((k + 1) & 1);
            if (k + 1 >= 2) HIP_TRY(hipStreamWaitEvent(pp.copy, pp.consumed[nb], 0));
            if ((rc = feeder.feed(k + 1, pp.copy))) { (void)hipDeviceSynchronize(); return rc; }
            HIP_TRY(hipEventRecord(pp.copied[nb], pp.copy));
        }
        HIP_TRY(hipStreamWaitEvent(pp.comp, pp.copied[b], 0));
        rc = score_dev_impl(c, (const uint32_t *)dd[b].p, ebwt ? (const uint8_t *)de[b].p : nullptr, q.end - q.lo,
                            (const lime_cluster_t *)dc[b].p, q.j - q.i, n_reads, n_refs, d_sim, 0, q.lo, pp.comp);
        if (rc) { (void)hipDeviceSynchronize(); return rc; }
        HIP_TRY(hipEventRecord(pp.consumed[b], pp.comp));
        lime_stats_t st;
        if ((rc = lime_get_stats(c, &st, pp.comp))) { (void)hipDeviceSynchronize(); return rc; }
    }
    HIP_TRY(hipStreamSynchronize(pp.copy));
    return LIME_OK;
}

extern "C" int lime_score(lime_ctx *c, const uint32_t *da, const uint8_t *ebwt, uint64_t n,
                          const lime_cluster_t *clusters, uint64_t n_clusters, uint32_t n_reads,
                          uint32_t n_refs, uint8_t *sim)
{
    int rc = check_ctx(c, "lime_score"); if (rc) return rc;
    if (!sim || (n && !da) || (n_clusters && !clusters)) return fail(LIME_ERR_ARG, "lime_score: NULL array");
    if (!n_reads || !n_refs) return fail(LIME_ERR_ARG, "lime_score: n_reads and n_refs must be > 0");
    DevBuf ds;
    if ((rc = ds.alloc(lime_sim_bytes(n_reads, n_refs)))) return rc;
    if ((rc = score_in_chunks(c, da, ebwt, n, clusters, n_clusters, n_reads, n_refs, (uint8_t *)ds.p))) return rc;
    if ((rc = d2h_pageable(c, sim, ds.p, (size_t)n_reads * n_refs, nullptr))) return rc;
    return LIME_OK;
}

extern "C" int lime_fused(lime_ctx *c, const uint32_t *lcp, const uint32_t *da, const uint8_t *ebwt, uint64_t n,
                          uint32_t n_reads, uint32_t n_refs, uint32_t alpha, uint8_t *sim, uint64_t *n_clusters,
                          uint64_t *max_len)
{
    int rc = check_ctx(c, "lime_fused"); if (rc) return rc;
    if (!sim || (n && (!lcp || !da))) return fail(LIME_ERR_ARG, "lime_fused: NULL array");
    if (n > 4 * STREAM_CHUNK)                             // large collections: bounded HBM footprint, copy under scan
        return lime_fused_stream(c, lcp, da, ebwt, n, n_reads, n_refs, alpha, 0, sim, n_clusters, max_len);
    DevBuf dl, dd, de, ds;
    if ((rc = dl.upload(lcp, n * 4))) return rc;
    if ((rc = dd.upload(da, n * 4))) return rc;
    if (ebwt && (rc = de.upload(ebwt, n))) return rc;
    if ((rc = ds.alloc(lime_sim_bytes(n_reads, n_refs)))) return rc;
    rc = lime_fused_dev(c, (const uint32_t *)dl.p, (const uint32_t *)dd.p, ebwt ? (const uint8_t *)de.p : nullptr,
                        n, n, 1, n_reads, n_refs, alpha, (uint8_t *)ds.p, 1, nullptr);
    if (rc) return rc;
    lime_stats_t s;
    rc = lime_get_stats(c, &s, nullptr);
    if (n_clusters) *n_clusters = s.n_clusters;
    if (max_len) *max_len = s.max_len;
    if (rc) return rc;
    if ((rc = d2h_pageable(c, sim, ds.p, (size_t)n_reads * n_refs, nullptr))) return rc;
    return LIME_OK;
}

extern "C" int lime_choose(lime_ctx *c, const uint8_t *sim, uint32_t n_reads, uint32_t n_refs, uint8_t *row_max,
                           uint32_t *row_nnz)
{
    int rc = check_ctx(c, "lime_choose"); if (rc) return rc;
    if (!sim || !row_max || !row_nnz) return fail(LIME_ERR_ARG, "lime_choose: NULL array");
    if (!n_reads) return LIME_OK;
    DevBuf ds, dm, dz;
    if ((rc = ds.alloc(lime_sim_bytes(n_reads, n_refs)))) return rc;
    HIP_TRY(hipMemcpy(ds.p, sim, (size_t)n_reads * n_refs, hipMemcpyHostToDevice));
    if ((rc = dm.alloc(n_reads))) return rc;
    if ((rc = dz.alloc((size_t)n_reads * 4))) return rc;
    if ((rc = lime_choose_dev(c, (const uint8_t *)ds.p, n_reads, n_refs, (uint8_t *)dm.p, (uint32_t *)dz.p, nullptr))) return rc;
    HIP_TRY(hipMemcpy(row_max, dm.p, n_reads, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(row_nnz, dz.p, (size_t)n_reads * 4, hipMemcpyDeviceToHost));
    return LIME_OK;
}

// Device memory -> freshly allocated pageable host memory (the (idRef, sim) lists: 0.7 GB when most of configs[2]'s rows pass): through two pinned
// slots, the copy of piece k + 1 under the host's copy of piece k by the staging threads.  The runtime's own staged copy does this on one thread,
// first-touch page faults included: 0.7 GB took 170 ms = 4 GB/s.
int lime_host::d2h_pageable(const lime_ctx *c, void *dst, const void *d_src, size_t bytes, hipStream_t st)
{
    constexpr size_t SLOT = (size_t)8 << 20, PIECE = (size_t)1 << 20;
    if (bytes < 4 * SLOT || (c && c->no_staging) || Feeder::pinned(dst)) {     // (pinned destinations: the copy engine writes them directly)
        HIP_TRY(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return LIME_OK;
    }
    struct Ring {
        void *slot[2] = {nullptr, nullptr}; hipEvent_t ev[2] = {nullptr, nullptr};
        ~Ring() { for (int i = 0; i < 2; ++i) { if (slot[i]) (void)hipHostFree(slot[i]); if (ev[i]) (void)hipEventDestroy(ev[i]); } }
    } r;
    for (int i = 0; i < 2; ++i) { HIP_TRY(hipHostMalloc(&r.slot[i], SLOT)); HIP_TRY(hipEventCreateWithFlags(&r.ev[i], hipEventDisableTiming)); }
    const int threads = staging_threads(c);
    IoPool pool;
    if (threads > 1) pool.start(threads);
    const size_t n_chunks = (bytes + SLOT - 1) / SLOT;
    auto len_of = [&](size_t k) { return k + 1 < n_chunks ? SLOT : bytes - k * SLOT; };
    for (size_t k = 0; k <= n_chunks; ++k) {
        if (k < n_chunks) {
            HIP_TRY(hipMemcpyAsync(r.slot[k & 1], static_cast<const uint8_t *>(d_src) + k * SLOT, len_of(k), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipEventRecord(r.ev[k & 1], st));
        }
        if (k >= 1) {                                      // (slot (k - 1) & 1 is written again by copy k + 1, issued after this returns)
            const size_t j = k - 1, len = len_of(j);
            HIP_TRY(hipEventSynchronize(r.ev[j & 1]));
            std::vector<IoPool::Task> t;
            for (size_t o = 0; o < len; o += PIECE)
                t.push_back({static_cast<uint8_t *>(dst) + j * SLOT + o, static_cast<const uint8_t *>(r.slot[j & 1]) + o, len - o < PIECE ? len - o : PIECE});
            pool.run(std::move(t));
        }
    }
    return LIME_OK;
}
