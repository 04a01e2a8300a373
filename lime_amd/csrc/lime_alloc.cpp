// lime_alloc.cpp -- where the library's device memory comes from: the process-wide cache of released blocks (BlockCache), the arenas of
// lime_reserve, lime_trim_cache, and dev_acquire / dev_release, through which every large buffer of a context goes.
#include <hip/hip_runtime.h>
#include <mutex>
#include <vector>

#include "lime_ctx.h"
#include "lime_extents.h"

using namespace lime;
using namespace lime_host;

std::atomic<bool> lime_host::g_debug_alloc{false}, lime_host::g_poison_cache{false};   // "poison_cache" (on under LIME_TEST_HOOKS): a block taken from the cache is filled with 0xA5 -- nothing may rely on what a fresh allocation holds          // lime_set_option "debug_alloc": every device allocation of the library on stderr

// ---- device blocks released by the contexts of this process, kept for the next one -------------------------------------------------
// Why (measured, tools/alloc_bench.hip, round 6): a hipMalloc on this platform costs 0.04-0.3 ms whatever its size AS LONG AS the driver hands
// out pages that were never used since they were last cleared; pages that this or another process has written and freed are cleared by the
// driver INSIDE the hipMalloc that gets them, at 25-35 GB/s -- 2.0 s for 25.8 GB allocated right after the same 25.8 GB were freed, 3.8 s
// for 12.9 GB after 3 x 32 GB were freed, 6.0 s for 215 GB -- and the allocator does not prefer clean pages.  That is the "1 ms to 5.2 s"
// of round 5's cold passes (bench.py frees 80-150 GB of arrays between workloads), and a pool that was re-grown by 0.02 % -- free 15.6 GB,
// allocate 15.6 GB -- paid 4.9 s for it.  So the library never gives a large block back while the process lives: lime_shutdown and a growing array (DevArr) put
// blocks of 64 MB and more here, the next request takes the smallest cached block that is large enough (and at most twice as large), and
// lime_trim_cache() -- or a failed hipMalloc -- returns them to the driver.  At most a quarter of the device's memory is held.
namespace {
struct BlockCache {
    struct B { void *p; size_t bytes; int dev; };
    static constexpr size_t MIN = (size_t)64 << 20;
    std::mutex mu;
    std::vector<B> idle, out;                               // cached blocks; blocks handed out (their true sizes)
    // lime_reserve: blocks taken from the driver ONCE (at process start, where the time shows as what it is), from which the large buffers of every
    // context are carved afterwards: first fit over the free extents (offset-sorted, merged on return), 2 MB granules (lime_extents.h)
    struct Arena { char *base; size_t bytes; int dev; Extents free_; size_t live; };
    struct Carve { void *p; size_t arena, off, bytes; };
    static constexpr size_t GRAN = (size_t)2 << 20;
    std::vector<Arena> arenas;
    std::vector<Carve> carved;
    bool add_arena(int dev, void *base, size_t bytes)
    {
        std::lock_guard<std::mutex> g(mu);
        arenas.push_back(Arena{static_cast<char *>(base), bytes, dev, Extents(bytes, GRAN), 0});
        return true;
    }
    void *carve(int dev, size_t bytes, size_t *got)
    {
        std::lock_guard<std::mutex> g(mu);
        for (size_t ai = 0; ai < arenas.size(); ++ai) {
            Arena &A = arenas[ai];
            if (A.dev != dev) continue;
            size_t want = 0;
            const size_t off = A.free_.take(bytes, &want);
            if (off == Extents::NONE) continue;
            A.live += want;
            carved.push_back(Carve{A.base + off, ai, off, want});
            *got = want;
            return A.base + off;
        }
        return nullptr;
    }
    bool uncarve(void *p)                                   // true: p was a piece of an arena and is free again
    {
        std::lock_guard<std::mutex> g(mu);
        for (size_t ci = 0; ci < carved.size(); ++ci)
            if (carved[ci].p == p) {
                const Carve c = carved[ci];
                carved.erase(carved.begin() + (long)ci);
                Arena &A = arenas[c.arena];
                A.live -= c.bytes;
                A.free_.give(c.off, c.bytes);
                return true;
            }
        return false;
    }
    void *take(int dev, size_t bytes, size_t *got)
    {
        std::lock_guard<std::mutex> g(mu);
        size_t best = (size_t)-1;
        for (size_t i = 0; i < idle.size(); ++i)
            if (idle[i].dev == dev && idle[i].bytes >= bytes && idle[i].bytes / 2 <= bytes && (best == (size_t)-1 || idle[i].bytes < idle[best].bytes)) best = i;
        if (best == (size_t)-1) return nullptr;
        const B b = idle[best];
        idle.erase(idle.begin() + (long)best);
        out.push_back(b);
        *got = b.bytes;
        return b.p;
    }
    bool tracked(const void *p)
    {
        std::lock_guard<std::mutex> g(mu);
        for (const B &b : out) if (b.p == p) return true;
        for (const Carve &c : carved) if (c.p == p) return true;
        return false;
    }
    void note(int dev, void *p, size_t bytes) { if (bytes >= MIN) { std::lock_guard<std::mutex> g(mu); out.push_back(B{p, bytes, dev}); } }
    // true: the cache keeps p; false: the caller frees it
    bool give(void *p)
    {
        std::lock_guard<std::mutex> g(mu);
        for (size_t i = 0; i < out.size(); ++i)
            if (out[i].p == p) {
                const B b = out[i];
                out.erase(out.begin() + (long)i);
                size_t held = b.bytes, total = 0, fr = 0;
                for (const B &x : idle) if (x.dev == b.dev) held += x.bytes;
                if (hipMemGetInfo(&fr, &total) != hipSuccess || held > total / 4) return false;
                idle.push_back(b);
                return true;
            }
        return false;
    }
    size_t trim(int dev)                                    // dev < 0: every device
    {
        std::vector<B> drop;
        {
            std::lock_guard<std::mutex> g(mu);
            for (size_t i = 0; i < idle.size();) if (dev < 0 || idle[i].dev == dev) { drop.push_back(idle[i]); idle.erase(idle.begin() + (long)i); } else ++i;
        }
        {
            // (arenas nothing is carved from any more go too; the indices of the others stay what the carve records hold: emptied in place)
            std::lock_guard<std::mutex> g(mu);
            for (Arena &A : arenas)
                if (A.base && A.live == 0 && (dev < 0 || A.dev == dev)) { drop.push_back(B{A.base, A.bytes, A.dev}); A.base = nullptr; A.bytes = 0; A.free_.free_.clear(); }
        }
        int cur = 0; (void)hipGetDevice(&cur);
        size_t bytes = 0;
        for (const B &b : drop) { (void)hipSetDevice(b.dev); (void)hipFree(b.p); bytes += b.bytes; }
        if (!drop.empty()) (void)hipSetDevice(cur);
        return bytes;
    }
};
BlockCache g_blocks;
}
extern "C" size_t lime_trim_cache(void) { return g_blocks.trim(-1); }
extern "C" int lime_reserve(size_t bytes)
{
    if (!bytes) return LIME_OK;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return LIME_ERR_HIP;
    void *p = nullptr;
    const size_t want = (bytes + BlockCache::GRAN - 1) / BlockCache::GRAN * BlockCache::GRAN;
    if (hipMalloc(&p, want) != hipSuccess) { (void)hipGetLastError(); return LIME_ERR_NOMEM; }
    g_blocks.add_arena(dev, p, want);
    return LIME_OK;
}

void lime_host::dev_release(void *p)
{
    if (!p) return;
    // (hipFree waits for the device before a block goes back; a block that goes to the cache instead can be handed out again at once, so it waits the
    // same way: on the success paths everything that used the block has been waited for anyway, on an error path work on it may still be queued)
    if (g_blocks.tracked(p)) (void)hipDeviceSynchronize();
    if (g_blocks.uncarve(p)) return;
    if (!g_blocks.give(p)) (void)hipFree(p);
}
hipError_t lime_host::dev_acquire(void **p, size_t bytes)
{
    int dev = 0; (void)hipGetDevice(&dev);
    size_t got = 0;
    if (bytes >= BlockCache::MIN && ((*p = g_blocks.take(dev, bytes, &got)) || (*p = g_blocks.carve(dev, bytes, &got)))) {
        if (g_poison_cache.load(std::memory_order_relaxed)) { (void)hipMemset(*p, 0xA5, got); (void)hipDeviceSynchronize(); }
        return hipSuccess;
    }
    hipError_t e = hipMalloc(p, bytes);
    if (e == hipErrorOutOfMemory && g_blocks.trim(dev)) { (void)hipGetLastError(); e = hipMalloc(p, bytes); }
    if (e == hipSuccess) g_blocks.note(dev, *p, bytes);
    return e;
}
