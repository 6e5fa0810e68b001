// runtime.hip -- the device runtime behind exec.h, host API only, no kernel: the calling thread's stream and device selection
// (ctx, select_device), the caching allocator behind every per-call buffer (pool_*, memory_*; rdr::Arena owns its blocks), batched
// transfers through a pinned staging buffer per host thread, constant tables per device, and what a host thread keeps per device
// (ThreadDeviceState: compaction scratch, side streams, the two rings of counters).  "Per device" is a rdr::PerDevice (../per_device.h).
#include "exec.h"
#include <algorithm>
#include <cstring>
#include <map>
#include <unordered_map>
#include <vector>

namespace exec {

Context &ctx() { static thread_local Context c; return c; }

void select_device(int use_gpu, int gpu_index) {
    if (!use_gpu)
        throw std::runtime_error("redner_amd renders on an MI355X (gfx950) GPU only: Scene(use_gpu=False) "
                                 "is not supported and there is no CPU fallback");
    gpu_index = rdr::device_slot(gpu_index);          // an index without a slot is an error whatever the machine holds
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count == 0)
        throw std::runtime_error("redner_amd: no HIP device is visible (hipGetDeviceCount) -- a gfx950 GPU is required");
    if (gpu_index >= count) throw std::runtime_error("redner_amd: gpu_index out of range");
    check(hipSetDevice(gpu_index), "hipSetDevice");
}

namespace {
struct PoolLists {                                              // of one device
    std::multimap<size_t, void *> free_blocks;                  // by capacity
    size_t parked = 0, from_driver = 0;      // bytes in free_blocks (kept in step: no walk per free); bytes held from hipMalloc (live + parked)
};
struct Pool {
    std::mutex lock;
    rdr::PerDevice<PoolLists> dev;
    std::unordered_map<void *, std::pair<size_t, int>> live;    // block -> (capacity, device: it has passed dev.at())
    size_t device_mallocs = 0;
    long long cap_override = -1;                                // rdr_set_pool_cap_mb
};
Pool &pool() { static Pool *p = new Pool(); return *p; }       // never destroyed: blocks may be returned during exit

// The cache is bounded: a torch process shares the device with torch's own allocator, which cannot reclaim what is parked
// here.  Default: a quarter of the device's memory but no more than 8 GiB (round 6; 16 GiB in rounds 4-5; round 3 parked up
// to 72 GB -- the 48 GB of a 2^24-lane sample batch -- for +4 % at 1024 x 1024).  More is a decision of the caller:
// rdr_set_pool_cap_mb / RDR_POOL_CAP_MB (bench.py owns its GPU, raises the bound and says so in its line);
// rdr_trim_cache() releases everything.
size_t pool_cap(const Pool &pl) {
    if (pl.cap_override >= 0) return (size_t)pl.cap_override;
    static const size_t dflt = [] {
        if (const char *e = std::getenv("RDR_POOL_CAP_MB")) return (size_t)std::max(0, std::atoi(e)) << 20;
        const size_t eight = (size_t)8192 << 20;
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return eight; }
        return std::min(total_b / 4, eight);
    }();
    return dflt;
}
}

size_t pool_cap_bytes() { Pool &pl = pool(); std::lock_guard<std::mutex> lk(pl.lock); return pool_cap(pl); }

void pool_set_cap(long long bytes) {
    Pool &pl = pool();
    std::lock_guard<std::mutex> lk(pl.lock);
    pl.cap_override = bytes;
}

// RDR_POOL_POISON=1 (debugging): every block handed out is filled with 0xFF bytes (NaN as a double or float, -1 as an int) on
// the calling thread's stream -- a buffer that is read before it is written then fails the same way every time instead of
// depending on what the pool last kept in it (fresh device memory is zero; the CPU harness gets zero pages from malloc).
static void *pool_alloc_raw(size_t bytes);
static void pool_release(int only_dev);
void *pool_alloc(size_t bytes) {
    void *p = pool_alloc_raw(bytes);
    static const bool poison = std::getenv("RDR_POOL_POISON") != nullptr;
    if (poison) check(hipMemsetAsync(p, 0xFF, std::max<size_t>(bytes, 16), ctx().stream), "pool poison");
    return p;
}
static void *pool_alloc_raw(size_t bytes) {
    const size_t want = (std::max<size_t>(bytes, 16) + 255) & ~(size_t)255;
    const int dev = current_device();
    Pool &pl = pool();
    PoolLists &mine = pl.dev.at(dev);             // the index enters here: pool_free and pool_release look it up unchecked
    {
        std::lock_guard<std::mutex> lk(pl.lock);
        auto it = mine.free_blocks.lower_bound(want);
        if (it != mine.free_blocks.end() && it->first <= want + want / 4 + 4096) {          // close fit: reuse
            void *p = it->second;
            pl.live[p] = {it->first, dev};
            mine.parked -= it->first;
            mine.free_blocks.erase(it);
            return p;
        }
    }
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) {             // out of memory with blocks parked in the cache: release them and retry once
        (void)hipGetLastError();
        pool_release(dev);             // this device's parked blocks only: the other devices' callers are not disturbed
        check(hipMalloc(&p, want), "hipMalloc");
    }
    std::lock_guard<std::mutex> lk(pl.lock);
    pl.device_mallocs++;
    mine.from_driver += want;
    pl.live[p] = {want, dev};
    return p;
}

void pool_free(void *p) {
    if (!p) return;
    Pool &pl = pool();
    std::unique_lock<std::mutex> lk(pl.lock);
    auto it = pl.live.find(p);
    if (it == pl.live.end()) { lk.unlock(); (void)hipFree(p); return; }
    const size_t bytes = it->second.first;
    PoolLists &home = pl.dev.slot[it->second.second];
    pl.live.erase(it);
    if (home.parked + bytes > pool_cap(pl)) {
        home.from_driver -= bytes;
        lk.unlock();
        (void)hipFree(p);              // waits for the device: safe whatever is in flight; outside the lock: the other workers go on
        return;
    }
    home.free_blocks.emplace(bytes, p);
    home.parked += bytes;
}

// Parked blocks of ONE device (-1: of every device) back to the driver.  The blocks are taken off the lists under the pool's
// lock and released outside it: hipFree waits for the device, and another device's allocations must not wait with it
// (one process driving several devices from several threads).
static void pool_release(int only_dev) {
    Pool &pl = pool();
    std::vector<std::pair<int, void *>> gone;
    {
        std::lock_guard<std::mutex> lk(pl.lock);
        for (int d = 0; d < rdr::kMaxDevices; ++d) {
            if (only_dev >= 0 && d != only_dev) continue;
            PoolLists &l = pl.dev.slot[d];
            for (auto &kv : l.free_blocks) gone.push_back({d, kv.second});
            l.free_blocks.clear();
            l.from_driver -= l.parked;
            l.parked = 0;
        }
    }
    if (gone.empty()) return;
    const int dev = current_device();
    int at = dev;
    for (auto &g : gone) {
        if (g.first != at) { (void)hipSetDevice(g.first); at = g.first; }
        (void)hipFree(g.second);
    }
    if (at != dev) (void)hipSetDevice(dev);
}
void pool_trim() { pool_release(-1); }

size_t pool_cached_bytes() {
    Pool &pl = pool();
    std::lock_guard<std::mutex> lk(pl.lock);
    size_t total = 0;
    for (const PoolLists &l : pl.dev) total += l.parked;
    return total;
}

size_t memory_available() {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return ~(size_t)0; }
    Pool &pl = pool();
    PoolLists &mine = pl.dev.at(current_device());
    std::lock_guard<std::mutex> lk(pl.lock);
    return free_b + mine.parked;
}

double memory_held_by_others() {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || total_b == 0) { (void)hipGetLastError(); return 0.0; }
    Pool &pl = pool();
    PoolLists &mine = pl.dev.at(current_device());
    std::lock_guard<std::mutex> lk(pl.lock);
    const double used = (double)(total_b - free_b), held = (double)mine.from_driver;
    return used > held ? (used - held) / (double)total_b : 0.0;
}

size_t pool_device_mallocs() { Pool &pl = pool(); std::lock_guard<std::mutex> lk(pl.lock); return pl.device_mallocs; }

namespace {
struct Staging { char *base = nullptr; size_t cap = 0, used = 0; };
Staging &staging() { static thread_local Staging s; return s; }
char *staging_reserve(size_t bytes) {          // 256-byte aligned slice of the pinned buffer; grows when idle
    Staging &st = staging();
    const size_t need = (bytes + 255) & ~(size_t)255;
    if (st.used + need > st.cap) {
        sync();                                 // nothing in flight may still read the old buffer
        st.used = 0;
        if (need > st.cap) {
            if (st.base) (void)hipHostFree(st.base);
            st.cap = std::max<size_t>(need * 2, (size_t)32 << 20);
            check(hipHostMalloc((void **)&st.base, st.cap, hipHostMallocDefault), "hipHostMalloc (staging)");
        }
    }
    char *p = st.base + st.used;
    st.used += need;
    return p;
}
// Device ints handed out one after the other, round and round: a launch's slot is reused `length` launches later.
struct IntRing {
    int *base = nullptr; int cursor = 0;
    int *next(int length) {
        if (!base) base = (int *)dmalloc(sizeof(int) * length);
        int *p = base + cursor;
        cursor = (cursor + 1) % length;
        return p;
    }
};
// What a host thread keeps on a device, created on first use and kept for the thread's life.
struct ThreadDeviceState {
    CompactScratch compact[2];          // compactions that may be in flight together use different scratch
    hipStream_t side[4] = {};           // side_stream(k)
    IntRing counts, walk_counters;      // new_count, persistent_counter
};
ThreadDeviceState &thread_device_state() {
    static thread_local rdr::PerDevice<ThreadDeviceState> per_device;
    return per_device.at(current_device());
}
}

void upload_async(void *dst, const void *src, size_t bytes) {
    if (!bytes) return;
    char *stage = staging_reserve(bytes);
    std::memcpy(stage, src, bytes);
    check(hipMemcpyAsync(dst, stage, bytes, hipMemcpyHostToDevice, ctx().stream), "upload_async");
}
void upload_flush() { sync(); staging().used = 0; }

void download_batch(const DownloadItem *items, int n) {
    size_t total = 0;
    for (int i = 0; i < n; ++i) total += (items[i].bytes + 255) & ~(size_t)255;
    if (!total) return;
    upload_flush();                              // the staging buffer is shared with queued uploads
    char *stage = staging_reserve(total);
    size_t at = 0;
    for (int i = 0; i < n; ++i) {
        if (items[i].bytes) check(hipMemcpyAsync(stage + at, items[i].src, items[i].bytes, hipMemcpyDeviceToHost, ctx().stream), "download_batch");
        at += (items[i].bytes + 255) & ~(size_t)255;
    }
    sync();
    at = 0;
    for (int i = 0; i < n; ++i) {
        if (items[i].bytes) std::memcpy(items[i].dst, stage + at, items[i].bytes);
        at += (items[i].bytes + 255) & ~(size_t)255;
    }
    staging().used = 0;
}

const void *device_constant(const void *host, size_t bytes) {
    static std::mutex lock;
    static std::map<std::pair<const void *, int>, void *> table;      // (host table, device) -> device copy, kept for the process
    std::lock_guard<std::mutex> lk(lock);
    void *&p = table[{host, current_device()}];
    if (!p) {
        p = dmalloc(bytes);
        check(hipMemcpy(p, host, bytes, hipMemcpyHostToDevice), "device_constant");
    }
    return p;
}

CompactScratch &compact_scratch(int nblocks, int which) {
    CompactScratch &s = thread_device_state().compact[which & 1];
    if (s.capacity < nblocks) {
        if (s.block_counts) (void)hipFree(s.block_counts);
        if (!s.total) {
            void *h = nullptr, *d = nullptr;
            check(hipHostMalloc(&h, 64, hipHostMallocMapped), "hipHostMalloc");
            check(hipHostGetDevicePointer(&d, h, 0), "hipHostGetDevicePointer");
            s.total_host = (volatile int *)h;
            s.total = (int *)d;
            s.total_host[0] = 0; s.total_host[1] = 0;       // [count, ticket of the compaction that wrote it]
        }
        s.capacity = nblocks + 1024;
        s.block_counts = (int *)dmalloc(sizeof(int) * s.capacity);
    }
    return s;
}

hipStream_t side_stream(int k) {
    // k = 0, 1: two non-blocking streams; k = 2, 3: two more at the LOWEST priority.  Where a kernel of the calling stream (a
    // sample's critical path: the continuation-ray traversal, the bounce adjoints) and one of a low-priority side stream
    // (shadow rays, edge picks) both have workgroups waiting, the calling stream's are dispatched first: closest-hit launch
    // 0.334 -> 0.307 ms in the 1024 x 1024 benchmark with the shadow-ray launch beside it, throughput +0.3 %.  Small renders
    // (one wave per SIMD per launch, several samples and the edge builder in flight) lose 20 % that way: render.cpp asks for
    // the low-priority pair only for large frames (RDR_NO_SIDE_PRIORITY=1: never).
    hipStream_t &s = thread_device_state().side[k & 3];
    if (!s) {
        static const bool allowed = std::getenv("RDR_NO_SIDE_PRIORITY") == nullptr;
        int least = 0, greatest = 0;
        if ((k & 2) && allowed && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && least != greatest)
            check(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, least), "hipStreamCreateWithPriority");
        else
            check(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), "hipStreamCreate");
    }
    return s;
}

int *new_count() { return thread_device_state().counts.next(8192); }      // written by the compaction it is handed to: not zeroed

int *persistent_counter() {
    // per host thread and per device; the slot is zeroed ON THE STREAM OF THE LAUNCH that is about to use it.  (Rounds 3-5 zeroed
    // the whole ring once per lap on whatever stream was current then: a kernel launched on ANOTHER stream right after the
    // ring's allocation could read its counter before that fill had run -- harmless while the only user was the gated overflow
    // walk, a wrong pick once in a while as soon as the hierarchical pick's descent took its chunks off such a counter; found as
    // an intermittent failure of the first test after a library load, round 6.)
    int *p = thread_device_state().walk_counters.next(4096);
    check(hipMemsetAsync(p, 0, sizeof(int), ctx().stream), "persistent_counter");
    return p;
}

} // namespace exec
