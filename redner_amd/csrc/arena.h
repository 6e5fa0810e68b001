// arena.h -- the one owner of device blocks from the caching allocator (exec::pool_alloc), and the check of the scratch a
// caller brings instead.  Needs of exec.h only pool_alloc / pool_free / device_sync / upload_async, so it compiles against
// hip/exec.h and against the CPU debugging harness's exec.h alike.
//
// THE RULE.  Blocks go back to the pool when the Arena dies, and the pool knows nothing of streams: a block is handed to the
// next caller, on any thread and any stream, the instant it is back.  So the code that owns an Arena has drained every stream
// that used its blocks before the Arena's scope ends -- a download, download_batch, upload_flush or exec::sync() stands just
// above that end.  Only when the Arena dies during stack unwinding, where kernels may still be running, does it wait itself:
// exec::device_sync() once, then the blocks go back.
#pragma once
#include "exec.h"   // resolved by include path, like vecmath.h's
#include <cstddef>
#include <cstdint>
#include <exception>
#include <stdexcept>
#include <string>
#include <vector>

namespace rdr {

struct Arena {
    std::vector<void *> blocks;
    Arena() = default;
    Arena(const Arena &) = delete;
    Arena &operator=(const Arena &) = delete;
    // `count` elements of T; a count of 0 still yields a block of its own
    template <class T> T *get(size_t count) {
        blocks.push_back(nullptr);                // first the slot: a block is never without an owner
        blocks.back() = exec::pool_alloc(sizeof(T) * (count ? count : 1));
        return (T *)blocks.back();
    }
    // ... filled from host memory through the staging buffer of exec::upload_async: QUEUED on the calling thread's stream;
    // `host` is free at once, and the owner ends the batch (exec::upload_flush / download_batch)
    template <class T> T *put(const T *host, size_t count) {
        T *p = get<T>(count);
        if (count) exec::upload_async(p, host, sizeof(T) * count);
        return p;
    }
    ~Arena() {
        if (!blocks.empty() && std::uncaught_exceptions() > 0) exec::device_sync();
        for (void *p : blocks) if (p) exec::pool_free(p);
    }
};

// Scratch the caller allocated (the stream-ordered calls allocate nothing): `need` floats at `scratch`, which holds `have`
inline void need_scratch(const char *who, size_t need, const float *scratch, size_t have, bool aligned_to_8 = false) {
    if (need > 0 && (!scratch || have < need || (aligned_to_8 && ((uintptr_t)scratch & 7) != 0)))
        throw std::runtime_error(std::string(who) + ": scratch of " + std::to_string(need) + " floats" +
                                 (aligned_to_8 ? ", aligned to 8 bytes," : "") + " is required");
}

} // namespace rdr
