// TEST INFRASTRUCTURE: what redner_amd/csrc/arena.h needs of exec.h, counted (tests/arena/arena_rule.cpp).  Every call gets
// the next number of one clock, so the order of a wait and the first release can be told.
#pragma once
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <set>
namespace exec {
struct Log {
    int clock = 0, allocs = 0, frees = 0, syncs = 0, uploads = 0, first_free = 0, last_sync = 0;
    std::set<void *> live;
};
inline Log &log() { static Log l; return l; }
inline void *pool_alloc(size_t bytes) { void *p = std::malloc(bytes); ++log().clock; ++log().allocs; log().live.insert(p); return p; }
inline void pool_free(void *p) {
    if (!log().live.erase(p)) std::abort();          // not a live block of the pool: freed twice, or never handed out
    ++log().clock; if (!log().frees++) log().first_free = log().clock;
    std::free(p);
}
inline void device_sync() { ++log().syncs; log().last_sync = ++log().clock; }
inline void upload_async(void *dst, const void *src, size_t bytes) { ++log().uploads; std::memcpy(dst, src, bytes); }
}
