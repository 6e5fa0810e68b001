// TEST INFRASTRUCTURE: the rule of redner_amd/csrc/arena.h, checked over the counting exec.h of this directory
// (tests/test_capi.py builds this with -fsanitize=address,undefined and runs it).
#include "arena.h"
#include <cstdio>
#include <stdexcept>
#include <type_traits>

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

static_assert(!std::is_copy_constructible<rdr::Arena>::value && !std::is_copy_assignable<rdr::Arena>::value, "an Arena is not copied");
static_assert(!std::is_move_constructible<rdr::Arena>::value, "no user moves an Arena: a moved-from owner does not exist");

int main() {
    exec::Log &log = exec::log();
    {   // leaving the scope normally: every block goes back, nobody waits
        rdr::Arena a;
        int *p = a.get<int>(100);
        double *q = a.get<double>(3);
        p[99] = 1; q[2] = 2.0;
        const float host[4] = {1.f, 2.f, 3.f, 4.f};
        float *r = a.put(host, 4);
        CHECK(r[3] == 4.f && log.uploads == 1);
        char *none = a.put((const char *)nullptr, 0);           // nothing to copy, still a block
        CHECK(none != nullptr && log.uploads == 1);
        CHECK(log.allocs == 4 && log.frees == 0);
    }
    CHECK(log.allocs == 4 && log.frees == 4 && log.syncs == 0 && log.live.empty());

    log = exec::Log();
    {   // a count of 0 still yields a block of its own, released like the rest
        rdr::Arena a;
        int *z = a.get<int>(0), *y = a.get<int>(0);
        CHECK(z && y && z != y);
        z[0] = 7;                                            // at least one element: ASan would object otherwise
    }
    CHECK(log.allocs == 2 && log.frees == 2 && log.syncs == 0 && log.live.empty());

    log = exec::Log();
    try {   // leaving by an exception: one wait for the device, before the first block goes back
        rdr::Arena a;
        a.get<int>(8); a.get<int>(8); a.get<int>(8);
        throw std::runtime_error("a launch failed");
    } catch (const std::exception &) {
    }
    CHECK(log.allocs == 3 && log.frees == 3 && log.syncs == 1 && log.live.empty());
    CHECK(log.last_sync < log.first_free);

    log = exec::Log();
    try {   // ... and an owner with no blocks has nothing to wait for
        rdr::Arena a;
        throw std::runtime_error("nothing was allocated");
    } catch (const std::exception &) {
    }
    CHECK(log.syncs == 0 && log.frees == 0);

    log = exec::Log();
    try {
        throw std::runtime_error("caught");
    } catch (const std::exception &) {
        rdr::Arena a;                                        // made and ended inside a handler: the exception is not in flight
        a.get<int>(1);
    }
    CHECK(log.frees == 1 && log.syncs == 0);

    std::printf("arena rule ok\n");
    return 0;
}
