// TEST INFRASTRUCTURE: the rule of redner_amd/csrc/per_device.h (tests/test_capi.py builds this with
// -fsanitize=address,undefined and runs it).
#include "per_device.h"
#include <climits>
#include <cstdio>
#include <mutex>
#include <string>

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

static_assert(rdr::kMaxDevices == 16, "the documented limit");

// at(index) must throw a runtime_error whose text names the index and the limit
template <class T> static bool refuses(rdr::PerDevice<T> &table, int index) {
    try {
        (void)table.at(index);
    } catch (const std::runtime_error &e) {
        const std::string text = e.what();
        return text.find(std::to_string(index)) != std::string::npos && text.find(std::to_string(rdr::kMaxDevices)) != std::string::npos;
    }
    return false;
}

int main() {
    rdr::PerDevice<int> table;
    for (int d = 0; d < rdr::kMaxDevices; ++d) CHECK(table.at(d) == 0);          // slots start value-initialised
    for (int d = 0; d < rdr::kMaxDevices; ++d) table.at(d) = 100 + d;
    for (int d = 0; d < rdr::kMaxDevices; ++d) CHECK(&table.at(d) == &table.slot[d] && table.slot[d] == 100 + d);

    CHECK(&table.at(0) != &table.at(15));                    // no two indices share a slot ...
    CHECK(table.at(0) == 100 && table.at(15) == 115);
    CHECK(&table.at(-1) == &table.at(0));                    // ... except host memory (negative: the harness), which takes slot 0
    CHECK(&table.at(INT_MIN) == &table.at(0));

    CHECK(refuses(table, 16));                               // the first index without a slot: an error, not device 0
    CHECK(refuses(table, 17));
    CHECK(refuses(table, 32));                               // (what `& 15` sent to slot 0)
    CHECK(refuses(table, INT_MAX));
    for (int d = 0; d < rdr::kMaxDevices; ++d) CHECK(table.slot[d] == 100 + d);  // a refused index touched nothing

    int visited = 0;                                         // iteration: every slot once, in index order
    for (int &v : table) { CHECK(&v == &table.slot[visited]); ++visited; }
    CHECK(visited == rdr::kMaxDevices);
    CHECK(table.end() - table.begin() == rdr::kMaxDevices);

    rdr::PerDevice<std::mutex> locks;                        // a type that is neither copied nor moved
    {
        std::lock_guard<std::mutex> first(locks.at(0)), last(locks.at(15));      // distinct objects: no deadlock
        CHECK(!locks.at(-1).try_lock());                     // -1 is device 0's lock, which is held
        CHECK(locks.at(7).try_lock());
        locks.at(7).unlock();
    }
    CHECK(refuses(locks, 16));
    auto *leaked = new rdr::PerDevice<std::mutex>();         // how the library makes the ones that must outlive exit
    CHECK(leaked->at(3).try_lock());
    leaked->at(3).unlock();
    delete leaked;                                           // (here only: LeakSanitizer)

    std::printf("per-device rule ok\n");
    return 0;
}
