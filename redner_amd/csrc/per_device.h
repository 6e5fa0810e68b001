// per_device.h -- the one way the library keeps "one T per device": locks, Scene caches, pool free lists, streams, scratch.
// Plain C++ (no HIP include): the product and the CPU debugging harness compile it alike.
//
// at(device) is where a device index ENTERS (the API lock, select_device, the allocation that records a block's device): a
// negative index means host memory, which only the harness accepts, and takes slot 0; an index the table has no slot for is an
// error, never an alias of another device's slot.  Code that runs with an index that has already passed at() -- a block's
// recorded device in pool_free, a handle's own device in its destroyer -- may read `slot` directly: it cannot throw.
#pragma once
#include <stdexcept>
#include <string>

namespace rdr {

constexpr int kMaxDevices = 16;

// The slot of a device index that enters the library; throws for an index without a slot.
inline int device_slot(int device) {
    if (device >= kMaxDevices)
        throw std::runtime_error("redner_amd: device index " + std::to_string(device) + " is out of range: the library keeps state for " +
                                 std::to_string(kMaxDevices) + " devices (indices 0 ... " + std::to_string(kMaxDevices - 1) + ")");
    return device < 0 ? 0 : device;
}

template <class T> struct PerDevice {
    T slot[kMaxDevices] = {};
    T &at(int device) { return slot[device_slot(device)]; }
    T *begin() { return slot; }
    T *end() { return slot + kMaxDevices; }
};

} // namespace rdr
