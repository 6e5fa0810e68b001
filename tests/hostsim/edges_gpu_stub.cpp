// TEST INFRASTRUCTURE: the CPU debugging harness has no kernels, so the two entry points of redner_amd/csrc/edges_gpu.cpp are
// stubs here (exec::kDeviceEdgeTrees is false in the harness's exec.h: they are never reached); the sort's test hook gets the
// definition of what it must compute.
#include "edges.h"
#include <algorithm>
#include <stdexcept>
#include <vector>
namespace rdr {
void build_edge_trees_device(EdgeData &) { throw std::runtime_error("harness: no device edge builder"); }
void download_edge_trees(EdgeData &) { throw std::runtime_error("harness: no device edge builder"); }
void gather_hierarchy_device(EdgeData &) { throw std::runtime_error("harness: no device edge builder"); }
void drop_gather_cache() {}
// rdr_debug_sort_pairs: what the kernels' sort is held to -- a stable sort by key
void debug_sort_pairs(const uint64_t *keys, const int32_t *vals, int n, uint64_t *keys_out, int32_t *vals_out) {
    if (n < 1 || !keys || !vals || !keys_out || !vals_out) throw std::runtime_error("rdr_debug_sort_pairs: bad arguments");
    std::vector<int> order((size_t)n);
    for (int i = 0; i < n; ++i) order[(size_t)i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return keys[a] < keys[b]; });
    for (int i = 0; i < n; ++i) { keys_out[i] = keys[order[(size_t)i]]; vals_out[i] = vals[order[(size_t)i]]; }
}
}

#include "bvh_gpu.h"
namespace rt {
BvhDev::~BvhDev() {}
void build_tri_bvh_device(const void *, const int *, int, const BvhBuildParams &, BvhDev &) { throw std::runtime_error("harness: no device hierarchy builder"); }
void build_box_bvh_device(const float *, int, const BvhBuildParams &, BvhDev &) { throw std::runtime_error("harness: no device hierarchy builder"); }
void refit_tri_bvh_device(const BvhDev &, const void *, BvhDev &) { throw std::runtime_error("harness: no device hierarchy builder"); }
void refit_box_bvh_device(const BvhDev &, const float *, BvhDev &) { throw std::runtime_error("harness: no device hierarchy builder"); }
}
