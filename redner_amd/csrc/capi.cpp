// capi.cpp -- extern "C" entry points declared in include/redner_amd.h.
#include "../../include/redner_amd.h"
#include "render.h"
#include "tuning.h"
#include "trace_plan.h"
#include "edges.h"
#include "deferred.h"
#include "mipmap.h"
#include "vertex_normal.h"
#include "sh_envmap.h"
#include <cstdio>
#include "scene.h"
#include <cstring>
#include <exception>
#include <mutex>
#include <string>
#include <vector>
#include <cstdlib>

namespace {
thread_local std::string g_last_error;
// rdr_render / rdr_scene_create / rdr_scene_trace are serialised PER DEVICE: the reference's render() is not re-entrant either
// (global thread pool, src/parallel.cpp:10-14) but runs with the GIL held; ctypes releases the GIL, and two concurrent calls on
// one device would share its replicated-accumulator symbols, its helper threads and the Scene caches.  Calls on DIFFERENT
// devices run side by side (one host thread per device in one process): every piece of state they touch is per device (buffer
// pool free lists, Scene caches, helper threads, streams, compaction scratch) or per host thread (stream, tuning, staging), and
// what is shared (host thread pool, edge-builder thread, trace statistics) has its own lock.
std::recursive_mutex g_device_lock[16];
std::recursive_mutex &device_lock(int gpu_index) { return g_device_lock[(gpu_index < 0 ? 0 : gpu_index) & 15]; }
void set_error(const char *what) { g_last_error = what ? what : "unknown error"; }
// rdr_set_stream: the stream the calling thread's launches are ordered on (null = the null stream)
thread_local void *g_user_stream = nullptr;
void use_caller_stream() { exec::ctx().stream = (hipStream_t)g_user_stream; }
}

// rdr_debug_libm: one argument per lane through the routines every stage calls
struct LibmProbe {
    int fn; const double *x, *y; double *out;
    RDR_FN void operator()(int i) const {
        const double a = x[i], b = y[i];
        double r;
        switch (fn) {
            case 0: r = gm::sin(a); break;
            case 1: r = gm::cos(a); break;
            case 2: r = gm::atan2(a, b); break;
            case 3: r = gm::atan(a); break;
            case 4: r = gm::acos(a); break;
            case 5: r = gm::log(a); break;
            default: r = gm::pow(a, b); break;
        }
        out[i] = r;
    }
};

// rdr_debug_compact: the predicate is a table look-up of the item's value
struct KeepProbe {
    const uint8_t *keep;
    RDR_FN bool operator()(int v) const { return keep[v] != 0; }
};
// rdr_debug_walk: item i walks len[i] steps and leaves behind how often it was begun and finished, how many steps it took and a
// sum that depends on the item and on every step number -- a lane that resumes with another lane's state shows in `acc`
struct WalkProbe {
    const int *len, *gate;
    int *begun, *finished, *steps_taken; unsigned *acc;
    struct State { int idx, left; unsigned k, acc; };
    RDR_FN bool gate_closed() const { return *gate != 0; }
    RDR_FN bool begin(int item, State &st) const {
        rdr::atomic_fetch_add(&begun[item], 1);
        st.idx = item; st.left = len[item]; st.k = 0; st.acc = 0;
        return st.left > 0;
    }
    RDR_FN bool step(State &st) const {
        st.acc += (unsigned)st.idx * 31u + ++st.k;
        return --st.left == 0;
    }
    RDR_FN void finish(State &st) const {
        rdr::atomic_fetch_add(&finished[st.idx], 1);
        steps_taken[st.idx] = (int)st.k; acc[st.idx] = st.acc;
    }
};
struct WalkProbeLane {             // the same walk as one lane of a plain launch
    WalkProbe w;
    RDR_FN void operator()(int i) const {
        WalkProbe::State st;
        if (w.begin(i, st)) { while (!w.step(st)) {} }
        w.finish(st);
    }
};
namespace {
struct DebugHeld {                 // pool blocks of a test hook: released on every path out, also when a launch or a copy throws
    std::vector<void *> p;
    void *get(size_t bytes) { p.push_back(nullptr); p.back() = exec::pool_alloc(bytes ? bytes : 16); return p.back(); }
    template <class T> T *put(const T *host, size_t n) { T *d = (T *)get(sizeof(T) * n); exec::upload(d, host, sizeof(T) * n); return d; }
    ~DebugHeld() { exec::device_sync(); for (void *q : p) exec::pool_free(q); }
};
constexpr int kDebugMaxItems = 1 << 24;
}
#ifdef RDR_HOSTSIM
// The CPU debugging harness defines the sort hook's body beside its other stand-ins for edges_gpu.cpp (tests/hostsim/
// edges_gpu_stub.cpp); a harness directory that predates the hook still links and loads, and the hook says what is missing.
namespace rdr {
__attribute__((weak)) void debug_sort_pairs(const uint64_t *, const int32_t *, int, uint64_t *, int32_t *) {
    throw std::runtime_error("rdr_debug_sort_pairs: this harness build has no stand-in for the sort");
}
}
#endif

extern "C" {

const char *rdr_last_error(void) { return g_last_error.c_str(); }

rdr_scene *rdr_scene_create(const rdr_camera_desc *camera, const rdr_shape_desc *shapes, int num_shapes,
                            const rdr_material_desc *materials, int num_materials,
                            const rdr_area_light_desc *area_lights, int num_area_lights,
                            const rdr_envmap_desc *envmap, int use_gpu, int gpu_index,
                            int use_primary_edge_sampling, int use_secondary_edge_sampling) {
    try {
        g_last_error.clear();
        std::lock_guard<std::recursive_mutex> lk(device_lock(gpu_index));
        use_caller_stream();
        return reinterpret_cast<rdr_scene *>(rdr::create_scene(camera, shapes, num_shapes, materials, num_materials,
                                                               area_lights, num_area_lights, envmap, use_gpu, gpu_index,
                                                               use_primary_edge_sampling, use_secondary_edge_sampling));
    } catch (const std::exception &e) {
        set_error(e.what());
        return nullptr;
    }
}

void rdr_scene_destroy(rdr_scene *scene) {
    if (!scene) return;
    rdr::Scene *s = reinterpret_cast<rdr::Scene *>(scene);
    // under the device's lock like every other call that touches its pool / caches (the destructor returns buffers and may join
    // the Scene's edge build)
    std::lock_guard<std::recursive_mutex> lk(device_lock(s->gpu_index));
    delete s;
}

int rdr_scene_max_generic_texture_dimension(const rdr_scene *scene) {
    return scene ? reinterpret_cast<const rdr::Scene *>(scene)->max_generic_texture_dimension : 0;
}

int rdr_render(const rdr_scene *scene, const rdr_render_options *options, float *rendered_image,
               const float *d_rendered_image, const rdr_dscene_desc *d_scene, float *screen_gradient_image,
               float *debug_image) {
    try {
        g_last_error.clear();
        if (!scene || !options) throw std::runtime_error("rdr_render: scene and options are required");
        const rdr::Scene &s = *reinterpret_cast<const rdr::Scene *>(scene);
        std::lock_guard<std::recursive_mutex> lk(device_lock(s.gpu_index));
        exec::select_device(1, s.gpu_index);
        use_caller_stream();
        rdr::render(s, *options, rendered_image, d_rendered_image, d_scene, screen_gradient_image, debug_image);
        return 0;
    } catch (const std::exception &e) {
        set_error(e.what());
        return 1;
    }
}

int rdr_deferred_shade(const rdr_deferred_desc *desc, const float *g_buffer, const float *light_params, float *image) {
    try {
        g_last_error.clear();
        if (!desc) throw std::runtime_error("rdr_deferred_shade: a description is required");
        std::lock_guard<std::recursive_mutex> lk(device_lock(desc->gpu_index));
        exec::select_device(desc->gpu_index >= 0, desc->gpu_index);
        use_caller_stream();
        rdr::dfr::shade(*desc, g_buffer, light_params, image);
        return 0;
    } catch (const std::exception &e) {
        set_error(e.what());
        return 1;
    }
}

int rdr_deferred_shade_backward(const rdr_deferred_desc *desc, const float *g_buffer, const float *light_params,
                                const float *d_image, float *d_g_buffer, float *d_light_params) {
    try {
        g_last_error.clear();
        if (!desc) throw std::runtime_error("rdr_deferred_shade_backward: a description is required");
        std::lock_guard<std::recursive_mutex> lk(device_lock(desc->gpu_index));
        exec::select_device(desc->gpu_index >= 0, desc->gpu_index);
        use_caller_stream();
        rdr::dfr::shade_backward(*desc, g_buffer, light_params, d_image, d_g_buffer, d_light_params);
        return 0;
    } catch (const std::exception &e) {
        set_error(e.what());
        return 1;
    }
}

int rdr_mip_num_levels(int height, int width) { return height > 0 && width > 0 ? rdr::mip::num_levels(height, width) : 0; }

int64_t rdr_mip_backward_scratch(int height, int width, int channels) {
    try {
        g_last_error.clear();
        return (int64_t)rdr::mip::scratch_floats(rdr::mip::make_shape(height, width, channels, rdr_mip_num_levels(height, width),
                                                                      "rdr_mip_backward_scratch"));
    } catch (const std::exception &e) {
        set_error(e.what());
        return -1;
    }
}

int rdr_mip_tiled_stages(int height, int width, int channels) {
    try {
        g_last_error.clear();
        return rdr::mip::tiled_stages(rdr::mip::make_shape(height, width, channels, rdr_mip_num_levels(height, width),
                                                           "rdr_mip_tiled_stages"));
    } catch (const std::exception &e) {
        set_error(e.what());
        return -1;
    }
}

// the product library reads and writes device memory only; host pointers are for the CPU debugging harness
static void mip_select(int gpu_index, const char *who) {
#if !defined(RDR_HOSTSIM)
    if (gpu_index < 0) throw std::runtime_error(std::string(who) + ": host memory (negative gpu_index) is for the CPU harness only");
#endif
    exec::select_device(gpu_index >= 0, gpu_index);
    use_caller_stream();
}

int rdr_mip_pyramid(int height, int width, int channels, int num_levels, float *const *levels, int gpu_index) {
    try {
        g_last_error.clear();
        std::lock_guard<std::recursive_mutex> lk(device_lock(gpu_index));
        mip_select(gpu_index, "rdr_mip_pyramid");
        rdr::mip::pyramid(height, width, channels, num_levels, levels);
        return 0;
    } catch (const std::exception &e) {
        set_error(e.what());
        return 1;
    }
}

int rdr_mip_pyramid_backward(int height, int width, int channels, int num_levels, const float *const *d_levels, float *d_texels,
                             float *scratch, int64_t scratch_floats, int gpu_index) {
    try {
        g_last_error.clear();
        std::lock_guard<std::recursive_mutex> lk(device_lock(gpu_index));
        mip_select(gpu_index, "rdr_mip_pyramid_backward");
        rdr::mip::pyramid_backward(height, width, channels, num_levels, d_levels, d_texels, scratch,
                                   scratch_floats > 0 ? (size_t)scratch_floats : 0);
        return 0;
    } catch (const std::exception &e) {
        set_error(e.what());
        return 1;
    }
}

// ---- SH reconstruction and the sampling tables of an environment map (csrc/sh_envmap.h) ----
int64_t rdr_sh_backward_scratch(int height, int width, int channels, int num_coeffs) {
    try {
        g_last_error.clear();
        return (int64_t)rdr::shenv::scratch_floats(rdr::shenv::make_plan(height, width, channels, num_coeffs, "rdr_sh_backward_scratch"));
    } catch (const std::exception &e) {
        set_error(e.what());
        return -1;
    }
}

int rdr_sh_reconstruct(const float *coeffs, int channels, int num_coeffs, int height, int width, float *image, uint8_t *clamp,
                       int gpu_index) {
    try {
        g_last_error.clear();
        std::lock_guard<std::recursive_mutex> lk(device_lock(gpu_index));
        mip_select(gpu_index, "rdr_sh_reconstruct");
        rdr::shenv::reconstruct(height, width, channels, num_coeffs, coeffs, image, clamp);
        return 0;
    } catch (const std::exception &e) {
        set_error(e.what());
        return 1;
    }
}

int rdr_sh_reconstruct_backward(const uint8_t *clamp, const float *d_image, int channels, int num_coeffs, int height, int width,
                                float *d_coeffs, float *scratch, int64_t scratch_floats, int gpu_index) {
    try {
        g_last_error.clear();
        std::lock_guard<std::recursive_mutex> lk(device_lock(gpu_index));
        mip_select(gpu_index, "rdr_sh_reconstruct_backward");
        rdr::shenv::reconstruct_backward(height, width, channels, num_coeffs, clamp, d_image, d_coeffs, scratch,
                                         scratch_floats > 0 ? (size_t)scratch_floats : 0);
        return 0;
    } catch (const std::exception &e) {
        set_error(e.what());
        return 1;
    }
}

int rdr_envmap_tables(const float *texels, const float *y_weight, int height, int width, float *sample_cdf_ys, float *sample_cdf_xs,
                      float *total, int gpu_index) {
    try {
        g_last_error.clear();
        std::lock_guard<std::recursive_mutex> lk(device_lock(gpu_index));
        mip_select(gpu_index, "rdr_envmap_tables");
        rdr::shenv::tables(height, width, texels, y_weight, sample_cdf_ys, sample_cdf_xs, total);
        return 0;
    } catch (const std::exception &e) {
        set_error(e.what());
        return 1;
    }
}

// ---- vertex normals (csrc/vertex_normal.h) ----
static const rdr::vnrm::Topology &topology_of(const rdr_mesh_topology *topology, const char *who) {
    if (!topology) throw std::runtime_error(std::string(who) + ": a topology is required");
    return *reinterpret_cast<const rdr::vnrm::Topology *>(topology);
}

rdr_mesh_topology *rdr_mesh_topology_create(const int *indices, int num_triangles, int num_vertices, int use_gpu, int gpu_index) {
    try {
        g_last_error.clear();
        const int place = use_gpu ? (gpu_index < 0 ? 0 : gpu_index) : -1;
        std::lock_guard<std::recursive_mutex> lk(device_lock(place));
        mip_select(place, "rdr_mesh_topology_create");
        return reinterpret_cast<rdr_mesh_topology *>(rdr::vnrm::create_topology(indices, num_triangles, num_vertices, place));
    } catch (const std::exception &e) {
        set_error(e.what());
        return nullptr;
    }
}

void rdr_mesh_topology_destroy(rdr_mesh_topology *topology) {
    if (!topology) return;
    rdr::vnrm::Topology *t = reinterpret_cast<rdr::vnrm::Topology *>(topology);
    std::lock_guard<std::recursive_mutex> lk(device_lock(t->gpu_index));
    try { exec::select_device(t->gpu_index >= 0, t->gpu_index); } catch (const std::exception &) {}
    delete t;
}

int rdr_mesh_topology_read(const rdr_mesh_topology *topology, int *offsets, int *corners) {
    try {
        g_last_error.clear();
        const rdr::vnrm::Topology &t = topology_of(topology, "rdr_mesh_topology_read");
        std::lock_guard<std::recursive_mutex> lk(device_lock(t.gpu_index));
        mip_select(t.gpu_index, "rdr_mesh_topology_read");
        rdr::vnrm::read_topology(t, offsets, corners);
        return 0;
    } catch (const std::exception &e) {
        set_error(e.what());
        return 1;
    }
}

int rdr_vertex_normal_scratch(const rdr_mesh_topology *topology, int scheme, int64_t *forward_floats, int64_t *backward_floats,
                              int64_t *saved_floats) {
    try {
        g_last_error.clear();
        const rdr::vnrm::Topology &t = topology_of(topology, "rdr_vertex_normal_scratch");
        const bool cot = rdr::vnrm::cotangent(scheme, "rdr_vertex_normal_scratch");
        if (forward_floats) *forward_floats = (int64_t)rdr::vnrm::forward_scratch_floats(t, cot);
        if (backward_floats) *backward_floats = (int64_t)rdr::vnrm::backward_scratch_floats(t, cot);
        if (saved_floats) *saved_floats = (int64_t)rdr::vnrm::saved_floats(t, cot);
        return 0;
    } catch (const std::exception &e) {
        set_error(e.what());
        return 1;
    }
}

int rdr_vertex_normal(const rdr_mesh_topology *topology, int scheme, const float *vertices, float *normals, float *saved,
                      float *scratch, int64_t scratch_floats) {
    try {
        g_last_error.clear();
        const rdr::vnrm::Topology &t = topology_of(topology, "rdr_vertex_normal");
        std::lock_guard<std::recursive_mutex> lk(device_lock(t.gpu_index));
        mip_select(t.gpu_index, "rdr_vertex_normal");
        rdr::vnrm::forward(t, scheme, vertices, normals, saved, scratch, scratch_floats > 0 ? (size_t)scratch_floats : 0);
        return 0;
    } catch (const std::exception &e) {
        set_error(e.what());
        return 1;
    }
}

int rdr_vertex_normal_backward(const rdr_mesh_topology *topology, int scheme, const float *vertices, const float *saved,
                               const float *d_normals, float *d_vertices, float *scratch, int64_t scratch_floats) {
    try {
        g_last_error.clear();
        const rdr::vnrm::Topology &t = topology_of(topology, "rdr_vertex_normal_backward");
        std::lock_guard<std::recursive_mutex> lk(device_lock(t.gpu_index));
        mip_select(t.gpu_index, "rdr_vertex_normal_backward");
        rdr::vnrm::backward(t, scheme, vertices, saved, d_normals, d_vertices, scratch, scratch_floats > 0 ? (size_t)scratch_floats : 0);
        return 0;
    } catch (const std::exception &e) {
        set_error(e.what());
        return 1;
    }
}

int rdr_compute_num_channels(const int *channels, int num_channels, int max_generic_texture_dimension) {
    return rdr::compute_num_channels(channels, num_channels, max_generic_texture_dimension);
}

void rdr_trace_stats_enable(int timing, int counting) {
    exec::trace_stats().timing = timing != 0;
    exec::trace_stats().counting = counting != 0;
}
void rdr_trace_stats_reset(void) {
    exec::TraceStats &s = exec::trace_stats();
    bool t = s.timing, c = s.counting;
    exec::trace_stats_collect();
    s = exec::TraceStats();
    s.timing = t; s.counting = c;
}
void rdr_trace_stats_get(rdr_trace_stats *out) {
    exec::trace_stats_collect();
    const exec::TraceStats &s = exec::trace_stats();
    out->closest_ms = s.closest_ms; out->any_ms = s.any_ms;
    out->closest_launches = s.closest_launches; out->any_launches = s.any_launches;
    out->closest_rays = s.closest_rays; out->any_rays = s.any_rays;
    out->closest_nodes = s.nodes[0]; out->closest_tris = s.tris[0];
    out->any_nodes = s.nodes[1]; out->any_tris = s.tris[1];
    out->closest_wide_nodes = s.wide_nodes[0]; out->any_wide_nodes = s.wide_nodes[1];
    out->closest_union_ms = s.closest_union_ms; out->any_union_ms = s.any_union_ms;
}

uint64_t rdr_trim_cache(void) {
    std::unique_lock<std::recursive_mutex> all[16];                 // every device, in index order (a call holds one lock only)
    for (int d = 0; d < 16; ++d) all[d] = std::unique_lock<std::recursive_mutex>(g_device_lock[d]);
    rdr::drop_edge_cache();            // the last Scene's edge structures, kept for the next one (scene.cpp: EdgeCache)
    const uint64_t bytes = exec::pool_cached_bytes();
    exec::pool_trim();
    return bytes;
}

void rdr_set_stream(void *hip_stream) { g_user_stream = hip_stream; }
void rdr_set_pool_cap_mb(int64_t megabytes) { exec::pool_set_cap(megabytes < 0 ? -1 : (long long)megabytes << 20); }
int64_t rdr_get_pool_cap_mb(void) { return (int64_t)(exec::pool_cap_bytes() >> 20); }
void rdr_set_build_flags(unsigned flags) { rdr::build_flags_ref().store(flags); }

void rdr_debug_counters_get(rdr_debug_counters *out) {
    out->device_mallocs = exec::pool_device_mallocs();
    out->host_count_reads = exec::host_count_reads();
    out->last_batch_samples = (uint64_t)rdr::last_schedule()[0].load();
    out->last_workers = (uint64_t)rdr::last_schedule()[1].load();
}

int rdr_debug_dump_edges(const rdr_scene *scene, const char *path) {
    const rdr::Scene &s = *reinterpret_cast<const rdr::Scene *>(scene);
    FILE *f = fopen(path, "w");
    if (!f) return 1;
    {
        std::lock_guard<std::recursive_mutex> lk(device_lock(s.gpu_index));
        exec::select_device(1, s.gpu_index);
        try { s.edge_data(); } catch (const std::exception &e) { set_error(e.what()); fclose(f); return 1; }
    }
    if (!s.edges) { fprintf(f, "edges 0\n"); fclose(f); return 0; }
    if (s.edges->device_trees) {
        std::lock_guard<std::recursive_mutex> lk(device_lock(s.gpu_index));
        try { rdr::download_edge_trees(*s.edges); } catch (const std::exception &e) { set_error(e.what()); fclose(f); return 1; }
    }
    const rdr::EdgeData &ed = *s.edges;
    fprintf(f, "edges %d\n", (int)ed.edges.size());
    for (const rdr::EdgeD &e : ed.edges) fprintf(f, "%d %d %d %d %d\n", e.shape_id, e.v0, e.v1, e.f0, e.f1);
    if (!ed.cs_nodes.empty() || !ed.ncs_nodes.empty()) {
        fprintf(f, "expand %.17g\n", ed.edge_bounds_expand);
        for (int t = 0; t < 2; ++t) {
            const std::vector<rdr::EdgeNode> &nodes = t == 0 ? ed.cs_nodes : ed.ncs_nodes;
            int nl = t == 0 ? ed.cs_leaves : ed.ncs_leaves;
            int nn = (int)nodes.size() - nl;
            fprintf(f, "%s %d %d\n", t == 0 ? "cs" : "ncs", nl == 0 ? 0 : nn, nl);
            for (size_t i = 0; i < nodes.size(); ++i) {
                const rdr::EdgeNode &n = nodes[i];
                fprintf(f, "%d %d %d %d %d %.17g %.17g", (int)i, n.parent, n.child0, n.child1, n.edge_id, n.wlen, n.cost);
                fprintf(f, " %.17g %.17g %.17g %.17g %.17g %.17g", n.p_min.x, n.p_min.y, n.p_min.z, n.p_max.x, n.p_max.y, n.p_max.z);
                if (t == 1) fprintf(f, " %.17g %.17g %.17g %.17g %.17g %.17g", n.d_min.x, n.d_min.y, n.d_min.z, n.d_max.x, n.d_max.y, n.d_max.z);
                fprintf(f, "\n");
            }
        }
    }
    fclose(f);
    return 0;
}

/* Test hook: the hierarchy this Scene's kernels built against the host builder's (bvh.cpp) on the same mesh arrays -- node
 * records, leaf order, triangle records, 4-wide records.  Returns the number of records that differ (0: identical), or -1
 * when the Scene's hierarchy is a refit of an earlier build / was not built by kernels. */
int rdr_debug_bvh_check(const rdr_scene *scene) {
    try {
        const rdr::Scene &s = *reinterpret_cast<const rdr::Scene *>(scene);
        if (!s.bvh_dev || s.bvh_dev->parent) return -1;
        std::lock_guard<std::recursive_mutex> lk(device_lock(s.gpu_index));
        exec::select_device(1, s.gpu_index);
        use_caller_stream();
        std::vector<rt::MeshView> meshes(s.shapes.size());
        for (size_t i = 0; i < s.shapes.size(); ++i) meshes[i] = rt::MeshView{s.h_vertices[i].data(), s.h_indices[i].data(), s.shapes[i].num_triangles};
        const rt::BvhHost h = rt::build_bvh(meshes);
        const rt::BvhDev &d = *s.bvh_dev;
        int bad = 0;
        if ((int)h.nodes.size() != d.num_nodes || (int)h.ids.size() != 2 * d.num_slots || (int)h.wide.size() != d.num_wide ||
            h.depth != d.depth || h.wide_stack_need != d.wide_stack_need)
            return 1000000 + std::abs((int)h.nodes.size() - d.num_nodes);
        std::vector<rt::Node> nodes(d.num_nodes);
        std::vector<int> ids((size_t)2 * d.num_slots);
        std::vector<float> tris((size_t)9 * d.num_slots);
        std::vector<rt::Node4> wide(d.num_wide);
        exec::download(nodes.data(), d.nodes, sizeof(rt::Node) * nodes.size());
        exec::download(ids.data(), d.ids, sizeof(int) * ids.size());
        exec::download(tris.data(), d.tris, sizeof(float) * tris.size());
        exec::download(wide.data(), d.wide, sizeof(rt::Node4) * wide.size());
        for (size_t i = 0; i < nodes.size(); ++i) {
            const rt::Node &a = nodes[i], &b = h.nodes[i];
            bool same = a.a == b.a && a.b == b.b;
            for (int k = 0; k < 3; ++k) same = same && a.lo[k] == b.lo[k] && a.hi[k] == b.hi[k];
            bad += !same;
        }
        for (size_t i = 0; i < ids.size(); ++i) bad += ids[i] != h.ids[i];
        for (size_t i = 0; i < tris.size(); ++i) bad += !(tris[i] == h.tris[i]);
        for (size_t i = 0; i < wide.size(); ++i) {
            const rt::Node4 &a = wide[i], &b = h.wide[i];
            bool same = a.aux[0] == b.aux[0];
            for (int k = 0; k < 4; ++k)
                same = same && a.link[k] == b.link[k] && a.lox[k] == b.lox[k] && a.loy[k] == b.loy[k] && a.loz[k] == b.loz[k] &&
                       a.hix[k] == b.hix[k] && a.hiy[k] == b.hiy[k] && a.hiz[k] == b.hiz[k];
            bad += !same;
        }
        return bad;
    } catch (const std::exception &e) {
        set_error(e.what());
        return -2;
    }
}

int rdr_scene_trace(const rdr_scene *scene, const float *rays, int32_t *hits, int num_rays, int any_hit) {
    try {
        g_last_error.clear();
        const rdr::Scene &s = *reinterpret_cast<const rdr::Scene *>(scene);
        std::lock_guard<std::recursive_mutex> lk(device_lock(s.gpu_index));
        exec::select_device(1, s.gpu_index);
        use_caller_stream();
        exec::trace(s.bvh, reinterpret_cast<const rt::RayRec *>(rays), reinterpret_cast<rt::HitRec *>(hits), num_rays, any_hit != 0);
        exec::sync();
        return 0;
    } catch (const std::exception &e) {
        set_error(e.what());
        return 1;
    }
}

/* Test hooks: the launch exec::trace() would make (trace_plan.h) -- for stated sizes of a hierarchy, and for a Scene's own.
 * Host arithmetic only: no device is selected or touched. */
static int write_trace_plan(const exec::TraceFacts &facts, int num_rays, int any_hit, int coherent, int counting,
                            const rdr_tuning *tuning, int32_t *out) {
    try {
        g_last_error.clear();
        if (num_rays <= 0 || !out || facts.num_nodes < 0 || facts.stack_need < 0 || facts.wide_stack_need < 0)
            throw std::runtime_error("rdr_debug_trace_plan: bad arguments");
        const exec::TracePlan p = exec::plan_trace(facts, num_rays, any_hit != 0, coherent != 0, counting != 0, rdr::resolve_tuning(tuning));
        const int32_t v[10] = {(int32_t)p.form, p.stack, p.short_index, p.stage_top, p.sorted, p.counting, p.blocks, p.rays_per_lane, p.idle_min, p.steps};
        std::memcpy(out, v, sizeof(v));
        return 0;
    } catch (const std::exception &e) {
        set_error(e.what());
        return 1;
    }
}
int rdr_debug_trace_plan(int num_nodes, int stack_need, int has_wide, int wide_stack_need, int num_rays, int any_hit, int coherent,
                         int counting, const rdr_tuning *tuning, int32_t *out) {
    return write_trace_plan(exec::TraceFacts{num_nodes, stack_need, wide_stack_need, has_wide != 0}, num_rays, any_hit, coherent, counting, tuning, out);
}
int rdr_debug_scene_trace_plan(const rdr_scene *scene, int num_rays, int any_hit, int coherent, int counting, const rdr_tuning *tuning,
                               int32_t *out) {
    if (!scene) { set_error("rdr_debug_scene_trace_plan: bad arguments"); return 1; }
    return write_trace_plan(exec::trace_facts(reinterpret_cast<const rdr::Scene *>(scene)->bvh), num_rays, any_hit, coherent, counting, tuning, out);
}

/* Test hook: the library's transcendental routines (libm_exact.h) evaluated by a kernel on `n` arguments (HOST pointers;
 * `y` only for the two-argument functions).  fn: 0 sin, 1 cos, 2 atan2(x, y), 3 atan, 4 acos, 5 log, 6 pow(x, y). */
int rdr_debug_libm(int fn, const double *x, const double *y, double *out, int n) {
    try {
        g_last_error.clear();
        if (fn < 0 || fn > 6 || n < 0) throw std::runtime_error("rdr_debug_libm: bad arguments");
        std::lock_guard<std::recursive_mutex> lk(device_lock(exec::current_device()));
        exec::select_device(1, exec::current_device());        // the calling thread's device: checked, not changed
        use_caller_stream();
        const size_t bytes = sizeof(double) * (size_t)n;
        struct Held {                      // released on every path out, also when the launch or a copy throws
            double *p[3] = {nullptr, nullptr, nullptr};
            ~Held() { exec::device_sync(); for (double *q : p) exec::dfree(q); }
        } held;
        for (double *&q : held.p) q = (double *)exec::dmalloc(bytes);
        double *dx = held.p[0], *dy = held.p[1], *dout = held.p[2];
        exec::upload(dx, x, bytes);
        if (y) exec::upload(dy, y, bytes); else exec::zero(dy, bytes);
        exec::launch(exec::Count(n), LibmProbe{fn, dx, dy, dout});
        exec::download(out, dout, bytes);
        exec::sync();
        return 0;
    } catch (const std::exception &e) {
        set_error(e.what());
        return 1;
    }
}

/* Test hook: the gradient store of a render, one stage that calls the scatter functions, the fold (render.cpp: debug_grad_scatter). */
int rdr_debug_grad_scatter(const rdr_scene *scene, const rdr_dscene_desc *d_scene, uint64_t job_samples, int op, int plain,
                           int num_lanes, const uint8_t *active, const int32_t *target, const int32_t *index,
                           const double *values) {
    try {
        g_last_error.clear();
        if (!scene || !d_scene) throw std::runtime_error("rdr_debug_grad_scatter: scene and d_scene are required");
        const rdr::Scene &s = *reinterpret_cast<const rdr::Scene *>(scene);
        std::lock_guard<std::recursive_mutex> lk(device_lock(s.gpu_index));
        exec::select_device(1, s.gpu_index);
        use_caller_stream();
        rdr::debug_grad_scatter(s, *d_scene, (size_t)job_samples, op, plain != 0, num_lanes, active, target, index, values);
        return 0;
    } catch (const std::exception &e) {
        set_error(e.what());
        return 1;
    }
}

/* Test hook: one stream compaction as render.cpp calls it (count on the host or on the device, appended, with positions, with the
 * edge sampler's counter, on the second scratch) or the host-visible form. */
int rdr_debug_compact(int upper, int count, const int32_t *in, const uint8_t *keep, int keep_len, int append_upper, int append_count,
                      int dyn_inc, int scratch, int host_form, int32_t *out, int32_t *pos_out, int32_t *result) {
    try {
        g_last_error.clear();
        const auto bad = [](const std::string &what) { throw std::runtime_error("rdr_debug_compact: " + what); };
        if (upper < 0 || upper > kDebugMaxItems) bad("upper out of range");
        if (!keep || keep_len < 0 || keep_len > kDebugMaxItems || !out || !result) bad("keep, out and result are required");
        if (count > kDebugMaxItems + 64) bad("count out of range");
        if (in) {
            for (int i = 0; i < upper; ++i) if (in[i] < 0 || in[i] >= keep_len) bad("value outside the keep table (item " + std::to_string(i) + ")");
        } else if (keep_len < upper) bad("the keep table is shorter than the identity list");
        const bool append = append_upper >= 0;
        if (append_upper > kDebugMaxItems) bad("append_upper out of range");
        if (append && (append_count < 0 || append_count > append_upper)) bad("append_count outside [0, append_upper]");
        if (scratch != 0 && scratch != 1) bad("scratch must be 0 or 1");
        if (host_form != 0 && host_form != 1) bad("host_form must be 0 or 1");
        if (host_form && (count >= 0 || append || dyn_inc != 0 || pos_out || scratch != 0))
            bad("the host form takes a host count, no append, no dyn, no pos_out, scratch 0");
        std::lock_guard<std::recursive_mutex> lk(device_lock(exec::current_device()));
        exec::select_device(1, exec::current_device());        // the calling thread's device: checked, not changed
        use_caller_stream();
        DebugHeld held;
        const size_t out_len = (size_t)(append ? append_upper : 0) + (size_t)upper;
        const int *d_in = in ? held.put(in, (size_t)upper) : nullptr;
        const uint8_t *d_keep = held.put(keep, (size_t)keep_len);
        int *d_out = held.put(out, out_len);
        int *d_pos = pos_out ? held.put(pos_out, out_len) : nullptr;
        const int *d_count = count >= 0 ? held.put(&count, 1) : nullptr;
        const int *d_append = append ? held.put(&append_count, 1) : nullptr;
        int *d_dyn = dyn_inc != 0 ? held.put(&result[2], 1) : nullptr;
        const exec::Count n = d_count ? exec::Count(d_count, upper) : exec::Count(upper);
        const exec::Count at(d_append, append ? append_upper : 0);
        const KeepProbe pred{d_keep};
        int32_t r[4] = {0, 0, result[2], -1};
        if (host_form) {
            r[3] = exec::compact(d_in, upper, d_out, pred);
            r[0] = r[3]; r[1] = upper;
        } else {
            const exec::Count got = exec::compact_dev(d_in, n, d_out, pred, append ? &at : nullptr, d_dyn, dyn_inc, d_pos, scratch);
            r[1] = got.upper;
            if (got.dev) exec::download(&r[0], got.dev, sizeof(int)); else r[0] = got.upper;
        }
        if (d_dyn) exec::download(&r[2], d_dyn, sizeof(int));
        exec::download(out, d_out, sizeof(int) * out_len);
        if (d_pos) exec::download(pos_out, d_pos, sizeof(int) * out_len);
        exec::sync();
        std::memcpy(result, r, sizeof(r));
        return 0;
    } catch (const std::exception &e) {
        set_error(e.what());
        return 1;
    }
}

/* Test hook: the walk kernels with lane refill (and the plain launch) over a walker whose every begin, step and finish is counted. */
int rdr_debug_walk(int kind, int upper, int count, const int32_t *len, int items_per_lane, int idle_min, int steps, int gate_closed,
                   int repeat, int32_t *begun, int32_t *finished, int32_t *steps_taken, uint32_t *acc) {
    try {
        g_last_error.clear();
        const auto bad = [](const std::string &what) { throw std::runtime_error("rdr_debug_walk: " + what); };
        if (kind < 0 || kind > 2) bad("unknown kind");
        if (upper < 0 || upper > kDebugMaxItems) bad("upper out of range");
        if (count > kDebugMaxItems + 64) bad("count out of range");
        if (!len || !begun || !finished || !steps_taken || !acc) bad("a per-item array is missing");
        for (int i = 0; i < upper; ++i) if (len[i] < 0 || len[i] > 65536) bad("walk length outside [0, 65536] (item " + std::to_string(i) + ")");
        // what resolve_tuning (tuning.h) clamps to; items_per_lane = 0 would hand out empty chunks for ever
        if (items_per_lane < 1 || items_per_lane > 64) bad("items_per_lane outside [1, 64]");
        if (idle_min < 1 || idle_min > 64) bad("idle_min outside [1, 64]");
        if (steps < 1 || steps > 1024) bad("steps outside [1, 1024]");
        if (gate_closed != 0 && (gate_closed != 1 || kind != 0)) bad("gate_closed is 0, or 1 with kind 0");
        if (repeat < 1 || repeat > 65536) bad("repeat outside [1, 65536]");
        std::lock_guard<std::recursive_mutex> lk(device_lock(exec::current_device()));
        exec::select_device(1, exec::current_device());        // the calling thread's device: checked, not changed
        use_caller_stream();
        DebugHeld held;
        const size_t n = (size_t)upper;
        WalkProbe w;
        w.len = held.put(len, n);
        w.gate = held.put(&gate_closed, 1);
        w.begun = held.put(begun, n); w.finished = held.put(finished, n); w.steps_taken = held.put(steps_taken, n);
        w.acc = held.put(acc, n);
        const int *d_count = count >= 0 ? held.put(&count, 1) : nullptr;
        const exec::Count c = d_count ? exec::Count(d_count, upper) : exec::Count(upper);
        for (int r = 0; r < repeat; ++r) {
            if (kind == 0) exec::launch_persistent(c, w);
            else if (kind == 1) exec::launch_chunked(c, w, items_per_lane, idle_min, steps);
            else exec::launch(c, WalkProbeLane{w});
        }
        exec::download(begun, w.begun, sizeof(int) * n);
        exec::download(finished, w.finished, sizeof(int) * n);
        exec::download(steps_taken, w.steps_taken, sizeof(int) * n);
        exec::download(acc, w.acc, sizeof(unsigned) * n);
        exec::sync();
        return 0;
    } catch (const std::exception &e) {
        set_error(e.what());
        return 1;
    }
}

/* Test hook: the stable radix sort of (64-bit code, edge id) pairs (edges_gpu.cpp: debug_sort_pairs). */
int rdr_debug_sort_pairs(const uint64_t *keys, const int32_t *vals, int n, uint64_t *keys_out, int32_t *vals_out) {
    try {
        g_last_error.clear();
        if (n < 1 || n > kDebugMaxItems) throw std::runtime_error("rdr_debug_sort_pairs: n outside [1, 2^24]");
        if (!keys || !vals || !keys_out || !vals_out) throw std::runtime_error("rdr_debug_sort_pairs: an array is missing");
        std::lock_guard<std::recursive_mutex> lk(device_lock(exec::current_device()));
        exec::select_device(1, exec::current_device());        // the calling thread's device: checked, not changed
        use_caller_stream();
        rdr::debug_sort_pairs(keys, vals, n, keys_out, vals_out);
        return 0;
    } catch (const std::exception &e) {
        set_error(e.what());
        return 1;
    }
}

} // extern "C"
