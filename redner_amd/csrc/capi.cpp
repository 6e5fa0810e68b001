// capi.cpp -- extern "C" entry points declared in include/redner_amd.h.
#include "../../include/redner_amd.h"
#include "../../include/redner_amd_debug.h"
#include "render.h"
#include "tuning.h"
#include "trace_plan.h"
#include "edges.h"
#include "deferred.h"
#include "deferred_specular_abi.h"
#include "deferred_specular.h"
#include "deferred_quad_abi.h"
#include "deferred_quad.h"
#include "deferred_quad_shadow_abi.h"
#include "deferred_quad_shadow.h"
#include "mipmap.h"
#include "vertex_normal.h"
#include "mesh_smooth.h"
#include "sh_envmap.h"
#include "pyramid_loss.h"
#include "pose.h"
#include <algorithm>
#include <cstdio>
#include "scene.h"
#include <cstring>
#include <exception>
#include <memory>
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
rdr::PerDevice<std::recursive_mutex> g_device_lock;
std::recursive_mutex &device_lock(int gpu_index) { return g_device_lock.at(gpu_index); }      // where a caller's index enters: may throw
// ... of a handle's own device, for its destroyer: the index passed device_lock when the handle was made, nothing can throw
std::recursive_mutex &lock_of_handle(int gpu_index) noexcept { return g_device_lock.slot[gpu_index < 0 ? 0 : gpu_index]; }
// rdr_set_stream: the stream the calling thread's launches are ordered on (null = the null stream)
thread_local void *g_user_stream = nullptr;

// ---- the protocol of every entry point that can fail, in two pieces ----
// guarded(error, body): the last error is cleared, `body` runs, and what it throws becomes rdr_last_error() and `error`.
template <class R, class Body> R guarded(R error, Body body) {
    g_last_error.clear();
    try {
        return body();
    } catch (const std::exception &e) {
        g_last_error = e.what() ? e.what() : "unknown error";
        return error;
    }
}
template <class Body> int status(Body body) { return guarded(1, [&] { body(); return 0; }); }      // the common case: 0, or 1
// OnDevice: while it lives, the calling thread holds the lock of the place it is made from, has that device selected and orders
// its launches on the caller's stream.  The places: a Scene's device; a gpu_index (an argument's, a description's, a topology's),
// where a negative one means host memory, which the product refuses -- with select_device's "no CPU fallback" text, or, when
// `host_is_for_harness` names the caller, with the text below; the calling thread's current device (the rdr_debug_* hooks:
// checked, not changed).  Entry points that are host arithmetic only -- the scratch-size queries, the two trace-plan hooks,
// rdr_compute_num_channels -- make none: they touch no device, no pool and no cache, so there is nothing to serialise.
struct OnDevice {
    std::lock_guard<std::recursive_mutex> lock;
    OnDevice(int use_gpu, int gpu_index, const char *host_is_for_harness = nullptr) : lock(device_lock(gpu_index)) {
#if !defined(RDR_HOSTSIM)
        if (!use_gpu && host_is_for_harness)
            throw std::runtime_error(std::string(host_is_for_harness) + ": host memory (negative gpu_index) is for the CPU harness only");
#endif
        exec::select_device(use_gpu, gpu_index);
        exec::ctx().stream = (hipStream_t)g_user_stream;
    }
    explicit OnDevice(int gpu_index, const char *host_is_for_harness = nullptr) : OnDevice(gpu_index >= 0, gpu_index, host_is_for_harness) {}
    explicit OnDevice(const rdr::Scene &s) : OnDevice(1, s.gpu_index) {}
};
const rdr::Scene &scene_of(const rdr_scene *scene, const char *who) {
    if (!scene) throw std::runtime_error(std::string(who) + ": a scene is required");
    return *reinterpret_cast<const rdr::Scene *>(scene);
}
const rdr::vnrm::Topology &topology_of(const rdr_mesh_topology *topology, const char *who) {
    if (!topology) throw std::runtime_error(std::string(who) + ": a topology is required");
    return *reinterpret_cast<const rdr::vnrm::Topology *>(topology);
}
size_t floats(int64_t n) { return n > 0 ? (size_t)n : 0; }
constexpr int kDebugMaxItems = 1 << 24;        // what the rdr_debug_* hooks accept
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
    return guarded((rdr_scene *)nullptr, [&] {
        OnDevice on(use_gpu, gpu_index);
        return reinterpret_cast<rdr_scene *>(rdr::create_scene(camera, shapes, num_shapes, materials, num_materials,
                                                               area_lights, num_area_lights, envmap, use_gpu, gpu_index,
                                                               use_primary_edge_sampling, use_secondary_edge_sampling));
    });
}

void rdr_scene_destroy(rdr_scene *scene) {
    if (!scene) return;
    rdr::Scene *s = reinterpret_cast<rdr::Scene *>(scene);
    // under the device's lock like every other call that touches its pool / caches (the destructor returns buffers and may join
    // the Scene's edge build)
    std::lock_guard<std::recursive_mutex> lk(lock_of_handle(s->gpu_index));
    delete s;
}

int rdr_scene_max_generic_texture_dimension(const rdr_scene *scene) {
    return scene ? reinterpret_cast<const rdr::Scene *>(scene)->max_generic_texture_dimension : 0;
}

int rdr_render(const rdr_scene *scene, const rdr_render_options *options, float *rendered_image,
               const float *d_rendered_image, const rdr_dscene_desc *d_scene, float *screen_gradient_image,
               float *debug_image) {
    return status([&] {
        if (!scene || !options) throw std::runtime_error("rdr_render: scene and options are required");
        const rdr::Scene &s = *reinterpret_cast<const rdr::Scene *>(scene);
        OnDevice on(s);
        rdr::render(s, *options, rendered_image, d_rendered_image, d_scene, screen_gradient_image, debug_image);
    });
}

int rdr_deferred_shade(const rdr_deferred_desc *desc, const float *g_buffer, const float *light_params, float *image) {
    return status([&] {
        if (!desc) throw std::runtime_error("rdr_deferred_shade: a description is required");
        OnDevice on(desc->gpu_index);
        rdr::dfr::shade(*desc, g_buffer, light_params, image);
    });
}

int rdr_deferred_shade_backward(const rdr_deferred_desc *desc, const float *g_buffer, const float *light_params,
                                const float *d_image, float *d_g_buffer, float *d_light_params) {
    return status([&] {
        if (!desc) throw std::runtime_error("rdr_deferred_shade_backward: a description is required");
        OnDevice on(desc->gpu_index);
        rdr::dfr::shade_backward(*desc, g_buffer, light_params, d_image, d_g_buffer, d_light_params);
    });
}

int rdr_deferred_specular(const rdr_deferred_desc *desc, const float *g_buffer, const float *material, const float *eye,
                          const float *light_params, float *image) {
    return status([&] {
        if (!desc) throw std::runtime_error("rdr_deferred_specular: a description is required");
        OnDevice on(desc->gpu_index);
        rdr::dfs::specular(*desc, g_buffer, material, eye, light_params, image);
    });
}

int rdr_deferred_specular_backward(const rdr_deferred_desc *desc, const float *g_buffer, const float *material, const float *eye,
                                   const float *light_params, const float *d_image, float *d_g_buffer, float *d_material,
                                   float *d_eye, float *d_light_params) {
    return status([&] {
        if (!desc) throw std::runtime_error("rdr_deferred_specular_backward: a description is required");
        OnDevice on(desc->gpu_index);
        rdr::dfs::specular_backward(*desc, g_buffer, material, eye, light_params, d_image, d_g_buffer, d_material, d_eye,
                                    d_light_params);
    });
}

int rdr_deferred_quad(const rdr_deferred_desc *desc, const float *g_buffer, const float *quads, float *image) {
    return status([&] {
        if (!desc) throw std::runtime_error("rdr_deferred_quad: a description is required");
        OnDevice on(desc->gpu_index);
        rdr::dfq::quad(*desc, g_buffer, quads, image);
    });
}

int rdr_deferred_quad_backward(const rdr_deferred_desc *desc, const float *g_buffer, const float *quads, const float *d_image,
                               float *d_g_buffer, float *d_quads) {
    return status([&] {
        if (!desc) throw std::runtime_error("rdr_deferred_quad_backward: a description is required");
        OnDevice on(desc->gpu_index);
        rdr::dfq::quad_backward(*desc, g_buffer, quads, d_image, d_g_buffer, d_quads);
    });
}

int rdr_deferred_quad_shadowed(const rdr_deferred_desc *desc, const float *g_buffer, const float *quads, int shadow_rays,
                               float *factors, float *image) {
    return status([&] {
        if (!desc) throw std::runtime_error("rdr_deferred_quad_shadowed: a description is required");
        OnDevice on(desc->gpu_index);
        rdr::dfq::quad_shadowed(*desc, g_buffer, quads, shadow_rays, factors, image);
    });
}

int rdr_deferred_quad_shadowed_backward(const rdr_deferred_desc *desc, const float *g_buffer, const float *quads,
                                        const float *factors, const float *d_image, float *d_g_buffer, float *d_quads) {
    return status([&] {
        if (!desc) throw std::runtime_error("rdr_deferred_quad_shadowed_backward: a description is required");
        OnDevice on(desc->gpu_index);
        rdr::dfq::quad_shadowed_backward(*desc, g_buffer, quads, factors, d_image, d_g_buffer, d_quads);
    });
}

int rdr_mip_num_levels(int height, int width) { return height > 0 && width > 0 ? rdr::mip::num_levels(height, width) : 0; }

int64_t rdr_mip_backward_scratch(int height, int width, int channels) {
    return guarded((int64_t)-1, [&] {
        return (int64_t)rdr::mip::scratch_floats(rdr::mip::make_shape(height, width, channels, rdr_mip_num_levels(height, width),
                                                                      "rdr_mip_backward_scratch"));
    });
}

int rdr_mip_tiled_stages(int height, int width, int channels) {
    return guarded(-1, [&] {
        return rdr::mip::tiled_stages(rdr::mip::make_shape(height, width, channels, rdr_mip_num_levels(height, width),
                                                           "rdr_mip_tiled_stages"));
    });
}

// (the product library reads and writes device memory only; host pointers are for the CPU debugging harness)
int rdr_mip_pyramid(int height, int width, int channels, int num_levels, float *const *levels, int gpu_index) {
    return status([&] {
        OnDevice on(gpu_index, "rdr_mip_pyramid");
        rdr::mip::pyramid(height, width, channels, num_levels, levels);
    });
}

int rdr_mip_pyramid_backward(int height, int width, int channels, int num_levels, const float *const *d_levels, float *d_texels,
                             float *scratch, int64_t scratch_floats, int gpu_index) {
    return status([&] {
        OnDevice on(gpu_index, "rdr_mip_pyramid_backward");
        rdr::mip::pyramid_backward(height, width, channels, num_levels, d_levels, d_texels, scratch, floats(scratch_floats));
    });
}

// ---- SH reconstruction and the sampling tables of an environment map (csrc/sh_envmap.h) ----
int64_t rdr_sh_backward_scratch(int height, int width, int channels, int num_coeffs) {
    return guarded((int64_t)-1, [&] {
        return (int64_t)rdr::shenv::scratch_floats(rdr::shenv::make_plan(height, width, channels, num_coeffs, "rdr_sh_backward_scratch"));
    });
}

int rdr_sh_reconstruct(const float *coeffs, int channels, int num_coeffs, int height, int width, float *image, uint8_t *clamp,
                       int gpu_index) {
    return status([&] {
        OnDevice on(gpu_index, "rdr_sh_reconstruct");
        rdr::shenv::reconstruct(height, width, channels, num_coeffs, coeffs, image, clamp);
    });
}

int rdr_sh_reconstruct_backward(const uint8_t *clamp, const float *d_image, int channels, int num_coeffs, int height, int width,
                                float *d_coeffs, float *scratch, int64_t scratch_floats, int gpu_index) {
    return status([&] {
        OnDevice on(gpu_index, "rdr_sh_reconstruct_backward");
        rdr::shenv::reconstruct_backward(height, width, channels, num_coeffs, clamp, d_image, d_coeffs, scratch, floats(scratch_floats));
    });
}

int rdr_envmap_tables(const float *texels, const float *y_weight, int height, int width, float *sample_cdf_ys, float *sample_cdf_xs,
                      float *total, int gpu_index) {
    return status([&] {
        OnDevice on(gpu_index, "rdr_envmap_tables");
        rdr::shenv::tables(height, width, texels, y_weight, sample_cdf_ys, sample_cdf_xs, total);
    });
}

// ---- the Gaussian pyramid loss (csrc/pyramid_loss.h, include/redner_amd_image.h) ----
int rdr_pyramid_loss_scratch(int batch, int height, int width, int channels, int num_levels, int64_t *forward_floats,
                             int64_t *backward_floats) {
    return status([&] {
        const rdr::pyl::Plan p = rdr::pyl::make_plan(batch, height, width, channels, num_levels, nullptr, 0.f, "rdr_pyramid_loss_scratch");
        if (forward_floats) *forward_floats = (int64_t)rdr::pyl::forward_floats(p);
        if (backward_floats) *backward_floats = (int64_t)rdr::pyl::backward_floats(p);
    });
}

int rdr_pyramid_loss_plan(int batch, int height, int width, int channels, int num_levels, int *tiled_levels, int *small_floats) {
    return status([&] {
        const rdr::pyl::Plan p = rdr::pyl::make_plan(batch, height, width, channels, num_levels, nullptr, 0.f, "rdr_pyramid_loss_plan");
        if (tiled_levels) *tiled_levels = p.tiled;
        if (small_floats) *small_floats = rdr::pyl::kSmall;
    });
}

int rdr_pyramid_loss(const float *image, const float *target, int batch, int height, int width, int channels, int num_levels,
                     const float *weights, float clamp, float *loss, double *terms, float *scratch, int64_t scratch_floats,
                     int gpu_index) {
    return status([&] {
        OnDevice on(gpu_index, "rdr_pyramid_loss");
        const rdr::pyl::Plan p = rdr::pyl::make_plan(batch, height, width, channels, num_levels, weights, clamp, "rdr_pyramid_loss");
        rdr::pyl::forward(p, image, target, loss, terms, scratch, floats(scratch_floats));
    });
}

int rdr_pyramid_loss_backward(const float *image, const float *target, int batch, int height, int width, int channels,
                              int num_levels, const float *weights, float clamp, const float *saved, int64_t saved_floats,
                              const float *upstream, float *d_image, float *d_target, float *scratch, int64_t scratch_floats,
                              int gpu_index) {
    return status([&] {
        OnDevice on(gpu_index, "rdr_pyramid_loss_backward");
        const rdr::pyl::Plan p = rdr::pyl::make_plan(batch, height, width, channels, num_levels, weights, clamp, "rdr_pyramid_loss_backward");
        rdr::pyl::backward(p, image, target, saved, floats(saved_floats), upstream, d_image, d_target, scratch, floats(scratch_floats));
    });
}

// ---- the rigid pose (csrc/pose.h, include/redner_amd_pose.h) ----
int rdr_pose_scratch(int num_sets, const int *counts, int64_t *forward_floats, int64_t *backward_floats) {
    return status([&] {
        const rdr::pose::Table tb = rdr::pose::make_table(num_sets, counts, "rdr_pose_scratch");
        if (forward_floats) *forward_floats = (int64_t)rdr::pose::forward_floats(tb);
        if (backward_floats) *backward_floats = (int64_t)rdr::pose::backward_floats(tb);
    });
}

int rdr_pose_plan(int num_sets, const int *counts, int *chunk_vertices, int *max_workgroups, int *workgroups) {
    return status([&] {
        const rdr::pose::Table tb = rdr::pose::make_table(num_sets, counts, "rdr_pose_plan");
        if (chunk_vertices) *chunk_vertices = rdr::pose::kChunk;
        if (max_workgroups) *max_workgroups = rdr::pose::kMaxGroups;
        if (workgroups) *workgroups = tb.groups;
    });
}

int rdr_rotate_matrix(const float *angles, float *matrix, int gpu_index) {
    return status([&] {
        OnDevice on(gpu_index, "rdr_rotate_matrix");
        rdr::pose::rotate_matrix(angles, matrix);
    });
}

int rdr_rotate_matrix_backward(const float *angles, const float *d_matrix, float *d_angles, int gpu_index) {
    return status([&] {
        OnDevice on(gpu_index, "rdr_rotate_matrix_backward");
        rdr::pose::rotate_matrix_backward(angles, d_matrix, d_angles);
    });
}

int rdr_pose_vertices(int num_sets, const float *const *vertices, const int *counts, const float *angles, const float *translation,
                      const float *center, float *const *out, float *saved, float *scratch, int64_t scratch_floats, int gpu_index) {
    return status([&] {
        OnDevice on(gpu_index, "rdr_pose_vertices");
        const rdr::pose::Table tb = rdr::pose::make_table(num_sets, counts, "rdr_pose_vertices");
        rdr::pose::forward(tb, vertices, angles, translation, center, out, saved, scratch, floats(scratch_floats));
    });
}

int rdr_pose_vertices_backward(int num_sets, const float *const *vertices, const int *counts, const float *angles, const float *saved,
                               int own_center, const float *const *d_out, float *const *d_vertices, float *d_angles,
                               float *d_translation, float *d_center, float *scratch, int64_t scratch_floats, int gpu_index) {
    return status([&] {
        OnDevice on(gpu_index, "rdr_pose_vertices_backward");
        const rdr::pose::Table tb = rdr::pose::make_table(num_sets, counts, "rdr_pose_vertices_backward");
        rdr::pose::backward(tb, vertices, angles, saved, own_center != 0, d_out, d_vertices, d_angles, d_translation, d_center, scratch,
                            floats(scratch_floats));
    });
}

// ---- vertex normals (csrc/vertex_normal.h) ----
rdr_mesh_topology *rdr_mesh_topology_create(const int *indices, int num_triangles, int num_vertices, int use_gpu, int gpu_index) {
    return guarded((rdr_mesh_topology *)nullptr, [&] {
        const int place = use_gpu ? (gpu_index < 0 ? 0 : gpu_index) : -1;
        OnDevice on(place, "rdr_mesh_topology_create");
        return reinterpret_cast<rdr_mesh_topology *>(rdr::vnrm::create_topology(indices, num_triangles, num_vertices, place));
    });
}

void rdr_mesh_topology_destroy(rdr_mesh_topology *topology) {
    if (!topology) return;
    rdr::vnrm::Topology *t = reinterpret_cast<rdr::vnrm::Topology *>(topology);
    std::lock_guard<std::recursive_mutex> lk(lock_of_handle(t->gpu_index));
    // best effort, not the guard: the plan is deleted also when its device cannot be selected any more, and there is nobody to
    // report that to
    try { exec::select_device(t->gpu_index >= 0, t->gpu_index); } catch (const std::exception &) {}
    delete t;
}

int rdr_mesh_topology_read(const rdr_mesh_topology *topology, int *offsets, int *corners) {
    return status([&] {
        const rdr::vnrm::Topology &t = topology_of(topology, "rdr_mesh_topology_read");
        OnDevice on(t.gpu_index, "rdr_mesh_topology_read");
        rdr::vnrm::read_topology(t, offsets, corners);
    });
}

int rdr_vertex_normal_scratch(const rdr_mesh_topology *topology, int scheme, int64_t *forward_floats, int64_t *backward_floats,
                              int64_t *saved_floats) {
    return status([&] {
        const rdr::vnrm::Topology &t = topology_of(topology, "rdr_vertex_normal_scratch");
        const bool cot = rdr::vnrm::cotangent(scheme, "rdr_vertex_normal_scratch");
        if (forward_floats) *forward_floats = (int64_t)rdr::vnrm::forward_scratch_floats(t, cot);
        if (backward_floats) *backward_floats = (int64_t)rdr::vnrm::backward_scratch_floats(t, cot);
        if (saved_floats) *saved_floats = (int64_t)rdr::vnrm::saved_floats(t, cot);
    });
}

int rdr_vertex_normal(const rdr_mesh_topology *topology, int scheme, const float *vertices, float *normals, float *saved,
                      float *scratch, int64_t scratch_floats) {
    return status([&] {
        const rdr::vnrm::Topology &t = topology_of(topology, "rdr_vertex_normal");
        OnDevice on(t.gpu_index, "rdr_vertex_normal");
        rdr::vnrm::forward(t, scheme, vertices, normals, saved, scratch, floats(scratch_floats));
    });
}

int rdr_vertex_normal_backward(const rdr_mesh_topology *topology, int scheme, const float *vertices, const float *saved,
                               const float *d_normals, float *d_vertices, float *scratch, int64_t scratch_floats) {
    return status([&] {
        const rdr::vnrm::Topology &t = topology_of(topology, "rdr_vertex_normal_backward");
        OnDevice on(t.gpu_index, "rdr_vertex_normal_backward");
        rdr::vnrm::backward(t, scheme, vertices, saved, d_normals, d_vertices, scratch, floats(scratch_floats));
    });
}

// ---- Laplacian smoothing (csrc/mesh_smooth.h) ----
int rdr_mesh_boundary(const rdr_mesh_topology *topology, float *bound) {
    return status([&] {
        const rdr::vnrm::Topology &t = topology_of(topology, "rdr_mesh_boundary");
        OnDevice on(t.gpu_index, "rdr_mesh_boundary");
        rdr::msm::boundary(t, bound);
    });
}

int rdr_mesh_smooth_scratch(const rdr_mesh_topology *topology, int scheme, int64_t *forward_floats, int64_t *backward_floats,
                            int64_t *saved_floats) {
    return status([&] {
        const rdr::vnrm::Topology &t = topology_of(topology, "rdr_mesh_smooth_scratch");
        rdr::msm::scheme_of(scheme, "rdr_mesh_smooth_scratch");
        if (forward_floats) *forward_floats = (int64_t)rdr::msm::forward_scratch_floats(t);
        if (backward_floats) *backward_floats = (int64_t)rdr::msm::backward_scratch_floats(t);
        if (saved_floats) *saved_floats = (int64_t)rdr::msm::saved_floats(t);
    });
}

int rdr_mesh_laplacian(const rdr_mesh_topology *topology, int scheme, const float *vertices, const float *control, float *shift,
                       float *saved, float *scratch, int64_t scratch_floats) {
    return status([&] {
        const rdr::vnrm::Topology &t = topology_of(topology, "rdr_mesh_laplacian");
        OnDevice on(t.gpu_index, "rdr_mesh_laplacian");
        rdr::msm::laplacian(t, scheme, vertices, control, shift, saved, scratch, floats(scratch_floats));
    });
}

int rdr_mesh_laplacian_backward(const rdr_mesh_topology *topology, int scheme, const float *vertices, const float *control,
                                const float *saved, const float *d_shift, float *d_vertices, float *scratch, int64_t scratch_floats) {
    return status([&] {
        const rdr::vnrm::Topology &t = topology_of(topology, "rdr_mesh_laplacian_backward");
        OnDevice on(t.gpu_index, "rdr_mesh_laplacian_backward");
        rdr::msm::laplacian_backward(t, scheme, vertices, control, saved, d_shift, d_vertices, scratch, floats(scratch_floats));
    });
}

int rdr_mesh_smooth(const rdr_mesh_topology *topology, int scheme, const float *vertices_in, const float *control, float lmd,
                    int iterations, float *vertices_out, float *scratch, int64_t scratch_floats) {
    return status([&] {
        const rdr::vnrm::Topology &t = topology_of(topology, "rdr_mesh_smooth");
        OnDevice on(t.gpu_index, "rdr_mesh_smooth");
        rdr::msm::smooth(t, scheme, vertices_in, control, lmd, iterations, vertices_out, scratch, floats(scratch_floats));
    });
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
    std::vector<std::unique_lock<std::recursive_mutex>> all;        // every device, in index order (a call holds one lock only)
    for (std::recursive_mutex &m : g_device_lock) all.emplace_back(m);
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
    return status([&] {
        const rdr::Scene &s = scene_of(scene, "rdr_debug_dump_edges");
        const std::unique_ptr<FILE, int (*)(FILE *)> file(path ? fopen(path, "w") : nullptr, fclose);      // closed on every way out
        if (!file) throw std::runtime_error("rdr_debug_dump_edges: the file cannot be written");
        {
            OnDevice on(s);
            s.edge_data();
            if (s.edges && s.edges->device_trees) rdr::download_edge_trees(*s.edges);
        }
        rdr::write_edge_dump(file.get(), s.edges);
    });
}

/* Test hook: the hierarchy this Scene's kernels built against the host builder's (bvh.cpp) on the same mesh arrays -- node
 * records, leaf order, triangle records, 4-wide records.  Returns the number of records that differ (0: identical), -1
 * when the Scene's hierarchy is a refit of an earlier build / was not built by kernels, or -2 with rdr_last_error() set. */
int rdr_debug_bvh_check(const rdr_scene *scene) {
    return guarded(-2, [&] {
        const rdr::Scene &s = scene_of(scene, "rdr_debug_bvh_check");
        if (!s.bvh_dev || s.bvh_dev->parent) return -1;
        OnDevice on(s);
        return rdr::compare_bvh_with_host_build(s);
    });
}

int rdr_scene_trace(const rdr_scene *scene, const float *rays, int32_t *hits, int num_rays, int any_hit) {
    return status([&] {
        const rdr::Scene &s = scene_of(scene, "rdr_scene_trace");
        OnDevice on(s);
        exec::trace(s.bvh, reinterpret_cast<const rt::RayRec *>(rays), reinterpret_cast<rt::HitRec *>(hits), num_rays, any_hit != 0);
        exec::sync();
    });
}

/* Test hooks: the launch exec::trace() would make (trace_plan.h) -- for stated sizes of a hierarchy, and for a Scene's own.
 * Host arithmetic only: no device is selected or touched. */
static void write_trace_plan(const exec::TraceFacts &facts, int num_rays, int any_hit, int coherent, int counting,
                             const rdr_tuning *tuning, int32_t *out) {
    if (num_rays <= 0 || !out || facts.num_nodes < 0 || facts.stack_need < 0 || facts.wide_stack_need < 0)
        throw std::runtime_error("rdr_debug_trace_plan: bad arguments");
    const exec::TracePlan p = exec::plan_trace(facts, num_rays, any_hit != 0, coherent != 0, counting != 0, rdr::resolve_tuning(tuning));
    const int32_t v[10] = {(int32_t)p.form, p.stack, p.short_index, p.stage_top, p.sorted, p.counting, p.blocks, p.rays_per_lane, p.idle_min, p.steps};
    std::memcpy(out, v, sizeof(v));
}
int rdr_debug_trace_plan(int num_nodes, int stack_need, int has_wide, int wide_stack_need, int num_rays, int any_hit, int coherent,
                         int counting, const rdr_tuning *tuning, int32_t *out) {
    return status([&] {
        write_trace_plan(exec::TraceFacts{num_nodes, stack_need, wide_stack_need, has_wide != 0}, num_rays, any_hit, coherent, counting, tuning, out);
    });
}
int rdr_debug_scene_trace_plan(const rdr_scene *scene, int num_rays, int any_hit, int coherent, int counting, const rdr_tuning *tuning,
                               int32_t *out) {
    return status([&] {
        if (!scene) throw std::runtime_error("rdr_debug_scene_trace_plan: bad arguments");
        write_trace_plan(exec::trace_facts(reinterpret_cast<const rdr::Scene *>(scene)->bvh), num_rays, any_hit, coherent, counting, tuning, out);
    });
}

/* Test hook: exec::trace() with every plan input chosen by the caller (include/redner_amd_debug.h). */
int rdr_debug_scene_trace(const rdr_scene *scene, const float *rays, int32_t *hits, int num_rays, int any_hit, int coherent,
                          const rdr_tuning *tuning, int trace_hybrid, const int32_t *device_count) {
    return status([&] {
        const rdr::Scene &s = scene_of(scene, "rdr_debug_scene_trace");
        if (num_rays < 0 || num_rays > kDebugMaxItems) throw std::runtime_error("rdr_debug_scene_trace: num_rays outside [0, 2^24]");
        if (num_rays > 0 && (!rays || !hits)) throw std::runtime_error("rdr_debug_scene_trace: an array is missing");
        if (trace_hybrid < -1 || trace_hybrid > 1) throw std::runtime_error("rdr_debug_scene_trace: trace_hybrid is -1, 0 or 1");
        OnDevice on(s);
        rdr::Tuning t = rdr::resolve_tuning(tuning);
        if (trace_hybrid >= 0) t.trace_hybrid = trace_hybrid != 0;
        const rdr::TuningScope scope(t);
        exec::trace(s.bvh, reinterpret_cast<const rt::RayRec *>(rays), reinterpret_cast<rt::HitRec *>(hits),
                    device_count ? exec::Count(device_count, num_rays) : exec::Count(num_rays), any_hit != 0, coherent != 0);
        exec::sync();
    });
}

/* Test hook: stack entries per ray on the host builder's hierarchy of the Scene's meshes (include/redner_amd_debug.h). */
int rdr_debug_trace_occupancy(const rdr_scene *scene, const float *host_rays, int num_rays, int any_hit, int wide, int32_t *max_entries) {
    return status([&] {
        const rdr::Scene &s = scene_of(scene, "rdr_debug_trace_occupancy");
        if (num_rays < 0 || num_rays > kDebugMaxItems) throw std::runtime_error("rdr_debug_trace_occupancy: num_rays outside [0, 2^24]");
        if (!max_entries || (num_rays > 0 && !host_rays)) throw std::runtime_error("rdr_debug_trace_occupancy: an array is missing");
        std::vector<rt::MeshView> meshes(s.shapes.size());
        for (size_t i = 0; i < s.shapes.size(); ++i) meshes[i] = rt::MeshView{s.h_vertices[i].data(), s.h_indices[i].data(), s.shapes[i].num_triangles};
        const rt::BvhHost h = rt::build_bvh(meshes);
        rt::BvhD view{};
        view.nodes = h.nodes.data(); view.tris = h.tris.data(); view.ids = h.ids.data();
        view.num_nodes = (int)h.nodes.size(); view.num_tris = (int)h.ids.size() / 2; view.stack_need = h.depth + 2;
        view.wide = h.wide.empty() ? nullptr : h.wide.data(); view.num_wide = (int)h.wide.size(); view.wide_stack_need = h.wide_stack_need;
        // No walk pushes this value: binary entries are node indices, wide entries links of children that were hit (bvh.h).  A binary
        // walk pushes at most once per level and a wide one at most three times, so the columns below cannot be overrun.
        constexpr int kNeverPushed = rt::kEmptyLink;
        std::vector<int> stack((size_t)4 * (wide ? view.wide_stack_need : view.stack_need) + 64);
        const rt::RayRec *rays = reinterpret_cast<const rt::RayRec *>(host_rays);
        for (int i = 0; i < num_rays; ++i) {
            const rt::RayRec &r = rays[i];
            max_entries[i] = 0;
            if (r.tmax < 0.f) continue;
            std::fill(stack.begin(), stack.end(), kNeverPushed);
            const float o[3] = {r.ox, r.oy, r.oz}, d[3] = {r.dx, r.dy, r.dz};
            if (wide) {
                if (any_hit) rt::traverse_wide<true>(view, o, d, r.tmin, r.tmax, stack.data(), 1, nullptr);
                else rt::traverse_wide<false>(view, o, d, r.tmin, r.tmax, stack.data(), 1, nullptr);
            } else {
                if (any_hit) rt::traverse<true>(view, o, d, r.tmin, r.tmax, stack.data(), 1);
                else rt::traverse<false>(view, o, d, r.tmin, r.tmax, stack.data(), 1);
            }
            int top = (int)stack.size();
            while (top > 0 && stack[top - 1] == kNeverPushed) --top;
            max_entries[i] = top;
        }
        const int32_t facts[4] = {view.num_nodes, view.stack_need, view.num_wide, view.wide_stack_need};
        std::memcpy(max_entries + num_rays, facts, sizeof(facts));
    });
}

/* Test hook: the library's transcendental routines (libm_exact.h) evaluated by a kernel on `n` arguments (HOST pointers;
 * `y` only for the two-argument functions).  fn: 0 sin, 1 cos, 2 atan2(x, y), 3 atan, 4 acos, 5 log, 6 pow(x, y). */
int rdr_debug_libm(int fn, const double *x, const double *y, double *out, int n) {
    return status([&] {
        if (fn < 0 || fn > 6 || n < 0) throw std::runtime_error("rdr_debug_libm: bad arguments");
        OnDevice on(exec::current_device());
        const size_t count = (size_t)n, bytes = sizeof(double) * count;
        rdr::Arena held;
        const double *dx = held.put(x, count);
        double *dy = held.get<double>(count), *dout = held.get<double>(count);
        if (y) exec::upload_async(dy, y, bytes); else exec::zero(dy, bytes);
        exec::upload_flush();
        exec::launch(exec::Count(n), LibmProbe{fn, dx, dy, dout});
        exec::download(out, dout, bytes);
        exec::sync();                  // the probe has finished: `held` may go back to the pool
    });
}

/* Test hook: the gradient store of a render, one stage that calls the scatter functions, the fold (render.cpp: debug_grad_scatter). */
int rdr_debug_grad_scatter(const rdr_scene *scene, const rdr_dscene_desc *d_scene, uint64_t job_samples, int op, int plain,
                           int num_lanes, const uint8_t *active, const int32_t *target, const int32_t *index,
                           const double *values) {
    return status([&] {
        if (!scene || !d_scene) throw std::runtime_error("rdr_debug_grad_scatter: scene and d_scene are required");
        const rdr::Scene &s = *reinterpret_cast<const rdr::Scene *>(scene);
        OnDevice on(s);
        rdr::debug_grad_scatter(s, *d_scene, (size_t)job_samples, op, plain != 0, num_lanes, active, target, index, values);
    });
}

/* Test hook: the lane park of the stage bodies alone (render.cpp: debug_lane_park). */
int rdr_debug_lane_park(int num_lanes, const uint8_t *active, const double *in, double *out, int32_t *columns) {
    return status([&] {
        if (num_lanes < 0 || num_lanes > kDebugMaxItems) throw std::runtime_error("rdr_debug_lane_park: num_lanes out of range");
        if (!columns || (num_lanes > 0 && (!active || !in || !out))) throw std::runtime_error("rdr_debug_lane_park: an array is missing");
        OnDevice on(exec::current_device());
        *columns = rdr::debug_lane_park(num_lanes, active, in, out);
    });
}

/* Test hook: one stream compaction as render.cpp calls it (count on the host or on the device, appended, with positions, with the
 * edge sampler's counter, on the second scratch) or the host-visible form. */
int rdr_debug_compact(int upper, int count, const int32_t *in, const uint8_t *keep, int keep_len, int append_upper, int append_count,
                      int dyn_inc, int scratch, int host_form, int32_t *out, int32_t *pos_out, int32_t *result) {
    return status([&] {
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
        OnDevice on(exec::current_device());
        rdr::Arena held;
        const size_t out_len = (size_t)(append ? append_upper : 0) + (size_t)upper;
        const int *d_in = in ? held.put(in, (size_t)upper) : nullptr;
        const uint8_t *d_keep = held.put(keep, (size_t)keep_len);
        int *d_out = held.put(out, out_len);
        int *d_pos = pos_out ? held.put(pos_out, out_len) : nullptr;
        const int *d_count = count >= 0 ? held.put(&count, 1) : nullptr;
        const int *d_append = append ? held.put(&append_count, 1) : nullptr;
        int *d_dyn = dyn_inc != 0 ? held.put(&result[2], 1) : nullptr;
        exec::upload_flush();
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
        exec::sync();                  // the compaction has finished: `held` may go back to the pool
        std::memcpy(result, r, sizeof(r));
    });
}

/* Test hook: the walk kernels with lane refill (and the plain launch) over a walker whose every begin, step and finish is counted. */
int rdr_debug_walk(int kind, int upper, int count, const int32_t *len, int items_per_lane, int idle_min, int steps, int gate_closed,
                   int repeat, int32_t *begun, int32_t *finished, int32_t *steps_taken, uint32_t *acc) {
    return status([&] {
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
        OnDevice on(exec::current_device());
        rdr::Arena held;
        const size_t n = (size_t)upper;
        WalkProbe w;
        w.len = held.put(len, n);
        w.gate = held.put(&gate_closed, 1);
        w.begun = held.put(begun, n); w.finished = held.put(finished, n); w.steps_taken = held.put(steps_taken, n);
        w.acc = held.put(acc, n);
        const int *d_count = count >= 0 ? held.put(&count, 1) : nullptr;
        exec::upload_flush();
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
        exec::sync();                  // the walks have finished: `held` may go back to the pool
    });
}

/* Test hook: the stable radix sort of (64-bit code, edge id) pairs (edges_gpu.cpp: debug_sort_pairs). */
int rdr_debug_sort_pairs(const uint64_t *keys, const int32_t *vals, int n, uint64_t *keys_out, int32_t *vals_out) {
    return status([&] {
        if (n < 1 || n > kDebugMaxItems) throw std::runtime_error("rdr_debug_sort_pairs: n outside [1, 2^24]");
        if (!keys || !vals || !keys_out || !vals_out) throw std::runtime_error("rdr_debug_sort_pairs: an array is missing");
        OnDevice on(exec::current_device());
        rdr::debug_sort_pairs(keys, vals, n, keys_out, vals_out);
    });
}

} // extern "C"
