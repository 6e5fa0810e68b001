/* redner_amd.h -- C ABI of the MI355X-native differentiable path tracer.
 *
 * This is the drop-in boundary for the one hot path of BachiLi/redner: everything the reference's
 * pybind11 module `redner` (src/redner.cpp:20-272) exposes for rendering, expressed as plain C
 * structs, raw pointers and sizes -- no torch / pybind types.  The Python module
 * redner_amd/redner.py re-creates the reference's class surface (redner.Camera, redner.Shape,
 * redner.Scene, redner.render, ...) on top of these entry points via ctypes, so the unmodified
 * pyredner/render_pytorch.py runs against it.
 *
 * Pointer conventions are the reference's own (src/ptr.h:10-24: raw addresses, no ownership, no
 * size, 0 = absent): `dev` pointers address GPU memory of device `gpu_index` (torch CUDA/HIP
 * tensors' data_ptr()), `host` pointers address CPU memory and are read during the call that
 * receives them.  All outputs are caller-owned and ACCUMULATED into (+=), never overwritten
 * (src/primary_contribution.cpp:39-43, src/atomic.h:43-141).
 *
 * Error handling: the reference aborts (assert/exit(1), src/cuda_utils.h:12-16).  Here every
 * entry point that can fail returns NULL / non-zero and writes a message retrievable with
 * rdr_last_error(); the Python layer raises RuntimeError.  There is NO CPU fallback: creating a
 * scene with use_gpu == 0, or without a usable gfx950 device, is an error.
 */
#ifndef REDNER_AMD_H
#define REDNER_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RDR_MAX_MIP_LEVELS 8 /* src/texture.h:11 max_num_texels */

/* enum values follow the declaration order of the reference's enums */
enum rdr_camera_type { RDR_CAMERA_PERSPECTIVE = 0, RDR_CAMERA_ORTHOGRAPHIC = 1, RDR_CAMERA_FISHEYE = 2,
                       RDR_CAMERA_PANORAMA = 3 };                 /* src/camera.h:12-17   */
enum rdr_sampler_type { RDR_SAMPLER_INDEPENDENT = 0, RDR_SAMPLER_SOBOL = 1 }; /* src/pathtracer.h:11-14 */
enum rdr_channel {                                                /* src/channels.h:6-23  */
    RDR_CH_RADIANCE = 0, RDR_CH_ALPHA, RDR_CH_DEPTH, RDR_CH_POSITION, RDR_CH_GEOMETRY_NORMAL,
    RDR_CH_SHADING_NORMAL, RDR_CH_UV, RDR_CH_BARYCENTRIC_COORDINATES, RDR_CH_DIFFUSE_REFLECTANCE,
    RDR_CH_SPECULAR_REFLECTANCE, RDR_CH_ROUGHNESS, RDR_CH_GENERIC_TEXTURE, RDR_CH_VERTEX_COLOR,
    RDR_CH_SHAPE_ID, RDR_CH_TRIANGLE_ID, RDR_CH_MATERIAL_ID
};

/* redner.Camera(...)  src/redner.cpp:34-50, src/camera.h:19-84.  All pointers HOST, read at
 * scene creation.  cam_to_world != NULL selects the matrix parameterisation (use_look_at = 0). */
typedef struct rdr_camera_desc {
    int width, height;
    const float *position, *look, *up;          /* 3 floats each, or NULL */
    const float *cam_to_world, *world_to_cam;   /* 16 floats row-major, or NULL */
    const float *intrinsic_mat_inv, *intrinsic_mat; /* 9 floats row-major */
    const float *distortion_params;             /* 8 floats or NULL */
    float clip_near;
    int camera_type;                            /* rdr_camera_type */
    int viewport_beg[2], viewport_end[2];       /* (x, y) */
} rdr_camera_desc;

/* redner.DCamera(...)  src/redner.cpp:52-60.  DEV pointers to fp32 gradient buffers (or NULL). */
typedef struct rdr_dcamera_desc {
    float *position, *look, *up, *cam_to_world, *world_to_cam, *intrinsic_mat_inv, *intrinsic_mat,
          *distortion_params;
} rdr_dcamera_desc;

/* redner.Shape(...)  src/redner.cpp:84-104, src/shape.h:9-61.  DEV pointers. */
typedef struct rdr_shape_desc {
    const float *vertices;      /* [num_vertices, 3] */
    const int32_t *indices;     /* [num_triangles, 3] */
    const float *uvs;           /* [num_uv_vertices, 2] or NULL */
    const float *normals;       /* [num_normal_vertices, 3] or NULL */
    const int32_t *uv_indices;  /* or NULL */
    const int32_t *normal_indices; /* or NULL */
    const float *colors;        /* [num_vertices, 3] or NULL */
    int num_vertices, num_uv_vertices, num_normal_vertices, num_triangles;
    int material_id, light_id;
} rdr_shape_desc;

/* redner.DShape(vertices, uvs, normals, colors)  src/redner.cpp:106-110.  DEV fp32. */
typedef struct rdr_dshape_desc { float *vertices, *uvs, *normals, *colors; } rdr_dshape_desc;

/* redner.Texture1/3/N(...)  src/redner.cpp:112-131, src/texture.h:14-47.  DEV pointers.
 * A constant texture has num_levels = 1 and width[0] = height[0] = 0. */
typedef struct rdr_texture_desc {
    const float *texels[RDR_MAX_MIP_LEVELS];
    int width[RDR_MAX_MIP_LEVELS], height[RDR_MAX_MIP_LEVELS];
    int channels;       /* 1, 3, or N for the generic texture */
    int num_levels;     /* 0 = texture absent */
    const float *uv_scale; /* 2 floats */
} rdr_texture_desc;

/* redner.Material(...)  src/redner.cpp:133-151 */
typedef struct rdr_material_desc {
    rdr_texture_desc diffuse_reflectance, specular_reflectance, roughness, generic_texture, normal_map;
    int compute_specular_lighting, two_sided, use_vertex_color;
} rdr_material_desc;

/* redner.DMaterial(...)  src/redner.cpp:153-158: same shape, texel pointers are fp32 gradients */
typedef struct rdr_dtexture_desc {
    float *texels[RDR_MAX_MIP_LEVELS];
    int num_levels;
    float *uv_scale;
} rdr_dtexture_desc;
typedef struct rdr_dmaterial_desc {
    rdr_dtexture_desc diffuse_reflectance, specular_reflectance, roughness, generic_texture, normal_map;
} rdr_dmaterial_desc;

/* redner.AreaLight(shape_id, intensity, two_sided, directly_visible)  src/redner.cpp:160-164.
 * intensity is copied (the reference reads its HOST pointer in the constructor). */
typedef struct rdr_area_light_desc {
    int shape_id;
    float intensity[3];
    int two_sided, directly_visible;
} rdr_area_light_desc;
/* redner.DAreaLight(intensity)  src/redner.cpp:166-167.  DEV fp32[3]. */
typedef struct rdr_darea_light_desc { float *intensity; } rdr_darea_light_desc;

/* redner.EnvironmentMap(...)  src/redner.cpp:169-177.  values/cdfs DEV, matrices HOST. */
typedef struct rdr_envmap_desc {
    rdr_texture_desc values;
    const float *env_to_world, *world_to_env;   /* 16 floats, HOST */
    const float *sample_cdf_ys, *sample_cdf_xs; /* DEV */
    float pdf_norm;
    int directly_visible;
} rdr_envmap_desc;
typedef struct rdr_denvmap_desc { rdr_dtexture_desc values; float *world_to_env; } rdr_denvmap_desc;

/* redner.RenderOptions(seed, num_samples, max_bounces, channels, sampler_type, sample_pixel_center)
 * src/redner.cpp:207-216, src/pathtracer.h:16-23.
 * Extension for multi-GPU sample sharding (no reference counterpart): this
 * call renders Sobol' samples [sample_offset, sample_offset + num_samples) of a total_samples-spp
 * estimate, i.e. with weight 1/total_samples.  total_samples == 0 means "num_samples". */
typedef struct rdr_tuning rdr_tuning;
typedef struct rdr_render_options {
    uint64_t seed;
    int num_samples, max_bounces;
    const int *channels; int num_channels;   /* rdr_channel values */
    int sampler_type;                        /* rdr_sampler_type */
    int sample_pixel_center;
    int sample_offset, total_samples;
    const rdr_tuning *tuning;                /* or NULL = every default (below) */
} rdr_render_options;

/* How a render() call is scheduled on the GPU -- which kernels, how many samples per launch, how many host threads.  No
 * reference counterpart (its RenderOptions stop at sample_pixel_center, src/pathtracer.h:16-23); results do not depend on any
 * of this beyond the order of floating-point atomics.  EVERY field: 0 = the library's default, so a zeroed struct (or a NULL
 * pointer) is the shipped configuration.  These fields replace the RDR_* environment switches of earlier rounds for
 * everything that selects a kernel or a schedule; a variable that is still set supplies the default of a field that is 0
 * (A/B scripts), the field wins. */
enum rdr_tune_flags {
    RDR_TUNE_NO_OVERLAP       = 1 << 0,   /* every stage on the calling stream (no side streams)              RDR_NO_OVERLAP */
    RDR_TUNE_FORCE_GENERAL    = 1 << 1,   /* no stage specialisation (lean / mid kernels)                     RDR_FORCE_GENERAL */
    RDR_TUNE_PICKN_WALK       = 1 << 2,   /* NEE-mode edge pick: reference-order walk for every slot          RDR_PICKN_WALK */
    RDR_TUNE_PICKH_FUSED      = 1 << 3,   /* hierarchical edge pick: the one-loop form                        RDR_PICKH_FUSED */
    RDR_TUNE_PICKH_LAZY       = 1 << 4,   /* ... per-field node loads                                         RDR_PICKH_LAZY */
    RDR_TUNE_NO_HOIST         = 1 << 5,   /* first-vertex edge picks inside the backward sweep                RDR_NO_HOIST */
    RDR_TUNE_REFILL_OFF       = 1 << 6,   /* never the refilling traversal kernel                             RDR_TRACE_REFILL=0 */
    RDR_TUNE_REFILL_ALL       = 1 << 7,   /* the refilling traversal kernel on every queue                    RDR_TRACE_REFILL_ALL */
    RDR_TUNE_TRACE_BINARY     = 1 << 8,   /* never the 4-wide node records                                    RDR_TRACE_BINARY */
    RDR_TUNE_TRACE_NO_LDS_TOP = 1 << 9,   /* hierarchy top not staged in LDS                                  RDR_TRACE_NO_LDS_TOP */
    RDR_TUNE_NO_FUSED_BOUNCE  = 1 << 10,  /* BounceContrib(d) and BounceSample(d+1) as two launches          RDR_NO_FUSED_BOUNCE */
    RDR_TUNE_PICKH_ONE_LAUNCH = 1 << 11,  /* hierarchical edge pick: one slot per lane, one launch (r1-r5)   RDR_PICKH_ONE_LAUNCH */
    RDR_TUNE_NO_NEE_COMPACT   = 1 << 12,  /* bounce adjoints without list compactions (next-event half over
                                           * the whole live-lane list, continuation half over the next
                                           * depth's list as it is)                                            RDR_NO_NEE_COMPACT */
    RDR_TUNE_LARGE_FORMS      = 1 << 13,  /* the stage forms of large frames (split pick, compacted adjoint
                                           * lists) at every size; default: from 2^19 lanes per launch set     RDR_LARGE_FRAME_FORMS */
    RDR_TUNE_TRACE_EVERY_CONTINUATION = 1 << 14   /* the last bounce's continuation rays are all traced (default in a
                                           * plain scene with <= 8 emitter triangles: those that meet no
                                           * emitter triangle are answered "no hit" untraced)                  RDR_TRACE_EVERY_CONTINUATION */
};
struct rdr_tuning {
    unsigned flags;                 /* rdr_tune_flags */
    int batch_samples;              /* most samples rendered as one set of lanes; 1 = one sample per launch (default 16)   RDR_BATCH */
    int64_t batch_lanes;            /* most lanes of such a set (default 2^24; 2^22 when another allocator holds > 10 % of
                                     * the device's memory)                                                                  RDR_BATCH_LANES */
    int workers;                    /* host threads that drive the batches of a gradient render (default: by size)         RDR_WORKERS */
    int refill_rays_per_lane, refill_idle_lanes, refill_steps;   /* trace_refill_kernel (4, 24, 4)                          RDR_TRACE_REFILL=k,idle,steps */
    int wide_max_rays;              /* queues of up to this many rays walk the 4-wide records (2^19)                       RDR_WIDE_MAX */
    int gather_budget;              /* pops per lane of SecEdgeGatherN before it hands over (256)                          RDR_GATHER_BUDGET */
    int gather_heavy_cap_plus1, gather_work_cap_plus1;   /* list capacities of the gather's hand-over paths, + 1 (tests: 1 = capacity 0)   RDR_GATHER_CAPS */
    int mem_available_mb;           /* size the batches as if this much device memory were free (tests)                    RDR_MEM_AVAILABLE_MB */
    int refill_order;               /* order in which trace_refill_kernel hands a wave's 256 rays out: 1 = queue order (rounds
                                     * 3-5), 2 = by direction octant (default), 3 = octant x dominant axis               RDR_REFILL_SORT=0|1|2 */
    int pickh_slots_per_lane, pickh_idle_lanes, pickh_steps;     /* the hierarchical pick's descent walk (1, 8, 8)           RDR_PICKH_REFILL=k,idle,steps */
    int stale_event_cap_plus1;      /* capacity, + 1, of the list of stale hit-position reads that a batched gradient render of an
                                     * environment-lit scene records (default: one per edge-ray lane); a list that overflows makes
                                     * the call start over unbatched (tests: 1 = capacity 0)                                 */
};

/* Library-wide settings (no reference counterpart).
 * rdr_set_stream: launches of later rdr_scene_create / rdr_render / rdr_scene_trace calls made by THIS host thread are
 *   ordered on `hip_stream` (a hipStream_t; NULL = the null stream, the default) -- a caller whose tensors are produced on
 *   a non-default stream (torch.cuda.stream(...)) passes that stream and needs no device-wide synchronisation of its own.
 *   The calls still return synchronised (like the reference, src/pathtracer.cpp:947-949).
 * rdr_set_pool_cap_mb: bound of the buffer cache per device (see rdr_trim_cache), default min(a quarter of the device, 8 GiB)
 *   or RDR_POOL_CAP_MB; a dedicated render process may raise it so that the ~48 GB of a 2^24-lane sample batch stay parked
 *   between calls.  Negative = back to the default.
 * rdr_set_build_flags: rdr_build_flags for later rdr_scene_create calls (debugging / tests). */
void rdr_set_stream(void *hip_stream);
void rdr_set_pool_cap_mb(int64_t megabytes);
int64_t rdr_get_pool_cap_mb(void);      /* the bound in effect on the calling thread's current device */
enum rdr_build_flags {
    RDR_BUILD_NO_REFIT        = 1 << 0,   /* no topology caches: hierarchies built from scratch every Scene   RDR_NO_REFIT */
    RDR_BUILD_NO_EDGE_CACHE   = 1 << 1,   /* edge structures never shared between Scenes                      RDR_NO_EDGE_CACHE */
    RDR_BUILD_SYNC_EDGES      = 1 << 2,   /* edge structures built inside rdr_scene_create                    RDR_SYNC_EDGES */
    RDR_BUILD_EDGE_HOST_BUILD = 1 << 3    /* edge hierarchies by the host builder                             RDR_EDGE_HOST_BUILD */
};
void rdr_set_build_flags(unsigned flags);

/* redner.DScene(...)  src/redner.cpp:75-82 */
typedef struct rdr_dscene_desc {
    rdr_dcamera_desc camera;
    const rdr_dshape_desc *shapes; int num_shapes;
    const rdr_dmaterial_desc *materials; int num_materials;
    const rdr_darea_light_desc *area_lights; int num_area_lights;
    const rdr_denvmap_desc *envmap;   /* or NULL */
} rdr_dscene_desc;

typedef struct rdr_scene rdr_scene;

/* redner.Scene(camera, shapes, materials, area_lights, envmap, use_gpu, gpu_index,
 *              use_primary_edge_sampling, use_secondary_edge_sampling)
 * src/redner.cpp:62-73, src/scene.cpp:63-307.  Copies the descriptors, keeps the data pointers
 * (the caller keeps the tensors alive), builds the triangle hierarchy, the light CDFs and the
 * edge-sampling structures.  Returns NULL on error. */
rdr_scene *rdr_scene_create(const rdr_camera_desc *camera,
                            const rdr_shape_desc *shapes, int num_shapes,
                            const rdr_material_desc *materials, int num_materials,
                            const rdr_area_light_desc *area_lights, int num_area_lights,
                            const rdr_envmap_desc *envmap,
                            int use_gpu, int gpu_index,
                            int use_primary_edge_sampling, int use_secondary_edge_sampling);
void rdr_scene_destroy(rdr_scene *scene);
/* Scene.max_generic_texture_dimension  src/redner.cpp:73 */
int rdr_scene_max_generic_texture_dimension(const rdr_scene *scene);

/* redner.render(scene, options, rendered_image, d_rendered_image, d_scene, screen_gradient_image,
 *               debug_image)   src/redner.cpp:257, src/pathtracer.cpp:177-958.
 * Forward iff rendered_image != NULL ([H_vp, W_vp, C] fp32 DEV, accumulated); backward iff
 * d_rendered_image != NULL (then d_scene must be given).  Synchronises the device before
 * returning, like the reference (src/pathtracer.cpp:947-949).  Returns 0 on success. */
int rdr_render(const rdr_scene *scene, const rdr_render_options *options,
               float *rendered_image, const float *d_rendered_image,
               const rdr_dscene_desc *d_scene,
               float *screen_gradient_image, float *debug_image);

/* redner.compute_num_channels(channels, max_generic_texture_dimension)  src/redner.cpp:201.
 * Returns -1 for an unknown channel id. */
int rdr_compute_num_channels(const int *channels, int num_channels, int max_generic_texture_dimension);

/* Deferred shading of a G-buffer (pyredner/render_utils.py:8-313: the four deferred lights, the loop over them, the
 * anti-aliasing resolve) and its adjoint, each one pass over the G-buffer (csrc/deferred.h).
 * The G-buffer is [num_images, height * aa_samples, width * aa_samples, 9 + alpha] fp32: position 3, shading normal 3, diffuse
 * reflectance 3 and, with alpha, alpha 1.  The image is [num_images, height, width, 3 + alpha]: per texel the sum over the lights
 * of its image, alpha passed through unshaded, the mean over each aa_samples x aa_samples block.
 * Lights are rows of one table: light_type[l] and light_params[l][10] = intensity 3, position 3, direction 3 (directional: its
 * direction; spot: the spot direction), spot exponent 1; entries a type does not use are ignored.  Image n is lit by the lights
 * [image_light_range[2n], image_light_range[2n+1]).
 *   ambient      I * a
 *   point        d = pos - p, l = d / |d|:            I * max(l.n, 0) * (a / pi) / d.d
 *   directional  l = -dir / |dir|:                    I * max(l.n, 0) * (a / pi)
 *   spot         l = (pos - p) / |pos - p|, s = -sdir / |sdir|:   I * pow(max(l.s, 0), e) * max(l.n, 0) * (a / pi)
 * SH ROWS (RDR_DL_SH_R, _G, _B; not in the reference): a row lights ONE colour channel c by a spherical-harmonic environment.
 * light_params[l][0..8] are the nine coefficients k_i of that channel in the order i = l*l + l + m of rdr_sh_reconstruct
 * (l = 0..2, m = -l..l); [9] is unused and its gradient is 0.  The basis and the directions are those of rdr_sh_reconstruct
 * and an environment map with identity env_to_world (the map's texel at (theta, phi) lies in world direction
 * (sin phi sin theta, cos theta, -cos phi sin theta)); there is no rotation of the SH frame.  With the normal as stored,
 * x = -n.z, y = n.x, z = n.y:
 *   Y0 = 0.28209479   Y1 = -0.48860251 y   Y2 = 0.48860251 z   Y3 = -0.48860251 x   Y4 = 1.09254843 x y   Y5 = -1.09254843 y z
 *   Y6 = 0.31539157 (3 z z - 1)   Y7 = -1.09254843 x z   Y8 = 0.54627422 (x x - y y)
 *   E = sum_i A_i k_i Y_i,  A = pi (l = 0), 2 pi / 3 (l = 1), pi / 4 (l = 2);   the row adds  max(E, 0) * a_c / pi  to channel c.
 * fp32, the sum in ascending i (csrc/deferred.h states the order of every operation).  At E == 0 exactly the clamp passes half
 * the gradient, like every max(x, 0) here: all-zero coefficients receive a gradient.  The position takes no part (its gradient
 * from an SH row is exactly 0).  A light with three colour channels is three consecutive rows (the Python SHLight); each row
 * is meaningful alone.
 * g_buffer, light_params, image, d_* are DEV pointers on device gpu_index (a negative gpu_index: host memory, which only the
 * CPU debugging harness accepts); with alpha the G-buffers must be 8-byte and the images 16-byte aligned.  The backward call
 * writes every element of d_g_buffer and d_light_params (no zero-filled buffers needed); the light gradients are summed in a
 * fixed order: bitwise reproducible from run to run.  Launches are ordered on the rdr_set_stream stream; both calls synchronise
 * before returning.  Return 0 on success.
 *
 * SHADOWS (not in the reference, whose render_deferred has none): with `occluders`, every texel of a shadowed image casts one
 * any-hit shadow ray per light over the triangles of its occluder scene, and a light that is blocked adds nothing to the texel.
 * The ray, in fp32 (csrc/deferred.h: shadow_ray): origin p, tmin = 1e-3f; point and spot: dir = (pos - p) / r with
 * r = |pos - p|, tmax = (1 - 1e-3f) * r; directional: dir = -dir_l / |dir_l|, tmax = +inf; ambient lights and SH rows cast none.  A ray is
 * cast only where dir.n > 0 (for a spot also dir.s > 0), r > 0 and the record is finite; elsewhere the light counts as reaching
 * the texel.  The texel is lit iff no triangle is hit in (tmin, tmax).
 *   - A shadowed image may have at most 32 lights in its range (one bit each in the texel's visibility word): more is an error
 *     that names the image and the count.  Bits go by row position, so SH rows count: three per SHLight.  Their bits stay set
 *     (occluders never dim an SH row).
 *   - A scene on another device than gpu_index, `occluders` without `visibility` and a `visibility` pointer that is not 4-byte
 *     aligned are errors, raised before anything is launched.
 *   - Visibility is a CONSTANT of the adjoint: rdr_deferred_shade_backward multiplies by the saved bits -- a light whose bit is 0
 *     adds nothing to the texel's gradient nor to its own -- and produces no gradient across a shadow boundary (shadows are hard
 *     and their edges are not differentiated).
 * Both fields NULL (a zeroed tail): no shadows, the same launches and the same bits as before the fields existed.
 *
 * AMBIENT OCCLUSION (not in the reference): with `ao_occluders`, the SKY rows of the light table -- RDR_DL_AMBIENT and
 * RDR_DL_SH_R / _G / _B, the rows that cast no shadow ray -- are dimmed by what is near the texel.  Every texel of an occluded
 * image casts K = ao_rays any-hit rays (1 .. 32), cosine-distributed about its shading normal, that end after ao_radius; with
 * o = popcount(word) / K, the fraction that escapes, a sky row adds o times what it adds without occlusion.  Point, directional
 * and spot rows are untouched: shadows are their business.  The two features are independent, and all four combinations work.
 * The rule, in fp32 (csrc/deferred.h: ao_ray, ao_directions):
 *   - A texel casts iff nn = n.n satisfies 0 < nn < inf and every float of p, of nh = n / sqrtf(nn) and of the ray is finite;
 *     background texels (normal 0) never cast.  A texel that does not cast has all K bits set: o = 1.
 *   - Local directions: a table l[16][K][3] computed on the HOST in fp64 and rounded once to fp32 (no trigonometry runs in a
 *     kernel): for ray r of rotation j, u1 = (r + 0.5) / K, u2 = the base-2 radical inverse of r, phi = 2 pi (u2 + (j + 0.5) / 16),
 *     l = (sqrt(u1) cos phi, sqrt(u1) sin phi, sqrt(1 - u1)); l.z >= sqrt(0.5 / K) >= 0.125.  The rotation of a texel is
 *     j = (x & 3) + 4 (y & 3), x and y its column and row in its own image of the G-buffer.  (The half step keeps phi off 0:
 *     a local direction with a component of exactly 0 gives, about an axis-aligned normal, a ray that the conservative box test
 *     of the traversal culls almost nothing for.)
 *   - Frame (Duff et al.): s = copysignf(1, nh.z), a = -1 / (s + nh.z), b = (nh.x nh.y) a, T = (1 + ((s nh.x) nh.x) a, s b,
 *     -(s nh.x)), B = (b, s + (nh.y nh.y) a, -nh.y).
 *   - Ray: dir[k] = (l.x T[k] + l.y B[k]) + l.z nh[k], origin p, tmin = 1e-3f, tmax = ao_radius.
 *   - Forward: a sky row's contribution is formed into a zeroed c[3], then rgb[k] += o * c[k], o = (float)popcount / (float)K;
 *     every other row accumulates as without occlusion, in the same order over the lights.
 *   - Occlusion is a CONSTANT of the adjoint: rdr_deferred_shade_backward calls a sky row's adjoint with o * w in place of the
 *     upstream gradient w (the texel's gradient and the row's own are both scaled; alpha is untouched), reads the saved words,
 *     traces nothing and needs no scene.  Nothing is differentiated through o.  With o == 1 both calls give the bits of the
 *     call without occlusion.
 *   - Errors, raised before anything is launched: ao_rays outside 1 .. 32 when either ao pointer is given; ao_radius that is
 *     not > 0 (NaN included; forward); one of the pair without the other (forward); an ao_words pointer that is not 4-byte
 *     aligned; a scene on another device than gpu_index.  The limit of 32 lights is that of SHADOWED images only.
 * A zeroed tail: no occlusion, the same launches and the same bits as before the fields existed. */
enum rdr_deferred_light_type { RDR_DL_AMBIENT = 0, RDR_DL_POINT = 1, RDR_DL_DIRECTIONAL = 2, RDR_DL_SPOT = 3,
                               RDR_DL_SH_R = 4, RDR_DL_SH_G = 5, RDR_DL_SH_B = 6 };
typedef struct rdr_deferred_desc {
    int num_images, height, width;      /* OUTPUT size */
    int aa_samples, alpha;
    int num_lights;
    const int32_t *light_type;          /* HOST [num_lights] */
    const int32_t *image_light_range;   /* HOST [num_images][2] */
    int gpu_index;
    const rdr_scene *const *occluders;  /* HOST [num_images], or NULL: no shadows.  occluders[n] == NULL: image n is not
                                           shadowed.  Every scene must live on device gpu_index (harness: host). */
    uint32_t *visibility;               /* DEV [num_images][height * aa_samples][width * aa_samples], required iff
                                           occluders != NULL (forward) / may be given alone (backward).  Bit b of a word: light
                                           range[2n] + b reaches the texel.  rdr_deferred_shade writes every word;
                                           rdr_deferred_shade_backward reads them and needs no scene.  Bits of ambient lights, of SH rows and
                                           of lights that cast no ray at the texel are 1; bits at and above the length of the
                                           image's range are 0. */
    const rdr_scene *const *ao_occluders; /* HOST [num_images], or NULL: no ambient occlusion.  ao_occluders[n] == NULL: image n
                                           is not occluded and every bit of its words is set.  May name other scenes than
                                           `occluders`.  Every scene must live on device gpu_index (harness: host). */
    uint32_t *ao_words;                 /* DEV [num_images][height * aa_samples][width * aa_samples], required iff
                                           ao_occluders != NULL (forward) / may be given alone (backward).  Bit r of a word:
                                           hemisphere ray r of the texel escaped, or the texel cast none; bits at and above
                                           ao_rays are 0.  rdr_deferred_shade writes every word; rdr_deferred_shade_backward
                                           reads them and needs no scene. */
    int ao_rays;                        /* K, 1 .. 32: hemisphere rays per texel */
    float ao_radius;                    /* > 0, +inf allowed: where the rays end */
} rdr_deferred_desc;
int rdr_deferred_shade(const rdr_deferred_desc *desc, const float *g_buffer, const float *light_params, float *image);
int rdr_deferred_shade_backward(const rdr_deferred_desc *desc, const float *g_buffer, const float *light_params,
                                const float *d_image, float *d_g_buffer, float *d_light_params);

/* The mip pyramid of an image texture (pyredner/texture.py:34-69, Texture.generate_mipmap) and its adjoint (csrc/mipmap.h).
 * texels are [height, width, channels] fp32, all three >= 1.  num_levels = min(ceil(log2(max(height, width))) + 1, 8)
 * (rdr_mip_num_levels); level l + 1 is max(Hl / 2, 1) x max(Wl / 2, 1), so a side that is not a power of two reaches 1 early and
 * the last levels repeat at 1 x 1.  A level is the 2 x 2 box filter of the level before it with WRAPPING indices, followed by
 * the mean over rows [floor(i Hp / Ho), ceil((i + 1) Hp / Ho)) and the like columns (interpolate(mode='area')): the wrapping
 * [1 2 1] x [1 2 1] / 16 filter at stride 2 for even sides, overlapping windows of 3 for odd sides, the identity for a side of 1.
 *   rdr_mip_pyramid           levels[0] is the caller's image (read); levels[1 .. num_levels) are written, every element.
 *   rdr_mip_pyramid_backward  d_texels = g_0 + A_1^T (g_1 + A_2^T (g_2 + ...)), g_l = d_levels[l], A_l = the map from level
 *                             l - 1 to level l.  d_levels[l] may be NULL (= zeros) and is not modified; every element of d_texels
 *                             [height, width, channels] is written.  `scratch` holds the partial sums of the levels between:
 *                             at least rdr_mip_backward_scratch(height, width, channels) floats in the same memory as the
 *                             tensors (may be NULL when that is 0); its contents afterwards are unspecified.
 * Both calls fail (rdr_last_error) if num_levels is not what the rule gives, if a size is not positive, a side exceeds 32768 or
 * the image 2^30 floats, or a required pointer is NULL.  Pointers are DEVICE memory of gpu_index; a negative gpu_index means
 * host memory and is accepted by the CPU debugging harness only.  fp32 arithmetic in a fixed order, gathers only, no atomics:
 * results are bitwise reproducible from run to run, and the harness computes the same bits as the kernels.  The library allocates
 * nothing.  One to three launches per call (one workgroup does a whole pyramid of up to 64 x 64 x 3 floats; otherwise a tiled
 * launch does three levels at a time while a level is larger than that, and one workgroup the rest: two launches up to
 * 512 x 512 x 3, three above; the same count backward), ordered on the rdr_set_stream stream and NOT synchronised: the results
 * are ready for later work on that stream.  Return 0 on success. */
int rdr_mip_num_levels(int height, int width);                                /* 0 for a size that is not positive */
int64_t rdr_mip_backward_scratch(int height, int width, int channels);        /* floats; -1 on error */
int rdr_mip_tiled_stages(int height, int width, int channels);                /* tiled launches of a call each way; -1 on error */
int rdr_mip_pyramid(int height, int width, int channels, int num_levels, float *const *levels, int gpu_index);
int rdr_mip_pyramid_backward(int height, int width, int channels, int num_levels, const float *const *d_levels, float *d_texels,
                             float *scratch, int64_t scratch_floats, int gpu_index);

/* An environment map from spherical-harmonic coefficients (pyredner/utils.py:10-60, SH_reconstruct), its adjoint, and the sampling
 * tables of an environment map (pyredner/envmap.py:36-60, generate_envmap_pdf); csrc/sh_envmap.h pins the meaning, the fp32
 * arithmetic and the summation orders.
 *   rdr_sh_reconstruct           image [height, width, channels] = max(sum_i Y_i(theta_r, phi_c) coeffs[ch, i], 0) from coeffs
 *                                [channels, num_coeffs] (contiguous); int(sqrt(num_coeffs)) bands, at most 8; the columns past
 *                                bands^2 are not read.  `clamp` [height, width, channels] bytes (may be NULL) receives twice the
 *                                derivative of the clamp: 2 where the sum is > 0, 0 where it is < 0, 1 at a tie.  One launch.
 *   rdr_sh_reconstruct_backward  d_coeffs [channels, num_coeffs], every element, from d_image and the forward call's `clamp`: a
 *                                reduction in a fixed order (fp64 partial sums per 32 x 32 tile in row-major order, the tiles in
 *                                ascending order, one rounding to fp32), no float atomics; the columns past bands^2 get 0.
 *                                `scratch`: at least rdr_sh_backward_scratch(...) floats, aligned to 8 bytes, in the same memory as
 *                                the tensors; its contents afterwards are unspecified.  Two launches.
 *   rdr_envmap_tables            sample_cdf_ys [height] and sample_cdf_xs [height, width] from texels [height, width, 3] and
 *                                y_weight [height] (the caller's sin(pi (y + 0.5) / height)), with the running sums taken as
 *                                torch.cumsum takes them on the CPU: a sequential fp64 accumulator rounded to fp32 at every output.
 *                                `*total` (HOST memory) receives the last unnormalised entry of the column table (pdf_norm is
 *                                height * width / (*total * 2 pi^2)).  Two launches and ONE synchronisation (that read-back).
 * The calls fail (rdr_last_error) for a size that is not positive, a side above 32768, an image above 2^30 floats, more than 8
 * bands, or a required pointer that is NULL.  Pointers are DEVICE memory of gpu_index; a negative gpu_index means host memory and is
 * accepted by the CPU debugging harness only.  Launches are ordered on the rdr_set_stream stream; the two SH calls are NOT
 * synchronised.  Results are bitwise reproducible from run to run, and the harness computes the same bits as the kernels.
 * Return 0 on success. */
int64_t rdr_sh_backward_scratch(int height, int width, int channels, int num_coeffs);     /* floats; -1 on error */
int rdr_sh_reconstruct(const float *coeffs, int channels, int num_coeffs, int height, int width, float *image, uint8_t *clamp,
                       int gpu_index);
int rdr_sh_reconstruct_backward(const uint8_t *clamp, const float *d_image, int channels, int num_coeffs, int height, int width,
                                float *d_coeffs, float *scratch, int64_t scratch_floats, int gpu_index);
int rdr_envmap_tables(const float *texels, const float *y_weight, int height, int width, float *sample_cdf_ys, float *sample_cdf_xs,
                      float *total, int gpu_index);

/* Smooth vertex normals of a triangle mesh (pyredner/shape.py:7-127, compute_vertex_normal) and their vertex adjoint
 * (csrc/vertex_normal.h, which pins the meaning, the arithmetic and the summation order).  vertices [V, 3] fp32, indices [T, 3]
 * int32, normals [V, 3] fp32.
 *   rdr_mesh_topology_create   the plan of one connectivity: validates (V >= 1, T >= 0, 3 T < 2^31, every index in [0, V); NULL
 *                              and rdr_last_error otherwise), copies `indices` and builds the rows of corners incident to every
 *                              vertex, each in ascending corner id 3 f + k.  `indices` is DEVICE memory of gpu_index when use_gpu
 *                              is set, host memory otherwise (accepted by the CPU debugging harness only).  Synchronises once.
 *                              Reuse the plan for every call with these indices; destroy it with rdr_mesh_topology_destroy.
 *   rdr_mesh_topology_read     test hook: row offsets [V + 1] and the corner list [3 T] into HOST memory.
 *   rdr_vertex_normal_scratch  floats the three buffers of a scheme need: `forward_floats` (scratch of rdr_vertex_normal),
 *                              `backward_floats` (scratch of rdr_vertex_normal_backward), `saved_floats` (what the forward
 *                              call saves for the backward call: the unnormalised sums).  Any of the three may be NULL.
 *   rdr_vertex_normal          writes every element of normals and saved.
 *   rdr_vertex_normal_backward writes every element of d_vertices [V, 3] from d_normals [V, 3], the vertices and `saved` of the
 *                              forward call.  The gradient of a degenerate corner or face, and of a vertex whose normal is the
 *                              (0, 0, 1) default, is 0.
 * The tensors and scratch are memory of the plan's place; the scratch contents afterwards are unspecified and it may be NULL
 * when the count is 0.  The library allocates nothing per call.  Two launches each way, ordered on the rdr_set_stream stream
 * and NOT synchronised.  Gathers and plain stores in a fixed order, no float atomics: bitwise reproducible from run to run,
 * and the harness computes the same bits as the kernels.  Return 0 on success. */
typedef enum { rdr_normal_weighting_max = 0, rdr_normal_weighting_cotangent = 1 } rdr_normal_weighting;
typedef struct rdr_mesh_topology rdr_mesh_topology;
rdr_mesh_topology *rdr_mesh_topology_create(const int *indices, int num_triangles, int num_vertices, int use_gpu, int gpu_index);
void rdr_mesh_topology_destroy(rdr_mesh_topology *topology);
int rdr_mesh_topology_read(const rdr_mesh_topology *topology, int *offsets, int *corners);
int rdr_vertex_normal_scratch(const rdr_mesh_topology *topology, int scheme, int64_t *forward_floats, int64_t *backward_floats,
                              int64_t *saved_floats);
int rdr_vertex_normal(const rdr_mesh_topology *topology, int scheme, const float *vertices, float *normals, float *saved,
                      float *scratch, int64_t scratch_floats);
int rdr_vertex_normal_backward(const rdr_mesh_topology *topology, int scheme, const float *vertices, const float *saved,
                               const float *d_normals, float *d_vertices, float *scratch, int64_t scratch_floats);

/* Laplacian smoothing on the plan above (rdr_mesh_boundary, rdr_mesh_smooth_scratch, rdr_mesh_laplacian, rdr_mesh_laplacian_backward,
 * rdr_mesh_smooth) is declared in its own header, redner_amd_mesh.h, which includes this one. */

/* Message of the last failure on the calling thread ("" if none). */
const char *rdr_last_error(void);

/* Measurement hooks (no reference counterpart; used by bench.py and the roofline report). */
typedef struct rdr_trace_stats {
    double closest_ms, any_ms;           /* accumulated device time of the two traversal kernels */
    uint64_t closest_launches, any_launches;
    uint64_t closest_rays, any_rays;
    /* 32-byte node records loaded / 36-byte triangle records tested, per query kind; only
     * counted when counting is enabled (instrumented kernel variant) */
    uint64_t closest_nodes, closest_tris, any_nodes, any_tris;
    /* 128-byte records of the 4-wide form of the hierarchy loaded (the kernels walk one form or the other per launch) */
    uint64_t closest_wide_nodes, any_wide_nodes;
    /* time during which at least one launch of the kind was in flight (union of the launches' intervals): equals closest_ms /
     * any_ms when launches of a kind never overlap, less when two sample workers trace side by side */
    double closest_union_ms, any_union_ms;
} rdr_trace_stats;
void rdr_trace_stats_enable(int timing, int counting);
void rdr_trace_stats_reset(void);
void rdr_trace_stats_get(rdr_trace_stats *out);

/* Closest-hit / any-hit queries on a batch of rays (DEV pointers; 32-byte ray records
 * {org.xyz, tmin, dir.xyz, tmax}, 8-byte hit records {shape, prim}).  This is the boundary the
 * reference crosses into Embree/OptiX (src/scene.cpp:503-597, 629-690); exposed for the
 * traversal parity tests and micro-benchmarks. */
int rdr_scene_trace(const rdr_scene *scene, const float *rays, int32_t *hits, int num_rays, int any_hit);

/* Per-call device buffers (the reference's PathBuffer, src/pathtracer.cpp:36-152, allocated and freed by every render())
 * come from a caching allocator: blocks are parked for the next call of the same shape (bounded by RDR_POOL_CAP_MB per device,
 * default a quarter of the device's memory).  rdr_trim_cache() returns every parked block to the driver -- for processes that share the device with
 * another allocator (torch) and change resolution.  Returns the number of bytes released. */
uint64_t rdr_trim_cache(void);

/* Test hook: how often the library has gone to the runtime for device memory (hipMalloc calls made by its caching allocator)
 * and how often the host has read a live-lane count back from the device, since the library was loaded.  A steady-state
 * rdr_render() adds nothing to either (the reference allocates its PathBuffer per call, src/pathtracer.cpp:36-152, and
 * reads a count after every stage, :292,590,833). */
typedef struct rdr_debug_counters {
    uint64_t device_mallocs, host_count_reads;
    uint64_t last_batch_samples, last_workers;      /* how the last gradient render of this process was scheduled: samples per launch set, host threads */
} rdr_debug_counters;
void rdr_debug_counters_get(rdr_debug_counters *out);

/* Test hook: the triangle hierarchy the kernels of this Scene built (bvh_gpu.cpp) against the host builder's on the same
 * arrays: the number of records that differ (0: identical), -1 when this Scene's hierarchy is a refit or was not built by
 * kernels, -2 on error. */
int rdr_debug_bvh_check(const rdr_scene *scene);

/* Test hook: writes the edge list and both edge hierarchies (links, edge ids, weights, costs) as
 * text, for the build-order parity test against the reference (tests/test_edge_build.py). */
int rdr_debug_dump_edges(const rdr_scene *scene, const char *path);

/* Test hook: the traversal launch the library would make (csrc/trace_plan.h: the rules) for a queue of num_rays rays on a
 * hierarchy of num_nodes node records whose binary / 4-wide walks need stack_need / wide_stack_need stack entries (has_wide:
 * the 4-wide records exist); `counting` as in rdr_trace_stats_enable; tuning NULL = every default and the environment.
 *   out[0] form: 0 trace_wide_kernel, 1 trace_refill_kernel, 2 trace_kernel      out[1] stack entries of the instantiation
 *   out[2] 16-bit stack entries   out[3] hierarchy top staged in LDS   out[4] rays handed out in refill_order (refill)
 *   out[5] counting variant       out[6] workgroups                    out[7 .. 9] rays per lane, idle lanes, steps (refill; else 0)
 * rdr_debug_scene_trace_plan: the same for the hierarchy of a Scene, i.e. what rdr_scene_trace(scene, ..., num_rays, any_hit)
 * launches.  Host arithmetic only (no device is touched).  Return 0, or 1 (rdr_last_error) for num_rays <= 0, a negative
 * size or a NULL out / scene. */
int rdr_debug_trace_plan(int num_nodes, int stack_need, int has_wide, int wide_stack_need, int num_rays, int any_hit, int coherent,
                         int counting, const rdr_tuning *tuning, int32_t *out /* [10] */);
int rdr_debug_scene_trace_plan(const rdr_scene *scene, int num_rays, int any_hit, int coherent, int counting,
                               const rdr_tuning *tuning, int32_t *out /* [10] */);

/* The library is built twice from the same sources (__graft_entry__.build_native):
 *   libredner_amd.so        the stage kernels call the DEVICE's own sin / cos / atan2 / atan / acos / log / pow (ocml): the
 *                           default, +1 ... 3 % throughput; every result is an equally valid sample of the same estimator, and
 *                           sample-for-sample equal to the reference wherever no transcendental feeds a chaotic decision
 *                           (perspective / orthographic cameras: all BASELINE configs);
 *   libredner_amd_exact.so  they call restatements of glibc 2.35's routines (csrc/libm_exact.h, see NOTICE), bit for bit what
 *                           the reference's CPU path computes: fisheye / panorama cameras with secondary edge sampling are then
 *                           sample-exact too.  The parity tests load this one (REDNER_AMD_LIBM=exact, redner_amd/_capi.py).
 * rdr_libm_exact(): 1 in the second, 0 in the first. */
int rdr_libm_exact(void);

/* Test hook: sin / cos / atan2 / atan / acos / log / pow as the EXACT routines evaluate them (in either build) (csrc/libm_exact.h: glibc 2.35's
 * results bit for bit -- the reference's CPU path calls glibc, src/camera.h:142-191, src/material.h, src/envmap.h), one
 * argument per lane; HOST pointers, `y` may be NULL for the one-argument functions.
 * fn: 0 sin(x), 1 cos(x), 2 atan2(x, y), 3 atan(x), 4 acos(x), 5 log(x), 6 pow(x, y). */
int rdr_debug_libm(int fn, const double *x, const double *y, double *out, int n);

/* Test hook: the gradient scatter alone.  Builds the gradient store of a gradient render of `scene` into `d_scene` (the struct
 * rdr_render takes; `job_samples` sizes the replicas of its large tier as pixels x samples of a render would), launches ONE
 * stage of `num_lanes` lanes in which lane i -- unless active[i] == 0: it returns first, as the lanes of production stages that
 * have nothing to add do -- makes one call of `op`, and folds the store into the fp32 tensors of `d_scene` (+=, as a render).
 * All per-lane arrays are HOST memory.
 *   RDR_SCATTER_ACCUM / _ACCUM_TEXEL / _ACCUM_PLAIN      values[i] is added to element index[i] of the lane's target
 *   RDR_SCATTER_ACCUM_TRIPLE / _ACCUM_TEXEL_TRIPLE       values[3 i .. 3 i + 2] to elements index[i] .. index[i] + 2
 *     target[3 i .. 3 i + 2] = (kind, a, b), kind an rdr_scatter_target:
 *       VERTICES / UVS / NORMALS / COLORS  of shape a            TEXTURE  level b % 8 of texture b / 8 (0 diffuse, 1 specular,
 *       2 roughness, 3 generic, 4 normal map) of material a      LIGHTS   the intensities, 3 per area light
 *       CAMERA  field a (the order of rdr_dcamera_desc)          ENVMAP   level b of the environment map's values
 *   RDR_SCATTER_TRIGRAD_WAVE     target[3 i], target[3 i + 1] = (shape, triangle), shape < 0: nothing; values[33 i ...] = the
 *                                corner gradients p[3], n[3] (3 doubles each), uv[3] (2 each), c[3] (3 each); `plain` as the
 *                                lean stages pass it (no uv / colour gradients); `index` is not read
 *   RDR_SCATTER_POSITIONS_WAVE   the same with values[9 i ...] = p[3]
 * Every lane, active or not, is checked on the host first: a target that `d_scene` does not ask for or an element, shape or
 * triangle out of range returns 1 (rdr_last_error) before anything is launched. */
enum rdr_scatter_op {
    RDR_SCATTER_ACCUM = 0, RDR_SCATTER_ACCUM_TEXEL, RDR_SCATTER_ACCUM_PLAIN, RDR_SCATTER_ACCUM_TRIPLE,
    RDR_SCATTER_ACCUM_TEXEL_TRIPLE, RDR_SCATTER_TRIGRAD_WAVE, RDR_SCATTER_POSITIONS_WAVE
};
enum rdr_scatter_target {
    RDR_TARGET_VERTICES = 0, RDR_TARGET_UVS, RDR_TARGET_NORMALS, RDR_TARGET_COLORS, RDR_TARGET_TEXTURE, RDR_TARGET_LIGHTS,
    RDR_TARGET_CAMERA, RDR_TARGET_ENVMAP
};
int rdr_debug_grad_scatter(const rdr_scene *scene, const rdr_dscene_desc *d_scene, uint64_t job_samples, int op, int plain,
                           int num_lanes, const uint8_t *active, const int32_t *target, const int32_t *index,
                           const double *values);

/* Test hooks: the three integer primitives that decide order, each alone (tests/test_exec_primitives.py).  All arrays are HOST
 * memory; the hook allocates from the library's pool, uploads, launches on the calling thread's stream and downloads.  Every
 * argument is checked on the host first: a bad one returns 1 (rdr_last_error names the hook) before anything is launched.
 *
 * rdr_debug_compact: one stable stream compaction (exec::compact_dev, or exec::compact when host_form = 1) of the list
 *   in[0 .. min(count, upper)) -- in = NULL: the identity 0, 1, ... -- under the predicate keep[value] != 0.
 *   upper          bound of the input count (0 .. 2^24)
 *   count          < 0: the count is the host-only Count(upper); else a device int holding this value (above `upper`: it clamps)
 *   in             `upper` values, each in [0, keep_len); NULL needs keep_len >= upper
 *   append_upper   < 0: the kept items go to out[0 ...]; else they continue a list of `append_count` items (0 <= append_count
 *                  <= append_upper, the count on the device, append_upper its bound)
 *   dyn_inc        != 0: compact_dev is handed a device counter, which starts at result[2] and advances by dyn_inc when the
 *                  input list is not empty
 *   scratch        0 or 1: which compaction scratch of the calling thread
 *   host_form      1: exec::compact, which reads the count back; only with count < 0, no append, dyn_inc = 0, no pos_out, scratch 0
 *   out            max(append_upper, 0) + upper ints, uploaded before the call and downloaded after it: the caller sees every slot
 *   pos_out        NULL, or as `out`: pos_out[k] = position in the input list of the k-th kept item
 *   result[4]      [0] the count after the call, as the device holds it   [1] the bound of the returned Count
 *                  [2] in: the dyn counter's start, out: its value after the call   [3] what the host form returned, or -1
 *
 * rdr_debug_walk: `repeat` launches back to back (no host synchronisation between them) of a walk over min(count, upper) items
 *   through kind 0 exec::launch_persistent, 1 exec::launch_chunked(items_per_lane, idle_min, steps), 2 exec::launch (begin, all
 *   steps and finish in one lane).  Item i walks len[i] steps (0 .. 65536; 0: begin returns false): begin adds 1 to begun[i],
 *   step k = 1, 2, ... adds i * 31 + k to a 32-bit sum, finish adds 1 to finished[i] and stores the number of steps in
 *   steps_taken[i] and the sum in acc[i] = (len * i * 31 + len * (len + 1) / 2) mod 2^32.  The four output arrays (`upper` entries)
 *   are uploaded first, like `out` above.  items_per_lane 1 .. 64, idle_min 1 .. 64, steps 1 .. 1024 (what rdr_tuning clamps to);
 *   gate_closed 0 or 1 (kind 0 only: the walker's gate_closed() reads a device flag of this value); repeat 1 .. 65536;
 *   upper 0 .. 2^24; count as above.
 *
 * rdr_debug_sort_pairs: the stable 64-bit radix sort of the edge hierarchies' builder on n (1 .. 2^24) pairs. */
int rdr_debug_compact(int upper, int count, const int32_t *in, const uint8_t *keep, int keep_len, int append_upper, int append_count,
                      int dyn_inc, int scratch, int host_form, int32_t *out, int32_t *pos_out, int32_t *result /* [4] */);
int rdr_debug_walk(int kind, int upper, int count, const int32_t *len, int items_per_lane, int idle_min, int steps, int gate_closed,
                   int repeat, int32_t *begun, int32_t *finished, int32_t *steps_taken, uint32_t *acc);
int rdr_debug_sort_pairs(const uint64_t *keys, const int32_t *vals, int n, uint64_t *keys_out, int32_t *vals_out);

#ifdef __cplusplus
}
#endif
#endif /* REDNER_AMD_H */
