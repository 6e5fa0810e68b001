"""ctypes binding of the C ABI in include/redner_amd.h and its companion headers (redner_amd_mesh.h, _image.h, _pose.h, _debug.h;
csrc/deferred_specular_abi.h, csrc/deferred_quad_abi.h, csrc/deferred_quad_shadow_abi.h).

The shared library is the product: `redner_amd/lib/libredner_amd.so`, built by
`__graft_entry__.build()` (hipcc, gfx950).  If it is missing the import fails loudly -- there is
no CPU fallback.  `load(path)` exists so the test-suite can point the binding at the
single-threaded debugging harness under tests/hostsim/ (test infrastructure); product code never
calls it with an argument.
"""
import ctypes as C
import os

MAX_MIP = 8
_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIBRARY = os.path.join(_HERE, 'lib', 'libredner_amd.so')
# the same library with glibc-exact transcendental functions in its kernels (include/redner_amd.h: rdr_libm_exact):
# REDNER_AMD_LIBM=exact selects it (the parity tests do, tests/conftest.py)
EXACT_LIBRARY = os.path.join(_HERE, 'lib', 'libredner_amd_exact.so')

c_float_p = C.POINTER(C.c_float)
c_int_p = C.POINTER(C.c_int32)


class CameraDesc(C.Structure):
    _fields_ = [('width', C.c_int), ('height', C.c_int),
                ('position', C.c_void_p), ('look', C.c_void_p), ('up', C.c_void_p),
                ('cam_to_world', C.c_void_p), ('world_to_cam', C.c_void_p),
                ('intrinsic_mat_inv', C.c_void_p), ('intrinsic_mat', C.c_void_p),
                ('distortion_params', C.c_void_p),
                ('clip_near', C.c_float), ('camera_type', C.c_int),
                ('viewport_beg', C.c_int * 2), ('viewport_end', C.c_int * 2)]


class DCameraDesc(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ('position', 'look', 'up', 'cam_to_world', 'world_to_cam',
                                          'intrinsic_mat_inv', 'intrinsic_mat', 'distortion_params')]


class ShapeDesc(C.Structure):
    _fields_ = [('vertices', C.c_void_p), ('indices', C.c_void_p), ('uvs', C.c_void_p),
                ('normals', C.c_void_p), ('uv_indices', C.c_void_p), ('normal_indices', C.c_void_p),
                ('colors', C.c_void_p),
                ('num_vertices', C.c_int), ('num_uv_vertices', C.c_int), ('num_normal_vertices', C.c_int),
                ('num_triangles', C.c_int), ('material_id', C.c_int), ('light_id', C.c_int)]


class DShapeDesc(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ('vertices', 'uvs', 'normals', 'colors')]


class TextureDesc(C.Structure):
    _fields_ = [('texels', C.c_void_p * MAX_MIP), ('width', C.c_int * MAX_MIP), ('height', C.c_int * MAX_MIP),
                ('channels', C.c_int), ('num_levels', C.c_int), ('uv_scale', C.c_void_p)]


class MaterialDesc(C.Structure):
    _fields_ = [('diffuse_reflectance', TextureDesc), ('specular_reflectance', TextureDesc),
                ('roughness', TextureDesc), ('generic_texture', TextureDesc), ('normal_map', TextureDesc),
                ('compute_specular_lighting', C.c_int), ('two_sided', C.c_int), ('use_vertex_color', C.c_int)]


class DTextureDesc(C.Structure):
    _fields_ = [('texels', C.c_void_p * MAX_MIP), ('num_levels', C.c_int), ('uv_scale', C.c_void_p)]


class DMaterialDesc(C.Structure):
    _fields_ = [(n, DTextureDesc) for n in ('diffuse_reflectance', 'specular_reflectance', 'roughness',
                                            'generic_texture', 'normal_map')]


class AreaLightDesc(C.Structure):
    _fields_ = [('shape_id', C.c_int), ('intensity', C.c_float * 3), ('two_sided', C.c_int),
                ('directly_visible', C.c_int)]


class DAreaLightDesc(C.Structure):
    _fields_ = [('intensity', C.c_void_p)]


class EnvmapDesc(C.Structure):
    _fields_ = [('values', TextureDesc), ('env_to_world', C.c_void_p), ('world_to_env', C.c_void_p),
                ('sample_cdf_ys', C.c_void_p), ('sample_cdf_xs', C.c_void_p),
                ('pdf_norm', C.c_float), ('directly_visible', C.c_int)]


class DEnvmapDesc(C.Structure):
    _fields_ = [('values', DTextureDesc), ('world_to_env', C.c_void_p)]


class Tuning(C.Structure):
    """rdr_tuning: every field 0 = the library's default (include/redner_amd.h)."""
    _fields_ = [('flags', C.c_uint), ('batch_samples', C.c_int), ('batch_lanes', C.c_int64), ('workers', C.c_int),
                ('refill_rays_per_lane', C.c_int), ('refill_idle_lanes', C.c_int), ('refill_steps', C.c_int),
                ('wide_max_rays', C.c_int), ('gather_budget', C.c_int),
                ('gather_heavy_cap_plus1', C.c_int), ('gather_work_cap_plus1', C.c_int), ('mem_available_mb', C.c_int),
                ('refill_order', C.c_int), ('pickh_slots_per_lane', C.c_int), ('pickh_idle_lanes', C.c_int), ('pickh_steps', C.c_int),
                ('stale_event_cap_plus1', C.c_int)]


# rdr_tune_flags / rdr_build_flags
TUNE_NO_OVERLAP, TUNE_FORCE_GENERAL, TUNE_PICKN_WALK, TUNE_PICKH_FUSED, TUNE_PICKH_LAZY, TUNE_NO_HOIST, TUNE_REFILL_OFF, \
    TUNE_REFILL_ALL, TUNE_TRACE_BINARY, TUNE_TRACE_NO_LDS_TOP, TUNE_NO_FUSED_BOUNCE, TUNE_PICKH_ONE_LAUNCH, TUNE_NO_NEE_COMPACT, \
    TUNE_LARGE_FORMS, TUNE_TRACE_EVERY_CONTINUATION = [1 << k for k in range(15)]
BUILD_NO_REFIT, BUILD_NO_EDGE_CACHE, BUILD_SYNC_EDGES, BUILD_EDGE_HOST_BUILD = [1 << k for k in range(4)]


class RenderOptionsDesc(C.Structure):
    _fields_ = [('seed', C.c_uint64), ('num_samples', C.c_int), ('max_bounces', C.c_int),
                ('channels', C.POINTER(C.c_int)), ('num_channels', C.c_int),
                ('sampler_type', C.c_int), ('sample_pixel_center', C.c_int),
                ('sample_offset', C.c_int), ('total_samples', C.c_int),
                ('tuning', C.POINTER(Tuning))]


class DSceneDesc(C.Structure):
    _fields_ = [('camera', DCameraDesc),
                ('shapes', C.POINTER(DShapeDesc)), ('num_shapes', C.c_int),
                ('materials', C.POINTER(DMaterialDesc)), ('num_materials', C.c_int),
                ('area_lights', C.POINTER(DAreaLightDesc)), ('num_area_lights', C.c_int),
                ('envmap', C.POINTER(DEnvmapDesc))]


class TraceStats(C.Structure):
    _fields_ = [('closest_ms', C.c_double), ('any_ms', C.c_double),
                ('closest_launches', C.c_uint64), ('any_launches', C.c_uint64),
                ('closest_rays', C.c_uint64), ('any_rays', C.c_uint64),
                ('closest_nodes', C.c_uint64), ('closest_tris', C.c_uint64),
                ('any_nodes', C.c_uint64), ('any_tris', C.c_uint64),
                ('closest_wide_nodes', C.c_uint64), ('any_wide_nodes', C.c_uint64),
                ('closest_union_ms', C.c_double), ('any_union_ms', C.c_double)]


class DebugCounters(C.Structure):
    _fields_ = [('device_mallocs', C.c_uint64), ('host_count_reads', C.c_uint64),
                ('last_batch_samples', C.c_uint64), ('last_workers', C.c_uint64)]


class DeferredDesc(C.Structure):
    """rdr_deferred_desc (include/redner_amd.h)."""
    _fields_ = [('num_images', C.c_int), ('height', C.c_int), ('width', C.c_int),
                ('aa_samples', C.c_int), ('alpha', C.c_int), ('num_lights', C.c_int),
                ('light_type', c_int_p), ('image_light_range', c_int_p), ('gpu_index', C.c_int),
                ('occluders', C.POINTER(C.c_void_p)), ('visibility', C.c_void_p),      # shadows; zeroed = none
                ('ao_occluders', C.POINTER(C.c_void_p)), ('ao_words', C.c_void_p),     # ambient occlusion; zeroed = none
                ('ao_rays', C.c_int), ('ao_radius', C.c_float)]


# rdr_deferred_light_type
DL_AMBIENT, DL_POINT, DL_DIRECTIONAL, DL_SPOT, DL_SH_R, DL_SH_G, DL_SH_B = range(7)

_p, _i, _i64 = C.c_void_p, C.c_int, C.c_int64
# Every function of the C ABI, under the header of include/ that declares it: header -> {name: (restype, argtypes)}.  load()
# requires every name of the loaded library and sets both on each function; a handle or pointer without argtypes would go through
# ctypes' default int conversion (tests/test_capi.py compares this table with the headers and the libraries' exports).
HEADERS = {
    'redner_amd.h': {
        'rdr_last_error': (C.c_char_p, []),
        'rdr_scene_create': (_p, [C.POINTER(CameraDesc), C.POINTER(ShapeDesc), _i, C.POINTER(MaterialDesc), _i,
                                  C.POINTER(AreaLightDesc), _i, C.POINTER(EnvmapDesc), _i, _i, _i, _i]),
        'rdr_scene_destroy': (None, [_p]),
        'rdr_scene_max_generic_texture_dimension': (_i, [_p]),
        'rdr_render': (_i, [_p, C.POINTER(RenderOptionsDesc), _p, _p, C.POINTER(DSceneDesc), _p, _p]),
        'rdr_compute_num_channels': (_i, [C.POINTER(C.c_int), _i, _i]),
        'rdr_trace_stats_enable': (None, [_i, _i]),
        'rdr_trace_stats_reset': (None, []),
        'rdr_trace_stats_get': (None, [C.POINTER(TraceStats)]),
        'rdr_scene_trace': (_i, [_p, _p, _p, _i, _i]),
        'rdr_trim_cache': (C.c_uint64, []),
        'rdr_set_stream': (None, [_p]),
        'rdr_set_pool_cap_mb': (None, [_i64]),
        'rdr_get_pool_cap_mb': (_i64, []),
        'rdr_set_build_flags': (None, [C.c_uint]),
        'rdr_libm_exact': (_i, []),
        'rdr_deferred_shade': (_i, [C.POINTER(DeferredDesc), _p, _p, _p]),
        'rdr_deferred_shade_backward': (_i, [C.POINTER(DeferredDesc), _p, _p, _p, _p, _p]),
        'rdr_mip_num_levels': (_i, [_i, _i]),
        'rdr_mip_backward_scratch': (_i64, [_i, _i, _i]),
        'rdr_mip_tiled_stages': (_i, [_i, _i, _i]),
        'rdr_mip_pyramid': (_i, [_i, _i, _i, _i, C.POINTER(_p), _i]),
        'rdr_mip_pyramid_backward': (_i, [_i, _i, _i, _i, C.POINTER(_p), _p, _p, _i64, _i]),
        'rdr_sh_backward_scratch': (_i64, [_i] * 4),
        'rdr_sh_reconstruct': (_i, [_p] + [_i] * 4 + [_p, _p, _i]),
        'rdr_sh_reconstruct_backward': (_i, [_p, _p] + [_i] * 4 + [_p, _p, _i64, _i]),
        'rdr_envmap_tables': (_i, [_p, _p, _i, _i, _p, _p, C.POINTER(C.c_float), _i]),
        'rdr_mesh_topology_create': (_p, [_p, _i, _i, _i, _i]),
        'rdr_mesh_topology_destroy': (None, [_p]),
        'rdr_mesh_topology_read': (_i, [_p, _p, _p]),
        'rdr_vertex_normal_scratch': (_i, [_p, _i, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)]),
        'rdr_vertex_normal': (_i, [_p, _i, _p, _p, _p, _p, _i64]),
        'rdr_vertex_normal_backward': (_i, [_p, _i, _p, _p, _p, _p, _p, _i64]),
        'rdr_debug_counters_get': (None, [C.POINTER(DebugCounters)]),
        'rdr_debug_dump_edges': (_i, [_p, C.c_char_p]),
        'rdr_debug_bvh_check': (_i, [_p]),
        'rdr_debug_libm': (_i, [_i, _p, _p, _p, _i]),
        'rdr_debug_trace_plan': (_i, [_i] * 8 + [C.POINTER(Tuning), _p]),
        'rdr_debug_scene_trace_plan': (_i, [_p] + [_i] * 4 + [C.POINTER(Tuning), _p]),
        'rdr_debug_grad_scatter': (_i, [_p, C.POINTER(DSceneDesc), C.c_uint64, _i, _i, _i, _p, _p, _p, _p]),
        'rdr_debug_compact': (_i, [_i, _i, _p, _p] + [_i] * 6 + [_p] * 3),
        'rdr_debug_walk': (_i, [_i, _i, _i, _p] + [_i] * 5 + [_p] * 4),
        'rdr_debug_sort_pairs': (_i, [_p, _p, _i, _p, _p]),
    },
    'redner_amd_mesh.h': {                   # Laplacian smoothing (csrc/mesh_smooth.h)
        'rdr_mesh_boundary': (_i, [_p, _p]),
        'rdr_mesh_smooth_scratch': (_i, [_p, _i, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)]),
        'rdr_mesh_laplacian': (_i, [_p, _i, _p, _p, _p, _p, _p, _i64]),
        'rdr_mesh_laplacian_backward': (_i, [_p, _i, _p, _p, _p, _p, _p, _p, _i64]),
        'rdr_mesh_smooth': (_i, [_p, _i, _p, _p, C.c_float, _i, _p, _p, _i64]),
    },
    'redner_amd_image.h': {                  # the Gaussian pyramid loss (csrc/pyramid_loss.h)
        'rdr_pyramid_loss_scratch': (_i, [_i] * 5 + [C.POINTER(_i64), C.POINTER(_i64)]),
        'rdr_pyramid_loss_plan': (_i, [_i] * 5 + [C.POINTER(_i), C.POINTER(_i)]),
        'rdr_pyramid_loss': (_i, [_p, _p] + [_i] * 5 + [c_float_p, C.c_float, _p, _p, _p, _i64, _i]),
        'rdr_pyramid_loss_backward': (_i, [_p, _p] + [_i] * 5 + [c_float_p, C.c_float, _p, _i64, _p, _p, _p, _p, _i64, _i]),
    },
    'redner_amd_pose.h': {                   # the rigid pose (csrc/pose.h)
        'rdr_pose_scratch': (_i, [_i, c_int_p, C.POINTER(_i64), C.POINTER(_i64)]),
        'rdr_pose_plan': (_i, [_i, c_int_p, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
        'rdr_rotate_matrix': (_i, [_p, _p, _i]),
        'rdr_rotate_matrix_backward': (_i, [_p, _p, _p, _i]),
        'rdr_pose_vertices': (_i, [_i, C.POINTER(_p), c_int_p, _p, _p, _p, C.POINTER(_p), _p, _p, _i64, _i]),
        'rdr_pose_vertices_backward': (_i, [_i, C.POINTER(_p), c_int_p, _p, _p, _i, C.POINTER(_p), C.POINTER(_p), _p, _p, _p, _p, _i64, _i]),
    },
    'redner_amd_debug.h': {                  # test hooks that came after redner_amd.h was fixed
        'rdr_debug_lane_park': (_i, [_i, _p, _p, _p, _p]),
        'rdr_debug_scene_trace': (_i, [_p, _p, _p, _i, _i, _i, C.POINTER(Tuning), _i, _p]),
        'rdr_debug_trace_occupancy': (_i, [_p, _p, _i, _i, _i, _p]),
    },
}

# Companion headers that stand under redner_amd/csrc/ (the set of files under include/ is fixed): bound by load() like HEADERS
CSRC_HEADERS = {
    'deferred_specular_abi.h': {             # specular highlights in deferred shading (csrc/deferred_specular.h)
        'rdr_deferred_specular': (_i, [C.POINTER(DeferredDesc), _p, _p, _p, _p, _p]),
        'rdr_deferred_specular_backward': (_i, [C.POINTER(DeferredDesc)] + [_p] * 9),
    },
    'deferred_quad_abi.h': {                 # rectangular area lights in deferred shading (csrc/deferred_quad.h)
        'rdr_deferred_quad': (_i, [C.POINTER(DeferredDesc), _p, _p, _p]),
        'rdr_deferred_quad_backward': (_i, [C.POINTER(DeferredDesc)] + [_p] * 5),
    },
    'deferred_quad_shadow_abi.h': {          # soft shadows of the quad lights (csrc/deferred_quad_shadow.h)
        'rdr_deferred_quad_shadowed': (_i, [C.POINTER(DeferredDesc), _p, _p, _i, _p, _p]),
        'rdr_deferred_quad_shadowed_backward': (_i, [C.POINTER(DeferredDesc)] + [_p] * 6),
    },
}

# rdr_scatter_op / rdr_scatter_target (rdr_debug_grad_scatter)
SCATTER_ACCUM, SCATTER_ACCUM_TEXEL, SCATTER_ACCUM_PLAIN, SCATTER_ACCUM_TRIPLE, SCATTER_ACCUM_TEXEL_TRIPLE, \
    SCATTER_TRIGRAD_WAVE, SCATTER_POSITIONS_WAVE = range(7)
TARGET_VERTICES, TARGET_UVS, TARGET_NORMALS, TARGET_COLORS, TARGET_TEXTURE, TARGET_LIGHTS, TARGET_CAMERA, TARGET_ENVMAP = range(8)

_lib = None
_lib_path = None


def load(path=None):
    """Load the C-ABI library (default: the HIP build).  Raises RuntimeError when it is missing."""
    global _lib, _lib_path
    # REDNER_AMD_LIB: another build of the same library (A/B of two builds inside one GPU session, tools/gpu_ab_builds.sh)
    path = path or os.environ.get('REDNER_AMD_LIB') or \
        (EXACT_LIBRARY if os.environ.get('REDNER_AMD_LIBM', '').lower() == 'exact' else DEFAULT_LIBRARY)
    if not os.path.exists(path):
        raise RuntimeError(
            "redner_amd: native library %s not found. Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950). "
            "There is no CPU fallback." % path)
    lib = C.CDLL(path)
    signatures = [item for table in list(HEADERS.values()) + list(CSRC_HEADERS.values()) for item in table.items()]
    for name, _ in signatures:
        if not hasattr(lib, name):
            raise RuntimeError("redner_amd: %s does not export %s" % (path, name))
    for name, (restype, argtypes) in signatures:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib, _lib_path = lib, path
    return lib


def use(handle, path):
    """Make a library that load() returned earlier the current one again (tools that alternate two builds in one process).
    Nothing in the package keeps a handle across calls: every entry point asks lib(); a Scene or MeshTopology keeps the one it was built with."""
    global _lib, _lib_path
    _lib, _lib_path = handle, path


def lib():
    if _lib is None:
        load()
    return _lib


def library_path():
    return _lib_path


def is_product_library():
    """The loaded library is one of the two HIP builds (not the CPU debugging harness, not an A/B variant)."""
    return _lib_path in (DEFAULT_LIBRARY, EXACT_LIBRARY)


def last_error():
    return lib().rdr_last_error().decode('utf-8', 'replace')
