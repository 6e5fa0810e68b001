"""`redner` -- drop-in mirror of the reference's pybind11 module (src/redner.cpp:20-272) on top of
the MI355X-native C ABI (include/redner_amd.h).

Same class names, constructor argument order and attributes as the reference, so that the
unmodified `pyredner/render_pytorch.py` runs against it:

    import redner_amd; redner_amd.install()     # registers this module as `redner`
    import pyredner                              # the reference's Python package, unchanged

What `render_pytorch.py` touches (rendering) is mirrored in full; of the asset helpers only `load_serialized` is
provided (pure Python: zlib + numpy), so that `pyredner.load_mitsuba('scenes/bunny_box.xml')` -- the reference's own
tests/test_bunny_box.py -- runs on this module; `automatic_uv_map` / `rebuild_topology` (xatlas, host-side mesh
processing) raise NotImplementedError (out of scope).
Errors raise RuntimeError instead of aborting the process (the reference: assert / exit(1)).
"""
import ctypes as C
import enum
import sys
import struct
import zlib

from . import _capi


def _addr(p):
    if p is None:
        return 0
    if isinstance(p, (float_ptr, int_ptr)):
        return p.addr
    return int(p)


def _ptr(p):
    """The address as a c_void_p argument of the C ABI takes it: None for NULL (a null float_ptr included)"""
    if p is None:
        return None
    return (p.addr if isinstance(p, (float_ptr, int_ptr)) else int(p)) or None


class float_ptr:                       # src/redner.cpp:23-24, src/ptr.h:10-24
    def __init__(self, addr):
        self.addr = int(addr)


class int_ptr:                         # src/redner.cpp:25-26
    def __init__(self, addr):
        self.addr = int(addr)


class CameraType(enum.IntEnum):        # src/redner.cpp:28-32
    perspective = 0
    orthographic = 1
    fisheye = 2
    panorama = 3


class channels(enum.IntEnum):          # src/redner.cpp:183-199
    radiance = 0
    alpha = 1
    depth = 2
    position = 3
    geometry_normal = 4
    shading_normal = 5
    uv = 6
    barycentric_coordinates = 7
    diffuse_reflectance = 8
    specular_reflectance = 9
    roughness = 10
    generic_texture = 11
    vertex_color = 12
    shape_id = 13
    triangle_id = 14
    material_id = 15


class SamplerType(enum.IntEnum):       # src/redner.cpp:203-205
    independent = 0
    sobol = 1


class Vector2i:                        # src/redner.cpp:218-221
    def __init__(self, x, y):
        self.x, self.y = int(x), int(y)


class Vector2f:
    def __init__(self, x, y):
        self.x, self.y = float(x), float(y)


class Vector3f:
    def __init__(self, x, y, z):
        self.x, self.y, self.z = float(x), float(y), float(z)


def _host_floats(addr, n):
    return list((C.c_float * n).from_address(addr)) if addr else None


class Camera:                          # src/redner.cpp:34-50
    def __init__(self, width, height, position, look, up, cam_to_world, world_to_cam,
                 intrinsic_mat_inv, intrinsic_mat, distortion_params, clip_near, camera_type,
                 viewport_beg, viewport_end):
        d = _capi.CameraDesc()
        d.width, d.height = int(width), int(height)
        # camera pointers are HOST memory read now (src/camera.h:44-65): snapshot them
        self._keep = []

        def snap(p, n):
            vals = _host_floats(_addr(p), n)
            if vals is None:
                return None
            arr = (C.c_float * n)(*vals)
            self._keep.append(arr)
            return C.cast(arr, C.c_void_p)

        d.position, d.look, d.up = snap(position, 3), snap(look, 3), snap(up, 3)
        d.cam_to_world, d.world_to_cam = snap(cam_to_world, 16), snap(world_to_cam, 16)
        d.intrinsic_mat_inv, d.intrinsic_mat = snap(intrinsic_mat_inv, 9), snap(intrinsic_mat, 9)
        d.distortion_params = snap(distortion_params, 8)
        d.clip_near = float(clip_near)
        d.camera_type = int(camera_type)
        d.viewport_beg[0], d.viewport_beg[1] = viewport_beg.x, viewport_beg.y
        d.viewport_end[0], d.viewport_end[1] = viewport_end.x, viewport_end.y
        self._desc = d
        self.use_look_at = not bool(d.cam_to_world)
        self._has_distortion = bool(d.distortion_params)

    def has_distortion_params(self):
        return self._has_distortion


class DCamera:                         # src/redner.cpp:52-60
    def __init__(self, position, look, up, cam_to_world, world_to_cam, intrinsic_mat_inv, intrinsic_mat,
                 distortion_params):
        d = _capi.DCameraDesc()
        d.position, d.look, d.up = _addr(position), _addr(look), _addr(up)
        d.cam_to_world, d.world_to_cam = _addr(cam_to_world), _addr(world_to_cam)
        d.intrinsic_mat_inv, d.intrinsic_mat = _addr(intrinsic_mat_inv), _addr(intrinsic_mat)
        d.distortion_params = _addr(distortion_params)
        self._desc = d


class Shape:                           # src/redner.cpp:84-104
    def __init__(self, vertices, indices, uvs, normals, uv_indices, normal_indices, colors,
                 num_vertices, num_uv_vertices, num_normal_vertices, num_triangles, material_id, light_id):
        d = _capi.ShapeDesc()
        d.vertices, d.indices = _addr(vertices), _addr(indices)
        d.uvs, d.normals = _addr(uvs), _addr(normals)
        d.uv_indices, d.normal_indices = _addr(uv_indices), _addr(normal_indices)
        d.colors = _addr(colors)
        d.num_vertices, d.num_uv_vertices = int(num_vertices), int(num_uv_vertices)
        d.num_normal_vertices, d.num_triangles = int(num_normal_vertices), int(num_triangles)
        d.material_id, d.light_id = int(material_id), int(light_id)
        self._desc = d
        self.num_vertices = d.num_vertices
        self.num_uv_vertices = d.num_uv_vertices
        self.num_normal_vertices = d.num_normal_vertices
        self.num_triangles = d.num_triangles
        self.material_id, self.light_id = d.material_id, d.light_id

    def has_uvs(self):
        return bool(self._desc.uvs)

    def has_normals(self):
        return bool(self._desc.normals)

    def has_colors(self):
        return bool(self._desc.colors)


class DShape:                          # src/redner.cpp:106-110
    def __init__(self, vertices, uvs, normals, colors):
        d = _capi.DShapeDesc()
        d.vertices, d.uvs, d.normals, d.colors = _addr(vertices), _addr(uvs), _addr(normals), _addr(colors)
        self._desc = d


class _Texture:                        # src/redner.cpp:112-131, src/texture.h:14-47
    _fixed_channels = None

    def __init__(self, texels, width, height, channels, uv_scale):
        assert len(texels) == len(width) == len(height)
        n = min(len(texels), _capi.MAX_MIP)
        self.texels = [_addr(t) for t in texels[:n]]
        self.width = [int(w) for w in width[:n]]
        self.height = [int(h) for h in height[:n]]
        self.channels = int(channels) if self._fixed_channels is None else self._fixed_channels
        self.num_levels = n
        self.uv_scale = _addr(uv_scale)

    def _to_desc(self):
        d = _capi.TextureDesc()
        for i in range(self.num_levels):
            d.texels[i], d.width[i], d.height[i] = self.texels[i], self.width[i], self.height[i]
        d.channels, d.num_levels, d.uv_scale = self.channels, self.num_levels, self.uv_scale
        return d

    def _to_ddesc(self):
        d = _capi.DTextureDesc()
        for i in range(self.num_levels):
            d.texels[i] = self.texels[i]
        d.num_levels, d.uv_scale = self.num_levels, self.uv_scale
        return d

    def _size(self, i):
        if i < self.num_levels:
            return self.width[i], self.height[i]
        return 0, 0


class Texture1(_Texture):
    _fixed_channels = 1


class Texture3(_Texture):
    _fixed_channels = 3


class TextureN(_Texture):
    _fixed_channels = None


class Material:                        # src/redner.cpp:133-151
    def __init__(self, diffuse_reflectance, specular_reflectance, roughness, generic_texture, normal_map,
                 compute_specular_lighting, two_sided, use_vertex_color):
        self.diffuse_reflectance, self.specular_reflectance = diffuse_reflectance, specular_reflectance
        self.roughness, self.generic_texture, self.normal_map = roughness, generic_texture, normal_map
        self.compute_specular_lighting = bool(compute_specular_lighting)
        self.two_sided, self.use_vertex_color = bool(two_sided), bool(use_vertex_color)

    def _to_desc(self):
        d = _capi.MaterialDesc()
        d.diffuse_reflectance = self.diffuse_reflectance._to_desc()
        d.specular_reflectance = self.specular_reflectance._to_desc()
        d.roughness = self.roughness._to_desc()
        d.generic_texture = self.generic_texture._to_desc()
        d.normal_map = self.normal_map._to_desc()
        d.compute_specular_lighting = int(self.compute_specular_lighting)
        d.two_sided, d.use_vertex_color = int(self.two_sided), int(self.use_vertex_color)
        return d

    def get_diffuse_levels(self):
        return self.diffuse_reflectance.num_levels

    def get_diffuse_size(self, i):
        return self.diffuse_reflectance._size(i)

    def get_specular_levels(self):
        return self.specular_reflectance.num_levels

    def get_specular_size(self, i):
        return self.specular_reflectance._size(i)

    def get_roughness_levels(self):
        return self.roughness.num_levels

    def get_roughness_size(self, i):
        return self.roughness._size(i)

    def get_generic_levels(self):
        return self.generic_texture.num_levels

    def get_generic_size(self, i):
        w, h = self.generic_texture._size(i)
        return self.generic_texture.channels, w, h

    def get_normal_map_levels(self):
        return self.normal_map.num_levels

    def get_normal_map_size(self, i):
        return self.normal_map._size(i)


class DMaterial:                       # src/redner.cpp:153-158
    def __init__(self, diffuse_reflectance, specular_reflectance, roughness, generic_texture, normal_map):
        self._parts = (diffuse_reflectance, specular_reflectance, roughness, generic_texture, normal_map)

    def _to_desc(self):
        d = _capi.DMaterialDesc()
        (d.diffuse_reflectance, d.specular_reflectance, d.roughness, d.generic_texture,
         d.normal_map) = [p._to_ddesc() for p in self._parts]
        return d


class AreaLight:                       # src/redner.cpp:160-164 (intensity: HOST pointer, read now)
    def __init__(self, shape_id, intensity, two_sided, directly_visible):
        d = _capi.AreaLightDesc()
        d.shape_id = int(shape_id)
        vals = _host_floats(_addr(intensity), 3)
        for k in range(3):
            d.intensity[k] = vals[k]
        d.two_sided, d.directly_visible = int(bool(two_sided)), int(bool(directly_visible))
        self._desc = d


class DAreaLight:                      # src/redner.cpp:166-167
    def __init__(self, intensity):
        d = _capi.DAreaLightDesc()
        d.intensity = _addr(intensity)
        self._desc = d


class EnvironmentMap:                  # src/redner.cpp:169-177
    def __init__(self, values, env_to_world, world_to_env, sample_cdf_ys, sample_cdf_xs, pdf_norm,
                 directly_visible):
        self.values = values
        self._keep = []
        d = _capi.EnvmapDesc()
        d.values = values._to_desc()
        for name, p in (('env_to_world', env_to_world), ('world_to_env', world_to_env)):
            arr = (C.c_float * 16)(*_host_floats(_addr(p), 16))
            self._keep.append(arr)
            setattr(d, name, C.cast(arr, C.c_void_p))
        d.sample_cdf_ys, d.sample_cdf_xs = _addr(sample_cdf_ys), _addr(sample_cdf_xs)
        d.pdf_norm, d.directly_visible = float(pdf_norm), int(bool(directly_visible))
        self._desc = d

    def get_levels(self):
        return self.values.num_levels

    def get_size(self, i):
        return self.values._size(i)


class DEnvironmentMap:                 # src/redner.cpp:179-181
    def __init__(self, values, world_to_env):
        d = _capi.DEnvmapDesc()
        d.values = values._to_ddesc()
        d.world_to_env = _addr(world_to_env)
        self._desc = d


class Scene:                           # src/redner.cpp:62-73
    def __init__(self, camera, shapes, materials, area_lights, envmap, use_gpu, gpu_index,
                 use_primary_edge_sampling, use_secondary_edge_sampling):
        lib = _capi.lib()
        self._lib = lib
        self.camera = camera
        sh = (_capi.ShapeDesc * max(len(shapes), 1))(*[s._desc for s in shapes])
        mt = (_capi.MaterialDesc * max(len(materials), 1))(*[m._to_desc() for m in materials])
        al = (_capi.AreaLightDesc * max(len(area_lights), 1))(*[l._desc for l in area_lights])
        env = C.byref(envmap._desc) if envmap is not None else None
        self._refs = (camera, shapes, materials, area_lights, envmap)
        self._handle = _call(lib, 'Scene', 'rdr_scene_create', C.byref(camera._desc), sh, len(shapes), mt, len(materials),
                             al, len(area_lights), env, int(bool(use_gpu)), int(gpu_index),
                             int(bool(use_primary_edge_sampling)), int(bool(use_secondary_edge_sampling)),
                             on=(use_gpu, gpu_index), ok=bool)
        self.max_generic_texture_dimension = lib.rdr_scene_max_generic_texture_dimension(self._handle)
        self.use_gpu, self.gpu_index = bool(use_gpu), int(gpu_index)

    def __del__(self):
        h, self._handle = getattr(self, '_handle', None), None
        if h:
            self._lib.rdr_scene_destroy(h)


class DScene:                          # src/redner.cpp:75-82
    def __init__(self, camera, shapes, materials, area_lights, envmap, use_gpu, gpu_index):
        self._refs = (camera, shapes, materials, area_lights, envmap)
        d = _capi.DSceneDesc()
        d.camera = camera._desc
        self._sh = (_capi.DShapeDesc * max(len(shapes), 1))(*[s._desc for s in shapes])
        self._mt = (_capi.DMaterialDesc * max(len(materials), 1))(*[m._to_desc() for m in materials])
        self._al = (_capi.DAreaLightDesc * max(len(area_lights), 1))(*[l._desc for l in area_lights])
        d.shapes, d.num_shapes = self._sh, len(shapes)
        d.materials, d.num_materials = self._mt, len(materials)
        d.area_lights, d.num_area_lights = self._al, len(area_lights)
        d.envmap = C.pointer(envmap._desc) if envmap is not None else None
        self._desc = d


class RenderOptions:                   # src/redner.cpp:207-216 (+ sample_offset/total_samples extension)
    def __init__(self, seed, num_samples, max_bounces, channels, sampler_type, sample_pixel_center):
        self.seed = int(seed)
        self.num_samples = int(num_samples)
        self.max_bounces = int(max_bounces)
        self.channels = [int(c) for c in channels]
        self.sampler_type = int(sampler_type)
        self.sample_pixel_center = bool(sample_pixel_center)
        self.sample_offset = 0
        self.total_samples = 0
        # rdr_tuning (redner_amd extension; every field 0 = the library's default): e.g. options.tuning.batch_samples = 1
        self.tuning = _capi.Tuning()

    def _to_desc(self):
        d = _capi.RenderOptionsDesc()
        self._ch = (C.c_int * max(len(self.channels), 1))(*self.channels)
        d.seed, d.num_samples, d.max_bounces = self.seed & 0xFFFFFFFFFFFFFFFF, self.num_samples, self.max_bounces
        d.channels, d.num_channels = self._ch, len(self.channels)
        d.sampler_type, d.sample_pixel_center = self.sampler_type, int(self.sample_pixel_center)
        d.sample_offset, d.total_samples = int(self.sample_offset), int(self.total_samples)
        d.tuning = C.pointer(self.tuning)
        return d


def compute_num_channels(channel_list, max_generic_texture_dimension):    # src/redner.cpp:201
    ch = (C.c_int * max(len(channel_list), 1))(*[int(c) for c in channel_list])
    n = _capi.lib().rdr_compute_num_channels(ch, len(channel_list), int(max_generic_texture_dimension))
    if n < 0:
        raise RuntimeError('redner.compute_num_channels: unknown channel')
    return n


def render(scene, options, rendered_image, d_rendered_image, d_scene, screen_gradient_image, debug_image):
    """redner.render(...)  src/redner.cpp:257 -- forward iff rendered_image != 0, backward iff
    d_rendered_image != 0."""
    od = options._to_desc()
    ds = C.byref(d_scene._desc) if d_scene is not None else None
    _call(scene._lib, 'render', 'rdr_render', scene._handle, C.byref(od), _addr(rendered_image), _addr(d_rendered_image), ds,
          _addr(screen_gradient_image), _addr(debug_image), on=(scene.use_gpu, scene.gpu_index))


class DeferredLightType(enum.IntEnum):     # rdr_deferred_light_type (not in the reference's module: its deferred lights are torch code)
    ambient = _capi.DL_AMBIENT
    point = _capi.DL_POINT
    directional = _capi.DL_DIRECTIONAL
    spot = _capi.DL_SPOT
    sh_r = _capi.DL_SH_R               # one colour channel of a spherical-harmonic environment light (an SHLight is three rows)
    sh_g = _capi.DL_SH_G
    sh_b = _capi.DL_SH_B


def _scene_handles(scenes, num_images, what):
    """one Scene (or None) per image -> the table of handles, which lives as long as the call"""
    scenes = list(scenes)
    if len(scenes) != num_images:
        raise RuntimeError('redner.deferred_shade: %d %s scenes for %d images' % (len(scenes), what, num_images))
    lib = _capi.lib()
    for sc in scenes:
        if sc is not None and (not isinstance(sc, Scene) or sc._handle is None or sc._lib is not lib):
            raise RuntimeError('redner.deferred_shade: an %s must be a live Scene of the loaded library, or None' % what)
    return (C.c_void_p * max(len(scenes), 1))(*[None if sc is None else sc._handle for sc in scenes]), scenes


def _deferred_desc(num_images, height, width, aa_samples, alpha, light_types, image_light_ranges, use_gpu, gpu_index,
                   occluders=None, visibility=None, ao_occluders=None, ao_words=None, ao_rays=0, ao_radius=float('inf')):
    d = _capi.DeferredDesc()
    d.num_images, d.height, d.width = int(num_images), int(height), int(width)
    d.aa_samples, d.alpha, d.num_lights = int(aa_samples), int(bool(alpha)), len(light_types)
    types = (C.c_int32 * max(len(light_types), 1))(*[int(t) for t in light_types])
    flat = [int(v) for r in image_light_ranges for v in r]
    if len(flat) != 2 * d.num_images:
        raise RuntimeError('redner.deferred_shade: %d light ranges for %d images' % (len(image_light_ranges), d.num_images))
    ranges = (C.c_int32 * max(len(flat), 1))(*flat)
    d.light_type, d.image_light_range = types, ranges
    d.gpu_index = _gpu_index(use_gpu, gpu_index)
    handles = ao_handles = None
    if occluders is not None:              # one Scene (or None: not shadowed) per image
        handles, occluders = _scene_handles(occluders, d.num_images, 'occluder')
        d.occluders = handles
    if visibility is not None:
        d.visibility = _ptr(visibility)
    if ao_occluders is not None:           # ... (or None: not occluded)
        ao_handles, ao_occluders = _scene_handles(ao_occluders, d.num_images, 'ao occluder')
        d.ao_occluders = ao_handles
    if ao_words is not None:
        d.ao_words = _ptr(ao_words)
    d.ao_rays, d.ao_radius = int(ao_rays), float(ao_radius)
    return d, (types, ranges, handles, occluders, ao_handles, ao_occluders)


def deferred_shade(g_buffer, light_params, image, num_images, height, width, aa_samples, alpha, light_types,
                   image_light_ranges, use_gpu, gpu_index, occluders=None, visibility=None, ao_occluders=None, ao_words=None,
                   ao_rays=0, ao_radius=float('inf')):
    """Not in the reference: rdr_deferred_shade (include/redner_amd.h).  g_buffer [N, H * aa, W * aa, 9 + alpha],
    light_params [L, 10], image [N, H, W, 3 + alpha]: float_ptr; light_types: L DeferredLightType; image_light_ranges: N
    (begin, end) pairs into the table.  Shadows: `occluders`, N Scenes (None: that image is not shadowed), and `visibility`,
    int_ptr to [N, H * aa, W * aa] 32-bit words, every one of which is written (bit b: light begin + b reaches the texel).
    Ambient occlusion of the ambient and SH rows: `ao_occluders`, N Scenes (None: that image is not occluded), `ao_words`, int_ptr
    to words of the same shape, every one written (bit r: hemisphere ray r of the texel escaped), `ao_rays` 1 .. 32 per texel
    and `ao_radius` > 0, where they end."""
    d, _keep = _deferred_desc(num_images, height, width, aa_samples, alpha, light_types, image_light_ranges, use_gpu, gpu_index,
                              occluders, visibility, ao_occluders, ao_words, ao_rays, ao_radius)
    _call(_capi.lib(), 'deferred_shade', 'rdr_deferred_shade', C.byref(d), _ptr(g_buffer), _ptr(light_params), _ptr(image),
          on=(use_gpu, gpu_index))


def deferred_shade_backward(g_buffer, light_params, d_image, d_g_buffer, d_light_params, num_images, height, width,
                            aa_samples, alpha, light_types, image_light_ranges, use_gpu, gpu_index, occluders=None,
                            visibility=None, ao_occluders=None, ao_words=None, ao_rays=0, ao_radius=float('inf')):
    """Not in the reference: rdr_deferred_shade_backward; writes every element of d_g_buffer and d_light_params.  `visibility`:
    the words the forward call wrote, held constant (no scene is needed); `ao_words` with `ao_rays` likewise."""
    d, _keep = _deferred_desc(num_images, height, width, aa_samples, alpha, light_types, image_light_ranges, use_gpu, gpu_index,
                              occluders, visibility, ao_occluders, ao_words, ao_rays, ao_radius)
    _call(_capi.lib(), 'deferred_shade_backward', 'rdr_deferred_shade_backward', C.byref(d), _ptr(g_buffer), _ptr(light_params),
          _ptr(d_image), _ptr(d_g_buffer), _ptr(d_light_params), on=(use_gpu, gpu_index))


def deferred_specular(g_buffer, material, eye, light_params, image, num_images, height, width, aa_samples, alpha, light_types,
                      image_light_ranges, use_gpu, gpu_index, visibility=None):
    """Not in the reference: rdr_deferred_specular (csrc/deferred_specular_abi.h).  g_buffer [N, H * aa, W * aa, 9 + alpha],
    material [N, H * aa, W * aa, 4] (ks rgb, roughness), eye [N, 3], light_params [L, 10], image [N, H, W, 3]: float_ptr; the
    table as for deferred_shade.  `visibility`: int_ptr to the words deferred_shade wrote, read only."""
    d, _keep = _deferred_desc(num_images, height, width, aa_samples, alpha, light_types, image_light_ranges, use_gpu, gpu_index,
                              visibility=visibility)
    _call(_capi.lib(), 'deferred_specular', 'rdr_deferred_specular', C.byref(d), _ptr(g_buffer), _ptr(material), _ptr(eye),
          _ptr(light_params), _ptr(image), on=(use_gpu, gpu_index))


def deferred_specular_backward(g_buffer, material, eye, light_params, d_image, d_g_buffer, d_material, d_eye, d_light_params,
                               num_images, height, width, aa_samples, alpha, light_types, image_light_ranges, use_gpu, gpu_index,
                               visibility=None):
    """Not in the reference: rdr_deferred_specular_backward; writes every element of d_g_buffer, d_material, d_eye and
    d_light_params.  `visibility`: the words of the forward call, held constant."""
    d, _keep = _deferred_desc(num_images, height, width, aa_samples, alpha, light_types, image_light_ranges, use_gpu, gpu_index,
                              visibility=visibility)
    _call(_capi.lib(), 'deferred_specular_backward', 'rdr_deferred_specular_backward', C.byref(d), _ptr(g_buffer), _ptr(material),
          _ptr(eye), _ptr(light_params), _ptr(d_image), _ptr(d_g_buffer), _ptr(d_material), _ptr(d_eye), _ptr(d_light_params),
          on=(use_gpu, gpu_index))


def deferred_quad(g_buffer, quads, image, num_images, height, width, aa_samples, alpha, two_sided, image_quad_ranges, use_gpu,
                  gpu_index):
    """Not in the reference: rdr_deferred_quad (csrc/deferred_quad_abi.h).  g_buffer [N, H * aa, W * aa, 9 + alpha], quads [Q, 16]
    (corners q0..q3, radiance, one unused float), image [N, H, W, 3]: float_ptr; two_sided: Q flags (0 one-sided, 1 two-sided);
    image_quad_ranges: N (begin, end) pairs into the rows of `quads`."""
    d, _keep = _deferred_desc(num_images, height, width, aa_samples, alpha, two_sided, image_quad_ranges, use_gpu, gpu_index)
    _call(_capi.lib(), 'deferred_quad', 'rdr_deferred_quad', C.byref(d), _ptr(g_buffer), _ptr(quads), _ptr(image),
          on=(use_gpu, gpu_index))


def deferred_quad_backward(g_buffer, quads, d_image, d_g_buffer, d_quads, num_images, height, width, aa_samples, alpha, two_sided,
                           image_quad_ranges, use_gpu, gpu_index):
    """Not in the reference: rdr_deferred_quad_backward; writes every element of d_g_buffer and d_quads."""
    d, _keep = _deferred_desc(num_images, height, width, aa_samples, alpha, two_sided, image_quad_ranges, use_gpu, gpu_index)
    _call(_capi.lib(), 'deferred_quad_backward', 'rdr_deferred_quad_backward', C.byref(d), _ptr(g_buffer), _ptr(quads),
          _ptr(d_image), _ptr(d_g_buffer), _ptr(d_quads), on=(use_gpu, gpu_index))


def deferred_quad_shadowed(g_buffer, quads, factors, image, num_images, height, width, aa_samples, alpha, two_sided,
                           image_quad_ranges, use_gpu, gpu_index, occluders, visibility, shadow_rays):
    """Not in the reference: rdr_deferred_quad_shadowed (csrc/deferred_quad_shadow_abi.h): deferred_quad with every (quad, texel)
    term scaled by a visibility factor from `shadow_rays` (1 .. 32) any-hit rays over `occluders`, N Scenes (None: that image
    is not shadowed).  `visibility`: int_ptr to [pairs, H * aa, W * aa] 32-bit words, `factors`: float_ptr to as many floats;
    every one of both is written (pairs: the sum of the images' range lengths)."""
    d, _keep = _deferred_desc(num_images, height, width, aa_samples, alpha, two_sided, image_quad_ranges, use_gpu, gpu_index,
                              occluders=occluders, visibility=visibility)
    _call(_capi.lib(), 'deferred_quad_shadowed', 'rdr_deferred_quad_shadowed', C.byref(d), _ptr(g_buffer), _ptr(quads),
          int(shadow_rays), _ptr(factors), _ptr(image), on=(use_gpu, gpu_index))


def deferred_quad_shadowed_backward(g_buffer, quads, factors, d_image, d_g_buffer, d_quads, num_images, height, width, aa_samples,
                                    alpha, two_sided, image_quad_ranges, use_gpu, gpu_index):
    """Not in the reference: rdr_deferred_quad_shadowed_backward; writes every element of d_g_buffer and d_quads.  `factors`:
    what the forward call wrote, held constant (no scene is needed)."""
    d, _keep = _deferred_desc(num_images, height, width, aa_samples, alpha, two_sided, image_quad_ranges, use_gpu, gpu_index)
    _call(_capi.lib(), 'deferred_quad_shadowed_backward', 'rdr_deferred_quad_shadowed_backward', C.byref(d), _ptr(g_buffer),
          _ptr(quads), _ptr(factors), _ptr(d_image), _ptr(d_g_buffer), _ptr(d_quads), on=(use_gpu, gpu_index))


def mip_num_levels(height, width):
    """Not in the reference's module: rdr_mip_num_levels, min(ceil(log2(max(height, width))) + 1, 8)."""
    return int(_capi.lib().rdr_mip_num_levels(int(height), int(width)))


def mip_backward_scratch(height, width, channels):
    """Not in the reference's module: floats of scratch mip_pyramid_backward needs for an image of this size."""
    return int(_call(_capi.lib(), 'mip_backward_scratch', 'rdr_mip_backward_scratch', int(height), int(width), int(channels),
                     ok=_not_negative))


def mip_tiled_stages(height, width, channels):
    """Not in the reference's module: how many tiled launches (three levels each) mip_pyramid and mip_pyramid_backward make for an
    image of this size before one workgroup does the rest (csrc/mipmap.h: tiled_stages); 0 = one workgroup does everything."""
    return int(_call(_capi.lib(), 'mip_tiled_stages', 'rdr_mip_tiled_stages', int(height), int(width), int(channels),
                     ok=_not_negative))


def _level_table(levels):
    return (C.c_void_p * max(len(levels), 1))(*[_ptr(l) for l in levels])


def mip_pyramid(levels, height, width, channels, use_gpu, gpu_index):
    """Not in the reference's module (its pyramid is torch code, pyredner/texture.py): rdr_mip_pyramid (include/redner_amd.h).
    levels: float_ptr of every level, [0] the image [height, width, channels]; levels 1.. are written.  Ordered on the
    current torch stream, not synchronised."""
    _call(_capi.lib(), 'mip_pyramid', 'rdr_mip_pyramid', int(height), int(width), int(channels), len(levels), _level_table(levels),
          _gpu_index(use_gpu, gpu_index), on=(use_gpu, gpu_index))


def mip_pyramid_backward(d_levels, d_texels, scratch, scratch_floats, height, width, channels, use_gpu, gpu_index):
    """Not in the reference's module: rdr_mip_pyramid_backward.  d_levels: float_ptr per level, float_ptr(0) = zeros; writes every
    element of d_texels."""
    _call(_capi.lib(), 'mip_pyramid_backward', 'rdr_mip_pyramid_backward', int(height), int(width), int(channels), len(d_levels),
          _level_table(d_levels), _ptr(d_texels), _ptr(scratch), int(scratch_floats), _gpu_index(use_gpu, gpu_index),
          on=(use_gpu, gpu_index))


def sh_backward_scratch(height, width, channels, num_coeffs):
    """Not in the reference's module: floats of scratch sh_reconstruct_backward needs (rdr_sh_backward_scratch)."""
    return int(_call(_capi.lib(), 'sh_backward_scratch', 'rdr_sh_backward_scratch', int(height), int(width), int(channels),
                     int(num_coeffs), ok=_not_negative))


def sh_reconstruct(coeffs, image, clamp, channels, num_coeffs, height, width, use_gpu, gpu_index):
    """Not in the reference's module (its SH_reconstruct is torch code, pyredner/utils.py): rdr_sh_reconstruct
    (include/redner_amd.h).  coeffs: float_ptr of [channels, num_coeffs]; writes image [height, width, channels] and, unless it
    is None, the clamp bytes.  Ordered on the current torch stream, not synchronised."""
    _call(_capi.lib(), 'sh_reconstruct', 'rdr_sh_reconstruct', _ptr(coeffs), int(channels), int(num_coeffs), int(height),
          int(width), _ptr(image), _ptr(clamp), _gpu_index(use_gpu, gpu_index), on=(use_gpu, gpu_index))


def sh_reconstruct_backward(clamp, d_image, d_coeffs, scratch, scratch_floats, channels, num_coeffs, height, width, use_gpu,
                            gpu_index):
    """Not in the reference's module: rdr_sh_reconstruct_backward.  Writes every element of d_coeffs [channels, num_coeffs]."""
    _call(_capi.lib(), 'sh_reconstruct_backward', 'rdr_sh_reconstruct_backward', _ptr(clamp), _ptr(d_image),
          int(channels), int(num_coeffs), int(height), int(width), _ptr(d_coeffs), _ptr(scratch),
          int(scratch_floats), _gpu_index(use_gpu, gpu_index), on=(use_gpu, gpu_index))


def pyramid_loss_scratch(batch, height, width, channels, num_levels):
    """Not in the reference's module: (forward_floats, backward_floats), the scratch pyramid_loss and pyramid_loss_backward need
    (rdr_pyramid_loss_scratch, include/redner_amd_image.h)."""
    return _outputs(C.c_int64, 2, _capi.lib(), 'pyramid_loss_scratch', 'rdr_pyramid_loss_scratch', int(batch), int(height), int(width),
                    int(channels), int(num_levels))


def pyramid_loss_plan(batch, height, width, channels, num_levels):
    """Not in the reference's module: (tiled_levels, small_floats) of rdr_pyramid_loss_plan: how many leading levels the tiled
    kernels do, and the floats per image at or below which a level is left to the one workgroup per image (csrc/pyramid_loss.h)."""
    return _outputs(C.c_int, 2, _capi.lib(), 'pyramid_loss_plan', 'rdr_pyramid_loss_plan', int(batch), int(height), int(width),
                    int(channels), int(num_levels))


def _weight_table(weights, num_levels):
    return None if weights is None else (C.c_float * max(int(num_levels), 1))(*[float(w) for w in weights])


def pyramid_loss(image, target, loss, terms, scratch, scratch_floats, batch, height, width, channels, num_levels, weights, clamp,
                 use_gpu, gpu_index):
    """Not in the reference's module (its scripts write the loss in torch): rdr_pyramid_loss.  image, target, loss, scratch:
    float_ptr; terms: the address of num_levels doubles or None; weights: num_levels numbers or None; clamp: 0 = none.  Ordered
    on the current torch stream, not synchronised."""
    _call(_capi.lib(), 'pyramid_loss', 'rdr_pyramid_loss', _ptr(image), _ptr(target), int(batch), int(height),
          int(width), int(channels), int(num_levels), _weight_table(weights, num_levels), float(clamp), _ptr(loss),
          _ptr(terms), _ptr(scratch), int(scratch_floats), _gpu_index(use_gpu, gpu_index), on=(use_gpu, gpu_index))


def pyramid_loss_backward(image, target, saved, saved_floats, upstream, d_image, d_target, scratch, scratch_floats, batch, height,
                          width, channels, num_levels, weights, clamp, use_gpu, gpu_index):
    """Not in the reference's module: rdr_pyramid_loss_backward.  Writes every element of d_image and, unless None, d_target."""
    _call(_capi.lib(), 'pyramid_loss_backward', 'rdr_pyramid_loss_backward', _ptr(image), _ptr(target), int(batch),
          int(height), int(width), int(channels), int(num_levels), _weight_table(weights, num_levels), float(clamp),
          _ptr(saved), int(saved_floats), _ptr(upstream), _ptr(d_image), _ptr(d_target),
          _ptr(scratch), int(scratch_floats), _gpu_index(use_gpu, gpu_index), on=(use_gpu, gpu_index))


def _count_table(counts):
    return (C.c_int32 * max(len(counts), 1))(*[int(n) for n in counts])


def _pointer_table(pointers, count):
    """A host table of `count` addresses (float_ptr, int or None = NULL), or NULL when `pointers` is None."""
    if pointers is None:
        return None
    pointers = list(pointers)
    if len(pointers) != count:
        raise RuntimeError('redner: a table of %d pointers for %d vertex sets' % (len(pointers), count))
    return (C.c_void_p * max(count, 1))(*[_ptr(p) for p in pointers])


def pose_scratch(counts):
    """Not in the reference's module: (forward_floats, backward_floats), the scratch pose_vertices (without a given centre) and
    pose_vertices_backward need for vertex sets of these sizes (rdr_pose_scratch, include/redner_amd_pose.h)."""
    return _outputs(C.c_int64, 2, _capi.lib(), 'pose_scratch', 'rdr_pose_scratch', len(counts), _count_table(counts))


def pose_plan(counts):
    """Not in the reference's module: (chunk_vertices, max_workgroups, workgroups) of rdr_pose_plan: the vertices of a chunk, the
    most workgroups a launch has, and how many it has for sets of these sizes (csrc/pose.h)."""
    return _outputs(C.c_int, 3, _capi.lib(), 'pose_plan', 'rdr_pose_plan', len(counts), _count_table(counts))


def rotate_matrix(angles, matrix, use_gpu, gpu_index):
    """Not in the reference's module (its gen_rotate_matrix is torch code, pyredner/transform.py): rdr_rotate_matrix.  float_ptr
    arguments; writes matrix [3, 3].  Ordered on the current torch stream, not synchronised."""
    _call(_capi.lib(), 'rotate_matrix', 'rdr_rotate_matrix', _ptr(angles), _ptr(matrix), _gpu_index(use_gpu, gpu_index),
          on=(use_gpu, gpu_index))


def rotate_matrix_backward(angles, d_matrix, d_angles, use_gpu, gpu_index):
    """Not in the reference's module: rdr_rotate_matrix_backward.  Writes d_angles [3]."""
    _call(_capi.lib(), 'rotate_matrix_backward', 'rdr_rotate_matrix_backward', _ptr(angles), _ptr(d_matrix),
          _ptr(d_angles), _gpu_index(use_gpu, gpu_index), on=(use_gpu, gpu_index))


def pose_vertices(vertices, counts, angles, translation, center, out, saved, scratch, scratch_floats, use_gpu, gpu_index):
    """Not in the reference's module (its scripts write the pose in torch): rdr_pose_vertices.  vertices, out: one float_ptr per
    set; counts: the sets' sizes; center: float_ptr or None = the sets' own mean; writes every out and saved [12].  Ordered on
    the current torch stream, not synchronised."""
    k = len(counts)
    _call(_capi.lib(), 'pose_vertices', 'rdr_pose_vertices', k, _pointer_table(vertices, k), _count_table(counts), _ptr(angles),
          _ptr(translation), _ptr(center), _pointer_table(out, k), _ptr(saved), _ptr(scratch),
          int(scratch_floats), _gpu_index(use_gpu, gpu_index), on=(use_gpu, gpu_index))


def pose_vertices_backward(vertices, counts, angles, saved, own_center, d_out, d_vertices, d_angles, d_translation, d_center, scratch,
                           scratch_floats, use_gpu, gpu_index):
    """Not in the reference's module: rdr_pose_vertices_backward.  d_out: per set a float_ptr or None = zeros; d_vertices: None, or
    per set a float_ptr or None = not wanted; writes d_angles, d_translation, d_center (a given centre) and the d_vertices."""
    k = len(counts)
    _call(_capi.lib(), 'pose_vertices_backward', 'rdr_pose_vertices_backward', k, _pointer_table(vertices, k), _count_table(counts),
          _ptr(angles), _ptr(saved), int(bool(own_center)), _pointer_table(d_out, k), _pointer_table(d_vertices, k),
          _ptr(d_angles), _ptr(d_translation), _ptr(d_center), _ptr(scratch), int(scratch_floats),
          _gpu_index(use_gpu, gpu_index), on=(use_gpu, gpu_index))


def envmap_tables(texels, y_weight, sample_cdf_ys, sample_cdf_xs, height, width, use_gpu, gpu_index):
    """Not in the reference's module (its tables are torch code, pyredner/envmap.py): rdr_envmap_tables.  float_ptr arguments;
    writes both tables and returns the last unnormalised entry of the column table (one synchronisation)."""
    total = C.c_float(0.0)
    _call(_capi.lib(), 'envmap_tables', 'rdr_envmap_tables', _ptr(texels), _ptr(y_weight), int(height), int(width),
          _ptr(sample_cdf_ys), _ptr(sample_cdf_xs), C.byref(total), _gpu_index(use_gpu, gpu_index),
          on=(use_gpu, gpu_index))
    return float(total.value)


class NormalWeighting(enum.IntEnum):
    """Not in the reference's module: rdr_normal_weighting, the weighting_scheme strings of pyredner.compute_vertex_normal."""
    max = 0
    cotangent = 1


class mesh_topology:
    """Not in the reference's module: the native plan of one connectivity (rdr_mesh_topology_create, csrc/vertex_normal.h): the
    corners incident to every vertex in ascending corner id.  indices: int_ptr of [num_triangles, 3] int32 in the memory the
    later calls' tensors live in.  Belongs to the library that was loaded when it was made and is destroyed with it on
    collection (or by destroy())."""

    def __init__(self, indices, num_triangles, num_vertices, use_gpu, gpu_index):
        self.lib, self.handle = _capi.lib(), None
        self.num_triangles, self.num_vertices = int(num_triangles), int(num_vertices)
        self.use_gpu, self.gpu_index = bool(use_gpu), int(gpu_index)
        self.handle = _call(self.lib, 'mesh_topology', 'rdr_mesh_topology_create', _ptr(indices), self.num_triangles,
                            self.num_vertices, int(self.use_gpu), self.gpu_index, on=(use_gpu, gpu_index), ok=bool)

    def destroy(self):
        if self.handle:
            self.lib.rdr_mesh_topology_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    def read(self):
        """(offsets [V + 1], corners [3 T]) as lists: the rows of the plan (tests)."""
        offsets, corners = (C.c_int * (self.num_vertices + 1))(), (C.c_int * max(3 * self.num_triangles, 1))()
        _call(self.lib, 'mesh_topology.read', 'rdr_mesh_topology_read', self.handle, offsets, corners)
        return list(offsets), list(corners)[:3 * self.num_triangles]

    def scratch(self, scheme):
        """floats of (forward scratch, backward scratch, saved) for a weighting scheme (rdr_vertex_normal_scratch)."""
        return _outputs(C.c_int64, 3, self.lib, 'mesh_topology.scratch', 'rdr_vertex_normal_scratch', self.handle, int(scheme))


def vertex_normal(topology, scheme, vertices, normals, saved, scratch, scratch_floats):
    """Not in the reference's module (its compute_vertex_normal is torch code, pyredner/shape.py): rdr_vertex_normal.  float_ptr
    arguments; writes normals [V, 3] and saved.  Ordered on the current torch stream, not synchronised."""
    _call(topology.lib, 'vertex_normal', 'rdr_vertex_normal', topology.handle, int(scheme), _ptr(vertices), _ptr(normals),
          _ptr(saved), _ptr(scratch), int(scratch_floats), on=(topology.use_gpu, topology.gpu_index))


def vertex_normal_backward(topology, scheme, vertices, saved, d_normals, d_vertices, scratch, scratch_floats):
    """Not in the reference's module: rdr_vertex_normal_backward.  Writes every element of d_vertices [V, 3]."""
    _call(topology.lib, 'vertex_normal_backward', 'rdr_vertex_normal_backward', topology.handle, int(scheme), _ptr(vertices),
          _ptr(saved), _ptr(d_normals), _ptr(d_vertices), _ptr(scratch), int(scratch_floats),
          on=(topology.use_gpu, topology.gpu_index))


class SmoothWeighting(enum.IntEnum):
    """Not in the reference's module: rdr_smooth_weighting, the weighting_scheme strings of pyredner.smooth."""
    reciprocal = 0
    uniform = 1
    cotangent = 2


def mesh_smooth_scratch(topology, scheme):
    """Not in the reference's module: floats of (forward scratch, backward scratch, saved) of a smoothing scheme
    (rdr_mesh_smooth_scratch); mesh_smooth needs the forward scratch."""
    return _outputs(C.c_int64, 3, topology.lib, 'mesh_smooth_scratch', 'rdr_mesh_smooth_scratch', topology.handle, int(scheme))


def mesh_boundary(topology, bound):
    """Not in the reference's module (its bound_vertices is torch code, pyredner/shape.py): rdr_mesh_boundary.  Writes bound [V]."""
    _call(topology.lib, 'mesh_boundary', 'rdr_mesh_boundary', topology.handle, _ptr(bound), on=(topology.use_gpu, topology.gpu_index))


def mesh_laplacian(topology, scheme, vertices, control, shift, saved, scratch, scratch_floats):
    """Not in the reference's module (its smooth is torch code, pyredner/shape.py): rdr_mesh_laplacian.  float_ptr arguments;
    control: float_ptr(0) = all 1; writes shift [V, 3] and saved.  Ordered on the current torch stream, not synchronised."""
    _call(topology.lib, 'mesh_laplacian', 'rdr_mesh_laplacian', topology.handle, int(scheme), _ptr(vertices), _ptr(control),
          _ptr(shift), _ptr(saved), _ptr(scratch), int(scratch_floats), on=(topology.use_gpu, topology.gpu_index))


def mesh_laplacian_backward(topology, scheme, vertices, control, saved, d_shift, d_vertices, scratch, scratch_floats):
    """Not in the reference's module: rdr_mesh_laplacian_backward.  Writes every element of d_vertices [V, 3]."""
    _call(topology.lib, 'mesh_laplacian_backward', 'rdr_mesh_laplacian_backward', topology.handle, int(scheme), _ptr(vertices),
          _ptr(control), _ptr(saved), _ptr(d_shift), _ptr(d_vertices), _ptr(scratch), int(scratch_floats),
          on=(topology.use_gpu, topology.gpu_index))


def mesh_smooth(topology, scheme, vertices_in, control, lmd, iterations, vertices_out, scratch, scratch_floats):
    """Not in the reference's module: rdr_mesh_smooth, `iterations` steps vertices + shift * lmd (lmd rounded to fp32).  Writes
    every element of vertices_out [V, 3], which may be vertices_in."""
    _call(topology.lib, 'mesh_smooth', 'rdr_mesh_smooth', topology.handle, int(scheme), _ptr(vertices_in), _ptr(control),
          float(lmd), int(iterations), _ptr(vertices_out), _ptr(scratch), int(scratch_floats),
          on=(topology.use_gpu, topology.gpu_index))


def _gpu_index(use_gpu, gpu_index):
    """The gpu_index argument of the C ABI: negative = host memory (the CPU debugging harness only)."""
    return int(gpu_index) if use_gpu else -1


def _not_negative(n):
    return n >= 0


def _outputs(ctype, n, lib, what, name, *args):
    """_call with n trailing outputs of `ctype` by reference (the scratch and plan queries) -> their values, a tuple of ints"""
    out = [ctype(0) for _ in range(n)]
    _call(lib, what, name, *args, *[C.byref(o) for o in out])
    return tuple(int(o.value) for o in out)


def _call(lib, what, name, *args, on=None, ok=lambda rc: rc == 0):
    """One checked call of the C ABI on `lib`: ordered on the current torch stream of on = (use_gpu, gpu_index) if given;
    a result that is not `ok` raises with the text of THAT library (another one may have been loaded since the handle was made)."""
    if on is not None:
        _use_torch_stream(lib, *on)
    result = getattr(lib, name)(*args)
    if not ok(result):
        raise RuntimeError('redner.%s: %s' % (what, lib.rdr_last_error().decode('utf-8', 'replace')))
    return result


def _use_torch_stream(lib, use_gpu, gpu_index=None):
    """The library orders its launches on the calling thread's CURRENT torch stream OF THE SCENE'S DEVICE (rdr_set_stream):
    tensors produced under `with torch.cuda.stream(s):` are read after their producers without a device-wide
    synchronisation.  (The reference's kernels run on the null stream, which torch's default stream is.)"""
    if not use_gpu:
        return
    torch = sys.modules.get('torch')
    stream = 0
    if torch is not None and torch.cuda.is_available():
        # a Scene may live on another device than torch's current one (pyredner.set_device without torch.cuda.set_device):
        # a stream handle is only valid on the device it was created on
        stream = int(torch.cuda.current_stream(gpu_index).cuda_stream)
    lib.rdr_set_stream(stream or None)


def set_pool_cap_mb(megabytes):
    """Not in the reference: bound of the library's buffer cache per device (default min(a quarter of the device, 8 GiB)).
    A dedicated render process may raise it (e.g. 65536) so that the buffers of a 2^24-lane sample batch stay parked
    between calls; negative = back to the default."""
    _capi.lib().rdr_set_pool_cap_mb(int(megabytes))


def get_pool_cap_mb():
    """Not in the reference: the bound of the buffer cache in effect (MiB)."""
    return int(_capi.lib().rdr_get_pool_cap_mb())


def set_build_flags(flags):
    """Not in the reference: rdr_build_flags (_capi.BUILD_*) for the Scenes created from now on (debugging / tests)."""
    _capi.lib().rdr_set_build_flags(int(flags))


def trim_cache():
    """Not in the reference: return the device buffers parked by the caching allocator to the driver (rdr_trim_cache) --
    for processes that share the GPU with torch's allocator and change resolution.  Returns the bytes released."""
    return int(_capi.lib().rdr_trim_cache())


# ---- Mitsuba .serialized meshes (src/redner.cpp:232-238, src/load_serialized.cpp:124-288) -----------------------------
class MitsubaTriMesh:
    """vertices [V,3] f32, indices [T,3] i32, uvs [V,2] f32 or [0], normals [V,3] f32 or [0] (numpy)."""

    def __init__(self, vertices, indices, uvs, normals):
        self.vertices, self.indices, self.uvs, self.normals = vertices, indices, uvs, normals


def load_serialized(filename, idx):
    """Sub-mesh `idx` of a Mitsuba 0.5 serialized file: u16 magic, u16 version (3 / 4), a zlib stream per mesh, and
    at the end of the file the offset table (u64 entries for v4, u32 for v3) followed by the mesh count (u32)."""
    import numpy as np
    E_NORMALS, E_TEXCOORDS, E_COLORS, E_DOUBLE = 0x0001, 0x0002, 0x0008, 0x2000
    with open(filename, 'rb') as f:
        data = f.read()
    if len(data) < 8:
        raise RuntimeError('load_serialized: %s is not a serialized mesh file' % filename)
    version = struct.unpack_from('<H', data, 2)[0]
    start = 4
    if idx > 0:
        count = struct.unpack_from('<I', data, len(data) - 4)[0]
        if idx >= count:
            raise RuntimeError('load_serialized: shape index %d out of range (%d meshes)' % (idx, count))
        if version == 4:
            off = struct.unpack_from('<Q', data, len(data) - 4 - 8 * (count - idx))[0]
        else:
            off = struct.unpack_from('<I', data, len(data) - 4 * (count - idx + 1))[0]
        start = off + 4                                   # skip that mesh's own magic + version
    try:
        raw = zlib.decompressobj().decompress(data[start:])
    except zlib.error as e:
        raise RuntimeError('load_serialized: inflate(): %s' % e)
    pos = 0
    flags = struct.unpack_from('<I', raw, pos)[0]
    pos += 4
    if version == 4:
        pos = raw.index(b'\0', pos) + 1                   # null-terminated mesh name
    n_vert, n_tri = struct.unpack_from('<QQ', raw, pos)
    pos += 16
    real = np.dtype('<f8') if flags & E_DOUBLE else np.dtype('<f4')

    def block(count, width, dtype):
        nonlocal pos
        a = np.frombuffer(raw, dtype=dtype, count=count * width, offset=pos).reshape(count, width)
        pos += a.nbytes
        return a

    vertices = block(n_vert, 3, real).astype(np.float32)
    normals = block(n_vert, 3, real).astype(np.float32) if flags & E_NORMALS else np.zeros((0,), np.float32)
    uvs = block(n_vert, 2, real).astype(np.float32) if flags & E_TEXCOORDS else np.zeros((0,), np.float32)
    if flags & E_COLORS:
        block(n_vert, 3, real)                             # read and dropped, like the reference
    indices = block(n_tri, 3, np.dtype('<i4')).astype(np.int32)
    return MitsubaTriMesh(np.ascontiguousarray(vertices), np.ascontiguousarray(indices), uvs, normals)


def _host_mesh_tool(name):
    def stub(*_a, **_k):
        raise NotImplementedError('redner.%s is host-side mesh processing outside the renderer hot path '
                                  '(SURVEY.md section 2.1); use the reference build for it' % name)
    stub.__name__ = name
    return stub


automatic_uv_map = _host_mesh_tool('automatic_uv_map')
copy_texture_atlas = _host_mesh_tool('copy_texture_atlas')
rebuild_topology = _host_mesh_tool('rebuild_topology')
