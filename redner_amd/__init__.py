"""redner_amd -- MI355X-native implementation of redner's differentiable path tracer hot path.

    redner_amd.redner            the `redner` module surface (ctypes over the C ABI)
    redner_amd.render_pytorch    RenderFunction (torch.autograd.Function) + minimal scene classes
    redner_amd.render_utils      render_deferred + the deferred lights, render_g_buffer / render_albedo /
                                 render_pathtracing / render_generic; all exported here:
                                 `from redner_amd import render_deferred, PointLight`; shadows (`shadows=True`) for the
                                 point, spot and directional lights and ambient occlusion (`ambient_occlusion=K, ao_radius=r`)
                                 for the AmbientLights and SHLights, both traced on the path tracer's any-hit kernels;
                                 specular highlights (`specular=True`, `deferred_specular`): the specular lobe of the path
                                 tracer's BSDF under the point, spot and directional lights, one native kernel and its adjoint
                                 rectangular area lights (`QuadLight`, `quad_light`, `deferred_quad`): the exact diffuse
                                 irradiance of a quad emitter, clipped to the horizon, one native kernel and its adjoint;
                                 softly shadowed by `quad_shadow_rays=K` (`deferred_quad(occluders=..., shadow_rays=K)`,
                                 `DeferredQuadShadowed`): K any-hit rays per texel and quad weight a visibility factor
    redner_amd.texture           mip-mapped Texture / EnvironmentMap and generate_mipmap on the native pyramid kernels:
                                 `from redner_amd import Texture, EnvironmentMap, generate_mipmap`; envmap_sampling_tables:
                                 the sampling tables of an environment map by one native call
    redner_amd.utils             SH_reconstruct on the native spherical-harmonic kernels (a coefficient gradient included):
                                 `from redner_amd import SH_reconstruct`
    redner_amd.shape             compute_vertex_normal on the native vertex-normal kernels (a vertex gradient included):
                                 `from redner_amd import compute_vertex_normal, MeshTopology`; smooth / bound_vertices and
                                 the differentiable mesh_laplacian on the native smoothing kernels, on the same plan
    redner_amd.loss              gaussian_pyramid_loss, the image pyramid loss of the reference's optimisation scripts, on the
                                 native pyramid-loss kernels (an image gradient included):
                                 `from redner_amd import gaussian_pyramid_loss, GaussianPyramidLoss`
    redner_amd.transform         gen_rotate_matrix and pose_vertices, the rigid pose of the reference's pose-estimation scripts
                                 (rotate every vertex set about a centre, translate), on the native pose kernels, with
                                 gradients to angles, translation, centre and vertices:
                                 `from redner_amd import gen_rotate_matrix, pose_vertices, RotateMatrix, PoseVertices`
    redner_amd.install()         register redner_amd.redner as `redner` for the reference's
                                 unmodified pyredner package
"""
import sys

_RENDER_UTILS = ('DeferredLight', 'AmbientLight', 'PointLight', 'DirectionalLight', 'SpotLight', 'SHLight', 'DeferredShade',
                 'deferred_shade', 'DeferredSpecular', 'deferred_specular', 'QuadLight', 'quad_light', 'DeferredQuad', 'DeferredQuadShadowed',
                 'deferred_quad', 'occluder_scene', 'render_deferred', 'render_generic', 'render_g_buffer', 'render_albedo',
                 'render_pathtracing')
_TEXTURE = ('Texture', 'EnvironmentMap', 'generate_mipmap', 'MipPyramid', 'envmap_sampling_tables')
_UTILS = ('SH_reconstruct', 'SHReconstruct')
_LOSS = ('gaussian_pyramid_loss', 'GaussianPyramidLoss')
_TRANSFORM = ('gen_rotate_matrix', 'pose_vertices', 'RotateMatrix', 'PoseVertices')
_SHAPE = ('compute_vertex_normal', 'MeshTopology', 'VertexNormals', 'smooth', 'mesh_laplacian', 'bound_vertices', 'MeshLaplacian')


def __getattr__(name):
    # resolved on first use: `import redner_amd` alone does not import torch
    if name in _RENDER_UTILS:
        from . import render_utils
        return getattr(render_utils, name)
    if name in _TEXTURE:
        from . import texture
        return getattr(texture, name)
    if name in _SHAPE:
        from . import shape
        return getattr(shape, name)
    if name in _UTILS:
        from . import utils
        return getattr(utils, name)
    if name in _LOSS:
        from . import loss
        return getattr(loss, name)
    if name in _TRANSFORM:
        from . import transform
        return getattr(transform, name)
    raise AttributeError('module %r has no attribute %r' % (__name__, name))


def install():
    """Make `import redner` resolve to the MI355X implementation (drop-in for pyredner)."""
    from . import redner as _redner
    sys.modules['redner'] = _redner
    return _redner


def trim_cache():
    """Release the per-call device buffers the library keeps parked between render() calls (bytes released)."""
    from . import redner as _redner
    return _redner.trim_cache()
