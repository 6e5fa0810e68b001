#!/usr/bin/env python3
"""Generate the wide-generic-texture fixtures under tests/golden/ (run in the BUILD container only).

A material's `generic_texture` may have any number of channels.  The expected values come from the REFERENCE's CPU core through
the oracle build (oracle/_ref), the pyramids from the reference's own `pyredner.Texture`, as in make_texture_golden.py whose
scene and recipe (`sphere_scene`, `render_e2e`) these cases use: constant specular reflectance and roughness, so no sample draw
depends on a texel; 4 x 4 samples; no geometry asks for a gradient, so there is no edge sampling (the reference overruns its own
scratch with generic textures under edge sampling, make_golden.py: CASES).

  wide_generic_sphere_<N>.npz    textured_sphere at 32 x 32 whose sphere carries Texture(diffuse 32 x 32 x 3) and
                                 Texture(generic 8 x 8 x N), N = 17, 33, 64: image (radiance + generic_texture),
                                 d(diffuse texels), d(generic texels).  The generic pyramid has four levels; at this size the
                                 sphere's lookups take the magnified branch and the between-levels branch (asserted below, on
                                 the oracle), but never get past level 1:
  wide_generic_sphere_33_far.npz the 33-wide case once more with uv_scale (12, 12) on the generic texture, which lifts every
                                 level by log2(12): the between-levels branch and the COARSEST-level branch (asserted too)
  wide_generic_constant_20.npz   the same with a CONSTANT 20-channel generic texture: image, d(diffuse texels), d(generic)
  wide_generic_quads.npz         16 x 16 frame over three abutting quads -- generic 8 x 8 x 5, generic 8 x 8 x 33, no generic
                                 texture -- so that single waves of 64 pixels straddle the three: image (generic_texture only,
                                 max_bounces 0), d(texels of the 5-wide), d(texels of the 33-wide)
  wide_generic_dropin_32.npz     the reference's own pyredner.render_generic of the sphere with a 32-channel pyredner.Texture:
                                 image, d(generic texels)

The helpers at the top (inputs, scenes) are also what tests/test_wide_generic.py builds its inputs from; they need neither the
reference nor the oracle.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [p for p in (HERE,) if p not in sys.path]
import make_deferred_golden as mk          # noqa: E402
import make_texture_golden as mt           # noqa: E402

WIDTHS = (17, 33, 64)
FAR_WIDTH, FAR_UV_SCALE = 33, (12.0, 12.0)
CONSTANT_WIDTH = 20
FRAME = (32, 32)
QUAD_FRAME = (16, 16)
QUAD_WIDTHS = (5, 33)
QUAD_SEED = 5
DROPIN_WIDTH, DROPIN_SEED = 32, 3
MAX_BYTES = mt.SPLIT_BYTES                 # every fixture stays below this


def _scenes():
    sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, 'tests')) if p not in sys.path]
    import scenes
    return scenes


def generic_texels(width, phase=2.0):
    """8 x 8 x width, values in [0.1, 0.9]: every channel its own pattern (tests/scenes.py)."""
    return torch.from_numpy(_scenes()._procedural(8, 8, width, phase))


def constant_generic():
    return torch.linspace(0.1, 0.9, CONSTANT_WIDTH)


def sphere_scene(device, make_texture, diffuse, generic, far=False):
    """make_texture_golden.sphere_scene on a 32 x 32 frame.  `generic` with one dimension is a constant texture; far: the
    generic texture gets FAR_UV_SCALE."""
    def make(t, uv):
        if t is generic and t.dim() == 1:
            return t
        return make_texture(t, torch.tensor(FAR_UV_SCALE, device=device) if t is generic and far else uv)
    sc = mt.sphere_scene(device, make, diffuse, generic)
    sc.camera.resolution = FRAME
    return sc


def quad_scene(device, make_texture, generics, only=None):
    """Three quads side by side in front of the camera, materials: generic[0] (5 wide), generic[1] (33 wide), no generic texture.
    only = k keeps quad k alone (the three materials stay, so the image keeps its channels)."""
    from redner_amd.render_pytorch import Camera, Shape, Material, AreaLight, Scene
    t = lambda x, dtype=torch.float32, dev=device: torch.tensor(x, dtype=dtype, device=dev)      # noqa: E731
    cam = Camera(position=t([0.1, 0.05, -5.0], dev='cpu'), look_at=t([0.0, 0.0, 0.0], dev='cpu'), up=t([0.0, 1.0, 0.0], dev='cpu'),
                 fov=t([45.0], dev='cpu'), clip_near=1e-2, resolution=QUAD_FRAME)
    quads = []
    for k, (x0, x1) in enumerate(((-1.7, -0.6), (-0.6, 0.5), (0.5, 1.7))):
        # one plane, tilted about the x axis: the footprint, and with it the level, changes down the quads, and none hides another
        z0, z1 = 0.0, 1.5
        quads.append(Shape(t([[x0, -1.6, z0], [x1, -1.6, z0], [x0, 1.6, z1], [x1, 1.6, z1]]), t([[0, 2, 1], [1, 2, 3]], torch.int32), k,
                           uvs=t([[0.0, 0.0], [1.3, 0.0], [0.0, 2.1], [1.3, 2.1]])))
    light = Shape(t([[-1.0, -1.0, -7.0], [1.0, -1.0, -7.0], [-1.0, 1.0, -7.0], [1.0, 1.0, -7.0]]), t([[0, 1, 2], [1, 3, 2]], torch.int32), 3)
    mats = [Material(diffuse_reflectance=t([0.5, 0.4, 0.3]), generic_texture=make_texture(generics[0], None)),
            Material(diffuse_reflectance=t([0.3, 0.4, 0.5]), generic_texture=make_texture(generics[1], None)),
            Material(diffuse_reflectance=t([0.4, 0.4, 0.4])),
            Material(diffuse_reflectance=t([0.0, 0.0, 0.0]))]
    shapes = quads if only is None else [quads[only]]
    return Scene(cam, shapes + [light], mats, [AreaLight(len(shapes), t([20.0, 20.0, 20.0], dev='cpu'))])


def render_quads(sc, device, backend, upstream=None):
    """generic_texture alone, first hits only, 4 x 4 samples; backward under mk.upstream (or `upstream`)."""
    from redner_amd.render_pytorch import RenderFunction
    args = RenderFunction.serialize_scene(sc, mt.E2E_SAMPLES, 0, channels=[backend.channels.generic_texture],
                                          sampler_type=backend.SamplerType.sobol, device=device, backend=backend)
    img = RenderFunction.apply(QUAD_SEED, *args)
    (img * (mk.upstream(img.shape) if upstream is None else upstream).to(device)).sum().backward()
    return img


# ---- everything below needs the reference -------------------------------------------------------------------------------------
def _save(name, out):
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < MAX_BYTES, (name, os.path.getsize(path))
    print(name, {k: v.shape for k, v in out.items()}, os.path.getsize(path), 'bytes')


def branch_counts(ref, sc):
    """-> pixels whose lookup is (magnified, between two levels, on the coarsest level alone), read off the oracle itself: the
    sphere's generic pyramid is swapped for one whose level l holds the value l everywhere, so a pixel-centre sample renders
    min(max(level, 0), 3) -- 0: the magnified branch, 3: the coarsest level alone, anything between: two levels mixed.  These are the lookups at the pixel centres, one per pixel; the fixtures' own
    4 x 4 jittered samples lie around them, so the assertion is about nearby lookups, not about the very samples compared."""
    from redner_amd.render_pytorch import RenderFunction, Texture
    kept = sc.materials[0].generic_texture
    sc.materials[0].generic_texture = Texture([torch.full((8 >> l, 8 >> l, 2), float(l)) for l in range(4)], kept.uv_scale)
    args = RenderFunction.serialize_scene(sc, (1, 1), 0, channels=[ref.channels.generic_texture, ref.channels.shape_id,
                                                                   ref.channels.alpha],
                                          sampler_type=ref.SamplerType.sobol, sample_pixel_center=True, device=torch.device('cpu'),
                                          backend=ref)
    g = RenderFunction.apply(1, *args).detach().numpy()
    sc.materials[0].generic_texture = kept
    level = g[:, :, 0][(g[:, :, 2] == 0) & (g[:, :, 3] > 0)]
    counts = (int((level == 0).sum()), int(((level > 0) & (level < 3)).sum()), int((level == 3).sum()))
    print('levels at the pixel centres: magnified %d, between levels %d, coarsest %d of %d pixels' % (counts + (len(level),)))
    return counts


def make_sphere_fixtures(ref, pyredner):
    from redner_amd import render_pytorch as rp
    cpu = torch.device('cpu')

    def ref_texture(texels, uv_scale):
        return rp.Texture(pyredner.Texture(texels).mipmap, uv_scale)

    for width, far in [(w, False) for w in WIDTHS + (CONSTANT_WIDTH,)] + [(FAR_WIDTH, True)]:
        diffuse = mt.sphere_texels()[0].requires_grad_(True)
        generic = (constant_generic() if width == CONSTANT_WIDTH else generic_texels(width)).requires_grad_(True)
        sc = sphere_scene(cpu, ref_texture, diffuse, generic, far)
        if width != CONSTANT_WIDTH:
            assert len(sc.materials[0].generic_texture.mipmap) == 4
            magnified, between, coarsest = branch_counts(ref, sc)
            assert between > 0 and (coarsest > 0 if far else magnified > 0), (width, far)
        img = mt.render_e2e(sc, 'sphere', [ref.channels.radiance, ref.channels.generic_texture], cpu, ref)
        assert tuple(img.shape) == FRAME + (3 + width,)
        out = {'image': img.detach().numpy(), 'grad_diffuse': diffuse.grad.numpy(), 'grad_generic': generic.grad.numpy()}
        assert np.isfinite(out['image']).all() and np.abs(out['grad_diffuse']).sum() > 0 and np.abs(out['grad_generic']).sum() > 0
        _save('wide_generic_constant_%d' % width if width == CONSTANT_WIDTH else
              'wide_generic_sphere_%d%s' % (width, '_far' if far else ''), out)


def hit_mask(ref, sc):
    """Pixels of which any of the fixture's 4 x 4 samples hits a quad (the alpha channel of the same render)."""
    from redner_amd.render_pytorch import RenderFunction
    args = RenderFunction.serialize_scene(sc, mt.E2E_SAMPLES, 0, channels=[ref.channels.alpha], sampler_type=ref.SamplerType.sobol,
                                          device=torch.device('cpu'), backend=ref)
    return RenderFunction.apply(QUAD_SEED, *args).detach().numpy()[:, :, 0] > 0


def make_quad_fixture(ref, pyredner):
    from redner_amd import render_pytorch as rp
    cpu = torch.device('cpu')
    generics = [generic_texels(w, 1.0 + k).requires_grad_(True) for k, w in enumerate(QUAD_WIDTHS)]
    sc = quad_scene(cpu, lambda t, uv: rp.Texture(pyredner.Texture(t).mipmap, uv), generics)
    img = render_quads(sc, cpu, ref)
    assert tuple(img.shape) == QUAD_FRAME + (max(QUAD_WIDTHS),)
    image = img.detach().numpy()
    # Every wave must see all three materials.  The first-hit stages run one lane per pixel of a sample, lane = pixel index in
    # row-major order (csrc/stages_fwd.h: GenPrimary / ShadePrimary index their slices by p; csrc/stages_bwd.h: AdjPrimary), and
    # a wave is 64 consecutive lanes: four rows of this 16-pixel-wide frame.
    assert QUAD_FRAME[1] * 4 == 64
    wide, narrow = np.abs(image[:, :, 5:]).sum(2) > 0, np.abs(image[:, :, :5]).sum(2) > 0
    hit = hit_mask(ref, sc)
    for rows in range(0, QUAD_FRAME[0], 4):
        w, n, h = wide[rows:rows + 4], narrow[rows:rows + 4], hit[rows:rows + 4]
        assert w.any() and (n & ~w).any() and (h & ~n & ~w).any(), rows        # 33 wide, 5 wide, a quad without the texture
    out = {'image': image, 'grad_generic5': generics[0].grad.numpy(), 'grad_generic33': generics[1].grad.numpy()}
    assert np.abs(out['grad_generic5']).sum() > 0 and np.abs(out['grad_generic33']).sum() > 0
    _save('wide_generic_quads', out)


def make_dropin_fixture(ref, pyredner):
    """What tests/test_wide_generic.py runs on the drop-in module, here on the reference's own."""
    out = dropin_render(pyredner, ref)
    _save('wide_generic_dropin_%d' % DROPIN_WIDTH, out)


def dropin_render(pyredner, redner):
    """pyredner.render_generic of the sphere under a 32-channel pyredner.Texture; reference classes throughout."""
    src = _scenes().textured_sphere(torch.device('cpu'), resolution=FRAME)
    cam = pyredner.Camera(position=torch.tensor([0.3, 0.2, -5.0]), look_at=torch.tensor([0.0, 0.0, 0.0]),
                          up=torch.tensor([0.0, 1.0, 0.0]), fov=torch.tensor([45.0]), clip_near=1e-2, resolution=FRAME)
    generic = generic_texels(DROPIN_WIDTH).requires_grad_(True)
    mats = [pyredner.Material(diffuse_reflectance=torch.tensor([0.5, 0.5, 0.5]), generic_texture=pyredner.Texture(generic)),
            pyredner.Material(diffuse_reflectance=torch.tensor([0.6, 0.55, 0.5])),
            pyredner.Material(diffuse_reflectance=torch.tensor([0.0, 0.0, 0.0]))]
    shapes = [pyredner.Shape(vertices=s.vertices.detach(), indices=s.indices, uvs=None if s.uvs is None else s.uvs.detach(),
                             normals=None if s.normals is None else s.normals.detach(), material_id=s.material_id)
              for s in src.shapes]
    scene = pyredner.Scene(cam, shapes, mats, [pyredner.AreaLight(shape_id=2, intensity=torch.tensor([25.0, 25.0, 25.0]))])
    img = pyredner.render_generic(scene, [redner.channels.generic_texture], max_bounces=0, sampler_type=redner.SamplerType.sobol,
                                  num_samples=(2, 2), seed=DROPIN_SEED, use_primary_edge_sampling=False,
                                  use_secondary_edge_sampling=False, device=torch.device('cpu'))
    (img * mk.upstream(img.shape)).sum().backward()
    return {'image': img.detach().numpy(), 'grad_generic': generic.grad.numpy()}


def main():
    # like make_golden.main: fresh zero pages for the reference's scratch buffers
    if os.environ.get('MALLOC_MMAP_THRESHOLD_') != '65536' or os.environ.get('MALLOC_PERTURB_') != '255':
        import subprocess
        env = dict(os.environ, MALLOC_MMAP_THRESHOLD_='65536', MALLOC_PERTURB_='255')
        sys.exit(subprocess.call([sys.executable] + sys.argv, env=env))
    ref, pyredner = mk.reference_package()
    make_sphere_fixtures(ref, pyredner)
    make_quad_fixture(ref, pyredner)
    make_dropin_fixture(ref, pyredner)


if __name__ == '__main__':
    main()
