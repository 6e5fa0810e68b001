#!/usr/bin/env python3
"""Generate the mip-pyramid fixtures under tests/golden/ (run in the BUILD container only).

The expected values come from the REFERENCE's own `pyredner.Texture` / `pyredner.EnvironmentMap` executed by torch on the CPU
(pad, conv2d, interpolate(area) per level, gradients from torch autograd); nothing here restates the pyramid's formula.  Needs
the reference checkout (its unmodified Python package, imported on top of the oracle build of its `redner` module, like
make_deferred_golden.reference_package()) and, for the end-to-end cases, the oracle build itself (oracle/_ref).

  texture_kernel_<H>x<W>x<C>.npz   for a seeded random image: level1 .. level<n-1>, num_levels, and d_texels under a fixed smooth
                                   upstream gradient on EVERY level (make_deferred_golden.upstream, scaled by 1 + 0.5 l so that
                                   a level mix-up shows).  `texels_sum` (fp64) guards the regenerated input.  The gradient of the
                                   largest image lives in texture_kernel_<H>x<W>x<C>_grad.npz (size limit of a committed file).
  texture_sphere.npz               the textured_sphere scene of tests/scenes.py whose sphere carries Texture(diffuse 32 x 32 x 3)
                                   and Texture(generic 8 x 8 x 5): channels radiance + generic_texture, 4 x 4 samples,
                                   max_bounces 1: image, d(diffuse texels), d(generic texels)
  texture_envmap.npz               the envmap_sphere scene under EnvironmentMap(values 16 x 32 x 3): image, d(values)

In the end-to-end cases the levels are built by the reference's `pyredner.Texture(texels).mipmap` (its torch ops, tracked by
autograd), handed to `render_pytorch.Texture(levels)` and rendered by the oracle; backward() then reaches `texels` through the
reference's own pyramid.  ROUGHNESS AND SPECULAR REFLECTANCE ARE CONSTANTS in both scenes: no sampling decision then depends on
a pyramid texel (light and lobe choice do not read the diffuse or generic texture, and the environment map's sampling tables
come from level 0, which is the input bit for bit), so a one-ulp difference between the native kernel's levels and torch's
cannot flip a sample, and the comparison at 1e-4 is one of arithmetic, not of sample draws.

The helpers at the top (inputs, upstream gradients, scenes) are also what tests/test_texture.py builds its inputs from; they need
neither the reference nor the oracle.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [p for p in (HERE,) if p not in sys.path]
import make_deferred_golden as mk          # noqa: E402

KERNEL_SIZES = [(1, 1, 3), (1, 7, 3), (2, 2, 1), (5, 3, 3), (13, 40, 5), (64, 64, 3), (100, 37, 1), (255, 129, 3), (300, 1, 2),
                (256, 256, 3), (96, 192, 3)]
SPLIT_BYTES = 900 * 1024                   # a fixture above this puts d_texels into a file of its own
E2E_SAMPLES, E2E_BOUNCES = (4, 4), 1
E2E_SEEDS = {'sphere': 7, 'envmap': 11}


def size_tag(size):
    return '%dx%dx%d' % tuple(size)


def kernel_texels(size):
    """The seeded random image of a kernel fixture, values in [0, 1)."""
    gen = torch.Generator().manual_seed(1000 + 7 * size[0] + 3 * size[1] + size[2])
    return torch.rand(*size, generator=gen)


def level_upstream(shape, level):
    return mk.upstream(tuple(shape)) * (1.0 + 0.5 * level)


def pyramid_loss(levels):
    """The scalar whose gradient the kernel fixtures hold: every level (level 0 too) under its own upstream gradient."""
    return sum((lv * level_upstream(lv.shape, l).to(lv.device)).sum() for l, lv in enumerate(levels))


def sphere_texels():
    sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, 'tests')) if p not in sys.path]
    import scenes
    return (torch.from_numpy(scenes._procedural(32, 32, 3, 0.0)), torch.from_numpy(scenes._procedural(8, 8, 5, 2.0)))


def _freeze(sc):
    """Only the textures under test ask for a gradient."""
    for sh in sc.shapes:
        for name in ('vertices', 'uvs', 'normals', 'colors'):
            t = getattr(sh, name)
            if t is not None:
                t.requires_grad_(False)
    return sc


def sphere_scene(device, make_texture, diffuse, generic):
    """tests/scenes.textured_sphere with the sphere's material swapped: make_texture(texels, uv_scale) -> a Texture; constant
    specular reflectance and roughness.  `diffuse` / `generic` are the leaf tensors whose gradients are compared."""
    sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, 'tests')) if p not in sys.path]
    import scenes
    from redner_amd.render_pytorch import Material
    sc = _freeze(scenes.textured_sphere(device, resolution=(48, 48)))
    sc.materials[0] = Material(diffuse_reflectance=make_texture(diffuse, torch.tensor([2.0, 1.0], device=device)),
                               specular_reflectance=torch.tensor([0.15, 0.2, 0.25], device=device),
                               roughness=torch.tensor([0.45], device=device),
                               generic_texture=make_texture(generic, None))
    sc.materials[1] = Material(diffuse_reflectance=torch.tensor([0.6, 0.55, 0.5], device=device))
    return sc


def envmap_values():
    sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, 'tests')) if p not in sys.path]
    import scenes
    return scenes.envmap_sphere(torch.device('cpu')).envmap.values.mipmap[0].detach().clone()


def envmap_scene(device, make_envmap, values):
    """tests/scenes.envmap_sphere with its environment map swapped: make_envmap(values, env_to_world) -> an EnvironmentMap.
    Its materials are constants already."""
    sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, 'tests')) if p not in sys.path]
    import scenes
    sc = _freeze(scenes.envmap_sphere(device, resolution=(48, 48)))
    for m in sc.materials:
        for name in ('diffuse_reflectance', 'specular_reflectance', 'roughness'):
            getattr(m, name).mipmap[0].requires_grad_(False)
    sc.envmap = make_envmap(values, sc.envmap.env_to_world.detach().clone())
    return sc


def render_e2e(sc, case, channels, device, backend):
    from redner_amd.render_pytorch import RenderFunction
    args = RenderFunction.serialize_scene(sc, E2E_SAMPLES, E2E_BOUNCES, channels=channels, sampler_type=backend.SamplerType.sobol,
                                          device=device, backend=backend)
    img = RenderFunction.apply(E2E_SEEDS[case], *args)
    (img * mk.upstream(img.shape).to(device)).sum().backward()
    return img


# ---- everything below needs the reference -------------------------------------------------------------------------------------
def make_kernel_fixtures(pyredner):
    for size in KERNEL_SIZES:
        texels = kernel_texels(size).requires_grad_(True)
        levels = pyredner.Texture(texels).mipmap
        pyramid_loss(levels).backward()
        out = {'num_levels': np.asarray(len(levels), np.int32), 'texels_sum': np.asarray(texels.detach().double().sum().item())}
        for l, lv in enumerate(levels[1:], start=1):
            out['level%d' % l] = lv.detach().numpy()
        grad = {'d_texels': texels.grad.numpy()}
        path = os.path.join(HERE, 'texture_kernel_%s.npz' % size_tag(size))
        if sum(v.nbytes for v in out.values()) + grad['d_texels'].nbytes > SPLIT_BYTES:
            np.savez_compressed(path[:-4] + '_grad.npz', **grad)
        else:
            out.update(grad)
        np.savez_compressed(path, **out)
        print(size_tag(size), [tuple(lv.shape) for lv in levels])


def make_e2e_fixtures(ref, pyredner):
    from redner_amd import render_pytorch as rp
    cpu = torch.device('cpu')

    def ref_texture(texels, uv_scale):
        return rp.Texture(pyredner.Texture(texels).mipmap, uv_scale)

    diffuse, generic = (t.requires_grad_(True) for t in sphere_texels())
    sc = sphere_scene(cpu, ref_texture, diffuse, generic)
    img = render_e2e(sc, 'sphere', [ref.channels.radiance, ref.channels.generic_texture], cpu, ref)
    out = {'image': img.detach().numpy(), 'grad_diffuse': diffuse.grad.numpy(), 'grad_generic': generic.grad.numpy()}
    assert np.isfinite(out['image']).all() and np.abs(out['grad_diffuse']).sum() > 0 and np.abs(out['grad_generic']).sum() > 0
    np.savez_compressed(os.path.join(HERE, 'texture_sphere.npz'), **out)
    print('sphere', {k: v.shape for k, v in out.items()})

    values = envmap_values().requires_grad_(True)
    sc = envmap_scene(cpu, lambda v, e2w: rp.EnvironmentMap(ref_texture(v, None), env_to_world=e2w), values)
    img = render_e2e(sc, 'envmap', [ref.channels.radiance], cpu, ref)
    out = {'image': img.detach().numpy(), 'grad_values': values.grad.numpy()}
    assert np.isfinite(out['image']).all() and np.abs(out['grad_values']).sum() > 0
    np.savez_compressed(os.path.join(HERE, 'texture_envmap.npz'), **out)
    print('envmap', {k: v.shape for k, v in out.items()})


def main():
    # like make_golden.main: fresh zero pages for the reference's scratch buffers
    if os.environ.get('MALLOC_MMAP_THRESHOLD_') != '65536' or os.environ.get('MALLOC_PERTURB_') != '255':
        import subprocess
        env = dict(os.environ, MALLOC_MMAP_THRESHOLD_='65536', MALLOC_PERTURB_='255')
        sys.exit(subprocess.call([sys.executable] + sys.argv, env=env))
    ref, pyredner = mk.reference_package()
    make_kernel_fixtures(pyredner)
    make_e2e_fixtures(ref, pyredner)


if __name__ == '__main__':
    main()
