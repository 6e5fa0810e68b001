#!/usr/bin/env python3
"""Generate the deferred-shading fixtures under tests/golden/ (run in the BUILD container only).

The expected values come from the REFERENCE's own deferred-shading code executed by torch on the CPU: the `.render` of the
light classes of its pyredner/render_utils.py, its `cat` of the alpha channel and its `interpolate(mode='area')` resolve, with
every gradient from torch autograd.  Nothing here restates a shading formula.  Needs the reference checkout (its unmodified
Python package, imported on top of the oracle build of its `redner` module, like tests/golden/make_golden.py) and, for the
end-to-end cases, the oracle build itself (oracle/_ref), which renders the G-buffers.

  deferred_kernel_aa<A>_alpha<0|1>.npz   a synthetic G-buffer of 20 x 24 output pixels and, for each light set (`one_each`,
                                         `two_each`, `empty`): light table, image, G-buffer gradient, every light tensor's gradient
  deferred_kernel_batch.npz              N = 3 G-buffers lit by light lists of different lengths (2, 0, 3)
  deferred_<scene>_alpha<0|1>.npz        render_deferred on two_triangles 64 x 64 and textured_sphere 48 x 48, aa_samples 2:
                                         image + the gradients of the vertices, the diffuse texels, the camera position, the lights

The helpers at the top (synthetic G-buffer, light sets, upstream gradient) are also what tests/test_deferred.py builds its
inputs from; they need neither the reference nor the oracle.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = '/root/reference'

KERNEL_H, KERNEL_W = 20, 24
FIELDS = {0: ('intensity',), 1: ('position', 'intensity'), 2: ('direction', 'intensity'),
          3: ('position', 'spot_direction', 'spot_exponent', 'intensity')}          # constructor order of the four light classes
CLASS_NAMES = {0: 'AmbientLight', 1: 'PointLight', 2: 'DirectionalLight', 3: 'SpotLight'}
# where a field lives in a row of the [L, 10] light table (redner_amd/csrc/deferred.h)
COLUMNS = {'intensity': slice(0, 3), 'position': slice(3, 6), 'direction': slice(6, 9), 'spot_direction': slice(6, 9),
           'spot_exponent': slice(9, 10)}


def upstream(shape):
    """The smooth upstream gradient of make_golden.render_case: every pixel / channel has its own weight.  [..., H, W, C]"""
    h, w, c = shape[-3:]
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing='ij')
    base = [1.0 + 0.5 * torch.sin(0.37 * xx + 0.11 * yy), 1.0 + 0.5 * torch.cos(0.23 * yy),
            1.0 - 0.3 * torch.sin(0.19 * (xx + yy))]
    up = torch.stack([base[k % 3] * (1.0 + 0.25 * (k // 3)) for k in range(c)], dim=2)
    lead = tuple(shape[:-3])
    if lead:
        scale = 1.0 + 0.1 * torch.arange(int(np.prod(lead)), dtype=torch.float32).reshape(lead + (1, 1, 1))
        up = up * scale
    return up.contiguous()


def synthetic_g_buffer(seed, n, h, w, aa, alpha):
    """[n, h * aa, w * aa, 9 + alpha]: positions in x, y in [-2, 2], z in [0.5, 2]; unit normals; albedo in [0.1, 0.9]; alpha in
    [0, 1].  The bottom-left quarter of every image is BACKGROUND (all zeros, as the renderer writes it), and the top-right
    eighth is a plane whose normal is exactly (0, 1, 0): perpendicular to a directional light along x."""
    gen = torch.Generator().manual_seed(seed)
    hg, wg = h * aa, w * aa
    pos = torch.rand(n, hg, wg, 3, generator=gen) * torch.tensor([4.0, 4.0, 1.5]) + torch.tensor([-2.0, -2.0, 0.5])
    nrm = torch.randn(n, hg, wg, 3, generator=gen)
    nrm = nrm / nrm.norm(dim=-1, keepdim=True)
    alb = 0.1 + 0.8 * torch.rand(n, hg, wg, 3, generator=gen)
    parts = [pos, nrm, alb]
    if alpha:
        parts.append(torch.rand(n, hg, wg, 1, generator=gen))
    g = torch.cat(parts, dim=-1)
    g[:, : hg // 4, wg // 2:, 3:6] = torch.tensor([0.0, 1.0, 0.0])
    g[:, hg // 2:, : wg // 2, :] = 0.0
    return g.contiguous()


def light_sets():
    """name -> [(type, {field: values})]: one light of each type, two of each, none.  Point and spot lights stay >= 1.5 away from
    every texel; the spot at (0, 0, -1) looks sideways, so the texels at negative x are BEHIND it; exponents 1 and 3."""
    amb = (0, {'intensity': [0.2, 0.25, 0.3]})
    point = (1, {'position': [1.0, 2.0, -3.0], 'intensity': [30.0, 25.0, 20.0]})
    tie = (2, {'direction': [2.0, 0.0, 0.0], 'intensity': [1.5, 1.2, 1.0]})              # perpendicular to the (0, 1, 0) plane
    spot3 = (3, {'position': [0.0, 0.0, -1.0], 'spot_direction': [1.0, 0.2, 0.3], 'spot_exponent': [3.0],
                 'intensity': [4.0, 5.0, 6.0]})
    amb2 = (0, {'intensity': [0.05, 0.02, 0.08]})
    point2 = (1, {'position': [-2.5, -1.0, -2.0], 'intensity': [12.0, 18.0, 9.0]})
    dir2 = (2, {'direction': [0.3, -0.5, 1.0], 'intensity': [0.8, 0.9, 1.1]})
    spot1 = (3, {'position': [0.5, -0.5, -1.2], 'spot_direction': [-1.0, 0.1, 0.4], 'spot_exponent': [1.0],
                 'intensity': [3.0, 2.0, 2.5]})
    return {'one_each': [amb, point, tie, spot3],
            'two_each': [amb, amb2, point, point2, tie, dir2, spot3, spot1],
            'empty': []}


def batch_lights():
    """Three light lists of different lengths (2, 0, 3) for the N = 3 fixture."""
    s = light_sets()['two_each']
    return [[s[0], s[2]], [], [s[4], s[7], s[3]]]


def light_table(spec):
    """[(type, fields)] -> (types [L] int32, params [L, 10] float32) in the layout of the native light table."""
    types = np.asarray([t for t, _ in spec], np.int32)
    params = np.zeros((len(spec), 10), np.float32)
    for i, (_, fields) in enumerate(spec):
        for name, v in fields.items():
            params[i, COLUMNS[name]] = v
    return types, params


def lights_from_table(module, types, params, device='cpu'):
    """Light objects of `module` (the reference's pyredner, or redner_amd) from a table; every field is its own leaf tensor."""
    lights = []
    for t, row in zip(types, params):
        kw = {f: torch.tensor(np.asarray(row[COLUMNS[f]]), dtype=torch.float32, device=device).requires_grad_(True)
              for f in FIELDS[int(t)]}
        lights.append(getattr(module, CLASS_NAMES[int(t)])(**kw))
    return lights


def light_gradients(types, lights, prefix='', base=0):
    """{'<prefix>grad_light<base + i>_<field>': gradient} of every light tensor (zeros where autograd left none)"""
    out = {}
    for i, (t, light) in enumerate(zip(types, lights), start=base):
        for f in FIELDS[int(t)]:
            g = getattr(light, f).grad
            out['%sgrad_light%d_%s' % (prefix, i, f)] = (torch.zeros(getattr(light, f).shape) if g is None else g).cpu().numpy()
    return out


# name -> (scene builder of tests/scenes.py, resolution, seed); lights of the end-to-end cases: one of each type
E2E_CASES = {'two_triangles': ('two_triangles', 64, 5), 'textured_sphere': ('textured_sphere', 48, 7)}
E2E_AA = 2


def e2e_lights():
    return [(0, {'intensity': [0.2, 0.2, 0.25]}),
            (1, {'position': [1.0, 2.0, -3.0], 'intensity': [40.0, 35.0, 30.0]}),
            (2, {'direction': [0.3, -0.5, 1.0], 'intensity': [0.8, 0.9, 1.1]}),
            (3, {'position': [-2.0, 1.0, -4.0], 'spot_direction': [2.0, -1.0, 4.0], 'spot_exponent': [2.0],
                 'intensity': [6.0, 5.0, 4.0]})]


def e2e_scene(builder, res, device):
    """The scene with gradients asked for on the vertices (as the builder sets them), the diffuse texels and the camera position."""
    sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, 'tests')) if p not in sys.path]
    import scenes
    sc = getattr(scenes, builder)(device, resolution=(res, res))
    for m in sc.materials:
        m.diffuse_reflectance.mipmap[0].requires_grad_(True)
    sc.camera.position.requires_grad_(True)
    return sc


def e2e_gradients(sc):
    out = {}
    for i, sh in enumerate(sc.shapes):
        if sh.vertices.grad is not None:
            out['grad_shape%d_vertices' % i] = sh.vertices.grad.cpu().numpy()
    for i, m in enumerate(sc.materials):
        t = m.diffuse_reflectance.mipmap[0]
        if t.grad is not None:
            out['grad_mat%d_diffuse' % i] = t.grad.cpu().numpy()
    out['grad_cam_position'] = sc.camera.position.grad.cpu().numpy()
    return out


# ---- everything below needs the reference -------------------------------------------------------------------------------------
def reference_package():
    sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, 'tests')) if p not in sys.path]
    import oracle_util
    ref = oracle_util.load_oracle()
    sys.modules['redner'] = ref
    sys.path[:0] = [os.path.join(ROOT, 'oracle', 'pystubs'), REF]
    import pyredner
    pyredner.set_use_gpu(False)
    return ref, pyredner


def reference_shade(g, light_lists, alpha, aa):
    """What the reference's render_deferred does with a stack of G-buffers [N, ...] and one light list per image
    (pyredner/render_utils.py:263-313): its lights' .render, summed; alpha appended; interpolate(area)."""
    imgs = []
    for n, lights in enumerate(light_lists):
        gb = g[n]
        pos, normal, albedo = gb[:, :, :3], gb[:, :, 3:6], gb[:, :, 6:9]
        img = torch.zeros(gb.shape[0], gb.shape[1], 3)
        for light in lights:
            img = img + light.render(pos, normal, albedo)
        if alpha:
            img = torch.cat((img, gb[:, :, 9:10]), dim=-1)
        imgs.append(img)
    imgs = torch.stack(imgs)
    if aa > 1:
        imgs = imgs.permute(0, 3, 1, 2)
        imgs = torch.nn.functional.interpolate(imgs, size=(g.shape[1] // aa, g.shape[2] // aa), mode='area')
        imgs = imgs.permute(0, 2, 3, 1)
    return imgs


def check_coverage(g, spec):
    """The fixture must contain what it is there for: the half-gradient tie, texels behind a spot, background."""
    pos, nrm, alb = g[..., :3], g[..., 3:6], g[..., 6:9]
    lit = alb.sum(-1) > 0
    assert (~lit).float().mean() > 0.2, 'no background'
    ties = behind = front = 0
    for t, f in spec:
        if t == 2:
            d = torch.tensor(f['direction'])
            l = -d / torch.norm(d)
            ties += int(((torch.sum(l.view(1, 1, 1, 3) * nrm, dim=-1) == 0) & lit).sum())
        if t == 3:
            l = torch.tensor(f['position']) - pos
            l = l / torch.norm(l, dim=-1, keepdim=True)
            s = -torch.tensor(f['spot_direction']) / torch.norm(torch.tensor(f['spot_direction']))
            c = torch.sum(l * s, dim=-1)
            behind += int(((c < 0) & lit).sum())
            front += int(((c > 0) & lit).sum())
        if t in (1, 3):
            assert float((torch.tensor(f['position']) - pos).norm(dim=-1).min()) > 0.5          # background texels sit at the origin
    if any(t == 2 for t, _ in spec):
        assert ties > 0, 'no texel sits on the max(l.n, 0) tie'
    if any(t == 3 for t, _ in spec):
        assert behind > 0 and front > 0, (behind, front)
    return ties, behind


def kernel_case(pyredner, g, specs, alpha, aa, prefix):
    """specs: one light spec list per image.  -> the fixture entries of this light set"""
    g = g.clone().requires_grad_(True)
    tables = [light_table(s) for s in specs]
    light_lists = [lights_from_table(pyredner, t, p) for t, p in tables]
    img = reference_shade(g, light_lists, alpha, aa)
    if img.requires_grad:                              # (no lights and no alpha: the image is a constant)
        (img * upstream(img.shape)).sum().backward()
    out = {prefix + 'types': np.concatenate([t for t, _ in tables]).astype(np.int32),
           prefix + 'params': np.concatenate([p for _, p in tables]).reshape(-1, 10).astype(np.float32),
           prefix + 'image': img.detach().numpy(),
           prefix + 'd_g_buffer': (g.grad if g.grad is not None else torch.zeros_like(g)).numpy()}
    base = 0
    for (types, _), lights in zip(tables, light_lists):
        out.update(light_gradients(types, lights, prefix, base))          # light indices are those of the concatenated table
        base += len(types)
    return out


def make_kernel_fixtures(pyredner):
    for aa in (1, 2, 3):
        for alpha in (0, 1):
            g = synthetic_g_buffer(100 + 10 * aa + alpha, 1, KERNEL_H, KERNEL_W, aa, alpha)
            out = {'g_buffer': g.numpy()}
            for name, spec in light_sets().items():
                ties, behind = check_coverage(g, spec)
                out.update(kernel_case(pyredner, g, [spec], alpha, aa, name + '__'))
                print('aa %d alpha %d %-8s: %d texels on the tie, %d behind a spot' % (aa, alpha, name, ties, behind))
            np.savez_compressed(os.path.join(HERE, 'deferred_kernel_aa%d_alpha%d.npz' % (aa, alpha)), **out)
    g = synthetic_g_buffer(77, 3, KERNEL_H, KERNEL_W, 2, 1)
    specs = batch_lights()
    out = {'g_buffer': g.numpy(), 'ranges': np.cumsum([0] + [len(s) for s in specs]).astype(np.int32)}
    out.update(kernel_case(pyredner, g, specs, 1, 2, 'batch__'))
    np.savez_compressed(os.path.join(HERE, 'deferred_kernel_batch.npz'), **out)


def make_e2e_fixtures(ref, pyredner):
    from redner_amd.render_pytorch import RenderFunction
    cpu = torch.device('cpu')
    for name, (builder, res, seed) in E2E_CASES.items():
        for alpha in (0, 1):
            sc = e2e_scene(builder, res, cpu)
            channels = [ref.channels.position, ref.channels.shading_normal, ref.channels.diffuse_reflectance]
            if alpha:
                channels.append(ref.channels.alpha)
            # the G-buffer as the reference's render_deferred asks for it (render_utils.py:174-193), rendered by the oracle
            sc.camera.resolution = (res * E2E_AA, res * E2E_AA)
            args = RenderFunction.serialize_scene(sc, (1, 1), 0, channels=channels, sampler_type=ref.SamplerType.sobol,
                                                  use_primary_edge_sampling=True, use_secondary_edge_sampling=False,
                                                  sample_pixel_center=False, device=cpu, backend=ref)
            sc.camera.resolution = (res, res)
            g = RenderFunction.apply(seed, *args)
            types, params = light_table(e2e_lights())
            lights = lights_from_table(pyredner, types, params)
            img = reference_shade(g.unsqueeze(0), [lights], alpha, E2E_AA)[0]
            (img * upstream(img.shape)).sum().backward()
            out = {'image': img.detach().numpy()}
            out.update(e2e_gradients(sc))
            out.update(light_gradients(types, lights))
            assert np.isfinite(out['image']).all()
            np.savez_compressed(os.path.join(HERE, 'deferred_%s_alpha%d.npz' % (name, alpha)), **out)
            print(name, alpha, {k: v.shape for k, v in out.items()})


def main():
    # like make_golden.main: fresh zero pages for the reference's scratch buffers (its primary-edge pass reads entries it never
    # wrote for scenes with mip-mapped textures)
    if os.environ.get('MALLOC_MMAP_THRESHOLD_') != '65536' or os.environ.get('MALLOC_PERTURB_') != '255':
        import subprocess
        env = dict(os.environ, MALLOC_MMAP_THRESHOLD_='65536', MALLOC_PERTURB_='255')
        sys.exit(subprocess.call([sys.executable] + sys.argv, env=env))
    ref, pyredner = reference_package()
    make_kernel_fixtures(pyredner)
    make_e2e_fixtures(ref, pyredner)


if __name__ == '__main__':
    main()
