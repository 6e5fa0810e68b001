"""Deferred shading (redner_amd.render_utils on rdr_deferred_shade / rdr_deferred_shade_backward) against fixtures made by the
reference's own deferred-shading code under torch autograd (tests/golden/make_deferred_golden.py).

Bars: parity_util.TOL = 1e-4 relative L2 on every whole tensor (image, G-buffer gradient, each light tensor's gradient, and for
the end-to-end cases the vertex, texel and camera gradients); the expected error is fp32 rounding, 1e-7 ... 1e-6
(profiles/deferred_shade.txt has the measured maxima).  The harness cases run the same per-texel bodies as the kernels, as
plain loops; the GPU cases run on both builds of the library."""
import os

import numpy as np
import pytest
import torch

import parity_util
from golden import make_deferred_golden as mk

GOLD = parity_util.GOLD
KERNEL_CASES = [(aa, alpha, name) for aa in (1, 2, 3) for alpha in (0, 1) for name in ('one_each', 'two_each', 'empty')]
E2E = [(name, alpha) for name in mk.E2E_CASES for alpha in (0, 1)]


def _render_utils(backend):
    from redner_amd import render_utils
    return render_utils


def _check(name, out, gold, tag):
    assert np.isfinite(out['image']).all(), name
    rep = parity_util.compare(out, gold, name)
    print(name, tag, {k: '%.2e' % e['rel_l2'] for k, e in rep.items()})
    parity_util.record(name, rep, tag)
    parity_util.assert_parity(rep, name)


def _shade_case(backend, device, g, types, params, ranges, aa, alpha):
    """forward + backward through the public surface -> the fixture's entries"""
    ru = _render_utils(backend)
    g = torch.from_numpy(g).to(device).requires_grad_(True)
    lights = mk.lights_from_table(ru, types, params, device='cpu')            # light tensors live on the host, as in user scripts
    per_image = [lights[b:e] for b, e in zip(ranges[:-1], ranges[1:])] if ranges is not None else lights
    img = ru.deferred_shade(g, per_image, alpha=bool(alpha), aa_samples=aa, backend=backend)
    (img * mk.upstream(img.shape).to(device)).sum().backward()
    out = {'image': img.detach().cpu().numpy(), 'd_g_buffer': g.grad.cpu().numpy()}
    out.update(mk.light_gradients(types, lights))
    return out


def _kernel_fixture(aa, alpha, name):
    z = np.load(os.path.join(GOLD, 'deferred_kernel_aa%d_alpha%d.npz' % (aa, alpha)))
    pre = name + '__'
    return z['g_buffer'], {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}


def _run_kernel_case(backend, device, aa, alpha, name, tag):
    g, gold = _kernel_fixture(aa, alpha, name)
    types, params = gold.pop('types'), gold.pop('params')
    out = _shade_case(backend, device, g, types, params, None, aa, alpha)
    _check('deferred_kernel_aa%d_alpha%d_%s' % (aa, alpha, name), out, gold, tag)


def _run_batch_case(backend, device, tag):
    z = np.load(os.path.join(GOLD, 'deferred_kernel_batch.npz'))
    gold = {k[len('batch__'):]: z[k] for k in z.files if k.startswith('batch__')}
    types, params = gold.pop('types'), gold.pop('params')
    out = _shade_case(backend, device, z['g_buffer'], types, params, [int(r) for r in z['ranges']], 2, 1)
    _check('deferred_kernel_batch', out, gold, tag)


@pytest.mark.parametrize('aa,alpha,name', KERNEL_CASES)
def test_deferred_shade_hostsim(hostsim_backend, aa, alpha, name):
    _run_kernel_case(hostsim_backend, torch.device('cpu'), aa, alpha, name, 'hostsim')


def test_deferred_shade_batch_hostsim(hostsim_backend):
    _run_batch_case(hostsim_backend, torch.device('cpu'), 'hostsim')


@pytest.mark.gpu
@pytest.mark.parametrize('aa,alpha,name', KERNEL_CASES)
def test_deferred_shade_gpu(gpu_backend, aa, alpha, name):
    _run_kernel_case(gpu_backend, torch.device('cuda:0'), aa, alpha, name, 'gpu')


@pytest.mark.gpu
def test_deferred_shade_batch_gpu(gpu_backend):
    _run_batch_case(gpu_backend, torch.device('cuda:0'), 'gpu')


def _render_deferred_case(backend, device, name, alpha):
    ru = _render_utils(backend)
    builder, res, seed = mk.E2E_CASES[name]
    sc = mk.e2e_scene(builder, res, device)
    types, params = mk.light_table(mk.e2e_lights())
    lights = mk.lights_from_table(ru, types, params)
    img = ru.render_deferred(sc, lights, alpha=bool(alpha), aa_samples=mk.E2E_AA, seed=seed, device=device, backend=backend)
    assert tuple(img.shape) == (res, res, 3 + alpha)
    (img * mk.upstream(img.shape).to(device)).sum().backward()
    out = {'image': img.detach().cpu().numpy()}
    out.update(mk.e2e_gradients(sc))
    out.update(mk.light_gradients(types, lights))
    return out


@pytest.mark.parametrize('name,alpha', E2E)
def test_render_deferred_hostsim(hostsim_backend, name, alpha):
    out = _render_deferred_case(hostsim_backend, torch.device('cpu'), name, alpha)
    _check('deferred_%s_alpha%d' % (name, alpha), out, np.load(os.path.join(GOLD, 'deferred_%s_alpha%d.npz' % (name, alpha))), 'hostsim')


@pytest.mark.gpu
@pytest.mark.parametrize('name,alpha', E2E)
def test_render_deferred_gpu(gpu_backend, name, alpha):
    out = _render_deferred_case(gpu_backend, torch.device('cuda:0'), name, alpha)
    _check('deferred_%s_alpha%d' % (name, alpha), out, np.load(os.path.join(GOLD, 'deferred_%s_alpha%d.npz' % (name, alpha))), 'gpu')


@pytest.mark.gpu
def test_light_gradients_bitwise_reproducible_gpu(gpu_backend):
    """The light gradients are sums over 4 M texels: a slab of per-block fp64 partials folded in a fixed order, no atomics."""
    ru = _render_utils(gpu_backend)
    dev = torch.device('cuda:0')
    g = mk.synthetic_g_buffer(5, 1, 1024, 1024, 2, 1).to(dev)
    types, params = mk.light_table(mk.light_sets()['one_each'])
    params = torch.from_numpy(params).to(dev)
    up = mk.upstream((1, 1024, 1024, 4)).to(dev)
    runs = []
    for _ in range(2):
        gl, pl = g.clone().requires_grad_(True), params.clone().requires_grad_(True)
        img = ru.DeferredShade.apply(gl, pl, tuple(types), ((0, len(types)),), 2, True, gpu_backend)
        img.backward(up)
        runs.append((gl.grad.cpu().numpy(), pl.grad.cpu().numpy()))
    assert np.isfinite(runs[0][1]).all() and np.abs(runs[0][1]).sum() > 0
    assert runs[0][1].tobytes() == runs[1][1].tobytes()
    assert runs[0][0].tobytes() == runs[1][0].tobytes()


@pytest.mark.gpu
def test_long_light_list_gpu(gpu_backend):
    """A light's parameter gradient does not depend on the other lights of the list: 200 lights (more than one adjoint launch
    covers) give, row by row, the bytes that a call with a 40-light slice of the list gives; the texel gradients of the two
    slices of a split list add up to those of the whole list."""
    ru = _render_utils(gpu_backend)
    dev = torch.device('cuda:0')
    g = mk.synthetic_g_buffer(9, 1, mk.KERNEL_H, mk.KERNEL_W, 2, 1).to(dev)
    types, params = mk.light_table(mk.light_sets()['two_each'] * 25)
    params = params * (1.0 + 0.001 * np.arange(len(types), dtype=np.float32))[:, None]       # 200 different lights
    up = mk.upstream((1, mk.KERNEL_H, mk.KERNEL_W, 4)).to(dev)

    def run(lo, hi):
        gl = g.clone().requires_grad_(True)
        pl = torch.from_numpy(params[lo:hi]).to(dev).requires_grad_(True)
        img = ru.DeferredShade.apply(gl, pl, tuple(types[lo:hi]), ((0, hi - lo),), 2, True, gpu_backend)
        img.backward(up)
        return img.detach(), gl.grad, pl.grad

    img, dg, dp = run(0, 200)
    assert torch.isfinite(img).all() and torch.isfinite(dp).all()
    for lo, hi in ((0, 40), (80, 120), (160, 200)):
        assert torch.equal(run(lo, hi)[2], dp[lo:hi]), (lo, hi)
    a, b = run(0, 120), run(120, 200)
    assert parity_util.rel_l2((a[1] + b[1])[..., :9], dg[..., :9]) < 1e-6          # (alpha's gradient is in both halves)
    assert torch.equal(a[1][..., 9], dg[..., 9])
    assert parity_util.rel_l2(a[0][..., :3] + b[0][..., :3], img[..., :3]) < 1e-6


@pytest.mark.gpu
def test_render_deferred_batch_equals_singles_gpu(gpu_backend):
    """One launch over N scenes does the same arithmetic per texel as N launches: the image and the G-buffer gradient are equal
    bit for bit.  Two kinds of tensors are sums whose order differs between the two ways of calling and are held to 1e-6 instead:
    the shared lights' gradients (ONE fp64 sum over all N images in the batch call, a sum of N rounded fp32 results in the single
    calls, and the adjoint's capped grid partitions the pixels differently), and the scene gradients, which the renderer's own
    adjoint accumulates with fp64 atomics (order-dependent in the last fp64 bits, whatever this kernel hands it)."""
    ru = _render_utils(gpu_backend)
    dev = torch.device('cuda:0')
    seeds = [3, 4, 5]
    types, params = mk.light_table(mk.e2e_lights())

    def scenes_and_lights():
        import scenes
        scs = [scenes.two_triangles(dev, resolution=(32, 32)) for _ in seeds]
        for k, sc in enumerate(scs):                                       # three different scenes
            sc.shapes[0].vertices.data[:, 0] += 0.1 * k
        return scs, mk.lights_from_table(ru, types, params)

    scs, lights = scenes_and_lights()
    batch = ru.render_deferred(scs, lights, alpha=True, aa_samples=2, seed=seeds, device=dev, backend=gpu_backend)
    assert tuple(batch.shape) == (3, 32, 32, 4)
    up = mk.upstream(batch.shape).to(dev)
    (batch * up).sum().backward()
    scs1, lights1 = scenes_and_lights()
    singles = [ru.render_deferred(sc, lights1, alpha=True, aa_samples=2, seed=se, device=dev, backend=gpu_backend)
               for sc, se in zip(scs1, seeds)]
    (torch.stack(singles) * up).sum().backward()
    assert torch.equal(batch, torch.stack(singles))
    for a, b in zip(scs, scs1):
        for i in (0, 1):
            assert parity_util.rel_l2(a.shapes[i].vertices.grad, b.shapes[i].vertices.grad) < 1e-6
    ga, gb = mk.light_gradients(types, lights), mk.light_gradients(types, lights1)
    for k in ga:
        assert parity_util.rel_l2(torch.from_numpy(ga[k]), torch.from_numpy(gb[k])) < 1e-6, k
    # the shading step alone on the stacked G-buffers: its texel gradients bit for bit
    ch = [gpu_backend.channels.position, gpu_backend.channels.shading_normal, gpu_backend.channels.diffuse_reflectance,
          gpu_backend.channels.alpha]
    for sc in scs:
        sc.camera.resolution = (64, 64)
    g = ru.render_g_buffer(scs, ch, seed=seeds, device=dev, backend=gpu_backend).detach()
    gb_ = g.clone().requires_grad_(True)
    (ru.deferred_shade(gb_, lights, alpha=True, aa_samples=2, backend=gpu_backend) * up).sum().backward()
    for k in range(len(seeds)):
        gs = g[k:k + 1].clone().requires_grad_(True)
        one = ru.deferred_shade(gs, lights, alpha=True, aa_samples=2, backend=gpu_backend)
        assert torch.equal(one[0], batch[k])
        (one * up[k:k + 1]).sum().backward()
        assert torch.equal(gs.grad[0], gb_.grad[k])


def test_render_deferred_restores_camera(hostsim_backend):
    from redner_amd import render_utils as ru
    import scenes
    cpu = torch.device('cpu')
    sc = scenes.single_triangle(cpu, resolution=(12, 16))
    sc.camera.viewport = (2, 4, 10, 12)
    lights = [ru.AmbientLight(torch.tensor([0.5, 0.5, 0.5]))]
    img = ru.render_deferred(sc, lights, aa_samples=2, seed=1, device=cpu, backend=hostsim_backend)
    assert tuple(img.shape) == (8, 8, 3)
    assert sc.camera.resolution == (12, 16) and sc.camera.viewport == (2, 4, 10, 12)
    sc.shapes[0].vertices.data[0, 0] = float('nan')                       # serialize_scene refuses non-finite scene tensors
    with pytest.raises(AssertionError):
        ru.render_deferred(sc, lights, aa_samples=3, seed=1, device=cpu, backend=hostsim_backend)
    assert sc.camera.resolution == (12, 16) and sc.camera.viewport == (2, 4, 10, 12)


def test_deferred_argument_errors(hostsim_backend):
    from redner_amd import render_utils as ru
    rd = hostsim_backend
    g = mk.synthetic_g_buffer(1, 1, 4, 4, 2, 0)
    params = torch.zeros(2, 10)
    img = torch.zeros(1, 4, 4, 3)
    ptr = lambda t: rd.float_ptr(t.data_ptr())
    with pytest.raises(RuntimeError, match='outside the table'):          # a light range that leaves the table
        rd.deferred_shade(ptr(g), ptr(params), ptr(img), 1, 4, 4, 2, False, [0, 1], [(1, 3)], False, 0)
    with pytest.raises(RuntimeError, match='outside the table'):
        rd.deferred_shade(ptr(g), ptr(params), ptr(img), 1, 4, 4, 2, False, [0, 1], [(2, 1)], False, 0)
    with pytest.raises(RuntimeError, match='unknown light type'):
        rd.deferred_shade(ptr(g), ptr(params), ptr(img), 1, 4, 4, 2, False, [0, 7], [(0, 2)], False, 0)
    with pytest.raises(RuntimeError, match='must be positive'):
        rd.deferred_shade_backward(ptr(g), ptr(params), ptr(img), ptr(g), ptr(params), 1, 0, 4, 2, False, [0, 1], [(0, 2)], False, 0)
    with pytest.raises(RuntimeError, match='light ranges'):               # one range for two images
        rd.deferred_shade(ptr(g), ptr(params), ptr(img), 2, 4, 4, 2, False, [0, 1], [(0, 2)], False, 0)
    # size mismatches are caught before anything native runs
    with pytest.raises(RuntimeError, match='does not divide'):
        ru.DeferredShade.apply(g, params, (0, 1), ((0, 2),), 3, False, rd)
    with pytest.raises(RuntimeError, match='G-buffer must be'):
        ru.DeferredShade.apply(g, params, (0, 1), ((0, 2),), 2, True, rd)
    with pytest.raises(RuntimeError, match='light_params must be'):
        ru.DeferredShade.apply(g, params, (0, 1, 2), ((0, 2),), 2, False, rd)
    with pytest.raises(RuntimeError, match='expected 3'):
        ru.deferred_shade(g, [ru.AmbientLight(torch.ones(4))], aa_samples=2, backend=rd)
    # ... and a light called directly goes through the same kernel as the batch path
    light = ru.PointLight(torch.tensor([1.0, 2.0, -3.0]), torch.tensor([30.0, 25.0, 20.0]))
    direct = light.render(g[0, :, :, :3], g[0, :, :, 3:6], g[0, :, :, 6:9])
    assert torch.equal(direct, ru.deferred_shade(g, [light], aa_samples=1, backend=rd)[0])


@pytest.mark.gpu
def test_render_family_matches_render_function_gpu(gpu_backend):
    from redner_amd import render_utils as ru
    from redner_amd.render_pytorch import RenderFunction
    import scenes
    rd, dev = gpu_backend, torch.device('cuda:0')
    sc = scenes.textured_sphere(dev, resolution=(48, 48))

    def explicit(channels, num_samples, max_bounces, sampler, seed):
        args = RenderFunction.serialize_scene(sc, num_samples, max_bounces, channels=channels, sampler_type=sampler, device=dev, backend=rd)
        return RenderFunction.apply(seed, *args)

    ch = [rd.channels.depth, rd.channels.shading_normal, rd.channels.uv]
    assert torch.equal(ru.render_g_buffer(sc, ch, seed=3, device=dev, backend=rd), explicit(ch, (1, 1), 0, rd.SamplerType.sobol, 3))
    assert torch.equal(ru.render_albedo(sc, alpha=True, seed=4, device=dev, backend=rd),
                       explicit([rd.channels.diffuse_reflectance, rd.channels.alpha], (16, 4), 0, rd.SamplerType.sobol, 4))
    assert torch.equal(ru.render_pathtracing(sc, max_bounces=2, seed=5, device=dev, backend=rd),
                       explicit([rd.channels.radiance], (4, 4), 2, rd.SamplerType.sobol, 5))
    both = ru.render_generic([sc, sc], [rd.channels.radiance], seed=[6, 7], device=dev, backend=rd)
    assert torch.equal(both[1], explicit([rd.channels.radiance], (4, 4), 1, rd.SamplerType.sobol, 7))
