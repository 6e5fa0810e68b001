"""Deferred shading (redner_amd.render_utils on rdr_deferred_shade / rdr_deferred_shade_backward) against fixtures made by the
reference's own deferred-shading code under torch autograd (tests/golden/make_deferred_golden.py).

Bars: parity_util.TOL = 1e-4 relative L2 on every whole tensor (image, G-buffer gradient, each light tensor's gradient, and for
the end-to-end cases the vertex, texel and camera gradients); the expected error is fp32 rounding, 1e-7 ... 1e-6
(profiles/deferred_shade.txt has the measured maxima).  The harness cases run the same per-texel bodies as the kernels, as
plain loops; the GPU cases run on both builds of the library.

The second half of the file (test_definition_* and after) compares the kernels with an fp64 definition of the four formulas written
here, per image slice and per light row, where the adjoint's launch plan changes and where the fixtures do not reach."""
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


# ---- an independent fp64 definition of shade and adjoint, on both sides of the adjoint's capped grid -------------------------------
# The fixtures above are 20 x 24 frames with ascending, disjoint light ranges.  The cases below compare the kernels with a
# definition written here from the four formulas of include/redner_amd.h (torch double, autograd for the adjoint) where the launch
# plan changes: the capped, striding adjoint grid (deferred.h: kAdjointBlocks), the slab rows of the fold under overlapping /
# descending / empty light ranges, frames smaller than a wave, aa_samples above 3, spot exponents below 1, and a G-buffer that is
# only 8-byte aligned.  Bar: parity_util.TOL (1e-4 relative L2) per IMAGE SLICE of the image and of the G-buffer gradient and per
# LIGHT ROW of the parameter gradient (one wrong image of 64, or one wrong light, cannot hide in the norm of the whole tensor);
# where the definition is exactly zero (an unlit image, a light no image uses, an entry a light type does not use) the kernels'
# value must be exactly zero.  The CPU harness has no grid: its legs prove the definition and the bar on the per-texel bodies.
ADJOINT_BLOCKS = 2048                                  # deferred.h: kAdjointBlocks, the documented cap of the adjoint grid
USED_COLUMNS = {0: (0, 1, 2), 1: (0, 1, 2, 3, 4, 5), 2: (0, 1, 2, 6, 7, 8), 3: tuple(range(10))}
SPOT_PLANE_X = 0.25
_definition_cache = {}


def _definition_shade(g, types, params, ranges, aa, alpha):
    """g [N, H * aa, W * aa, 9 + alpha] and params [L, 10] in torch double -> [N, H, W, 3 + alpha].  One pass per light over the
    images whose range holds it.  torch.max(x, zeros) splits the gradient at a tie, as the header says.  A spot exponent below 1:
    pow(c, e) has no finite slope at c == 0, and the documented meaning (deferred.h) is the value pow(0, e)
    with gradient 0 there -- stated here with `where`, so that no inf * 0 arises."""
    n, hg, wg, _ = g.shape
    pos, nrm, alb = g[..., 0:3], g[..., 3:6], g[..., 6:9]
    rgb = torch.zeros(n, hg, wg, 3, dtype=torch.float64)
    for l, t in enumerate(types):
        sel = torch.tensor([k for k, (b, e) in enumerate(ranges) if b <= l < e], dtype=torch.long)
        if sel.numel() == 0:
            continue
        p, nn, a = pos[sel], nrm[sel], alb[sel]
        intensity = params[l, 0:3]
        if t == 0:
            rgb = rgb.index_add(0, sel, intensity * a)
            continue
        if t == 2:
            lv = (-params[l, 6:9] / params[l, 6:9].norm()).expand_as(nn)
        else:
            d = params[l, 3:6] - p
            lv = d / d.norm(dim=-1, keepdim=True)
        cos = (lv * nn).sum(-1, keepdim=True)
        c = intensity * torch.max(cos, torch.zeros_like(cos)) * (a / np.pi)
        if t == 1:
            c = c / (d * d).sum(-1, keepdim=True)
        if t == 3:
            s = -params[l, 6:9] / params[l, 6:9].norm()
            sc = (lv * s).sum(-1, keepdim=True)
            sc = torch.max(sc, torch.zeros_like(sc))
            e = params[l, 9]
            if float(e.detach()) < 1.0:
                lit = sc > 0
                f = torch.where(lit, torch.pow(torch.where(lit, sc, torch.ones_like(sc)), e),
                                torch.pow(torch.zeros_like(sc), float(e.detach())))
            else:
                f = torch.pow(sc, e)
            c = c * f
        rgb = rgb.index_add(0, sel, c)
    img = torch.cat([rgb, g[..., 9:10]], dim=-1) if alpha else rgb
    return img.reshape(n, hg // aa, aa, wg // aa, aa, img.shape[-1]).mean(dim=(2, 4))


def _off_the_kinks(g, types, params, margin=1e-5):
    """The gradient of max(x, 0) jumps at x == 0: a texel whose fp32 x is +1e-8 where the exact one is -1e-8 differs by its whole
    gradient, which says nothing about the kernel.  Texels closer than `margin` to a kink of any light WITHOUT being on it get
    albedo 0 (they then carry no gradient through the clamp); the exact ties (x == 0) stay.  -> (g, how many)"""
    gd = g.double()
    pos, nrm = gd[..., 0:3], gd[..., 3:6]
    near = torch.zeros(g.shape[:3], dtype=torch.bool)
    for t, row in zip(types, torch.from_numpy(np.asarray(params)).double()):
        if t == 0:
            continue
        if t == 2:
            lv = (-row[6:9] / row[6:9].norm()).expand_as(nrm)
        else:
            lv = (row[3:6] - pos) / (row[3:6] - pos).norm(dim=-1, keepdim=True)
        xs = [(lv * nrm).sum(-1)]
        if t == 3:
            xs.append((lv * (-row[6:9] / row[6:9].norm())).sum(-1))
        for x in xs:
            near |= (x != 0) & (x.abs() < margin)
    g = g.clone()
    g[..., 6:9] = torch.where(near[..., None], torch.zeros(()), g[..., 6:9])
    return g, int(near.sum())


def _scaled_lights(spec):
    """the light table of `spec`, every light scaled by its own factor (as test_long_light_list_gpu does): no two rows alike"""
    types, params = mk.light_table(spec)
    params = params * (1.0 + 0.001 * np.arange(len(types), dtype=np.float32))[:, None]
    return [int(t) for t in types], params.astype(np.float32)


def _cycled_ranges(n, num_lights):
    """ranges that differ from image to image: all lights, without the first, without the last, the second half"""
    kinds = [(0, num_lights), (1, num_lights), (0, num_lights - 1), (num_lights // 2, num_lights)]
    return tuple(kinds[k % 4] for k in range(n))


def _spot_case_inputs(seed, exponents):
    """Spot lights at x = SPOT_PLANE_X looking along +x (s = (-1, 0, 0) exactly): texels with p_x == SPOT_PLANE_X sit exactly on
    l.s == 0 (four columns of them, background included), those with smaller p_x are behind the spot.  Every other texel is at
    least 0.1 away from the plane in x: for e < 1 the slope of pow(c, e) grows without bound as c -> 0+, and no fp32 evaluation of c
    holds 1e-4 there."""
    g = mk.synthetic_g_buffer(seed, 1, mk.KERNEL_H, mk.KERNEL_W, 2, 0)
    dx = g[..., 0] - SPOT_PLANE_X
    g[..., 0] = torch.where(dx.abs() < 0.1, SPOT_PLANE_X + torch.where(dx < 0, dx - 0.1, dx + 0.1), g[..., 0])
    wg = g.shape[2]
    g[:, :, wg // 4: wg // 4 + 4, 0] = SPOT_PLANE_X
    spec = [(3, {'position': [SPOT_PLANE_X, 0.5 - 0.3 * k, -1.0], 'spot_direction': [2.0, 0.0, 0.0], 'spot_exponent': [e],
                 'intensity': [4.0 + k, 5.0, 6.0 - k]}) for k, e in enumerate(exponents)]
    types, params = mk.light_table(spec)
    assert int((g[..., 0] == SPOT_PLANE_X).sum()) >= 4 * g.shape[1] and int((g[..., 0] < SPOT_PLANE_X).sum()) > 100
    return g, [int(t) for t in types], params


def _build_case(name):
    """-> dict(g, types, params, ranges, aa, alpha[, capped]); `capped` only for the cases that are about the adjoint grid"""
    one_each, two_each = mk.light_sets()['one_each'], mk.light_sets()['two_each']
    kind, _, rest = name.partition('_')
    seed = 500 + sum(ord(ch) * (k + 1) for k, ch in enumerate(name)) % 1000
    if kind == 'grid':                                 # grid_<N>x<H>x<W>_<capped|uncapped>
        shape, _, side = rest.partition('_')
        n, h, w = (int(v) for v in shape.split('x'))
        types, params = _scaled_lights(one_each)
        case = dict(g=mk.synthetic_g_buffer(seed, n, h, w, 1, 1), types=types, params=params, ranges=_cycled_ranges(n, 4), aa=1,
                    alpha=1, capped=(side == 'capped'))
    elif kind == 'frame':                              # frame_<H>x<W>_aa<A>: two images, aa 1 without alpha and aa 3 with
        shape, _, aa = rest.partition('_aa')
        h, w = (int(v) for v in shape.split('x'))
        types, params = _scaled_lights(two_each)
        case = dict(g=mk.synthetic_g_buffer(seed, 2, h, w, int(aa), int(aa) == 3), types=types, params=params,
                    ranges=((0, 8), (3, 7)), aa=int(aa), alpha=int(int(aa) == 3))
    elif kind == 'aa':                                 # aa_<A>: 6 x 10 output
        types, params = _scaled_lights(two_each)
        case = dict(g=mk.synthetic_g_buffer(seed, 1, 6, 10, int(rest), 1), types=types, params=params, ranges=((0, 8),),
                    aa=int(rest), alpha=1)
    elif kind == 'ranges':                             # six lights, four images
        types, params = _scaled_lights([two_each[k] for k in (0, 2, 4, 6, 3, 7)])
        ranges = {'overlapping_descending_empty': ((2, 6), (0, 3), (3, 3), (0, 6)),        # the longest range on the LAST image
                  'longest_first': ((0, 6), (2, 6), (0, 3), (3, 3))}[rest]
        case = dict(g=mk.synthetic_g_buffer(seed, 4, mk.KERNEL_H, mk.KERNEL_W, 2, 1), types=types, params=params, ranges=ranges,
                    aa=2, alpha=1)
    else:
        assert name == 'spot_exponents'
        g, types, params = _spot_case_inputs(seed, (0.0, 0.5, 1.0, 3.0))
        case = dict(g=g, types=types, params=params, ranges=((0, 4),), aa=2, alpha=0)
    case['g'], case['moved'] = _off_the_kinks(case['g'], case['types'], case['params'])
    return case


def _definition_case(name):
    """inputs + the fp64 image and gradients, computed once and shared by the harness leg and the GPU legs of both builds"""
    if name not in _definition_cache:
        case = _build_case(name)
        g = case['g'].double().requires_grad_(True)
        params = torch.from_numpy(case['params']).double().requires_grad_(True)
        img = _definition_shade(g, case['types'], params, case['ranges'], case['aa'], case['alpha'])
        up = mk.upstream(img.shape)
        img.backward(up.double())
        case.update(up=up, want={'image': img.detach(), 'd_g_buffer': g.grad, 'd_light_params': params.grad})
        assert all(bool(torch.isfinite(v).all()) for v in case['want'].values()), name
        _definition_cache[name] = case
    return _definition_cache[name]


def _worst_slice(out, ref, what):
    """max over the slices [k] of the relative L2 error; a slice whose definition is all zero must be exactly zero"""
    o, r = out.detach().cpu().double().reshape(out.shape[0], -1), ref.reshape(ref.shape[0], -1)
    assert o.shape == r.shape and bool(torch.isfinite(o).all()), what
    rn = r.norm(dim=1)
    assert bool((o[rn == 0] == 0).all()), what + ': not exactly zero where the definition is'
    rel = (o - r).norm(dim=1)[rn > 0] / rn[rn > 0]
    return float(rel.max()) if rel.numel() else 0.0


def _run_definition_case(backend, device, name, tag):
    from redner_amd import render_utils as ru
    case = _definition_case(name)
    n, hg, wg, _ = case['g'].shape
    h, w = hg // case['aa'], wg // case['aa']
    if 'capped' in case:                               # from the documented cap: is the case on the side it is there for?
        needed, cap = (h * w + 255) // 256, max(ADJOINT_BLOCKS // n, 1)
        assert (needed > cap) == case['capped'], (name, needed, cap)
        assert needed >= cap, (name, needed, cap)      # the uncapped one sits exactly on the cap
    gl = case['g'].clone().to(device).requires_grad_(True)
    pl = torch.from_numpy(case['params']).to(device).requires_grad_(True)
    img = ru.DeferredShade.apply(gl, pl, tuple(case['types']), case['ranges'], case['aa'], bool(case['alpha']), backend)
    img.backward(case['up'].to(device))
    out = {'image': img, 'd_g_buffer': gl.grad, 'd_light_params': pl.grad}
    rep = {k: {'rel_l2': _worst_slice(out[k], case['want'][k], name + ' ' + k), 'tol': parity_util.TOL, 'flipped_rows': 0,
               'measure': 'the worst light row' if k == 'd_light_params' else 'the worst image slice'} for k in out}
    print('deferred_definition_' + name, tag, {k: '%.2e' % e['rel_l2'] for k, e in rep.items()}, 'bar %.0e;' % parity_util.TOL,
          case['moved'], 'texels taken off a kink')
    parity_util.record('deferred_definition_' + name, rep, tag)
    d_params = pl.grad.cpu()
    for l, t in enumerate(case['types']):
        unused = [k for k in range(10) if k not in USED_COLUMNS[t]]
        assert bool((d_params[l, unused] == 0).all()), (name, 'light', l, 'an entry its type does not use has a gradient')
    parity_util.assert_parity(rep, name)


GRID_CASES = ['grid_64x96x96_capped', 'grid_2049x20x24_capped', 'grid_1x512x1024_uncapped', 'grid_1x513x1024_capped']
PLAIN_CASES = ['frame_%dx%d_aa%d' % (h, w, aa) for h, w in ((1, 1), (1, 63), (1, 65), (3, 85), (1, 257)) for aa in (1, 3)] + \
    ['aa_4', 'aa_5', 'aa_7', 'ranges_overlapping_descending_empty', 'ranges_longest_first', 'spot_exponents']


@pytest.mark.parametrize('name', PLAIN_CASES)
def test_definition_hostsim(hostsim_backend, name):
    _run_definition_case(hostsim_backend, torch.device('cpu'), name, 'hostsim')


@pytest.mark.gpu
@pytest.mark.parametrize('name', GRID_CASES + PLAIN_CASES)
def test_definition_gpu(gpu_backend, name):
    _run_definition_case(gpu_backend, torch.device('cuda:0'), name, 'gpu')


def _run_spot_behind_case(backend, device):
    """One spot light with exponent 0.5: a texel on l.s == 0 or behind the spot gets NO gradient at all -- pow(0, 0.5) = 0 takes
    the light away and the documented slope of pow at 0 is 0 where the reference has inf * 0 = NaN -- and the light's parameters
    get none from it.  Exactly zero, and everything finite."""
    from redner_amd import render_utils as ru
    g, types, params = _spot_case_inputs(77, (0.5,))
    gl = g.clone().to(device).requires_grad_(True)
    pl = torch.from_numpy(params).to(device).requires_grad_(True)
    img = ru.DeferredShade.apply(gl, pl, tuple(types), ((0, 1),), 2, False, backend)
    img.backward(mk.upstream(img.shape).to(device))
    dark = g[..., 0] <= SPOT_PLANE_X
    d_g = gl.grad.cpu()
    assert bool(torch.isfinite(d_g).all()) and bool(torch.isfinite(pl.grad).all()) and bool(torch.isfinite(img).all())
    assert bool((d_g[dark] == 0).all()) and float(d_g[~dark].abs().sum()) > 0
    # with every texel on the plane or behind it the light's own gradient is exactly zero too
    g[..., 0] = torch.where(dark, g[..., 0], torch.full((), SPOT_PLANE_X))
    gl = g.clone().to(device).requires_grad_(True)
    pl = torch.from_numpy(params).to(device).requires_grad_(True)
    img = ru.DeferredShade.apply(gl, pl, tuple(types), ((0, 1),), 2, False, backend)
    img.backward(mk.upstream(img.shape).to(device))
    assert bool((img == 0).all()) and bool((gl.grad == 0).all()) and bool((pl.grad == 0).all())


def test_spot_exponent_below_one_behind_hostsim(hostsim_backend):
    _run_spot_behind_case(hostsim_backend, torch.device('cpu'))


@pytest.mark.gpu
def test_spot_exponent_below_one_behind_gpu(gpu_backend):
    _run_spot_behind_case(gpu_backend, torch.device('cuda:0'))


def _run_alignment_case(rd, device):
    """The C ABI promises 8-byte alignment of an alpha G-buffer (40-byte texels read as 8-byte pairs); the Python surface clones
    anything that is not 16-byte aligned and never gets there.  Through the raw entry points: the G-buffer and its gradient as
    views of flat tensors at an offset of 2 floats (8 mod 16), the images 16-byte aligned.  Bit for bit what the aligned call
    gives, and nothing written outside the view."""
    n, h, w, aa = 2, mk.KERNEL_H, mk.KERNEL_W, 2
    g = mk.synthetic_g_buffer(41, n, h, w, aa, 1).to(device)
    types, params = _scaled_lights(mk.light_sets()['one_each'])
    params = torch.from_numpy(params).to(device)
    up = mk.upstream((n, h, w, 4)).to(device)
    ranges, use_gpu = [(0, 4), (1, 3)], device.type == 'cuda'
    ptr = lambda t: rd.float_ptr(t.data_ptr())

    def run(offset):
        flat_g, flat_d = torch.zeros(g.numel() + 4, device=device), torch.full((g.numel() + 4,), 7.0, device=device)
        gv, dv = (f[offset: offset + g.numel()].view(g.shape) for f in (flat_g, flat_d))
        gv.copy_(g)
        assert flat_g.data_ptr() % 16 == 0 and gv.data_ptr() % 16 == dv.data_ptr() % 16 == (4 * offset) % 16
        img, d_params = torch.empty(n, h, w, 4, device=device), torch.empty_like(params)
        assert img.data_ptr() % 16 == 0 and up.data_ptr() % 16 == 0
        rd.deferred_shade(ptr(gv), ptr(params), ptr(img), n, h, w, aa, True, types, ranges, use_gpu, 0)
        rd.deferred_shade_backward(ptr(gv), ptr(params), ptr(up), ptr(dv), ptr(d_params), n, h, w, aa, True, types, ranges,
                                   use_gpu, 0)
        assert bool((flat_d[:offset] == 7.0).all()) and bool((flat_d[offset + g.numel():] == 7.0).all())
        return img.cpu(), dv.cpu().clone(), d_params.cpu()

    aligned, shifted = run(0), run(2)
    assert float(aligned[0].abs().sum()) > 0 and float(aligned[2].abs().sum()) > 0
    for a, b in zip(aligned, shifted):
        assert torch.equal(a, b)


def test_g_buffer_aligned_to_8_bytes_hostsim(hostsim_backend):
    _run_alignment_case(hostsim_backend, torch.device('cpu'))


@pytest.mark.gpu
def test_g_buffer_aligned_to_8_bytes_gpu(gpu_backend):
    _run_alignment_case(gpu_backend, torch.device('cuda:0'))
