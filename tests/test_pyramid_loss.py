"""gaussian_pyramid_loss (redner_amd.loss on rdr_pyramid_loss / rdr_pyramid_loss_backward, csrc/pyramid_loss.h) against fixtures
made by the torch formulation the reference's scripts write (tests/golden/make_pyramid_loss_golden.py), against an independent
fp64 definition written here, and through RenderFunction against the same render driven by the torch formulation's gradient.

Bars
  * fixtures: loss and every term at 1e-6 relative, the gradient at parity_util.TOL = 1e-4 relative L2; shape, dtype and device
    exact.
  * fp64 definition (_down / _up below: numpy, the separable 7-tap filter with zero padding, then the 2 x 2 mean), per element,
    one level step at a time: level l + 1 of the kernels against the definition applied to the kernels' own level l (level 0 is
    one IEEE subtraction and a clamp, formed here in fp32).  With u = 2^-24 and beta_t = (a_t + a_{t-1}) / 2 the exact folded tap,
    the header's order puts on the path of one term beta_i beta_j D[r, c] of one coarse texel
        b_j = fp32(beta_j) and b_i = fp32(beta_i)          2 roundings
        b_j * D                                             1
        the row's sum of eight                              8 additions at most (the first adds to 0.f)
        b_i * row                                           1
        the sum of the eight rows                           8
    K_DOWN = 20 roundings, so |D_{l+1} - exact| <= 20 u sum |beta_i beta_j D| (the second-order terms are 1e-6 of that).  The
    generator asserted that the torch formulation's own fp32 levels lie within the same bar (at most 0.21 of it), and that a plain
    truncated filter, wrapped padding and a swapped odd-side rule each exceed it.
    The terms are fp64 sums of exact squares: 1e-12 relative against numpy's sum of the kernels' own levels; the loss is their
    sum rounded once: u relative.
    The gradient, from the kernels' own levels taken as exact: acc_l = fl(fl(c_l D_l) + up) has 3 roundings on the direct term
    (c_l, the product, the addition); a gathered term passes two taps, two products, at most 4 + 4 additions and that final
    addition: 13 per level it descends; the product with upstream is 1 more.  The longest path has 13 (L - 1) + 4 roundings;
    k_grad = 14 (L - 1) + 5 bounds it with the second-order terms, and the bar is k_grad u absacc_0 with
    absacc_l = |c_l D_l| + A^T absacc_{l+1}.  Where the clamp does not pass the gradient is exactly 0.  The generator asserted
    that torch's own image.grad lies within that bar of the definition on its own levels (at most 0.21 of it).
  * reproducibility: two calls give the same bits, loss and gradient; loss, terms and the gradient's digest are the harness's
    recorded in the fixture, on both builds.
  * adjoint identity: <A^T A x, y> == <A x, A y> to 1e-5 relative, fp64 accumulation, per level.
  * clamp ties: at D = +-c the gradient is bit for bit the one of the unclamped op on the clamped difference; beyond, exactly 0.
The harness cases run the same per-texel bodies as the kernels, as plain loops; the GPU cases run on both builds."""
import hashlib
import os

import numpy as np
import pytest
import torch

import parity_util
from golden import make_pyramid_loss_golden as mp
from redner_amd import gaussian_pyramid_loss, GaussianPyramidLoss

CPU, GPU = torch.device('cpu'), torch.device('cuda:0')
U = 2.0 ** -24
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _loss_module():
    from redner_amd import loss
    return loss


# ---- the fp64 definition --------------------------------------------------------------------------------------------------------
def _blur(x, a, axis):
    """the 7 taps along `axis` of x [N, H, W, C], zero padding of 3"""
    x = np.moveaxis(x, axis, 0)
    p = np.zeros((x.shape[0] + 6,) + x.shape[1:])
    p[3:-3] = x
    out = np.zeros(x.shape)
    for t in range(7):
        out += float(a[t]) * p[t:t + x.shape[0]]
    return np.moveaxis(out, 0, axis)


def _down(d, a):
    n, h, w, c = d.shape
    g = _blur(_blur(d, a, 1), a, 2)[:, :2 * (h // 2), :2 * (w // 2)]
    return g.reshape(n, h // 2, 2, w // 2, 2, c).mean(axis=(2, 4))


def _up(acc, shape, a):
    g = np.zeros(shape)
    h, w = acc.shape[1], acc.shape[2]
    g[:, :2 * h, :2 * w] = 0.25 * np.repeat(np.repeat(acc, 2, axis=1), 2, axis=2)
    return _blur(_blur(g, a, 2), a, 1)


def _counts(shape, num_levels):
    return [(shape[1] / 2 ** l) * (shape[2] / 2 ** l) for l in range(num_levels)]


def _gradient(levels, weights, a):
    cnt = _counts(levels[0].shape, len(levels))
    acc = absacc = None
    for l in range(len(levels) - 1, -1, -1):
        direct = (2.0 * weights[l] / cnt[l]) * levels[l]
        if acc is None:
            acc, absacc = direct, np.abs(direct)
        else:
            acc, absacc = direct + _up(acc, levels[l].shape, a), np.abs(direct) + _up(absacc, levels[l].shape, a)
    return acc, absacc


# ---- running the op -------------------------------------------------------------------------------------------------------------
def _native(backend, device, image, target, num_levels, clamp, weights, levels=False):
    x = image.detach().clone().to(device).requires_grad_(True)
    t = target.to(device)
    loss, terms = gaussian_pyramid_loss(x, t, num_levels, clamp=clamp, weights=weights, return_terms=True, backend=backend)
    assert loss.shape == () and loss.dtype == torch.float32 and loss.device.type == device.type
    assert terms.shape == (num_levels,) and terms.dtype == torch.float64 and not terms.requires_grad
    loss.backward()
    assert x.grad.shape == x.shape and x.grad.dtype == torch.float32 and x.grad.device.type == device.type
    out = {'loss': loss.detach().cpu().numpy(), 'terms': terms.cpu().numpy(), 'grad': x.grad.cpu().numpy()}
    if levels:
        out['levels'] = [v.cpu().numpy() for v in _loss_module().pyramid_levels(x, t, num_levels, clamp=clamp, backend=backend)]
    return out


def _case(backend, device, name, levels=False):
    _, num_levels, clamp, weights = mp.CASES[name]
    image, target = mp.inputs(name)
    return _native(backend, device, image, target, num_levels, clamp, weights, levels)


def _fixture(name):
    gold = dict(np.load(mp.fixture_path(name)))
    assert abs(mp.inputs_sum(name) - float(gold['inputs_sum'])) < 1e-9, 'the regenerated inputs are not the fixture\'s'
    return gold


def _rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


# ---- 1. the public names --------------------------------------------------------------------------------------------------------
def test_public_names():
    import redner_amd
    mod = _loss_module()
    assert redner_amd.gaussian_pyramid_loss is mod.gaussian_pyramid_loss and redner_amd.GaussianPyramidLoss is mod.GaussianPyramidLoss
    assert issubclass(GaussianPyramidLoss, torch.autograd.Function)


def test_taps_are_the_committed_scipy_table():
    table = np.load(mp.TABLE_PATH)
    a = mp.taps().astype(np.float64)
    assert table.shape == (7, 7) and table.dtype == np.float32
    assert np.max(np.abs(table.astype(np.float64) - np.outer(a, a))) <= 3 * U * table.max()
    plain = mp.taps(truncated=True).astype(np.float64)
    assert abs(plain[0] / a[0] - 1.0) > 0.02            # the plain truncated filter is another one


# ---- 2. against the torch formulation's fixtures --------------------------------------------------------------------------------
def _run_fixture(backend, device, name, tag):
    gold, out = _fixture(name), _case(backend, device, name)
    shape = mp.CASES[name][0]
    assert out['grad'].shape == tuple(shape)
    e_loss = abs(float(out['loss']) - float(gold['loss'])) / abs(float(gold['loss']))
    e_terms = np.abs(out['terms'] - gold['terms']) / np.maximum(np.abs(gold['terms']), 1e-300)
    e_grad = _rel_l2(out['grad'], gold['grad'])
    print('%s %s: loss %.3e terms %.3e grad %.3e' % (tag, name, e_loss, float(e_terms.max()), e_grad))
    assert e_loss <= 1e-6 and np.all(e_terms <= 1e-6), (name, e_loss, e_terms)
    assert e_grad < parity_util.TOL, (name, e_grad)


@pytest.mark.parametrize('name', list(mp.CASES))
def test_fixture_hostsim(hostsim_backend, name):
    _run_fixture(hostsim_backend, CPU, name, 'hostsim')


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(mp.CASES))
def test_fixture_gpu(gpu_backend, name):
    _run_fixture(gpu_backend, GPU, name, 'gpu')


# ---- 3. against the fp64 definition, per element --------------------------------------------------------------------------------
def _check_definition(out, image, target, num_levels, clamp, weights, tag):
    a = mp.taps()
    weights = weights or (1.0,) * num_levels
    d0, mask = mp.diff32(image.numpy(), target.numpy(), clamp)
    batched = (lambda v: v if v.ndim == 4 else v[None])
    levels = [batched(d0).astype(np.float64)] + [v.astype(np.float64) for v in out['levels']]
    assert len(levels) == num_levels
    worst = 0.0
    for l in range(1, num_levels):
        want, bar = _down(levels[l - 1], a), mp.K_DOWN * U * _down(np.abs(levels[l - 1]), a)
        assert levels[l].shape == want.shape, (tag, l, levels[l].shape, want.shape)
        ratio = np.abs(levels[l] - want) / np.maximum(bar, 1e-300)
        worst = max(worst, float(ratio.max()))
        assert np.all(np.abs(levels[l] - want) <= bar), (tag, 'level', l, float(ratio.max()))
    cnt = _counts(levels[0].shape, num_levels)
    terms = np.array([weights[l] * float((levels[l] ** 2).sum()) / cnt[l] for l in range(num_levels)])
    assert np.all(np.abs(out['terms'] - terms) <= 1e-12 * np.abs(terms)), (tag, out['terms'], terms)
    assert abs(float(out['loss']) - out['terms'].sum()) <= U * abs(out['terms'].sum()), (tag, out['loss'], out['terms'].sum())
    acc, absacc = _gradient(levels, weights, a)
    grad, mask = batched(out['grad']).astype(np.float64), batched(mask)
    bar = mp.k_grad(num_levels) * U * absacc
    assert np.all(grad[~mask] == 0.0), (tag, 'gradient where the clamp does not pass')
    ratio = float((np.abs(grad - acc)[mask] / np.maximum(bar[mask], 1e-300)).max())
    print('%s: worst level error / bar %.3f, gradient %.3f' % (tag, worst, ratio))
    assert np.all(np.abs(grad - acc)[mask] <= bar[mask]), (tag, 'gradient', ratio)


def _run_definition(backend, device, name, tag):
    _, num_levels, clamp, weights = mp.CASES[name]
    image, target = mp.inputs(name)
    _check_definition(_case(backend, device, name, levels=True), image, target, num_levels, clamp, weights, '%s %s' % (tag, name))


@pytest.mark.parametrize('name', list(mp.CASES))
def test_definition_hostsim(hostsim_backend, name):
    _run_definition(hostsim_backend, CPU, name, 'hostsim')


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(mp.CASES))
def test_definition_gpu(gpu_backend, name):
    _run_definition(gpu_backend, GPU, name, 'gpu')


# one shape on each side of every switch of the launch plan, found through the plan query: the first height at which level 1 of
# an H x 128 x 3 image goes to the tiled kernel (with two levels: whether there is a chain workgroup at all; with three: where
# it starts), and the step from one chunk of channels to two
def _switch_shapes(backend):
    shapes = []
    for num_levels in (2, 3):
        tiled = [backend.pyramid_loss_plan(1, h, 128, 3, num_levels)[0] for h in range(100, 200)]
        step = [i for i in range(1, len(tiled)) if tiled[i] != tiled[i - 1]]
        assert len(step) == 1 and tiled[step[0] - 1] == 1 and tiled[step[0]] == 2, tiled
        small = backend.pyramid_loss_plan(1, 100 + step[0], 128, 3, num_levels)[1]
        assert ((100 + step[0] - 1) // 2) * 64 * 3 <= small < ((100 + step[0]) // 2) * 64 * 3
        shapes += [((100 + step[0] - 1, 128, 3), num_levels), ((100 + step[0], 128, 3), num_levels)]
    return shapes + [((12, 10, 4), 2), ((12, 10, 5), 2), ((9, 11, 9), 2)]


def _run_switches(backend, device, tag):
    for shape, num_levels in _switch_shapes(backend):
        gen = torch.Generator().manual_seed(shape[0] * 1000 + shape[2] + num_levels)
        image, target = torch.rand(*shape, generator=gen), torch.rand(*shape, generator=gen)
        out = _native(backend, device, image, target, num_levels, None, None, levels=True)
        _check_definition(out, image, target, num_levels, None, None, '%s %s L%d' % (tag, shape, num_levels))


def test_plan_switches_hostsim(hostsim_backend):
    _run_switches(hostsim_backend, CPU, 'hostsim')


@pytest.mark.gpu
def test_plan_switches_gpu(gpu_backend):
    _run_switches(gpu_backend, GPU, 'gpu')


# ---- 4. bitwise reproducible, and the same bits as the harness -------------------------------------------------------------------
def _run_bitwise(backend, device, name):
    gold, first, second = _fixture(name), _case(backend, device, name), _case(backend, device, name)
    for key in ('loss', 'terms', 'grad'):
        assert first[key].tobytes() == second[key].tobytes(), (name, key, 'two calls differ')
    assert first['loss'].tobytes() == gold['harness_loss'].tobytes(), (name, first['loss'], gold['harness_loss'])
    assert first['terms'].tobytes() == gold['harness_terms'].tobytes(), (name, first['terms'], gold['harness_terms'])
    digest = np.frombuffer(hashlib.sha256(first['grad'].tobytes()).digest(), dtype=np.uint8)
    assert np.array_equal(digest, gold['harness_grad_sha256']), (name, 'not the gradient bits the harness computes')


@pytest.mark.parametrize('name', list(mp.CASES))
def test_bitwise_hostsim(hostsim_backend, name):
    _run_bitwise(hostsim_backend, CPU, name)


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(mp.CASES))
def test_bitwise_gpu(gpu_backend, name):
    """Both builds: tiles, rows and levels are added in the harness's order, and no transcendental function enters."""
    _run_bitwise(gpu_backend, GPU, name)


# ---- 5. the adjoint identity ----------------------------------------------------------------------------------------------------
def _run_adjoint_identity(backend, device):
    shape, num_levels = (70, 38, 4), 4
    gen = torch.Generator().manual_seed(31)
    x, y, zero = torch.randn(*shape, generator=gen), torch.randn(*shape, generator=gen), torch.zeros(*shape)
    levels = _loss_module().pyramid_levels
    ax = [x[None]] + levels(x.to(device), zero.to(device), num_levels, backend=backend)
    ay = [y[None]] + levels(y.to(device), zero.to(device), num_levels, backend=backend)
    cnt = _counts((1,) + shape, num_levels)
    for l in range(num_levels):
        weights = [1.0 if k == l else 0.0 for k in range(num_levels)]
        g = _native(backend, device, x, zero, num_levels, None, weights)['grad'].astype(np.float64)      # (2 / N_l) A^T A x
        lhs = float((g * y.numpy().astype(np.float64)).sum())
        axl, ayl = ax[l].cpu().numpy().astype(np.float64), ay[l].cpu().numpy().astype(np.float64)
        rhs = 2.0 / cnt[l] * float((axl * ayl).sum())
        scale = 2.0 / cnt[l] * float(np.linalg.norm(axl) * np.linalg.norm(ayl))
        print('adjoint level %d: %.9e vs %.9e (scale %.3e)' % (l, lhs, rhs, scale))
        assert abs(lhs - rhs) <= 1e-5 * scale, (l, lhs, rhs, scale)


def test_adjoint_identity_hostsim(hostsim_backend):
    _run_adjoint_identity(hostsim_backend, CPU)


@pytest.mark.gpu
def test_adjoint_identity_gpu(gpu_backend):
    _run_adjoint_identity(gpu_backend, GPU)


# ---- 6. the clamp's ties --------------------------------------------------------------------------------------------------------
def _run_clamp_ties(backend, device):
    name = '33x33x3_L3_clamp1'
    _, num_levels, clamp, _ = mp.CASES[name]
    image, target = mp.inputs(name)
    raw = image.numpy() - target.numpy()
    ties, beyond = np.abs(raw) == clamp, np.abs(raw) > clamp
    assert ties.sum() >= 100 and (raw == clamp).any() and (raw == -clamp).any() and beyond.sum() >= 100
    clamped = _native(backend, device, image, target, num_levels, clamp, None)['grad']
    # the unclamped op on the clamped difference itself (D - 0 is exact): the same D_0, every element passes
    d0 = torch.from_numpy(np.clip(raw, -clamp, clamp))
    free = _native(backend, device, d0, torch.zeros_like(d0), num_levels, None, None)['grad']
    assert np.all(clamped[beyond] == 0.0)
    assert clamped[ties].tobytes() == free[ties].tobytes() and np.count_nonzero(clamped[ties]) > 0
    assert clamped[~beyond].tobytes() == free[~beyond].tobytes()


def test_clamp_ties_hostsim(hostsim_backend):
    _run_clamp_ties(hostsim_backend, CPU)


@pytest.mark.gpu
def test_clamp_ties_gpu(gpu_backend):
    _run_clamp_ties(gpu_backend, GPU)


def test_gradient_to_target_and_upstream_hostsim(hostsim_backend):
    image, target = mp.inputs('5x9x3_L3')
    x, t = image.clone().requires_grad_(True), target.clone().requires_grad_(True)
    (3.0 * gaussian_pyramid_loss(x, t, 3, backend=hostsim_backend)).backward()
    y = image.clone().requires_grad_(True)
    gaussian_pyramid_loss(y, target, 3, backend=hostsim_backend).backward()
    assert torch.equal(t.grad, -x.grad) and torch.equal(x.grad, 3.0 * y.grad)
    only = target.clone().requires_grad_(True)
    gaussian_pyramid_loss(image, only, 3, backend=hostsim_backend).backward()
    assert torch.equal(only.grad, -y.grad)


# ---- 7. errors ------------------------------------------------------------------------------------------------------------------
def _run_errors(backend, device):
    ok = torch.zeros(8, 8, 3, device=device)
    for kwargs in (dict(num_levels=5), dict(num_levels=0), dict(num_levels=2, weights=[1.0]), dict(num_levels=2, clamp=0.0),
                   dict(num_levels=2, clamp=-1.0)):
        with pytest.raises(ValueError):
            gaussian_pyramid_loss(ok, ok, backend=backend, **kwargs)
    with pytest.raises(ValueError):
        gaussian_pyramid_loss(ok, torch.zeros(8, 9, 3, device=device), 2, backend=backend)
    with pytest.raises(ValueError):
        gaussian_pyramid_loss(ok.double(), ok.double(), 2, backend=backend)
    with pytest.raises(ValueError):
        gaussian_pyramid_loss(torch.zeros(8, 8, device=device), torch.zeros(8, 8, device=device), 2, backend=backend)
    assert float(gaussian_pyramid_loss(ok, ok, 4, backend=backend)) == 0.0                       # 8 >> 3 == 1: the last level allowed
    # the C calls, through rdr_last_error
    rd, use_gpu = backend, device.type == 'cuda'
    fwd, bwd = rd.pyramid_loss_scratch(1, 8, 8, 3, 3)
    assert fwd > 0 and bwd > 0
    scratch = torch.zeros(fwd, dtype=torch.float64, device=device)
    loss = torch.zeros((), device=device)
    ptr = (lambda t: rd.float_ptr(t.data_ptr()))
    with pytest.raises(RuntimeError, match='too many levels'):
        rd.pyramid_loss_scratch(1, 8, 8, 3, 5)
    with pytest.raises(RuntimeError, match='too many levels'):
        rd.pyramid_loss(ptr(ok), ptr(ok), ptr(loss), None, ptr(scratch), fwd, 1, 8, 8, 3, 17, None, 0.0, use_gpu, 0)
    with pytest.raises(RuntimeError, match='required'):
        rd.pyramid_loss(None, ptr(ok), ptr(loss), None, ptr(scratch), fwd, 1, 8, 8, 3, 3, None, 0.0, use_gpu, 0)
    with pytest.raises(RuntimeError, match='required'):
        rd.pyramid_loss(ptr(ok), ptr(ok), None, None, ptr(scratch), fwd, 1, 8, 8, 3, 3, None, 0.0, use_gpu, 0)
    with pytest.raises(RuntimeError, match='scratch of %d floats' % fwd):
        rd.pyramid_loss(ptr(ok), ptr(ok), ptr(loss), None, ptr(scratch), fwd - 1, 1, 8, 8, 3, 3, None, 0.0, use_gpu, 0)
    with pytest.raises(RuntimeError, match='scratch of %d floats' % fwd):
        rd.pyramid_loss(ptr(ok), ptr(ok), ptr(loss), None, None, fwd, 1, 8, 8, 3, 3, None, 0.0, use_gpu, 0)
    with pytest.raises(RuntimeError, match='clamp'):
        rd.pyramid_loss(ptr(ok), ptr(ok), ptr(loss), None, ptr(scratch), fwd, 1, 8, 8, 3, 3, None, -1.0, use_gpu, 0)
    rd.pyramid_loss(ptr(ok), ptr(ok), ptr(loss), None, ptr(scratch), fwd, 1, 8, 8, 3, 3, None, 0.0, use_gpu, 0)
    grad, acc = torch.zeros_like(ok), torch.zeros(bwd, device=device)
    one = torch.ones((), device=device)
    back = (lambda **kw: rd.pyramid_loss_backward(
        kw.get('image', ptr(ok)), ptr(ok), kw.get('saved', ptr(scratch)), kw.get('saved_floats', 2 * fwd), kw.get('upstream', ptr(one)),
        kw.get('d_image', ptr(grad)), None, ptr(acc), kw.get('scratch_floats', bwd), 1, 8, 8, 3, 3, None, 0.0, use_gpu, 0))
    for bad in (dict(image=None), dict(upstream=None), dict(d_image=None)):
        with pytest.raises(RuntimeError, match='required'):
            back(**bad)
    with pytest.raises(RuntimeError, match='saved must hold'):
        back(saved=None)
    with pytest.raises(RuntimeError, match='saved must hold'):
        back(saved_floats=bwd - 1)
    with pytest.raises(RuntimeError, match='scratch of %d floats' % bwd):
        back(scratch_floats=bwd - 1)
    back()
    if use_gpu:
        torch.cuda.synchronize()
    assert float(loss) == 0.0 and not grad.any()


def test_errors_hostsim(hostsim_backend):
    _run_errors(hostsim_backend, CPU)


@pytest.mark.gpu
def test_errors_gpu(gpu_backend):
    _run_errors(gpu_backend, GPU)
    # no torch fall-back and no silent CPU path: CPU tensors are for the harness library only
    with pytest.raises(RuntimeError, match='gaussian_pyramid_loss.*harness'):
        gaussian_pyramid_loss(torch.zeros(8, 8, 3), torch.zeros(8, 8, 3), 2, backend=gpu_backend)


# ---- 9. end to end: a render, the loss, the vertex gradient ----------------------------------------------------------------------
@pytest.mark.gpu
def test_end_to_end_gpu(gpu_backend):
    """single_triangle at 64 x 64 and 4 spp through RenderFunction, gaussian_pyramid_loss with three levels against a fixed target,
    backward; against the same render driven by the d_image of the torch formulation, which is computed on the CPU from the
    rendered image (no convolution runs on the device here)."""
    import scenes
    from redner_amd.render_pytorch import RenderFunction

    def render():
        sc = scenes.single_triangle(GPU, resolution=(64, 64))
        args = RenderFunction.serialize_scene(sc, 4, 1, sampler_type=gpu_backend.SamplerType.sobol, device=GPU)
        return sc, RenderFunction.apply(1, *args)

    yy, xx = torch.meshgrid(torch.arange(64, dtype=torch.float32), torch.arange(64, dtype=torch.float32), indexing='ij')
    target = torch.stack([0.5 + 0.3 * torch.sin(0.21 * xx), 0.4 + 0.2 * torch.cos(0.17 * yy), 0.3 + 0.1 * torch.sin(0.13 * (xx + yy))], dim=2)
    sc, img = render()
    assert tuple(img.shape) == (64, 64, 3)
    loss = gaussian_pyramid_loss(img, target.to(GPU), 3, backend=gpu_backend)
    loss.backward()
    got = sc.shapes[0].vertices.grad.cpu().numpy()
    sc2, img2 = render()
    x = img2.detach().cpu().requires_grad_(True)
    want_loss, _ = mp.torch_formulation(x, target, 3, None, None, np.load(mp.TABLE_PATH))
    want_loss.backward()
    img2.backward(x.grad.to(GPU))
    want = sc2.shapes[0].vertices.grad.cpu().numpy()
    e = _rel_l2(got, want)
    print('end to end: loss %.9g vs %.9g, vertex gradient rel-L2 %.3e' % (float(loss), float(want_loss), e))
    assert abs(float(loss) - float(want_loss)) <= 1e-6 * abs(float(want_loss))
    assert np.linalg.norm(want) > 0 and e < parity_util.TOL, e
