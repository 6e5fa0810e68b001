"""SH_reconstruct and the sampling tables of an environment map (redner_amd.utils / redner_amd.texture on rdr_sh_reconstruct,
rdr_sh_reconstruct_backward, rdr_envmap_tables) against fixtures made by the reference's own pyredner.SH_reconstruct and
pyredner.EnvironmentMap (tests/golden/make_sh_golden.py), against an independent fp64 definition written here, and through
redner_amd.EnvironmentMap and RenderFunction against the oracle.

Bars
  * tables: np.array_equal / == against the reference's fixtures, and (harness) against render_pytorch.EnvironmentMap on the same
    CPU tensor.  The running sums are defined as a sequential fp64 accumulator rounded to fp32 at every output, which is what
    torch.cumsum computes on the CPU; there is no tolerance.
  * SH fixtures: parity_util.TOL = 1e-4 relative L2 of image and d_coeffs, shapes exact.  The generator asserted that no pixel's
    unclamped value is within 1e-4 S of zero, so a last-bit difference in cos cannot flip a clamp.
  * fp64 definition (_definition: closed-form associated Legendre functions by their power series, not the recurrence of the
    header), per element.  With A_i = |K_i P_i(x_r)| (the amplitude of basis function i in row r), D_i = |K_i dP_i/dx (x_r)| and
    u = 2^-24, the roundings of one term Y_i c_i of one pixel are
      - the column angle: fp32(2 pi / W), its product with c + 0.5 and the product with m are each one rounding of a number of
        size at most |m| phi, and cos / sin move by at most the error of their argument; their own result is rounded once:
        (3 |m| phi_c + 1) u A_i
      - the row angle: fp32(pi / H) and its product with r + 0.5 (2 theta_r u), through sin(theta_r) into x = cos(theta_r), which
        is rounded itself (u / 2, |x| <= 1):  (2 theta_r sin(theta_r) + 1/2) u D_i.  D_i carries the 1 / sqrt(1 - x^2) of the odd
        orders near the poles, where the reference's sqrt((1 - x)(1 + x)) on an fp32 x loses the same digits
      - the recurrence: four roundings per step, at most L steps (upward recurrence in l: errors are not amplified beyond the
        amplitude), K' * trig, * P and * c: (4 L + 3) u A_i
      - the running sum: one rounding per addition of a partial sum that is at most S_A = sum_i |c_i| A_i: N u S_A per pixel
    so |out - exact| <= u * [sum_i |c_i| ((3 |m| phi_c + 4 L + 4) A_i + (2 theta_r sin(theta_r) + 1/2) D_i) + N S_A]  (= FORWARD_BAR,
    evaluated per element in fp64).  At order 8 that is about 250 u S_A; the reference's own fp32 result was measured at up to
    37 u S (order 4, 128 x 128) and 15 u S (order 8, 64 x 128) from fp64, S = sum |Y_i| |c_i| <= S_A: the bar is not below what the
    reference achieves.  A wrong constant, sign, index or recurrence step is off by 1e-2 S or more: a thousand bars.
    d_coeffs[ch, i] = sum over pixels of Y_i g w: the same per-term bound on Y_i (without c_i and without the running sum)
    weighted by |g w|; g w is exact (w is 0, 1/2 or 1), the products and sums are fp64 (2^-53: not counted) and the result is
    rounded once: u * sum_px |g w| ((3 |m| phi + 4 L + 4) A_i + (2 theta sin(theta) + 1/2) D_i)  (= GRADIENT_BAR).  The
    reference's own gradient was measured within 1.3 u sum |Y| |g|.
  * ties: image exactly 0, d_coeffs against the reference's fixture at TOL (half of the unclamped adjoint).
  * reproducibility: d_coeffs of two calls bit for bit; the kernels' d_coeffs bit for bit what the harness computes (recorded in
    the fixture), on BOTH builds: cos and sin of the factors are the fp64 routines of csrc/libm_exact.h in either build
    (capi.cpp is compiled once), so the device's own sin / cos never enter.
  * adjoint identity: <J c, y> == <c, J^T y> to 1e-5 relative in fp64 accumulation, clamp inactive.
  * end to end: parity_util.TOL on image and coeffs.grad.
The harness cases run the same per-element bodies as the kernels, as plain loops; the GPU cases run on both builds."""
import math
import os

import numpy as np
import pytest
import torch

import parity_util
from golden import make_sh_golden as ms
from golden import make_texture_golden as mt

GOLD = parity_util.GOLD
CPU, GPU = torch.device('cpu'), torch.device('cuda:0')
U = 2.0 ** -24
_cache = {}


def _utils():
    from redner_amd import utils
    return utils


def _texture():
    from redner_amd import texture
    return texture


# ---- 1. the public names --------------------------------------------------------------------------------------------------------
def test_public_names():
    from redner_amd import SH_reconstruct, envmap_sampling_tables
    assert callable(SH_reconstruct) and callable(envmap_sampling_tables)


# ---- 2. tables, bit for bit -----------------------------------------------------------------------------------------------------
def _run_tables(backend, device, size, against_torch):
    gold = np.load(os.path.join(GOLD, 'sh_tables_%s.npz' % ms.size_tag(size)))
    for kind in ms.TABLE_KINDS:
        texels = ms.table_texels(size, kind)
        assert abs(float(texels.double().sum()) - float(gold[kind + '_sum'])) <= 1e-9 * max(1.0, float(gold[kind + '_sum']))
        ys, xs, norm = _texture().envmap_sampling_tables(texels.to(device), backend=backend)
        assert tuple(ys.shape) == (size[0],) and tuple(xs.shape) == size and ys.device.type == device.type
        assert ys.is_contiguous() and xs.is_contiguous() and isinstance(norm, float)
        assert np.array_equal(xs.cpu().numpy(), gold[kind + '_cdf_xs']), (size, kind, 'sample_cdf_xs')
        assert np.array_equal(ys.cpu().numpy(), gold[kind + '_cdf_ys']), (size, kind, 'sample_cdf_ys')
        assert norm == float(gold[kind + '_pdf_norm']), (size, kind, norm, float(gold[kind + '_pdf_norm']))
        if against_torch:
            from redner_amd import render_pytorch as rp
            env = rp.EnvironmentMap(texels)
            assert torch.equal(xs, env.sample_cdf_xs) and torch.equal(ys, env.sample_cdf_ys) and norm == env.pdf_norm


@pytest.mark.parametrize('size', ms.TABLE_SIZES, ids=ms.size_tag)
def test_tables_hostsim(hostsim_backend, size):
    _run_tables(hostsim_backend, CPU, size, True)


@pytest.mark.gpu
@pytest.mark.parametrize('size', ms.TABLE_SIZES, ids=ms.size_tag)
def test_tables_gpu(gpu_backend, size):
    _run_tables(gpu_backend, GPU, size, False)


def test_environment_map_uses_tables_hostsim(hostsim_backend):
    """redner_amd.EnvironmentMap builds its tables by envmap_sampling_tables; for a CPU tensor nothing changes."""
    import redner_amd
    from redner_amd import render_pytorch as rp
    texels = ms.table_texels((16, 32), 'hdr')
    env, old = redner_amd.EnvironmentMap(texels, backend=hostsim_backend), rp.EnvironmentMap(texels)
    assert torch.equal(env.sample_cdf_xs, old.sample_cdf_xs) and torch.equal(env.sample_cdf_ys, old.sample_cdf_ys)
    assert env.pdf_norm == old.pdf_norm


# ---- 3. SH forward and gradient against the reference's fixtures ----------------------------------------------------------------
def _native(backend, device, name):
    """(image, d_coeffs) as numpy, the leaf's gradient under the case's upstream gradient."""
    res = ms.case_shape(name)[0]
    coeffs = ms.sh_coeffs(name).to(device)
    if name in ms.SH_CASES and ms.SH_CASES[name][4]:
        wide = torch.zeros(coeffs.shape[0], 2 * coeffs.shape[1], device=device)
        wide[:, ::2] = coeffs
        coeffs = wide[:, ::2]
        assert not coeffs.is_contiguous()
    coeffs = coeffs.detach().requires_grad_(True)
    image = _utils().SH_reconstruct(coeffs, res, backend=backend)
    assert image.dtype == torch.float32 and image.device.type == device.type and image.is_contiguous()
    (image * ms.sh_upstream(name).to(device)).sum().backward()
    assert tuple(coeffs.grad.shape) == tuple(coeffs.shape)
    return image.detach().cpu().numpy(), coeffs.grad.cpu().numpy()


def _fixture(name):
    gold = dict(np.load(os.path.join(GOLD, 'sh_case_%s.npz' % name)))
    assert abs(float(ms.sh_coeffs(name).double().sum()) - float(gold.pop('coeffs_sum'))) < 1e-9, 'the regenerated input is not the fixture\'s'
    return gold


def _run_fixture(backend, device, name, tag):
    gold = _fixture(name)
    gold.pop('harness_d_coeffs', None)
    image, d_coeffs = _native(backend, device, name)
    res, n, c = ms.case_shape(name)
    assert image.shape == (res[0], res[1], c) == gold['image'].shape and d_coeffs.shape == (c, n) == gold['d_coeffs'].shape
    rep = parity_util.compare({'image': image, 'd_coeffs': d_coeffs}, gold, 'sh_case_' + name)
    print('sh_case_' + name, tag, {k: '%.2e' % e['rel_l2'] for k, e in rep.items()})
    parity_util.record('sh_case_' + name, rep, tag)
    parity_util.assert_parity(rep, name)
    bands = int(math.sqrt(n))
    assert not d_coeffs[:, bands * bands:].any(), 'the unused columns get a zero gradient'
    clamped = float((gold['image'] == 0).mean())
    if name in ('16x32_o4', '33x17_o6', '64x129_o8'):
        assert 0.1 < clamped < 0.6, ('the clamp is exercised', name, clamped)


@pytest.mark.parametrize('name', list(ms.SH_CASES))
def test_sh_fixture_hostsim(hostsim_backend, name):
    _run_fixture(hostsim_backend, CPU, name, 'hostsim')


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(ms.SH_CASES))
def test_sh_fixture_gpu(gpu_backend, name):
    _run_fixture(gpu_backend, GPU, name, 'gpu')


# ---- 4. an independent definition in fp64 ---------------------------------------------------------------------------------------
def _binom(a, k):
    """The generalised binomial coefficient C(a, k), a real, k a non-negative integer."""
    out = 1.0
    for j in range(k):
        out *= (a - j) / (j + 1.0)
    return out


def _legendre(l, m, x):
    """P_l^m(x), 0 <= m <= l, Condon-Shortley phase included, by its power series:
    (-1)^m 2^l (1 - x^2)^(m/2) sum_{k=m}^{l} k! / (k - m)! x^(k-m) C(l, k) C((l + k - 1) / 2, l)."""
    total = torch.zeros_like(x)
    for k in range(m, l + 1):
        total = total + (math.factorial(k) / math.factorial(k - m)) * _binom(l, k) * _binom((l + k - 1) / 2.0, l) * x ** (k - m)
    return (-1.0) ** m * 2.0 ** l * (1.0 - x * x) ** (m / 2.0) * total


def _definition(res, bands):
    """Per basis function i: amplitude K P [H] (fp64), its derivative by x [H], the order m, and the angles."""
    h, w = res
    theta = math.pi * (torch.arange(h, dtype=torch.float64) + 0.5) / h
    phi = 2.0 * math.pi * (torch.arange(w, dtype=torch.float64) + 0.5) / w
    x = torch.cos(theta).requires_grad_(True)
    amp, damp, orders = [], [], []
    for l in range(bands):
        for m in range(-l, l + 1):
            a = abs(m)
            k = math.sqrt((2 * l + 1) / (4 * math.pi) * math.factorial(l - a) / math.factorial(l + a)) * (1.0 if m == 0 else math.sqrt(2.0))
            p = k * _legendre(l, a, x)
            d, = torch.autograd.grad(p.sum(), x, allow_unused=True)
            amp.append(p.detach())
            damp.append(torch.zeros_like(p.detach()) if d is None else d)
            orders.append(m)
    return torch.stack(amp), torch.stack(damp), orders, theta, phi


def _reference64_of(res, coeffs, upstream):
    """The fp64 image and d_coeffs of coeffs [C, N] at `res` under the upstream gradient [H, W, C], and the two bars."""
    n, c = int(coeffs.shape[1]), int(coeffs.shape[0])
    bands = int(math.sqrt(n))
    nb = bands * bands
    amp, damp, orders, theta, phi = _definition(res, bands)
    trig = torch.stack([torch.ones_like(phi) if m == 0 else (torch.cos(m * phi) if m > 0 else torch.sin(-m * phi)) for m in orders])
    basis = amp[:, :, None] * trig[:, None, :]                                    # [nb, H, W]
    coeffs = coeffs.double()[:, :nb]                                               # [C, nb]
    unclamped = torch.einsum('ihw,ci->hwc', basis, coeffs)
    image = unclamped.clamp(min=0.0)
    weight = torch.where(unclamped > 0, 1.0, torch.where(unclamped == 0, 0.5, 0.0)).double()
    gw = upstream.double() * weight
    d_coeffs = torch.zeros(c, n, dtype=torch.float64)
    d_coeffs[:, :nb] = torch.einsum('ihw,hwc->ci', basis, gw)
    # the error of one basis function at one pixel, in units of u (without the running sum)
    m_abs = torch.tensor([abs(m) for m in orders], dtype=torch.float64)
    per_basis = (3.0 * m_abs[:, None, None] * phi[None, None, :] + 4.0 * bands + 4.0) * amp.abs()[:, :, None] + \
        ((2.0 * theta * torch.sin(theta) + 0.5)[None, :] * damp.abs())[:, :, None]  # [nb, H, W]
    s_a = torch.einsum('ih,ci->hc', amp.abs(), coeffs.abs())[:, None, :]
    forward_bar = U * (torch.einsum('ihw,ci->hwc', per_basis, coeffs.abs()) + nb * s_a)
    gradient_bar = torch.zeros(c, n, dtype=torch.float64)
    gradient_bar[:, :nb] = U * torch.einsum('ihw,hwc->ci', per_basis, gw.abs())
    s = torch.einsum('ihw,ci->hwc', basis.abs(), coeffs.abs())
    return image.numpy(), d_coeffs.numpy(), forward_bar.numpy(), gradient_bar.numpy(), s.numpy()


def _reference64(name):
    """Computed once per case and shared by the harness leg and the GPU legs: the fp64 image and d_coeffs, and the two bars."""
    if name not in _cache:
        res, n, c = ms.case_shape(name)
        assert tuple(ms.sh_coeffs(name).shape) == (c, n)
        _cache[name] = _reference64_of(res, ms.sh_coeffs(name), ms.sh_upstream(name))
    return _cache[name]


def _hold_definition(image, d_coeffs, reference, name, tag):
    """image and d_coeffs (numpy) within the per-element bars of `reference` (_reference64_of)"""
    want_image, want_grad, forward_bar, gradient_bar, s = reference
    err, gerr = np.abs(image.astype(np.float64) - want_image), np.abs(d_coeffs.astype(np.float64) - want_grad)
    worst = float((err / forward_bar).max())
    gworst = float(np.max(np.where(gradient_bar > 0, gerr / np.where(gradient_bar > 0, gradient_bar, 1.0), np.where(gerr > 0, np.inf, 0.0))))
    print('sh definition', name, tag, 'image: max error / bar = %.3f, max error = %.1f u S; d_coeffs: max error / bar = %.3f'
          % (worst, float((err / s).max()) / U, gworst))
    parity_util.record('sh_definition_' + name, {
        'image': {'rel_l2': worst, 'tol': 1.0, 'flipped_rows': 0, 'measure': 'max over the elements of |error| / FORWARD_BAR',
                  'max_error_in_u_S': float((err / s).max()) / U},
        'd_coeffs': {'rel_l2': gworst, 'tol': 1.0, 'flipped_rows': 0, 'measure': 'max over the entries of |error| / GRADIENT_BAR'}}, tag)
    assert worst <= 1.0, (name, worst)
    assert gworst <= 1.0, (name, gworst)


DEFINITION_CASES = ['1x7_o2', '5x3_o3', '16x32_o4', '33x17_o6', '64x129_o8', '33x17_o3_c5', '16x32_n17']


def _run_definition(backend, device, name, tag):
    image, d_coeffs = _native(backend, device, name)
    _hold_definition(image, d_coeffs, _reference64(name), name, tag)


@pytest.mark.parametrize('name', DEFINITION_CASES)
def test_sh_definition_hostsim(hostsim_backend, name):
    _run_definition(hostsim_backend, CPU, name, 'hostsim')


@pytest.mark.gpu
@pytest.mark.parametrize('name', DEFINITION_CASES)
def test_sh_definition_gpu(gpu_backend, name):
    _run_definition(gpu_backend, GPU, name, 'gpu')


# ---- 5. ties --------------------------------------------------------------------------------------------------------------------
def _run_ties(backend, device, tag):
    gold = _fixture(ms.TIES)
    image, d_coeffs = _native(backend, device, ms.TIES)
    assert image.shape == (5, 3, 3) and not image.any() and not gold['image'].any()
    assert float(np.abs(gold['d_coeffs']).sum()) > 0
    rep = parity_util.compare({'d_coeffs': d_coeffs}, {'d_coeffs': gold['d_coeffs']}, 'sh_case_ties')
    parity_util.record('sh_case_ties', rep, tag)
    parity_util.assert_parity(rep, 'ties')


def test_sh_ties_hostsim(hostsim_backend):
    _run_ties(hostsim_backend, CPU, 'hostsim')


@pytest.mark.gpu
def test_sh_ties_gpu(gpu_backend):
    _run_ties(gpu_backend, GPU, 'gpu')


# ---- 6. bitwise reproducible, and the same bits as the harness ------------------------------------------------------------------
def _run_bitwise(backend, device, name):
    first, second = _native(backend, device, name), _native(backend, device, name)
    assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()
    assert first[1].tobytes() == _fixture(name)['harness_d_coeffs'].tobytes(), 'not the bits the harness computes'


@pytest.mark.parametrize('name', ms.BITWISE_CASES)
def test_sh_bitwise_hostsim(hostsim_backend, name):
    _run_bitwise(hostsim_backend, CPU, name)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ms.BITWISE_CASES)
def test_sh_bitwise_gpu(gpu_backend, name):
    """Both builds: the tile order is the same as the harness's, and cos / sin are csrc/libm_exact.h's in either build."""
    _run_bitwise(gpu_backend, GPU, name)


# ---- 7. adjoint identity --------------------------------------------------------------------------------------------------------
def _run_adjoint_identity(backend, device, res, n):
    gen = torch.Generator().manual_seed(res[0] + n)
    coeffs = 0.05 * torch.randn(3, n, generator=gen)
    coeffs[:, 0] += 4.0                                # Y_0 = 0.28: the sum stays above 1 - 0.05 * sum |Y_i| > 0, the clamp is inactive
    coeffs = coeffs.to(device).requires_grad_(True)
    y = torch.randn(res[0], res[1], 3, generator=gen).to(device)
    image = _utils().SH_reconstruct(coeffs, res, backend=backend)
    assert float(image.detach().min()) > 0
    (image * y).sum().backward()
    lhs = float((image.detach().double() * y.double()).sum())
    rhs = float((coeffs.detach().double() * coeffs.grad.double()).sum())
    print('sh adjoint identity', res, n, lhs, rhs)
    assert lhs != 0.0 and abs(lhs - rhs) <= 1e-5 * abs(lhs), (res, n, lhs, rhs)


ADJOINT_CASES = [((1, 7), 4), ((5, 3), 9), ((16, 32), 16), ((33, 17), 36), ((64, 129), 64)]


@pytest.mark.parametrize('res,n', ADJOINT_CASES)
def test_sh_adjoint_identity_hostsim(hostsim_backend, res, n):
    _run_adjoint_identity(hostsim_backend, CPU, res, n)


@pytest.mark.gpu
@pytest.mark.parametrize('res,n', ADJOINT_CASES)
def test_sh_adjoint_identity_gpu(gpu_backend, res, n):
    _run_adjoint_identity(gpu_backend, GPU, res, n)


# ---- 8. end to end --------------------------------------------------------------------------------------------------------------
def _run_e2e(backend, device, tag):
    import redner_amd
    coeffs = ms.e2e_coeffs().to(device).requires_grad_(True)
    values = _utils().SH_reconstruct(coeffs, ms.E2E_RES, backend=backend)
    sc = mt.envmap_scene(device, lambda v, e2w: redner_amd.EnvironmentMap(v, env_to_world=e2w, backend=backend), values)
    assert isinstance(sc.envmap.values, redner_amd.Texture) and len(sc.envmap.values.mipmap) == 6
    img = mt.render_e2e(sc, 'envmap', [backend.channels.radiance], device, backend)
    assert tuple(coeffs.grad.shape) == (3, ms.E2E_COEFFS)
    out = {'image': img.detach().cpu().numpy(), 'grad_coeffs': coeffs.grad.cpu().numpy()}
    rep = parity_util.compare(out, np.load(os.path.join(GOLD, 'sh_e2e.npz')), 'sh_e2e')
    print('sh_e2e', tag, {k: '%.2e' % e['rel_l2'] for k, e in rep.items()})
    parity_util.record('sh_e2e', rep, tag)
    parity_util.assert_parity(rep, 'sh_e2e')


def test_sh_e2e_hostsim(hostsim_backend):
    _run_e2e(hostsim_backend, CPU, 'hostsim')


@pytest.mark.gpu
def test_sh_e2e_gpu(gpu_backend):
    _run_e2e(gpu_backend, GPU, 'gpu')


# ---- 9. errors ------------------------------------------------------------------------------------------------------------------
def _run_errors(backend, device):
    sh, tables = _utils().SH_reconstruct, _texture().envmap_sampling_tables
    with pytest.raises((RuntimeError, ValueError), match='SH_reconstruct'):
        sh(torch.zeros(3, 81, device=device), (8, 8), backend=backend)                    # 9 bands
    with pytest.raises((RuntimeError, ValueError), match='SH_reconstruct'):
        sh(torch.zeros(16, device=device), (8, 8), backend=backend)
    with pytest.raises((RuntimeError, ValueError), match='SH_reconstruct'):
        sh(torch.zeros(3, 16, dtype=torch.float64, device=device), (8, 8), backend=backend)
    for res in [(0, 8), (8, -1)]:
        with pytest.raises((RuntimeError, ValueError), match='SH_reconstruct'):
            sh(torch.zeros(3, 16, device=device), res, backend=backend)
    for shape in [(4, 4), (4, 4, 1), (4, 4, 4)]:
        with pytest.raises((RuntimeError, ValueError), match='envmap_sampling_tables'):
            tables(torch.ones(*shape, device=device), backend=backend)
    assert tuple(sh(torch.zeros(3, 80, device=device), (2, 2), backend=backend).shape) == (2, 2, 3)      # 8 bands, 16 unused columns


def test_errors_hostsim(hostsim_backend):
    _run_errors(hostsim_backend, CPU)
    from redner_amd import _capi
    lib = _capi.lib()
    assert lib.rdr_sh_backward_scratch(64, 129, 3, 64) == 2 * 2 * 5 * 3 * 64
    assert lib.rdr_sh_backward_scratch(8, 8, 3, 81) == -1 and 'rdr_sh_backward_scratch' in _capi.last_error()
    a = torch.zeros(4, 4, 3)
    assert lib.rdr_sh_reconstruct(None, 3, 16, 4, 4, a.data_ptr(), None, -1) != 0 and 'rdr_sh_reconstruct' in _capi.last_error()
    assert lib.rdr_envmap_tables(a.data_ptr(), None, 4, 4, None, None, None, -1) != 0 and 'rdr_envmap_tables' in _capi.last_error()


@pytest.mark.gpu
def test_errors_gpu(gpu_backend):
    _run_errors(gpu_backend, GPU)
    # no torch fall-back and no silent CPU path: CPU tensors are for the harness library only
    with pytest.raises(RuntimeError, match='SH_reconstruct.*harness'):
        _utils().SH_reconstruct(torch.zeros(3, 16), (8, 8), backend=gpu_backend)
    with pytest.raises(RuntimeError, match='envmap_sampling_tables.*harness'):
        _texture().envmap_sampling_tables(torch.ones(4, 4, 3), backend=gpu_backend)


@pytest.mark.gpu
def test_readme_snippet_gpu(gpu_backend):
    """The loop step of the README: coefficients -> environment map -> coefficient gradient, on the device."""
    from redner_amd import EnvironmentMap, SH_reconstruct
    coeffs = torch.zeros(3, 16, device=GPU)
    coeffs[:, 0] = 0.5
    coeffs.requires_grad_(True)
    env = EnvironmentMap(SH_reconstruct(coeffs, (128, 128), backend=gpu_backend), backend=gpu_backend)
    assert tuple(env.values.mipmap[0].shape) == (128, 128, 3) and tuple(env.sample_cdf_xs.shape) == (128, 128)
    sum(l.sum() for l in env.values.mipmap).backward()
    assert tuple(coeffs.grad.shape) == (3, 16) and float(coeffs.grad[:, 0].min()) > 0
