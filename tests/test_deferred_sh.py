"""SHLight: a spherical-harmonic environment light in the deferred pass (rows RDR_DL_SH_R / _G / _B of the light table;
redner_amd.render_utils.SHLight).  The reference has no such light: the oracle is the fp64 definition written here from the formula
of include/redner_amd.h (torch double, autograd for the adjoint), next to test_deferred's definition of the four other lights.

What the cases are held to:
  * values and gradients against the definition at parity_util.TOL (1e-4 relative L2, the bar of test_deferred.py) on the worst
    image slice, the worst G-buffer-gradient slice and the worst light row, on mixed tables (two SH lights among one light of
    each other type), on frames below a wave, across a wave, across a block and over two blocks, and (GPU) with the adjoint grid
    exactly on its cap and just over it;
  * the tie rule: all-zero coefficients receive half the unclamped gradient;
  * agreement with SH_reconstruct: the irradiance the kernel gives equals the cosine-weighted integral over the reconstructed map
    (this pins the axis convention);
  * bit-for-bit equality between the coefficient orders, with and without occluders, and under the calling contract.
Every case runs on the CPU harness; the GPU legs run the same bodies on both builds of the library.  Frames are a few hundred
texels, except where a test is about a size."""
import math

import numpy as np
import pytest
import torch

import parity_util
import scenes
from golden import make_deferred_golden as mk
from redner_amd import SHLight
from test_deferred import ADJOINT_BLOCKS, _definition_shade, _off_the_kinks, _worst_slice
from test_deferred_shadows import BLOCKERS, LIGHTS, any_rays, as_words, floor_g_buffer, occluder, shade

CPU, GPU = torch.device('cpu'), torch.device('cuda:0')
SH_R, SH_G, SH_B = 4, 5, 6
# the real basis of bands 0..2 and the clamped-cosine factors, from their closed forms
K0, K1, K2 = 0.5 * math.sqrt(1.0 / math.pi), math.sqrt(3.0 / (4.0 * math.pi)), 0.5 * math.sqrt(15.0 / math.pi)
K20, K22 = 0.25 * math.sqrt(5.0 / math.pi), 0.25 * math.sqrt(15.0 / math.pi)
LOBE = torch.tensor([math.pi] + [2.0 * math.pi / 3.0] * 3 + [math.pi / 4.0] * 5, dtype=torch.float64)
NEAR_KINK = 1e-3                      # |E| below this share of the channel's largest |E|: the texel is taken off the kink
_cache = {}


def _ru():
    from redner_amd import render_utils
    return render_utils


# ---- the fp64 definition ------------------------------------------------------------------------------------------------------------
def sh_basis64(n):
    """n [..., 3] double -> Y [..., 9]: x = -n.z, y = n.x, z = n.y"""
    x, y, z = -n[..., 2], n[..., 0], n[..., 1]
    return torch.stack([torch.full_like(x, K0), -K1 * y, K1 * z, -K1 * x, K2 * x * y, -K2 * y * z, K20 * (3.0 * z * z - 1.0),
                        -K2 * x * z, K22 * (x * x - y * y)], dim=-1)


def sh_irradiance64(n, k):
    """E(n) = sum_i A_i k_i Y_i(n) for the nine coefficients k of one channel"""
    return (sh_basis64(n) * (LOBE * k)).sum(-1)


def definition(g, types, params, ranges, aa, alpha, clamp=True):
    """g [N, H * aa, W * aa, 9 + alpha], params [L, 10] in torch double -> [N, H, W, 3 + alpha].  SH rows by the formula above
    (torch.max(E, zeros) splits the gradient at a tie); every other row is test_deferred's definition of that light alone."""
    n, hg, wg, _ = g.shape
    rgb = torch.zeros(n, hg, wg, 3, dtype=torch.float64)
    for l, t in enumerate(types):
        uses = torch.tensor([1.0 if b <= l < e else 0.0 for b, e in ranges], dtype=torch.float64)
        if float(uses.sum()) == 0:
            continue
        if t >= SH_R:
            e = sh_irradiance64(g[..., 3:6], params[l, :9])
            if clamp:
                e = torch.max(e, torch.zeros_like(e))
            channel = torch.zeros(3, dtype=torch.float64)
            channel[t - SH_R] = 1.0
            one = (e * g[..., 6 + t - SH_R] / math.pi)[..., None] * channel
        else:
            one = _definition_shade(g[..., :9], [t], params[l:l + 1], ((0, 1),) * n, 1, 0)
        rgb = rgb + one * uses[:, None, None, None]
    img = torch.cat([rgb, g[..., 9:10]], dim=-1) if alpha else rgb
    return img.reshape(n, hg // aa, aa, wg // aa, aa, img.shape[-1]).mean(dim=(2, 4))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def sh_coefficients(seed):
    """[3, 9] fp32: a small constant term under bands 1 and 2 of either sign, so that the irradiance changes sign over the sphere"""
    k = np.random.default_rng(seed).uniform(-1.0, 1.0, (3, 9))
    k[:, 0] *= 0.2
    return k.astype(np.float32)


def sh_rows(coeffs):
    """[3, n] -> the three table rows [3, 10] and their types"""
    rows = np.zeros((3, 10), np.float32)
    rows[:, :coeffs.shape[1]] = coeffs
    return [SH_R, SH_G, SH_B], rows


def mixed_table(seed):
    """ambient, SH light, point, directional, SH light, spot: ten rows"""
    types4, params4 = mk.light_table(mk.light_sets()['one_each'])
    params4 = params4 * (1.0 + 0.001 * np.arange(4, dtype=np.float32))[:, None]
    t1, r1 = sh_rows(sh_coefficients(seed))
    t2, r2 = sh_rows(sh_coefficients(seed + 100000))
    types = [int(types4[0])] + t1 + [int(types4[1]), int(types4[2])] + t2 + [int(types4[3])]
    params = np.concatenate([params4[0:1], r1, params4[1:3], r2, params4[3:4]]).astype(np.float32)
    return types, params


def sh_off_the_kink(g, types, params):
    """The gradient of max(E, 0) jumps at E == 0, and an fp32 E on the other side of it than the exact one says nothing about the
    kernel: texels with |E| below NEAR_KINK of the row's largest |E| get albedo 0 (as test_deferred._off_the_kinks does for the
    cosines).  -> (g, how many texels, [(share of texels with E > 0, share with E < 0) per SH row])"""
    nrm = g[..., 3:6].double()
    near = torch.zeros(g.shape[:3], dtype=torch.bool)
    shares = []
    for t, row in zip(types, params):
        if t < SH_R:
            continue
        e = sh_irradiance64(nrm, torch.from_numpy(np.asarray(row[:9])).double())
        near |= e.abs() < NEAR_KINK * e.abs().max()
        shares.append((float((e > 0).double().mean()), float((e < 0).double().mean())))
    g = g.clone()
    g[..., 6:9] = torch.where(near[..., None], torch.zeros(()), g[..., 6:9])
    return g, int(near.sum()), shares


def _build_case(name):
    """frame_<H>x<W>_aa<A>: two images, aa 1 without alpha and aa 3 with, ranges (0, 10) and (1, 9): both hold every SH row;
    grid_1x<H>x<W>_<capped|uncapped>: one image, aa 1 with alpha.  The seed of the coefficients is the first, counted up from the
    case's own, with which the DEFINITION has every SH row positive on >= 10 % and negative on >= 10 % of the texels and at most
    5 % of the texels near a kink."""
    kind, _, rest = name.partition('_')
    seed = 700 + sum(ord(ch) * (k + 1) for k, ch in enumerate(name)) % 1000
    if kind == 'grid':
        shape, _, side = rest.partition('_')
        n, h, w = (int(v) for v in shape.split('x'))
        aa, alpha, ranges = 1, 1, ((0, 10),) * n
        case = dict(capped=(side == 'capped'))
    else:
        shape, _, aa = rest.partition('_aa')
        h, w = (int(v) for v in shape.split('x'))
        n, aa = 2, int(aa)
        alpha, ranges = int(aa == 3), ((0, 10), (1, 9))
        case = {}
    g0 = mk.synthetic_g_buffer(seed, n, h, w, aa, alpha)
    texels = g0.shape[0] * g0.shape[1] * g0.shape[2]
    for coeff_seed in range(seed, seed + 4000):
        types, params = mixed_table(coeff_seed)
        g, moved_sh, shares = sh_off_the_kink(g0, types, params)
        if all(p >= 0.1 and m >= 0.1 for p, m in shares) and moved_sh <= 0.05 * texels:
            break
    else:
        raise AssertionError('no coefficient seed gives %s both signs of E in every row' % name)
    others = [k for k, t in enumerate(types) if t < SH_R]
    g, moved = _off_the_kinks(g, [types[k] for k in others], params[others])
    case.update(g=g, types=types, params=params, ranges=ranges, aa=aa, alpha=alpha, moved=moved, moved_sh=moved_sh, shares=shares,
                texels=texels, coeff_seed=coeff_seed)
    return case


def _definition_case(name):
    """inputs + the fp64 image and gradients, computed once and shared by the harness leg and the GPU legs of both builds"""
    if name not in _cache:
        case = _build_case(name)
        g = case['g'].double().requires_grad_(True)
        params = torch.from_numpy(case['params']).double().requires_grad_(True)
        img = definition(g, case['types'], params, case['ranges'], case['aa'], case['alpha'])
        up = mk.upstream(img.shape)
        img.backward(up.double())
        case.update(up=up, want={'image': img.detach(), 'd_g_buffer': g.grad, 'd_light_params': params.grad})
        assert all(bool(torch.isfinite(v).all()) for v in case['want'].values()), name
        _cache[name] = case
    return _cache[name]


def _apply(backend, device, g, types, params, ranges, aa, alpha, up):
    ru = _ru()
    gl = g.clone().to(device).requires_grad_(True)
    pl = torch.from_numpy(np.asarray(params, np.float32)).to(device).requires_grad_(True)
    img = ru.DeferredShade.apply(gl, pl, tuple(types), tuple(ranges), aa, bool(alpha), backend)
    img.backward(up.to(device))
    return img.detach().cpu(), gl.grad.cpu(), pl.grad.cpu()


# ---- 1. values and gradients against the fp64 definition --------------------------------------------------------------------------
def _run_definition_case(backend, device, name, tag):
    case = _definition_case(name)
    # the inputs are what the case is there for (in fp64, from the definition alone)
    nrm = case['g'][..., 3:6].double()
    for t, row in zip(case['types'], case['params']):
        if t >= SH_R:
            e = sh_irradiance64(nrm, torch.from_numpy(row[:9]).double())
            assert float((e > 0).double().mean()) >= 0.1 and float((e < 0).double().mean()) >= 0.1, (name, t)
    assert case['moved_sh'] <= 0.05 * case['texels'], (name, case['moved_sh'], case['texels'])
    n, hg, wg, _ = case['g'].shape
    h, w = hg // case['aa'], wg // case['aa']
    if 'capped' in case:
        needed, cap = (h * w + 255) // 256, max(ADJOINT_BLOCKS // n, 1)
        assert (needed > cap) == case['capped'] and needed >= cap, (name, needed, cap)
    img, d_g, d_p = _apply(backend, device, case['g'], case['types'], case['params'], case['ranges'], case['aa'], case['alpha'],
                           case['up'])
    out = {'image': img, 'd_g_buffer': d_g, 'd_light_params': d_p}
    rep = {k: {'rel_l2': _worst_slice(out[k], case['want'][k], name + ' ' + k), 'tol': parity_util.TOL, 'flipped_rows': 0,
               'measure': 'the worst light row' if k == 'd_light_params' else 'the worst image slice'} for k in out}
    print('deferred_sh_' + name, tag, {k: '%.2e' % e['rel_l2'] for k, e in rep.items()}, 'bar %.0e;' % parity_util.TOL,
          case['moved_sh'], '+', case['moved'], 'of', case['texels'], 'texels taken off a kink; coefficient seed', case['coeff_seed'])
    parity_util.record('deferred_sh_' + name, rep, tag)
    for l, t in enumerate(case['types']):
        if t >= SH_R:
            assert float(d_p[l, 9]) == 0.0, (name, 'row', l, 'column 9 of an SH row has a gradient')
            assert float(d_p[l, :9].abs().sum()) > 0
    parity_util.assert_parity(rep, name)


FRAME_CASES = ['frame_%dx%d_aa%d' % (h, w, aa) for h, w in ((1, 1), (1, 63), (1, 65), (3, 85), (1, 257)) for aa in (1, 3)]
GRID_CASES = ['grid_1x512x1024_uncapped', 'grid_1x513x1024_capped']


@pytest.mark.parametrize('name', FRAME_CASES)
def test_definition_hostsim(hostsim_backend, name):
    _run_definition_case(hostsim_backend, CPU, name, 'hostsim')


@pytest.mark.gpu
@pytest.mark.parametrize('name', GRID_CASES + FRAME_CASES)
def test_definition_gpu(gpu_backend, name):
    _run_definition_case(gpu_backend, GPU, name, 'gpu')


def _run_sh_only(backend, device):
    """A table of SH rows alone: the position takes no part, so its gradient is exactly 0.  And at the C level a row is a light
    of its own: a range that holds only an SH_G row lights green and nothing else."""
    g = mk.synthetic_g_buffer(31, 2, 3, 85, 3, 1)
    types, rows = sh_rows(sh_coefficients(32))
    up = mk.upstream((2, 3, 85, 4))
    img, d_g, d_p = _apply(backend, device, g, types, rows, ((0, 3), (0, 3)), 3, 1, up)
    assert float(img[..., :3].abs().sum()) > 0 and float(d_g[..., 3:9].abs().sum()) > 0 and float(d_p.abs().sum()) > 0
    assert bool((d_g[..., 0:3] == 0).all())
    # ambient, SH_G, point in the table; the image's range holds the SH_G row only
    types4, params4 = mk.light_table(mk.light_sets()['one_each'])
    table = np.stack([params4[0], rows[1], params4[1]])
    ttypes = [0, SH_G, 1]
    g = sh_off_the_kink(mk.synthetic_g_buffer(33, 1, 5, 13, 2, 0), [SH_G], rows[1:2])[0]
    up = mk.upstream((1, 5, 13, 3))
    img, d_g, d_p = _apply(backend, device, g, ttypes, table, ((1, 2),), 2, 0, up)
    g64 = g.double().requires_grad_(True)
    p64 = torch.from_numpy(table).double().requires_grad_(True)
    want = definition(g64, ttypes, p64, ((1, 2),), 2, 0)
    want.backward(up.double())
    assert bool((img[..., 0] == 0).all()) and bool((img[..., 2] == 0).all()) and float(img[..., 1].abs().sum()) > 0
    errors = {'image': _worst_slice(img, want.detach(), 'image'), 'd_g_buffer': _worst_slice(d_g, g64.grad, 'd_g_buffer'),
              'd_light_params': _worst_slice(d_p, p64.grad, 'd_light_params')}          # (rows 0 and 2: exactly zero)
    print('sh_g row alone', {k: '%.2e' % v for k, v in errors.items()})
    for k, v in errors.items():
        assert v < parity_util.TOL, (k, v)
    assert bool((d_g[..., [6, 8]] == 0).all())          # the albedo of the channels the row does not light


def test_sh_only_hostsim(hostsim_backend):
    _run_sh_only(hostsim_backend, CPU)


@pytest.mark.gpu
def test_sh_only_gpu(gpu_backend):
    _run_sh_only(gpu_backend, GPU)


# ---- 2. the tie rule ------------------------------------------------------------------------------------------------------------------
def _run_tie_rule(backend, device):
    """All-zero coefficients -- where an optimisation starts: E == 0 at every texel, the image is exactly 0, the clamp passes half
    the gradient to the coefficients, and the normal gets exactly none."""
    ru = _ru()
    g = mk.synthetic_g_buffer(41, 1, 6, 10, 2, 0)
    up = mk.upstream((1, 6, 10, 3))
    gl = g.clone().to(device).requires_grad_(True)
    coeffs = torch.zeros(3, 9, requires_grad=True)
    img = ru.deferred_shade(gl, [SHLight(coeffs)], aa_samples=2, backend=backend)
    img.backward(up.to(device))
    assert bool((img == 0).all())
    assert bool((gl.grad[..., 0:6] == 0).all())
    p64 = torch.zeros(3, 10, dtype=torch.float64, requires_grad=True)
    definition(g.double(), [SH_R, SH_G, SH_B], p64, ((0, 3),), 2, 0, clamp=False).backward(up.double())
    err = _worst_slice(coeffs.grad, 0.5 * p64.grad[:, :9], 'coefficient gradient at the tie')
    print('tie rule: worst row %.2e' % err)
    assert float(coeffs.grad.abs().sum()) > 0 and err < parity_util.TOL
    # (the albedo's gradient is w max(E, 0) / pi = 0 too)
    assert bool((gl.grad == 0).all())


def test_tie_rule_hostsim(hostsim_backend):
    _run_tie_rule(hostsim_backend, CPU)


@pytest.mark.gpu
def test_tie_rule_gpu(gpu_backend):
    _run_tie_rule(gpu_backend, GPU)


# ---- 3. orders ------------------------------------------------------------------------------------------------------------------------
def _run_orders(backend, device):
    ru = _ru()
    g = mk.synthetic_g_buffer(43, 1, 6, 10, 2, 1)
    up = mk.upstream((1, 6, 10, 4)).to(device)
    full = torch.from_numpy(sh_coefficients(44))

    def run(coeffs):
        gl = g.clone().to(device).requires_grad_(True)
        c = coeffs.clone().requires_grad_(True)
        img = ru.deferred_shade(gl, [SHLight(c)], alpha=True, aa_samples=2, backend=backend)
        img.backward(up)
        return img.detach(), gl.grad, c.grad

    for n in (1, 4):
        padded = torch.zeros(3, 9)
        padded[:, :n] = full[:, :n]
        a, b = run(full[:, :n]), run(padded)
        assert float(a[0][..., :3].abs().sum()) > 0
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), n
        assert tuple(a[2].shape) == (3, n) and torch.equal(a[2], b[2][:, :n]), n


def test_orders_hostsim(hostsim_backend):
    _run_orders(hostsim_backend, CPU)


@pytest.mark.gpu
def test_orders_gpu(gpu_backend):
    _run_orders(gpu_backend, GPU)


# ---- 4. agreement with SH_reconstruct ------------------------------------------------------------------------------------------------
def _run_sh_reconstruct_agreement(backend, device):
    """The irradiance E_c(n) the kernel gives (albedo pi, upstream 1: the image IS max(E, 0)) equals the cosine-weighted integral
    of the environment map that SH_reconstruct makes of the same coefficients, by midpoint quadrature over its 64 x 128 texels:
    sum L(w) max(n.w, 0) sin(theta) dtheta dphi, the texel at (theta, phi) lying in direction
    (sin phi sin theta, cos theta, -cos phi sin theta).  Coefficients: constant term 3.0, the other eight uniform in +-0.3 (the
    map stays positive, so its clamp does not act).  The quadrature's own error, measured in fp64 numpy for this family, is 2.3e-4
    of the largest |E| at 64 x 128 (7e-5 at 128 x 256, 1.6e-5 at 256 x 512); the bar is 1e-3, four times that (fp32 adds on the
    order of 1e-6).  A permuted axis or a dropped sign misses the bar by two orders of magnitude (profiles/deferred_sh.txt)."""
    from redner_amd import SH_reconstruct
    ru = _ru()
    rng = np.random.default_rng(51)
    coeffs = rng.uniform(-0.3, 0.3, (3, 9)).astype(np.float32)
    coeffs[:, 0] = 3.0
    res = (64, 128)
    env = SH_reconstruct(torch.from_numpy(coeffs).to(device), res, backend=backend).cpu().double().numpy()
    assert env.min() > 0
    normals = rng.normal(size=(200, 3))
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    g = torch.zeros(1, 1, 200, 9)
    g[0, 0, :, 3:6] = torch.from_numpy(normals.astype(np.float32))
    g[..., 6:9] = math.pi
    got = ru.deferred_shade(g.to(device), [SHLight(torch.from_numpy(coeffs))], aa_samples=1, backend=backend)[0, 0].cpu().double().numpy()
    theta = math.pi * (np.arange(res[0]) + 0.5) / res[0]
    phi = 2.0 * math.pi * (np.arange(res[1]) + 0.5) / res[1]
    st, ct = np.sin(theta)[:, None], np.cos(theta)[:, None]
    w = np.stack([np.sin(phi)[None] * st, ct * np.ones_like(phi)[None], -np.cos(phi)[None] * st], axis=-1)          # [64, 128, 3]
    n32 = g[0, 0, :, 3:6].double().numpy()
    cosine = np.maximum(np.einsum('rcx,nx->nrc', w, n32), 0.0)
    weight = st * (math.pi / res[0]) * (2.0 * math.pi / res[1])
    want = np.einsum('nrc,rck->nk', cosine * weight[None], env)
    err = np.abs(got - want).max() / np.abs(want).max()
    print('SH_reconstruct agreement: %.2e of the largest |E| (bar 1e-3)' % err)
    assert err < 1e-3


def test_sh_reconstruct_agreement_hostsim(hostsim_backend):
    _run_sh_reconstruct_agreement(hostsim_backend, CPU)


@pytest.mark.gpu
def test_sh_reconstruct_agreement_gpu(gpu_backend):
    _run_sh_reconstruct_agreement(gpu_backend, GPU)


# ---- 5. end to end --------------------------------------------------------------------------------------------------------------------
def _run_end_to_end(backend, device):
    ru = _ru()
    res, aa, seed = 16, 2, 7

    def scene_and_lights():
        sc = scenes.two_triangles(device, resolution=(res, res))
        coeffs = torch.from_numpy(sh_coefficients(61)).requires_grad_(True)
        return sc, coeffs, [ru.AmbientLight(torch.tensor([0.2, 0.25, 0.3])), SHLight(coeffs)]

    sc, coeffs, lights = scene_and_lights()
    img = ru.render_deferred(sc, lights, aa_samples=aa, seed=seed, device=device, backend=backend)
    assert tuple(img.shape) == (res, res, 3)
    (img * mk.upstream(img.shape).to(device)).sum().backward()
    for t in (sc.shapes[0].vertices.grad, sc.shapes[1].vertices.grad, coeffs.grad):
        assert t is not None and bool(torch.isfinite(t).all()) and float(t.abs().sum()) > 0
    assert tuple(coeffs.grad.shape) == (3, 9)
    sc2, _, lights2 = scene_and_lights()
    sc2.camera.resolution = (res * aa, res * aa)
    ch = [backend.channels.position, backend.channels.shading_normal, backend.channels.diffuse_reflectance]
    g = ru.render_g_buffer(sc2, ch, seed=seed, device=device, backend=backend).detach().unsqueeze(0)
    pieces = ru.deferred_shade(g, lights2, aa_samples=aa, backend=backend)
    assert torch.equal(pieces[0], img.detach())
    no_sh = ru.deferred_shade(g, lights2[:1], aa_samples=aa, backend=backend)
    assert int((no_sh[0] != img.detach()).any(dim=-1).sum()) >= 8          # the SH light is in the image


def test_end_to_end_hostsim(hostsim_backend):
    _run_end_to_end(hostsim_backend, CPU)


@pytest.mark.gpu
def test_end_to_end_gpu(gpu_backend):
    _run_end_to_end(gpu_backend, GPU)


# ---- 6. with shadows ------------------------------------------------------------------------------------------------------------------
def _run_shadows(backend, device):
    ru = _ru()
    hg, wg, aa = 20, 24, 2
    g = floor_g_buffer(hg, wg, 0)
    blockers = occluder(backend, BLOCKERS, device)
    up = mk.upstream((1, hg // aa, wg // aa, 3))
    types, rows = sh_rows(sh_coefficients(71) + np.float32([[1.0] + [0.0] * 8]))          # (lit from above: the floor sees E > 0)
    # SH rows alone: occluders change nothing, and every bit stays set
    plain = shade(backend, device, g, types, rows, ((0, 3),), aa, 0, None, up)
    shadowed = shade(backend, device, g, types, rows, ((0, 3),), aa, 0, (blockers,), up)
    assert float(plain[0].abs().sum()) > 0 and float(plain[3].abs().sum()) > 0
    for a, b, what in zip(plain, shadowed, ('image', None, 'd_g_buffer', 'd_light_params')):
        if what:
            assert torch.equal(a, b), what
    assert (as_words(shadowed[1]) == 7).all()
    # a point light that the blockers do block: the SH rows beside it cast no ray of their own and keep their bits
    ptypes, pparams = mk.light_table([LIGHTS[1]])
    before = any_rays(backend)
    alone = shade(backend, device, g, [1], pparams, ((0, 1),), aa, 0, (blockers,), up)
    rays_alone = any_rays(backend) - before
    both = shade(backend, device, g, [1] + types, np.concatenate([pparams, rows]), ((0, 4),), aa, 0, (blockers,), up)
    assert any_rays(backend) - before - rays_alone == rays_alone and rays_alone > 0
    words_alone, words_both = as_words(alone[1])[0], as_words(both[1])[0]
    assert (words_alone == 0).any() and ((words_both & 1) == words_alone).all() and ((words_both >> 1) == 7).all()
    # the 32 bits of a word are rows of the table: ten SHLights and two others fit, eleven SHLights do not
    lights = [SHLight(torch.from_numpy(sh_coefficients(80 + k))) for k in range(11)]
    others = [ru.AmbientLight(torch.tensor([0.1, 0.1, 0.1])), ru.PointLight(torch.tensor([0.3, 0.2, 2.0]), torch.tensor([30.0, 25.0, 20.0]))]
    img, vis = ru.deferred_shade(g.to(device), lights[:10] + others, aa_samples=aa, backend=backend, occluders=blockers,
                                 return_visibility=True)
    assert bool(torch.isfinite(img).all()) and (as_words(vis.cpu()) >> 31 == words_alone).all()          # (the point light is row 31)
    with pytest.raises(RuntimeError, match='image 0 has 33 lights, at most 32'):
        ru.deferred_shade(g.to(device), lights, aa_samples=aa, backend=backend, occluders=blockers)


def test_shadows_hostsim(hostsim_backend):
    _run_shadows(hostsim_backend, CPU)


@pytest.mark.gpu
def test_shadows_gpu(gpu_backend):
    _run_shadows(gpu_backend, GPU)


# ---- 7. calling contract --------------------------------------------------------------------------------------------------------------
def _run_calling_contract(backend, device):
    ru = _ru()
    g = mk.synthetic_g_buffer(91, 2, 6, 10, 2, 1)
    up = mk.upstream((2, 6, 10, 4)).to(device)
    values = torch.from_numpy(sh_coefficients(92))
    ambient = ru.AmbientLight(torch.tensor([0.2, 0.25, 0.3]))

    def run(coeffs, upstream=up, lights=None):
        gl = g.clone().to(device).requires_grad_(True)
        img = ru.deferred_shade(gl, lights or [ambient, SHLight(coeffs)], alpha=True, aa_samples=2, backend=backend)
        if upstream is None:
            img.sum().backward()                          # a stride-0 expanded upstream gradient
        else:
            img.backward(upstream)
        return img.detach(), gl.grad

    fresh = values.clone().to(device).requires_grad_(True)
    ref = run(fresh)
    wide = torch.zeros(3, 18)
    wide[:, ::2] = values
    wide.requires_grad_(True)
    view = wide[:, ::2]                                   # a view that is not contiguous
    assert not view.is_contiguous()
    out = run(view)
    assert torch.equal(out[0], ref[0]) and torch.equal(out[1], ref[1])
    assert torch.equal(wide.grad[:, ::2], fresh.grad.cpu()) and bool((wide.grad[:, 1::2] == 0).all())
    host = values.clone().requires_grad_(True)            # coefficients on the host, whatever the G-buffer's device
    out = run(host)
    assert host.grad.device.type == 'cpu' and torch.equal(out[0], ref[0]) and torch.equal(out[1], ref[1])
    assert torch.equal(host.grad, fresh.grad.cpu())
    a, b = values.clone().requires_grad_(True), values.clone().requires_grad_(True)
    ones = run(a, upstream=None)
    explicit = run(b, upstream=torch.ones_like(ref[0]))
    assert torch.equal(ones[1], explicit[1]) and torch.equal(a.grad, b.grad)
    # per-image light lists: the ranges count rows (an SHLight is three), and an image sees its own list only
    c0, c1 = values.clone().requires_grad_(True), (0.5 * values).requires_grad_(True)
    point = ru.PointLight(torch.tensor([1.0, 2.0, -3.0]), torch.tensor([30.0, 25.0, 20.0]))
    lists = [[SHLight(c0), ambient], [point, SHLight(c1)]]
    batch = run(None, lights=lists)
    for k in range(2):
        gl = g[k:k + 1].clone().to(device).requires_grad_(True)
        one = ru.deferred_shade(gl, lists[k], alpha=True, aa_samples=2, backend=backend)
        one.backward(up[k:k + 1])
        assert torch.equal(one[0], batch[0][k]) and torch.equal(gl.grad[0], batch[1][k]), k
    # ... and a light called directly goes through the same kernel
    light = SHLight(values)
    direct = light.render(g[0, :, :, :3].to(device), g[0, :, :, 3:6].to(device), g[0, :, :, 6:9].to(device))
    assert torch.equal(direct, ru.deferred_shade(g[0:1, ..., :9].contiguous().to(device), [light], aa_samples=1, backend=backend)[0])


def test_calling_contract_hostsim(hostsim_backend):
    _run_calling_contract(hostsim_backend, CPU)


@pytest.mark.gpu
def test_calling_contract_gpu(gpu_backend):
    _run_calling_contract(gpu_backend, GPU)


# ---- 8. reproducibility ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_coefficient_gradient_bitwise_reproducible_gpu(gpu_backend):
    """The coefficient gradients are sums over 4 M texels: per-block fp64 partials folded in a fixed order, no atomics."""
    ru = _ru()
    g = mk.synthetic_g_buffer(5, 1, 1024, 1024, 2, 1).to(GPU)
    up = mk.upstream((1, 1024, 1024, 4)).to(GPU)
    values = torch.from_numpy(sh_coefficients(95))
    runs = []
    for _ in range(2):
        coeffs = values.clone().to(GPU).requires_grad_(True)
        ru.deferred_shade(g, [SHLight(coeffs)], alpha=True, aa_samples=2, backend=gpu_backend).backward(up)
        runs.append(coeffs.grad.cpu().numpy())
    assert np.isfinite(runs[0]).all() and np.abs(runs[0]).sum() > 0
    assert runs[0].tobytes() == runs[1].tobytes()


# ---- 9. errors ------------------------------------------------------------------------------------------------------------------------
def test_errors_hostsim(hostsim_backend):
    rd, ru = hostsim_backend, _ru()
    for shape in ((3, 5), (9,), (4, 9)):
        with pytest.raises(RuntimeError, match='SHLight'):
            SHLight(torch.zeros(shape))
    g = mk.synthetic_g_buffer(1, 1, 4, 4, 2, 0)
    light = SHLight(torch.zeros(3, 9))
    light.coeffs = torch.zeros(3, 5)                      # a shape that went wrong after the light was made
    with pytest.raises(RuntimeError, match='SHLight'):
        ru.deferred_shade(g, [light], aa_samples=2, backend=rd)
    with pytest.raises(RuntimeError, match='SHLight'):       # before the G-buffer is rendered
        ru.render_deferred(None, [ru.AmbientLight(torch.ones(3)), light], aa_samples=2, seed=1, device=CPU, backend=rd)
    assert [int(rd.DeferredLightType[n]) for n in ('sh_r', 'sh_g', 'sh_b')] == [SH_R, SH_G, SH_B]
    params, img = torch.zeros(2, 10), torch.zeros(1, 4, 4, 3)
    ptr = lambda t: rd.float_ptr(t.data_ptr())
    rd.deferred_shade(ptr(g), ptr(params), ptr(img), 1, 4, 4, 2, False, [0, SH_B], [(0, 2)], False, 0)
    with pytest.raises(RuntimeError, match='unknown light type'):
        rd.deferred_shade(ptr(g), ptr(params), ptr(img), 1, 4, 4, 2, False, [0, 7], [(0, 2)], False, 0)
    with pytest.raises(RuntimeError, match='unknown light type'):
        rd.deferred_shade(ptr(g), ptr(params), ptr(img), 1, 4, 4, 2, False, [0, -1], [(0, 2)], False, 0)
