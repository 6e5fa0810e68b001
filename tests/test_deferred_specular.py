"""Specular highlights in deferred shading (rdr_deferred_specular / _backward, csrc/deferred_specular.h;
redner_amd.render_utils.DeferredSpecular, deferred_specular, render_deferred(specular=True)).

The oracle is the definition of csrc/deferred_specular_abi.h written here in torch fp64 (`lobe64`), with autograd for the five
gradients: the image, d_g_buffer, d_material, d_eye and d_light_params are each held to parity_util.TOL (1e-4 relative L2 of the
tensor's own norm) on the worst image slice / light row.  Gates are `where` on conditions, which autograd holds constant; every
max(x, 0) and the roughness floor are torch.max of two tensors, which splits the gradient at a tie.

The generator (seeded): positions in [-1, 1]^2 x [-0.1, 0.1]; three quarters of the normals in a cone about +z
(+z + 0.6 U(-1, 1)^3), a quarter uniform on the sphere, stored lengths in [0.5, 2]; roughness log-uniform in [0.02, 1.5] (fp32
powf with e <= 98 stays inside the bar); ks uniform in [-0.1, 1]; the eye near (0.3, 0.2, 2); the lights near (-0.5, 0.4, 1.5).

A texel within K = 1e-3 of a gate -- |cv|, |cl - 1e-3|, |cm|, |a / 1.6 - 1| of either G1, |rho - 1|, |ks_k| -- is excluded (its
normal is set to 0: a background texel): an fp32 value on the other side of a gate than the exact one says nothing about the
kernel.  A case asserts that at most 2 % of its texels are excluded and that it covers both G1 branches and both sides of every
gate; its seed is the first, counted up from the case's own, for which the DEFINITION says so.

Every case runs on the CPU harness; the GPU legs run the same bodies on both builds of the library."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import parity_util
from golden import make_deferred_golden as mk
from test_deferred import ADJOINT_BLOCKS, _worst_slice

CPU, GPU = torch.device('cpu'), torch.device('cuda:0')
AMBIENT, POINT, DIRECTIONAL, SPOT, SH_R, SH_G, SH_B = range(7)
FLOOR = float(np.float32(1e-3))         # the roughness floor and the grazing rule, as the fp32 kernels hold them
GRAZING = float(np.float32(1e-3))
K = 1e-3                                # how near a gate a texel is excluded
INPLACE = 'modified by an inplace operation'
_cache = {}


def _ru():
    from redner_amd import render_utils
    return render_utils


# ---- the fp64 definition ------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a * b).sum(-1)


def _g1(c, r):
    """c > 0 (the caller substitutes a harmless cosine where the texel is gated) -> G1, a, which texels take the rational branch"""
    u = 1.0 / (c * c) - 1.0
    sloped = u > 0
    t = torch.sqrt(torch.where(sloped, u, torch.ones_like(u)))
    a = 1.0 / (torch.sqrt(r) * t)
    rational = (3.535 * a + 2.181 * a * a) / (1.0 + 2.276 * a + 2.577 * a * a)
    use = sloped & (a < 1.6)
    return torch.where(use, rational, torch.ones_like(a)), a.detach(), use


def _incident(t, row, p):
    intensity = row[0:3]
    if t == DIRECTIONAL:
        l = (-row[6:9] / row[6:9].norm()).expand_as(p)
        return l, intensity.expand_as(p)
    d = row[3:6] - p
    r2 = _dot(d, d)[..., None]
    l = d / torch.sqrt(r2)
    if t == POINT:
        return l, intensity / r2
    s = -row[6:9] / row[6:9].norm()
    ls = _dot(l, s)
    return l, intensity * torch.pow(torch.max(ls, torch.zeros_like(ls)), row[9])[..., None]


def lobe64(g, mat, eye, types, params, ranges, aa, vis=None, clamp_e=True, clamp_ks=True, floor=True):
    """g [N, Hg, Wg, >= 6], mat [N, Hg, Wg, 4], eye [N, 3], params [L, 10] in torch double -> (image [N, H, W, 3], report).
    `vis`: int64 words, bit (row - range begin) clear: the light adds nothing.  clamp_e / clamp_ks / floor = False: that max() is
    left out (the tie tests compare with half of the gradient of the expression without it); clamp_e = 'constant': e takes no part
    in the gradient (the roughness still acts through G).
    report: per lit (texel, light) pair which side of each gate / branch it is on, and which texels are within K of a gate."""
    n, hg, wg, _ = g.shape
    p, nrm = g[..., 0:3], g[..., 3:6]
    ks, rho = mat[..., 0:3], mat[..., 3]
    nn = _dot(nrm, nrm)
    has_n = (nn > 0) & torch.isfinite(nn)
    nh = nrm / torch.sqrt(torch.where(has_n, nn, torch.ones_like(nn)))[..., None]
    ev = eye[:, None, None, :] - p
    v = ev / ev.norm(dim=-1, keepdim=True)
    cv = _dot(nh, v)
    r = torch.max(rho, torch.full_like(rho, FLOOR)) if floor else rho
    e = 2.0 / r - 2.0
    if clamp_e == 'constant':
        e = e.detach()
    elif clamp_e:
        e = torch.max(e, torch.zeros_like(e))
    k = torch.max(ks, torch.zeros_like(ks)) if clamp_ks else ks
    rgb = torch.zeros(n, hg, wg, 3, dtype=torch.float64)
    near = (rho.detach() - 1.0).abs() < K
    near |= (ks.detach().abs() < K).any(-1)
    sides = {name: [0, 0] for name in ('cv', 'cl', 'cm', 'g1', 'rho', 'ks')}
    lit_pairs = 0
    for li, t in enumerate(types):
        if t not in (POINT, DIRECTIONAL, SPOT):
            continue
        uses = torch.tensor([b <= li < e_ for b, e_ in ranges])
        if not bool(uses.any()):
            continue
        in_range = uses[:, None, None].expand(n, hg, wg)
        l, E = _incident(t, params[li], p)
        cl = _dot(nh, l)
        hv = v + l
        m = hv / hv.norm(dim=-1, keepdim=True)
        cm = _dot(nh, m)
        shaded = in_range & has_n
        if vis is not None:
            bit = torch.tensor([max(li - b, 0) for b, _ in ranges], dtype=torch.int64)[:, None, None]
            shaded = shaded & (((vis >> bit) & 1) != 0)
        lit = shaded & (cv > 0) & (cl > GRAZING) & (cm > 0)
        half = torch.full_like(cv, 0.5)
        cvs, cls, cms = torch.where(lit, cv, half), torch.where(lit, cl, half), torch.where(lit, cm, half)
        D = torch.pow(cms, e) * (e + 2.0) / (2.0 * math.pi)
        g1v, av, use_v = _g1(cvs, r)
        g1l, al, use_l = _g1(cls, r)
        q = 1.0 - _dot(m, l).abs()
        q = torch.max(q, torch.zeros_like(q))
        F = k + (1.0 - k) * (q ** 5)[..., None]
        value = E * F * (D * g1v * g1l / (4.0 * cvs))[..., None]
        rgb = rgb + torch.where(lit[..., None], value, torch.zeros_like(value))
        with torch.no_grad():
            near |= shaded & ((cv.abs() < K) | ((cl - GRAZING).abs() < K) | (cm.abs() < K))
            near |= lit & (((av / 1.6 - 1.0).abs() < K) | ((al / 1.6 - 1.0).abs() < K))
            for name, c, gate in (('cv', cv, 0.0), ('cl', cl, GRAZING), ('cm', cm, 0.0)):
                sides[name][0] += int((shaded & (c > gate)).sum())
                sides[name][1] += int((shaded & ~(c > gate)).sum())
            sides['g1'][0] += int((lit & use_v).sum()) + int((lit & use_l).sum())
            sides['g1'][1] += int((lit & ~use_v).sum()) + int((lit & ~use_l).sum())
            lit_pairs += int(lit.sum())
    with torch.no_grad():
        sides['rho'] = [int((has_n & (rho >= 1)).sum()), int((has_n & (rho < 1)).sum())]
        sides['ks'] = [int((has_n[..., None] & (ks > 0)).sum()), int((has_n[..., None] & (ks < 0)).sum())]
    image = rgb.reshape(n, hg // aa, aa, wg // aa, aa, 3).mean(dim=(2, 4))
    return image, {'near': near & has_n, 'sides': sides, 'lit_pairs': lit_pairs}


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def generate(seed, n, h, w, aa, alpha):
    """-> g [n, h aa, w aa, 9 + alpha], material [n, h aa, w aa, 4], eye [n, 3] fp32, by the module docstring"""
    rng = np.random.default_rng(seed)
    hg, wg = h * aa, w * aa
    shape = (n, hg, wg)
    pos = rng.uniform(-1.0, 1.0, shape + (3,)) * np.array([1.0, 1.0, 0.1])
    cone = np.array([0.0, 0.0, 1.0]) + 0.6 * rng.uniform(-1.0, 1.0, shape + (3,))
    ball = rng.normal(size=shape + (3,))
    nrm = np.where(rng.uniform(size=shape + (1,)) < 0.75, cone, ball)
    nrm = nrm / np.linalg.norm(nrm, axis=-1, keepdims=True) * rng.uniform(0.5, 2.0, shape + (1,))
    parts = [pos, nrm, rng.uniform(0.1, 0.9, shape + (3,))]
    if alpha:
        parts.append(rng.uniform(0.0, 1.0, shape + (1,)))
    rough = np.exp(rng.uniform(math.log(0.02), math.log(1.5), shape + (1,)))
    mat = np.concatenate([rng.uniform(-0.1, 1.0, shape + (3,)), rough], axis=-1)
    eye = np.array([0.3, 0.2, 2.0]) + 0.1 * rng.uniform(-1.0, 1.0, (n, 3))
    as32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return as32(np.concatenate(parts, axis=-1)), as32(mat), as32(eye)


def light_row(rng, t):
    """one row of the table near (-0.5, 0.4, 1.5); a spot aims at the origin with exponent in [1.5, 4]"""
    row = np.zeros(10, np.float32)
    if t in (SH_R, SH_G, SH_B):
        row[:9] = rng.uniform(-1.0, 1.0, 9)
        return row
    row[0:3] = rng.uniform(0.5, 2.0, 3)
    pos = np.array([-0.5, 0.4, 1.5]) + 0.2 * rng.uniform(-1.0, 1.0, 3)
    if t in (POINT, SPOT):
        row[3:6] = pos
    if t == DIRECTIONAL:
        row[6:9] = -pos * rng.uniform(0.5, 2.0)
    if t == SPOT:
        row[6:9] = -pos + 0.2 * rng.uniform(-1.0, 1.0, 3)
        row[9] = rng.uniform(1.5, 4.0)
    return row


def light_rows(seed, types):
    rng = np.random.default_rng(seed)
    return np.stack([light_row(rng, t) for t in types]).astype(np.float32)


MIXED = [AMBIENT, POINT, SH_R, DIRECTIONAL, SPOT, SH_G, SH_B]
SIZES = ((5, 7), (16, 16), (17, 16))
GRID_CASES = ['grid_%dx%d_aa%d_alpha%d' % (h, w, aa, alpha) for h, w in SIZES for aa in (1, 2, 3) for alpha in (0, 1)]
OTHER_CASES = ['empty_range', 'point_alone', 'directional_alone', 'spot_alone']
PLAN_CASE = 'plan_725x725'


def _shape_of(name):
    """-> n, h, w, aa, alpha, types, ranges"""
    if name.startswith('grid_'):
        size, aa, alpha = re.match(r'grid_(\d+x\d+)_aa(\d)_alpha(\d)', name).groups()
        h, w = (int(v) for v in size.split('x'))
        return 2, h, w, int(aa), int(alpha), MIXED, ((0, 7), (1, 5))
    if name == 'empty_range':
        return 2, 5, 7, 2, 0, MIXED, ((0, 7), (3, 3))
    if name == PLAN_CASE:
        return 1, 725, 725, 1, 0, [POINT], ((0, 1),)
    alone = {'point_alone': POINT, 'directional_alone': DIRECTIONAL, 'spot_alone': SPOT}[name]
    return 1, 17, 16, 2, 1, [alone], ((0, 1),)


def _covers(report, texels):
    return all(a > 0 and b > 0 for a, b in report['sides'].values()) and int(report['near'].sum()) <= 0.02 * texels


def _build_case(name):
    n, h, w, aa, alpha, types, ranges = _shape_of(name)
    base = 900 + sum(ord(ch) * (k + 1) for k, ch in enumerate(name)) % 1000
    for seed in range(base, base + 200):
        g, mat, eye = generate(seed, n, h, w, aa, alpha)
        params = light_rows(seed + 5000, types)
        texels = n * h * aa * w * aa
        with torch.no_grad():
            _, report = lobe64(g.double(), mat.double(), eye.double(), types, torch.from_numpy(params).double(), ranges, aa)
        excluded = int(report['near'].sum())
        g[..., 3:6] = torch.where(report['near'][..., None], torch.zeros(()), g[..., 3:6])
        with torch.no_grad():
            _, report = lobe64(g.double(), mat.double(), eye.double(), types, torch.from_numpy(params).double(), ranges, aa)
        if excluded <= 0.02 * texels and _covers(report, texels):
            break
    else:
        raise AssertionError('no seed gives %s both sides of every gate' % name)
    return dict(g=g, mat=mat, eye=eye, types=types, params=params, ranges=ranges, aa=aa, alpha=alpha, texels=texels,
                excluded=excluded, report=report, seed=seed, n=n, h=h, w=w)


def _reference(case, vis=None, **variant):
    """the fp64 image and the five gradients for the case's upstream gradient"""
    g = case['g'].double().requires_grad_(True)
    mat = case['mat'].double().requires_grad_(True)
    eye = case['eye'].double().requires_grad_(True)
    params = torch.from_numpy(case['params']).double().requires_grad_(True)
    img, _ = lobe64(g, mat, eye, case['types'], params, case['ranges'], case['aa'], vis=vis, **variant)
    up = mk.upstream(img.shape)
    img.backward(up.double())
    want = {'image': img.detach(), 'd_g_buffer': g.grad, 'd_material': mat.grad, 'd_eye': eye.grad, 'd_light_params': params.grad}
    assert all(bool(torch.isfinite(t).all()) for t in want.values())
    return up, want


def _definition_case(name):
    """inputs + the fp64 image and gradients, computed once and shared by the harness leg and the GPU legs of both builds"""
    if name not in _cache:
        case = _build_case(name)
        case['up'], case['want'] = _reference(case)
        _cache[name] = case
    return _cache[name]


def _apply(backend, device, case, up, vis=None, g=None, mat=None, eye=None):
    ru = _ru()
    gl = (case['g'] if g is None else g).clone().to(device).requires_grad_(True)
    ml = (case['mat'] if mat is None else mat).clone().to(device).requires_grad_(True)
    el = (case['eye'] if eye is None else eye).clone().to(device).requires_grad_(True)
    pl = torch.from_numpy(np.asarray(case['params'], np.float32)).to(device).requires_grad_(True)
    words = None if vis is None else vis.to(device)
    img = ru.DeferredSpecular.apply(gl, ml, el, pl, tuple(case['types']), tuple(case['ranges']), case['aa'], bool(case['alpha']),
                                    backend, words)
    img.backward(up.to(device))
    return {'image': img.detach().cpu(), 'd_g_buffer': gl.grad.cpu(), 'd_material': ml.grad.cpu(), 'd_eye': el.grad.cpu(),
            'd_light_params': pl.grad.cpu()}


def _errors(out, want, name):
    errors = {k: _worst_slice(out[k], want[k], name + ' ' + k) for k in want}
    print(name, {k: '%.2e' % e for k, e in errors.items()}, 'bar %.0e' % parity_util.TOL)
    return errors


def _assert_parity(out, want, name):
    for k, e in _errors(out, want, name).items():
        assert e < parity_util.TOL, (name, k, e)


# ---- 1. values and gradients against the fp64 definition --------------------------------------------------------------------------
def _run_definition_case(backend, device, name, tag):
    case = _definition_case(name)
    report = case['report']
    assert case['excluded'] <= 0.02 * case['texels'], (name, case['excluded'], case['texels'])
    assert all(a > 0 and b > 0 for a, b in report['sides'].values()), (name, report['sides'])
    assert int(report['near'].sum()) == 0 and report['lit_pairs'] > 0
    if name == PLAN_CASE:                   # the capped adjoint grid strides
        assert (case['h'] * case['w'] + 255) // 256 > ADJOINT_BLOCKS
    print('deferred_specular', name, tag, 'seed', case['seed'], 'excluded', case['excluded'], 'of', case['texels'], report['sides'])
    out = _apply(backend, device, case, case['up'])
    rep = {k: {'rel_l2': e, 'tol': parity_util.TOL, 'flipped_rows': 0} for k, e in _errors(out, case['want'], name).items()}
    parity_util.record('deferred_specular_' + name, rep, tag)
    for l, t in enumerate(case['types']):               # ambient and SH rows: exactly zero
        if t in (AMBIENT, SH_R, SH_G, SH_B):
            assert bool((out['d_light_params'][l] == 0).all()), (name, l)
    assert bool((out['d_g_buffer'][..., 6:] == 0).all())          # the albedo and alpha channels
    parity_util.assert_parity(rep, name)


@pytest.mark.parametrize('name', GRID_CASES + OTHER_CASES + [PLAN_CASE])
def test_definition_hostsim(hostsim_backend, name):
    _run_definition_case(hostsim_backend, CPU, name, 'hostsim')


@pytest.mark.gpu
@pytest.mark.parametrize('name', GRID_CASES + OTHER_CASES + [PLAN_CASE])
def test_definition_gpu(gpu_backend, name):
    _run_definition_case(gpu_backend, GPU, name, 'gpu')


# ---- 2. gates -------------------------------------------------------------------------------------------------------------------------
def _plane(h, w, normal, rho, seed):
    """a flat patch in z = 0 with one normal and one roughness everywhere"""
    g, mat, eye = generate(seed, 1, h, w, 1, 0)
    g[..., 2] = 0.0
    g[..., 3:6] = torch.tensor(normal, dtype=torch.float32)
    mat[..., 3] = rho
    eye[:] = torch.tensor([0.3, 0.2, 2.0])
    return g, mat, eye


def _run_gates(backend, device):
    types = [AMBIENT, POINT, DIRECTIONAL, SPOT, SH_R]
    params = light_rows(11, types)
    base = dict(types=types, params=params, ranges=((0, 5),), aa=1, alpha=0)
    up = mk.upstream((1, 6, 11, 3))
    rough = float(np.float32(0.3))
    off_mirror = params.copy()               # every light low in -x: the half vector is some 45 degrees off +z
    off_mirror[:, 3:6] = np.float32([-3.0, 0.4, 0.5])
    off_mirror[:, 6:9] = np.float32([3.0, -0.4, -0.5])
    below = light_rows(12, types)            # every light under the plane
    below[:, 3:6] *= np.float32([1, 1, -1])
    below[:, 6:9] *= np.float32([1, 1, -1])
    gates = {
        'background texels': (_plane(6, 11, [0.0, 0.0, 0.0], rough, 21), params),
        'facing away from the eye': (_plane(6, 11, [0.0, 0.0, -1.5], rough, 22), params),
        'facing away from the light': (_plane(6, 11, [0.0, 0.0, 0.7], rough, 23), below),
        'roughness 0': (_plane(6, 11, [0.0, 0.0, 1.0], 0.0, 24), off_mirror),
        'roughness below the floor': (_plane(6, 11, [0.0, 0.0, 1.0], 5e-4, 25), off_mirror),
    }
    for what, ((g, mat, eye), table) in gates.items():
        out = _apply(backend, device, dict(base, g=g, mat=mat, eye=eye, params=table), up)
        for k, t in out.items():
            assert bool(torch.isfinite(t).all()) and bool((t == 0).all()), (what, k)
    # ... and the lit patch is lit (the gates above are not the kernel returning zeros)
    g, mat, eye = _plane(6, 11, [0.0, 0.0, 1.0], rough, 26)
    out = _apply(backend, device, dict(base, g=g, mat=mat, eye=eye), up)
    assert all(float(t.abs().sum()) > 0 and bool(torch.isfinite(t).all()) for t in out.values())
    assert bool((out['d_light_params'][[0, 4]] == 0).all())          # the ambient row and the SH row
    # the floor on the generator's texels: roughness 0 and below the floor give the bits of roughness 1e-3, everything is
    # finite, and the roughness gets exactly no gradient
    g, mat, eye = generate(27, 1, 6, 11, 1, 0)
    runs = []
    for rho in (FLOOR, 0.0, 5e-4):
        m = mat.clone()
        m[..., 3] = rho
        runs.append(_apply(backend, device, dict(base, g=g, mat=m, eye=eye), up))
        assert all(bool(torch.isfinite(t).all()) for t in runs[-1].values()), rho
    for run in runs[1:]:
        assert bool((run['d_material'][..., 3] == 0).all())
        for k in ('image', 'd_g_buffer', 'd_eye', 'd_light_params'):
            assert torch.equal(run[k], runs[0][k]), k
        assert torch.equal(run['d_material'][..., :3], runs[0]['d_material'][..., :3])


def test_gates_hostsim(hostsim_backend):
    _run_gates(hostsim_backend, CPU)


@pytest.mark.gpu
def test_gates_gpu(gpu_backend):
    _run_gates(gpu_backend, GPU)


# ---- 3. the tie rule ------------------------------------------------------------------------------------------------------------------
def _run_tie_rule(backend, device):
    types, ranges = [POINT, DIRECTIONAL], ((0, 2),)
    params = light_rows(31, types)
    g, mat, eye = generate(32, 1, 6, 11, 2, 0)
    g[..., 3:6] = g[..., 3:6].abs() * torch.tensor([0.3, 0.3, 1.0])          # towards the eye and the lights: mostly lit
    base = dict(g=g, eye=eye, types=types, params=params, ranges=ranges, aa=2, alpha=0)
    # rho == 1 exactly: e = max(2 / r - 2, 0) at its tie.  The roughness also acts through G, which no max stands before: the
    # gradient is the mean of the one with e left free and the one with e held constant
    m = mat.clone()
    m[..., 3] = 1.0
    case = dict(base, mat=m)
    up, want = _reference(case)
    _, free = _reference(case, clamp_e=False)
    _, held = _reference(case, clamp_e='constant')
    out = _apply(backend, device, case, up)
    _assert_parity(out, want, 'tie rho == 1')
    through_e = free['d_material'][..., 3] - held['d_material'][..., 3]
    assert float(through_e.norm()) > 0.1 * float(held['d_material'][..., 3].norm()) > 0
    err = _worst_slice(out['d_material'][..., 3], held['d_material'][..., 3] + 0.5 * through_e, 'rho == 1: half')
    assert err < parity_util.TOL, err
    # ks_k == 0 exactly: half of the gradient of the expression without max(ks, 0)
    m = mat.clone()
    m[..., 0:3] = 0.0
    case = dict(base, mat=m)
    up, want = _reference(case)
    _, free = _reference(case, clamp_ks=False)
    out = _apply(backend, device, case, up)
    _assert_parity(out, want, 'tie ks == 0')
    err = _worst_slice(out['d_material'][..., :3], 0.5 * free['d_material'][..., :3], 'ks == 0: half')
    assert float(free['d_material'][..., :3].abs().sum()) > 0 and err < parity_util.TOL, err
    # rho == 1e-3 exactly, the floor's tie.  e = 1998 there, beyond what fp32 powf holds to the bar against fp64, so the kernel
    # is compared with itself: one ulp above the floor the whole gradient passes, one ulp below none, at it half.  One ulp of
    # rho moves e by 2 ulp / r^2 = 2.3e-4 of 1998, and the gradient by about that share times |log cm| <= 0.02 here: far
    # inside the bar.  The normals are the half vectors (cm ~ 1), or pow(cm, 1998) underflows and there is nothing to halve.
    light = params[0:1].copy()
    p64, e64 = g[..., 0:3].double(), eye.double()[:, None, None, :]
    v = (e64 - p64) / (e64 - p64).norm(dim=-1, keepdim=True)
    l = torch.from_numpy(light[0, 3:6]).double() - p64
    l = l / l.norm(dim=-1, keepdim=True)
    half = (v + l) / (v + l).norm(dim=-1, keepdim=True)
    gt = g.clone()
    gt[..., 3:6] = (half * 1.25).float()
    runs = {}
    floor32 = np.float32(1e-3)
    for which, rho in (('at', floor32), ('above', np.nextafter(floor32, np.float32(1))), ('below', np.nextafter(floor32, np.float32(0)))):
        m = mat.clone()
        m[..., 3] = float(rho)
        runs[which] = _apply(backend, device, dict(base, g=gt, mat=m, types=[POINT], params=light, ranges=((0, 1),)), up)
        assert all(bool(torch.isfinite(t).all()) for t in runs[which].values())
    full = runs['above']['d_material'][..., 3].double()
    assert float(full.abs().sum()) > 0 and bool((runs['below']['d_material'][..., 3] == 0).all())
    err = float((runs['at']['d_material'][..., 3].double() - 0.5 * full).norm() / (0.5 * full).norm())
    print('tie rho == floor: %.2e' % err)
    assert err < parity_util.TOL, err


def test_tie_rule_hostsim(hostsim_backend):
    _run_tie_rule(hostsim_backend, CPU)


@pytest.mark.gpu
def test_tie_rule_gpu(gpu_backend):
    _run_tie_rule(gpu_backend, GPU)


# ---- 4. visibility --------------------------------------------------------------------------------------------------------------------
def _run_visibility(backend, device):
    ru = _ru()
    case = dict(_definition_case('grid_17x16_aa2_alpha1'))
    n, hg, wg = case['g'].shape[:3]
    words = torch.from_numpy(np.random.default_rng(41).integers(-2 ** 31, 2 ** 31, (n, hg, wg), dtype=np.int64))
    vis32 = words.to(torch.int32)
    up, want = _reference(case, vis=words & 0xffffffff)
    assert float((want['image'] - case['want']['image']).abs().sum()) > 0          # the mask removes light
    _assert_parity(_apply(backend, device, case, up, vis=vis32), want, 'random visibility words')
    ones = _apply(backend, device, case, up, vis=torch.full((n, hg, wg), -1, dtype=torch.int32))
    plain = _apply(backend, device, case, up)
    for k in plain:
        assert torch.equal(ones[k], plain[k]), k
    # 33 lights fit no word; without words they are fine
    many = dict(case, types=[POINT] * 33, params=light_rows(42, [POINT] * 33), ranges=((0, 33), (0, 1)))
    _apply(backend, device, many, up)
    with pytest.raises(RuntimeError, match='image 0 has 33 lights, at most 32'):
        _apply(backend, device, many, up, vis=vis32)
    with pytest.raises(RuntimeError, match='visibility must be'):
        ru.DeferredSpecular.apply(case['g'].to(device), case['mat'].to(device), case['eye'].to(device),
                                  torch.from_numpy(case['params']).to(device), tuple(case['types']), case['ranges'], case['aa'],
                                  True, backend, vis32[:, :-1].to(device))


def test_visibility_hostsim(hostsim_backend):
    _run_visibility(hostsim_backend, CPU)


@pytest.mark.gpu
def test_visibility_gpu(gpu_backend):
    _run_visibility(gpu_backend, GPU)


# ---- 5. end to end --------------------------------------------------------------------------------------------------------------------
def _sphere_over_plane(device, resolution, camera_type=0):
    """a smooth-shaded sphere over a floor, both glossy; the camera looks down at them"""
    from redner_amd.render_pytorch import AreaLight, Camera, Material, Scene, Shape
    t = lambda x, dev=device, dtype=torch.float32, grad=False: torch.tensor(x, dtype=dtype, device=dev).requires_grad_(grad)
    cam = Camera(position=t([0.2, 2.5, -4.0], 'cpu', grad=True), look_at=t([0.0, -0.2, 0.0], 'cpu'), up=t([0.0, 1.0, 0.0], 'cpu'),
                 fov=t([40.0], 'cpu'), clip_near=1e-2, resolution=resolution, camera_type=camera_type)
    nu, nv, radius = 16, 10, 0.7
    verts, tris = [], []
    for j in range(nv + 1):
        th = math.pi * j / nv
        for i in range(nu + 1):
            ph = 2 * math.pi * i / nu
            verts.append([radius * math.sin(th) * math.cos(ph), radius * math.cos(th), radius * math.sin(th) * math.sin(ph)])
    for j in range(nv):
        for i in range(nu):
            a, b = j * (nu + 1) + i, j * (nu + 1) + i + 1
            c, d = a + nu + 1, b + nu + 1
            if j > 0:
                tris.append([a, b, c])
            if j < nv - 1:
                tris.append([b, d, c])
    verts = np.asarray(verts, np.float32)
    normals = verts / np.linalg.norm(verts, axis=1, keepdims=True)
    sphere = Shape(t(verts.tolist(), grad=True), t(tris, dtype=torch.int32), 0, normals=t(normals.tolist()))
    floor = Shape(t([[-3.0, -0.9, -3.0], [-3.0, -0.9, 3.0], [3.0, -0.9, -3.0], [3.0, -0.9, 3.0]], grad=True),
                  t([[0, 1, 2], [1, 3, 2]], dtype=torch.int32), 1)
    far = Shape(t([[-1.0, 30.0, -1.0], [1.0, 30.0, -1.0], [-1.0, 30.0, 1.0]]), t([[0, 1, 2]], dtype=torch.int32), 2)
    mats = [Material(diffuse_reflectance=t([0.4, 0.3, 0.2]), specular_reflectance=t([0.6, 0.7, 0.8], grad=True),
                     roughness=t([0.15], grad=True)),
            Material(diffuse_reflectance=t([0.3, 0.35, 0.4]), specular_reflectance=t([0.5, 0.5, 0.5], grad=True),
                     roughness=t([0.3], grad=True)),
            Material(diffuse_reflectance=t([0.0, 0.0, 0.0]))]
    return Scene(cam, [sphere, floor, far], mats, [AreaLight(2, t([1.0, 1.0, 1.0], 'cpu'))])


def _e2e_lights(ru):
    intensity = torch.tensor([12.0, 11.0, 10.0], requires_grad=True)
    return intensity, [ru.PointLight(torch.tensor([1.5, 3.0, -1.0]), intensity),
                       ru.DirectionalLight(torch.tensor([-0.4, -1.0, 0.6]), torch.tensor([0.8, 0.9, 1.0]))]


def _cam_to_world_scene(device, resolution):
    """the sphere over the plane seen by the same camera, given as a cam_to_world matrix (a leaf that requires a gradient): columns
    x = normalize(cross(d, up)), y = cross(x, d), d = normalize(look_at - position), position"""
    from redner_amd.render_pytorch import Camera
    sc = _sphere_over_plane(device, resolution)
    cam = sc.camera
    pos = cam.position.detach()
    d = (cam.look_at - pos) / (cam.look_at - pos).norm()
    x = torch.cross(d, cam.up, dim=0)
    x = x / x.norm()
    matrix = torch.eye(4)
    matrix[:3, 0], matrix[:3, 1], matrix[:3, 2], matrix[:3, 3] = x, torch.cross(x, d, dim=0), d, pos
    sc.camera = Camera(fov=torch.tensor([40.0]), clip_near=1e-2, resolution=resolution, cam_to_world=matrix.contiguous().requires_grad_(True))
    return sc


def _run_cam_to_world(backend, device, monkeypatch):
    """render_utils._eye_of takes the translation column of a cam_to_world as the eye: the image is the diffuse image + the
    definition's lobe with that eye, and the eye's share of the gradient arrives in that column."""
    from test_schedule_matrix import GPU_BAR
    ru = _ru()
    res, aa, seed = 32, 2, 5
    _, lights = _e2e_lights(ru)
    sc = _cam_to_world_scene(device, (res, res))
    img = ru.render_deferred(sc, lights, aa_samples=aa, seed=seed, device=device, backend=backend, specular=True)
    up = mk.upstream(img.shape).to(device)
    (img * up).sum().backward()
    # the look-at camera it was made from gives the same picture (the matrix is rounded to fp32: not the same bits)
    look_at = ru.render_deferred(_sphere_over_plane(device, (res, res)), lights, aa_samples=aa, seed=seed, device=device,
                                 backend=backend, specular=True).detach()
    same = _worst_slice(img.detach().cpu()[None], look_at.cpu().double()[None], 'cam_to_world against look-at')
    print('cam_to_world against the look-at camera: %.2e' % same)
    assert same < parity_util.TOL, same
    # = the diffuse image + the definition's lobe on render_g_buffer's own channels, the eye being the translation column
    ch = [backend.channels.position, backend.channels.shading_normal, backend.channels.diffuse_reflectance,
          backend.channels.specular_reflectance, backend.channels.roughness]
    sc2 = _cam_to_world_scene(device, (res * aa, res * aa))
    gb = ru.render_g_buffer(sc2, ch, seed=seed, device=device, backend=backend).detach().cpu().unsqueeze(0)
    diffuse = ru.render_deferred(_cam_to_world_scene(device, (res, res)), lights, aa_samples=aa, seed=seed, device=device,
                                 backend=backend).detach().cpu()
    params, types = ru.pack_lights(lights, CPU)
    lobe, _ = lobe64(gb[..., :9].double(), gb[..., 9:13].double(), sc2.camera.cam_to_world.detach()[:3, 3].double().reshape(1, 3),
                     types, params.detach().double(), ((0, 2),), aa)
    assert float(lobe.abs().sum()) > 0.01 * float(diffuse.abs().sum())
    err = _worst_slice(img.detach().cpu()[None], diffuse.double()[None] + lobe, 'cam_to_world end to end')
    print('cam_to_world end to end: %.2e' % err)
    assert err < parity_util.TOL, err
    # the eye's share of the gradient: with _eye_of handing out a fresh leaf of the same values, that leaf's gradient + what
    # reaches the column through the G-buffer render is what reached the column before.  The two sides differ in the order of
    # two or three fp32 additions and, on the GPU, by the renderer's run-to-run bar
    whole = sc.camera.cam_to_world.grad[:3, 3].clone()
    sc_p = _cam_to_world_scene(device, (res, res))
    eye = sc_p.camera.cam_to_world.detach()[:3, 3].clone().requires_grad_(True)
    with monkeypatch.context() as patch:
        patch.setattr(ru, '_eye_of', lambda camera, rd: eye)
        img_p = ru.render_deferred(sc_p, lights, aa_samples=aa, seed=seed, device=device, backend=backend, specular=True)
    assert torch.equal(img_p.detach(), img.detach())
    (img_p * up).sum().backward()
    rest = sc_p.camera.cam_to_world.grad[:3, 3]
    assert float(eye.grad.abs().sum()) > 0 and float(rest.abs().sum()) > 0 and float(whole.abs().sum()) > 0
    d, n = float((eye.grad.double() + rest.double() - whole.double()).norm()), float(whole.double().norm())
    print('the eye\'s share %s + the rest %s against the column %s: %.2e of GPU_BAR %.0e' % (eye.grad.tolist(), rest.tolist(), whole.tolist(), d / n, GPU_BAR))
    assert d <= GPU_BAR * n, (d / n, GPU_BAR)
    assert not torch.equal(rest, whole)


def _run_end_to_end(backend, device, monkeypatch):
    ru = _ru()
    res, aa, seed = 32, 2, 5
    _run_cam_to_world(backend, device, monkeypatch)
    sc = _sphere_over_plane(device, (res, res))
    intensity, lights = _e2e_lights(ru)
    img = ru.render_deferred(sc, lights, aa_samples=aa, seed=seed, device=device, backend=backend, specular=True)
    assert tuple(img.shape) == (res, res, 3)
    (img * mk.upstream(img.shape).to(device)).sum().backward()
    reached = {'sphere ks': sc.materials[0].specular_reflectance.mipmap[0], 'sphere roughness': sc.materials[0].roughness.mipmap[0],
               'floor ks': sc.materials[1].specular_reflectance.mipmap[0], 'floor roughness': sc.materials[1].roughness.mipmap[0],
               'sphere vertices': sc.shapes[0].vertices, 'camera position': sc.camera.position, 'intensity': intensity}
    for what, t in reached.items():
        assert t.grad is not None and bool(torch.isfinite(t.grad).all()), what
    for what in ('sphere ks', 'sphere roughness', 'floor ks', 'floor roughness'):
        assert float(reached[what].grad.abs().sum()) > 0, what
    # = the diffuse image + the definition's lobe on render_g_buffer's own channels
    sc2 = _sphere_over_plane(device, (res * aa, res * aa))
    _, lights2 = _e2e_lights(ru)
    ch = [backend.channels.position, backend.channels.shading_normal, backend.channels.diffuse_reflectance,
          backend.channels.specular_reflectance, backend.channels.roughness]
    gb = ru.render_g_buffer(sc2, ch, seed=seed, device=device, backend=backend).detach().cpu().unsqueeze(0)
    sc3 = _sphere_over_plane(device, (res, res))
    diffuse = ru.render_deferred(sc3, lights2, aa_samples=aa, seed=seed, device=device, backend=backend).detach().cpu()
    params, types = ru.pack_lights(lights2, CPU)
    lobe, _ = lobe64(gb[..., :9].double(), gb[..., 9:13].double(), sc2.camera.position.detach().double().reshape(1, 3), types,
                     params.detach().double(), ((0, 2),), aa)
    assert float(lobe.abs().sum()) > 0.01 * float(diffuse.abs().sum())             # there are highlights to speak of
    err = _worst_slice(img.detach().cpu()[None], diffuse.double()[None] + lobe, 'end to end')
    print('end to end: %.2e' % err)
    assert err < parity_util.TOL, err
    # specular=False: the bits of a call without the argument
    off = ru.render_deferred(sc3, lights2, aa_samples=aa, seed=seed, device=device, backend=backend, specular=False)
    assert torch.equal(off.detach().cpu(), diffuse)
    # shadows: a floor texel in the sphere's shadow of the point light has no highlight from it
    _, point_only = _e2e_lights(ru)
    point_only = point_only[:1]
    lit = ru.render_deferred(sc3, point_only, aa_samples=1, seed=seed, device=device, backend=backend, specular=True).detach().cpu()
    dark = ru.render_deferred(sc3, point_only, aa_samples=1, seed=seed, device=device, backend=backend, specular=True,
                              shadows=True).detach().cpu()
    no_lobe = ru.render_deferred(sc3, point_only, aa_samples=1, seed=seed, device=device, backend=backend,
                                 shadows=True).detach().cpu()
    g1 = ru.render_g_buffer(sc3, ch[:3], seed=seed, device=device, backend=backend).detach()
    _, words = ru.deferred_shade(g1.unsqueeze(0), point_only, aa_samples=1, backend=backend,
                                 occluders=ru.occluder_scene(sc3, device=device, backend=backend), return_visibility=True)
    blocked = (words[0].cpu() & 1) == 0
    assert int(blocked.sum()) >= 8
    assert bool((dark[blocked] == 0).all()) and torch.equal(dark[blocked], no_lobe[blocked])
    assert torch.equal(dark[~blocked], lit[~blocked]) and float((lit[blocked] - no_lobe[blocked]).abs().sum()) > 0
    # with alpha, shadows and ambient occlusion at once: alpha is the diffuse pass's, the highlights only add light; and a batch
    # of two scenes gives each scene's own image
    every = lights2 + [ru.AmbientLight(torch.tensor([0.1, 0.1, 0.1]))]
    kw = dict(alpha=True, aa_samples=aa, seed=seed, device=device, backend=backend, shadows=True, ambient_occlusion=4, ao_radius=1.0)
    with_lobe, without = ru.render_deferred(sc3, every, specular=True, **kw).detach(), ru.render_deferred(sc3, every, **kw).detach()
    assert tuple(with_lobe.shape) == (res, res, 4) and torch.equal(with_lobe[..., 3], without[..., 3])
    assert float((with_lobe[..., :3] - without[..., :3]).min()) >= 0 and float((with_lobe - without).sum()) > 0
    batch = ru.render_deferred([sc3, _sphere_over_plane(device, (res, res))], lights2, aa_samples=aa, seed=[seed, seed], device=device,
                               backend=backend, specular=True)
    assert torch.equal(batch[0], img.detach()) and torch.equal(batch[1], img.detach())
    # an orthographic camera has no eye point
    with pytest.raises(RuntimeError, match='orthographic'):
        ru.render_deferred(_sphere_over_plane(device, (res, res), camera_type=1), lights2, aa_samples=aa, seed=seed, device=device,
                           backend=backend, specular=True)


def test_end_to_end_hostsim(hostsim_backend, monkeypatch):
    _run_end_to_end(hostsim_backend, CPU, monkeypatch)


@pytest.mark.gpu
def test_end_to_end_gpu(gpu_backend, monkeypatch):
    _run_end_to_end(gpu_backend, GPU, monkeypatch)


# ---- 6. calling contract --------------------------------------------------------------------------------------------------------------
def _strided(x, device):
    view = torch.full(tuple(reversed(x.shape)), 7.0, device=device).permute(*reversed(range(x.dim())))
    view.copy_(x)
    assert not view.is_contiguous()
    return view


def _offset(x, device):
    view = torch.full((x.numel() + 1,), 7.0, device=device)[1:].view(x.shape)
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


def _run_calling_contract(backend, device):
    ru = _ru()
    case = _definition_case('grid_5x7_aa2_alpha1')
    up = case['up'].to(device)
    params = torch.from_numpy(case['params']).to(device)

    def run(place=None, upstream=up, edit=None):
        tensors = {k: (place or {}).get(k, lambda x, d: x.clone().to(d))(case[k], device).requires_grad_(True)
                   for k in ('g', 'mat', 'eye')}
        pl = params.clone().requires_grad_(True)
        img = ru.DeferredSpecular.apply(tensors['g'], tensors['mat'], tensors['eye'], pl, tuple(case['types']), case['ranges'],
                                        case['aa'], True, backend)
        if edit:
            with torch.no_grad():
                tensors[edit].mul_(2.0)
        if upstream is None:
            img.sum().backward()                          # autograd's stride-0 expanded ones
        elif callable(upstream):
            upstream(img)
        else:
            img.backward(upstream)
        return [img.detach()] + [tensors[k].grad for k in ('g', 'mat', 'eye')] + [pl.grad]

    plain = run()
    for name in ('g', 'mat', 'eye'):
        for placing in (_strided, _offset):
            for a, b in zip(run({name: placing}), plain):
                assert torch.equal(a, b), (name, placing.__name__)
    for a, b in zip(run({k: _strided for k in ('g', 'mat', 'eye')}), plain):
        assert torch.equal(a, b)
    ones = torch.ones_like(plain[0])
    for a, b in zip(run(upstream=None), run(upstream=ones)):
        assert torch.equal(a, b)
    weight = _strided(up, device)
    for a, b in zip(run(upstream=lambda img: img.backward(weight)), plain):
        assert torch.equal(a, b)
    for name in ('g', 'mat', 'eye'):
        with pytest.raises(RuntimeError, match=INPLACE):                # a saved contiguous input, edited before backward
            run(edit=name)
        for a, b in zip(run({name: _strided}, edit=name), plain):          # the op read a private copy: the plain gradient
            assert torch.equal(a, b), name
    # through the public function: light lists, a [3] eye for all images, lights and eye on the host
    lights = mk.lights_from_table(ru, case['types'][1:2] + case['types'][3:5], case['params'][[1, 3, 4]])
    eye = case['eye'][0].clone().requires_grad_(True)
    gl = case['g'].clone().to(device).requires_grad_(True)
    img = ru.deferred_specular(gl, case['mat'].to(device), lights, eye, alpha=True, aa_samples=case['aa'], backend=backend)
    img.backward(up)
    assert tuple(img.shape) == (2, 5, 7, 3) and eye.grad.device.type == 'cpu' and float(eye.grad.abs().sum()) > 0
    assert all(getattr(light, f).grad is not None for light in lights for f in ('intensity',))


def test_calling_contract_hostsim(hostsim_backend):
    _run_calling_contract(hostsim_backend, CPU)


@pytest.mark.gpu
def test_calling_contract_gpu(gpu_backend):
    _run_calling_contract(gpu_backend, GPU)


# ---- 7. reproducibility ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_light_and_eye_gradients_bitwise_reproducible_gpu(gpu_backend):
    """d_light_params and d_eye are sums over every texel: per-block fp64 partials folded in a fixed order, no atomics."""
    case = _definition_case(PLAN_CASE)
    runs = [_apply(gpu_backend, GPU, case, case['up']) for _ in range(2)]
    for k in ('d_light_params', 'd_eye'):
        assert float(runs[0][k].abs().sum()) > 0
        assert runs[0][k].numpy().tobytes() == runs[1][k].numpy().tobytes(), k


# ---- 8. errors and the binding ----------------------------------------------------------------------------------------------------
def _run_errors(rd, device):
    ru = _ru()
    from redner_amd import _capi
    case = _definition_case('grid_5x7_aa2_alpha1')
    g, mat, eye = case['g'].to(device), case['mat'].to(device), case['eye'].to(device)
    params = torch.from_numpy(case['params']).to(device)
    elsewhere = torch.device('meta') if device.type == 'cpu' else CPU
    args = lambda **kw: [kw.get('g', g), kw.get('mat', mat), kw.get('eye', eye), kw.get('params', params), tuple(case['types']),
                         case['ranges'], case['aa'], kw.get('alpha', True), rd]
    ru.DeferredSpecular.apply(*args())
    for what, bad in (('G-buffer must be', dict(g=g[..., :9])), ('G-buffer must be', dict(alpha=False)),
                      ('material must be', dict(mat=mat[..., :3])), ('material must be', dict(mat=mat[:, :-1])),
                      ('eye must be', dict(eye=eye[0])), ('eye must be', dict(eye=eye[:, :2])),
                      ('light_params must be', dict(params=params[:, :9])),
                      ('fp32 tensors only', dict(g=g.double())), ('fp32 tensors only', dict(mat=mat.double())),
                      ('fp32 tensors only', dict(eye=eye.double())), ('fp32 tensors only', dict(params=params.double())),
                      ('the material is on', dict(mat=mat.to(elsewhere)))):
        with pytest.raises(RuntimeError, match=what):
            ru.DeferredSpecular.apply(*args(**bad))
    # the C ABI: the ao fields and occluders must be zero, a null tensor and a misaligned material are refused
    lib = _capi.lib()
    keep = [(ctypes.c_int32 * 7)(*case['types']), (ctypes.c_int32 * 4)(0, 7, 1, 5), (ctypes.c_void_p * 2)(),
            torch.full((2, 10, 14), -1, dtype=torch.int32, device=device)]
    image = torch.empty(2, 5, 7, 3, device=device)

    def call(m=mat, **fields):
        desc = _capi.DeferredDesc()
        desc.num_images, desc.height, desc.width, desc.aa_samples, desc.alpha, desc.num_lights = 2, 5, 7, 2, 1, 7
        desc.light_type, desc.image_light_range, desc.gpu_index = keep[0], keep[1], -1 if device.type == 'cpu' else 0
        for field, value in fields.items():
            setattr(desc, field, value)
        return lib.rdr_deferred_specular(ctypes.byref(desc), g.data_ptr(), m.data_ptr(), eye.data_ptr(), params.data_ptr(),
                                         image.data_ptr()), desc

    assert call()[0] == 0 and _capi.last_error() == ''
    for fields in (dict(ao_rays=4), dict(ao_words=keep[3].data_ptr()), dict(ao_occluders=keep[2]), dict(occluders=keep[2])):
        assert call(**fields)[0] == 1 and 'must be zero' in _capi.last_error(), fields
    assert call(visibility=keep[3].data_ptr())[0] == 0
    desc = call()[1]
    assert call(torch.zeros(mat.numel() + 1, device=device)[1:])[0] == 1 and '16-byte aligned' in _capi.last_error()
    assert lib.rdr_deferred_specular(None, None, None, None, None, None) == 1 and 'description' in _capi.last_error()
    assert lib.rdr_deferred_specular(ctypes.byref(desc), g.data_ptr(), None, eye.data_ptr(), params.data_ptr(), image.data_ptr()) == 1
    assert 'null tensor' in _capi.last_error()
    assert lib.rdr_deferred_specular_backward(ctypes.byref(desc), *[None] * 9) == 1 and 'null tensor' in _capi.last_error()


def test_errors_hostsim(hostsim_backend):
    _run_errors(hostsim_backend, CPU)


@pytest.mark.gpu
def test_errors_gpu(gpu_backend):
    _run_errors(gpu_backend, GPU)


def test_binding_matches_the_header(hostsim_backend):
    """csrc/deferred_specular_abi.h, its table in _capi and the libraries' exports say the same (what tests/test_capi.py holds the
    headers under include/ to)."""
    from conftest import HOSTSIM_LIB
    from redner_amd import _capi
    from test_capi import declared_signatures
    header = os.path.join('..', 'redner_amd', 'csrc', 'deferred_specular_abi.h')
    declared, table = declared_signatures(header), _capi.CSRC_HEADERS['deferred_specular_abi.h']
    assert sorted(declared) == ['rdr_deferred_specular', 'rdr_deferred_specular_backward'] == sorted(table)
    for name, count in declared.items():
        assert len(table[name][1]) == count, name
        assert not any(name in others for others in _capi.HEADERS.values())
    for path in (HOSTSIM_LIB, _capi.DEFAULT_LIBRARY, _capi.EXACT_LIBRARY):
        if path == HOSTSIM_LIB or os.path.exists(path):
            lib = ctypes.CDLL(path)
            assert all(hasattr(lib, name) for name in declared), path
    import redner_amd
    assert redner_amd.deferred_specular is _ru().deferred_specular and redner_amd.DeferredSpecular is _ru().DeferredSpecular
