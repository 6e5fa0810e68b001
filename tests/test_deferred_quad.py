"""Rectangular area lights in deferred shading (rdr_deferred_quad / _backward, csrc/deferred_quad.h;
redner_amd.render_utils.QuadLight, quad_light, DeferredQuad, deferred_quad, render_deferred with QuadLights).

The oracle is the definition of csrc/deferred_quad_abi.h written here in torch fp64 (`quad64`), with autograd for the gradients:
the image, d_g_buffer and d_quads are each held to parity_util.TOL (1e-4 relative L2 of the tensor's own norm) on the worst image
slice / quad row.  Gates are `where` on conditions, which autograd holds constant; max(S, 0) is torch.max of two tensors, which
splits the gradient at a tie; |S| is torch.abs, whose gradient at 0 is 0.

The texels are those of test_deferred_specular's generator (seeded): positions in [-1, 1]^2 x [-0.1, 0.1]; three quarters of the
normals in a cone about +z, a quarter uniform on the sphere, stored lengths in [0.5, 2]; one texel in sixteen is made a
background texel (normal 0).  Three quads (`three_quads`): one high above the patch near (-0.5, 0.4, 1.5) facing it; one low and
upright in the plane x = 0.3 with centre z = 0.25, which straddles many texels' horizons and is seen from both sides; one
two-sided, upright in the plane y = -0.2.

A texel is excluded (its normal set to 0: a background texel) only where some (texel, quad) pair has 0 < |S| < 1e-4, the kink of
the clamp: an fp32 sign on the other side than the exact one says nothing about the kernel.  A case asserts that at most 2 % of
its texels are excluded and that every class of (texel, quad) pair its quads can produce occurs; its seed is the first, counted
up from the case's own, for which the DEFINITION says so.

The 725 x 725 case, whose purpose is that the capped adjoint grid strides, is lit by the high quad alone.  Its half a million texels
are about 4e-6 apart in x, so under the upright quad some would lie within 1e-5 of the emitter's own plane inside its outline.
There the integral itself jumps (front against back), the two ends of the horizon arc are antipodal as seen from the texel, and
their cross product is formed by cancellation: the definition evaluated in fp32 TORCH misses the fp64 position gradient of such a
texel by a factor of ten (213 against -15.7 at 2.5e-6 from the plane), and one such texel outweighs the other 525 624 in the L2
norm.  That is a property of the closed form in fp32 on the emitter's own surface, which is out of scope,
not of the launch plan this case is about.  The grids, at most 4896 texels, hold no such texel for their seeds.

The closed forms of section 2 are the view factors of a differential element to a parallel and to a perpendicular rectangle as
the heat-transfer tables give them, not the contour integral.

Every case runs on the CPU harness; the GPU legs run the same bodies on both builds of the library."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import parity_util
import test_deferred_specular as t_spec
from golden import make_deferred_golden as mk
from test_deferred import ADJOINT_BLOCKS, _worst_slice

CPU, GPU = torch.device('cpu'), torch.device('cuda:0')
KINK = 1e-4                              # how near S == 0 a texel is excluded
INPLACE = 'modified by an inplace operation'
_cache = {}


def _ru():
    from redner_amd import render_utils
    return render_utils


# ---- the fp64 definition ------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a * b).sum(-1)


def _edge(A, B, nh):
    c = torch.cross(B, A, dim=-1)
    cc = _dot(c, c)
    ok = cc > 0
    s = torch.sqrt(torch.where(ok, cc, torch.ones_like(cc)))
    value = torch.atan2(s, _dot(A, B)) * _dot(c, nh) / s
    return torch.where(ok, value, torch.zeros_like(value))


def contour64(p, nh, corners):
    """p, nh [..., 3], corners [4, 3] -> S [...] and the number of corners above the horizon"""
    r = [corners[i] - p for i in range(4)]
    h = [_dot(nh, r[i]) for i in range(4)]
    S = torch.zeros_like(h[0])
    leave, enter = torch.zeros_like(p), torch.zeros_like(p)
    crossed = torch.zeros_like(h[0], dtype=torch.bool)
    for i in range(4):
        j = (i + 1) % 4
        A, B, hA, hB = r[i], r[j], h[i], h[j]
        upA, upB = hA > 0, hB > 0
        exits, enters = upA & ~upB, ~upA & upB
        cut = exits | enters
        den = torch.where(cut, hA - hB, torch.ones_like(hA))
        x = A + (B - A) * (hA / den)[..., None]
        e = _edge(torch.where(enters[..., None], x, A), torch.where(exits[..., None], x, B), nh)
        S = S + torch.where(upA | upB, e, torch.zeros_like(e))
        leave = torch.where(exits[..., None], x, leave)
        enter = torch.where(enters[..., None], x, enter)
        crossed = crossed | cut
    arc = _edge(leave, enter, nh)
    S = S + torch.where(crossed, arc, torch.zeros_like(arc))
    return S, sum((hi > 0).to(torch.int64) for hi in h)


def quad64(g, quads, flags, ranges, aa):
    """g [N, Hg, Wg, >= 9] and quads [Q, 16] in torch double -> (image [N, H, W, 3], report).  report: per (texel, quad) pair that
    is shaded, how many corners are up and the sign of S; which texels are within KINK of S == 0; the background texels."""
    n, hg, wg, _ = g.shape
    p, nrm, alb = g[..., 0:3], g[..., 3:6], g[..., 6:9]
    nn, pp = _dot(nrm, nrm), _dot(p, p)
    has = (nn > 0) & torch.isfinite(nn) & torch.isfinite(pp)
    nh = nrm / torch.sqrt(torch.where(has, nn, torch.ones_like(nn)))[..., None]
    nh = torch.where(has[..., None], nh, torch.zeros_like(nh))
    ps = torch.where(has[..., None], p, torch.zeros_like(p))
    rgb = torch.zeros(n, hg, wg, 3, dtype=torch.float64)
    near = torch.zeros(n, hg, wg, dtype=torch.bool)
    classes = {}
    for qi, two_sided in enumerate(flags):
        uses = torch.tensor([b <= qi < e for b, e in ranges])
        if not bool(uses.any()):
            continue
        shaded = uses[:, None, None].expand(n, hg, wg) & has
        S, up = contour64(ps, nh, quads[qi, :12].reshape(4, 3))
        F = (S.abs() if two_sided else torch.max(S, torch.zeros_like(S))) / 2.0
        value = quads[qi, 12:15] * (alb / math.pi) * F[..., None]
        rgb = rgb + torch.where(shaded[..., None], value, torch.zeros_like(value))
        with torch.no_grad():
            near |= shaded & (S.abs() > 0) & (S.abs() < KINK)
            side = 'two_sided' if two_sided else 'one_sided'
            for k in range(5):
                classes['%d up' % k] = classes.get('%d up' % k, 0) + int((shaded & (up == k)).sum())
            for name, mask in (('S > 0', S > 0), ('S < 0', S < 0)):
                key = '%s %s' % (side, name)
                classes[key] = classes.get(key, 0) + int((shaded & mask).sum())
    classes['background'] = int((~has).sum())
    image = rgb.reshape(n, hg // aa, aa, wg // aa, aa, 3).mean(dim=(2, 4))
    return image, {'near': near, 'classes': classes}


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def generate(seed, n, h, w, aa, alpha):
    """test_deferred_specular's texels, one in sixteen of them a background texel -> g [n, h aa, w aa, 9 + alpha] fp32"""
    g, _, _ = t_spec.generate(seed, n, h, w, aa, alpha)
    background = torch.from_numpy(np.random.default_rng(seed + 77).uniform(size=tuple(g.shape[:3])) < 1.0 / 16.0)
    g[..., 3:6] = torch.where(background[..., None], torch.zeros(()), g[..., 3:6])
    return g


def _rect(origin, u, v, radiance, rng, jitter=0.05):
    """corners origin, origin + u, origin + u + v, origin + v (the emitting side is that of u x v), moved by the seed"""
    o, u, v = (np.asarray(t, np.float64) for t in (origin, u, v))
    o = o + jitter * rng.uniform(-1.0, 1.0, 3)
    row = np.zeros(16, np.float32)
    row[:12] = np.concatenate([o, o + u, o + u + v, o + v])
    row[12:15] = radiance * rng.uniform(0.5, 2.0, 3)
    return row


def three_quads(seed):
    """-> quads [3, 16] fp32 and their two_sided flags, by the module docstring"""
    rng = np.random.default_rng(seed)
    high = _rect([-1.0, 0.0, 1.5], [0.0, 0.8, 0.1], [1.0, 0.0, 0.1], 4.0, rng)           # u x v points down
    upright = _rect([0.3, -0.5, -0.15], [0.0, 1.0, 0.0], [0.05, 0.0, 0.8], 2.0, rng)      # ... towards +x
    both = _rect([-0.7, -0.2, 0.0], [0.0, 0.05, 0.8], [1.2, 0.0, 0.0], 2.0, rng)          # ... towards +y; two-sided
    return np.stack([high, upright, both]), (0, 0, 1)


SIZES = ((5, 7), (16, 16), (17, 16))
GRID_CASES = ['grid_%dx%d_aa%d_alpha%d' % (h, w, aa, alpha) for h, w in SIZES for aa in (1, 2, 3) for alpha in (0, 1)]
OTHER_CASES = ['empty_range']
PLAN_CASE = 'plan_725x725'


def _shape_of(name):
    """-> n, h, w, aa, alpha, which of the three quads, ranges"""
    if name.startswith('grid_'):
        size, aa, alpha = re.match(r'grid_(\d+x\d+)_aa(\d)_alpha(\d)', name).groups()
        h, w = (int(v) for v in size.split('x'))
        return 2, h, w, int(aa), int(alpha), (0, 1, 2), ((0, 3), (1, 2))
    if name == 'empty_range':
        return 2, 5, 7, 2, 0, (0, 1, 2), ((0, 3), (2, 2))
    assert name == PLAN_CASE             # the high quad: see the module docstring
    return 1, 725, 725, 1, 0, (0,), ((0, 1),)


def _wanted_classes(which):
    """the classes of (texel, quad) pair that the quads `which` of three_quads can produce: no texel is behind the high quad"""
    wanted = ['%d up' % k for k in range(5)] + ['background', 'one_sided S > 0']
    if 1 in which:
        wanted += ['one_sided S < 0']
    if 2 in which:
        wanted += ['two_sided S < 0']
    return wanted


def _build_case(name):
    n, h, w, aa, alpha, which, ranges = _shape_of(name)
    base = 700 + sum(ord(ch) * (k + 1) for k, ch in enumerate(name)) % 1000
    texels = n * h * aa * w * aa
    for seed in range(base, base + 200):
        g = generate(seed, n, h, w, aa, alpha)
        rows, all_flags = three_quads(seed + 5000)
        quads, flags = rows[list(which)], tuple(all_flags[k] for k in which)
        with torch.no_grad():
            _, report = quad64(g.double(), torch.from_numpy(quads).double(), flags, ranges, aa)
        excluded = int(report['near'].sum())
        g[..., 3:6] = torch.where(report['near'][..., None], torch.zeros(()), g[..., 3:6])
        with torch.no_grad():
            _, report = quad64(g.double(), torch.from_numpy(quads).double(), flags, ranges, aa)
        if excluded <= 0.02 * texels and all(report['classes'][c] > 0 for c in _wanted_classes(which)):
            break
    else:
        raise AssertionError('no seed gives %s every class of pair' % name)
    return dict(g=g, quads=quads, flags=flags, ranges=ranges, aa=aa, alpha=alpha, texels=texels, excluded=excluded, report=report,
                which=which, seed=seed, n=n, h=h, w=w)


def _reference(case):
    """the fp64 image and the two gradients for the case's upstream gradient"""
    g = case['g'].double().requires_grad_(True)
    quads = torch.from_numpy(np.asarray(case['quads'], np.float32)).double().requires_grad_(True)
    img, _ = quad64(g, quads, case['flags'], case['ranges'], case['aa'])
    up = mk.upstream(img.shape)
    img.backward(up.double())
    want = {'image': img.detach(), 'd_g_buffer': g.grad, 'd_quads': quads.grad}
    assert all(bool(torch.isfinite(t).all()) for t in want.values())
    return up, want


def _definition_case(name):
    """inputs + the fp64 image and gradients, computed once and shared by the harness leg and the GPU legs of both builds"""
    if name not in _cache:
        case = _build_case(name)
        case['up'], case['want'] = _reference(case)
        _cache[name] = case
    return _cache[name]


def _apply(backend, device, case, up, g=None, quads=None):
    ru = _ru()
    gl = (case['g'] if g is None else g).clone().to(device).requires_grad_(True)
    ql = torch.from_numpy(np.asarray(case['quads'] if quads is None else quads, np.float32)).clone().to(device).requires_grad_(True)
    img = ru.DeferredQuad.apply(gl, ql, tuple(case['flags']), tuple(case['ranges']), case['aa'], bool(case['alpha']), backend)
    img.backward(up.to(device))
    return {'image': img.detach().cpu(), 'd_g_buffer': gl.grad.cpu(), 'd_quads': ql.grad.cpu()}


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
    assert all(report['classes'][c] > 0 for c in _wanted_classes(case['which'])), (name, report['classes'])
    assert int(report['near'].sum()) == 0
    if name == PLAN_CASE:                   # the capped adjoint grid strides
        assert (case['h'] * case['w'] + 255) // 256 > ADJOINT_BLOCKS
    if name == 'empty_range':
        assert any(b == e for b, e in case['ranges'])
    print('deferred_quad', name, tag, 'seed', case['seed'], 'excluded', case['excluded'], 'of', case['texels'], report['classes'])
    out = _apply(backend, device, case, case['up'])
    want = dict(case['want'])
    if case['alpha']:                       # the alpha channel of d_g_buffer: exactly zero
        assert bool((out['d_g_buffer'][..., 9] == 0).all())
    assert bool((out['d_quads'][:, 15] == 0).all())
    if name == 'empty_range':
        assert bool((out['image'][1] == 0).all()) and bool((out['d_g_buffer'][1] == 0).all())
    rep = {k: {'rel_l2': e, 'tol': parity_util.TOL, 'flipped_rows': 0} for k, e in _errors(out, want, name).items()}
    parity_util.record('deferred_quad_' + name, rep, tag)
    parity_util.assert_parity(rep, name)


@pytest.mark.parametrize('name', GRID_CASES + OTHER_CASES + [PLAN_CASE])
def test_definition_hostsim(hostsim_backend, name):
    _run_definition_case(hostsim_backend, CPU, name, 'hostsim')


@pytest.mark.gpu
@pytest.mark.parametrize('name', GRID_CASES + OTHER_CASES + [PLAN_CASE])
def test_definition_gpu(gpu_backend, name):
    _run_definition_case(gpu_backend, GPU, name, 'gpu')


# ---- 2. independent closed forms ------------------------------------------------------------------------------------------------------
def _parallel_view_factor(a, b, c):
    """a differential element to a parallel rectangle [0, a] x [0, b] at height c, one corner straight above the element"""
    A, B = a / c, b / c
    return (A / math.sqrt(1 + A * A) * math.atan(B / math.sqrt(1 + A * A)) +
            B / math.sqrt(1 + B * B) * math.atan(A / math.sqrt(1 + B * B))) / (2 * math.pi)


def _perpendicular_view_factor(a, b, c):
    """... to a rectangle [0, b] x [0, c] in the plane x = a that stands on the element's own plane"""
    Y = math.sqrt(a * a + c * c)
    return (math.atan(b / a) - a / Y * math.atan(b / Y)) / (2 * math.pi)


CLOSED_FORM_SIZES = ((1.0, 1.0, 1.0), (0.3, 2.0, 0.7), (2.5, 0.4, 1.1), (0.05, 0.08, 1.0), (3.0, 5.0, 0.2), (1.0, 0.2, 3.0))


def _run_closed_forms(backend, device):
    ru = _ru()
    texel = torch.tensor([[[[0.0, 0.0, 0.0, 0.0, 0.0, 2.0, 1.0, 1.0, 1.0]]]], device=device)
    one = torch.ones(3)
    for a, b, c in CLOSED_FORM_SIZES:
        walls = {
            'parallel': ([[0, 0, c], [0, b, c], [a, b, c], [a, 0, c]], _parallel_view_factor(a, b, c)),
            'perpendicular': ([[a, 0, 0], [a, 0, c], [a, b, c], [a, b, 0]], _perpendicular_view_factor(a, b, c)),
            'sunk': ([[a, 0, -c], [a, 0, c], [a, b, c], [a, b, -c]], _perpendicular_view_factor(a, b, c)),
        }
        for what, (corners, want) in walls.items():
            light = ru.QuadLight(torch.tensor(corners, dtype=torch.float32), one)
            got = ru.deferred_quad(texel, [light], backend=backend).cpu().double().reshape(3)
            err = float((got - want).abs().max()) / want
            print('closed form %s (%g, %g, %g): %.9f against %.9f, %.2e' % (what, a, b, c, float(got[0]), want, err))
            assert err < parity_util.TOL, (what, a, b, c, float(got[0]), want)


def test_closed_forms_hostsim(hostsim_backend):
    _run_closed_forms(hostsim_backend, CPU)


@pytest.mark.gpu
def test_closed_forms_gpu(gpu_backend):
    _run_closed_forms(gpu_backend, GPU)


# ---- 3. structure ---------------------------------------------------------------------------------------------------------------------
def _rotated(quads, k):
    """the corners of every row rotated by k places"""
    out = np.array(quads, np.float32, copy=True)
    out[:, :12] = np.roll(out[:, :12].reshape(-1, 4, 3), -k, axis=1).reshape(-1, 12)
    return out


def _reversed(quads):
    """the corners of every row in the opposite sense: q0, q3, q2, q1"""
    out = np.array(quads, np.float32, copy=True)
    out[:, :12] = out[:, :12].reshape(-1, 4, 3)[:, [0, 3, 2, 1]].reshape(-1, 12)
    return out


def _run_structure(backend, device):
    case = dict(_definition_case('grid_17x16_aa2_alpha1'))
    up = case['up']
    one = dict(case, quads=case['quads'][1:2], flags=(0,), ranges=((0, 1), (0, 1)))          # the upright quad, one-sided
    front = _apply(backend, device, one, up)
    # reversed winding: every texel that saw the front sees the back, and the other way round
    back = _apply(backend, device, dict(one, quads=_reversed(one['quads'])), up)
    g64 = one['g'].double()
    with torch.no_grad():
        nn = _dot(g64[..., 3:6], g64[..., 3:6])
        nh = g64[..., 3:6] / torch.sqrt(torch.where(nn > 0, nn, torch.ones_like(nn)))[..., None]
        S, _ = contour64(g64[..., 0:3], nh, torch.from_numpy(one['quads'][0, :12]).double().reshape(4, 3))
    sees_back = (S < -KINK) | (nn == 0)
    assert int(sees_back.sum()) > 50 and int((S > KINK).sum()) > 50
    aa = one['aa']
    whole_pixels = sees_back.reshape(2, 17, aa, 16, aa).all(dim=4).all(dim=2)
    assert int(whole_pixels.sum()) > 10
    assert bool((front['image'][whole_pixels] == 0).all()) and bool((front['d_g_buffer'][sees_back] == 0).all())
    assert bool((back['d_g_buffer'][(S > KINK) | (nn == 0)] == 0).all())
    everything_behind = dict(one, g=torch.where(sees_back[..., None], one['g'], torch.zeros(())))
    dark = _apply(backend, device, everything_behind, up)
    assert all(bool((t == 0).all()) for t in dark.values())
    # two-sided = the one-sided quad + its reversed copy
    both = _apply(backend, device, dict(one, flags=(1,)), up)
    total = {k: front[k].double() + back[k].double() for k in ('image', 'd_g_buffer')}
    total['d_quads'] = front['d_quads'].double().clone()
    total['d_quads'][:, :12] += torch.from_numpy(_reversed(back['d_quads'].numpy())[:, :12]).double()
    total['d_quads'][:, 12:15] += back['d_quads'][:, 12:15].double()
    assert float(front['image'].abs().sum()) > 0 and float(back['image'].abs().sum()) > 0
    _assert_parity(both, total, 'two-sided against front + back')
    # cyclic rotation of the corners: the same light, and the corner gradients rotate with it
    plain = _apply(backend, device, case, up)
    for k in (1, 2, 3):
        turned = _apply(backend, device, dict(case, quads=_rotated(case['quads'], k)), up)
        want = {'image': plain['image'].double(), 'd_g_buffer': plain['d_g_buffer'].double(),
                'd_quads': torch.from_numpy(_rotated(plain['d_quads'].numpy(), k)).double()}
        _assert_parity(turned, want, 'corners rotated by %d' % k)
    # two backward calls: the same bits
    again = _apply(backend, device, case, up)
    for k in plain:
        assert plain[k].numpy().tobytes() == again[k].numpy().tobytes(), k
    assert bool((plain['d_quads'][:, 15] == 0).all()) and bool((plain['d_g_buffer'][..., 9] == 0).all())
    assert float(plain['d_quads'][:, :15].abs().min()) > 0
    # NaN or inf in a texel's position or normal: that texel is exactly 0, every other texel is unchanged
    g = case['g'].clone()
    lit = torch.nonzero(plain['d_g_buffer'][..., :6].abs().sum(-1) > 0)          # six lit texels, spread over both images
    assert len(lit) > 600
    hit = torch.zeros(g.shape[:3], dtype=torch.bool)
    poison = ((0, float('nan')), (2, float('inf')), (1, float('-inf')), (3, float('nan')), (5, float('inf')), (4, float('-inf')))
    for k, (ch, value) in enumerate(poison):
        n, y, x = lit[(k * len(lit)) // 6 + 5].tolist()
        g[n, y, x, ch] = value
        hit[n, y, x] = True
    assert int(hit.sum()) == 6 and bool(hit[0].any()) and bool(hit[1].any())
    bad = _apply(backend, device, dict(case, g=g), up)
    assert all(bool(torch.isfinite(t).all()) for t in bad.values())
    assert bool((bad['d_g_buffer'][hit] == 0).all()) and torch.equal(bad['d_g_buffer'][~hit], plain['d_g_buffer'][~hit])
    clean = _apply(backend, device, dict(case, g=torch.where(hit[..., None], torch.zeros(()), case['g'])), up)
    assert torch.equal(bad['image'], clean['image']) and torch.equal(bad['d_quads'], clean['d_quads'])
    assert not torch.equal(bad['image'], plain['image'])


def test_structure_hostsim(hostsim_backend):
    _run_structure(hostsim_backend, CPU)


@pytest.mark.gpu
def test_structure_gpu(gpu_backend):
    _run_structure(gpu_backend, GPU)


# ---- 4. against the path tracer (CPU harness) ---------------------------------------------------------------------------------------
def _floor_under_a_quad(ru, device, resolution, position, look_at, size, radiance):
    """a diffuse floor in y = 0 that fills the frame of a camera looking straight down from y = 1, and above the camera the
    rectangle of quad_light as an emitter: the same four corners, triangles (0, 1, 3) and (1, 2, 3) -> scene, QuadLight"""
    from redner_amd.render_pytorch import AreaLight, Camera, Material, Scene, Shape
    t = lambda x, dev=device, dtype=torch.float32: torch.tensor(x, dtype=dtype, device=dev)
    light = ru.quad_light(t(position, 'cpu'), t(look_at, 'cpu'), t(size, 'cpu'), t(radiance, 'cpu'))
    cam = Camera(position=t([0.0, 1.0, 0.0], 'cpu'), look_at=t([0.0, 0.0, 0.0], 'cpu'), up=t([0.0, 0.0, 1.0], 'cpu'),
                 fov=t([50.0], 'cpu'), clip_near=1e-2, resolution=resolution)
    floor = Shape(t([[-3.0, 0.0, -3.0], [-3.0, 0.0, 3.0], [3.0, 0.0, -3.0], [3.0, 0.0, 3.0]]), t([[0, 1, 2], [1, 3, 2]], dtype=torch.int32), 0)
    emitter = Shape(light.vertices.to(device).contiguous(), t([[0, 1, 3], [1, 2, 3]], dtype=torch.int32), 1)
    mats = [Material(diffuse_reflectance=t([0.7, 0.5, 0.3])), Material(diffuse_reflectance=t([0.0, 0.0, 0.0]))]
    return Scene(cam, [floor, emitter], mats, [AreaLight(1, t(radiance, 'cpu'))]), light


def test_against_the_path_tracer_hostsim(hostsim_backend):
    """The frame mean of render_pathtracing (direct light only, 64 samples per pixel) over M = 8 seeds, per channel, lies within
    5 standard errors -- estimated from the 8 renders themselves -- of render_deferred with the QuadLight of the same rectangle.
    Measured: the deferred means (0.213683, 0.122105, 0.054947) against the path tracer's (0.213652, 0.122087, 0.054939), standard
    errors (2.8e-5, 1.6e-5, 7.2e-6; the Sobol' sampler): 1.1 standard errors apart in every channel, 1.4e-4 of the value.  No
    bias of the two pixel filters shows at that, so nothing is added to the bar."""
    ru = _ru()
    sc, light = _floor_under_a_quad(ru, CPU, (8, 8), [0.4, 2.0, -0.3], [0.1, 0.0, 0.2], [1.2, 0.8], [5.0, 4.0, 3.0])
    corners = light.vertices
    assert torch.allclose((corners[0] + corners[2]) / 2, torch.tensor([0.4, 2.0, -0.3]), atol=1e-6)
    facing = torch.cross(corners[1] - corners[0], corners[3] - corners[0], dim=0)
    assert float(facing @ (torch.tensor([0.1, 0.0, 0.2]) - torch.tensor([0.4, 2.0, -0.3]))) > 0          # it emits towards look_at
    deferred = ru.render_deferred(sc, [light], aa_samples=4, seed=3, device=CPU, backend=hostsim_backend).double()
    means = torch.stack([ru.render_pathtracing(sc, max_bounces=1, num_samples=(64, 1), seed=100 + m, device=CPU,
                                               backend=hostsim_backend).double().mean(dim=(0, 1)) for m in range(8)])
    mean, se = means.mean(0), means.std(0, unbiased=True) / math.sqrt(8)
    apart = (deferred.mean(dim=(0, 1)) - mean).abs() / se
    print('deferred', deferred.mean(dim=(0, 1)).tolist(), 'path tracer', mean.tolist(), 'standard error', se.tolist(), 'apart', apart.tolist())
    assert float(deferred.min()) > 0 and bool((se > 0).all())
    assert bool((apart < 5.0).all()), apart


# ---- 5. render_deferred ---------------------------------------------------------------------------------------------------------------
class _Recorder:
    """render_utils.deferred_shade / deferred_specular / deferred_quad, passed on and written down"""

    def __init__(self, ru, monkeypatch):
        self.calls = []
        for name in ('deferred_shade', 'deferred_specular', 'deferred_quad'):
            monkeypatch.setattr(ru, name, self._wrap(name, getattr(ru, name)))

    def _wrap(self, name, fn):
        def wrapped(*args, **kw):
            out = fn(*args, **kw)
            self.calls.append((name, args, kw, out))
            return out
        return wrapped

    def of(self, name):
        return [c for c in self.calls if c[0] == name]


def _quad_lights(ru, requires_grad=False, dtype=torch.float32):
    leaf = lambda x: torch.tensor(x, dtype=dtype, requires_grad=requires_grad)
    leaves = {'position': leaf([1.0, 2.5, -0.5]), 'look_at': leaf([0.0, -0.5, 0.2]), 'size': leaf([1.5, 1.0]), 'intensity': leaf([6.0, 5.0, 4.0])}
    return leaves, [ru.quad_light(leaves['position'], leaves['look_at'], leaves['size'], leaves['intensity']),
                    ru.QuadLight(torch.tensor([[-2.0, 0.5, 1.0], [-2.0, 1.5, 1.0], [-2.0, 1.5, -1.0], [-2.0, 0.5, -1.0]]),
                                 torch.tensor([1.0, 2.0, 3.0]), two_sided=True)]


def _run_render_deferred(backend, device, monkeypatch):
    ru = _ru()
    res, aa, seed = 16, 2, 5
    scene = lambda: t_spec._sphere_over_plane(device, (res, res))
    _, table_lights = t_spec._e2e_lights(ru)
    _, quads = _quad_lights(ru)
    kw = dict(aa_samples=aa, seed=seed, device=device, backend=backend)
    with monkeypatch.context() as patch:
        rec = _Recorder(ru, patch)
        # a mixed list, with alpha: deferred_shade of the table lights + deferred_quad of the quads, bit for bit
        mixed = ru.render_deferred(scene(), [quads[0], table_lights[0], quads[1], table_lights[1]], alpha=True, **kw).detach()
        (_, s_args, s_kw, s_out), = rec.of('deferred_shade')
        (_, q_args, q_kw, q_out), = rec.of('deferred_quad')
        assert list(s_args[1]) == table_lights and list(q_args[1]) == quads and not rec.of('deferred_specular')
        assert torch.equal(s_args[0], q_args[0]) and s_args[0].shape[-1] == 10 and tuple(q_out.shape) == (1, res, res, 3)
        assert torch.equal(mixed[..., :3], (s_out[0][..., :3] + q_out[0]).detach()) and torch.equal(mixed[..., 3], s_out[0][..., 3].detach())
        assert float(q_out.detach().abs().sum()) > 0.01 * float(s_out[..., :3].detach().abs().sum())
        quad_term = q_out.detach().clone()
        # no QuadLight: the calls and the bits of deferred_shade alone
        rec.calls.clear()
        plain = ru.render_deferred(scene(), table_lights, alpha=True, **kw).detach()
        assert not rec.of('deferred_quad') and len(rec.of('deferred_shade')) == 1
        assert rec.of('deferred_shade')[0][1][1] is table_lights and torch.equal(plain, s_out[0].detach())
        # shadows, ambient occlusion and specular leave the quad term's bits alone: it is added last, to what they give without it
        for extra in (dict(shadows=True), dict(ambient_occlusion=4, ao_radius=1.0), dict(specular=True),
                      dict(shadows=True, ambient_occlusion=4, ao_radius=1.0, specular=True)):
            every = table_lights + [ru.AmbientLight(torch.tensor([0.1, 0.1, 0.1]))]
            rec.calls.clear()
            with_quads = ru.render_deferred(scene(), every + quads, alpha=True, **kw, **extra).detach()
            (_, q_args, _, q_out), = rec.of('deferred_quad')
            assert torch.equal(q_out.detach(), quad_term) and q_args[0].shape[-1] == 10, extra
            without = ru.render_deferred(scene(), every, alpha=True, **kw, **extra).detach()
            assert torch.equal(with_quads[..., :3], without[..., :3] + quad_term[0]) and torch.equal(with_quads[..., 3], without[..., 3]), extra
        # per-image lists, one image without a quad
        rec.calls.clear()
        batch = ru.render_deferred([scene(), scene()], [[table_lights[0], quads[0]], [table_lights[1]]], seed=[seed, seed],
                                   aa_samples=aa, device=device, backend=backend).detach()
        (_, q_args, _, q_out), = rec.of('deferred_quad')
        assert [len(l) for l in q_args[1]] == [1, 0] and bool((q_out[1] == 0).all()) and float(q_out[0].detach().abs().sum()) > 0
        first = ru.render_deferred(scene(), [table_lights[0], quads[0]], **kw).detach()
        second = ru.render_deferred(scene(), [table_lights[1]], **kw).detach()
        assert torch.equal(batch[0], first) and torch.equal(batch[1], second)
        # only quads
        only = ru.render_deferred(scene(), quads, **kw).detach()
        assert torch.equal(only, quad_term[0])
    # gradients reach quad_light's position, look_at, size and intensity, and agree with the fp64 composition on the same G-buffer
    leaves, lights = _quad_lights(ru, requires_grad=True)
    sc = scene()
    img = ru.render_deferred(sc, lights, **kw)
    up = mk.upstream(img.shape)
    (img * up.to(device)).sum().backward()
    assert sc.shapes[0].vertices.grad is not None and float(sc.shapes[0].vertices.grad.abs().sum()) > 0
    big = t_spec._sphere_over_plane(device, (res * aa, res * aa))
    ch = [backend.channels.position, backend.channels.shading_normal, backend.channels.diffuse_reflectance]
    gb = ru.render_g_buffer(big, ch, seed=seed, device=device, backend=backend).detach().cpu().double().unsqueeze(0)
    leaves64, lights64 = _quad_lights(ru, requires_grad=True, dtype=torch.float64)
    table, flags = ru.pack_quads(lights64, CPU)            # (packs to fp32: the fp64 table is made here)
    table64 = torch.cat([torch.cat([l.vertices.reshape(-1), torch.as_tensor(l.intensity).double().reshape(-1), torch.zeros(1, dtype=torch.float64)])
                         for l in lights64]).reshape(2, 16)
    img64, _ = quad64(gb, table64, tuple(flags), ((0, 2),), aa)
    (img64[0] * up.double()).sum().backward()
    err = _worst_slice(img.detach().cpu()[None], img64.detach(), 'render_deferred with quads')
    print('render_deferred with quads: image %.2e' % err)
    assert err < parity_util.TOL
    for name, leaf in leaves.items():
        want = leaves64[name].grad
        got = leaf.grad.double()
        rel = float((got - want).norm() / want.norm())
        print('d %s: %s against %s, %.2e' % (name, got.tolist(), want.tolist(), rel))
        assert float(want.norm()) > 0 and rel < parity_util.TOL, (name, rel)


def test_render_deferred_hostsim(hostsim_backend, monkeypatch):
    _run_render_deferred(hostsim_backend, CPU, monkeypatch)


@pytest.mark.gpu
def test_render_deferred_gpu(gpu_backend, monkeypatch):
    _run_render_deferred(gpu_backend, GPU, monkeypatch)


def test_quad_light_is_the_emitter_rectangle():
    """quad_light's corners: the rectangle of `size` centred at `position` in the plane through it whose normal is the direction
    to `look_at`, emitting towards look_at, in the frame x = (1 - dx dx a, b, -dx), y = (b, 1 - dy dy a, -dy); at the pole the
    frame is (0, -1, 0), (-1, 0, 0).  QuadLight.render goes through the native call (test_closed_forms_*)."""
    ru = _ru()
    for position, look_at, size in (([0.4, 2.0, -0.3], [0.1, 0.0, 0.2], [1.2, 0.8]), ([0.0, 0.0, 3.0], [0.0, 0.0, 0.0], [2.0, 1.0]),
                                    ([1.0, 1.0, 1.0], [4.0, -2.0, 2.5], [0.3, 0.7])):
        p, l, s = (torch.tensor(v, dtype=torch.float64) for v in (position, look_at, size))
        q = ru.quad_light(p, l, s, torch.ones(3)).vertices
        d = (l - p) / (l - p).norm()
        assert torch.allclose(q.mean(0), p, atol=1e-12)
        assert torch.allclose((q[1] - q[0]).norm(), s[0], atol=1e-12) and torch.allclose((q[3] - q[0]).norm(), s[1], atol=1e-12)
        assert torch.allclose(q[2] - q[1], q[3] - q[0], atol=1e-12) and abs(float((q[1] - q[0]) @ (q[3] - q[0]))) < 1e-12
        n = torch.cross(q[1] - q[0], q[3] - q[0], dim=0)
        assert torch.allclose(n / n.norm(), d, atol=1e-12)
        if float(d[2]) < -1 + 1e-6:
            x = torch.tensor([0.0, -1.0, 0.0], dtype=torch.float64)
        else:
            a = 1 / (1 + d[2])
            x = torch.stack([1 - d[0] * d[0] * a, -d[0] * d[1] * a, -d[0]])
        assert torch.allclose((q[1] - q[0]) / s[0], x, atol=1e-12)
    with pytest.raises(RuntimeError, match=r'vertices must be \[4, 3\]'):
        ru.QuadLight(torch.zeros(3, 3), torch.ones(3))
    with pytest.raises(RuntimeError, match=r'intensity must be \[3\]'):
        ru.QuadLight(torch.zeros(4, 3), torch.ones(4))


# ---- 6. errors, raised before any launch ------------------------------------------------------------------------------------------
def _run_errors(rd, device):
    ru = _ru()
    from redner_amd import _capi
    case = _definition_case('grid_5x7_aa2_alpha1')
    g = case['g'].to(device)
    quads = torch.from_numpy(case['quads']).to(device)
    args = lambda **kw: [kw.get('g', g), kw.get('quads', quads), kw.get('flags', case['flags']), kw.get('ranges', case['ranges']),
                         kw.get('aa', case['aa']), kw.get('alpha', True), rd]
    ru.DeferredQuad.apply(*args())
    for what, bad in (('G-buffer must be', dict(g=g[..., :9])), ('G-buffer must be', dict(alpha=False)), ('G-buffer must be', dict(g=g[0])),
                      ('does not divide', dict(aa=4)), ('quads must be', dict(quads=quads[:, :15])), ('quads must be', dict(quads=quads[:2])),
                      ('quad ranges for', dict(ranges=case['ranges'][:1])),
                      ('fp32 tensors only', dict(g=g.double())), ('fp32 tensors only', dict(quads=quads.double())),
                      ('outside the table', dict(ranges=((0, 4), (1, 2)))), ('outside the table', dict(ranges=((0, 3), (2, 1)))),
                      ('must be 0 .one-sided. or 1 .two-sided.', dict(flags=(0, 2, 1))), ('must be 0 .one-sided.', dict(flags=(-1, 0, 1)))):
        with pytest.raises(RuntimeError, match=what):
            ru.DeferredQuad.apply(*args(**bad))
    # a QuadLight has no row in the light table
    light = ru.QuadLight(quads[0, :12].reshape(4, 3), quads[0, 12:15])
    for call in (lambda: ru.deferred_shade(g, [light], alpha=True, aa_samples=2, backend=rd),
                 lambda: ru.deferred_specular(g, torch.zeros(2, 10, 14, 4, device=device), [light], torch.zeros(3), alpha=True,
                                              aa_samples=2, backend=rd),
                 lambda: ru.pack_lights([ru.AmbientLight(torch.ones(3)), light], device)):
        with pytest.raises(RuntimeError, match='deferred_quad'):
            call()
    with pytest.raises(RuntimeError, match='is not a QuadLight'):
        ru.deferred_quad(g, [ru.AmbientLight(torch.ones(3))], alpha=True, aa_samples=2, backend=rd)
    # create_graph=True
    gl = g.clone().requires_grad_(True)
    img = ru.deferred_quad(gl, [light], alpha=True, aa_samples=2, backend=rd)
    with pytest.raises(RuntimeError, match='cannot be differentiated again'):
        torch.autograd.grad(img.sum(), gl, create_graph=True)
    # the C ABI: the occluder, visibility and ao fields must be zero; a null tensor and a misaligned alpha buffer are refused
    lib = _capi.lib()
    keep = [(ctypes.c_int32 * 3)(*case['flags']), (ctypes.c_int32 * 4)(0, 3, 1, 2), (ctypes.c_void_p * 2)(),
            torch.full((2, 10, 14), -1, dtype=torch.int32, device=device)]
    image = torch.full((2, 5, 7, 3), 7.0, device=device)

    def call(buffer=g, **fields):
        desc = _capi.DeferredDesc()
        desc.num_images, desc.height, desc.width, desc.aa_samples, desc.alpha, desc.num_lights = 2, 5, 7, 2, 1, 3
        desc.light_type, desc.image_light_range, desc.gpu_index = keep[0], keep[1], -1 if device.type == 'cpu' else 0
        for field, value in fields.items():
            setattr(desc, field, value)
        return lib.rdr_deferred_quad(ctypes.byref(desc), buffer.data_ptr(), quads.data_ptr(), image.data_ptr()), desc

    for fields in (dict(ao_rays=4), dict(ao_words=keep[3].data_ptr()), dict(ao_occluders=keep[2]), dict(occluders=keep[2]),
                   dict(visibility=keep[3].data_ptr())):
        assert call(**fields)[0] == 1 and 'must be zero' in _capi.last_error(), fields
    misaligned = torch.zeros(g.numel() + 1, device=device)[1:]
    assert misaligned.data_ptr() % 8 == 4 and call(misaligned)[0] == 1 and '8-byte aligned' in _capi.last_error()
    assert call(num_lights=-1)[0] == 1 and call(aa_samples=0)[0] == 1 and call(alpha=2)[0] == 1
    assert bool((image == 7.0).all())                     # nothing was launched
    rc, desc = call()
    assert rc == 0 and _capi.last_error() == '' and not bool((image == 7.0).any())
    assert lib.rdr_deferred_quad(None, None, None, None) == 1 and 'description' in _capi.last_error()
    assert lib.rdr_deferred_quad(ctypes.byref(desc), g.data_ptr(), None, image.data_ptr()) == 1 and 'null tensor' in _capi.last_error()
    assert lib.rdr_deferred_quad_backward(ctypes.byref(desc), *[None] * 5) == 1 and 'null tensor' in _capi.last_error()
    d_g = torch.zeros(g.numel() + 1, device=device)[1:]
    assert lib.rdr_deferred_quad_backward(ctypes.byref(desc), g.data_ptr(), quads.data_ptr(), image.data_ptr(), d_g.data_ptr(),
                                          torch.empty_like(quads).data_ptr()) == 1 and '8-byte aligned' in _capi.last_error()


def test_errors_hostsim(hostsim_backend):
    _run_errors(hostsim_backend, CPU)


@pytest.mark.gpu
def test_errors_gpu(gpu_backend):
    _run_errors(gpu_backend, GPU)


# ---- 7. reproducibility ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_quad_gradients_bitwise_reproducible_gpu(gpu_backend):
    """d_quads is a sum over every texel: per-block fp64 partials folded in a fixed order, no atomics (the strided grid)."""
    case = _definition_case(PLAN_CASE)
    runs = [_apply(gpu_backend, GPU, case, case['up']) for _ in range(2)]
    assert float(runs[0]['d_quads'].abs().sum()) > 0
    for k in runs[0]:
        assert runs[0][k].numpy().tobytes() == runs[1][k].numpy().tobytes(), k


# ---- 8. the binding -------------------------------------------------------------------------------------------------------------------
def test_binding_matches_the_header(hostsim_backend):
    """csrc/deferred_quad_abi.h, its table in _capi and the libraries' exports say the same (what tests/test_capi.py holds the
    headers under include/ to)."""
    from conftest import HOSTSIM_LIB
    from redner_amd import _capi, redner
    from test_capi import declared_signatures
    header = os.path.join('..', 'redner_amd', 'csrc', 'deferred_quad_abi.h')
    declared, table = declared_signatures(header), _capi.CSRC_HEADERS['deferred_quad_abi.h']
    assert sorted(declared) == ['rdr_deferred_quad', 'rdr_deferred_quad_backward'] == sorted(table)
    for name, count in declared.items():
        assert len(table[name][1]) == count, name
        assert not any(name in others for others in _capi.HEADERS.values())
        assert not any(name in others for header_name, others in _capi.CSRC_HEADERS.items() if header_name != 'deferred_quad_abi.h')
    for path in (HOSTSIM_LIB, _capi.DEFAULT_LIBRARY, _capi.EXACT_LIBRARY):
        if path == HOSTSIM_LIB or os.path.exists(path):
            lib = ctypes.CDLL(path)
            assert all(hasattr(lib, name) for name in declared), path
    import redner_amd
    ru = _ru()
    assert callable(redner.deferred_quad) and callable(redner.deferred_quad_backward)
    for name in ('QuadLight', 'quad_light', 'DeferredQuad', 'deferred_quad'):
        assert getattr(redner_amd, name) is getattr(ru, name), name
    assert issubclass(ru.QuadLight, ru.DeferredLight) and ru.QuadLight.light_type is None
