"""Soft shadows of the quad lights (rdr_deferred_quad_shadowed / _backward, csrc/deferred_quad_shadow.h;
redner_amd.render_utils.DeferredQuadShadowed, deferred_quad(occluders=..., shadow_rays=K), render_deferred(quad_shadow_rays=K)).

The rule of csrc/deferred_quad_shadow_abi.h is restated here in numpy fp64 (`sample_table`, `samples64`): the table is computed in
fp64 and rounded once to fp32, the points, weights and rays are formed from the fp32 inputs in fp64.  What the cases are held to:
  * the words against test_deferred_shadows' brute-force fp64 intersector.  A ray is a BOUNDARY ray when its fp64 answer flips as
    the blockers are scaled by 1 +- 1e-3 about their centroids, or when its cs or ce lies within 1e-5 of 0 relative to |d| |nh| or
    |d| |J| (whether the sample counts is then a matter of rounding); boundary rays are left out, and may be at most 2 % of the
    counting rays, of which at least 10 % are robustly blocked and at least 10 % robustly clear;
  * the factors against the fp64 num / den of the device's own words, at parity_util.TOL;
  * values and gradients against test_deferred_quad's fp64 definition with every (quad, texel) term scaled by the device's factor,
    held constant, at parity_util.TOL per image slice, G-buffer slice and quad row;
  * bit-for-bit equality with the unshadowed call where nothing is in the way, with the single-image call in a batch, and across
    chunk sizes of the ray queue.
Every case runs on the CPU harness; the GPU legs run the same bodies on both builds of the library.  Frames are a few hundred to
a few thousand texels."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import parity_util
import test_deferred_quad as t_quad
import test_deferred_specular as t_spec
from test_deferred import _worst_slice
from test_deferred_quad import KINK, contour64, generate, quad64, three_quads
from test_deferred_shadows import BLOCKERS, FAR_AWAY, TMAX_SCALE, any_hit64, any_rays, floor_g_buffer, occluder

CPU, GPU = torch.device('cpu'), torch.device('cuda:0')
MARGIN = 1e-5                            # how near cs == 0 or ce == 0 a ray is a boundary ray
_cache = {}


def _ru():
    from redner_amd import render_utils
    return render_utils


def full_mask(k):
    return np.uint32(0xffffffff if k >= 32 else (1 << k) - 1)


# ---- the rule in numpy fp64 ------------------------------------------------------------------------------------------------------
def sample_table(k_rays):
    """uv[16][K][2]: fp64, rounded once to fp32"""
    pow2 = 1
    while pow2 < k_rays:
        pow2 *= 2
    table = np.zeros((16, k_rays, 2), np.float64)
    for j in range(16):
        for k in range(k_rays):
            inverse, digit, b = 0.0, 0.5, k
            while b:
                if b & 1:
                    inverse += digit
                b >>= 1
                digit *= 0.5
            table[j, k, 0] = (k + ((j & 3) + 0.5) / 4.0) / k_rays
            table[j, k, 1] = inverse + ((j >> 2) + 0.5) / (4.0 * pow2)
    return table.astype(np.float32)


def samples64(g, quad, two_sided, k_rays):
    """g [hg, wg, >= 6] fp32 numpy, quad: sixteen fp32 floats -> per sample k and texel: counts, near (a boundary of counting), w,
    the ray's direction and tmax; and the texels' origins.  The gate of the texel is taken in fp32, as the kernels take it."""
    hg, wg = g.shape[:2]
    p, n = g[..., 0:3].astype(np.float64), g[..., 3:6].astype(np.float64)
    with np.errstate(all='ignore'):
        nn32 = (g[..., 3] * g[..., 3] + g[..., 4] * g[..., 4]) + g[..., 5] * g[..., 5]
        pp32 = (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]
        framed = (nn32 > 0) & np.isfinite(nn32) & np.isfinite(pp32)
        nh = n / np.sqrt(np.where(framed, (n * n).sum(-1), 1.0))[..., None]
    q = np.asarray(quad, np.float32).astype(np.float64)[:12].reshape(4, 3)
    a, b = q[1] - q[0], q[3] - q[0]
    gg = (q[2] - q[1]) - b
    table = sample_table(k_rays).astype(np.float64)
    yy, xx = np.meshgrid(np.arange(hg), np.arange(wg), indexing='ij')
    rotation = (xx & 3) + 4 * (yy & 3)
    out = {k: [] for k in ('counts', 'near', 'w', 'dir', 'tmax')}
    with np.errstate(all='ignore'):
        for k in range(k_rays):
            u, v = table[rotation, k, 0][..., None], table[rotation, k, 1][..., None]
            s = q[0] + u * a + v * b + (u * v) * gg
            J = np.cross(a + v * gg, b + u * gg)
            d = s - p
            r2, cs, dj = (d * d).sum(-1), (d * nh).sum(-1), (d * J).sum(-1)
            ce = np.abs(dj) if two_sided else -dj
            w = cs * ce / (r2 * r2)
            r = np.sqrt(r2)
            counts = framed & (r2 > 0) & (cs > 0) & (ce > 0) & np.isfinite(w) & (w > 0)
            near = framed & ((np.abs(cs) < MARGIN * r) | (np.abs(ce) < MARGIN * r * np.sqrt((J * J).sum(-1))))
            out['counts'].append(counts & ~near)
            out['near'].append(near)
            out['w'].append(np.where(counts, w, 0.0))
            out['dir'].append(np.where(counts[..., None], d / r[..., None], 0.0))
            out['tmax'].append(np.where(counts, TMAX_SCALE * r, 0.0))
    out = {k: np.stack(v) for k, v in out.items()}
    out['origin'] = np.where(framed[..., None], p, 0.0)
    return out


def brute_words(g, quad, two_sided, k_rays, tris):
    """-> the rule's samples + `clear` [K, hg, wg] (the fp64 any-hit answer, inverted) and `robust` (not a boundary ray)"""
    tris = np.asarray(tris, np.float64)
    centre = tris.mean(axis=1, keepdims=True)
    s = samples64(g, quad, two_sided, k_rays)
    hg, wg = g.shape[:2]
    o = np.broadcast_to(s['origin'][None], s['dir'].shape).reshape(-1, 3)
    answers = [any_hit64(o, s['dir'].reshape(-1, 3), s['tmax'].reshape(-1), centre + f * (tris - centre)).reshape(k_rays, hg, wg)
               for f in (1.0, 1.0 + 1e-3, 1.0 - 1e-3)]
    s['clear'] = ~answers[0]
    s['robust'] = (answers[0] == answers[1]) & (answers[0] == answers[2]) & ~s['near']
    return s


def factors64(samples, words):
    """num / den by the rule, in fp64, from the device's own words [hg, wg] uint32"""
    k_rays = samples['w'].shape[0]
    num, den = np.zeros(words.shape), np.zeros(words.shape)
    for k in range(k_rays):
        w = np.where(samples['counts'][k] | samples['near'][k], samples['w'][k], 0.0)
        den = den + w
        num = num + np.where(((words >> np.uint32(k)) & 1).astype(bool), w, 0.0)
    with np.errstate(all='ignore'):
        return np.where(den > 0, num / np.where(den > 0, den, 1.0), 1.0)


# ---- calling the op ---------------------------------------------------------------------------------------------------------------
def apply(backend, device, g, quads, flags, ranges, aa, alpha, occluders, k_rays, up=None):
    """DeferredQuadShadowed (DeferredQuad when `occluders` is None) forward (+ backward when `up` is given) -> dict of CPU tensors"""
    ru = _ru()
    gl = g.clone().to(device).requires_grad_(True)
    ql = torch.from_numpy(np.asarray(quads, np.float32)).clone().to(device).requires_grad_(True)
    if occluders is None:
        out = {'image': ru.DeferredQuad.apply(gl, ql, tuple(flags), tuple(ranges), aa, bool(alpha), backend)}
    else:
        scenes = tuple(o.scene if o is not None else None for o in occluders)
        img, words, factors = ru.DeferredQuadShadowed.apply(gl, ql, tuple(flags), tuple(ranges), aa, bool(alpha), backend, scenes, k_rays)
        assert words.dtype == torch.int32 and factors.dtype == torch.float32 and words.shape == factors.shape
        assert not words.requires_grad and not factors.requires_grad
        out = {'image': img, 'words': words.cpu(), 'factors': factors.cpu()}
    if up is not None:
        out['image'].backward(up.to(device))
        out.update(d_g_buffer=gl.grad.cpu(), d_quads=ql.grad.cpu())
    out['image'] = out['image'].detach().cpu()
    return out


def as_words(t):
    return t.numpy().view(np.uint32)


def random_upstream(shape, seed=5):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


class Spy:
    """a backend that passes everything on and writes down which deferred_* entry points were called"""

    def __init__(self, rd):
        self._rd, self.calls = rd, []

    def __getattr__(self, name):
        value = getattr(self._rd, name)
        if not name.startswith('deferred_'):
            return value

        def recorded(*args, **kw):
            self.calls.append(name)
            return value(*args, **kw)
        return recorded


# ---- the floor under four quads: the words case ---------------------------------------------------------------------------------------
def floor_quads():
    """three_quads (high and facing down; low and upright in x = 0.3, towards +x, cut by the floor's horizon; two-sided and upright in
    y = -0.2) + the high quad with its corners reversed: one-sided and seen from behind by every texel of the floor"""
    rows, flags = three_quads(6001)
    rows = np.concatenate([rows, t_quad._reversed(rows[0:1])])
    return rows, tuple(flags) + (0,)


def floor_case(aa, alpha, k_rays):
    key = ('floor', aa, alpha, k_rays)
    if key not in _cache:
        hg, wg = (20, 24) if aa == 1 else (21, 24)
        g = floor_g_buffer(hg, wg, alpha)
        rows, flags = floor_quads()
        brute = [brute_words(g[0].numpy(), rows[l], flags[l], k_rays, BLOCKERS) for l in range(len(flags))]
        _cache[key] = dict(g=g, quads=rows, flags=flags, brute=brute, hg=hg, wg=wg)
    return _cache[key]


def _census(brute):
    counting = sum(int((b['counts'] | b['near']).sum()) for b in brute)
    boundary = sum(int(((b['counts'] | b['near']) & ~b['robust']).sum()) for b in brute)
    blocked = sum(int((b['counts'] & b['robust'] & ~b['clear']).sum()) for b in brute)
    clear = sum(int((b['counts'] & b['robust'] & b['clear']).sum()) for b in brute)
    return counting, boundary, blocked, clear


WORD_CASES = [(aa, alpha, k) for aa, alpha in ((1, 0), (3, 1)) for k in (1, 5, 32)]


@pytest.mark.parametrize('aa,alpha,k_rays', WORD_CASES)
def test_the_rule_alone_meets_the_caps(aa, alpha, k_rays):
    """numpy only: the fp64 rule on the words case leaves out at most 2 % of the counting rays and keeps at least 10 % robustly
    blocked and 10 % robustly clear; some texels of the upright quad have only some samples counting (K > 1); no sample of the
    quad seen from behind counts"""
    case = floor_case(aa, alpha, k_rays)
    counting, boundary, blocked, clear = _census(case['brute'])
    print('K = %d: counting rays %d, boundary %d, robustly blocked %d, robustly clear %d' % (k_rays, counting, boundary, blocked, clear))
    assert counting > 0 and boundary <= 0.02 * counting and blocked >= 0.10 * counting and clear >= 0.10 * counting
    upright = case['brute'][1]['counts'].sum(0)
    if k_rays > 1:
        assert int(((upright > 0) & (upright < k_rays)).sum()) >= 8
    behind = case['brute'][3]
    assert not (behind['counts'] | behind['near']).any()


def _run_words_and_factors(backend, device, aa, alpha, k_rays, harness):
    case = floor_case(aa, alpha, k_rays)
    nq = len(case['flags'])
    blockers = occluder(backend, BLOCKERS, device)
    before = any_rays(backend)
    out = apply(backend, device, case['g'], case['quads'], case['flags'], ((0, nq),), aa, alpha, (blockers,), k_rays)
    words, factors = as_words(out['words']), out['factors'].numpy()
    assert words.shape == (nq, case['hg'], case['wg'])
    assert (words >> np.uint32(k_rays) == 0).all() if k_rays < 32 else True
    listed = 0
    for l in range(nq):
        b = case['brute'][l]
        for k in range(k_rays):
            got = ((words[l] >> np.uint32(k)) & 1).astype(bool)
            want = ~b['counts'][k] | b['clear'][k]
            assert (got == want)[b['robust'][k]].all(), 'quad %d sample %d: %d bits differ' % (l, k, int((got != want)[b['robust'][k]].sum()))
        silent = ~(b['counts'] | b['near']).any(0)                              # no counting sample, robustly
        assert (words[l][silent] == full_mask(k_rays)).all() and (factors[l][silent] == 1.0).all(), l
        listed += int((b['counts'] | b['near']).any(0).sum()) if not b['near'].any() else -10 ** 9
        # 5. the factor against the fp64 ratio of the device's own words
        want_v = factors64(b, words[l])
        err = float(np.linalg.norm(factors[l] - want_v) / np.linalg.norm(want_v))
        print('quad %d K = %d: factor %.2e (mean %.4f, min %.4f)' % (l, k_rays, err, float(factors[l].mean()), float(factors[l].min())))
        assert err < parity_util.TOL, (l, err)
        assert (factors[l] >= 0).all() and (factors[l] <= 1).all()
    assert (words[:, :2] == full_mask(k_rays)).all() and (factors[:, :2] == 1).all()              # the background rows
    assert (words[3] == full_mask(k_rays)).all() and (factors[3] == 1).all()                      # seen from behind
    if k_rays == 32:
        assert (words[0] == 0xffffffff).any() and ((words[0] >> np.uint32(31)) & 1 == 0).any()
    assert float(factors[0].min()) < 0.5
    if harness and listed >= 0:               # the queue held K rays per listed texel and nothing else (the quad from behind: none)
        assert any_rays(backend) - before == k_rays * listed


@pytest.mark.parametrize('aa,alpha,k_rays', WORD_CASES)
def test_words_and_factors_hostsim(hostsim_backend, aa, alpha, k_rays):
    _run_words_and_factors(hostsim_backend, CPU, aa, alpha, k_rays, True)


@pytest.mark.gpu
@pytest.mark.parametrize('aa,alpha,k_rays', WORD_CASES)
def test_words_and_factors_gpu(gpu_backend, aa, alpha, k_rays):
    _run_words_and_factors(gpu_backend, GPU, aa, alpha, k_rays, False)


# ---- 1. off is off -----------------------------------------------------------------------------------------------------------------------
def _run_off_is_off(backend, device):
    ru = _ru()
    case = t_quad._definition_case('grid_5x7_aa2_alpha1')
    lights = [ru.QuadLight(torch.from_numpy(case['quads'][l, :12].reshape(4, 3)), torch.from_numpy(case['quads'][l, 12:15]),
                           two_sided=bool(case['flags'][l])) for l in range(3)]
    up = random_upstream((2, 5, 7, 3))
    plain = apply(backend, device, case['g'], case['quads'], case['flags'], ((0, 3), (0, 3)), 2, 1, None, 0, up)
    spy = Spy(backend)
    gl = case['g'].clone().to(device).requires_grad_(True)
    img = ru.deferred_quad(gl, lights, alpha=True, aa_samples=2, backend=spy)
    img.backward(up.to(device))
    assert spy.calls == ['deferred_quad', 'deferred_quad_backward']
    assert torch.equal(img.detach().cpu(), plain['image']) and torch.equal(gl.grad.cpu(), plain['d_g_buffer'])
    # render_deferred: the same entry points, in the same order, and the same bits whether the keyword is given or not
    scene = lambda: t_spec._sphere_over_plane(device, (8, 8))
    _, quads = t_quad._quad_lights(ru)
    table = t_spec._e2e_lights(ru)[1]
    kw = dict(aa_samples=2, seed=5, device=device)
    rays_before = any_rays(backend)
    spy = Spy(backend)
    without = ru.render_deferred(scene(), table + quads, backend=spy, **kw).detach()
    assert spy.calls == ['deferred_shade', 'deferred_quad']
    spy = Spy(backend)
    zero = ru.render_deferred(scene(), table + quads, backend=spy, quad_shadow_rays=0, **kw).detach()
    assert spy.calls == ['deferred_shade', 'deferred_quad'] and torch.equal(zero, without)
    # rays without a QuadLight in the list: nothing to shadow, nothing built, the same calls
    spy = Spy(backend)
    ru.render_deferred(scene(), table, backend=spy, quad_shadow_rays=8, **kw)
    assert spy.calls == ['deferred_shade']
    if device.type == 'cpu':
        assert any_rays(backend) == rays_before


def test_off_is_off_hostsim(hostsim_backend):
    _run_off_is_off(hostsim_backend, CPU)


@pytest.mark.gpu
def test_off_is_off_gpu(gpu_backend):
    _run_off_is_off(gpu_backend, GPU)


# ---- 2. nothing in the way is bit for bit nothing ------------------------------------------------------------------------------------
def _run_nothing_in_the_way(backend, device):
    far = occluder(backend, FAR_AWAY, device)
    blockers = occluder(backend, BLOCKERS, device)
    for name, k_rays in (('grid_5x7_aa2_alpha1', 5), ('grid_5x7_aa3_alpha0', 32)):
        case = t_quad._definition_case(name)
        args = (case['g'], case['quads'], case['flags'], case['ranges'], case['aa'], case['alpha'])
        up = random_upstream(case['up'].shape)
        plain = apply(backend, device, *args, None, 0, up)
        shadowed = apply(backend, device, *args, (far, far), k_rays, up)
        for k in plain:
            assert torch.equal(plain[k], shadowed[k]), (name, k)
        assert (as_words(shadowed['words']) == full_mask(k_rays)).all() and bool((shadowed['factors'] == 1).all())
        assert tuple(shadowed['words'].shape) == (4,) + tuple(case['g'].shape[1:3])
        # a NULL occluder for the second image of two: that image is the unshadowed one, the first is shadowed
        half = apply(backend, device, *args, (blockers, None), k_rays, up)
        assert torch.equal(half['image'][1], plain['image'][1]) and torch.equal(half['d_g_buffer'][1], plain['d_g_buffer'][1])
        assert (as_words(half['words'])[3] == full_mask(k_rays)).all() and bool((half['factors'][3] == 1).all())
        assert bool((half['factors'][0] < 1).any()) and not torch.equal(half['image'][0], plain['image'][0])


def test_nothing_in_the_way_hostsim(hostsim_backend):
    _run_nothing_in_the_way(hostsim_backend, CPU)


@pytest.mark.gpu
def test_nothing_in_the_way_gpu(gpu_backend):
    _run_nothing_in_the_way(gpu_backend, GPU)


# ---- 3. the rule against itself (numpy only) -----------------------------------------------------------------------------------------
def test_the_weights_integrate_to_the_form_factor():
    """A unit square 3 above a tilted texel, the whole of it above the texel's horizon: the fp64 mean of w over a 1500 x 1500 grid
    of the unit square is contour64's F = S / 2 to 1e-6 relative, and at K = 16 every rotation's sum of w / K lies within 1 %."""
    quad = np.zeros(16, np.float32)
    quad[:12] = np.array([[-0.5, 0.5, 3.0], [0.5, 0.5, 3.0], [0.5, -0.5, 3.0], [-0.5, -0.5, 3.0]], np.float32).reshape(-1)   # faces down
    n = np.array([0.3, -0.2, 1.0])
    nh = n / np.linalg.norm(n)
    p = np.array([0.2, -0.1, 0.0])
    S, up = contour64(torch.from_numpy(p)[None], torch.from_numpy(nh)[None], torch.from_numpy(quad[:12].astype(np.float64)).reshape(4, 3))
    F = float(S[0]) / 2.0
    assert int(up[0]) == 4 and F > 0
    q = quad[:12].astype(np.float64).reshape(4, 3)
    a, b = q[1] - q[0], q[3] - q[0]
    gg = (q[2] - q[1]) - b

    def weight(u, v):
        s = q[0] + u[..., None] * a + v[..., None] * b + (u * v)[..., None] * gg
        J = np.cross(a + v[..., None] * gg, b + u[..., None] * gg)
        d = s - p
        return (d * nh).sum(-1) * -(d * J).sum(-1) / ((d * d).sum(-1) ** 2)

    m = (np.arange(1500) + 0.5) / 1500
    u, v = np.meshgrid(m, m, indexing='ij')
    mean = float(weight(u, v).mean())
    print('F %.9f, mean of w %.9f' % (F, mean))
    assert abs(mean - F) < 1e-6 * F
    table = sample_table(16).astype(np.float64)
    assert (table > 0).all() and (table < 1).all()
    worst = max(abs(float(weight(table[j, :, 0], table[j, :, 1]).mean()) - F) / F for j in range(16))
    print('K = 16: the worst rotation is %.3f %% off' % (100 * worst))
    assert worst < 0.01
    # the table is a stratification: one u per stratum, jittered; the sixteen rotations interleave
    for k_rays in (1, 5, 16, 32):
        t = sample_table(k_rays).astype(np.float64)
        assert (np.floor(t[:, :, 0] * k_rays) == np.arange(k_rays)[None]).all() and (t > 0).all() and (t < 1).all()
        assert len({(float(t[j, 0, 0]), float(t[j, 0, 1])) for j in range(16)}) == 16
    # through samples64: the same weights from a one-texel G-buffer
    g = np.zeros((1, 1, 9), np.float32)
    g[0, 0, 0:3], g[0, 0, 3:6] = p, n
    s = samples64(g, quad, False, 16)
    assert s['counts'].all() and abs(float(s['w'].sum()) / 16 - F) < 0.01 * F


# ---- 6. values and gradients ---------------------------------------------------------------------------------------------------------
def definition_scaled(g64, quads64, flags, ranges, aa, factors):
    """quad64 with every (quad, texel) term scaled by factors [pairs, hg, wg] (a constant), resolved over aa"""
    n, hg, wg, _ = g64.shape
    rgb = torch.zeros(n, hg, wg, 3, dtype=torch.float64)
    bases = np.concatenate([[0], np.cumsum([e - b for b, e in ranges])])
    for l in range(len(flags)):
        uses = [(0, 1) if b <= l < e else (0, 0) for b, e in ranges]
        if not any(e for _, e in uses):
            continue
        one, _ = quad64(g64, quads64[l:l + 1], (flags[l],), uses, 1)
        scale = torch.ones(n, hg, wg, dtype=torch.float64)
        for i, (b, e) in enumerate(ranges):
            if b <= l < e:
                scale[i] = factors[int(bases[i]) + l - b].double()
        rgb = rgb + one * scale[..., None]
    return rgb.reshape(n, hg // aa, aa, wg // aa, aa, 3).mean(dim=(2, 4))


VALUE_CASES = ['grid_5x7_aa1_alpha0', 'grid_5x7_aa2_alpha1', 'grid_5x7_aa3_alpha0', 'grid_17x16_aa1_alpha1', 'grid_17x16_aa2_alpha0',
               'grid_17x16_aa3_alpha1']


def _run_values_and_gradients(backend, device, name):
    case = t_quad._definition_case(name)                      # (its texels are off the kink: 0 < |S| < KINK nowhere)
    assert int(case['report']['near'].sum()) == 0 and KINK == 1e-4
    up = random_upstream(case['up'].shape, seed=17)
    blockers = occluder(backend, BLOCKERS, device)
    out = apply(backend, device, case['g'], case['quads'], case['flags'], case['ranges'], case['aa'], case['alpha'],
                (blockers, blockers), 16, up)
    factors = out['factors']
    assert bool((factors < 1).any()) and bool((factors == 1).any()) and float(factors.min()) >= 0 and float(factors.max()) <= 1
    g64 = case['g'].double().requires_grad_(True)
    q64 = torch.from_numpy(case['quads']).double().requires_grad_(True)
    want = definition_scaled(g64, q64, case['flags'], case['ranges'], case['aa'], factors)
    want.backward(up.double())
    errors = {'image': _worst_slice(out['image'], want.detach(), name + ' image'),
              'd_g_buffer': _worst_slice(out['d_g_buffer'][..., :9], g64.grad[..., :9], name + ' d_g_buffer'),
              'd_quads': _worst_slice(out['d_quads'], q64.grad, name + ' d_quads')}
    print(name, {k: '%.2e' % e for k, e in errors.items()}, 'bar %.0e' % parity_util.TOL)
    for k, e in errors.items():
        assert e < parity_util.TOL, (name, k, e)
    if case['alpha']:
        assert bool((out['d_g_buffer'][..., 9] == 0).all())
    assert bool((out['d_quads'][:, 15] == 0).all())
    # the shadowed image is not the unshadowed one
    plain = apply(backend, device, case['g'], case['quads'], case['flags'], case['ranges'], case['aa'], case['alpha'], None, 0)
    assert float((plain['image'] - out['image']).abs().max()) > 1e-3 and bool((plain['image'] >= out['image']).all())


@pytest.mark.parametrize('name', VALUE_CASES)
def test_values_and_gradients_hostsim(hostsim_backend, name):
    _run_values_and_gradients(hostsim_backend, CPU, name)


@pytest.mark.gpu
@pytest.mark.parametrize('name', VALUE_CASES)
def test_values_and_gradients_gpu(gpu_backend, name):
    _run_values_and_gradients(gpu_backend, GPU, name)


# ---- 7. a batch ----------------------------------------------------------------------------------------------------------------------
def _run_batch(backend, device):
    base = t_quad._definition_case('grid_5x7_aa2_alpha1')
    g = torch.cat([base['g'], generate(991, 1, 5, 7, 2, 1)])
    ranges, k_rays = ((0, 3), (1, 2), (2, 2)), 5
    blockers = occluder(backend, BLOCKERS, device)
    up = random_upstream((3, 5, 7, 3), seed=23)
    whole = apply(backend, device, g, base['quads'], base['flags'], ranges, 2, 1, (blockers,) * 3, k_rays, up)
    assert tuple(whole['words'].shape) == (4, 10, 14) and bool((whole['factors'] < 1).any())
    first_pair = (0, 3, 4)
    for n, (b, e) in enumerate(ranges):
        single = apply(backend, device, g[n:n + 1], base['quads'], base['flags'], ((b, e),), 2, 1, (blockers,), k_rays, up[n:n + 1])
        assert tuple(single['words'].shape) == (e - b, 10, 14)
        assert torch.equal(single['image'][0], whole['image'][n]) and torch.equal(single['d_g_buffer'][0], whole['d_g_buffer'][n]), n
        pairs = slice(first_pair[n], first_pair[n] + e - b)
        assert torch.equal(single['words'], whole['words'][pairs]) and torch.equal(single['factors'], whole['factors'][pairs]), n
    assert bool((whole['image'][2] == 0).all()) and bool((whole['d_g_buffer'][2] == 0).all())
    assert not torch.equal(whole['words'][1], whole['words'][3])          # quad 1 over two different images
    # the quad gradients of the batch: the fp64 definition with the batch's factors (the sum over images has no single-image twin)
    g64, q64 = g.double().requires_grad_(True), torch.from_numpy(base['quads']).double().requires_grad_(True)
    definition_scaled(g64, q64, base['flags'], ranges, 2, whole['factors']).backward(up.double())
    assert _worst_slice(whole['d_quads'], q64.grad, 'batch d_quads') < parity_util.TOL


def test_batch_hostsim(hostsim_backend):
    _run_batch(hostsim_backend, CPU)


@pytest.mark.gpu
def test_batch_gpu(gpu_backend):
    _run_batch(gpu_backend, GPU)


# ---- 8. chunks of the ray queue ----------------------------------------------------------------------------------------------------
def _run_chunks(backend, device):
    case = floor_case(1, 0, 5)
    nq, k_rays = len(case['flags']), 5
    blockers = occluder(backend, BLOCKERS, device)
    up = random_upstream((1, 20, 24, 3), seed=29)
    args = (case['g'], case['quads'], case['flags'], ((0, nq),), 1, 0, (blockers,), k_rays, up)
    whole = apply(backend, device, *args)
    assert 'RDR_DEFERRED_SHADOW_CHUNK' not in os.environ
    for texels_per_chunk in (37, 101):        # 480 texels in rows of 24: thirteen and five chunks, none of which ends with a row
        os.environ['RDR_DEFERRED_SHADOW_CHUNK'] = str(k_rays * texels_per_chunk + 2)
        try:
            split = apply(backend, device, *args)
        finally:
            del os.environ['RDR_DEFERRED_SHADOW_CHUNK']
        for k in whole:
            assert torch.equal(whole[k], split[k]), (texels_per_chunk, k)
    assert bool((whole['factors'] < 1).any())


def test_chunks_hostsim(hostsim_backend):
    _run_chunks(hostsim_backend, CPU)


@pytest.mark.gpu
def test_chunks_gpu(gpu_backend):
    _run_chunks(gpu_backend, GPU)


# ---- 9. reproducible -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_reproducible_gpu(gpu_backend):
    case = t_quad._definition_case('grid_17x16_aa3_alpha1')
    blockers = occluder(gpu_backend, BLOCKERS, GPU)
    up = random_upstream(case['up'].shape, seed=31)
    runs = [apply(gpu_backend, GPU, case['g'], case['quads'], case['flags'], case['ranges'], 3, 1, (blockers, blockers), 16, up)
            for _ in range(2)]
    assert bool((runs[0]['factors'] < 1).any()) and float(runs[0]['d_quads'].abs().sum()) > 0
    for k in runs[0]:
        assert runs[0][k].numpy().tobytes() == runs[1][k].numpy().tobytes(), k


# ---- 10. degenerate texels -----------------------------------------------------------------------------------------------------------
def _run_degenerate(backend, device, harness):
    k_rays = 5
    quads = np.zeros((1, 16), np.float32)
    quads[0, :12] = np.array([[-0.5, 0.5, 1.0], [0.5, 0.5, 1.0], [0.5, -0.5, 1.0], [-0.5, -0.5, 1.0]], np.float32).reshape(-1)   # in z = 1, faces down
    quads[0, 12:15] = (3.0, 2.0, 1.0)
    g = torch.zeros(1, 2, 4, 9)
    g[..., 5], g[..., 6:9] = 1.0, 0.5                                             # a floor at z = 0 under the quad
    g[0, :, :, 0] = torch.tensor([-0.3, -0.1, 0.1, 0.3])
    g[0, 0, 0, 3:6] = 0.0                                                         # background
    g[0, 0, 1, 1] = float('nan')                                                  # a NaN position
    g[0, 0, 2, 3:6] = torch.tensor([0.0, 0.0, 1e20])                              # n.n overflows
    g[0, 0, 3, 0:3], g[0, 0, 3, 3:6] = torch.tensor([2.0, 0.0, 1.0]), torch.tensor([-1.0, 0.0, 0.0])      # on the emitter's plane: ce == 0
    roof = occluder(backend, [[[-30.0, -30.0, 0.5], [30.0, -30.0, 0.5], [0.0, 40.0, 0.5]]], device)      # blocks whatever is cast
    before = any_rays(backend)
    up = random_upstream((1, 2, 4, 3), seed=37)
    out = apply(backend, device, g, quads, (0,), ((0, 1),), 1, 0, (roof,), k_rays, up)
    words, factors = as_words(out['words'])[0], out['factors'][0]
    assert (words[0] == full_mask(k_rays)).all() and bool((factors[0] == 1).all())
    assert (words[1] == 0).all() and bool((factors[1] == 0).all())                # the four plain texels: every ray blocked
    assert all(bool(torch.isfinite(out[k]).all()) for k in ('image', 'factors', 'd_g_buffer', 'd_quads'))
    assert bool((out['d_g_buffer'][0, 0, :3] == 0).all())
    if harness:
        assert any_rays(backend) - before == 4 * k_rays                          # no ray of a degenerate texel
    s = samples64(g[0].numpy(), quads[0], False, k_rays)
    assert not (s['counts'] | s['near'])[:, 0, :3].any() and s['counts'][:, 1].all()


def test_degenerate_texels_hostsim(hostsim_backend):
    _run_degenerate(hostsim_backend, CPU, True)


@pytest.mark.gpu
def test_degenerate_texels_gpu(gpu_backend):
    _run_degenerate(gpu_backend, GPU, False)


# ---- 11. errors, raised before any launch -----------------------------------------------------------------------------------------------
def _run_errors(rd, device):
    ru = _ru()
    from redner_amd import _capi
    case = t_quad._definition_case('grid_5x7_aa2_alpha1')
    g = case['g'].to(device)
    quads = torch.from_numpy(case['quads']).to(device)
    blockers = occluder(rd, BLOCKERS, device)
    lights = [ru.QuadLight(quads[l, :12].reshape(4, 3), quads[l, 12:15]) for l in range(3)]
    kw = dict(alpha=True, aa_samples=2, backend=rd)
    spy = Spy(rd)
    for what, bad in (('shadow_rays', dict(occluders=blockers, shadow_rays=0)), ('shadow_rays', dict(occluders=blockers, shadow_rays=33)),
                      ('occluders', dict(shadow_rays=4)), ('occluders', dict(return_visibility=True))):
        with pytest.raises(RuntimeError, match=what):
            ru.deferred_quad(g, lights, **dict(kw, backend=spy), **bad)
    with pytest.raises(RuntimeError, match='quad_shadow_rays'):
        ru.render_deferred(t_spec._sphere_over_plane(device, (4, 4)), lights, backend=spy, device=device, quad_shadow_rays=33)
    scenes = (blockers.scene, blockers.scene)
    args = lambda **k: [k.get('g', g), quads, case['flags'], case['ranges'], 2, True, spy, k.get('scenes', scenes), k.get('rays', 4)] + \
        ([k['factors']] if 'factors' in k else [])
    for what, bad in (('shadow_rays', dict(rays=0)), ('shadow_rays', dict(rays=33)), ('occluders', dict(scenes=None)),
                      ('occluders', dict(scenes=scenes[:1])), ('factors', dict(factors=torch.empty(3, 10, 14, device=device))),
                      ('factors', dict(factors=torch.empty(4, 10, 15, device=device))),
                      ('factors', dict(factors=torch.empty(4, 10, 14, dtype=torch.float64, device=device))),
                      ('G-buffer must be', dict(g=g[..., :9]))):
        with pytest.raises(RuntimeError, match=what):
            ru.DeferredQuadShadowed.apply(*args(**bad))
    assert spy.calls == []                    # nothing native was called
    given = torch.full((4, 10, 14), 7.0, device=device)
    image, words, factors = ru.DeferredQuadShadowed.apply(*args(factors=given))
    assert not bool((given == 7.0).any()) and torch.equal(factors, given) and spy.calls == ['deferred_quad_shadowed']
    # the C ABI
    lib = _capi.lib()
    keep = [(ctypes.c_int32 * 3)(*case['flags']), (ctypes.c_int32 * 4)(0, 3, 1, 2), (ctypes.c_void_p * 2)(blockers.scene._handle, None)]
    words = torch.full((4, 10, 14), -7, dtype=torch.int32, device=device)
    factors = torch.full((4, 10, 14), 7.0, device=device)
    image = torch.full((2, 5, 7, 3), 7.0, device=device)
    d_g, d_q = torch.full_like(g, 7.0), torch.full_like(quads, 7.0)
    occluders = ctypes.cast(keep[2], ctypes.POINTER(ctypes.c_void_p))
    # four images of three quads over 14000 x 14000 texels: 12 x 1.96e8 words
    keep.append((ctypes.c_int32 * 8)(0, 3, 0, 3, 0, 3, 0, 3))
    keep.append((ctypes.c_void_p * 4)())
    many = ctypes.cast(keep[4], ctypes.POINTER(ctypes.c_void_p))

    def desc_of(**fields):
        desc = _capi.DeferredDesc()
        desc.num_images, desc.height, desc.width, desc.aa_samples, desc.alpha, desc.num_lights = 2, 5, 7, 2, 1, 3
        desc.light_type, desc.image_light_range, desc.gpu_index = keep[0], keep[1], -1 if device.type == 'cpu' else 0
        for field, value in fields.items():
            setattr(desc, field, value)
        return desc

    def forward(rays=4, factors_ptr=None, **fields):
        desc = desc_of(**dict(dict(occluders=occluders, visibility=words.data_ptr()), **fields))
        return lib.rdr_deferred_quad_shadowed(ctypes.byref(desc), g.data_ptr(), quads.data_ptr(), rays,
                                              factors.data_ptr() if factors_ptr is None else factors_ptr, image.data_ptr())

    def backward(**fields):
        desc = desc_of(**fields)
        return lib.rdr_deferred_quad_shadowed_backward(ctypes.byref(desc), g.data_ptr(), quads.data_ptr(), factors.data_ptr(),
                                                       image.data_ptr(), d_g.data_ptr(), d_q.data_ptr())

    for what, call in (('shadow_rays', lambda: forward(rays=0)), ('shadow_rays', lambda: forward(rays=33)),
                       ('occluders', lambda: forward(occluders=None)), ('visibility', lambda: forward(visibility=None)),
                       ('ao_', lambda: forward(ao_rays=4)), ('ao_', lambda: forward(ao_words=words.data_ptr())),
                       ('ao_', lambda: forward(ao_occluders=occluders)), ('cannot be indexed', lambda: forward(num_images=4, image_light_range=keep[3], occluders=many, height=7000, width=7000)),
                       ('occluders and visibility must be zero', lambda: backward(occluders=occluders)),
                       ('occluders and visibility must be zero', lambda: backward(visibility=words.data_ptr())),
                       ('ao_', lambda: backward(ao_rays=4))):
        assert call() == 1 and what in _capi.last_error(), (what, _capi.last_error())
    assert forward(factors_ptr=0) == 1 and 'null tensor' in _capi.last_error()
    assert lib.rdr_deferred_quad_shadowed(None, None, None, 4, None, None) == 1 and 'description' in _capi.last_error()
    assert lib.rdr_deferred_quad_shadowed_backward(None, *[None] * 6) == 1 and 'description' in _capi.last_error()
    for t in (words.float() + 14.0, factors, image, d_g, d_q):
        assert bool((t == 7.0).all())         # nothing was launched
    assert forward() == 0 and _capi.last_error() == ''
    assert not bool((words == -7).any()) and not bool((factors == 7.0).any()) and not bool((image == 7.0).any())
    assert backward() == 0 and not bool((d_g[..., :9] == 7.0).any()) and not bool((d_q == 7.0).any())
    assert (as_words(words.cpu())[3] == full_mask(4)).all() and bool((factors[3] == 1).all())          # image 1: a NULL occluder


def test_errors_hostsim(hostsim_backend):
    _run_errors(hostsim_backend, CPU)


@pytest.mark.gpu
def test_errors_gpu(gpu_backend):
    _run_errors(gpu_backend, GPU)


@pytest.mark.gpu
def test_an_occluder_on_another_device_is_refused_gpu(gpu_backend):
    """the one error that only the GPU library has: an occluder scene that lives on another device than the call's gpu_index"""
    if torch.cuda.device_count() < 2:
        pytest.skip('needs two GPUs (the round-end multi-GPU tier)')
    ru = _ru()
    case = t_quad._definition_case('grid_5x7_aa2_alpha1')
    elsewhere = occluder(gpu_backend, BLOCKERS, torch.device('cuda:1'))
    with pytest.raises(RuntimeError, match='the occluder scene of image 0 lives on device 1, the call runs on device 0'):
        ru.DeferredQuadShadowed.apply(case['g'].to(GPU), torch.from_numpy(case['quads']).to(GPU), case['flags'], case['ranges'], 2, True,
                                      gpu_backend, (elsewhere.scene, None), 4)


# ---- 12. the binding ---------------------------------------------------------------------------------------------------------------------
def test_binding_matches_the_header(hostsim_backend):
    """csrc/deferred_quad_shadow_abi.h, its table in _capi and the libraries' exports say the same; the two names stand in no
    other table"""
    from conftest import HOSTSIM_LIB
    from redner_amd import _capi, redner
    from test_capi import declared_signatures
    name_of = 'deferred_quad_shadow_abi.h'
    declared, table = declared_signatures(os.path.join('..', 'redner_amd', 'csrc', name_of)), _capi.CSRC_HEADERS[name_of]
    assert sorted(declared) == ['rdr_deferred_quad_shadowed', 'rdr_deferred_quad_shadowed_backward'] == sorted(table)
    for name, count in declared.items():
        assert len(table[name][1]) == count, name
        assert not any(name in others for others in _capi.HEADERS.values())
        assert not any(name in others for header_name, others in _capi.CSRC_HEADERS.items() if header_name != name_of)
    assert table['rdr_deferred_quad_shadowed'][1][3] is ctypes.c_int                   # shadow_rays
    for path in (HOSTSIM_LIB, _capi.DEFAULT_LIBRARY, _capi.EXACT_LIBRARY):
        if path == HOSTSIM_LIB or os.path.exists(path):
            lib = ctypes.CDLL(path)
            assert all(hasattr(lib, name) for name in declared), path
    import redner_amd
    ru = _ru()
    assert callable(redner.deferred_quad_shadowed) and callable(redner.deferred_quad_shadowed_backward)
    assert redner_amd.DeferredQuadShadowed is ru.DeferredQuadShadowed and issubclass(ru.DeferredQuadShadowed, torch.autograd.Function)
    assert ru.DeferredQuadShadowed is not ru.DeferredQuad


# ---- 14. end to end ----------------------------------------------------------------------------------------------------------------------
def _run_end_to_end(backend, device):
    ru = _ru()
    res, aa, seed, k_rays = 16, 2, 5, 16
    scene = lambda: t_spec._sphere_over_plane(device, (res, res))
    leaf = lambda x: torch.tensor(x, requires_grad=True)
    leaves = {'position': leaf([0.1, 3.0, 0.2]), 'size': leaf([1.5, 1.0]), 'intensity': leaf([30.0, 25.0, 20.0])}
    quad = ru.quad_light(leaves['position'], torch.tensor([0.0, -0.9, 0.0]), leaves['size'], leaves['intensity'])
    _, table_lights = t_spec._e2e_lights(ru)
    lights = [table_lights[0], quad]
    kw = dict(aa_samples=aa, seed=seed, device=device, backend=backend)
    sc = scene()
    shadowed = ru.render_deferred(sc, lights, quad_shadow_rays=k_rays, **kw)
    plain = ru.render_deferred(scene(), lights, **kw).detach().cpu()
    # the composition on render_g_buffer's channels
    big = t_spec._sphere_over_plane(device, (res * aa, res * aa))
    ch = [backend.channels.position, backend.channels.shading_normal, backend.channels.diffuse_reflectance]
    gb = ru.render_g_buffer(big, ch, seed=seed, device=device, backend=backend).detach().unsqueeze(0).contiguous()
    built = ru.occluder_scene(scene(), device=device, backend=backend)
    light, (words, factors) = ru.deferred_quad(gb, [quad], aa_samples=aa, backend=backend, occluders=built, shadow_rays=k_rays,
                                                return_visibility=True)
    composed = ru.deferred_shade(gb, [table_lights[0]], aa_samples=aa, backend=backend) + light
    assert torch.equal(shadowed.detach(), composed[0].detach())
    assert tuple(words.shape) == tuple(factors.shape) == (1, res * aa, res * aa)
    # gradients reach quad_light's position, size and intensity (and the scene)
    (shadowed * random_upstream(shadowed.shape, seed=41).to(device)).sum().backward()
    for name, t in leaves.items():
        assert t.grad is not None and bool(torch.isfinite(t.grad).all()) and float(t.grad.abs().sum()) > 0, name
    assert float(sc.shapes[0].vertices.grad.abs().sum()) > 0
    # under the sphere the floor is darker; where every texel of a pixel has the factor 1 the bits are those without shadows
    shadowed = shadowed.detach().cpu()
    pos = gb[0].cpu().reshape(res, aa, res, aa, 9)[..., 0:3]
    v = factors[0].cpu().reshape(res, aa, res, aa)
    on_floor = (pos[..., 1] < -0.85).all(dim=3).all(dim=1)
    under = on_floor & ((pos[..., 0] ** 2 + pos[..., 2] ** 2) < 0.75 ** 2).all(dim=3).all(dim=1)      # (the sphere's radius is 0.7)
    open_sky = (v == 1).all(dim=3).all(dim=1)
    print('pixels under the sphere %d, with an open view of the quad %d of %d' % (int(under.sum()), int(open_sky.sum()), res * res))
    assert int(under.sum()) >= 2 and int(open_sky.sum()) >= res * res // 4
    assert bool((shadowed[under] < plain[under]).all())
    assert torch.equal(shadowed[open_sky], plain[open_sky]) and bool((shadowed <= plain).all())
    v_of_pixel = v.permute(0, 2, 1, 3)[under]
    assert bool((v_of_pixel < 1).all()) and float(v_of_pixel.min()) < 0.5


def test_end_to_end_hostsim(hostsim_backend):
    _run_end_to_end(hostsim_backend, CPU)


@pytest.mark.gpu
def test_end_to_end_gpu(gpu_backend):
    _run_end_to_end(gpu_backend, GPU)


# ---- 15. against the path tracer (CPU harness) ---------------------------------------------------------------------------------------
# what test_against_the_path_tracer_hostsim measured (profiles/deferred_quad_shadows.txt, section 1): |deferred - path tracer| of the
# frame mean per channel, with quad_shadow_rays = 32 and aa 4; the bar is twice that (the spread between seeds; the ratio estimator is
# biased, so a bar in standard errors is not the right one)
MEASURED_DEVIATION = (1.988e-3, 1.136e-3, 5.111e-4)


def _floor_under_a_blocked_quad(ru, device, resolution):
    """test_deferred_quad's floor and rectangle (the emitter above the camera), and between them, above the camera too, a black
    rectangle in y = 1.5 that covers part of the quad as the floor sees it"""
    from redner_amd.render_pytorch import Shape
    position, look_at, size, radiance = [0.4, 2.0, -0.3], [0.1, 0.0, 0.2], [1.2, 0.8], [5.0, 4.0, 3.0]
    sc, light = t_quad._floor_under_a_quad(ru, device, resolution, position, look_at, size, radiance)
    t = lambda x, dtype=torch.float32: torch.tensor(x, dtype=dtype, device=device)
    blocker = Shape(t([[-0.3, 1.5, -0.9], [-0.3, 1.5, 0.0], [0.5, 1.5, -0.9], [0.5, 1.5, 0.0]]), t([[0, 1, 2], [1, 3, 2]], dtype=torch.int32), 1)
    sc.shapes.append(blocker)
    return sc, light


def test_against_the_path_tracer_hostsim(hostsim_backend):
    """The frame mean of render_pathtracing (direct light only, 64 samples per pixel, 8 seeds) against render_deferred with
    quad_shadow_rays = 32, aa 4.  The figures are in profiles/deferred_quad_shadows.txt, section 1."""
    ru = _ru()
    sc, light = _floor_under_a_blocked_quad(ru, CPU, (8, 8))
    kw = dict(aa_samples=4, seed=3, device=CPU, backend=hostsim_backend)
    unshadowed = ru.render_deferred(sc, [light], **kw).double().mean(dim=(0, 1))
    shadowed = ru.render_deferred(sc, [light], quad_shadow_rays=32, **kw).double().mean(dim=(0, 1))
    means = torch.stack([ru.render_pathtracing(sc, max_bounces=1, num_samples=(64, 1), seed=100 + m, device=CPU,
                                               backend=hostsim_backend).double().mean(dim=(0, 1)) for m in range(8)])
    mean, se = means.mean(0), means.std(0, unbiased=True) / math.sqrt(8)
    overshoot, deviation = unshadowed - mean, (shadowed - mean).abs()
    print('path tracer', mean.tolist(), 'standard error', se.tolist())
    print('unshadowed', unshadowed.tolist(), 'overshoot in standard errors', (overshoot / se).tolist())
    print('shadowed', shadowed.tolist(), 'deviation', deviation.tolist(), 'of the overshoot', (deviation / overshoot).tolist())
    assert bool((se > 0).all()) and bool((overshoot > 20.0 * se).all()), 'the blocker does nothing'
    assert bool((deviation <= 0.25 * overshoot).all()), (deviation / overshoot).tolist()
    assert bool((deviation < 2.0 * torch.tensor(MEASURED_DEVIATION, dtype=torch.float64)).all()), deviation.tolist()
