"""Ambient occlusion in deferred shading (rdr_deferred_shade with `ao_occluders`; redner_amd.render_utils:
deferred_shade(ambient_occlusion=K), render_deferred(ambient_occlusion=K, ao_radius=r)): K any-hit hemisphere rays per texel,
one word per texel, the escaping fraction o = popcount(word) / K on the ambient and SH rows.

What the cases are held to:
  * the words against a brute-force fp64 intersector (test_deferred_shadows.any_hit64), rays formed by the rule of
    include/redner_amd.h in numpy fp64 from the fp32-rounded direction table.  A ray whose fp64 answer changes when every blocker is
    scaled about its centroid by 1 +- 1e-3 or, for a finite radius, when the radius is scaled by 1 +- 1e-3 is a boundary ray and
    is left out: at most 2 % of the cast rays, with at least 10 % robustly blocked and 10 % robustly escaping;
  * values and gradients against the fp64 definition (test_deferred_sh.definition, one row at a time), its sky rows scaled by
    the o of the device's own words, held constant, at parity_util.TOL (1e-4 relative L2) per image slice, per G-buffer slice
    and per light row;
  * bit-for-bit equality with the call without occlusion wherever nothing is in reach or no sky row is present, with the
    single-image call in a batch, with contiguous inputs under the calling contract, across chunk sizes, and from run to run.
Every case runs on the CPU harness; the GPU legs run the same bodies on both builds of the library.  Frames are a few hundred to
a few thousand texels."""
import os

import numpy as np
import pytest
import torch

import parity_util
import scenes
from golden import make_deferred_golden as mk
from test_deferred import _off_the_kinks, _worst_slice
from test_deferred_sh import definition, sh_coefficients, sh_off_the_kink, sh_rows
from test_deferred_shadows import (AA, BLOCKERS, FAR_AWAY, HG, LIGHTS, WG, any_hit64, any_rays, as_words, floor_g_buffer,
                                   occluder)

CPU, GPU = torch.device('cpu'), torch.device('cuda:0')
INF = float('inf')
SKY = (0, 4, 5, 6)                            # the rows occlusion scales: ambient and the three SH rows
_cache = {}


def _ru():
    from redner_amd import render_utils
    return render_utils


def ao_lights(seed=3):
    """ambient, an SH triple of nine coefficients, point, directional, spot: seven rows"""
    types4, params4 = mk.light_table(LIGHTS)
    t_sh, r_sh = sh_rows(sh_coefficients(seed))
    types = [int(types4[0])] + t_sh + [int(t) for t in types4[1:]]
    return types, np.concatenate([params4[0:1], r_sh, params4[1:]]).astype(np.float32)


# ---- the rule in numpy ---------------------------------------------------------------------------------------------------------------
def direction_table(k):
    """[16, K, 3]: fp64, rounded once to fp32 (the rotations sit half a step off 0, as include/redner_amd.h states)"""
    table = np.zeros((16, k, 3))
    for j in range(16):
        for r in range(k):
            u2, digit, b = 0.0, 0.5, r
            while b:
                u2 += digit * (b & 1)
                b >>= 1
                digit *= 0.5
            u1, phi = (r + 0.5) / k, 2.0 * np.pi * (u2 + (j + 0.5) / 16.0)
            table[j, r] = (np.sqrt(u1) * np.cos(phi), np.sqrt(u1) * np.sin(phi), np.sqrt(1.0 - u1))
    return table.astype(np.float32)


def casts(g):
    """g [hg, wg, >= 6] fp32 -> [hg, wg] bool: 0 < n.n < inf in fp32, p and n / sqrt(n.n) finite"""
    p, n = g[..., 0:3].astype(np.float32), g[..., 3:6].astype(np.float32)
    with np.errstate(all='ignore'):
        nn = (n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]
        ok = (nn > 0) & np.isfinite(nn)
        nh = n / np.sqrt(nn)[..., None]
        return ok & np.isfinite(p).all(-1) & np.isfinite(nh).all(-1)


def rays64(g, k):
    """-> cast [hg, wg], origins [hg, wg, 3], dirs [hg, wg, K, 3] in fp64 by the stated rule (Duff's frame about n / |n|)"""
    hg, wg = g.shape[:2]
    cast = casts(g)
    p, n = g[..., 0:3].astype(np.float64), g[..., 3:6].astype(np.float64)
    table = direction_table(k).astype(np.float64)
    with np.errstate(all='ignore'):
        nh = np.where(cast[..., None], n / np.sqrt((n * n).sum(-1))[..., None], np.array([0.0, 0.0, 1.0]))
    s = np.copysign(1.0, nh[..., 2])
    a = -1.0 / (s + nh[..., 2])
    b = nh[..., 0] * nh[..., 1] * a
    t = np.stack([1.0 + s * nh[..., 0] * nh[..., 0] * a, s * b, -s * nh[..., 0]], -1)
    bt = np.stack([b, s + nh[..., 1] * nh[..., 1] * a, -nh[..., 1]], -1)
    yy, xx = np.meshgrid(np.arange(hg), np.arange(wg), indexing='ij')
    local = table[(xx & 3) + 4 * (yy & 3)]                                # [hg, wg, K, 3]
    d = local[..., 0:1] * t[:, :, None] + local[..., 1:2] * bt[:, :, None] + local[..., 2:3] * nh[:, :, None]
    return cast, p, d


def brute_words(g, k, radius, tris):
    """-> words [hg, wg] uint32, cast [hg, wg], robust [hg, wg, K], escaped [hg, wg, K]"""
    tris = np.asarray(tris, np.float64)
    centre = tris.mean(axis=1, keepdims=True)
    hg, wg = g.shape[:2]
    cast, p, d = rays64(g, k)
    o = np.repeat(p[:, :, None], k, axis=2).reshape(-1, 3)
    variants = [(1.0, 1.0), (1.0 + 1e-3, 1.0), (1.0 - 1e-3, 1.0)]
    if np.isfinite(radius):
        variants += [(1.0, 1.0 + 1e-3), (1.0, 1.0 - 1e-3)]
    answers = [any_hit64(o, d.reshape(-1, 3), np.full(len(o), radius * rs), centre + ts * (tris - centre)).reshape(hg, wg, k)
               for ts, rs in variants]
    robust = np.all([a == answers[0] for a in answers[1:]], axis=0)
    escaped = ~(cast[..., None] & answers[0])
    words = (escaped.astype(np.uint32) << np.arange(k, dtype=np.uint32)).sum(-1).astype(np.uint32)
    return words, cast, robust, escaped


# ---- calling ---------------------------------------------------------------------------------------------------------------------------
def shade(backend, device, g, types, params, ranges, aa, alpha, occluders=None, ao=None, up=None):
    """forward (+ backward when `up` is given) through DeferredShade.  `ao`: None, or (occluder scenes, K, radius).
    -> dict(image, vis, words, d_g, d_p), the extras None where they were not asked for"""
    ru = _ru()
    gl = g.to(device).clone().requires_grad_(True)
    pl = torch.from_numpy(np.asarray(params, np.float32)).to(device).requires_grad_(True)
    unwrap = lambda occ: None if occ is None else tuple(o.scene if o is not None else None for o in occ)
    args = [gl, pl, tuple(types), tuple(ranges), aa, bool(alpha), backend, unwrap(occluders)]
    if ao is not None:
        args += [unwrap(ao[0]), ao[1], ao[2]]
    out = ru.DeferredShade.apply(*args)
    out = list(out) if isinstance(out, tuple) else [out]
    assert len(out) == 1 + (occluders is not None) + (ao is not None)
    res = dict(image=out[0].detach().cpu(), vis=out[1].cpu() if occluders is not None else None,
               words=out[-1].cpu() if ao is not None else None, d_g=None, d_p=None)
    if up is not None:
        out[0].backward(up.to(device))
        res.update(d_g=gl.grad.cpu(), d_p=pl.grad.cpu())
    return res


def same(a, b, keys=('image', 'd_g', 'd_p')):
    for k in keys:
        assert (a[k] is None) == (b[k] is None), k
        assert a[k] is None or torch.equal(a[k], b[k]), k


def factor(words, k):
    """[..] int32 words -> o in fp64, as the kernels form it: (float)popcount / (float)K"""
    w = as_words(words)
    count = sum(((w >> np.uint32(b)) & 1).astype(np.int64) for b in range(32))
    return torch.from_numpy((count.astype(np.float32) / np.float32(k)).astype(np.float64))


def definition_ao(g, types, params, ranges, o, lit, aa, alpha):
    """sum over the rows of the one-row fp64 definition, sky rows times o [N, hg, wg], every row times its mask lit[l]
    [N, hg, wg] (None: no shadows), resolved over aa"""
    n, hg, wg, _ = g.shape
    rgb = torch.zeros(n, hg, wg, 3, dtype=torch.float64)
    for l, t in enumerate(types):
        uses = torch.tensor([1.0 if b <= l < e else 0.0 for b, e in ranges], dtype=torch.float64)
        one = definition(g[..., :9], [t], params[l:l + 1], ((0, 1),) * n, 1, 0) * uses[:, None, None, None]
        if t in SKY:
            one = one * o[..., None]
        if lit is not None:
            one = one * lit[l][..., None]
        rgb = rgb + one
    img = torch.cat([rgb, g[..., 9:10]], dim=-1) if alpha else rgb
    return img.reshape(n, hg // aa, aa, wg // aa, aa, img.shape[-1]).mean(dim=(2, 4))


def tilted_floor(alpha, seed=41):
    """the floor patch with normals tilted from texel to texel and NOT of unit length (the rays go about n / |n|), taken off the
    kinks of the seven lights"""
    types, params = ao_lights()
    g = floor_g_buffer(HG, WG, alpha, seed=seed)
    yy, xx = torch.meshgrid(torch.arange(HG, dtype=torch.float32), torch.arange(WG, dtype=torch.float32), indexing='ij')
    body = slice(2, HG)
    g[0, body, :, 3] = (0.3 * torch.sin(0.9 * xx + 0.4 * yy))[body]
    g[0, body, :, 4] = (0.25 * torch.cos(0.7 * yy - 0.3 * xx))[body]
    g[0, body] = torch.cat([g[0, body, :, :3], g[0, body, :, 3:6] * (0.6 + 0.05 * xx[body])[..., None], g[0, body, :, 6:]], dim=-1)
    g, _ = _off_the_kinks(g, [t for t in types if t < 4], params[[l for l, t in enumerate(types) if t < 4]])
    g, _, _ = sh_off_the_kink(g, types, params)
    return g.contiguous(), types, params


# ---- 1. off is off -------------------------------------------------------------------------------------------------------------------
def _run_off_is_off(backend, device):
    ru = _ru()
    blockers = occluder(backend, BLOCKERS, device)
    spec = [ru.AmbientLight(torch.tensor([0.2, 0.25, 0.3])), ru.SHLight(torch.from_numpy(sh_coefficients(3))),
            ru.PointLight(torch.tensor([0.3, 0.2, 2.0]), torch.tensor([30.0, 25.0, 20.0]))]
    for alpha in (0, 1):
        g = floor_g_buffer(HG, WG, alpha)
        up = mk.upstream((1, HG // AA, WG // AA, 3 + alpha)).to(device)
        for kw in ({}, {'occluders': blockers}, {'occluders': blockers, 'return_visibility': True}):
            results = []
            for extra in ({}, {'ambient_occlusion': 0}, {'ambient_occlusion': 0, 'ao_radius': 0.5, 'ao_occluders': None,
                                                           'return_occlusion': False}):
                leaf = g.to(device).clone().requires_grad_(True)
                inten = torch.tensor([0.2, 0.25, 0.3], requires_grad=True)
                lights = [ru.AmbientLight(inten)] + spec[1:]
                out = ru.deferred_shade(leaf, lights, alpha=bool(alpha), aa_samples=AA, backend=backend, **kw, **extra)
                outs = out if isinstance(out, tuple) else (out,)
                outs[0].backward(up)
                results.append((type(out), [o.detach().cpu() for o in outs], leaf.grad.cpu(), inten.grad.clone()))
            for other in results[1:]:
                assert other[0] is results[0][0] and len(other[1]) == len(results[0][1])
                assert all(torch.equal(a, b) for a, b in zip(other[1], results[0][1]))
                assert torch.equal(other[2], results[0][2]) and torch.equal(other[3], results[0][3])


def test_off_is_off_hostsim(hostsim_backend):
    _run_off_is_off(hostsim_backend, CPU)


@pytest.mark.gpu
def test_off_is_off_gpu(gpu_backend):
    _run_off_is_off(gpu_backend, GPU)


# ---- 2. nothing in reach is bit for bit nothing -----------------------------------------------------------------------------------
def _run_nothing_in_reach(backend, device):
    types, params = ao_lights()
    types, params = types[:6], params[:6]                                  # ambient, the SH triple, point, directional
    far, near = occluder(backend, FAR_AWAY, device), occluder(backend, BLOCKERS, device)
    for alpha in (0, 1):
        g = floor_g_buffer(HG, WG, alpha)
        up = mk.upstream((1, HG // AA, WG // AA, 3 + alpha))
        plain = shade(backend, device, g, types, params, ((0, 6),), AA, alpha, up=up)
        for k in (1, 16, 32):
            for occ, radius in ((far, INF), (near, 0.05)):                 # the blockers start 0.40 above the floor
                got = shade(backend, device, g, types, params, ((0, 6),), AA, alpha, ao=((occ,), k, radius), up=up)
                assert (as_words(got['words']) == (1 << k) - 1).all(), (alpha, k, radius)
                same(got, plain)


def test_nothing_in_reach_hostsim(hostsim_backend):
    _run_nothing_in_reach(hostsim_backend, CPU)


@pytest.mark.gpu
def test_nothing_in_reach_gpu(gpu_backend):
    _run_nothing_in_reach(gpu_backend, GPU)


# ---- 3. the words against the fp64 brute force ------------------------------------------------------------------------------------
def _brute(k, radius):
    if ('brute', k, radius) not in _cache:
        _cache['brute', k, radius] = brute_words(floor_g_buffer(HG, WG, 0)[0].numpy(), k, radius, BLOCKERS)
    return _cache['brute', k, radius]


def _run_words(backend, device):
    types, params = ao_lights()
    g = floor_g_buffer(HG, WG, 0)
    blockers = occluder(backend, BLOCKERS, device)
    blocked_at = {}
    for k in (4, 16, 32):
        for radius in (INF, 0.8):
            _, cast, robust, escaped = _brute(k, radius)
            got = as_words(shade(backend, device, g, types, params, ((0, 7),), AA, 0, ao=((blockers,), k, radius))['words'])[0]
            bits = ((got[..., None] >> np.arange(k, dtype=np.uint32)) & 1).astype(bool)
            rays, keep = int(cast.sum()) * k, robust & cast[..., None]
            left_out = rays - int(keep.sum())
            blocked, free = int((keep & ~escaped).sum()), int((keep & escaped).sum())
            print('K %2d radius %s: cast rays %d, left out %d, robustly blocked %d (%.1f %%), escaping %d'
                  % (k, radius, rays, left_out, blocked, 100.0 * blocked / rays, free))
            assert int(cast.sum()) == 432 and rays == 432 * k
            assert left_out <= 0.02 * rays and blocked >= 0.10 * rays and free >= 0.10 * rays
            assert (bits[keep] == escaped[keep]).all(), '%d robust bits differ' % int((bits != escaped)[keep].sum())
            assert (bits[~cast]).all()                                     # a texel that does not cast: all K bits
            assert (got >> np.uint32(k) == 0).all() if k < 32 else True
            assert (got[:2] == (1 << k) - 1).all()                         # the two background rows
            blocked_at[k, radius] = int((cast[..., None] & ~bits).sum())
        assert blocked_at[k, 0.8] < blocked_at[k, INF], k


def test_words_against_brute_force_hostsim(hostsim_backend):
    _run_words(hostsim_backend, CPU)


@pytest.mark.gpu
def test_words_against_brute_force_gpu(gpu_backend):
    _run_words(gpu_backend, GPU)


# ---- 4. values and gradients against the fp64 definition, occlusion held constant ------------------------------------------------
def _check_definition(got, g, types, params, ranges, k, aa, alpha, up, what):
    """`got` of shade(..., up=up) against definition_ao with the o (and the visibility) of the device's own words"""
    o = factor(got['words'], k)
    lit = None
    if got['vis'] is not None:
        vis = as_words(got['vis'])
        lit = []
        for l in range(len(types)):
            rows = [((vis[n] >> np.uint32(l - b)) & 1).astype(np.float64) if b <= l < e else np.zeros(vis[n].shape)
                    for n, (b, e) in enumerate(ranges)]
            lit.append(torch.from_numpy(np.stack(rows)))
    g64 = g.double().requires_grad_(True)
    p64 = torch.from_numpy(np.asarray(params)).double().requires_grad_(True)
    want = definition_ao(g64, types, p64, ranges, o, lit, aa, alpha)
    want.backward(up.double())
    errors = {'image': _worst_slice(got['image'], want.detach(), 'image'), 'd_g_buffer': _worst_slice(got['d_g'], g64.grad, 'd_g_buffer'),
              'd_light_params': _worst_slice(got['d_p'], p64.grad, 'd_light_params')}
    print(what, {name: '%.2e' % v for name, v in errors.items()})
    for name, v in errors.items():
        assert v < parity_util.TOL, (what, name, v)
    return o


def _run_values_and_gradients(backend, device):
    blockers = occluder(backend, BLOCKERS, device)
    for alpha, aa, k, radius in ((0, 1, 16, INF), (1, 2, 16, INF), (1, 1, 5, 0.8), (0, 2, 32, 0.8)):
        g, types, params = tilted_floor(alpha)
        up = mk.upstream((1, HG // aa, WG // aa, 3 + alpha))
        got = shade(backend, device, g, types, params, ((0, 7),), aa, alpha, ao=((blockers,), k, radius), up=up)
        o = _check_definition(got, g, types, params, ((0, 7),), k, aa, alpha, up, 'alpha %d aa %d K %d radius %s' % (alpha, aa, k, radius))
        assert float(o.min()) < 0.8 and float((o == 1).double().mean()) > 0.1 and float((o < 1).double().mean()) > 0.1
    # only point and directional rows: occlusion touches no other row
    g, types, params = tilted_floor(1)
    up = mk.upstream((1, HG // AA, WG // AA, 4))
    plain = shade(backend, device, g, types[4:6], params[4:6], ((0, 2),), AA, 1, up=up)
    got = shade(backend, device, g, types[4:6], params[4:6], ((0, 2),), AA, 1, ao=((blockers,), 16, INF), up=up)
    assert (as_words(got['words']) != 0xffff).any()
    same(got, plain)


def test_values_and_gradients_hostsim(hostsim_backend):
    _run_values_and_gradients(hostsim_backend, CPU)


@pytest.mark.gpu
def test_values_and_gradients_gpu(gpu_backend):
    _run_values_and_gradients(gpu_backend, GPU)


# ---- 5. with shadows ---------------------------------------------------------------------------------------------------------------
def _run_with_shadows(backend, device):
    alpha, k = 1, 8
    g, types, params = tilted_floor(alpha)
    up = mk.upstream((1, HG // AA, WG // AA, 4))
    blockers = occluder(backend, BLOCKERS, device)
    roof = occluder(backend, [[[-0.9, -0.9, 0.3], [0.9, -0.8, 0.3], [0.0, 0.9, 0.35]]], device)
    shadows_only = shade(backend, device, g, types, params, ((0, 7),), AA, alpha, occluders=(blockers,), up=up)
    for ao_occ in (blockers, roof):                                        # the same occluders, and different ones
        ao_only = shade(backend, device, g, types, params, ((0, 7),), AA, alpha, ao=((ao_occ,), k, 0.9), up=up)
        both = shade(backend, device, g, types, params, ((0, 7),), AA, alpha, occluders=(blockers,), ao=((ao_occ,), k, 0.9), up=up)
        assert torch.equal(both['vis'], shadows_only['vis']) and torch.equal(both['words'], ao_only['words'])
        assert (as_words(both['vis']) != 127).any() and (as_words(both['words']) != 255).any()
        _check_definition(both, g, types, params, ((0, 7),), k, AA, alpha, up, 'with shadows')
    # 33 ambient rows: too many for a shadowed image, fine for one that is only occluded
    many_types, many = [0] * 33, np.tile(params[0:1], (33, 1)) * (1.0 + 0.01 * np.arange(33, dtype=np.float32))[:, None]
    got = shade(backend, device, g, many_types, many, ((0, 33),), AA, alpha, ao=((blockers,), k, 0.9), up=up)
    _check_definition(got, g, many_types, many, ((0, 33),), k, AA, alpha, up, '33 rows')
    with pytest.raises(RuntimeError, match='image 0 has 33 lights'):
        shade(backend, device, g, many_types, many, ((0, 33),), AA, alpha, occluders=(blockers,), ao=((blockers,), k, 0.9))


def test_with_shadows_hostsim(hostsim_backend):
    _run_with_shadows(hostsim_backend, CPU)


@pytest.mark.gpu
def test_with_shadows_gpu(gpu_backend):
    _run_with_shadows(gpu_backend, GPU)


# ---- 6. batch ------------------------------------------------------------------------------------------------------------------------
def _run_batch(backend, device):
    alpha, k = 1, 16
    types, params = ao_lights()
    g = torch.cat([floor_g_buffer(HG, WG, alpha, seed=s) for s in (21, 22, 23)])
    ranges = ((0, 7), (0, 4), (1, 6))                                      # per-image light lists; every one has sky rows
    occ = (occluder(backend, BLOCKERS, device), None, occluder(backend, BLOCKERS[:1], device))
    up = mk.upstream((3, HG // AA, WG // AA, 4))
    whole = shade(backend, device, g, types, params, ranges, AA, alpha, ao=(occ, k, INF), up=up)
    words = as_words(whole['words'])
    assert (words[0] != 0xffff).any() and (words[1] == 0xffff).all() and (words[2] != 0xffff).any()
    assert (words[0] != words[2]).any()
    for n in range(3):
        one = shade(backend, device, g[n:n + 1], types, params, ranges[n:n + 1], AA, alpha, ao=(occ[n:n + 1], k, INF), up=up[n:n + 1])
        assert torch.equal(one['image'][0], whole['image'][n]) and torch.equal(one['words'][0], whole['words'][n]), n
        assert torch.equal(one['d_g'][0], whole['d_g'][n]), n
    none = shade(backend, device, g[1:2], types, params, ranges[1:2], AA, alpha, up=up[1:2])
    assert torch.equal(none['image'][0], whole['image'][1]) and torch.equal(none['d_g'][0], whole['d_g'][1])
    assert torch.equal(shade(backend, device, g[0:1], types, params, ranges[0:1], AA, alpha, ao=(occ[0:1], k, INF),
                             up=up[0:1])['d_p'][6], whole['d_p'][6])         # the spot row: image 0 alone uses it


def test_batch_hostsim(hostsim_backend):
    _run_batch(hostsim_backend, CPU)


@pytest.mark.gpu
def test_batch_gpu(gpu_backend):
    _run_batch(gpu_backend, GPU)


# ---- 7. chunks -----------------------------------------------------------------------------------------------------------------------
def _run_chunks(backend, device):
    types, params = ao_lights()
    g = floor_g_buffer(40, 40, 0, seed=12)
    blockers = occluder(backend, BLOCKERS, device)
    up = mk.upstream((1, 40, 40, 3))
    for k in (16, 3):
        whole = shade(backend, device, g, types, params, ((0, 7),), 1, 0, ao=((blockers,), k, INF), up=up)
        assert (as_words(whole['words']) != (1 << k) - 1).any()
        # 1000 rays per chunk: 62 (K = 16) or 333 (K = 3) texels, neither a multiple of the 40-texel row nor 1000 of K
        os.environ['RDR_DEFERRED_SHADOW_CHUNK'] = '1000'
        try:
            chunked = shade(backend, device, g, types, params, ((0, 7),), 1, 0, ao=((blockers,), k, INF), up=up)
        finally:
            del os.environ['RDR_DEFERRED_SHADOW_CHUNK']
        same(whole, chunked, ('image', 'words', 'd_g', 'd_p'))
    os.environ['RDR_DEFERRED_SHADOW_CHUNK'] = '7'                          # fewer rays than K: one texel per chunk
    try:
        tiny = shade(backend, device, g[:, 18:22, 18:24].contiguous(), types, params, ((0, 7),), 1, 0, ao=((blockers,), 16, INF))
    finally:
        del os.environ['RDR_DEFERRED_SHADOW_CHUNK']
    ref = shade(backend, device, g[:, 18:22, 18:24].contiguous(), types, params, ((0, 7),), 1, 0, ao=((blockers,), 16, INF))
    same(tiny, ref, ('image', 'words'))


def test_chunks_hostsim(hostsim_backend):
    _run_chunks(hostsim_backend, CPU)


@pytest.mark.gpu
def test_chunks_gpu(gpu_backend):
    _run_chunks(gpu_backend, GPU)


# ---- 8. degenerate texels ------------------------------------------------------------------------------------------------------------
def _run_degenerate(backend, device, harness):
    types, params = ao_lights()
    k = 8
    g = floor_g_buffer(HG, WG, 0, seed=31)
    blockers = occluder(backend, BLOCKERS, device)
    clean = as_words(shade(backend, device, g, types[:4], params[:4], ((0, 4),), 1, 0, ao=((blockers,), k, INF))['words'])[0]
    assert (clean[HG - 2:] == 255).all() and casts(g[0].numpy())[HG - 2:].all()      # normal (0, 0, -1): casts, and escapes downwards
    assert int(casts(g[0].numpy()).sum()) == (HG - 2) * WG
    bad = g.clone()
    spots = [(5, 3), (6, 7), (7, 11), (8, 2), (9, 9), (10, 14), (11, 5)]
    bad[0, 5, 3, 3:6] = 0.0                                                # normal 0
    bad[0, 6, 7, 1] = float('nan')                                         # NaN in p
    bad[0, 7, 11, 0] = float('inf')                                        # inf in p
    bad[0, 8, 2, 4] = float('nan')                                         # NaN in n
    bad[0, 9, 9, 5] = float('inf')                                         # inf in n: n.n overflows
    bad[0, 10, 14, 3:6] = torch.tensor([1e-30, 0.0, 1e-30])                # n.n underflows to 0
    bad[0, 11, 5, 3:6] = torch.tensor([1e30, 0.0, 1e30])                   # n.n overflows to inf
    assert not any(casts(bad[0].numpy())[y, x] for y, x in spots)
    before = any_rays(backend)
    got = shade(backend, device, bad, types[:4], params[:4], ((0, 4),), 1, 0, ao=((blockers,), k, INF))      # the call returns
    if harness:                                                            # (the GPU build tallies the queues' upper bounds)
        assert any_rays(backend) - before == k * ((HG - 2) * WG - len(spots))
    words = as_words(got['words'])[0]
    mask = np.ones((HG, WG), bool)
    for y, x in spots:
        assert words[y, x] == 255, (y, x)
        mask[y, x] = False
    assert (words[mask] == clean[mask]).all() and (clean[[y for y, _ in spots], [x for _, x in spots]] != 255).any()


def test_degenerate_texels_hostsim(hostsim_backend):
    _run_degenerate(hostsim_backend, CPU, True)


@pytest.mark.gpu
def test_degenerate_texels_gpu(gpu_backend):
    _run_degenerate(gpu_backend, GPU, False)


# ---- 9. errors -----------------------------------------------------------------------------------------------------------------------
def _run_errors(rd, device):
    """every error of the occlusion fields, raised before anything is launched: the same texts from the harness and from the GPU
    library (every tensor lives as long as the calls that were given its address)"""
    ru = _ru()
    on_gpu = device.type == 'cuda'
    blockers = occluder(rd, BLOCKERS, device)
    g = floor_g_buffer(4, 4, 0).to(device)
    ptr = lambda t: rd.float_ptr(t.data_ptr())
    img, words = torch.zeros(1, 4, 4, 3, device=device), torch.zeros(17, dtype=torch.int32, device=device)
    vis = torch.zeros(16, dtype=torch.int32, device=device)
    params = torch.zeros(1, 10, device=device)
    call = lambda **kw: rd.deferred_shade(ptr(g), ptr(params), ptr(img), 1, 4, 4, 1, False, [0], [(0, 1)], on_gpu, 0, **kw)
    d_g, d_p = torch.zeros_like(g), torch.zeros_like(params)
    back = lambda **kw: rd.deferred_shade_backward(ptr(g), ptr(params), ptr(img), ptr(d_g), ptr(d_p), 1, 4, 4, 1, False, [0], [(0, 1)],
                                                   on_gpu, 0, **kw)
    wp = rd.int_ptr(words.data_ptr())
    for rays in (0, 33, -1):
        with pytest.raises(RuntimeError, match='ao_rays must be 1 .. 32'):
            call(ao_occluders=[blockers.scene], ao_words=wp, ao_rays=rays, ao_radius=1.0)
        with pytest.raises(RuntimeError, match='ao_rays must be 1 .. 32'):
            back(ao_words=wp, ao_rays=rays)
    for radius in (0.0, -1.0, float('nan'), -INF):
        with pytest.raises(RuntimeError, match='ao_radius must be positive'):
            call(ao_occluders=[blockers.scene], ao_words=wp, ao_rays=4, ao_radius=radius)
    with pytest.raises(RuntimeError, match='ao_occluders need an ao_words buffer'):
        call(ao_occluders=[blockers.scene], ao_rays=4, ao_radius=1.0)
    with pytest.raises(RuntimeError, match='an ao_words buffer needs ao_occluders'):
        call(ao_words=wp, ao_rays=4, ao_radius=1.0)
    with pytest.raises(RuntimeError, match='ao_words buffer must be 4-byte aligned'):
        call(ao_occluders=[blockers.scene], ao_words=rd.int_ptr(words.data_ptr() + 2), ao_rays=4, ao_radius=1.0)
    with pytest.raises(RuntimeError, match='ao_words buffer must be 4-byte aligned'):
        back(ao_words=rd.int_ptr(words.data_ptr() + 2), ao_rays=4)
    with pytest.raises(RuntimeError, match='2 ao occluder scenes for 1 images'):
        call(ao_occluders=[blockers.scene, None], ao_words=wp, ao_rays=4, ao_radius=1.0)
    with pytest.raises(RuntimeError, match='an ao occluder must be a live Scene'):
        call(ao_occluders=[blockers], ao_words=wp, ao_rays=4, ao_radius=1.0)
    call(ao_occluders=[blockers.scene], ao_words=wp, ao_rays=32, ao_radius=INF)          # the largest K, an unbounded radius
    assert (as_words(words.cpu())[:16] == 0xffffffff).all() and int(words[16]) == 0       # 16 words written (nothing is in reach), no more
    back(ao_words=wp, ao_rays=32)                                                      # the words alone
    # the Python layer
    amb = [ru.AmbientLight(torch.ones(3))]
    with pytest.raises(RuntimeError, match='deferred_shade: ambient_occlusion needs ao_occluders or occluders'):
        ru.deferred_shade(g, amb, ambient_occlusion=4, backend=rd)
    with pytest.raises(RuntimeError, match='ambient_occlusion must be 0 .off. or 1 .. 32'):
        ru.deferred_shade(g, amb, ambient_occlusion=33, ao_occluders=blockers, backend=rd)
    with pytest.raises(RuntimeError, match='deferred_shade: ao_occluders holds 2 occluder scenes for 1 images'):
        ru.deferred_shade(g, amb, ambient_occlusion=4, ao_occluders=[blockers, blockers], backend=rd)
    with pytest.raises(RuntimeError, match='deferred_shade: occluders holds 2 occluder scenes for 1 images'):
        ru.deferred_shade(g, amb, ambient_occlusion=4, occluders=[blockers, blockers], ao_occluders=blockers, backend=rd)
    with pytest.raises(RuntimeError, match='2 ao occluder scenes for 1 images'):
        ru.DeferredShade.apply(g, params, (0,), ((0, 1),), 1, False, rd, None, (blockers.scene, None), 4, 1.0)
    with pytest.raises(RuntimeError, match='ao_radius must be positive'):
        ru.deferred_shade(g, amb, ambient_occlusion=4, ao_radius=0.0, ao_occluders=blockers, backend=rd)
    sc = scenes.glossy_floor_blocker(device, resolution=(4, 4))
    with pytest.raises(RuntimeError, match='ambient_occlusion must be 0 .off. or 1 .. 32'):
        ru.render_deferred(sc, amb, aa_samples=1, seed=1, device=device, backend=rd, ambient_occlusion=40)
    # what was refused before is refused as before
    with pytest.raises(RuntimeError, match='unknown light type'):
        rd.deferred_shade(ptr(g), ptr(params), ptr(img), 1, 4, 4, 1, False, [7], [(0, 1)], on_gpu, 0,
                          ao_occluders=[blockers.scene], ao_words=wp, ao_rays=4, ao_radius=1.0)
    with pytest.raises(RuntimeError, match='occluders need a visibility buffer'):
        call(occluders=[blockers.scene], ao_occluders=[blockers.scene], ao_words=wp, ao_rays=4, ao_radius=1.0)
    with pytest.raises(RuntimeError, match='must be 4-byte aligned'):
        call(occluders=[blockers.scene], visibility=rd.int_ptr(vis.data_ptr() + 2), ao_occluders=[blockers.scene], ao_words=wp,
             ao_rays=4, ao_radius=1.0)
    with pytest.raises(RuntimeError, match='light_params must be'):
        ru.DeferredShade.apply(g, params, (0, 1), ((0, 2),), 1, False, rd, None, (blockers.scene,), 4, 1.0)


def test_errors_hostsim(hostsim_backend):
    _run_errors(hostsim_backend, CPU)


@pytest.mark.gpu
def test_errors_gpu(gpu_backend):
    _run_errors(gpu_backend, GPU)


@pytest.mark.gpu
def test_scene_on_another_device_gpu(gpu_backend):
    """the one error that only the GPU library has: an occluder scene that lives on another device than the call's gpu_index"""
    if torch.cuda.device_count() < 2:
        pytest.skip('needs two GPUs (the round-end multi-GPU tier)')
    rd, ru = gpu_backend, _ru()
    other = torch.device('cuda:1')
    elsewhere, here = occluder(rd, BLOCKERS, other), occluder(rd, BLOCKERS, GPU)
    g = floor_g_buffer(4, 4, 0).to(GPU)
    amb = [ru.AmbientLight(torch.ones(3))]
    with pytest.raises(RuntimeError, match='the ao occluder scene of image 0 lives on device 1, the call runs on device 0'):
        ru.deferred_shade(g, amb, ambient_occlusion=4, ao_occluders=elsewhere, backend=rd)
    with pytest.raises(RuntimeError, match='the ao occluder scene of image 0 lives on device 1, the call runs on device 0'):
        ru.deferred_shade(g, amb, ambient_occlusion=4, occluders=here, ao_occluders=elsewhere, backend=rd)
    with pytest.raises(RuntimeError, match='the occluder scene of image 0 lives on device 1'):
        ru.deferred_shade(g, amb, ambient_occlusion=4, occluders=elsewhere, ao_occluders=here, backend=rd)
    img, words = ru.deferred_shade(g, amb, ambient_occlusion=4, ao_occluders=here, backend=rd, return_occlusion=True)
    assert bool(torch.isfinite(img).all()) and tuple(words.shape) == (1, 4, 4)


# ---- 10. calling contract ------------------------------------------------------------------------------------------------------------
def _run_calling_contract(backend, device):
    ru = _ru()
    g0, types, params = tilted_floor(1)
    blockers = occluder(backend, BLOCKERS, device)
    params = torch.from_numpy(params).to(device)
    k = 16

    def args(alpha):
        return (tuple(types), ((0, 7),), AA, bool(alpha), backend, None, (blockers.scene,), k, 0.9)

    for alpha in (0, 1):
        g = g0[..., :9 + alpha].contiguous().to(device)
        up = mk.upstream((1, HG // AA, WG // AA, 3 + alpha)).to(device)
        fresh = g.clone().requires_grad_(True)
        img, words = ru.DeferredShade.apply(fresh, params, *args(alpha))
        img.backward(up)
        assert (as_words(words.cpu()) != 0xffff).any()
        wide = torch.zeros(1, HG, WG, 14, device=device)                     # a view that is not contiguous
        wide[..., 3:12 + alpha] = g
        wide.requires_grad_(True)
        img_v, words_v = ru.DeferredShade.apply(wide[..., 3:12 + alpha], params, *args(alpha))
        img_v.backward(up)
        assert torch.equal(img_v, img) and torch.equal(words_v, words) and torch.equal(wide.grad[..., 3:12 + alpha], fresh.grad)
        flat = torch.zeros(g.numel() + 1, device=device)                     # contiguous at an odd float offset: with alpha, misaligned
        flat[1:] = g.reshape(-1)
        flat.requires_grad_(True)
        odd = flat[1:].view_as(g)
        assert odd.is_contiguous() and odd.data_ptr() % 8 == 4
        img_o, words_o = ru.DeferredShade.apply(odd, params, *args(alpha))
        img_o.backward(up)
        assert torch.equal(img_o, img) and torch.equal(words_o, words) and torch.equal(flat.grad[1:].view_as(g), fresh.grad)
        ones = g.clone().requires_grad_(True)
        ru.DeferredShade.apply(ones, params, *args(alpha))[0].sum().backward()                     # a stride-0 upstream gradient
        ref = g.clone().requires_grad_(True)
        ru.DeferredShade.apply(ref, params, *args(alpha))[0].backward(torch.ones_like(img))          # (its occlusion output unused)
        assert torch.equal(ones.grad, ref.grad)
        big = torch.zeros(1, HG // AA, WG // AA, 2 * (3 + alpha), device=device)
        big[..., ::2] = up
        strided = g.clone().requires_grad_(True)
        ru.DeferredShade.apply(strided, params, *args(alpha))[0].backward(big[..., ::2])             # a non-contiguous one
        assert torch.equal(strided.grad, fresh.grad)
        leaf = g.clone().requires_grad_(True)
        edited = leaf * 1.0                                                                            # contiguous: saved as it is
        out = ru.DeferredShade.apply(edited, params, *args(alpha))[0]
        edited.mul_(2.0)
        with pytest.raises(RuntimeError, match='modified by an inplace operation'):
            out.sum().backward()
    assert not words.requires_grad and words.dtype == torch.int32


def test_calling_contract_hostsim(hostsim_backend):
    _run_calling_contract(hostsim_backend, CPU)


@pytest.mark.gpu
def test_calling_contract_gpu(gpu_backend):
    _run_calling_contract(gpu_backend, GPU)


# ---- 11. end to end ------------------------------------------------------------------------------------------------------------------
def _run_end_to_end(backend, device):
    ru = _ru()
    res, aa, seed, k, radius = 16, 2, 9, 8, 9.0

    def scene_and_lights():
        sc = scenes.glossy_floor_blocker(device, resolution=(res, res))
        sc.materials[0] = scenes.Material(diffuse_reflectance=scenes._t([0.6, 0.5, 0.4], device))     # a floor that is lit
        lights = [ru.AmbientLight(torch.tensor([0.3, 0.35, 0.4], requires_grad=True)),
                  ru.SHLight(torch.tensor([[0.9, 0.1, 0.5, 0.1], [0.8, 0.1, 0.5, 0.0], [0.7, 0.0, 0.5, 0.1]], requires_grad=True))]
        return sc, lights

    sc, lights = scene_and_lights()
    img = ru.render_deferred(sc, lights, aa_samples=aa, seed=seed, device=device, backend=backend, ambient_occlusion=k, ao_radius=radius)
    assert tuple(img.shape) == (res, res, 3) and sc.camera.resolution == (res, res)
    img.sum().backward()
    for t in (sc.shapes[0].vertices.grad, sc.shapes[1].vertices.grad, lights[0].intensity.grad, lights[1].coeffs.grad):
        assert t is not None and bool(torch.isfinite(t).all())
    assert float(lights[0].intensity.grad.abs().sum()) > 0 and float(lights[1].coeffs.grad.abs().sum()) > 0
    sc1, lights1 = scene_and_lights()
    again = ru.render_deferred(sc1, lights1, aa_samples=aa, seed=seed, device=device, backend=backend, ambient_occlusion=k,
                               ao_radius=radius)
    again.sum().backward()
    assert torch.equal(again.detach(), img.detach())                      # the same seed: the same bits
    assert torch.equal(lights1[0].intensity.grad, lights[0].intensity.grad) and torch.equal(lights1[1].coeffs.grad, lights[1].coeffs.grad)
    sc2, lights2 = scene_and_lights()
    plain = ru.render_deferred(sc2, lights2, aa_samples=aa, seed=seed, device=device, backend=backend).detach()
    assert bool((img.detach() <= plain).all()) and int((img.detach() < plain).any(dim=-1).sum()) >= 4
    # the same from the pieces
    sc2.camera.resolution = (res * aa, res * aa)
    ch = [backend.channels.position, backend.channels.shading_normal, backend.channels.diffuse_reflectance]
    g = ru.render_g_buffer(sc2, ch, seed=seed, device=device, backend=backend).detach().unsqueeze(0)
    sc2.camera.resolution = (res, res)
    pieces, words = ru.deferred_shade(g, lights2, aa_samples=aa, backend=backend, ambient_occlusion=k, ao_radius=radius,
                                      ao_occluders=ru.occluder_scene(sc2, device=device, backend=backend), return_occlusion=True)
    assert torch.equal(pieces[0].detach(), img.detach())
    assert tuple(words.shape) == (1, res * aa, res * aa) and (as_words(words.cpu()) != 255).any()
    # `occluders` alone serves both; image, visibility, occlusion in that order
    occ = ru.occluder_scene(sc2, device=device, backend=backend)
    three = ru.deferred_shade(g, lights2, aa_samples=aa, backend=backend, occluders=occ, ambient_occlusion=k, ao_radius=radius,
                              return_visibility=True, return_occlusion=True)
    assert len(three) == 3 and torch.equal(three[2], words) and torch.equal(three[0].detach(), pieces.detach())
    assert bool((as_words(three[1].cpu()) == 15).all())                    # four rows, none of which casts a shadow ray


def test_end_to_end_hostsim(hostsim_backend):
    _run_end_to_end(hostsim_backend, CPU)


@pytest.mark.gpu
def test_end_to_end_gpu(gpu_backend):
    _run_end_to_end(gpu_backend, GPU)
