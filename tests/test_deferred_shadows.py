"""Shadows in deferred shading (rdr_deferred_shade with `occluders`; redner_amd.render_utils: deferred_shade(occluders=...),
render_deferred(shadows=True)): any-hit shadow rays from the G-buffer, one visibility bit per texel and light.

What the cases are held to:
  * the visibility words against a brute-force fp64 intersector written here (Moeller-Trumbore over all triangles, rays formed by
    the rule of include/redner_amd.h in numpy fp64).  A ray whose fp64 answer changes when every blocker is scaled about its
    centroid by 1 +- 1e-3 is a boundary ray: an fp32 and an fp64 evaluation may both be right about it, and it is left out
    (at most 10 % of the cast rays; every ray-casting light keeps at least 8 lit and 8 shadowed texels);
  * values and gradients against test_deferred's fp64 definition times that mask, visibility held constant, at parity_util.TOL
    (1e-4 relative L2, the bar of test_deferred.py) per image slice and per light row;
  * bit-for-bit equality with the unshadowed call wherever nothing is in the way, with the single-image call in a batch, with
    contiguous inputs under the calling contract, and across chunk sizes of the ray queue.
Every case runs on the CPU harness; the GPU legs run the same bodies on both builds of the library.  All frames are a few
thousand texels."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import parity_util
import scenes
from golden import make_deferred_golden as mk
from test_deferred import _definition_shade, _off_the_kinks, _worst_slice

CPU, GPU = torch.device('cpu'), torch.device('cuda:0')
HG, WG, AA = 20, 24, 2                       # the floor patch: 20 x 24 texels, 10 x 12 pixels
TMIN = float(np.float32(1e-3))
TMAX_SCALE = float(np.float32(1.0) - np.float32(1e-3))
BLOCKERS = np.array([[[-0.65, -0.55, 0.60], [0.45, -0.45, 0.50], [-0.15, 0.55, 0.70]],
                     [[0.15, 0.05, 0.40], [0.95, 0.25, 0.50], [0.50, 0.95, 0.45]]], np.float64)
FAR_AWAY = np.array([[[50.0, 50.0, 90.0], [51.0, 50.0, 90.0], [50.0, 51.0, 91.0]]], np.float64)      # behind every light
LIGHTS = [(0, {'intensity': [0.2, 0.25, 0.3]}),
          (1, {'position': [0.3, 0.2, 2.0], 'intensity': [30.0, 25.0, 20.0]}),
          (2, {'direction': [0.2, -0.1, -1.0], 'intensity': [1.5, 1.2, 1.0]}),
          (3, {'position': [-0.5, 0.4, 1.8], 'spot_direction': [0.2, -0.1, -1.0], 'spot_exponent': [2.0],
               'intensity': [4.0, 5.0, 6.0]})]
_cache = {}


def _ru():
    from redner_amd import render_utils
    return render_utils


def floor_g_buffer(hg, wg, alpha, seed=11):
    """A floor patch at z = 0, x and y in [-1, 1], normals +z, albedo in [0.1, 0.9]; the first two rows are BACKGROUND (all
    zeros), the last two face away (normal -z)."""
    gen = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(-1.0, 1.0, hg), torch.linspace(-1.0, 1.0, wg), indexing='ij')
    xx = xx + 0.01 * torch.rand(hg, wg, generator=gen)
    g = torch.zeros(1, hg, wg, 9 + alpha)
    g[0, ..., 0], g[0, ..., 1], g[0, ..., 5] = xx, yy, 1.0
    g[0, ..., 6:9] = 0.1 + 0.8 * torch.rand(hg, wg, 3, generator=gen)
    if alpha:
        g[0, ..., 9] = torch.rand(hg, wg, generator=gen)
    g[0, hg - 2:, :, 5] = -1.0
    g[0, :2] = 0.0
    return g.contiguous()


def triangle_scene(tris, device):
    """a Scene of loose triangles [T, 3, 3] (one shape, one black material); it is only ever traced, never rendered.  `tris`: numbers
    or, for a caller whose vertices exist on `device` only (tests/test_native_op_calls.py), a contiguous fp32 tensor there, which
    the scene's shape then points into: no value of it passes through the host."""
    cam = scenes.Camera(position=scenes._t([0.0, 0.0, 5.0], 'cpu'), look_at=scenes._t([0.0, 0.0, 0.0], 'cpu'),
                        up=scenes._t([0.0, 1.0, 0.0], 'cpu'), fov=scenes._t([45.0], 'cpu'), clip_near=1e-2, resolution=(4, 4))
    if isinstance(tris, torch.Tensor):
        assert tris.dtype == torch.float32 and tris.is_contiguous() and tris.device == torch.device(device)
        shape = scenes.Shape(tris.reshape(-1, 3), torch.arange(3 * len(tris), dtype=torch.int32, device=device).reshape(-1, 3), 0)
    else:
        tris = np.asarray(tris, np.float32)
        shape = scenes.Shape(scenes._t(tris.reshape(-1, 3), device),
                             scenes._t(np.arange(3 * len(tris)).reshape(-1, 3), device, torch.int32), 0)
    return scenes.Scene(cam, [shape], [scenes.Material(diffuse_reflectance=scenes._t([0.0, 0.0, 0.0], device))], [])


def occluder(backend, tris, device):
    return _ru().occluder_scene(triangle_scene(tris, device), device=device, backend=backend)


# ---- the fp64 brute-force side ----------------------------------------------------------------------------------------------------
def rays64(g, t, row):
    """The shadow-ray rule in numpy fp64 for light (t, row) over g [hg, wg, >= 6] -> cast [hg, wg] bool, dir [hg, wg, 3], tmax"""
    p, n = g[..., 0:3].astype(np.float64), g[..., 3:6].astype(np.float64)
    row = np.asarray(row, np.float64)
    if t == 0:
        return np.zeros(p.shape[:2], bool), np.zeros_like(p), np.zeros(p.shape[:2])
    with np.errstate(invalid='ignore', divide='ignore'):
        if t == 2:
            d = np.broadcast_to(-row[6:9] / np.linalg.norm(row[6:9]), p.shape).copy()
            tmax = np.full(p.shape[:2], np.inf)
            cast = np.ones(p.shape[:2], bool)
        else:
            v = row[3:6] - p
            r = np.sqrt((v * v).sum(-1))
            d = v / r[..., None]
            tmax = TMAX_SCALE * r
            cast = (r > 0) & np.isfinite(tmax)
            if t == 3:
                cast &= (d * (-row[6:9] / np.linalg.norm(row[6:9]))).sum(-1) > 0
        cast &= (d * n).sum(-1) > 0
        cast &= np.isfinite(p).all(-1) & np.isfinite(d).all(-1)
    return cast, np.where(cast[..., None], d, 0.0), np.where(cast, tmax, 0.0)


def any_hit64(o, d, tmax, tris):
    """Moeller-Trumbore in fp64: rays [R, 3] against all triangles [T, 3, 3] -> [R] bool, a hit in (TMIN, tmax)"""
    a, e1, e2 = tris[:, 0], tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    pv = np.cross(d[:, None, :], e2[None])
    det = (e1[None] * pv).sum(-1)
    with np.errstate(invalid='ignore', divide='ignore'):
        inv = 1.0 / det
        s = o[:, None, :] - a[None]
        u = (s * pv).sum(-1) * inv
        q = np.cross(s, e1[None])
        v = (d[:, None, :] * q).sum(-1) * inv
        t = (e2[None] * q).sum(-1) * inv
        hit = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > TMIN) & (t < tmax[:, None])
    return hit.any(-1)


def brute_mask(g, types, params, tris):
    """g [hg, wg, C] numpy -> (words [hg, wg] uint32, cast [L, hg, wg], robust [L, hg, wg], lit [L, hg, wg])"""
    tris = np.asarray(tris, np.float64)
    centre = tris.mean(axis=1, keepdims=True)
    hg, wg = g.shape[:2]
    words = np.zeros((hg, wg), np.uint32)
    casts, robusts, lits = [], [], []
    for b, (t, row) in enumerate(zip(types, params)):
        cast, d, tmax = rays64(g, int(t), row)
        o = g[..., 0:3].astype(np.float64).reshape(-1, 3)
        answers = [any_hit64(o, d.reshape(-1, 3), tmax.reshape(-1), centre + k * (tris - centre)).reshape(hg, wg)
                   for k in (1.0, 1.0 + 1e-3, 1.0 - 1e-3)]
        lit = ~(cast & answers[0])
        casts.append(cast)
        robusts.append((answers[0] == answers[1]) & (answers[0] == answers[2]))
        lits.append(lit)
        words |= lit.astype(np.uint32) << np.uint32(b)
    return words, np.stack(casts), np.stack(robusts), np.stack(lits)


def floor_case(alpha):
    if ('floor', alpha) not in _cache:
        types, params = mk.light_table(LIGHTS)
        types = [int(t) for t in types]
        g, moved = _off_the_kinks(floor_g_buffer(HG, WG, alpha), types, params)
        words, cast, robust, lit = brute_mask(g[0].numpy(), types, params, BLOCKERS)
        _cache['floor', alpha] = dict(g=g, types=types, params=params, words=words, cast=cast, robust=robust, lit=lit)
    return _cache['floor', alpha]


def shade(backend, device, g, types, params, ranges, aa, alpha, occluders, up=None):
    """forward (+ backward when `up` is given) through DeferredShade -> image, visibility | None, d_g, d_params"""
    ru = _ru()
    gl = g.to(device).clone().requires_grad_(True)
    pl = torch.from_numpy(np.asarray(params, np.float32)).to(device).requires_grad_(True)
    scn = None if occluders is None else tuple(o.scene if o is not None else None for o in occluders)
    out = ru.DeferredShade.apply(gl, pl, tuple(types), tuple(ranges), aa, bool(alpha), backend, scn)
    img, vis = out if occluders is not None else (out, None)
    if up is None:
        return img.detach().cpu(), None if vis is None else vis.cpu(), None, None
    img.backward(up.to(device))
    return img.detach().cpu(), None if vis is None else vis.cpu(), gl.grad.cpu(), pl.grad.cpu()


def as_words(vis):
    return vis.numpy().view(np.uint32)


# ---- 1. nothing in the way is bit for bit nothing ------------------------------------------------------------------------------------
def _run_nothing_in_the_way(backend, device):
    far = occluder(backend, FAR_AWAY, device)
    for alpha in (0, 1):
        case = floor_case(alpha)
        n = len(case['types'])
        up = mk.upstream((1, HG // AA, WG // AA, 3 + alpha))
        plain = shade(backend, device, case['g'], case['types'], case['params'], ((0, n),), AA, alpha, None, up)
        shadowed = shade(backend, device, case['g'], case['types'], case['params'], ((0, n),), AA, alpha, (far,), up)
        for a, b, what in zip(plain, shadowed, ('image', None, 'd_g_buffer', 'd_light_params')):
            if what:
                assert torch.equal(a, b), (what, alpha)
        assert (as_words(shadowed[1]) == (1 << n) - 1).all()


def test_nothing_in_the_way_hostsim(hostsim_backend):
    _run_nothing_in_the_way(hostsim_backend, CPU)


@pytest.mark.gpu
def test_nothing_in_the_way_gpu(gpu_backend):
    _run_nothing_in_the_way(gpu_backend, GPU)


# ---- 2. the mask against the fp64 brute-force intersector ---------------------------------------------------------------------------
def _run_mask(backend, device):
    case = floor_case(0)
    n = len(case['types'])
    _, vis, _, _ = shade(backend, device, case['g'], case['types'], case['params'], ((0, n),), AA, 0,
                         (occluder(backend, BLOCKERS, device),))
    words = as_words(vis)[0]
    cast, robust = case['cast'], case['robust']
    left_out = int((cast & ~robust).sum())
    print('cast rays %d, boundary rays left out %d' % (int(cast.sum()), left_out))
    assert left_out <= 0.10 * int(cast.sum())
    for b, t in enumerate(case['types']):
        got = ((words >> np.uint32(b)) & 1).astype(bool)
        keep = robust[b]
        assert (got[keep] == case['lit'][b][keep]).all(), 'light %d: %d bits differ' % (b, int((got != case['lit'][b])[keep].sum()))
        if t == 0:
            assert not cast[b].any() and got.all()
            continue
        assert int((cast[b] & keep & case['lit'][b]).sum()) >= 8 and int((cast[b] & keep & ~case['lit'][b]).sum()) >= 8, b
    assert (words[:2] == (1 << n) - 1).all() and (words[HG - 2:] == (1 << n) - 1).all()       # background, facing away
    assert (words >> np.uint32(n) == 0).all()


def test_mask_against_brute_force_hostsim(hostsim_backend):
    _run_mask(hostsim_backend, CPU)


@pytest.mark.gpu
def test_mask_against_brute_force_gpu(gpu_backend):
    _run_mask(gpu_backend, GPU)


# ---- 3. values and gradients against the fp64 definition, visibility held constant ---------------------------------------------------
def definition_shadowed(g, types, params, lit, aa, alpha):
    """sum over the lights of test_deferred's one-light definition times the light's mask [hg, wg], resolved over aa"""
    n, hg, wg, _ = g.shape
    rgb = torch.zeros(n, hg, wg, 3, dtype=torch.float64)
    for l, t in enumerate(types):
        one = _definition_shade(g[..., :9], [t], params[l:l + 1], ((0, 1),) * n, 1, 0)
        rgb = rgb + one * torch.from_numpy(lit[l].astype(np.float64))[None, ..., None]
    img = torch.cat([rgb, g[..., 9:10]], dim=-1) if alpha else rgb
    return img.reshape(n, hg // aa, aa, wg // aa, aa, img.shape[-1]).mean(dim=(2, 4))


def _run_values_and_gradients(backend, device):
    alpha = 1
    case = floor_case(alpha)
    n = len(case['types'])
    up = mk.upstream((1, HG // AA, WG // AA, 3 + alpha))
    img, vis, d_g, d_params = shade(backend, device, case['g'], case['types'], case['params'], ((0, n),), AA, alpha,
                                    (occluder(backend, BLOCKERS, device),), up)
    words = as_words(vis)[0]
    # a boundary ray (see the module docstring) has no single right answer: there the definition takes the bit the kernels took
    lit = np.stack([np.where(case['robust'][b], case['lit'][b], ((words >> np.uint32(b)) & 1).astype(bool)) for b in range(n)])
    g64 = case['g'].double().requires_grad_(True)
    p64 = torch.from_numpy(case['params']).double().requires_grad_(True)
    want = definition_shadowed(g64, case['types'], p64, lit, AA, alpha)
    want.backward(up.double())
    errors = {'image': _worst_slice(img, want.detach(), 'image'), 'd_g_buffer': _worst_slice(d_g, g64.grad, 'd_g_buffer'),
              'd_light_params': _worst_slice(d_params, p64.grad, 'd_light_params')}
    print({k: '%.2e' % v for k, v in errors.items()})
    for k, v in errors.items():
        assert v < parity_util.TOL, (k, v)
    # a light that reaches no texel it faces: its ten parameter gradients are exactly 0
    roof = occluder(backend, [[[-30.0, -30.0, 1.0], [30.0, -30.0, 1.0], [0.0, 40.0, 1.0]]], device)
    _, vis1, _, d_one = shade(backend, device, case['g'], case['types'][1:2], case['params'][1:2], ((0, 1),), AA, alpha, (roof,), up)
    assert (as_words(vis1)[0][2:HG - 2] == 0).all()
    assert (d_one == 0).all()


def test_values_and_gradients_hostsim(hostsim_backend):
    _run_values_and_gradients(hostsim_backend, CPU)


@pytest.mark.gpu
def test_values_and_gradients_gpu(gpu_backend):
    _run_values_and_gradients(gpu_backend, GPU)


# ---- 4. queue boundaries ------------------------------------------------------------------------------------------------------------
def any_rays(backend):
    from redner_amd import _capi
    st = _capi.TraceStats()
    _capi.lib().rdr_trace_stats_get(C.byref(st))
    return int(st.any_rays)


def _run_queue_boundaries(backend, device, harness):
    types, params = mk.light_table(LIGHTS[1:])                           # three ray-casting lights
    types = [int(t) for t in types]
    g = floor_g_buffer(40, 40, 0, seed=12)                              # 1600 texels x 3 lights = 4800 rays at most
    blockers = occluder(backend, BLOCKERS, device)
    up = mk.upstream((1, 40, 40, 3))
    whole = shade(backend, device, g, types, params, ((0, 3),), 1, 0, (blockers,), up)
    words, cast, robust, lit = brute_mask(g[0].numpy(), types, params, BLOCKERS)
    got = as_words(whole[1])[0]
    for b in range(3):
        keep = robust[b]
        assert ((((got >> np.uint32(b)) & 1).astype(bool)) == lit[b])[keep].all(), b
        assert int((cast[b] & keep & ~lit[b]).sum()) >= 8
    # the same rays in chunks of 640 texels: every pass of 1600 texels takes three trace launches, the last one ragged
    os.environ['RDR_DEFERRED_SHADOW_CHUNK'] = '640'
    try:
        chunked = shade(backend, device, g, types, params, ((0, 3),), 1, 0, (blockers,), up)
    finally:
        del os.environ['RDR_DEFERRED_SHADOW_CHUNK']
    for a, b in zip(whole, chunked):
        assert torch.equal(a, b)
    # calls that cast no ray at all: only ambient lights; only background texels
    amb_types, amb_params = mk.light_table([LIGHTS[0], (0, {'intensity': [0.05, 0.02, 0.08]})])
    for gz, tz, pz in ((g, [int(t) for t in amb_types], amb_params), (torch.zeros_like(g), types, params)):
        before = any_rays(backend)
        shadowed = shade(backend, device, gz, tz, pz, ((0, len(tz)),), 1, 0, (blockers,), up)
        if harness:                                                      # (the GPU build tallies the queues' upper bounds)
            assert any_rays(backend) == before
        plain = shade(backend, device, gz, tz, pz, ((0, len(tz)),), 1, 0, None, up)
        for a, b in zip((shadowed[0], shadowed[2], shadowed[3]), (plain[0], plain[2], plain[3])):
            assert torch.equal(a, b)
        assert (as_words(shadowed[1]) == (1 << len(tz)) - 1).all()


def test_queue_boundaries_hostsim(hostsim_backend):
    _run_queue_boundaries(hostsim_backend, CPU, True)


@pytest.mark.gpu
def test_queue_boundaries_gpu(gpu_backend):
    _run_queue_boundaries(gpu_backend, GPU, False)


# ---- 5. batch -----------------------------------------------------------------------------------------------------------------------
def _run_batch(backend, device):
    alpha = 1
    types, params = mk.light_table(LIGHTS)
    types = [int(t) for t in types]
    g = torch.cat([floor_g_buffer(HG, WG, alpha, seed=21), floor_g_buffer(HG, WG, alpha, seed=22)])
    ranges = ((0, 4), (1, 3))                                           # light lists of different lengths, sharing two lights
    occ = (occluder(backend, BLOCKERS, device), None)
    up = mk.upstream((2, HG // AA, WG // AA, 3 + alpha))
    img, vis, d_g, d_p = shade(backend, device, g, types, params, ranges, AA, alpha, occ, up)
    assert (as_words(vis)[0] != 15).any() and (as_words(vis)[1] == 3).all()
    total = torch.zeros_like(d_p)
    for k in range(2):
        one = shade(backend, device, g[k:k + 1], types, params, ranges[k:k + 1], AA, alpha, occ[k:k + 1], up[k:k + 1])
        assert torch.equal(one[0][0], img[k]) and torch.equal(one[1][0], vis[k]) and torch.equal(one[2][0], d_g[k]), k
        total += one[3]
    for l in range(4):                                                   # (one fp64 sum over both images / two rounded results)
        assert parity_util.rel_l2(total[l], d_p[l]) < 1e-6 or bool((total[l] == d_p[l]).all()), l
    assert torch.equal(total[0], d_p[0]) and torch.equal(total[3], d_p[3])          # lights of one image only


def test_batch_hostsim(hostsim_backend):
    _run_batch(hostsim_backend, CPU)


@pytest.mark.gpu
def test_batch_gpu(gpu_backend):
    _run_batch(gpu_backend, GPU)


# ---- 6. no host reads, no new allocations -------------------------------------------------------------------------------------------
def _run_no_host_reads_no_new_allocations(backend, device):
    from redner_amd import _capi
    case = floor_case(1)
    n = len(case['types'])
    blockers = occluder(backend, BLOCKERS, device)
    up = mk.upstream((1, HG // AA, WG // AA, 4))

    def counters():
        c = _capi.DebugCounters()
        _capi.lib().rdr_debug_counters_get(C.byref(c))
        return int(c.device_mallocs), int(c.host_count_reads)

    first = shade(backend, device, case['g'], case['types'], case['params'], ((0, n),), AA, 1, (blockers,), up)
    before = counters()
    second = shade(backend, device, case['g'], case['types'], case['params'], ((0, n),), AA, 1, (blockers,), up)
    assert counters() == before
    for a, b in zip(first, second):
        assert torch.equal(a, b)


def test_no_host_reads_no_new_allocations_hostsim(hostsim_backend):
    _run_no_host_reads_no_new_allocations(hostsim_backend, CPU)            # (the harness has no pool: the call repeats itself)


@pytest.mark.gpu
def test_no_host_reads_no_new_allocations_gpu(gpu_backend):
    _run_no_host_reads_no_new_allocations(gpu_backend, GPU)


# ---- 7. guards (harness only: a ray that is not finite never reaches a traversal kernel) -----------------------------------------
def test_guards_hostsim(hostsim_backend):
    types, params = mk.light_table([LIGHTS[1]])
    g = floor_g_buffer(8, 8, 0, seed=31)
    blockers = occluder(hostsim_backend, BLOCKERS, CPU)
    _, vis, _, _ = shade(hostsim_backend, CPU, g, [1], params, ((0, 1),), 1, 0, (blockers,))
    base_cast = int(brute_mask(g[0].numpy(), [1], params, BLOCKERS)[1].sum())
    assert base_cast == 4 * 8                                            # rows 2 .. 5 face the light
    g[0, 3, 3, 0] = float('inf')                                         # a position that is not finite
    g[0, 4, 4, 0:3] = torch.from_numpy(params[0, 3:6])                   # the light sits exactly on this texel: r == 0
    before = any_rays(hostsim_backend)
    _, vis, _, _ = shade(hostsim_backend, CPU, g, [1], params, ((0, 1),), 1, 0, (blockers,))
    assert any_rays(hostsim_backend) - before == base_cast - 2
    words = as_words(vis)[0]
    assert words[3, 3] == 1 and words[4, 4] == 1


# ---- 8. errors ----------------------------------------------------------------------------------------------------------------------
def test_errors_hostsim(hostsim_backend):
    rd, ru = hostsim_backend, _ru()
    blockers = occluder(rd, BLOCKERS, CPU)
    g = floor_g_buffer(4, 4, 0)
    ptr = lambda t: rd.float_ptr(t.data_ptr())
    img, vis = torch.zeros(1, 4, 4, 3), torch.zeros(17, dtype=torch.int32)
    many = torch.zeros(33, 10)
    with pytest.raises(RuntimeError, match='image 0 has 33 lights'):
        rd.deferred_shade(ptr(g), ptr(many), ptr(img), 1, 4, 4, 1, False, [0] * 33, [(0, 33)], False, 0,
                          occluders=[blockers.scene], visibility=rd.int_ptr(vis.data_ptr()))
    # ... which an image that is not shadowed may have
    rd.deferred_shade(ptr(g), ptr(many), ptr(img), 1, 4, 4, 1, False, [0] * 33, [(0, 33)], False, 0,
                      occluders=[None], visibility=rd.int_ptr(vis.data_ptr()))
    assert (vis[:16].numpy().view(np.uint32) == 0xffffffff).all()
    params = torch.zeros(1, 10)
    with pytest.raises(RuntimeError, match='2 occluder scenes for 1 images'):
        rd.deferred_shade(ptr(g), ptr(params), ptr(img), 1, 4, 4, 1, False, [0], [(0, 1)], False, 0,
                          occluders=[blockers.scene, None], visibility=rd.int_ptr(vis.data_ptr()))
    with pytest.raises(RuntimeError, match='occluder scenes for 1 images'):
        ru.deferred_shade(g, [ru.AmbientLight(torch.ones(3))], occluders=[blockers, blockers], backend=rd)
    with pytest.raises(RuntimeError, match='occluders need a visibility buffer'):
        rd.deferred_shade(ptr(g), ptr(params), ptr(img), 1, 4, 4, 1, False, [0], [(0, 1)], False, 0, occluders=[blockers.scene])
    with pytest.raises(RuntimeError, match='must be 4-byte aligned'):
        rd.deferred_shade(ptr(g), ptr(params), ptr(img), 1, 4, 4, 1, False, [0], [(0, 1)], False, 0,
                          occluders=[blockers.scene], visibility=rd.int_ptr(vis.data_ptr() + 2))
    with pytest.raises(RuntimeError, match='must be 4-byte aligned'):
        rd.deferred_shade_backward(ptr(g), ptr(params), ptr(img), ptr(torch.zeros_like(g)), ptr(torch.zeros_like(params)),
                                   1, 4, 4, 1, False, [0], [(0, 1)], False, 0, visibility=rd.int_ptr(vis.data_ptr() + 2))
    # what was refused before is refused as before
    with pytest.raises(RuntimeError, match='unknown light type'):
        rd.deferred_shade(ptr(g), ptr(params), ptr(img), 1, 4, 4, 1, False, [7], [(0, 1)], False, 0,
                          occluders=[blockers.scene], visibility=rd.int_ptr(vis.data_ptr()))
    with pytest.raises(RuntimeError, match='light_params must be'):
        ru.DeferredShade.apply(g, params, (0, 1), ((0, 2),), 1, False, rd, (blockers.scene,))


# ---- 9. calling contract ------------------------------------------------------------------------------------------------------------
def _run_calling_contract(backend, device):
    ru = _ru()
    case = floor_case(1)
    n = len(case['types'])
    blockers = occluder(backend, BLOCKERS, device)
    params = torch.from_numpy(case['params']).to(device)
    args = (tuple(case['types']), ((0, n),), AA, True, backend, (blockers.scene,))
    up = mk.upstream((1, HG // AA, WG // AA, 4)).to(device)
    fresh = case['g'].to(device).clone().requires_grad_(True)
    img, vis = ru.DeferredShade.apply(fresh, params, *args)
    img.backward(up)
    wide = torch.zeros(1, HG, WG, 13, device=device)
    wide[..., 2:12] = case['g'].to(device)
    wide.requires_grad_(True)
    img_v, vis_v = ru.DeferredShade.apply(wide[..., 2:12], params, *args)                       # a view that is not contiguous
    img_v.backward(up)
    assert torch.equal(img_v, img) and torch.equal(vis_v, vis) and torch.equal(wide.grad[..., 2:12], fresh.grad)
    ones = case['g'].to(device).clone().requires_grad_(True)
    ru.DeferredShade.apply(ones, params, *args)[0].sum().backward()                              # a stride-0 upstream gradient
    ref = case['g'].to(device).clone().requires_grad_(True)
    ru.DeferredShade.apply(ref, params, *args)[0].backward(torch.ones_like(img))
    assert torch.equal(ones.grad, ref.grad)
    leaf = case['g'].to(device).clone().requires_grad_(True)
    edited = leaf * 1.0                                                                            # contiguous: saved as it is
    out = ru.DeferredShade.apply(edited, params, *args)[0]
    edited.mul_(2.0)
    with pytest.raises(RuntimeError, match='modified by an inplace operation'):
        out.sum().backward()


def test_calling_contract_hostsim(hostsim_backend):
    _run_calling_contract(hostsim_backend, CPU)


@pytest.mark.gpu
def test_calling_contract_gpu(gpu_backend):
    _run_calling_contract(gpu_backend, GPU)


# ---- 10. end to end -----------------------------------------------------------------------------------------------------------------
def _run_end_to_end(backend, device):
    ru = _ru()
    res, aa, seed = 24, 2, 9

    def scene_and_light():
        sc = scenes.glossy_floor_blocker(device, resolution=(res, res))
        sc.materials[0] = scenes.Material(diffuse_reflectance=scenes._t([0.6, 0.5, 0.4], device))     # a floor that is lit
        light = ru.PointLight(torch.tensor([0.5, 10.0, 1.5], requires_grad=True), torch.tensor([60.0, 55.0, 50.0], requires_grad=True))
        return sc, light

    sc, light = scene_and_light()
    img = ru.render_deferred(sc, [light], aa_samples=aa, seed=seed, device=device, backend=backend, shadows=True)
    assert tuple(img.shape) == (res, res, 3) and sc.camera.resolution == (res, res) and sc.camera.viewport is None
    img.sum().backward()
    for t in (sc.shapes[0].vertices.grad, sc.shapes[1].vertices.grad, light.position.grad, light.intensity.grad):
        assert t is not None and bool(torch.isfinite(t).all())
    assert float(light.intensity.grad.abs().sum()) > 0
    # the same from the pieces
    sc2, light2 = scene_and_light()
    sc2.camera.resolution = (res * aa, res * aa)
    ch = [backend.channels.position, backend.channels.shading_normal, backend.channels.diffuse_reflectance]
    g = ru.render_g_buffer(sc2, ch, seed=seed, device=device, backend=backend).detach().unsqueeze(0)
    sc2.camera.resolution = (res, res)
    pieces, vis = ru.deferred_shade(g, [light2], aa_samples=aa, backend=backend,
                                    occluders=ru.occluder_scene(sc2, device=device, backend=backend), return_visibility=True)
    assert torch.equal(pieces[0], img.detach())
    plain = ru.render_deferred(sc2, [light2], aa_samples=aa, seed=seed, device=device, backend=backend)
    blocked = (vis[0] == 0).reshape(res, aa, res, aa).any(dim=3).any(dim=1)
    assert int(blocked.sum()) >= 8 and int((~blocked).sum()) >= 8
    differs = (plain.detach() != img.detach()).any(dim=-1)
    assert bool((differs & ~blocked).sum() == 0) and int(differs.sum()) >= 8


def test_end_to_end_hostsim(hostsim_backend):
    _run_end_to_end(hostsim_backend, CPU)


@pytest.mark.gpu
def test_end_to_end_gpu(gpu_backend):
    _run_end_to_end(gpu_backend, GPU)
