"""Every native tensor op under the ways a training loop calls it: the layer between torch and the kernels (redner_amd/_op.py,
the autograd Functions in front of the kernels, the one `_call(..., on=...)` of redner_amd/redner.py).

The per-op test files hold the kernels to their fp64 definitions at the shapes where the launch plans switch.  This module is a
matrix of every op against every calling condition; TABLE below is that matrix, written out.

What a result is compared with
  * the PLAIN call -- contiguous, freshly allocated inputs, the default stream, dense fp32 upstream gradients (fixed seeded
    normal tensors) -- is held to the fp64 definition of the op that its own test file holds (imported from there, not restated),
    under the bar that file applies to that comparison: the per-element bar derived from the roundings where the file has one
    (the mip pyramid, SH_reconstruct, the pyramid loss), otherwise parity_util.TOL = 1e-4 relative L2 of every whole tensor (of
    every image slice and light row for deferred_shade); the tables of an environment map and bound_vertices exactly.
    test_plain_is_the_definition_*.
  * every condition is held to the plain call with torch.equal.  That is not a measured tolerance: every op is documented as
    bitwise reproducible, `.contiguous()` and the coercion of an fp32 tensor copy values exactly, so a call that differs only
    in where the same numbers live has the same bits.

Conditions (one small case per entry point: every kernel of the op runs and one tile or chunk boundary is crossed)
  A  where the inputs live: each tensor input in turn, then all together, as a view that is not contiguous (a transposed buffer;
     every second element for a vector) and as a contiguous view one float into its buffer (4-byte aligned only).  Nothing
     outside a view is written.  smooth writes through a view that is not contiguous.
  B  the upstream gradient: autograd's stride-0 expanded ones against dense ones; upstream gradients that are not contiguous
     (the output times a transposed weight, and the transposed weight handed to backward itself); outputs without an upstream
     gradient against explicit zeros.
  C  which inputs want a gradient: subsets of the differentiable inputs; torch.no_grad() and no input that wants one (the same
     bits, no node, and for SH_reconstruct no clamp mask).
  D  backward(retain_graph=True), then backward(): the first gradient is the plain one, .grad ends at exactly twice it.
  E  edits in place between forward and backward: of a contiguous input the adjoint reads -> torch's saved-tensor RuntimeError;
     of the same input given as a view that is not contiguous (the op read a private copy), of an input the adjoint does not
     read, and of a differentiable OUTPUT -> the plain gradient; of a word output that the op also saved for its adjoint (the
     visibility and occlusion words of deferred_shade: Case.saved_extras) -> the saved-tensor RuntimeError.
  F  (GPU) the small inputs of a case (Case.small: the angles, translation and centre of pose_vertices, the light table of
     deferred_shade, the eye and the light table of deferred_specular) on the CPU: the plain bits, their gradients back on the
     CPU, every other gradient on the GPU.
  G  (GPU) a side stream: see _side_stream.
  H  (GPU) two host threads, each under its own stream: see test_two_host_threads_gpu.
  I  torch.autograd.grad(..., create_graph=True): the native adjoints cannot be differentiated again and say so
     (redner_amd/_op.py: first_order_only) instead of handing back a first gradient that silently does not require one; a plain
     run afterwards gives the plain bits.
The deferred_shade cases with occluders build their occluder scene inside the call, from the case's `triangles` input, and run
under a RDR_DEFERRED_SHADOW_CHUNK that splits their 480 texels into several chunks of the ray queue; their word outputs are
extras.  The harness legs run everything but F, G and H; the GPU legs run on both builds of the library.
test_render_deferred_side_stream_gpu is G for the composite render_deferred, outside the matrix."""
import contextlib
import itertools
import os
import threading

import numpy as np
import pytest
import torch

import parity_util
import test_deferred as t_deferred
import test_deferred_ao as t_ao
import test_deferred_sh as t_dsh
import test_deferred_shadows as t_shadows
import test_deferred_specular as t_spec
import test_mesh_smooth as t_smooth
import test_pose as t_pose
import test_pyramid_loss as t_loss
import test_sh_envmap as t_sh
import test_texture as t_texture
import test_vertex_normal as t_normal
from golden import make_deferred_golden as mk
from golden import make_mesh_golden as mg
from golden import make_pose_golden as mpose
from golden import make_pyramid_loss_golden as mloss

CPU, GPU = torch.device('cpu'), torch.device('cuda:0')
INPLACE = 'modified by an inplace operation'

# The matrix: public native op -> the conditions that apply to it.  test_table_is_complete holds it to the list of ops and to
# the list of conditions; CASES (below) gives every op its case(s).  envmap_sampling_tables, smooth and bound_vertices have no
# gradient: the view and stream conditions only.
TABLE = {
    'generate_mipmap': 'ABCDEGI',
    'SH_reconstruct': 'ABCDEGI',
    'envmap_sampling_tables': 'AG',
    'deferred_shade': 'ABCDEFGHI',
    'deferred_specular': 'ABCDEFGHI',
    'compute_vertex_normal': 'ABCDEGI',
    'mesh_laplacian': 'ABCDEGI',
    'smooth': 'AG',
    'bound_vertices': 'AG',
    'gaussian_pyramid_loss': 'ABCDEGHI',
    'gen_rotate_matrix': 'ABCDEGI',
    'pose_vertices': 'ABCDEFGHI',
}
NATIVE_OPS = ('generate_mipmap', 'SH_reconstruct', 'envmap_sampling_tables', 'deferred_shade', 'deferred_specular',
              'compute_vertex_normal', 'mesh_laplacian', 'smooth', 'bound_vertices', 'gaussian_pyramid_loss', 'gen_rotate_matrix',
              'pose_vertices')
HARNESS_CONDITIONS, GPU_CONDITIONS = 'ABCDEI', 'ABCDEFGI'          # (H is one test of its own)


def _modules():
    from redner_amd import loss, render_utils, shape, texture, transform, utils
    return loss, render_utils, shape, texture, transform, utils


# ---- placing a tensor -----------------------------------------------------------------------------------------------------------
def _fresh(x, device):
    return x.clone().to(device)


def _strided(x, device):
    """x's values in a view that is not contiguous: a transposed buffer; where that is contiguous (a vector, sides of
    1), every second element along the last side longer than 1.  The rest of the buffer holds 7."""
    view = torch.full(tuple(reversed(x.shape)), 7, dtype=x.dtype, device=device).permute(*reversed(range(x.dim())))
    if view.is_contiguous():
        d = max(k for k, n in enumerate(x.shape) if n > 1)
        doubled = tuple(2 * n if k == d else n for k, n in enumerate(x.shape))
        view = torch.full(doubled, 7, dtype=x.dtype, device=device)[(slice(None),) * d + (slice(None, None, 2),)]
    view.copy_(x)
    assert not view.is_contiguous() and tuple(view.shape) == tuple(x.shape)
    return view


def _offset(x, device):
    """x's values in a contiguous view one element (4 bytes) into its buffer"""
    assert x.element_size() == 4
    view = torch.full((x.numel() + 1,), 7, dtype=x.dtype, device=device)[1:].view(x.shape)
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


def _on_cpu(x, device):
    return x.clone()


# ---- a case ---------------------------------------------------------------------------------------------------------------------
class Case:
    """One call of one op.  inputs: name -> CPU tensor (never written; every run gets its own copy).  diff: the inputs that may
    want a gradient.  call(backend, tensors) -> (differentiable outputs, other results).  cotangents: one fixed CPU tensor per
    differentiable output.  reads / unread: the inputs the adjoint reads / does not read.  subsets: condition C.  unused:
    condition B, the only outputs used.  leaf: inputs that require a gradient although nothing is differentiated (smooth).
    saved_extras: condition E, the indices of the other results that the op saved for its adjoint.  small: condition F, the
    inputs that may live on the host.  definition(case, plain, backend, device): holds the plain call to the fp64 definition."""

    def __init__(self, op, name, inputs, call, definition, diff=(), cotangents=(), reads=(), unread=(), subsets=(), unused=None,
                 leaf=(), saved_extras=(), small=()):
        self.op, self.name, self.inputs, self.call, self.definition = op, name, inputs, call, definition
        self.diff, self.cotangents, self.reads, self.unread = tuple(diff), list(cotangents), tuple(reads), tuple(unread)
        self.subsets, self.unused, self.leaf = tuple(subsets), unused, tuple(leaf)
        self.saved_extras, self.small = tuple(saved_extras), tuple(small)

    def __repr__(self):
        return self.name


def _make(case, device, place=None, wants=None):
    place = place or {}
    wants = case.diff if wants is None else wants
    tensors = {}
    for name, x in case.inputs.items():
        v = place.get(name, _fresh)(x, device)
        if name in wants or name in case.leaf:
            v.requires_grad_(True)
        tensors[name] = v
    return tensors


def _guards(tensors):
    return [(v, v._base.clone()) for v in tensors.values() if v._base is not None]


def _check_guards(guards):
    """Nothing outside a view was written."""
    for v, before in guards:
        after = v._base.clone()
        for b in (before, after):
            b.as_strided(v.shape, v.stride(), v.storage_offset()).zero_()
        assert torch.equal(before, after), 'written outside the view'


def _keep(t):
    return None if t is None else t.detach().cpu().clone()


def _snapshot(case, tensors, outs, extras):
    return {'outs': [_keep(o) for o in outs], 'extras': [_keep(e) for e in extras],
            'grads': {name: _keep(tensors[name].grad) for name in case.diff}}


def _cotangents(case, device):
    return [c.clone().to(device) for c in case.cotangents]


def _run(case, backend, device, place=None, wants=None, cotangents=None, between=None):
    tensors = _make(case, device, place, wants)
    guards = _guards(tensors)
    outs, extras = case.call(backend, tensors)
    if between is not None:
        with torch.no_grad():
            between(tensors, outs)
    if any(o.requires_grad for o in outs):
        torch.autograd.backward(outs, _cotangents(case, device) if cotangents is None else cotangents)
    _check_guards(guards)
    return _snapshot(case, tensors, outs, extras)


def _same(got, want, what, keys=('outs', 'extras', 'grads')):
    for key in keys:
        a, b = got[key], want[key]
        pairs = [(name, a[name], b[name]) for name in b] if isinstance(b, dict) else list(zip(itertools.count(), a, b))
        assert len(a) == len(b), (what, key)
        for name, x, y in pairs:
            assert (x is None) == (y is None), (what, key, name, 'a gradient is missing' if x is None else 'a gradient too many')
            if x is not None:
                assert x.dtype == y.dtype and tuple(x.shape) == tuple(y.shape), (what, key, name, x.dtype, tuple(x.shape))
                assert torch.equal(x, y), (what, key, name, 'differs from the plain call in %d of %d elements, at most by %.3e'
                                           % (int((x != y).sum()), x.numel(), float((x.double() - y.double()).abs().max())))


_PLAIN = {}


def _plain(case, backend, device):
    """The plain call, once per loaded library and shared by every condition."""
    from redner_amd import _capi
    key = (_capi.library_path(), case.name)
    if key not in _PLAIN:
        _PLAIN[key] = _run(case, backend, device)
        for name in case.diff:
            assert _PLAIN[key]['grads'][name] is not None and bool(_PLAIN[key]['grads'][name].any()), (case, name)
    return _PLAIN[key]


def _rel_hold(out, want, tag):
    """parity_util.TOL relative L2 of every whole tensor"""
    rep = parity_util.compare(out, want)
    print(tag, {k: '%.2e' % e['rel_l2'] for k, e in rep.items()})
    parity_util.assert_parity(rep, tag)


def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def _mip_case(size):
    """texels and upstream gradients are those of test_texture's reference for this size (seeded there)"""
    texels, _, ups, _, _ = t_texture._plan_reference(size, None)

    def call(rd, t):
        return list(_modules()[3].generate_mipmap(t['texels'], rd)), []

    def definition(case, plain, backend, device):
        _, want_levels, _, want_grad, m0 = t_texture._plan_reference(size, None)
        assert backend.mip_tiled_stages(*size) == t_texture._stages_by_rule(size) == (1 if size[0] > 64 else 0)
        bound = 84.0 * 2.0 ** -24 * float(texels.abs().max())                  # test_texture._run_plan_case, both bars
        assert [tuple(l.shape) for l in plain['outs']] == [tuple(l.shape) for l in want_levels]
        for l, (got, ref) in enumerate(zip(plain['outs'], want_levels)):
            assert float(np.abs(got.numpy().astype(np.float64) - ref).max()) <= bound, (size, 'level', l)
        err = np.abs(plain['grads']['texels'].numpy().astype(np.float64) - want_grad)
        units = float(np.max(np.where(m0 > 0.0, err / np.where(m0 > 0.0, m0, 1.0), np.where(err > 0.0, np.inf, 0.0)))) * 2.0 ** 24
        print(case, 'd_texels max error / M_0 = %.2f x 2^-24' % units)
        assert units <= t_texture.ADJOINT_ROUNDINGS_PER_LEVEL * (len(want_levels) - 1), (size, units)

    return Case('generate_mipmap', 'mipmap_%dx%dx%d' % size, {'texels': texels.clone()}, call, definition, diff=('texels',),
                cotangents=ups, unread=('texels',), unused=(2,))


SH_RES = (9, 33)


def _sh_case():
    coeffs, weights = _randn(2101, 3, 16), _randn(2102, SH_RES[0], SH_RES[1], 3)

    def call(rd, t):
        return [_modules()[5].SH_reconstruct(t['coeffs'], SH_RES, backend=rd)], []

    def definition(case, plain, backend, device):
        reference = t_sh._reference64_of(SH_RES, coeffs, weights)              # the per-element bars of test_sh_envmap
        want_image, _, _, _, scale = reference
        # (as the generator of the SH fixtures asserted: no pixel so near zero that a last bit could flip its clamp)
        lit = want_image > 0
        assert float((want_image / scale)[lit].min()) > 1e-4, 'choose another seed, not another bar'
        assert 0.1 < float(lit.mean()) < 0.9, 'the clamp is exercised'
        t_sh._hold_definition(plain['outs'][0].numpy(), plain['grads']['coeffs'].numpy(), reference, str(case), str(device))

    return Case('SH_reconstruct', 'sh_3x16_9x33', {'coeffs': coeffs}, call, definition, diff=('coeffs',), cotangents=[weights],
                unread=('coeffs',))


def _envmap_case():
    texels = torch.rand(6, 70, 3, generator=torch.Generator().manual_seed(2201)) * 3.0 + 0.01

    def call(rd, t):
        ys, xs, norm = _modules()[3].envmap_sampling_tables(t['texels'], rd)
        return [], [ys, xs, torch.tensor(norm, dtype=torch.float64)]

    def definition(case, plain, backend, device):
        from redner_amd import render_pytorch as rp
        env = rp.EnvironmentMap(texels.clone())                                 # torch on the CPU: test_sh_envmap._run_tables
        ys, xs, norm = plain['extras']
        assert torch.equal(xs, env.sample_cdf_xs) and torch.equal(ys, env.sample_cdf_ys) and float(norm) == env.pdf_norm

    return Case('envmap_sampling_tables', 'envmap_tables_6x70', {'texels': texels}, call, definition)


def _deferred_case(alpha):
    types, params = t_deferred._scaled_lights(mk.light_sets()['one_each'])
    assert sorted(types) == [0, 1, 2, 3]
    g, _ = t_deferred._off_the_kinks(mk.synthetic_g_buffer(2301 + alpha, 1, 6, 10, 2, alpha), types, params)
    params, ranges = torch.from_numpy(params), ((0, 4),)
    weights = _randn(2303 + alpha, 1, 6, 10, 3 + alpha)

    def call(rd, t):
        return [_modules()[1].DeferredShade.apply(t['g_buffer'], t['light_params'], tuple(types), ranges, 2, bool(alpha), rd)], []

    def definition(case, plain, backend, device):
        g64, p64 = g.double().requires_grad_(True), params.double().requires_grad_(True)
        img = t_deferred._definition_shade(g64, types, p64, ranges, 2, alpha)
        img.backward(weights.double())
        got = {'image': plain['outs'][0], 'd_g_buffer': plain['grads']['g_buffer'], 'd_light_params': plain['grads']['light_params']}
        want = {'image': img.detach(), 'd_g_buffer': g64.grad, 'd_light_params': p64.grad}
        for k in got:                                                           # test_deferred._run_definition_case
            worst = t_deferred._worst_slice(got[k], want[k], '%s %s' % (case, k))
            print(case, k, '%.2e' % worst)
            assert worst < parity_util.TOL, (case, k, worst)
        # the public front end packs the same table from light objects
        ru = _modules()[1]
        lights = mk.lights_from_table(ru, np.asarray(types), params.numpy(), device=device)
        with torch.no_grad():
            again = ru.deferred_shade(g.clone().to(device), lights, alpha=bool(alpha), aa_samples=2, backend=backend)
        assert torch.equal(again.cpu(), plain['outs'][0])

    return Case('deferred_shade', 'deferred_6x10_aa2_alpha%d' % alpha, {'g_buffer': g, 'light_params': params}, call, definition,
                diff=('g_buffer', 'light_params'), cotangents=[weights], reads=('g_buffer', 'light_params'),
                subsets=(('g_buffer',), ('light_params',)), small=('light_params',))


@contextlib.contextmanager
def _shadow_chunk(rays):
    """csrc/deferred.h: shadow_chunk reads RDR_DEFERRED_SHADOW_CHUNK on every call (process-wide: one setter at a time)"""
    assert 'RDR_DEFERRED_SHADOW_CHUNK' not in os.environ
    os.environ['RDR_DEFERRED_SHADOW_CHUNK'] = str(rays)
    try:
        yield
    finally:
        del os.environ['RDR_DEFERRED_SHADOW_CHUNK']


AO_RAYS, AO_RADIUS = 8, 0.8
# the 480 texels of the 20 x 24 floor in at least two chunks: 256 texels of shadow rays; 8 rays x 64 texels of occlusion rays; with
# both at once 256 serves both (two chunks of shadow rays, fifteen of 32 texels' occlusion rays)
SHADED = {'shadowed': (True, False, 256), 'occluded': (False, True, AO_RAYS * 64), 'shadowed_occluded': (True, True, 256)}


def _shaded_case(kind, seed=None, shared=None):
    """deferred_shade over the floor patch of test_deferred_shadows with its BLOCKERS as the occluder scene, whose triangles are an
    input: `call` builds the scene from t['triangles'] on every run (the adjoint needs no scene, so they are `unread`) and runs
    the shade under the kind's chunk size.  `shared`, condition H: an occluder scene built by the caller, who also holds the
    chunk size (the environment is the process's); `seed`: another floor."""
    shadows, occlusion, chunk = SHADED[kind]
    alpha = 1
    if occlusion:                                                            # seven rows with the SH triple; normals tilted
        g, types, params = t_ao.tilted_floor(alpha, **({} if seed is None else {'seed': seed}))
        assert types == t_ao.ao_lights()[0] and len(types) == 7
    else:
        assert seed is None
        floor = t_shadows.floor_case(alpha)
        g, types, params = floor['g'], floor['types'], floor['params']
    assert tuple(g.shape) == (1, t_shadows.HG, t_shadows.WG, 10) and t_shadows.HG * t_shadows.WG == 480
    ranges = ((0, len(types)),)
    up = mk.upstream((1, t_shadows.HG // t_shadows.AA, t_shadows.WG // t_shadows.AA, 3 + alpha))
    triangles = torch.from_numpy(t_shadows.BLOCKERS.astype(np.float32))

    def shade(rd, t, scene):
        scenes = (scene.scene,)
        return _modules()[1].DeferredShade.apply(t['g_buffer'], t['light_params'], tuple(types), ranges, t_shadows.AA, bool(alpha), rd,
                                                 scenes if shadows else None, *((scenes, AO_RAYS, AO_RADIUS) if occlusion else ()))

    def call(rd, t):
        if shared is not None:
            out = shade(rd, t, shared)
        else:
            device = t['g_buffer'].device
            scene = _modules()[1].occluder_scene(t_shadows.triangle_scene(t['triangles'].contiguous(), device), device=device, backend=rd)
            with _shadow_chunk(chunk):
                out = shade(rd, t, scene)
        return [out[0]], list(out[1:])

    def definition(case, plain, backend, device):
        words = list(plain['extras'])
        assert len(words) == shadows + occlusion and all(w.dtype == torch.int32 and tuple(w.shape) == (1, 20, 24) for w in words)
        vis = words.pop(0) if shadows else None
        if shadows:
            assert (t_shadows.as_words(vis) != (1 << len(types)) - 1).any()
        if occlusion:                                                        # test_deferred_ao._run_values_and_gradients, _run_with_shadows
            got = dict(image=plain['outs'][0], vis=vis, words=words[0], d_g=plain['grads']['g_buffer'], d_p=plain['grads']['light_params'])
            o = t_ao._check_definition(got, g, types, params, ranges, AO_RAYS, t_shadows.AA, alpha, up, str(case))
            assert float(o.min()) < 0.8 and float((o == 1).double().mean()) > 0.1 and float((o < 1).double().mean()) > 0.1
            return
        # test_deferred_shadows._run_values_and_gradients, with the mask of the device's own words
        bits = t_shadows.as_words(vis)[0]
        lit = np.stack([((bits >> np.uint32(b)) & 1).astype(bool) for b in range(len(types))])
        g64, p64 = g.double().requires_grad_(True), torch.from_numpy(params).double().requires_grad_(True)
        want = t_shadows.definition_shadowed(g64, types, p64, lit, t_shadows.AA, alpha)
        want.backward(up.double())
        for k, a, b in (('image', plain['outs'][0], want.detach()), ('d_g_buffer', plain['grads']['g_buffer'], g64.grad),
                        ('d_light_params', plain['grads']['light_params'], p64.grad)):
            worst = t_deferred._worst_slice(a, b, '%s %s' % (case, k))
            print(case, k, '%.2e' % worst)
            assert worst < parity_util.TOL, (case, k, worst)

    name = 'deferred_%s_20x24_aa2_alpha%d' % (kind, alpha) + ('' if seed is None else '_%d' % seed)
    inputs = {'g_buffer': g.clone(), 'light_params': torch.from_numpy(np.asarray(params, np.float32)).clone(), 'triangles': triangles}
    return Case('deferred_shade', name, inputs, call, definition, diff=('g_buffer', 'light_params'), cotangents=[up],
                reads=('g_buffer', 'light_params'), unread=('triangles',), subsets=(('g_buffer',), ('light_params',)),
                saved_extras=tuple(range(shadows + occlusion)), small=('light_params',))


SPECULAR_MASK_SEED = 41                                                      # test_deferred_specular._run_visibility


def _specular_case(masked, seed=None):
    """DeferredSpecular on a case of test_deferred_specular (two images, the seven mixed rows, per-image ranges): `masked`, that of
    _run_visibility with its seeded random words as the fifth input.  `seed`, condition H: the same shapes from the generator at
    another seed (no texel is taken off a gate: such a case is held to its own plain bits only)."""
    name = 'grid_17x16_aa2_alpha1' if masked else 'grid_5x7_aa2_alpha1'
    if seed is None:
        base = t_spec._definition_case(name)
    else:
        n, h, w, aa, alpha, types, ranges = t_spec._shape_of(name)
        g, mat, eye = t_spec.generate(seed, n, h, w, aa, alpha)
        base = dict(g=g, mat=mat, eye=eye, types=types, params=t_spec.light_rows(seed + 5000, types), ranges=ranges, aa=aa, alpha=alpha)
    n, hg, wg = base['g'].shape[:3]
    inputs = {'g_buffer': base['g'].clone(), 'material': base['mat'].clone(), 'eye': base['eye'].clone(),
              'light_params': torch.from_numpy(np.asarray(base['params'], np.float32)).clone()}
    words = None
    if masked:
        words = torch.from_numpy(np.random.default_rng(SPECULAR_MASK_SEED).integers(-2 ** 31, 2 ** 31, (n, hg, wg), dtype=np.int64))
        inputs['visibility'] = words.to(torch.int32)
    up = mk.upstream((n, hg // base['aa'], wg // base['aa'], 3))

    def call(rd, t):
        return [_modules()[1].DeferredSpecular.apply(t['g_buffer'], t['material'], t['eye'], t['light_params'], tuple(base['types']),
                                                     tuple(base['ranges']), base['aa'], bool(base['alpha']), rd, t.get('visibility'))], []

    def definition(case, plain, backend, device):
        assert seed is None
        if masked:
            up64, want = t_spec._reference(base, vis=words & 0xffffffff)
            assert float((want['image'] - base['want']['image']).abs().sum()) > 0          # the mask removes light
        else:
            up64, want = base['up'], base['want']
        assert torch.equal(up64, up)
        out = {'image': plain['outs'][0], 'd_g_buffer': plain['grads']['g_buffer'], 'd_material': plain['grads']['material'],
               'd_eye': plain['grads']['eye'], 'd_light_params': plain['grads']['light_params']}
        t_spec._assert_parity(out, want, str(case))

    diff = ('g_buffer', 'material', 'eye', 'light_params')
    label = 'specular_%s%dx%d_aa%d_alpha%d' % ('masked_' if masked else '', hg // base['aa'], wg // base['aa'], base['aa'], base['alpha'])
    return Case('deferred_specular', label + ('' if seed is None else '_%d' % seed), inputs, call, definition, diff=diff,
                cotangents=[up], reads=tuple(inputs), subsets=tuple((n,) for n in diff) + (('material', 'eye'),),
                small=('eye', 'light_params'))


BOX, GRID = 'box4', 'grid7x9'               # closed, irregular, 98 vertices: more than one workgroup; open, 63 vertices
LMD = 0.3


def _normal_case(scheme):
    vertices, indices = mg.mesh(BOX)
    weights = _randn(2401, len(vertices), 3)

    def call(rd, t):
        sm = _modules()[2]
        topology = sm.MeshTopology(t['indices'], len(vertices), backend=rd)
        return [sm.compute_vertex_normal(t['vertices'], t['indices'], scheme, topology=topology)], []

    def definition(case, plain, backend, device):
        x = vertices.double().requires_grad_(True)
        normals = t_normal._definition(x, indices.long(), scheme)
        grad, = torch.autograd.grad(normals, x, weights.double())
        _rel_hold({'normals': plain['outs'][0].numpy(), 'd_vertices': plain['grads']['vertices'].numpy()},
                  {'normals': normals.detach().numpy(), 'd_vertices': grad.numpy()}, str(case))

    return Case('compute_vertex_normal', 'vertex_normal_%s' % scheme, {'vertices': vertices, 'indices': indices}, call, definition,
                diff=('vertices',), cotangents=[weights], reads=('vertices',), unread=('indices',))


def _laplacian_case(scheme):
    vertices, indices = mg.mesh(BOX)
    weights = _randn(2501, len(vertices), 3)
    control = torch.rand(len(vertices), generator=torch.Generator().manual_seed(2502)) * 0.75 + 0.25

    def call(rd, t):
        sm = _modules()[2]
        topology = sm.MeshTopology(t['indices'], len(vertices), backend=rd)
        return [sm.mesh_laplacian(t['vertices'], t['indices'], scheme, t['control'], topology=topology)], []

    def definition(case, plain, backend, device):
        x = vertices.double().requires_grad_(True)
        shift, _ = t_smooth._definition(x, indices.long(), scheme, control.double())
        grad, = torch.autograd.grad(shift, x, weights.double())
        _rel_hold({'shift': plain['outs'][0].numpy(), 'd_vertices': plain['grads']['vertices'].numpy()},
                  {'shift': shift.detach().numpy(), 'd_vertices': grad.numpy()}, str(case))

    return Case('mesh_laplacian', 'mesh_laplacian_%s' % scheme, {'vertices': vertices, 'indices': indices, 'control': control}, call,
                definition, diff=('vertices',), cotangents=[weights], reads=('vertices', 'control'), unread=('indices',))


def _smooth_case():
    vertices, indices = mg.mesh(GRID)

    def call(rd, t):
        sm = _modules()[2]
        topology = sm.MeshTopology(t['indices'], len(vertices), backend=rd)
        address, version = t['vertices'].data_ptr(), t['vertices']._version
        assert sm.smooth(t['vertices'], t['indices'], LMD, 'reciprocal', topology=topology, iterations=2) is None
        # written through, into the caller's memory, whatever its layout; a leaf stays a leaf
        assert t['vertices'].data_ptr() == address and t['vertices']._version > version
        assert t['vertices'].is_leaf and t['vertices'].requires_grad and t['vertices'].grad is None
        return [], [t['vertices']]

    def definition(case, plain, backend, device):
        v, control = vertices.double(), t_smooth._integer_bound(indices, len(vertices)).double()
        for _ in range(2):
            v = v + t_smooth._definition(v, indices.long(), 'reciprocal', control)[0] * LMD
        moved = plain['extras'][0].double() - vertices.double()                 # (test_mesh_smooth._displacement)
        assert float(moved.abs().max()) > 1e-3
        _rel_hold({'displacement': moved.numpy()}, {'displacement': (v - vertices.double()).numpy()}, str(case))

    return Case('smooth', 'smooth_grid', {'vertices': vertices, 'indices': indices}, call, definition, leaf=('vertices',))


def _bound_case():
    vertices, indices = mg.mesh(GRID)

    def call(rd, t):
        sm = _modules()[2]
        topology = sm.MeshTopology(t['indices'], len(vertices), backend=rd)
        return [], [sm.bound_vertices(t['vertices'], t['indices'], topology=topology)]

    def definition(case, plain, backend, device):
        want = t_smooth._integer_bound(indices, len(vertices))
        assert torch.equal(plain['extras'][0], want) and 0 < int(want.sum()) < len(vertices)

    return Case('bound_vertices', 'bound_vertices_grid', {'vertices': vertices, 'indices': indices}, call, definition)


# (weights that are fp32 numbers: the C ABI takes them as floats, and test_pyramid_loss holds the fp64 terms to 1e-12)
LOSS_SHAPE, LOSS_LEVELS, LOSS_CLAMP, LOSS_WEIGHTS, LOSS_UPSTREAM = (2, 37, 41, 3), 3, 0.5, (0.75, 1.25, 2.0), 0.625


def _loss_case(seed=2601):
    image = torch.rand(*LOSS_SHAPE, generator=torch.Generator().manual_seed(seed))
    target = torch.rand(*LOSS_SHAPE, generator=torch.Generator().manual_seed(seed + 1))

    def call(rd, t):
        loss, terms = _modules()[0].gaussian_pyramid_loss(t['image'], t['target'], LOSS_LEVELS, clamp=LOSS_CLAMP, weights=LOSS_WEIGHTS,
                                                          return_terms=True, backend=rd)
        return [loss], [terms]

    def definition(case, plain, backend, device):
        # the per-element bars of test_pyramid_loss on a run with upstream 1 (what they are derived for) ...
        unit = t_loss._native(backend, device, image, target, LOSS_LEVELS, LOSS_CLAMP, LOSS_WEIGHTS, levels=True)
        t_loss._check_definition(unit, image, target, LOSS_LEVELS, LOSS_CLAMP, LOSS_WEIGHTS, str(case))
        clamped = float(((image - target).abs() > LOSS_CLAMP).float().mean())
        assert 0.05 < clamped < 0.6, ('the clamp is exercised', clamped)
        # ... and the plain call (upstream 0.625): the same loss and terms, the gradient within the same per-element bar
        assert np.array_equal(plain['outs'][0].numpy(), unit['loss']) and np.array_equal(plain['extras'][0].numpy(), unit['terms'])
        # k_grad counts the product with the upstream gradient, and every term of the bar scales with it
        a = mloss.taps()
        d0, passes = mloss.diff32(image.numpy(), target.numpy(), LOSS_CLAMP)
        acc, absacc = t_loss._gradient([d0.astype(np.float64)] + [v.astype(np.float64) for v in unit['levels']], LOSS_WEIGHTS, a)
        want, bar = LOSS_UPSTREAM * acc, mloss.k_grad(LOSS_LEVELS) * t_loss.U * LOSS_UPSTREAM * absacc
        for name, sign in (('image', 1.0), ('target', -1.0)):
            grad = plain['grads'][name].numpy().astype(np.float64)
            assert np.all(grad[~passes] == 0.0), (case, name, 'gradient where the clamp does not pass')
            ratio = float((np.abs(grad - sign * want)[passes] / np.maximum(bar[passes], 1e-300)).max())
            print(case, 'd_' + name, 'worst error / bar %.3f' % ratio)
            assert np.all(np.abs(grad - sign * want)[passes] <= bar[passes]), (case, name, ratio)

    both = ('image', 'target')
    return Case('gaussian_pyramid_loss', 'pyramid_loss_%d' % seed, {'image': image, 'target': target}, call, definition, diff=both,
                cotangents=[torch.tensor(LOSS_UPSTREAM)], reads=both, subsets=(('image',), ('target',), both))


ANGLES = mpose.ANGLES[2]


def _rotate_case():
    angles, weights = torch.tensor(ANGLES), _randn(2701, 3, 3)

    def call(rd, t):
        return [_modules()[4].gen_rotate_matrix(t['angles'], backend=rd)], []

    def definition(case, plain, backend, device):
        a = angles.double().requires_grad_(True)
        R = t_pose._rotation64(a)
        (R * weights.double()).sum().backward()
        t_pose._hold({'R': plain['outs'][0].numpy(), 'd_angles': plain['grads']['angles'].numpy()},
                     {'R': R.detach().numpy(), 'd_angles': a.grad.numpy()}, str(case))

    return Case('gen_rotate_matrix', 'rotate_matrix', {'angles': angles}, call, definition, diff=('angles',), cotangents=[weights],
                reads=('angles',))


def _pose_case(given, seed=2801):
    """two sets of 513 and 8 vertices: past one chunk of 512 (csrc/pose.h), and a set smaller than a wave"""
    sets = [_randn(seed, 513, 3) + torch.tensor([0.5, -1.0, 2.0]), _randn(seed + 1, 8, 3) + torch.tensor([0.5, -1.0, 2.0])]
    weights = [_randn(seed + 2, 513, 3), _randn(seed + 3, 8, 3)]
    inputs = {'v0': sets[0], 'v1': sets[1], 'angles': torch.tensor(ANGLES), 'translation': torch.tensor(mpose.TRANSLATION)}
    if given:
        inputs['center'] = torch.tensor(mpose.CENTER)

    def call(rd, t):
        return list(_modules()[4].pose_vertices([t['v0'], t['v1']], t['angles'], t['translation'], center=t.get('center'), backend=rd)), []

    def definition(case, plain, backend, device):
        want = t_pose._definition(sets, weights, ANGLES, not given)
        got = {'d_angles': plain['grads']['angles'].numpy(), 'd_translation': plain['grads']['translation'].numpy()}
        if given:
            got['d_center'] = plain['grads']['center'].numpy()
        for k in range(2):
            got['out%d' % k], got['d_vertices%d' % k] = plain['outs'][k].numpy(), plain['grads']['v%d' % k].numpy()
        # R as the node of the outputs keeps it (`grad_fn.saved`, what make_pose_golden.constants reads)
        t = _make(case, device)
        got['R'] = mpose.constants(case.call(backend, t)[0])[0].cpu().numpy()
        t_pose._hold(got, want, str(case))
        assert backend.pose_plan([513, 8])[2] >= 3                              # chunks: two of the first set, one of the second

    diff = tuple(inputs)
    reads = tuple(n for n in inputs if n != 'translation')
    subsets = (('translation',), ('v1',)) + ((('center',),) if given else ())
    return Case('pose_vertices', 'pose_%s_%d' % ('given' if given else 'own', seed), inputs, call, definition, diff=diff, cotangents=weights,
                reads=reads, unread=('translation',), subsets=subsets, unused=(1,),
                small=tuple(n for n in ('angles', 'translation', 'center') if n in inputs))


# op -> its cases, name -> how the case is made.  A case is built (inputs, and for the mip pyramid the fp64 reference it shares
# with test_texture) when a test first asks for it, not when the module is collected.
CASES = {
    'generate_mipmap': {'mipmap_5x7x3': lambda: _mip_case((5, 7, 3)), 'mipmap_70x66x3': lambda: _mip_case((70, 66, 3))},
    'SH_reconstruct': {'sh_3x16_9x33': _sh_case},
    'envmap_sampling_tables': {'envmap_tables_6x70': _envmap_case},
    'deferred_shade': {'deferred_6x10_aa2_alpha0': lambda: _deferred_case(0), 'deferred_6x10_aa2_alpha1': lambda: _deferred_case(1),
                       'deferred_shadowed_20x24_aa2_alpha1': lambda: _shaded_case('shadowed'),
                       'deferred_occluded_20x24_aa2_alpha1': lambda: _shaded_case('occluded'),
                       'deferred_shadowed_occluded_20x24_aa2_alpha1': lambda: _shaded_case('shadowed_occluded')},
    'deferred_specular': {'specular_5x7_aa2_alpha1': lambda: _specular_case(False),
                          'specular_masked_17x16_aa2_alpha1': lambda: _specular_case(True)},
    'compute_vertex_normal': {'vertex_normal_max': lambda: _normal_case('max'), 'vertex_normal_cotangent': lambda: _normal_case('cotangent')},
    'mesh_laplacian': {'mesh_laplacian_reciprocal': lambda: _laplacian_case('reciprocal'),
                       'mesh_laplacian_uniform': lambda: _laplacian_case('uniform'),
                       'mesh_laplacian_cotangent': lambda: _laplacian_case('cotangent')},
    'smooth': {'smooth_grid': _smooth_case},
    'bound_vertices': {'bound_vertices_grid': _bound_case},
    'gaussian_pyramid_loss': {'pyramid_loss_2601': _loss_case},
    'gen_rotate_matrix': {'rotate_matrix': _rotate_case},
    'pose_vertices': {'pose_own_2801': lambda: _pose_case(False), 'pose_given_2801': lambda: _pose_case(True)},
}
ALL_CASES = [name for op in TABLE for name in CASES[op]]
_BUILT = {}


def _case(name):
    if name not in _BUILT:
        op, = [op for op in CASES if name in CASES[op]]
        _BUILT[name] = CASES[op][name]()
        assert _BUILT[name].name == name and _BUILT[name].op == op, (name, op, _BUILT[name])
    return _BUILT[name]


def _pairs(conditions):
    return [pytest.param(name, letter, id='%s-%s' % (name, letter)) for op, letters in TABLE.items() for name in CASES[op]
            for letter in letters if letter in conditions]


def test_table_is_complete():
    """No op and no condition can drop out of the matrix unnoticed."""
    import redner_amd
    from redner_amd import render_utils
    assert sorted(TABLE) == sorted(NATIVE_OPS) == sorted(CASES)
    for op in NATIVE_OPS:
        assert callable(getattr(redner_amd, op, None) or getattr(render_utils, op)), op
        assert CASES[op] and all(_case(name).op == op for name in CASES[op]) and set(TABLE[op]) <= set('ABCDEFGHI'), op
        assert all(('B' in TABLE[op]) == bool(_case(name).diff) for name in CASES[op]), op                # an op with a gradient gets the gradient conditions
        assert ('I' in TABLE[op]) == ('B' in TABLE[op]), op                                              # ... and refuses a second differentiation
        assert all(('F' in TABLE[op]) == bool(_case(name).small) for name in CASES[op]), op                # ... F, where inputs may live on the host
    assert 'deferred_specular' in TABLE and 'I' in HARNESS_CONDITIONS and 'I' in GPU_CONDITIONS
    assert set(''.join(TABLE.values())) == set('ABCDEFGHI') == set(CONDITIONS) | {'H'}
    assert set(HARNESS_CONDITIONS) | set('FGH') == set(GPU_CONDITIONS) | {'H'} == set('ABCDEFGHI')
    assert len(set(ALL_CASES)) == len(ALL_CASES)
    # every existing case keeps no word output; the occluder cases save theirs; the small inputs are inputs
    for case in map(_case, ALL_CASES):
        assert bool(case.saved_extras) == ('shadowed' in case.name or 'occluded' in case.name), case
        assert set(case.small) <= set(case.diff), case
    # condition E names every input of every differentiable op on one side or the other
    for case in map(_case, ALL_CASES):
        if case.diff:
            assert set(case.reads) | set(case.unread) == set(case.inputs) and not set(case.reads) & set(case.unread), case


# ---- the plain call against the fp64 definition -----------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ALL_CASES)
def test_plain_is_the_definition_hostsim(hostsim_backend, name):
    case = _case(name)
    case.definition(case, _plain(case, hostsim_backend, CPU), hostsim_backend, CPU)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ALL_CASES)
def test_plain_is_the_definition_gpu(gpu_backend, name):
    case = _case(name)
    case.definition(case, _plain(case, gpu_backend, GPU), gpu_backend, GPU)


# ---- A. where the inputs live ---------------------------------------------------------------------------------------------------
def _views(case, backend, device):
    plain = _plain(case, backend, device)
    for kind in (_strided, _offset):
        for names in [(name,) for name in case.inputs] + [tuple(case.inputs)]:
            got = _run(case, backend, device, place={name: kind for name in names})
            _same(got, plain, '%s: %s as %s' % (case, ', '.join(names), kind.__name__))


# ---- B. what the upstream gradient is ---------------------------------------------------------------------------------------------
def _upstream(case, backend, device):
    plain = _plain(case, backend, device)
    # autograd's stride-0 expanded ones against dense ones
    tensors = _make(case, device)
    outs, extras = case.call(backend, tensors)
    sum(o.sum() for o in outs).backward()
    expanded = _snapshot(case, tensors, outs, extras)
    dense = _run(case, backend, device, cotangents=[torch.ones_like(c).to(device) for c in case.cotangents])
    _same(expanded, dense, '%s: out.sum().backward() against dense ones' % case)
    # upstream gradients that are not contiguous: by a product with a transposed weight, and handed over as they are
    wide = [k for k, c in enumerate(case.cotangents) if c.numel() > 1]
    for direct in ((False, True) if wide else ()):                              # (a 0-dim gradient has no layout)
        tensors = _make(case, device)
        outs, extras = case.call(backend, tensors)
        weights = [_strided(c, device) if k in wide else c.clone().to(device) for k, c in enumerate(case.cotangents)]
        seen = []
        for k in wide:
            outs[k].register_hook(lambda g, k=k: seen.append((k, g.is_contiguous())))
        if direct:
            torch.autograd.backward(outs, weights)
        else:
            sum((o * w).sum() for o, w in zip(outs, weights)).backward()
        # (handed over, every gradient arrives as it is; the product is contiguous where the weight's view is not dense)
        assert sorted(k for k, _ in seen) == wide and not (any if direct else all)(flat for _, flat in seen), \
            ('the gradient arrived contiguous', seen)
        _same(_snapshot(case, tensors, outs, extras), plain, '%s: an upstream gradient that is not contiguous (direct: %s)' % (case, direct))
    # outputs nobody uses against explicit zeros
    if case.unused is not None:
        tensors = _make(case, device)
        outs, extras = case.call(backend, tensors)
        weights = _cotangents(case, device)
        torch.autograd.backward([outs[k] for k in case.unused], [weights[k] for k in case.unused])
        partial = _snapshot(case, tensors, outs, extras)
        zeros = _run(case, backend, device, cotangents=[w if k in case.unused else torch.zeros_like(w) for k, w in enumerate(weights)])
        _same(partial, zeros, '%s: only outputs %s used' % (case, case.unused))
        assert not all(torch.equal(partial['grads'][n], plain['grads'][n]) for n in case.diff)


# ---- C. which inputs want a gradient ----------------------------------------------------------------------------------------------
def _wanted(case, backend, device):
    plain = _plain(case, backend, device)
    for subset in case.subsets:
        got = _run(case, backend, device, wants=subset)
        want = dict(plain, grads={n: (g if n in subset else None) for n, g in plain['grads'].items()})
        _same(got, want, '%s: only %s want a gradient' % (case, ', '.join(subset)))
        if case.op == 'gaussian_pyramid_loss' and subset == ('target',):
            assert torch.equal(got['grads']['target'], -plain['grads']['image'])
    for wants, guard in ((None, torch.no_grad), ((), torch.enable_grad)):
        with guard():
            tensors = _make(case, device, wants=wants)
            outs, extras = case.call(backend, tensors)
        assert all(o.grad_fn is None for o in outs) and (wants is None or not any(o.requires_grad for o in outs)), case
        _same(_snapshot(case, tensors, outs, extras), plain, '%s: no gradient recorded' % case, keys=('outs', 'extras'))
    if case.op == 'SH_reconstruct' and device.type == 'cuda':
        # the clamp mask (one byte per element) is allocated only where a gradient can be asked for
        def allocated(wants, guard):
            tensors = _make(case, device, wants=wants)
            torch.cuda.synchronize(device)
            before = torch.cuda.memory_allocated(device)
            with guard():
                outs, _ = case.call(backend, tensors)
            return torch.cuda.memory_allocated(device) - before, outs

        image_bytes = (4 * SH_RES[0] * SH_RES[1] * 3 + 511) // 512 * 512          # (torch's allocator hands out multiples of 512)
        for wants, guard in ((None, torch.no_grad), ((), torch.enable_grad)):
            without, _ = allocated(wants, guard)
            assert without == image_bytes, (wants, without, image_bytes)
        with_mask, _ = allocated(None, torch.enable_grad)
        assert with_mask > image_bytes, (with_mask, image_bytes)                # (the measure sees the mask where there is one)


# ---- D. the graph used twice ------------------------------------------------------------------------------------------------------
def _twice(case, backend, device):
    plain = _plain(case, backend, device)
    tensors = _make(case, device)
    outs, extras = case.call(backend, tensors)
    torch.autograd.backward(outs, _cotangents(case, device), retain_graph=True)
    _same(_snapshot(case, tensors, outs, extras), plain, '%s: the first of two backward passes' % case)
    torch.autograd.backward(outs, _cotangents(case, device))
    got = _snapshot(case, tensors, outs, extras)
    for name, g in plain['grads'].items():
        assert torch.equal(got['grads'][name], g + g) and torch.equal(got['grads'][name], 2.0 * g), (case, name)


# ---- E. edits between forward and backward ----------------------------------------------------------------------------------------
def _edit(t):
    t.zero_() if t.dtype == torch.int32 else t.mul_(0.5).add_(1.0)


def _edits(case, backend, device):
    plain = _plain(case, backend, device)
    for name in case.reads:
        # the adjoint reads this input; given contiguous it is the caller's own memory: torch's saved-tensor check must fire
        tensors = _make(case, device)
        outs, _ = case.call(backend, tensors)
        with torch.no_grad():
            _edit(tensors[name])
        with pytest.raises(RuntimeError, match=INPLACE):
            torch.autograd.backward(outs, _cotangents(case, device))
        # given as a view that is not contiguous the op read a private copy
        got = _run(case, backend, device, place={name: _strided}, between=lambda t, o, name=name: _edit(t[name]))
        _same(got, plain, '%s: %s (not contiguous) edited between forward and backward' % (case, name), keys=('outs', 'grads'))
    for name in case.unread:
        got = _run(case, backend, device, between=lambda t, o, name=name: _edit(t[name]))
        _same(got, plain, '%s: %s edited between forward and backward' % (case, name), keys=('grads',))
    # a word output that the op saved for its adjoint is the caller's tensor too: the same check must fire
    for k in case.saved_extras:
        tensors = _make(case, device)
        outs, extras = case.call(backend, tensors)
        assert not extras[k].requires_grad and extras[k].dtype == torch.int32
        with torch.no_grad():
            _edit(extras[k])
        with pytest.raises(RuntimeError, match=INPLACE):
            torch.autograd.backward(outs, _cotangents(case, device))
    # no op keeps its result by alias
    for k in range(len(case.cotangents)):
        got = _run(case, backend, device, between=lambda t, o, k=k: _edit(o[k]))
        _same(got, plain, '%s: output %d edited between forward and backward' % (case, k), keys=('grads',))
        assert not torch.equal(got['outs'][k], plain['outs'][k])


# ---- F. small parameters on the CPU -----------------------------------------------------------------------------------------------
def _small_on_cpu(case, backend, device):
    assert device.type == 'cuda' and case.small
    plain = _plain(case, backend, device)
    small = [n for n in case.small if n in case.inputs]
    assert small == list(case.small) and set(small) < set(case.diff)
    tensors = _make(case, device, place={n: _on_cpu for n in small})
    assert all(tensors[n].device.type == 'cpu' for n in small)
    outs, extras = case.call(backend, tensors)
    torch.autograd.backward(outs, _cotangents(case, device))
    assert all(tensors[n].grad.device.type == ('cpu' if n in small else 'cuda') for n in case.diff)
    _same(_snapshot(case, tensors, outs, extras), plain, '%s: %s on the CPU' % (case, ', '.join(small)))


# ---- G. a side stream -------------------------------------------------------------------------------------------------------------
def _poisoned(t):
    """A buffer of t's shape that no kernel may read yet: NaN (an index tensor: zeros, which stay in range)."""
    return torch.full_like(t, float('nan')) if t.is_floating_point() else torch.zeros_like(t)


def _late(device):
    """The producer chain of _side_stream, on the current stream: 20 additions over 2^26 floats -> a 0-dim tensor that is 0, but
    not before the chain has run."""
    big = torch.zeros(1 << 26, device=device)
    for _ in range(20):
        big = big + 1.0
    return big[:1].sum() - 20.0


def _side_stream(case, backend, device):
    """Forward and backward under `with torch.cuda.stream(side)`.  Every input and every upstream gradient is on the device
    beforehand (a copy from the host would make the host wait for the stream) and is written into a buffer of NaN, inside the
    `with`, as x + (big[:1].sum() - 20.0) behind a long producer chain on that stream (20 additions over 2^26 floats): the plain
    values, but not before the chain has run.  MeshTopology is built inside as well (its plan has the one read-back).  One torch
    reduction per result is the consumer on the same stream; then side.synchronize() and the plain bits.  A launch ordered
    on any other stream reads NaN.  A correct library can never fail this test; a wrong one can pass it by luck of timing."""
    assert device.type == 'cuda'
    plain = _plain(case, backend, device)
    staged = {name: x.clone().to(device) for name, x in case.inputs.items()}
    weights = _cotangents(case, device)
    buffers, weight_buffers = {name: _poisoned(x) for name, x in staged.items()}, [_poisoned(w) for w in weights]
    side = torch.cuda.Stream(device=device)
    torch.cuda.synchronize(device)
    with torch.cuda.stream(side):
        late = _late(device)                                                    # == 0, but ordered after the chain
        tensors = _make(case, device, place={name: (lambda x, d, name=name: torch.add(staged[name], late.to(staged[name].dtype),
                                                                                      out=buffers[name])) for name in case.inputs})
        cotangents = [torch.add(w, late, out=b) for w, b in zip(weights, weight_buffers)]
        outs, extras = case.call(backend, tensors)
        if outs:
            torch.autograd.backward(outs, cotangents)
        totals = [r.detach().double().sum() for r in outs + extras]
    side.synchronize()
    _same(_snapshot(case, tensors, outs, extras), plain, '%s: on a side stream' % case)
    for total, want in zip(totals, plain['outs'] + plain['extras']):
        assert float(total) == float(want.to(device).double().sum()), case
    del tensors, outs, extras, staged, buffers
    torch.cuda.empty_cache()                                                    # (the producer's 256 MB blocks)


# ---- I. a second differentiation --------------------------------------------------------------------------------------------------
def _second_order(case, backend, device):
    """Autograd runs `backward` in grad mode exactly under create_graph=True; the kernels of an adjoint record nothing, so the
    first gradient would come back not requiring a gradient and a loss built on it would drop that term without a word."""
    plain = _plain(case, backend, device)
    tensors = _make(case, device)
    outs, _ = case.call(backend, tensors)
    with pytest.raises(RuntimeError, match='cannot be differentiated again'):
        torch.autograd.grad(outs, [tensors[n] for n in case.diff], _cotangents(case, device), create_graph=True)
    assert all(tensors[n].grad is None for n in case.diff)
    # nothing was left half-done: the same case, plain
    _same(_run(case, backend, device), plain, '%s: a plain run after the refused one' % case)


CONDITIONS = {'A': _views, 'B': _upstream, 'C': _wanted, 'D': _twice, 'E': _edits, 'F': _small_on_cpu, 'G': _side_stream,
              'I': _second_order}


@pytest.mark.parametrize('name,letter', _pairs(HARNESS_CONDITIONS))
def test_calls_hostsim(hostsim_backend, name, letter):
    CONDITIONS[letter](_case(name), hostsim_backend, CPU)


@pytest.mark.gpu
@pytest.mark.parametrize('name,letter', _pairs(GPU_CONDITIONS))
def test_calls_gpu(gpu_backend, name, letter):
    CONDITIONS[letter](_case(name), gpu_backend, GPU)


# ---- H. two host threads ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_host_threads_gpu(gpu_backend):
    """rdr_set_stream is state of the calling host thread: two Python threads, each under its own side stream, started
    together, each run gaussian_pyramid_loss, pose_vertices, the shadowed and occluded deferred_shade and the masked
    deferred_specular forward and backward ten times on their own inputs and get the plain bits of those inputs every time.
    (One process, two threads.)  The occluder scene is built once, by the main thread, and traced by both threads under their
    two streams -- the walk kernels and their counters (hip/runtime.hip: persistent_counter) with two customers at once; the
    chunk size is set once around both, the environment being the process's.  What this covers is the FORWARD launches:
    autograd runs the backward node of a device tensor on its one worker thread of that device (under the forward call's
    stream), not on the Python thread that called backward(), so the backward launches of both threads come from the same host
    thread."""
    assert all('H' in TABLE[op] for op in ('gaussian_pyramid_loss', 'pose_vertices', 'deferred_shade', 'deferred_specular'))
    blockers = t_shadows.occluder(gpu_backend, t_shadows.BLOCKERS, GPU)
    work = [[_loss_case(2900 + 10 * k), _pose_case(bool(k), 2950 + 10 * k), _shaded_case('shadowed_occluded', 3000 + 10 * k, blockers),
             _specular_case(True, 3050 + 10 * k)] for k in range(2)]
    with _shadow_chunk(SHADED['shadowed_occluded'][2]):
        _two_host_threads(gpu_backend, work)


def _two_host_threads(gpu_backend, work):
    plains = [[_plain(case, gpu_backend, GPU) for case in cases] for cases in work]
    for item in range(len(work[0])):
        assert not torch.equal(plains[0][item]['outs'][0], plains[1][item]['outs'][0]), item
    for k in range(2):                                                         # both occluder paths and the mask did something
        vis, occlusion = (t_shadows.as_words(w) for w in plains[k][2]['extras'])
        assert (vis != 127).any() and (occlusion != (1 << AO_RAYS) - 1).any()
    staged = [[({n: x.clone().to(GPU) for n, x in case.inputs.items()}, _cotangents(case, GPU)) for case in cases] for cases in work]
    torch.cuda.synchronize(GPU)
    start, failures = threading.Barrier(2), []

    def worker(k):
        try:
            side = torch.cuda.Stream(device=GPU)
            with torch.cuda.stream(side):
                start.wait(timeout=20)
                for it in range(10):
                    for case, plain, (inputs, weights) in zip(work[k], plains[k], staged[k]):
                        # (device-to-device copies: the host does not wait for the stream between the launches)
                        place = {n: (lambda x, d, n=n: inputs[n].clone()) for n in case.inputs}
                        got = _run(case, gpu_backend, GPU, place=place, cotangents=[w.clone() for w in weights])
                        _same(got, plain, 'thread %d, pass %d, %s' % (k, it, case))
                side.synchronize()
        except BaseException as error:                                          # (reported by the main thread)
            failures.append((k, error))
            start.abort()                                                       # (the other thread does not wait for this one)

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not failures, failures


# ---- G for the composite: render_deferred with everything on, on a side stream ------------------------------------------------------
@pytest.mark.gpu
def test_render_deferred_side_stream_gpu(gpu_backend):
    """render_deferred(alpha, shadows, ambient occlusion, specular) of test_deferred_specular's sphere over a plane at 16 x 16,
    forward and backward under `with torch.cuda.stream(side)`: the G-buffer render, the occluder scene, the shadow and
    occlusion rays, both deferred kernels and their adjoints, and RenderFunction's adjoint, all behind _side_stream's producer
    chain -- the sphere's vertices, both materials' specular reflectance and roughness and the point light's intensity are
    written into NaN buffers as x + late on that stream; the camera position stays on the host.  Held to the same call on the
    default stream: the image and the gradient of the light's intensity (which passes through the deferred kernels only) bit for
    bit; the gradients that pass through RenderFunction (vertices, materials, camera position), which are summed with fp64
    atomics and are not bitwise reproducible from run to run, to test_schedule_matrix.GPU_BAR relative L2.  As for
    _side_stream: a correct library cannot fail this; a wrong one can pass by timing."""
    from redner_amd.render_pytorch import Texture
    from test_schedule_matrix import GPU_BAR
    ru = _modules()[1]
    res, aa, seed = 16, 2, 5
    written = ('vertices', 'ks0', 'roughness0', 'ks1', 'roughness1', 'intensity')

    def run(side):
        sc = t_spec._sphere_over_plane(GPU, (res, res))
        on = lambda x: torch.tensor(x, device=GPU)
        staged = {'vertices': sc.shapes[0].vertices.detach().clone(), 'intensity': on([12.0, 11.0, 10.0])}
        for m in range(2):
            staged['ks%d' % m] = sc.materials[m].specular_reflectance.mipmap[0].detach().clone()
            staged['roughness%d' % m] = sc.materials[m].roughness.mipmap[0].detach().clone()
        assert sorted(staged) == sorted(written) and sc.camera.position.device.type == 'cpu' and sc.camera.position.requires_grad
        # (the lights' other tensors on the device beforehand: a copy from the host would make the host wait for the stream)
        rest = [on([1.5, 3.0, -1.0]), on([-0.4, -1.0, 0.6]), on([0.8, 0.9, 1.0]), on([0.1, 0.12, 0.14]),
                torch.from_numpy(t_dsh.sh_coefficients(3)).to(GPU)]
        buffers, weights = {name: _poisoned(x) for name, x in staged.items()}, mk.upstream((res, res, 4)).to(GPU)
        buffers['upstream'] = _poisoned(weights)
        torch.cuda.synchronize(GPU)
        with (torch.cuda.stream(side) if side is not None else contextlib.nullcontext()):
            late = _late(GPU) if side is not None else torch.zeros((), device=GPU)
            leaf = {name: torch.add(x, late, out=buffers[name]).requires_grad_(True) for name, x in staged.items()}
            sc.shapes[0].vertices = leaf['vertices']
            for m in range(2):
                sc.materials[m].specular_reflectance, sc.materials[m].roughness = Texture(leaf['ks%d' % m]), Texture(leaf['roughness%d' % m])
            lights = [ru.PointLight(rest[0], leaf['intensity']), ru.DirectionalLight(rest[1], rest[2]), ru.AmbientLight(rest[3]),
                      ru.SHLight(rest[4])]
            img = ru.render_deferred(sc, lights, alpha=True, shadows=True, ambient_occlusion=4, ao_radius=1.0, specular=True,
                                     aa_samples=aa, seed=seed, device=GPU, backend=gpu_backend)
            img.backward(torch.add(weights, late, out=buffers['upstream']))
            total = img.detach().double().sum()                                 # a consumer on the same stream
        if side is not None:
            side.synchronize()
        else:
            torch.cuda.synchronize(GPU)
        out = {'image': _keep(img), 'camera position': _keep(sc.camera.position.grad)}
        out.update({name: _keep(t.grad) for name, t in leaf.items()})
        assert float(total) == float(out['image'].double().sum())
        return out

    want = run(None)
    assert tuple(want['image'].shape) == (res, res, 4)
    for name, t in want.items():
        assert t is not None and bool(torch.isfinite(t).all()) and bool(t.any()), name
    got = run(torch.cuda.Stream(device=GPU))
    torch.cuda.empty_cache()                                                    # (the producer's 256 MB blocks)
    for name in ('image', 'intensity'):
        assert torch.equal(got[name], want[name]), (name, 'differs from the default stream in %d of %d elements'
                                                    % (int((got[name] != want[name]).sum()), want[name].numel()))
    for name in ('vertices', 'ks0', 'roughness0', 'ks1', 'roughness1', 'camera position'):
        assert got[name] is not None and got[name].device.type == 'cpu', name
        d, n = float((got[name].double() - want[name].double()).norm()), float(want[name].double().norm())
        print('render_deferred on a side stream, d_%s: %.2e of GPU_BAR %.0e' % (name, d / n, GPU_BAR))
        assert d <= GPU_BAR * n + 1e-30, (name, d / n)
