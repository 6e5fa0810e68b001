"""Generic textures of any width (csrc/bsdf.h: tex_fetch_each / adj_tex_fetch).  A material's `generic_texture` used to be
refused above 16 channels; now its channels are streamed, forward and backward, without a per-lane array.

1. parity with the reference (fixtures of tests/golden/make_wide_generic_golden.py: the oracle's values): 8 x 8 x {17, 33, 64}
   with mips on the textured sphere at 32 x 32 -- the magnified and the between-levels branch of the lookup --, the 33-wide once
   more under a uv scale that reaches the coarsest level alone, and a constant 20-channel texture;
2. the forward split, bit for bit: the first 16 generic channels of cat(A, B) are the render of A alone;
3. linearity under primary edge sampling (no oracle exists there): a 32-wide render's gradients are those of its two halves;
4. lanes of one wave on materials of different widths (5, 33, none): against the oracle, and against one quad per scene;
5. the reference's unmodified pyredner.render_generic on the drop-in module with a 32-channel pyredner.Texture.
Every render test runs on the CPU harness and, marked gpu, on both builds of the library."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import parity_util
from oracle_util import rel_l2
from golden import make_deferred_golden as mk
from golden import make_texture_golden as mt
from golden import make_wide_generic_golden as mw

GOLD = parity_util.GOLD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU, GPU = torch.device('cpu'), torch.device('cuda:0')
# fp32 results that differ only in the order of fp64 atomics (and in one final rounding): the bar of tests/test_schedule_matrix.py
ORDER_TOL = 2e-6


def _check(name, out, gold, tag):
    rep = parity_util.compare(out, gold, name)
    print(name, tag, {k: '%.2e' % e['rel_l2'] for k, e in rep.items()})
    parity_util.record(name, rep, tag)
    parity_util.assert_parity(rep, name)


def _texture(backend):
    import redner_amd
    return lambda t, uv: redner_amd.Texture(t, uv, backend=backend)


# ---- 1. parity with the reference -----------------------------------------------------------------------------------------------
SPHERE_CASES = [(w, False) for w in mw.WIDTHS] + [(mw.CONSTANT_WIDTH, False), (mw.FAR_WIDTH, True)]


def _sphere_id(case):
    return ('constant_%d' if case[0] == mw.CONSTANT_WIDTH else 'sphere_%d') % case[0] + ('_far' if case[1] else '')


def _run_sphere_case(backend, device, tag, width, far):
    constant = width == mw.CONSTANT_WIDTH
    diffuse = mt.sphere_texels()[0].to(device).requires_grad_(True)
    generic = (mw.constant_generic() if constant else mw.generic_texels(width)).to(device).requires_grad_(True)
    sc = mw.sphere_scene(device, _texture(backend), diffuse, generic, far)
    assert len(sc.materials[0].generic_texture.mipmap) == (1 if constant else 4)
    img = mt.render_e2e(sc, 'sphere', [backend.channels.radiance, backend.channels.generic_texture], device, backend)
    assert tuple(img.shape) == mw.FRAME + (3 + width,) and generic.grad.shape == generic.shape
    out = {'image': img.detach().cpu().numpy(), 'grad_diffuse': diffuse.grad.cpu().numpy(), 'grad_generic': generic.grad.cpu().numpy()}
    name = 'wide_generic_' + _sphere_id((width, far))
    _check(name, out, np.load(os.path.join(GOLD, name + '.npz')), tag)


@pytest.mark.parametrize('case', SPHERE_CASES, ids=_sphere_id)
def test_sphere_parity_hostsim(hostsim_backend, case):
    _run_sphere_case(hostsim_backend, CPU, 'hostsim', *case)


@pytest.mark.gpu
@pytest.mark.parametrize('case', SPHERE_CASES, ids=_sphere_id)
def test_sphere_parity_gpu(gpu_backend, case):
    _run_sphere_case(gpu_backend, GPU, 'gpu', *case)


# ---- 2. forward split -------------------------------------------------------------------------------------------------------------
def _forward(sc, backend, device, channels, bounces=1):
    from redner_amd.render_pytorch import RenderFunction
    args = RenderFunction.serialize_scene(sc, mt.E2E_SAMPLES, bounces, channels=channels, sampler_type=backend.SamplerType.sobol,
                                          device=device, backend=backend)
    return RenderFunction.apply(mt.E2E_SEEDS['sphere'], *args)


def _run_forward_split(backend, device):
    diffuse = mt.sphere_texels()[0].to(device)
    a, b = mw.generic_texels(16).to(device), mw.generic_texels(17, 0.5).to(device)
    channels = [backend.channels.radiance, backend.channels.generic_texture]
    with torch.no_grad():
        both = _forward(mw.sphere_scene(device, _texture(backend), diffuse, torch.cat([a, b], dim=2)), backend, device, channels)
        alone = _forward(mw.sphere_scene(device, _texture(backend), diffuse, a), backend, device, channels)
    assert tuple(both.shape) == mw.FRAME + (36,) and tuple(alone.shape) == mw.FRAME + (19,)
    assert alone[:, :, 3:].abs().sum() > 0
    assert torch.equal(both[:, :, :19], alone)


def test_forward_split_hostsim(hostsim_backend):
    _run_forward_split(hostsim_backend, CPU)


@pytest.mark.gpu
def test_forward_split_gpu(gpu_backend):
    _run_forward_split(gpu_backend, GPU)


# ---- 3. linearity under primary edge sampling -------------------------------------------------------------------------------------
def _edge_render(backend, device, texels, upstream):
    """-> (vertex gradient of the sphere, texel gradient): generic_texture alone, first hits, primary edge sampling on."""
    from redner_amd.render_pytorch import RenderFunction
    diffuse = mt.sphere_texels()[0].to(device)
    generic = texels.to(device).requires_grad_(True)
    sc = mw.sphere_scene(device, _texture(backend), diffuse, generic)
    vertices = sc.shapes[0].vertices.requires_grad_(True)
    args = RenderFunction.serialize_scene(sc, mt.E2E_SAMPLES, 0, channels=[backend.channels.generic_texture],
                                          sampler_type=backend.SamplerType.sobol, use_primary_edge_sampling=True,
                                          use_secondary_edge_sampling=False, device=device, backend=backend)
    img = RenderFunction.apply(mt.E2E_SEEDS['sphere'], *args)
    (img * upstream.to(device)).sum().backward()
    return vertices.grad.cpu(), generic.grad.cpu()


def _run_edge_linearity(backend, device):
    a, b = mw.generic_texels(16), mw.generic_texels(16, 0.5)
    up = mk.upstream(mw.FRAME + (32,))
    v_both, t_both = _edge_render(backend, device, torch.cat([a, b], dim=2), up)
    v_a, t_a = _edge_render(backend, device, a, up[:, :, :16].contiguous())
    v_b, t_b = _edge_render(backend, device, b, up[:, :, 16:].contiguous())
    assert v_both.abs().sum() > 0 and t_both.abs().sum() > 0
    ev, et = rel_l2(v_both, v_a.double() + v_b.double()), rel_l2(t_both, torch.cat([t_a, t_b], dim=2))
    print('edge linearity: vertices %.2e texels %.2e' % (ev, et))
    assert ev < ORDER_TOL and et < ORDER_TOL, (ev, et)


def test_edge_linearity_hostsim(hostsim_backend):
    _run_edge_linearity(hostsim_backend, CPU)


@pytest.mark.gpu
def test_edge_linearity_gpu(gpu_backend):
    _run_edge_linearity(gpu_backend, GPU)


# ---- 4. mixed widths in one wave ----------------------------------------------------------------------------------------------------
def _quad_render(backend, device, only=None):
    generics = [mw.generic_texels(w, 1.0 + k).to(device).requires_grad_(True) for k, w in enumerate(mw.QUAD_WIDTHS)]
    img = mw.render_quads(mw.quad_scene(device, _texture(backend), generics, only), device, backend)
    zero = lambda g: torch.zeros_like(g) if g.grad is None else g.grad       # noqa: E731
    return {'image': img.detach().cpu().numpy(), 'grad_generic5': zero(generics[0]).cpu().numpy(),
            'grad_generic33': zero(generics[1]).cpu().numpy()}


def _run_quads(backend, device, tag):
    out = _quad_render(backend, device)
    assert out['image'].shape == mw.QUAD_FRAME + (max(mw.QUAD_WIDTHS),)
    _check('wide_generic_quads', out, np.load(os.path.join(GOLD, 'wide_generic_quads.npz')), tag)
    singles = [_quad_render(backend, device, only=k) for k in range(3)]
    for key in out:
        total = sum(s[key].astype(np.float64) for s in singles)
        e = rel_l2(torch.from_numpy(out[key]), torch.from_numpy(total))
        print('quads one per scene:', key, '%.2e' % e)
        assert e < ORDER_TOL, (key, e)


def test_mixed_widths_hostsim(hostsim_backend):
    _run_quads(hostsim_backend, CPU, 'hostsim')


@pytest.mark.gpu
def test_mixed_widths_gpu(gpu_backend):
    _run_quads(gpu_backend, GPU, 'gpu')


# ---- 5. drop-in ---------------------------------------------------------------------------------------------------------------------
PYREF = os.path.join(ROOT, 'oracle', '_ref', 'pyref')
DROPIN_SCRIPT = r'''
import sys
sys.path[:0] = [%(root)r, %(root)r + '/tests', %(root)r + '/tests/golden', %(root)r + '/oracle/pystubs', %(pyref)r]
import numpy as np
from redner_amd import _capi
_capi.load(%(lib)r)                       # test harness in place of the GPU library
import redner_amd
redner_amd.install()                      # `import redner` now resolves to redner_amd.redner
import redner, pyredner                   # the reference's package, unmodified
pyredner.set_use_gpu(False)
import make_wide_generic_golden as mw
np.savez(sys.argv[1], **mw.dropin_render(pyredner, redner))
'''


@pytest.mark.skipif(not os.path.isfile(os.path.join(PYREF, 'pyredner', 'render_pytorch.py')),
                    reason='oracle/_ref/pyref not staged (make -C oracle)')
def test_unmodified_pyredner_render_generic_32_channels(hostsim_backend, tmp_path):
    from conftest import HOSTSIM_LIB
    script, out = tmp_path / 'dropin_wide.py', str(tmp_path / 'mine.npz')
    script.write_text(DROPIN_SCRIPT % {'root': ROOT, 'pyref': PYREF, 'lib': HOSTSIM_LIB})
    subprocess.check_call([sys.executable, str(script), out], stdout=subprocess.DEVNULL, timeout=600)
    name = 'wide_generic_dropin_%d' % mw.DROPIN_WIDTH
    _check(name, dict(np.load(out)), np.load(os.path.join(GOLD, name + '.npz')), 'hostsim')
