"""deferred_quad with soft shadows under the ways a training loop calls it: conditions A to I of tests/test_native_op_calls.py
(that module's docstring states them) on one case of tests/test_deferred_quad.py -- two images, the three quads, per-image ranges,
aa 2, alpha -- shadowed by test_deferred_shadows' BLOCKERS with 5 rays per texel and quad, the ray queue split into chunks of 37
texels.

The case object is that module's `Case`, and conditions A (views), B (upstream gradients), C (gradient subsets), D (retain_graph),
E (edits in place), F (the quad table on the host), G (a side stream) and I (create_graph) are its own runners, imported; the
occluder's triangles are an input, as in that module's shadowed cases.  The words and the factors are the case's other results:
every condition holds them, too, to the plain call's bits.  The op saves its FACTORS (fp32) for the adjoint, not the words, so
the saved-result half of condition E is restated here: that module's runner takes a saved result to be a word tensor.  The plain
call is held to the fp64 definition scaled by the device's factors under parity_util.TOL, every condition to the plain call with
torch.equal."""
import numpy as np
import pytest
import torch

import parity_util
import test_deferred_quad as t_quad
import test_deferred_quad_shadows as t_soft
import test_deferred_shadows as t_shadows
import test_native_op_calls as calls
from test_deferred import _worst_slice

CPU, GPU = calls.CPU, calls.GPU
LETTERS = 'ABCDEFGI'
NAME, RAYS, CHUNK_TEXELS = 'grid_5x7_aa2_alpha1', 5, 37


def _soft_case():
    base = t_quad._definition_case(NAME)
    n, hg, wg = base['g'].shape[:3]
    inputs = {'g_buffer': base['g'].clone(), 'quads': torch.from_numpy(base['quads']).clone(),
              'triangles': torch.from_numpy(t_shadows.BLOCKERS.astype(np.float32))}
    up = t_soft.random_upstream((n, hg // base['aa'], wg // base['aa'], 3), seed=43)

    def call(rd, t):
        ru = calls._modules()[1]
        device = t['g_buffer'].device
        scene = ru.occluder_scene(t_shadows.triangle_scene(t['triangles'].contiguous(), device), device=device, backend=rd)
        with calls._shadow_chunk(RAYS * CHUNK_TEXELS):
            out = ru.DeferredQuadShadowed.apply(t['g_buffer'], t['quads'], tuple(base['flags']), tuple(base['ranges']), base['aa'],
                                                bool(base['alpha']), rd, (scene.scene,) * n, RAYS)
        return [out[0]], list(out[1:])

    def definition(case, plain, backend, device):
        words, factors = plain['extras']
        assert words.dtype == torch.int32 and factors.dtype == torch.float32 and tuple(words.shape) == tuple(factors.shape) == (4, hg, wg)
        assert bool((factors < 1).any()) and bool((factors == 1).any())
        g64, q64 = base['g'].double().requires_grad_(True), torch.from_numpy(base['quads']).double().requires_grad_(True)
        want = t_soft.definition_scaled(g64, q64, base['flags'], base['ranges'], base['aa'], factors)
        want.backward(up.double())
        for k, a, b in (('image', plain['outs'][0], want.detach()), ('d_g_buffer', plain['grads']['g_buffer'][..., :9], g64.grad[..., :9]),
                        ('d_quads', plain['grads']['quads'], q64.grad)):
            worst = _worst_slice(a, b, '%s %s' % (case, k))
            print(case, k, '%.2e' % worst)
            assert worst < parity_util.TOL, (case, k, worst)

    return calls.Case('deferred_quad', 'quad_shadowed_5x7_aa2_alpha1', inputs, call, definition, diff=('g_buffer', 'quads'),
                      cotangents=[up], reads=('g_buffer', 'quads'), unread=('triangles',), subsets=(('g_buffer',), ('quads',)),
                      small=('quads',))


_BUILT = {}


def _case():
    if 'case' not in _BUILT:
        _BUILT['case'] = _soft_case()
    return _BUILT['case']


def test_the_case_takes_every_condition():
    """what test_native_op_calls.test_table_is_complete holds its own cases to"""
    import redner_amd
    case = _case()
    assert callable(redner_amd.deferred_quad) and case.op == 'deferred_quad' and case.diff and case.small
    assert set(LETTERS) == set(calls.CONDITIONS) and set(calls.HARNESS_CONDITIONS) | set('FG') == set(LETTERS)
    assert set(case.small) <= set(case.diff)
    assert set(case.reads) | set(case.unread) == set(case.inputs) and not set(case.reads) & set(case.unread)


def test_plain_is_the_definition_hostsim(hostsim_backend):
    case = _case()
    case.definition(case, calls._plain(case, hostsim_backend, CPU), hostsim_backend, CPU)


@pytest.mark.gpu
def test_plain_is_the_definition_gpu(gpu_backend):
    case = _case()
    case.definition(case, calls._plain(case, gpu_backend, GPU), gpu_backend, GPU)


@pytest.mark.parametrize('letter', [l for l in LETTERS if l in calls.HARNESS_CONDITIONS])
def test_calls_hostsim(hostsim_backend, letter):
    calls.CONDITIONS[letter](_case(), hostsim_backend, CPU)


@pytest.mark.gpu
@pytest.mark.parametrize('letter', [l for l in LETTERS if l in calls.GPU_CONDITIONS])
def test_calls_gpu(gpu_backend, letter):
    calls.CONDITIONS[letter](_case(), gpu_backend, GPU)


def _run_saved_factors(backend, device):
    """E, the saved result: the factors are the caller's tensor and the adjoint reads them -- an edit in place between forward and
    backward raises torch's saved-tensor error; the words are not saved, and an edit of them changes no gradient."""
    case = _case()
    plain = calls._plain(case, backend, device)
    tensors = calls._make(case, device)
    outs, (words, factors) = case.call(backend, tensors)
    assert not factors.requires_grad and not words.requires_grad
    with torch.no_grad():
        factors.mul_(0.5)
    with pytest.raises(RuntimeError, match=calls.INPLACE):
        torch.autograd.backward(outs, calls._cotangents(case, device))
    got = calls._run(case, backend, device, between=lambda t, o: None)
    calls._same(got, plain, 'a plain run after the refused one')
    tensors = calls._make(case, device)
    outs, (words, factors) = case.call(backend, tensors)
    with torch.no_grad():
        words.zero_()
    torch.autograd.backward(outs, calls._cotangents(case, device))
    calls._same(calls._snapshot(case, tensors, outs, [words, factors]), plain, 'the words edited', keys=('outs', 'grads'))


def test_saved_factors_hostsim(hostsim_backend):
    _run_saved_factors(hostsim_backend, CPU)


@pytest.mark.gpu
def test_saved_factors_gpu(gpu_backend):
    _run_saved_factors(gpu_backend, GPU)
