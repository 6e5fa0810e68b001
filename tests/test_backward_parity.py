"""Gradient parity against the oracle: every gradient tensor of the reference's backward pass
(vertices via the continuous adjoint + primary/secondary edge sampling, light intensity,
diffuse reflectance, camera) within 1e-4 relative L2 (BASELINE.json north_star) on identical
random sequences -- whole tensors, no masks.  The oracle's own run-to-run noise (fp32 atomics) is ~4e-7.

The config-size cases (BASELINE configs 2 and 3) live in tests/test_config_parity.py."""
import os

import numpy as np
import pytest
import torch

from golden.make_golden import CASES, render_case
from parity_util import DEFAULT_BUILD_DRAWS_OTHER_SAMPLES, GOLD, assert_parity, compare, libm_exact, record


def _check(backend, device, name, tag, tuning=None):
    b, res, spp, mb = CASES[name][:4]
    channels = CASES[name][4] if len(CASES[name]) > 4 else None
    opts = dict(CASES[name][5] if len(CASES[name]) > 5 else {})
    if tuning:
        opts['tuning'] = tuning
    out = render_case(backend, b, res, spp, mb, channels, opts, device=device)
    rep = compare(out, np.load(os.path.join(GOLD, name + '.npz')))
    if device.type == 'cuda' and not libm_exact():
        tag += '-default-build'
        if name in DEFAULT_BUILD_DRAWS_OTHER_SAMPLES:
            # the device's own libm: other, equally valid edge samples (parity_util.py lists the cases).  The forward image
            # involves no chaotic decision and is held as everywhere; the gradients are held to the statistical test.
            record(name, rep, tag + '-image-only')
            assert rep['image']['rel_l2'] < 1e-6, (name, rep['image'])
            return
    record(name, rep, tag)
    assert_parity(rep, name)


@pytest.mark.parametrize('name', list(CASES))
def test_backward_hostsim(hostsim_backend, name):
    _check(hostsim_backend, torch.device('cpu'), name, 'hostsim')


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(CASES))
def test_backward_gpu(gpu_backend, name):
    """Includes bunny_box_96x96x8: big enough that side streams, the second sample worker and the wave-summed
    gradient scatters are all active, compared with the oracle's fixture -- and the fisheye / panorama cameras WITH secondary
    edge sampling (make_golden.CHAOTIC_PICK_CASES): sample-exact on the GPU since its sin / cos / atan2 are glibc's."""
    _check(gpu_backend, torch.device('cuda:0'), name, 'gpu')


# The session asks for the large-frame forms at every size (tests/conftest.py: RDR_LARGE_FRAME_FORMS), so the two tests above
# check what the benchmark runs.  What the library picks BY ITSELF below 2^19 lanes per launch set -- every fixture here, every
# 256 x 256 optimisation loop -- is the one-launch hierarchical pick and the adjoint lists as they are.  In process the
# variable cannot be taken back (tuning.h: EnvDefaults is read once and ORed into every call's flags); these two flags select
# the same forms, because Backward::large_forms() has exactly two readers (nee_compact(), start_picks).  That this IS the
# same thing is pinned by test_small_frame_flags_equal_the_unset_variable_* below.
def _small_frame_forms():
    from redner_amd import _capi as K
    return K.TUNE_PICKH_ONE_LAUNCH | K.TUNE_NO_NEE_COMPACT


@pytest.mark.parametrize('name', list(CASES))
def test_backward_small_frame_forms_hostsim(hostsim_backend, name):
    _check(hostsim_backend, torch.device('cpu'), name, 'hostsim-small-frame-forms', {'flags': _small_frame_forms()})


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(CASES))
def test_backward_small_frame_forms_gpu(gpu_backend, name):
    _check(gpu_backend, torch.device('cuda:0'), name, 'gpu-small-frame-forms', {'flags': _small_frame_forms()})


UNSET_CODE = r'''
import os, sys
assert 'RDR_LARGE_FRAME_FORMS' not in os.environ and 'RDR_PICKH_ONE_LAUNCH' not in os.environ and 'RDR_NO_NEE_COMPACT' not in os.environ
sys.path[:0] = [%(root)r, %(root)r + '/tests']
import numpy as np, torch
from redner_amd import _capi
_capi.load(%(lib)r)
from redner_amd import redner
from golden.make_golden import CASES, render_case
out = {}
for name in %(cases)r:
    b, res, spp, mb = CASES[name][:4]
    for k, v in render_case(redner, b, res, spp, mb, None, {'tuning': %(tuning)r} if %(tuning)r else None, device=torch.device(%(dev)r)).items():
        out[name + '/' + k] = v
np.savez(sys.argv[1], **out)
print('RENDERED WITHOUT RDR_LARGE_FRAME_FORMS')
'''
UNSET_CASES = ('bunny_box_32x32x4', 'envmap_sphere_48x48x4')          # one lean, one environment-lit


def _unset_variable_vs_flags(backend, lib, dev, tuning, tmp_path):
    """-> {case/tensor: (a process without RDR_LARGE_FRAME_FORMS, zeroed flags; this process, the two flags)}"""
    import subprocess
    import sys
    from conftest import ROOT
    assert 'RDR_LARGE_FRAME_FORMS' in os.environ          # (the session: otherwise this test compares a thing with itself)
    env = {k: v for k, v in os.environ.items() if k not in ('RDR_LARGE_FRAME_FORMS', 'RDR_PICKH_ONE_LAUNCH', 'RDR_NO_NEE_COMPACT')}
    p = str(tmp_path / 'unset.npz')
    code = UNSET_CODE % {'root': ROOT, 'lib': lib, 'cases': UNSET_CASES, 'dev': dev, 'tuning': tuning}
    r = subprocess.run([sys.executable, '-c', code, p], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and 'RENDERED WITHOUT RDR_LARGE_FRAME_FORMS' in r.stdout, r.stdout[-1000:] + r.stderr[-2000:]
    unset = np.load(p)
    pairs = {}
    for name in UNSET_CASES:
        b, res, spp, mb = CASES[name][:4]
        mine = render_case(backend, b, res, spp, mb, None, {'tuning': dict(tuning, flags=_small_frame_forms())}, device=torch.device(dev))
        assert {name + '/' + k for k in mine} == {k for k in unset.files if k.startswith(name + '/')}
        for k, v in mine.items():
            pairs[name + '/' + k] = (unset[name + '/' + k], np.asarray(v))
    return pairs


def test_small_frame_flags_equal_the_unset_variable_hostsim(hostsim_backend, tmp_path):
    from conftest import HOSTSIM_LIB
    for k, (a, b) in _unset_variable_vs_flags(hostsim_backend, HOSTSIM_LIB, 'cpu', {'workers': 1}, tmp_path).items():
        assert np.array_equal(a, b), k


@pytest.mark.gpu
def test_small_frame_flags_equal_the_unset_variable_gpu(gpu_backend, tmp_path):
    from redner_amd import _capi
    for k, (a, b) in _unset_variable_vs_flags(gpu_backend, _capi.library_path(), 'cuda:0', {}, tmp_path).items():
        if k.endswith('/image'):
            assert np.array_equal(a, b), k
        else:          # the same terms in another order of fp64 atomics (tests/test_sample_batches.py)
            assert np.isfinite(b).all(), k
            a, b = a.astype(np.float64), b.astype(np.float64)
            n = np.linalg.norm(a)
            assert np.linalg.norm(a - b) <= 2e-6 * n + 1e-30, (k, np.linalg.norm(a - b) / max(n, 1e-300))


@pytest.mark.gpu
def test_pickh_leaves_walk_gpu(gpu_backend):
    """RDR_PICKH_LEAVES_WALK: the split hierarchical pick with its leaves stage as a walk with wave-local refill (render.cpp:
    pick_hierarchical; read once per process: a subprocess, with the session's large-frame forms, to which the split pick
    belongs).  The picks must not change: two fixtures with secondary edges at every depth, on the build under test."""
    import subprocess
    import sys
    from conftest import ROOT
    assert 'RDR_LARGE_FRAME_FORMS' in os.environ
    cmd = [sys.executable, '-m', 'pytest', '-q', '-x', '-m', 'gpu', os.path.join(ROOT, 'tests', 'test_backward_parity.py'), '-k',
           'test_backward_gpu and (bunny_box_32x32x4 or glossy_floor_blocker_48x48x4)']
    env = dict(os.environ, RDR_PICKH_LEAVES_WALK='1', RDR_TEST_LIBM='exact' if libm_exact() else 'default')
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-1000:]
    assert '2 passed' in r.stdout and 'failed' not in r.stdout, r.stdout[-500:]


def _gather_overflow(budget, caps, lib, dev, cases):
    """The NEE-mode gather hands work over in three ways -- subtrees to SecEdgeGatherSub when a lane's pop budget is spent,
    candidates to the 256-entry lists when a slot has more than 8, and the slot to the reference-order walk when even those
    lists (or the heavy / work registries) are full.  Tiny budgets and registry sizes force every one of them; the picks
    must not change (bit-identical fixtures).  Run in a subprocess: the switches are read once per process."""
    import subprocess
    import sys
    from conftest import ROOT
    code = r'''
import os, sys
sys.path[:0] = [%r, %r + '/tests']
import numpy as np, torch
from redner_amd import _capi
_capi.load(%r)
from redner_amd import redner
from golden.make_golden import CASES, render_case
from parity_util import GOLD, assert_parity, compare
for name in %r:
    rep = compare(render_case(redner, *CASES[name], device=torch.device(%r)), np.load(os.path.join(GOLD, name + '.npz')))
    assert_parity(rep, name)
    assert sum(e['flipped_rows'] for e in rep.values()) == 0, name
''' % (ROOT, ROOT, lib, cases, dev)
    env = dict(os.environ, RDR_GATHER_BUDGET=budget)
    if caps is not None:
        env['RDR_GATHER_CAPS'] = caps
    subprocess.check_call([sys.executable, '-c', code], env=env, timeout=900)


@pytest.mark.parametrize('budget,caps', [('4', None), ('2', '3,5'), ('1', '0,0'), ('6', '100000,2')])
def test_gather_overflow_paths_hostsim(budget, caps, tmp_path):
    from conftest import HOSTSIM_LIB
    _gather_overflow(budget, caps, HOSTSIM_LIB, 'cpu', ('bunny_box_32x32x4', 'bunny_box_96x96x8', 'envmap_sphere_48x48x4'))


@pytest.mark.gpu
@pytest.mark.parametrize('budget,caps', [('2', '3,5'), ('1', '0,0')])
def test_gather_overflow_paths_gpu(gpu_backend, budget, caps, tmp_path):
    """The same hand-over paths on the GPU build (subtree hand-off across lanes, the 256-entry lists, the fallback walk)."""
    from redner_amd import _capi
    _gather_overflow(budget, caps, _capi.library_path(), 'cuda:0', ('bunny_box_32x32x4', 'bunny_box_96x96x8'))
