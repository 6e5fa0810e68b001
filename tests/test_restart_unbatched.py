"""The restart of an environment-lit batched gradient render (render.cpp: RestartUnbatched, g_unbatchable).

Such a render records the reads of the reference's hit-position scratch that reach across the samples of a batch and replays
them after the sweep.  Should the list of recorded reads overflow, the call starts over with one sample per launch -- on the
claim that nothing of the abandoned attempt has reached the caller's tensors or survives in the library's accumulators -- and
scenes of that shape start unbatched from then on.  The list has one entry per edge-ray lane and does not overflow by itself;
rdr_tuning::stale_event_cap_plus1 = 1 gives it capacity 0, so the first recorded read overflows it.

In a subprocess: a restart stores the scene's shape key for the life of the process and would un-batch later tests of the
same fixture.  Bars: the restarted render equals the `batch_samples: 1` render bit for bit on the sequential harness, and to
2e-6 relative L2 per gradient tensor on the GPU (image bit for bit) -- the bar of tests/test_sample_batches.py for the same
terms in another order of fp64 atomics."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CODE = r'''
import ctypes, os, sys
sys.path[:0] = [%(root)r, %(root)r + '/tests']
import numpy as np, torch
from redner_amd import _capi
_capi.load(%(lib)r)
from redner_amd import redner
from golden.make_golden import CASES, render_case
from parity_util import GOLD, assert_parity, compare
dev = torch.device(%(dev)r)
exact = dev.type == 'cpu'
base = %(base)r


def render(name, **fields):
    b, res, spp, mb = CASES[name][:4]
    out = render_case(redner, b, res, spp, mb, None, {'tuning': dict(base, **fields)} if (base or fields) else None, device=dev)
    c = _capi.DebugCounters()
    _capi.lib().rdr_debug_counters_get(ctypes.byref(c))
    return {k: np.asarray(v) for k, v in out.items()}, int(c.last_batch_samples)


def same(a, b, what):
    assert set(a) == set(b), what
    worst = 0.0
    for k in a:
        assert np.isfinite(b[k]).all(), (what, k)
        if exact or k == 'image':
            assert np.array_equal(a[k], b[k]), (what, k, float(np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)).max()))
        else:
            x, y = a[k].astype(np.float64), b[k].astype(np.float64)
            n = np.linalg.norm(x)
            worst = max(worst, np.linalg.norm(x - y) / max(n, 1e-300))
            assert np.linalg.norm(x - y) <= 2e-6 * n + 1e-30, (what, k, np.linalg.norm(x - y) / max(n, 1e-300))
    print('%%s: worst relative L2 %%.3e' %% (what, worst))


CASE, OTHER = 'envmap_sphere_48x48x4', 'envmap_convex_48x48x4'
spp = CASES[CASE][2]
# the scene of another shape, before anything has restarted: batched
other_before, S = render(OTHER)
assert S == CASES[OTHER][2], S
one, S = render(CASE, batch_samples=1)
assert S == 1, S
_, S = render(CASE)
assert S == spp, ('the default schedule batches this scene', S)
# capacity 0: the first recorded stale read overflows the list.  That the render comes back UNBATCHED is also the proof that this
# scene records at least one such read (no event, no overflow, no restart).
restarted, S = render(CASE, stale_event_cap_plus1=1)
assert S == 1, ('no restart: the scene recorded no stale read', S)
same(one, restarted, 'restarted render against one sample per launch')
# the shape is remembered: the same scene starts unbatched, without the field
again, S = render(CASE)
assert S == 1, S
same(one, again, 'the same shape afterwards against one sample per launch')
# ... and a scene of another shape is batched as before, renders what it rendered before the restart, and is on its fixture
# (the bars of tests/test_backward_parity.py; on the sequential harness the image bit for bit as well -- the GPU's image of an
# environment-lit fixture is ~1e-7 off the oracle's in any process, profiles/r6_parity_report.jsonl, so there the test for
# left-over state is the comparison with the render before the restart)
other, S = render(OTHER)
assert S == CASES[OTHER][2], S
same(other_before, other, 'a scene of another shape, after the restart against before')
gold = np.load(os.path.join(GOLD, OTHER + '.npz'))
print('%%s image against its fixture: largest difference %%.3e' %% (OTHER, float(np.abs(other['image'].astype(np.float64) - gold['image']).max())))
if exact:
    assert np.array_equal(other['image'], gold['image'])
assert_parity(compare(other, gold), OTHER)
print('RESTART PATH OK')
'''


def _run(lib, dev, base):
    code = CODE % {'root': ROOT, 'lib': lib, 'dev': dev, 'base': base}
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ), capture_output=True, text=True, timeout=900)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and 'RESTART PATH OK' in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_restart_leaves_nothing_behind_hostsim(hostsim_backend):
    from conftest import HOSTSIM_LIB
    _run(HOSTSIM_LIB, 'cpu', {'workers': 1})


@pytest.mark.gpu
def test_restart_leaves_nothing_behind_gpu(gpu_backend):
    from redner_amd import _capi
    _run(_capi.library_path(), 'cuda:0', {})
