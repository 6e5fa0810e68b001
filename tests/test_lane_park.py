"""The lane park (csrc/lane_park.h: RDR_PARK_DECL / rdr::LanePark): per-lane state of a stage body kept outside the registers
across a stretch of the body that needs them -- in LDS columns on the GPU, entry k of lane t at [k * 256 + t], in a local array
on the CPU harness.

1. The primitive alone, through rdr_debug_lane_park: one stage whose inactive lanes return before the park is declared and whose
   active lanes park K doubles (K: the widest park a shipped stage declares) through every typed form -- double, V3, V2,
   double[4], `+=` on six of the columns -- and fetch them back in the opposite order.  Every double that comes back must be
   the double that went in (x + x / 2 on the six: one correctly rounded operation, the same in numpy), bit for bit, and an
   inactive lane's output must be untouched: a lane that read a neighbour's column, or a column of its own under another
   index, shows.  Lane counts around the wave (64) and the workgroup (256); masks all / none / alternating / one wave only.
2. Renders whose lane counts leave partial waves and partial workgroups in the stages that park (BounceContrib, AdjBounceNee),
   large-frame forms, one worker: each GPU build against the CPU harness on the same call -- image bit for bit, gradients to
   parity_util's bars."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from golden.make_golden import render_case
from parity_util import assert_parity, compare
from redner_amd import _capi as K

LANES = [1, 63, 64, 65, 255, 256, 257, 1000]
MASKS = ['all', 'none', 'alternating', 'one_wave']
SENTINEL = -12345.678


def _mask(kind, n):
    act = np.ones(n, np.uint8)
    if kind == 'none':
        act[:] = 0
    elif kind == 'alternating':
        act[1::2] = 0
    elif kind == 'one_wave':                 # the second wave of every workgroup (the first where there is no second)
        lane = np.arange(n)
        act = (((lane % 256) // 64) == (1 if n > 64 else 0)).astype(np.uint8)
    return act


def _park_round_trip(n, kind):
    lib = K.lib()
    cols = ctypes.c_int32(0)
    assert lib.rdr_debug_lane_park(0, None, None, None, ctypes.byref(cols)) == 0, K.last_error()
    k = cols.value
    assert 22 <= k <= 26              # 26 doubles per lane: what three workgroups per CU leave of the LDS
    rng = np.random.default_rng(1000 * n + MASKS.index(kind))
    # every double distinct, all magnitudes, both signs; no two lanes and no two columns share a value
    x = rng.standard_normal((n, k)) * np.exp2(rng.integers(-40, 40, (n, k)).astype(np.float64))
    x += (np.arange(n * k).reshape(n, k) + 1) * 2.0 ** -30
    act = _mask(kind, n)
    out = np.full((n, k), SENTINEL)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.rdr_debug_lane_park(n, p(act), p(x), p(out), ctypes.byref(cols)) == 0, K.last_error()
    assert cols.value == k
    want = x.copy()
    want[:, 10:16] = x[:, 10:16] + 0.5 * x[:, 10:16]
    want[act == 0] = SENTINEL
    assert np.array_equal(out, want), np.argwhere(out != want)[:8]


@pytest.mark.parametrize('kind', MASKS)
@pytest.mark.parametrize('n', LANES)
def test_park_round_trip_hostsim(hostsim_backend, n, kind):
    _park_round_trip(n, kind)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', MASKS)
@pytest.mark.parametrize('n', LANES)
def test_park_round_trip_gpu(gpu_backend, n, kind):
    _park_round_trip(n, kind)


def test_probe_rejects_bad_arguments(hostsim_backend):
    lib = K.lib()
    cols = ctypes.c_int32(0)
    assert lib.rdr_debug_lane_park(-1, None, None, None, ctypes.byref(cols)) == 1
    assert 'rdr_debug_lane_park' in K.last_error()
    assert lib.rdr_debug_lane_park(4, None, None, None, ctypes.byref(cols)) == 1
    assert lib.rdr_debug_lane_park(0, None, None, None, None) == 1


# ---- renders with partial waves / partial workgroups -------------------------------------------------------------------------------
# name -> (scene builder, (rows, columns), samples, bounces): 15 lanes; one 45-lane batch; 272 lanes (a workgroup and a quarter
# wave); the glossy floor (secondary edges at every depth) at 35 lanes x 2 samples
RENDERS = {
    'bunny_box_5x3x1': ('bunny_box', (3, 5), 1, 4),
    'bunny_box_5x3x3': ('bunny_box', (3, 5), 3, 4),
    'bunny_box_17x16x1': ('bunny_box', (16, 17), 1, 4),
    'glossy_floor_blocker_7x5x2': ('glossy_floor_blocker', (5, 7), 2, 2),
}
FIELDS = {'workers': 1, 'flags': K.TUNE_LARGE_FORMS}
_harness = {}


def _render(backend, name, device):
    b, res, spp, mb = RENDERS[name]
    return render_case(backend, b, res, spp, mb, None, {'tuning': dict(FIELDS)}, device=device)


def _harness_render(name):
    """The same call on the CPU harness, once per session; the library that was loaded is loaded again afterwards."""
    if name not in _harness:
        from conftest import HOSTSIM_LIB, ROOT
        from redner_amd import redner
        subprocess.check_call(['make', '-C', os.path.join(ROOT, 'tests', 'hostsim'), '-j8'], stdout=subprocess.DEVNULL)
        before = K.library_path()
        K.load(HOSTSIM_LIB)
        try:
            for n in RENDERS:
                _harness[n] = _render(redner, n, torch.device('cpu'))
        finally:
            if before:
                K.load(before)
    return _harness[name]


@pytest.mark.parametrize('name', list(RENDERS))
def test_partial_wave_renders_hostsim(hostsim_backend, name):
    """The harness runs the same stage source through its own LanePark: finite, and the same twice."""
    a = _harness_render(name)
    b = _render(hostsim_backend, name, torch.device('cpu'))
    assert a.keys() == b.keys() and len(a) > 1
    for k in a:
        assert np.isfinite(a[k]).all(), k
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(RENDERS))
def test_partial_wave_renders_gpu(gpu_backend, name):
    want = _harness_render(name)
    assert K.is_product_library(), K.library_path()
    out = _render(gpu_backend, name, torch.device('cuda:0'))
    assert np.array_equal(out['image'], want['image'])
    assert_parity(compare(out, want), name)
