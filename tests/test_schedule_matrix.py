"""Every render schedule crossed with every kernel kind, compared with the DEFAULT schedule of the same build.

render() picks its kernels from the scene's kind (render.cpp: scene_kind -> lean / mid / general, the PCG sampler, chain mode
under mip levels or an environment light, the replay of stale hit positions) and from the schedule (rdr_tuning).  with_kind /
with_walk_kind instantiate one kernel per (stage, kind) pair, and adj_scatter, hoist_first_vertex_picks and start_picks branch
on the scene as well -- so a schedule that is right on a lean scene says little about the mid or the general form of the same
stage.  tests/test_tuning.py runs the schedules on two lean fixtures against the oracle's fixture at 1e-4 per tensor; here
every schedule runs on one scene of every kind and is compared with the default schedule's output:

* CPU harness (sequential, one sample worker): EVERY tensor bit for bit.  A schedule changes which launches carry a term,
  never the term nor -- on one thread -- the order of the additions.  One exception is written down (REPLAY_BAR), as in
  tests/test_sample_batches.py: it is applied only where bitwise equality in fact fails, and printed with its value.
* GPU, both builds: the image bit for bit (fp32 sums in the reference's order); every gradient to GPU_BAR = 2e-6 relative L2,
  the bar tests/test_sample_batches.py uses for "the same terms in another order of fp64 atomics".  Every pair's worst figure
  goes to $RDR_PARITY_REPORT.

The tables are not copied: schedules from tests/test_tuning.py, cases from tests/golden/make_golden.py.  MATRIX names what
each case is expected to be; the test checks that against the scene itself and against what the library reports about the
render (rdr_debug_counters: samples per launch set, workers).  A schedule that cannot take effect on a case -- ragged batches
on a scene that is not batched -- is still rendered and still has to agree, but it is reported as "not applicable" and is not
counted among the pairs that exercise something (test_matrix_is_complete prints the table)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import scenes
from golden.make_golden import CASES, render_case
from parity_util import GOLD, assert_parity, compare, record
from redner_amd import _capi as K
from test_tuning import GPU_ONLY, SCHEDULES

GPU_BAR = 2e-6           # tests/test_sample_batches.py: test_batches_equal_single_samples_gpu (+ its 1e-30 floor)
REPLAY_BAR = 1e-6        # tests/test_sample_batches.py: REPLAYED, harness

# case -> what it is expected to be.  kind: the stage specialisation (render.cpp: scene_kind); chain: chain mode (mip levels or
# an environment light, with an edge estimator on); batched: the gradient render puts several samples into one launch set
# under the default schedule; env_edges: environment light AND edge sampling (stale hit positions are replayed).
MATRIX = {
    'bunny_box_32x32x4':                         dict(kind='lean', chain=False, batched=True, env_edges=False, what='lean, diffuse'),
    'glossy_floor_blocker_48x48x4':              dict(kind='lean', chain=False, batched=True, env_edges=False, what='lean, glossy'),
    'living_room_standin_40x40x2':               dict(kind='mid', chain=True, batched=True, env_edges=False, what='mid: mip-mapped textures, chain mode'),
    'misc_features_viewport_40x56x4':            dict(kind='mid', chain=True, batched=True, env_edges=False,
                                                      what='viewport, samples at pixel centres, two lights, separate uv / normal indices'),
    'two_triangles_ortho_64x64x4':               dict(kind='general', chain=False, batched=True, env_edges=False, what='general by camera: orthographic'),
    'bunny_box_fisheye_32x32x4':                 dict(kind='general', chain=False, batched=True, env_edges=False, what='general by camera: fisheye'),
    'textured_sphere_ids_radiance_last_48x48x3': dict(kind='general', chain=True, batched=True, env_edges=False,
                                                      what='general by channels: ids, radiance last'),
    'living_room_standin_envmap_32x32x2':        dict(kind='general', chain=True, batched=True, env_edges=True,
                                                      what='general by environment light, with area lights'),
    'envmap_sphere_48x48x4':                     dict(kind='general', chain=True, batched=True, env_edges=True,
                                                      what='general by environment light, no area light'),
    'envmap_convex_48x48x4':                     dict(kind='general', chain=True, batched=True, env_edges=True,
                                                      what='environment light, path depths without live lanes'),
    'bunny_box_pcg_32x32x3':                     dict(kind='lean', chain=False, batched=False, env_edges=False, what='lean, PCG sampler (stateful: not batched)'),
}

# Schedules that act through the batch size or the number of workers: whether they took effect is OBSERVED (the counters of the
# render differ from the default schedule's), not assumed.
SHAPES_BATCHES = ('one_sample_per_launch', 'ragged_batches', 'lane_cap', 'little_memory', 'one_worker', 'three_workers')
# Schedules that act on one kind only (render.cpp: fuse_bounces and run_bounce's emitter_test are for lean scenes with the
# stateless sampler / lean scenes; FORCE_GENERAL changes nothing where the kind is general already).
NEEDS = {
    'unfused_bounce': lambda t, case: t['kind'] == 'lean' and t['batched'],
    'trace_every_continuation': lambda t, case: t['kind'] == 'lean',
    'general_kernels': lambda t, case: t['kind'] != 'general',
}

NOT_APPLICABLE = {}      # (leg, schedule, case) -> why; filled while the pairs run, printed by test_matrix_is_complete
EXCEPTIONS = {}          # (schedule, case, tensor) -> measured relative L2 of a harness pair held to REPLAY_BAR
_DEFAULT = {}            # (library, case) -> (outputs, counters) of the default schedule: rendered once per case and build


def _counters():
    c = K.DebugCounters()
    K.lib().rdr_debug_counters_get(ctypes.byref(c))
    return int(c.last_batch_samples), int(c.last_workers)


def _render(backend, device, case, fields):
    b, res, spp, mb = CASES[case][:4]
    channels = CASES[case][4] if len(CASES[case]) > 4 else None
    opts = dict(CASES[case][5] if len(CASES[case]) > 5 else {})
    opts['tuning'] = fields
    out = render_case(backend, b, res, spp, mb, channels, opts, device=device)
    return {k: np.asarray(v) for k, v in out.items()}, _counters()


def _traits(case):
    """What the scene itself says about its kind (the conditions of render.cpp: scene_is_lean / scene_kind / `chain`)."""
    b, res = CASES[case][:2]
    channels = CASES[case][4] if len(CASES[case]) > 4 else None
    opts = CASES[case][5] if len(CASES[case]) > 5 else {}
    sc = getattr(scenes, b)(torch.device('cpu'), resolution=res if isinstance(res, tuple) else (res, res))
    env = getattr(sc, 'envmap', None) is not None
    plain_camera = sc.camera.camera_type == 0 and sc.camera.distortion_params is None
    radiance_only = channels is None or list(channels) == ['radiance']
    texs = [t for m in sc.materials for t in (m.diffuse_reflectance, m.specular_reflectance, m.roughness, m.generic_texture, m.normal_map)
            if t is not None]
    mips = any(len(t.mipmap) > 1 for t in texs) or (env and len(sc.envmap.values.mipmap) > 1)
    textured = any(t.mipmap[0].dim() == 3 for t in texs) or any(m.normal_map is not None for m in sc.materials)
    colors = any(getattr(s, 'colors', None) is not None for s in sc.shapes)
    if not env and plain_camera and radiance_only and not mips and not textured and not colors:
        kind = 'lean'
    elif not env and plain_camera and radiance_only:
        kind = 'mid'
    else:
        kind = 'general'
    edges = opts.get('use_primary_edge_sampling', True) or opts.get('use_secondary_edge_sampling', True)
    return dict(kind=kind, chain=bool((mips or env) and edges), env_edges=bool(env and edges),
                sobol=opts.get('sampler', 'sobol') == 'sobol')


def _default(backend, device, case, fields, leg):
    key = (K.library_path(), case)
    if key not in _DEFAULT:
        t, seen = MATRIX[case], _traits(case)
        assert (t['kind'], t['chain'], t['env_edges']) == (seen['kind'], seen['chain'], seen['env_edges']), (case, t, seen)
        out, (S, workers) = _render(backend, device, case, fields)
        spp = CASES[case][2]
        # what the library reports about the render it has just made
        assert (S > 1) == t['batched'], (case, 'samples per launch set', S)
        assert t['batched'] == seen['sobol'], (case, t, seen)
        if t['batched']:
            assert S == min(spp, 16), (case, S)          # these frames are far below 2^17 lanes: all samples in one set
        if t['chain'] or not t['batched']:
            assert workers == 1, (case, workers)         # the scratch chain / the sampler's state runs through the samples in order
        for k, v in out.items():
            assert np.isfinite(v).all(), (case, k)
        _DEFAULT[key] = (out, (S, workers))
    return _DEFAULT[key]


def _applicable(leg, name, case, fields, got, base):
    """-> None, or why the schedule cannot have changed this render."""
    t = MATRIX[case]
    if name in SHAPES_BATCHES and got == base:
        return 'same samples per launch set and workers as the default schedule %s' % (base,)
    if name in NEEDS and not NEEDS[name](t, case):
        return 'acts on another kind than %s%s' % (t['kind'], '' if t['batched'] else ' (PCG sampler)')
    return None


def _rel(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float(np.linalg.norm(a - b)), float(np.linalg.norm(a))


def _check_schedule_took(name, case, fields, got, base):
    """Where the effect of a schedule on the launch plan is known, it must be what the counters report."""
    S, workers = got
    if not MATRIX[case]['batched']:
        assert S == 1, (name, case, got)
        return
    spp = CASES[case][2]
    if 'batch_samples' in fields:
        assert S == min(fields['batch_samples'], spp), (name, case, got)
    if name == 'one_sample_per_launch':
        assert got != base, (name, case, got, base)      # a batched case: this schedule always applies
    if 'batch_lanes' in fields:
        assert S <= max(1, fields['batch_lanes'] // _pixels(case)), (name, case, got)


def _pixels(case):
    b, res = CASES[case][:2]
    sc = getattr(scenes, b)(torch.device('cpu'), resolution=res if isinstance(res, tuple) else (res, res))
    vp = getattr(sc.camera, 'viewport', None)
    if vp is not None:
        return (vp[2] - vp[0]) * (vp[3] - vp[1])
    h, w = sc.camera.resolution
    return h * w


HARNESS_PAIRS = [(s, c) for s in SCHEDULES if s != 'default' for c in MATRIX]
GPU_PAIRS = [(s, c) for s in list(SCHEDULES) + list(GPU_ONLY) if s != 'default' for c in MATRIX]


@pytest.mark.parametrize('case', list(MATRIX))
def test_default_schedule_against_fixture_hostsim(hostsim_backend, case):
    """The value every pair below is compared with is itself held to the oracle's fixture (as tests/test_tuning.py: _check)."""
    out, _ = _default(hostsim_backend, torch.device('cpu'), case, {'workers': 1}, 'hostsim')
    gold = np.load(os.path.join(GOLD, case + '.npz'))
    assert np.array_equal(out['image'], gold['image'])
    assert_parity(compare(out, gold), case)


@pytest.mark.parametrize('name,case', HARNESS_PAIRS)
def test_schedule_equals_default_hostsim(hostsim_backend, name, case):
    dev = torch.device('cpu')
    base_out, base = _default(hostsim_backend, dev, case, {'workers': 1}, 'hostsim')
    fields = dict(SCHEDULES[name])
    fields.setdefault('workers', 1)
    out, got = _render(hostsim_backend, dev, case, fields)
    _check_schedule_took(name, case, fields, got, base)
    why = _applicable('hostsim', name, case, fields, got, base)
    if why:
        NOT_APPLICABLE[('hostsim', name, case)] = why
    assert set(out) == set(base_out)
    for k in out:
        if np.array_equal(out[k], base_out[k]):
            continue
        # the one exception (tests/test_sample_batches.py: REPLAYED): another batching of an environment-lit scene with edge
        # sampling replays the stale hit positions in another order of fp64 additions
        d, n = _rel(out[k], base_out[k])
        if k != 'image' and MATRIX[case]['env_edges'] and name in SHAPES_BATCHES and got != base:
            EXCEPTIONS[(name, case, k)] = d / max(n, 1e-300)
            print('replayed pair %s x %s: %s differs by %.3e (bar %.0e)' % (name, case, k, d / max(n, 1e-300), REPLAY_BAR))
            assert d <= REPLAY_BAR * n, (name, case, k, d / max(n, 1e-300))
            continue
        assert False, (name, case, k, 'not bit for bit the default schedule\'s: relative L2 %.3e, largest difference %.3e'
                       % (d / max(n, 1e-300), float(np.abs(out[k].astype(np.float64) - base_out[k].astype(np.float64)).max())))


@pytest.mark.gpu
@pytest.mark.parametrize('name,case', GPU_PAIRS)
def test_schedule_equals_default_gpu(gpu_backend, name, case):
    dev = torch.device('cuda:0')
    leg = 'gpu-exact' if K.lib().rdr_libm_exact() else 'gpu-default-build'
    base_out, base = _default(gpu_backend, dev, case, {}, leg)
    fields = dict(SCHEDULES.get(name, GPU_ONLY.get(name)))
    out, got = _render(gpu_backend, dev, case, fields)
    _check_schedule_took(name, case, fields, got, base)
    if 'workers' in fields and MATRIX[case]['batched'] and not MATRIX[case]['chain']:
        assert got[1] == min(fields['workers'], -(-CASES[case][2] // got[0])), (name, case, got)
    why = _applicable(leg, name, case, fields, got, base)
    if why:
        NOT_APPLICABLE[(leg, name, case)] = why
    assert set(out) == set(base_out)
    rep, late = {}, []
    for k in out:
        assert np.isfinite(out[k]).all(), (name, case, k)
        if k == 'image':
            assert np.array_equal(out[k], base_out[k]), (name, case, 'image is not bit for bit the default schedule\'s')
            continue
        d, n = _rel(out[k], base_out[k])
        rep[k] = {'rel_l2': d / n if n > 0 else d, 'tol': GPU_BAR, 'flipped_rows': 0, **({'zero_reference': True} if n == 0 else {})}
        if not d <= GPU_BAR * n + 1e-30:
            late.append((k, rep[k]['rel_l2']))
    record('schedule_matrix %s x %s%s' % (name, case, ' (not applicable: %s)' % why if why else ''), rep, leg + '-vs-default-schedule')
    assert not late, (name, case, late)


def test_matrix_is_complete():
    """>= 20 schedules x >= 11 cases, every kind present; prints which pairs could not exercise their schedule."""
    assert len(SCHEDULES) - 1 >= 20 and len(MATRIX) >= 11
    kinds = {(t['kind'], t['chain'], t['batched'], t['env_edges']) for t in MATRIX.values()}
    for needed in (('lean', False, True, False), ('mid', True, True, False), ('general', False, True, False), ('general', True, True, False),
                   ('general', True, True, True), ('lean', False, False, False)):
        assert needed in kinds, needed
    assert set(MATRIX) <= set(CASES)
    print('schedule matrix: %d + %d GPU-only schedules x %d cases' % (len(SCHEDULES) - 1, len(GPU_ONLY), len(MATRIX)))
    for (leg, name, case), why in sorted(NOT_APPLICABLE.items()):
        print('  not applicable [%s] %s x %s: %s' % (leg, name, case, why))
    for (name, case, k), e in sorted(EXCEPTIONS.items()):
        print('  held to %.0e instead of bit for bit: %s x %s, %s: %.3e' % (REPLAY_BAR, name, case, k, e))
