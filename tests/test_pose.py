"""gen_rotate_matrix / pose_vertices (redner_amd.transform on rdr_rotate_matrix* / rdr_pose_vertices*, csrc/pose.h) against
fixtures made by the reference's own gen_rotate_matrix and the expression its pose-estimation scripts write
(tests/golden/make_pose_golden.py), against an independent fp64 definition written here, bit for bit against the CPU harness,
and through RenderFunction and gaussian_pyramid_loss against the same render driven by the torch fp64 formulation of the pose.

Bars
  * fixtures and the fp64 definition: every tensor (R, every posed set, d_angles, d_translation, d_center, every d_vertices) at
    parity_util.TOL = 1e-4 relative L2 of the whole tensor through parity_util.compare / assert_parity; a tensor that is exactly
    zero in the reference is exactly zero here.  (The generator held the reference's own fp32 values to 5e-6 of fp64.)
  * bits: two runs are torch.equal in every output and gradient; every case's digest is the one the fixture records for the CPU
    harness, on the harness and on both GPU builds; a list call equals the sets posed one by one about the list's centre.
  * exact relations: zero angles give the identity; with zero translation and a centre of 0 the vertices' own bits come back;
    gen_rotate_matrix is the R pose_vertices used; d_translation of integer-valued upstream gradients is their exact column sum.
  * the adjoint identity, test_adjoint_identity_*: see its docstring.
The harness cases run the same per-vertex and per-chunk bodies as the kernels, as plain loops; the GPU cases run on both builds."""
import os

import numpy as np
import pytest
import torch

import parity_util
from golden import make_pose_golden as mp
from redner_amd import gen_rotate_matrix, pose_vertices, PoseVertices, RotateMatrix

CPU, GPU = torch.device('cpu'), torch.device('cuda:0')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the fp64 definition ---------------------------------------------------------------------------------------------------------
def _rotation64(a):
    """R = Rz(psi) (Ry(phi) Rx(theta)) from three fp64 plane rotations, signs as in the reference"""
    one, zero = torch.ones((), dtype=torch.float64), torch.zeros((), dtype=torch.float64)
    st, ct, sp, cp, ss, cs = a[0].sin(), a[0].cos(), a[1].sin(), a[1].cos(), a[2].sin(), a[2].cos()
    rx = torch.stack([torch.stack([one, zero, zero]), torch.stack([zero, ct, st]), torch.stack([zero, -st, ct])])
    ry = torch.stack([torch.stack([cp, zero, -sp]), torch.stack([zero, one, zero]), torch.stack([sp, zero, cp])])
    rz = torch.stack([torch.stack([cs, -ss, zero]), torch.stack([ss, cs, zero]), torch.stack([zero, zero, one])])
    return rz @ (ry @ rx)


def _definition(sets, upstream, angles, own, translation=mp.TRANSLATION, center=mp.CENTER):
    """fp64 on the CPU by torch autograd; upstream[k] None = that output is not used"""
    a = torch.tensor(angles, dtype=torch.float64, requires_grad=True)
    t = torch.tensor(translation, dtype=torch.float64, requires_grad=True)
    vs = [v.double().clone().requires_grad_(True) for v in sets]
    given = None if own else torch.tensor(center, dtype=torch.float64, requires_grad=True)
    R = _rotation64(a)
    c = torch.cat(vs).mean(0) if own else given
    outs = [(v - c) @ R.t() + c + t for v in vs]
    sum((o * u.double()).sum() for o, u in zip(outs, upstream) if u is not None).backward()
    res = {'R': R.detach().numpy(), 'd_angles': a.grad.numpy(), 'd_translation': t.grad.numpy()}
    if not own:
        res['d_center'] = given.grad.numpy()
    for k, (o, v) in enumerate(zip(outs, vs)):
        res['out%d' % k] = o.detach().numpy()
        res['d_vertices%d' % k] = (v.grad if v.grad is not None else torch.zeros_like(v)).numpy()
    return res


def _hold(out, want, tag):
    rep = parity_util.compare(out, want)
    print('%s: worst rel-L2 %.3e' % (tag, parity_util.summary(rep)['worst_rel_l2']))
    parity_util.assert_parity(rep, tag)
    for name, value in want.items():
        if not np.any(value):
            assert not np.any(out[name]), (tag, name, 'exactly zero in the reference')


def _fixture(case):
    gold = dict(np.load(mp.fixture_path(case)))
    assert abs(mp.inputs_sum(case) - float(gold.pop('inputs_sum'))) < 1e-9, 'the regenerated inputs are not the fixture\'s'
    return gold


_RUNS = {}


def _run_case(backend, device, case, tag):
    """{pose key: run_native()} of a fixture case, computed once per library"""
    key = (tag, case)
    if key not in _RUNS:
        sets, ups = mp.sets_of(case), mp.upstream_of(case)
        _RUNS[key] = {k: mp.run_native(backend, device, sets, ups, angles, own) for k, angles, own in mp.poses(case)}
    return _RUNS[key]


def _tag(backend, device):
    return 'hostsim' if device.type == 'cpu' else 'gpu-%s' % ('exact' if parity_util.libm_exact() else 'default')


# ---- 9. the public names --------------------------------------------------------------------------------------------------------
def test_public_names():
    import redner_amd
    from redner_amd import transform
    for name in ('gen_rotate_matrix', 'pose_vertices', 'RotateMatrix', 'PoseVertices'):
        assert getattr(redner_amd, name) is getattr(transform, name)
    assert issubclass(RotateMatrix, torch.autograd.Function) and issubclass(PoseVertices, torch.autograd.Function)


# ---- 1. against the reference's fixtures ----------------------------------------------------------------------------------------
def _run_fixture(backend, device, case):
    tag = _tag(backend, device)
    gold, runs = _fixture(case), _run_case(backend, device, case, tag)
    gold.pop('harness_sha256')
    out = {'%s_%s' % (key, name): value for key, res in runs.items() for name, value in res.items()}
    _hold(out, gold, '%s %s' % (tag, case))
    if case == 'vertex':
        for key, _, own in mp.poses(case):
            assert own == (not np.any(out[key + '_d_angles'])), key      # one vertex about itself does not move with the angles


@pytest.mark.parametrize('case', list(mp.CASES))
def test_fixture_hostsim(hostsim_backend, case):
    _run_fixture(hostsim_backend, CPU, case)


@pytest.mark.gpu
@pytest.mark.parametrize('case', list(mp.CASES))
def test_fixture_gpu(gpu_backend, case):
    _run_fixture(gpu_backend, GPU, case)


# ---- 2. against the fp64 definition -----------------------------------------------------------------------------------------------
def _run_definition(backend, device, case):
    tag = _tag(backend, device)
    sets, ups, runs = mp.sets_of(case), mp.upstream_of(case), _run_case(backend, device, case, tag)
    for key, angles, own in mp.poses(case):
        _hold(runs[key], _definition(sets, ups, angles, own), '%s %s %s' % (tag, case, key))


@pytest.mark.parametrize('case', list(mp.CASES))
def test_definition_hostsim(hostsim_backend, case):
    _run_definition(hostsim_backend, CPU, case)


@pytest.mark.gpu
@pytest.mark.parametrize('case', list(mp.CASES))
def test_definition_gpu(gpu_backend, case):
    _run_definition(gpu_backend, GPU, case)


def _run_switches(backend, device):
    """Both sides of every switch of the plan (mp.switch_sizes, through the plan query): against the fp64 definition, and bit
    for bit against what the fixture records for the harness -- at 65 537 vertices and beyond a workgroup owns several chunks,
    which no mesh of the fixtures reaches."""
    tag = _tag(backend, device)
    recorded = np.load(mp.SWITCH_PATH)
    all_sizes = mp.switch_sizes(backend)
    assert len(all_sizes) * 2 == len(recorded.files)
    for i, sizes in enumerate(all_sizes):
        assert recorded['sizes_%d' % i].tolist() == sizes, 'the plan has changed: regenerate tests/golden/pose_switches.npz'
        sets, ups = mp.switch_inputs(i, sizes)
        out, again = mp.run_switch(backend, device, i, sizes), mp.run_switch(backend, device, i, sizes)
        for key, angles, own in mp.SWITCH_POSES:
            assert all(out[key][k].tobytes() == again[key][k].tobytes() for k in out[key]), (sizes, key, 'two runs differ')
            _hold(out[key], _definition(sets, ups, angles, own), '%s sizes %s %s' % (tag, sizes, key))
        assert np.array_equal(mp.digest(out), recorded['harness_sha256_%d' % i]), (sizes, 'not the bits the harness computes')


def test_plan_switches_hostsim(hostsim_backend):
    _run_switches(hostsim_backend, CPU)


@pytest.mark.gpu
def test_plan_switches_gpu(gpu_backend):
    _run_switches(gpu_backend, GPU)


# ---- 3. bits --------------------------------------------------------------------------------------------------------------------
def _run_bitwise(backend, device, case):
    tag = _tag(backend, device)
    sets, ups, first = mp.sets_of(case), mp.upstream_of(case), _run_case(backend, device, case, tag)
    for key, angles, own in mp.poses(case):
        second = mp.run_native(backend, device, sets, ups, angles, own)
        for name in first[key]:
            assert first[key][name].tobytes() == second[name].tobytes(), (case, key, name, 'two runs differ')
    recorded = np.load(mp.fixture_path(case))['harness_sha256']
    assert np.array_equal(mp.digest(first), recorded), (case, 'not the bits the harness computes')


@pytest.mark.parametrize('case', list(mp.CASES))
def test_bitwise_hostsim(hostsim_backend, case):
    _run_bitwise(hostsim_backend, CPU, case)


@pytest.mark.gpu
@pytest.mark.parametrize('case', list(mp.CASES))
def test_bitwise_gpu(gpu_backend, case):
    """Both builds: chunks, lanes, trees and workgroups add in the harness's order, and sin / cos are the same routines."""
    _run_bitwise(gpu_backend, GPU, case)


def _run_list_equals_one_by_one(backend, device):
    case = 'sphere40x64_fan5_grid7x9'
    sets = [v.to(device) for v in mp.sets_of(case)]
    a, t = torch.tensor(mp.ANGLES[2], device=device, requires_grad=True), torch.tensor(mp.TRANSLATION, device=device)
    together = pose_vertices(sets, a, t, backend=backend)
    R, center = mp.constants(together)
    mean = torch.cat(sets).double().mean(0)
    assert float((center.double() - mean).abs().max()) <= 2.0 ** -24 * float(mean.abs().max())      # the fp64 mean, rounded once
    for v, both in zip(sets, together):
        alone = pose_vertices(v, a, t, center=center, backend=backend)
        assert isinstance(alone, torch.Tensor) and torch.equal(alone, both)
    as_tuple = pose_vertices(tuple(sets), a, t, backend=backend)
    assert isinstance(as_tuple, tuple) and all(torch.equal(x, y) for x, y in zip(as_tuple, together))
    assert torch.equal(R, gen_rotate_matrix(a, backend=backend))


def test_list_equals_one_by_one_hostsim(hostsim_backend):
    _run_list_equals_one_by_one(hostsim_backend, CPU)


@pytest.mark.gpu
def test_list_equals_one_by_one_gpu(gpu_backend):
    _run_list_equals_one_by_one(gpu_backend, GPU)


# ---- 4. exact relations ---------------------------------------------------------------------------------------------------------
def _run_exact_relations(backend, device):
    zero = torch.zeros(3, device=device)
    assert torch.equal(gen_rotate_matrix(zero, backend=backend), torch.eye(3, device=device))
    v = mp.sets_of('box9')[0].to(device)
    assert not (v == 0).any()
    out = pose_vertices(v, zero, zero, center=zero, backend=backend)
    assert out.data_ptr() != v.data_ptr() and torch.equal(out.view(torch.int32), v.view(torch.int32))
    for angles in mp.ANGLES:
        a = torch.tensor(angles, device=device, requires_grad=True)
        for center in (None, torch.tensor(mp.CENTER, device=device)):
            R, c = mp.constants(pose_vertices(v, a, zero, center=center, backend=backend))
            assert torch.equal(R, gen_rotate_matrix(a, backend=backend))
            assert center is None or torch.equal(c, center)
    # integer-valued upstream gradients: every order of summation gives the same column sums
    sizes = [backend.pose_plan([1])[0] * 2 + 3, 7]
    gen = torch.Generator().manual_seed(41)
    sets = [torch.randn(n, 3, generator=gen).to(device) for n in sizes]
    ups = [torch.randint(-8, 9, (n, 3), generator=gen).float() for n in sizes]
    for center in (None, torch.tensor(mp.CENTER, device=device)):
        t = torch.tensor(mp.TRANSLATION, device=device, requires_grad=True)
        outs = pose_vertices(sets, torch.tensor(mp.ANGLES[2], device=device), t, center=center, backend=backend)
        sum((o * u.to(device)).sum() for o, u in zip(outs, ups)).backward()
        want = sum(u.double().sum(0) for u in ups).float()
        assert torch.equal(t.grad.cpu(), want), (t.grad, want)


def test_exact_relations_hostsim(hostsim_backend):
    _run_exact_relations(hostsim_backend, CPU)


@pytest.mark.gpu
def test_exact_relations_gpu(gpu_backend):
    _run_exact_relations(gpu_backend, GPU)


def _run_rotate_matrix(backend, device):
    for i, angles in enumerate(mp.ANGLES):
        a = torch.tensor(angles, device=device, requires_grad=True)
        w = torch.randn(3, 3, generator=torch.Generator().manual_seed(60 + i))
        R = gen_rotate_matrix(a, backend=backend)
        assert R.shape == (3, 3) and R.dtype == torch.float32 and R.device == a.device
        (R * w.to(device)).sum().backward()
        a64 = torch.tensor(angles, dtype=torch.float64, requires_grad=True)
        R64 = _rotation64(a64)
        (R64 * w.double()).sum().backward()
        _hold({'R': R.detach().cpu().numpy(), 'd_angles': a.grad.cpu().numpy()}, {'R': R64.detach().numpy(), 'd_angles': a64.grad.numpy()},
              '%s rotate %s' % (_tag(backend, device), angles))
        b = torch.tensor(angles, device=device, requires_grad=True)
        (gen_rotate_matrix(b, backend=backend) * w.to(device)).sum().backward()
        assert torch.equal(a.grad, b.grad)


def test_rotate_matrix_hostsim(hostsim_backend):
    _run_rotate_matrix(hostsim_backend, CPU)


@pytest.mark.gpu
def test_rotate_matrix_gpu(gpu_backend):
    _run_rotate_matrix(gpu_backend, GPU)


# ---- 5. the adjoint identity ----------------------------------------------------------------------------------------------------
ADJOINT_BAR = 1e-6


def _run_adjoint_identity(backend, device):
    """<J u, w> against <u, J^T w> in fp64 for x = (angles, translation, centre, vertices), J u from finite differences of the
    native forward pass and J^T w from the native backward pass, relative to |J u| |w|.

    Every coordinate of x is a multiple of 2^-12 and every coordinate of u a multiple of 1/8, so x +- h u is exact in fp32 for
    h = 2^-6 and 2^-7; the two central differences are combined (4 D(h / 2) - D(h)) / 3, which leaves a truncation error of
    h^4 |f^(5)| / 480 < 2e-10 in the angles (the pose is linear in everything else).  What remains is the rounding of the fp32
    forward pass, about 2^-24 |out| / h = 8e-6 per element of J u and of random sign, and the fp32 rounding of J^T w.
    Measured on the harness: own centre 1.6e-7, given centre 1.3e-7 (301 + 56 vertices).  The bar is 1e-6: the measured gap with
    a margin of 6, a hundredth of the 1e-4 that the other tests hold every gradient tensor to."""
    gen = torch.Generator().manual_seed(77)
    quant = (lambda x: torch.round(x * 4096.0) / 4096.0)
    sets = [quant(v) for v in mp.sets_of('fan300') + mp.sets_of('sphere6x8')]
    x0 = {'angles': quant(torch.tensor(mp.ANGLES[2])), 'translation': quant(torch.tensor(mp.TRANSLATION)),
          'center': quant(torch.tensor(mp.CENTER))}
    eighths = (lambda *shape: torch.randint(-8, 9, shape, generator=gen).float() / 8.0)
    u = {'angles': eighths(3), 'translation': eighths(3), 'center': eighths(3), 'sets': [eighths(*v.shape) for v in sets]}
    w = [torch.randn(*v.shape, generator=gen) for v in sets]
    gaps = {}
    for own in (True, False):
        def forward(h):
            moved = [(v + h * du).to(device) for v, du in zip(sets, u['sets'])]
            center = None if own else (x0['center'] + h * u['center']).to(device)
            outs = pose_vertices(moved, (x0['angles'] + h * u['angles']).to(device), (x0['translation'] + h * u['translation']).to(device),
                                 center=center, backend=backend)
            return torch.cat([o.double().cpu().reshape(-1) for o in outs])

        def central(h):
            return (forward(h) - forward(-h)) / (2.0 * h)

        ju = (4.0 * central(2.0 ** -7) - central(2.0 ** -6)) / 3.0
        wf = torch.cat([x.double().reshape(-1) for x in w])
        lhs = float((ju * wf).sum())
        a, t = x0['angles'].clone().to(device).requires_grad_(True), x0['translation'].clone().to(device).requires_grad_(True)
        c = None if own else x0['center'].clone().to(device).requires_grad_(True)
        vs = [v.clone().to(device).requires_grad_(True) for v in sets]
        outs = pose_vertices(vs, a, t, center=c, backend=backend)
        torch.autograd.backward(outs, [x.to(device) for x in w])
        rhs = float((a.grad.double().cpu() * u['angles'].double()).sum() + (t.grad.double().cpu() * u['translation'].double()).sum())
        rhs += sum(float((v.grad.double().cpu() * du.double()).sum()) for v, du in zip(vs, u['sets']))
        if not own:
            rhs += float((c.grad.double().cpu() * u['center'].double()).sum())
        scale = float(ju.norm() * wf.norm())
        gaps[own] = abs(lhs - rhs) / scale
        print('adjoint identity, own centre %s: %.12e vs %.12e, gap / scale %.3e' % (own, lhs, rhs, gaps[own]))
    assert all(g <= ADJOINT_BAR for g in gaps.values()), gaps


def test_adjoint_identity_hostsim(hostsim_backend):
    _run_adjoint_identity(hostsim_backend, CPU)


@pytest.mark.gpu
def test_adjoint_identity_gpu(gpu_backend):
    _run_adjoint_identity(gpu_backend, GPU)


# ---- 6. gradient plumbing -------------------------------------------------------------------------------------------------------
def _run_plumbing(backend, device):
    tag = _tag(backend, device)
    sets, ups = mp.sets_of('box4_sphere6x8'), mp.upstream_of('box4_sphere6x8')
    angles = mp.ANGLES[2]

    def native(own, used, scale=1.0, angles_on=device, vertex_grads=(True, True)):
        a = torch.tensor(angles, device=angles_on, requires_grad=True)
        t = torch.tensor(mp.TRANSLATION, device=device, requires_grad=True)
        c = None if own else torch.tensor(mp.CENTER, device=angles_on, requires_grad=True)
        vs = [v.clone().to(device).requires_grad_(wanted) for v, wanted in zip(sets, vertex_grads)]
        outs = pose_vertices(vs, a, t, center=c, backend=backend)
        (scale * sum((outs[k] * ups[k].to(device)).sum() for k in used)).backward()
        assert a.grad.device == a.device and t.grad.device == t.device and (c is None or c.grad.device == c.device)
        res = {'d_angles': a.grad.cpu().numpy(), 'd_translation': t.grad.cpu().numpy()}
        if c is not None:
            res['d_center'] = c.grad.cpu().numpy()
        for k, v in enumerate(vs):
            assert (v.grad is not None) == vertex_grads[k]
            if v.grad is not None:
                res['d_vertices%d' % k] = v.grad.cpu().numpy()
        return res

    def want(own, used, scale=1.0):
        res = _definition(sets, [scale * ups[k] if k in used else None for k in range(2)], angles, own)
        return {k: v for k, v in res.items() if k.startswith('d_')}

    for own in (True, False):
        # only the second output is used downstream: the first counts as a zero gradient
        part = native(own, (1,))
        _hold(part, want(own, (1,)), '%s own %s, one output used' % (tag, own))
        # ... so its vertices get the centre's share and nothing else: one row repeated, which is zero for a given centre
        rows = part['d_vertices0']
        assert (rows == rows[0]).all() and bool(rows.any()) == own
        # a non-unit upstream gradient: autograd hands 3 * upstream to the op, which is what a call with that upstream computes
        whole, tripled = native(own, (0, 1)), native(own, (0, 1), scale=3.0)
        _hold(tripled, want(own, (0, 1), 3.0), '%s own %s, upstream times 3' % (tag, own))
        assert not np.array_equal(whole['d_angles'], tripled['d_angles'])
        # angles (and a given centre) on the CPU with the vertices on the device: the same bits, gradients back on the CPU
        moved = native(own, (0, 1), angles_on=CPU)
        assert all(np.array_equal(whole[k], moved[k]) for k in whole)
        # only one set asks for a gradient, none does: the others' and the small gradients keep their bits
        for vertex_grads in ((False, True), (False, False)):
            some = native(own, (0, 1), vertex_grads=vertex_grads)
            assert all(np.array_equal(whole[k], some[k]) for k in some) and ('d_vertices1' in some) == vertex_grads[1]
    # the centre term is in d_vertices under the sets' own centre and absent under a given one
    own_rows, given_rows = native(True, (0, 1))['d_vertices0'], native(False, (0, 1))['d_vertices0']
    shift = own_rows.astype(np.float64) - given_rows.astype(np.float64)
    assert np.abs(shift).max() > 0 and np.abs(shift - shift.mean(0)).max() <= 2.0 ** -22 * np.abs(given_rows).max()


def test_gradient_plumbing_hostsim(hostsim_backend):
    _run_plumbing(hostsim_backend, CPU)


@pytest.mark.gpu
def test_gradient_plumbing_gpu(gpu_backend):
    _run_plumbing(gpu_backend, GPU)


# ---- 7. errors ------------------------------------------------------------------------------------------------------------------
def _run_errors(backend, device):
    v, a, t = torch.zeros(5, 3, device=device), torch.zeros(3, device=device), torch.zeros(3, device=device)
    assert len(pose_vertices([v] * 16, a, t, backend=backend)) == 16
    bad_calls = [
        lambda: pose_vertices([v] * 17, a, t, backend=backend), lambda: pose_vertices([], a, t, backend=backend),
        lambda: pose_vertices(v.reshape(-1), a, t, backend=backend), lambda: pose_vertices(torch.zeros(5, 4, device=device), a, t, backend=backend),
        lambda: pose_vertices(v.double(), a, t, backend=backend), lambda: pose_vertices(v, a.double(), t, backend=backend),
        lambda: pose_vertices(v, a, t.double(), backend=backend), lambda: pose_vertices(v, a, t, center=t.double(), backend=backend),
        lambda: pose_vertices([v, torch.zeros(0, 3, device=device)], a, t, backend=backend),
        lambda: pose_vertices(v, torch.zeros(4, device=device), t, backend=backend), lambda: pose_vertices(v, a, torch.zeros(3, 1, device=device), backend=backend),
        lambda: pose_vertices(v, a, t, center=torch.zeros(2, device=device), backend=backend), lambda: pose_vertices('v', a, t, backend=backend),
        lambda: pose_vertices(v, [0.0, 0.0, 0.0], t, backend=backend),
        lambda: gen_rotate_matrix(torch.zeros(4, device=device), backend=backend), lambda: gen_rotate_matrix(a.double(), backend=backend),
        lambda: gen_rotate_matrix([0.0, 0.0, 0.0], backend=backend),
    ]
    if device.type == 'cuda':
        bad_calls += [lambda: pose_vertices([v, v.cpu()], a, t, backend=backend)]                 # mixed devices
    for i, call in enumerate(bad_calls):
        with pytest.raises(ValueError, match='^(pose_vertices|gen_rotate_matrix): '):
            call()
            print('call %d did not raise' % i)
    # the C calls, through rdr_last_error
    rd, use_gpu = backend, device.type == 'cuda'
    ptr = (lambda x: rd.float_ptr(x.data_ptr()))
    fwd, bwd = rd.pose_scratch([5, 600])
    assert fwd == 2 * 3 * 3 and bwd == 2 * 12 * 3
    for counts in ([], [1] * 17, [3, 0]):
        with pytest.raises(RuntimeError, match='rdr_pose_scratch'):
            rd.pose_scratch(counts)
        with pytest.raises(RuntimeError, match='rdr_pose_plan'):
            rd.pose_plan(counts)
    out, saved = torch.zeros_like(v), torch.zeros(12, device=device)
    scratch = torch.zeros(bwd, dtype=torch.float64, device=device)
    one = rd.pose_scratch([5])
    with pytest.raises(RuntimeError, match='required'):
        rd.pose_vertices([ptr(v)], [5], None, ptr(t), None, [ptr(out)], ptr(saved), ptr(scratch), one[0], use_gpu, 0)
    with pytest.raises(RuntimeError, match='required'):
        rd.pose_vertices([None], [5], ptr(a), ptr(t), None, [ptr(out)], ptr(saved), ptr(scratch), one[0], use_gpu, 0)
    with pytest.raises(RuntimeError, match='scratch of %d floats' % one[0]):
        rd.pose_vertices([ptr(v)], [5], ptr(a), ptr(t), None, [ptr(out)], ptr(saved), ptr(scratch), one[0] - 1, use_gpu, 0)
    with pytest.raises(RuntimeError, match='scratch of %d floats' % one[0]):
        rd.pose_vertices([ptr(v)], [5], ptr(a), ptr(t), None, [ptr(out)], ptr(saved), None, one[0], use_gpu, 0)
    rd.pose_vertices([ptr(v)], [5], ptr(a), ptr(t), ptr(t), [ptr(out)], ptr(saved), None, 0, use_gpu, 0)       # a given centre needs none
    grads = torch.zeros(9, device=device)
    back = (lambda **kw: rd.pose_vertices_backward(
        [ptr(v)], [5], kw.get('angles', ptr(a)), kw.get('saved', ptr(saved)), kw.get('own', True), [None], None, ptr(grads[0:3]),
        kw.get('d_translation', ptr(grads[3:6])), kw.get('d_center', None), ptr(scratch), kw.get('scratch_floats', one[1]), use_gpu, 0))
    for bad in (dict(angles=None), dict(saved=None), dict(d_translation=None), dict(own=False)):
        with pytest.raises(RuntimeError, match='required'):
            back(**bad)
    with pytest.raises(RuntimeError, match='scratch of %d floats' % one[1]):
        back(scratch_floats=one[1] - 1)
    back()
    with pytest.raises(RuntimeError, match='required'):
        rd.rotate_matrix(None, ptr(saved), use_gpu, 0)
    with pytest.raises(RuntimeError, match='required'):
        rd.rotate_matrix_backward(ptr(a), None, ptr(grads), use_gpu, 0)
    if use_gpu:
        torch.cuda.synchronize()
    assert not grads.any() and torch.equal(saved[:9].reshape(3, 3), torch.eye(3, device=device))


def test_errors_hostsim(hostsim_backend):
    _run_errors(hostsim_backend, CPU)


@pytest.mark.gpu
def test_errors_gpu(gpu_backend):
    _run_errors(gpu_backend, GPU)
    # no torch fall-back and no silent CPU path: CPU tensors are for the harness library only
    with pytest.raises(RuntimeError, match='pose_vertices.*harness'):
        pose_vertices(torch.zeros(5, 3), torch.zeros(3), torch.zeros(3), backend=gpu_backend)
    with pytest.raises(RuntimeError, match='gen_rotate_matrix.*harness'):
        gen_rotate_matrix(torch.zeros(3), backend=gpu_backend)


# ---- 10. end to end: the pose, a render, the loss, the gradients of angles and translation ------------------------------------------
@pytest.mark.gpu
def test_end_to_end_gpu(gpu_backend):
    """single_triangle at 64 x 64 and 4 spp: its vertices posed natively from angles and translation, through RenderFunction and
    gaussian_pyramid_loss with three levels against a fixed target, backward; against a second render whose vertex gradient is
    pushed through the torch fp64 formulation of the pose on the CPU (no pose arithmetic runs on the device in that leg; it
    renders the first leg's posed vertices, so both legs draw the same samples)."""
    import scenes
    from redner_amd import gaussian_pyramid_loss
    from redner_amd.render_pytorch import RenderFunction

    def render(vertices):
        sc = scenes.single_triangle(GPU, resolution=(64, 64))
        sc.shapes[0].vertices = vertices
        args = RenderFunction.serialize_scene(sc, 4, 1, sampler_type=gpu_backend.SamplerType.sobol, device=GPU)
        return RenderFunction.apply(1, *args)

    yy, xx = torch.meshgrid(torch.arange(64, dtype=torch.float32), torch.arange(64, dtype=torch.float32), indexing='ij')
    target = torch.stack([0.5 + 0.3 * torch.sin(0.21 * xx), 0.4 + 0.2 * torch.cos(0.17 * yy), 0.3 + 0.1 * torch.sin(0.13 * (xx + yy))], dim=2)
    v0 = scenes.single_triangle(GPU, resolution=(64, 64)).shapes[0].vertices.detach()
    a = torch.tensor([0.1, -0.1, 0.1], requires_grad=True)                                       # on the CPU, like the scripts' parameters
    t = torch.tensor([0.1, 0.2, 0.1], device=GPU, requires_grad=True)
    posed = pose_vertices(v0, a, t, backend=gpu_backend)
    loss = gaussian_pyramid_loss(render(posed), target.to(GPU), 3, backend=gpu_backend)
    loss.backward()
    leaf = posed.detach().clone().requires_grad_(True)
    loss2 = gaussian_pyramid_loss(render(leaf), target.to(GPU), 3, backend=gpu_backend)
    loss2.backward()
    want = _definition([v0.cpu()], [leaf.grad.cpu()], (0.1, -0.1, 0.1), True, translation=(0.1, 0.2, 0.1))
    out = {'d_angles': a.grad.numpy(), 'd_translation': t.grad.cpu().numpy()}
    assert float(loss.detach()) == float(loss2.detach()) and np.linalg.norm(want['d_angles']) > 0 and np.linalg.norm(want['d_translation']) > 0
    assert float((posed.detach().cpu().double() - torch.from_numpy(want['out0'])).norm()) < parity_util.TOL * np.linalg.norm(want['out0'])
    _hold(out, {k: want[k] for k in out}, 'end to end')
