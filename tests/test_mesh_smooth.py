"""redner_amd.smooth, mesh_laplacian and bound_vertices (redner_amd.shape on rdr_mesh_boundary / rdr_mesh_laplacian /
rdr_mesh_laplacian_backward / rdr_mesh_smooth) against fixtures made by the reference's own pyredner.smooth and
pyredner.bound_vertices (tests/golden/make_smooth_golden.py), against an independent fp64 definition written here, and against
the exact relations between the three functions.

Bars
  * fixtures and the fp64 definition: parity_util.TOL = 1e-4 relative L2 of every whole tensor (shift, the displacement of
    smooth, d_vertices).  The reference's own fp32 sits 4e-8 ... 4.3e-6 from an fp64 evaluation on these meshes (the generator
    asserts 5e-6); a wrong weight, sign or row entry is off by 1e-2 or more.
  * bound_vertices: torch.equal with the fixture and with an integer formula written here.
  * the degenerate mesh: the same bar on the rows where the reference is finite, which must be exactly the sets the generator
    recorded; against the definition (whose degenerate corners and vertices are masked out BEFORE any division, so its autograd
    is finite) on every row, forward and gradient.
  * exact relations: torch.equal, or equal bit patterns where "unchanged" is the claim.
The meshes are those of make_mesh_golden.py (the smallest at which the code can go wrong: rows of 1 to 300 corners, V not a
multiple of the workgroup, more than one workgroup, open and closed, degenerate faces) and collapsed_box().

What "a vertex with W == 0 has a zero gradient" means here.  Such a vertex has shift 0 and passes NOTHING BACK THROUGH ITS OWN
SHIFT: with an upstream gradient that is nonzero on those vertices only, d_vertices is exactly 0 everywhere.  Its row of
d_vertices under a dense upstream gradient need not be 0: on the degenerate mesh vertex 6 has W == 0 under 'reciprocal' and
'uniform', and the shift of vertex 7 (= p6 - p7, from the one live corner of face [6, 6, 7]) depends on p6.  That row is held to
the definition like every other, and is exactly 0 wherever the definition's is.

The harness cases run the same per-item bodies as the kernels, as plain loops; the GPU cases run on both builds of the library."""
import ctypes
import os

import numpy as np
import pytest
import torch

import parity_util
from golden import make_mesh_golden as mg
from golden import make_smooth_golden as msg

GOLD = parity_util.GOLD
CPU, GPU = torch.device('cpu'), torch.device('cuda:0')
SCHEMES, CONTROLS = msg.SCHEMES, msg.CONTROLS
REGULAR = [name for name in mg.MESHES if name != 'degenerate']                    # the seven meshes without degenerate faces
FIXTURE_CASES = [(name, scheme) for name in mg.MESHES for scheme in SCHEMES]
FIXTURE_IDS = ['%s-%s' % c for c in FIXTURE_CASES]
DEFINITION_MESHES = list(mg.MESHES) + ['collapsed_box']
DEFINITION_CASES = [(name, scheme, which) for name in DEFINITION_MESHES for scheme in SCHEMES for which in (0, 1, 2)]
DEFINITION_IDS = ['%s-%s-w%d' % c for c in DEFINITION_CASES]
EXACT_MESHES = ('grid7x9', 'fan300', 'box9', 'sphere40x64')
LMD = 0.3                                                                        # (not an fp32 number)


def _shape_module():
    from redner_amd import shape
    return shape


def _mesh(name):
    if name == 'collapsed_box':
        vertices, indices, _ = mg.collapsed_box()
        return vertices, indices
    return mg.mesh(name)


def _gold(name):
    gold = dict(np.load(os.path.join(GOLD, 'smooth_%s.npz' % name)))
    vertices, indices = mg.mesh(name)
    want = float(gold['vertices_sum'])
    assert abs(mg.checksum(vertices) - want) <= 1e-12 * abs(want), 'the regenerated mesh is not the fixture\'s'
    assert mg.checksum(indices) == float(gold['indices_sum'])
    return gold


def _check(name, out, gold, tag):
    rep = parity_util.compare(out, gold)
    print(name, tag, {k: '%.2e' % e['rel_l2'] for k, e in rep.items()})
    parity_util.record(name, rep, tag)
    parity_util.assert_parity(rep, name)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _fixture_control(ctl, num_vertices, device):
    return None if ctl == 'default' else torch.ones(num_vertices, device=device)


def _displacement(before, after):
    """what the generator recorded: the fp64 difference of the two fp32 tensors"""
    return (after.detach().cpu().double() - before.detach().cpu().double()).numpy()


# ---- 1. fixtures ----------------------------------------------------------------------------------------------------------------
def _run_fixture_case(backend, device, name, scheme, tag):
    sm = _shape_module()
    gold = _gold(name)
    vertices, indices = mg.mesh(name)
    x, idx = vertices.to(device), indices.to(device)
    topology = sm.MeshTopology(idx, len(vertices), backend=backend)
    out, want = {}, {}
    for ctl in CONTROLS:
        key = '%s_%s' % (scheme, ctl)
        control = _fixture_control(ctl, len(vertices), device)
        shift = sm.mesh_laplacian(x, idx, scheme, control, topology=topology)
        assert shift.dtype == torch.float32 and shift.is_contiguous() and shift.device == x.device
        assert tuple(shift.shape) == tuple(vertices.shape) and bool(torch.isfinite(shift).all())
        moved = x.clone()
        assert sm.smooth(moved, idx, 0.5, scheme, control, topology=topology) is None
        got = {'shift_' + key: shift.cpu().double().numpy(), 'half_' + key: _displacement(x, moved)}
        for k, mine in got.items():
            rows = slice(None)
            if name == 'degenerate':
                # the bar holds where the reference has a value, and that is exactly where the generator found it
                rows = msg.finite_rows(gold[k])
                assert rows == msg.DEGENERATE_FINITE[scheme], (k, rows)
            else:
                assert np.isfinite(gold[k]).all(), k
            out[k], want[k] = mine[rows], gold[k][rows]
    _check('smooth_%s_%s' % (name, scheme), out, want, tag)


@pytest.mark.parametrize('name,scheme', FIXTURE_CASES, ids=FIXTURE_IDS)
def test_fixture_hostsim(hostsim_backend, name, scheme):
    _run_fixture_case(hostsim_backend, CPU, name, scheme, 'hostsim')


@pytest.mark.gpu
@pytest.mark.parametrize('name,scheme', FIXTURE_CASES, ids=FIXTURE_IDS)
def test_fixture_gpu(gpu_backend, name, scheme):
    _run_fixture_case(gpu_backend, GPU, name, scheme, 'gpu')


def _integer_bound(indices, num_vertices):
    """bound_vertices in integers: 1 where the signed sum of the opposite edges' index differences is 0"""
    idx = indices.long()
    total = torch.zeros(num_vertices, dtype=torch.int64)
    for k in range(3):
        total.index_add_(0, idx[:, k], idx[:, (k + 2) % 3] - idx[:, (k + 1) % 3])
    return (total == 0).float()


def _run_bound(backend, device, name):
    sm = _shape_module()
    vertices, indices = mg.mesh(name)
    bound = sm.bound_vertices(vertices.to(device), indices.to(device), backend=backend)
    assert bound.dtype == torch.float32 and tuple(bound.shape) == (len(vertices),) and bound.device == vertices.to(device).device
    assert torch.equal(bound.cpu(), torch.from_numpy(_gold(name)['bound']))
    assert torch.equal(bound.cpu(), _integer_bound(indices, len(vertices)))
    if name == 'degenerate':
        assert bound.cpu().tolist() == msg.DEGENERATE_BOUND
    else:
        assert int(bound.sum()) == msg.INTERIOR[name]


@pytest.mark.parametrize('name', list(mg.MESHES))
def test_bound_vertices_hostsim(hostsim_backend, name):
    _run_bound(hostsim_backend, CPU, name)


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(mg.MESHES))
def test_bound_vertices_gpu(gpu_backend, name):
    _run_bound(gpu_backend, GPU, name)


# ---- 2. an independent definition in fp64 ---------------------------------------------------------------------------------------
def _safe_sqrt(sq):
    """(sqrt(sq) where sq > 0 else 0, the mask), with a finite gradient everywhere"""
    live = sq > 0
    return torch.sqrt(torch.where(live, sq, torch.ones_like(sq))) * live, live


def _definition(v, idx, scheme, control):
    """The meaning of csrc/mesh_smooth.h in torch double -> (shift, W): angles by atan2(|a x b|, a . b), sums by index_add,
    every corner that adds nothing and every vertex that does not move masked out before the division it would spoil.  A
    'cotangent' corner of a zero-area face whose sides point in opposite directions is spread (its angle is pi and its cot a
    huge finite number, as in the reference) and, as csrc/vertex_normal.h specifies for a corner with |e1 x e2| == 0, enters as
    a constant: its gradient is 0."""
    def cross(a, b):
        # products rounded one by one (see test_vertex_normal._definition): the cross product of two EQUAL vectors must be 0
        return torch.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                            a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], dim=1)

    p = [v[idx[:, k]] for k in range(3)]
    C, W = torch.zeros_like(v), torch.zeros(v.shape[0], dtype=v.dtype)
    for k in range(3):
        p0, p1, p2 = p[k], p[(k + 1) % 3], p[(k + 2) % 3]
        e1, e2 = p1 - p0, p2 - p0
        l1, live1 = _safe_sqrt((e1 * e1).sum(1))
        l2, live2 = _safe_sqrt((e2 * e2).sum(1))
        live = live1 & live2
        one, zero = torch.ones_like(l1), torch.zeros_like(l1)
        s1, s2 = torch.where(live, l1, one), torch.where(live, l2, one)
        a, b = e1 / s1[:, None], e2 / s2[:, None]
        if scheme == 'reciprocal':
            C = C.index_add(0, idx[:, k], (a + b) * live[:, None])
            W = W.index_add(0, idx[:, k], torch.where(live, 1.0 / s1 + 1.0 / s2, zero))
        elif scheme == 'uniform':
            C = C.index_add(0, idx[:, k], (e1 + e2) * live[:, None])
            W = W.index_add(0, idx[:, k], torch.where(live, 2.0 * one, zero))
        else:
            c_len, has_area = _safe_sqrt((cross(a, b) ** 2).sum(1))
            cos = (a * b).sum(1)
            spread = live & (has_area | (cos < 0))
            angle = torch.atan2(torch.where(has_area, c_len, zero), torch.where(spread, cos, one))
            cot = torch.where(spread, 1.0 / torch.tan(torch.where(spread, angle, one)), zero)
            w = (p2 - p1) * cot[:, None]
            flat = spread & ~has_area
            cot, w = torch.where(flat, cot.detach(), cot), torch.where(flat[:, None], w.detach(), w)
            C = C.index_add(0, idx[:, (k + 1) % 3], w).index_add(0, idx[:, (k + 2) % 3], -w)
            W = W.index_add(0, idx[:, (k + 1) % 3], cot).index_add(0, idx[:, (k + 2) % 3], cot)
    moves = W != 0
    shift = torch.where(moves[:, None], C / torch.where(moves, W, torch.ones_like(W))[:, None], torch.zeros_like(C))
    return shift * control[:, None], W


def _definition_control(name, which):
    """which = 0: the default (the boundary mask, in integers); 1: a seeded control in [0.25, 1]; 2: all ones"""
    vertices, indices = _mesh(name)
    if which == 0:
        return _integer_bound(indices, len(vertices))
    if which == 1:
        return torch.rand(len(vertices), generator=torch.Generator().manual_seed(700)) * 0.75 + 0.25
    return torch.ones(len(vertices))


_definition_cache = {}


def _definition_case(name, scheme, which):
    """Computed once per case and shared by the harness leg and the GPU legs of both builds."""
    key = (name, scheme, which)
    if key not in _definition_cache:
        vertices, indices = _mesh(name)
        x = vertices.double().requires_grad_(True)
        shift, W = _definition(x, indices.long(), scheme, _definition_control(name, which).double())
        grad, = torch.autograd.grad(shift, x, mg.upstream(len(vertices), which).double())
        assert bool(torch.isfinite(shift).all()) and bool(torch.isfinite(grad).all()), key
        _definition_cache[key] = (shift.detach().numpy(), grad.numpy(), (W.detach() == 0).nonzero().flatten().tolist())
    return _definition_cache[key]


def _native(backend, device, name, scheme, control, weights):
    """shift and the gradient of sum(shift * weights), from a fresh MeshTopology"""
    sm = _shape_module()
    vertices, indices = _mesh(name)
    x = vertices.clone().to(device).requires_grad_(True)
    topology = sm.MeshTopology(indices.to(device), len(vertices), backend=backend)
    shift = sm.mesh_laplacian(x, indices.to(device), scheme, None if control is None else control.to(device), topology=topology)
    (shift * weights.to(device)).sum().backward()
    return shift.detach().cpu(), x.grad.cpu()


def _run_definition_case(backend, device, name, scheme, which, tag):
    want_shift, want_grad, still = _definition_case(name, scheme, which)
    vertices, _ = _mesh(name)
    control = None if which == 0 else _definition_control(name, which)
    shift, grad = _native(backend, device, name, scheme, control, mg.upstream(len(vertices), which))
    assert bool(torch.isfinite(shift).all()) and bool(torch.isfinite(grad).all())
    _check('smooth_definition_%s_%s_w%d' % (name, scheme, which), {'shift': shift.numpy(), 'd_vertices': grad.numpy()},
           {'shift': want_shift, 'd_vertices': want_grad}, tag)
    if name in ('degenerate', 'collapsed_box'):
        # the vertices with W == 0 (module docstring)
        if name == 'degenerate':
            assert still == ([4, 6, 7] if scheme == 'cotangent' else [4, 6])
        assert bool((shift[still] == 0).all())
        exact = [i for i in still if not want_grad[i].any()]
        assert bool((grad[exact] == 0).all()) and (name != 'degenerate' or 4 in exact)
        only_still = torch.zeros(len(vertices), 3)
        only_still[still] = mg.upstream(len(vertices), 1)[still]
        _, through = _native(backend, device, name, scheme, control, only_still)
        assert bool((through == 0).all())


@pytest.mark.parametrize('name,scheme,which', DEFINITION_CASES, ids=DEFINITION_IDS)
def test_definition_hostsim(hostsim_backend, name, scheme, which):
    _run_definition_case(hostsim_backend, CPU, name, scheme, which, 'hostsim')


@pytest.mark.gpu
@pytest.mark.parametrize('name,scheme,which', DEFINITION_CASES, ids=DEFINITION_IDS)
def test_definition_gpu(gpu_backend, name, scheme, which):
    _run_definition_case(gpu_backend, GPU, name, scheme, which, 'gpu')


def test_definition_is_the_reference_on_fixtures():
    """The definition written here and the reference agree (on the reference's fixtures): the two yardsticks are one."""
    for name in REGULAR:
        gold = _gold(name)
        vertices, indices = mg.mesh(name)
        for scheme in SCHEMES:
            for ctl in CONTROLS:
                control = _integer_bound(indices, len(vertices)) if ctl == 'default' else torch.ones(len(vertices))
                shift, _ = _definition(vertices.double(), indices.long(), scheme, control.double())
                key = 'shift_%s_%s' % (scheme, ctl)
                parity_util.assert_parity(parity_util.compare({key: shift.numpy()}, {key: gold[key]}), name)


# ---- 3. exact relations ---------------------------------------------------------------------------------------------------------
def _run_exact(backend, device, name):
    sm = _shape_module()
    vertices, indices = mg.mesh(name)
    v, idx = vertices.to(device), indices.to(device)
    topology = sm.MeshTopology(idx, len(vertices), backend=backend)
    bound = sm.bound_vertices(v, idx, topology=topology)
    rim = (bound == 0).cpu()
    weights = mg.upstream(len(vertices), 1).to(device)
    for scheme in SCHEMES:
        # smooth(lmd) is v + mesh_laplacian(v) * fp32(lmd): two roundings
        for control in (None, torch.ones(len(vertices), device=device)):
            shift = sm.mesh_laplacian(v, idx, scheme, control, topology=topology)
            once = v.clone()
            sm.smooth(once, idx, LMD, scheme, control, topology=topology)
            assert torch.equal(once, v + shift * torch.tensor(LMD, dtype=torch.float32, device=device))
            lmd_tensor = v.clone()
            sm.smooth(lmd_tensor, idx, torch.tensor([LMD], device=device), scheme, control, topology=topology)
            assert torch.equal(lmd_tensor, once)
        assert not torch.equal(once, v)
        # iterations = 3 is three calls
        thrice, three = v.clone(), v.clone()
        for _ in range(3):
            sm.smooth(thrice, idx, LMD, scheme, topology=topology)
        sm.smooth(three, idx, LMD, scheme, topology=topology, iterations=3)
        assert torch.equal(_bits(three), _bits(thrice))
        # two runs of forward and backward
        runs = []
        for _ in range(2):
            x = v.clone().requires_grad_(True)
            s = sm.mesh_laplacian(x, idx, scheme, topology=topology)
            (s * weights).sum().backward()
            runs.append((s.detach(), x.grad))
        assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0])) and torch.equal(_bits(runs[0][1]), _bits(runs[1][1]))
        assert float(runs[0][1].abs().sum()) > 0
        # a control of zeros leaves every bit; the default control leaves the rim
        frozen = v.clone()
        sm.smooth(frozen, idx, LMD, scheme, torch.zeros(len(vertices), device=device), topology=topology, iterations=2)
        assert torch.equal(_bits(frozen), _bits(v))
        default = v.clone()
        sm.smooth(default, idx, LMD, scheme, topology=topology, iterations=2)
        assert torch.equal(_bits(default)[rim], _bits(v)[rim]) and int(rim.sum()) == len(vertices) - msg.INTERIOR[name]
        # (not every interior vertex moves: the cotangent weights reproduce a plane, so a box's planar vertices stay put)
        assert not torch.equal(default, v)
        # the C ABI in place: vertices_out = vertices_in
        rd, native = topology.rd, topology.native
        n_fwd = rd.mesh_smooth_scratch(native, sm.SMOOTH_SCHEMES[scheme])[0]
        here, scratch = v.clone(), torch.empty(max(n_fwd, 1), device=device)
        rd.mesh_smooth(native, sm.SMOOTH_SCHEMES[scheme], rd.float_ptr(here.data_ptr()), rd.float_ptr(bound.data_ptr()), LMD, 2,
                       rd.float_ptr(here.data_ptr()), rd.float_ptr(scratch.data_ptr()), n_fwd)
        assert torch.equal(_bits(here), _bits(default))


@pytest.mark.parametrize('name', EXACT_MESHES)
def test_exact_relations_hostsim(hostsim_backend, name):
    _run_exact(hostsim_backend, CPU, name)


@pytest.mark.gpu
@pytest.mark.parametrize('name', EXACT_MESHES)
def test_exact_relations_gpu(gpu_backend, name):
    _run_exact(gpu_backend, GPU, name)


def _run_in_place(backend, device):
    """smooth writes the tensor's own memory, moves its version on and leaves no autograd record; the default control and the
    plan come from the same cache as compute_vertex_normal's."""
    sm = _shape_module()
    vertices, indices = mg.mesh('grid7x9')
    idx = indices.to(device)
    leaf = vertices.clone().to(device).requires_grad_(True)
    address, version = leaf.data_ptr(), leaf._version
    sm._plans.clear()
    assert sm.smooth(leaf, idx, LMD, backend=backend) is None
    assert leaf.data_ptr() == address and leaf._version > version
    assert leaf.grad_fn is None and leaf.is_leaf and leaf.requires_grad and leaf.grad is None
    assert not torch.equal(leaf.detach().cpu(), vertices)
    assert len(sm._plans) == 1
    plan = next(iter(sm._plans.values()))[1]
    sm.compute_vertex_normal(leaf, idx, backend=backend)
    sm.mesh_laplacian(leaf, idx, backend=backend)
    sm.bound_vertices(leaf, idx, backend=backend)
    assert len(sm._plans) == 1 and next(iter(sm._plans.values()))[1] is plan
    sm._plans.clear()
    # a leaf that was smoothed still takes a gradient, through mesh_laplacian: the regulariser |L v|^2
    (sm.mesh_laplacian(leaf, idx, 'uniform', backend=backend) ** 2).sum().backward()
    assert bool(torch.isfinite(leaf.grad).all()) and float(leaf.grad.abs().sum()) > 0
    # a view that is not contiguous is written through
    wide = torch.zeros(len(vertices), 5, device=device)
    wide[:, 1:4] = vertices.to(device)
    dense = vertices.clone().to(device)
    sm.smooth(wide[:, 1:4], idx, LMD, 'cotangent', backend=backend)
    sm.smooth(dense, idx, LMD, 'cotangent', backend=backend)
    assert torch.equal(wide[:, 1:4], dense) and bool((wide[:, 0] == 0).all()) and bool((wide[:, 4] == 0).all())


def test_in_place_hostsim(hostsim_backend):
    _run_in_place(hostsim_backend, CPU)


@pytest.mark.gpu
def test_in_place_gpu(gpu_backend):
    _run_in_place(gpu_backend, GPU)


# ---- 4. errors ------------------------------------------------------------------------------------------------------------------
def _run_errors(backend, device, elsewhere):
    sm = _shape_module()
    vertices, indices = mg.mesh('fan5')
    v, idx = vertices.to(device), indices.to(device)
    topology = sm.MeshTopology(idx, len(vertices), backend=backend)
    before = v.clone()
    for call in (lambda **kw: sm.smooth(v, idx, LMD, topology=topology, **kw), lambda **kw: sm.mesh_laplacian(v, idx, topology=topology, **kw)):
        with pytest.raises(ValueError, match='Unknown weighting_scheme: max'):
            call(weighting_scheme='max')
        with pytest.raises(ValueError, match='Size of control tensor inconsistent with number of vertices'):
            call(control=torch.ones(len(vertices) + 1, device=device))
    for call in (lambda x: sm.smooth(x, idx, LMD, topology=topology), lambda x: sm.mesh_laplacian(x, idx, topology=topology),
                 lambda x: sm.bound_vertices(x, idx, topology=topology)):
        with pytest.raises(RuntimeError, match='the topology on'):
            call(elsewhere)
        with pytest.raises(RuntimeError, match='fp32'):
            call(v.double())
        with pytest.raises(RuntimeError, match=r'\[6, 3\]'):
            call(v[:4])
    with pytest.raises(ValueError, match='iterations'):
        sm.smooth(v, idx, LMD, topology=topology, iterations=0)
    assert torch.equal(v, before)
    # the C boundary says the same
    rd, native = topology.rd, topology.native
    n_fwd, n_bwd, n_saved = rd.mesh_smooth_scratch(native, 0)
    assert (n_fwd, n_bwd, n_saved) == (12 * len(indices), 9 * len(indices), 4 * len(vertices))
    out, scratch = torch.empty_like(v), torch.empty(n_fwd, device=device)
    args = (rd.float_ptr(v.data_ptr()), None, LMD)
    with pytest.raises(RuntimeError, match='iterations must be at least 1'):
        rd.mesh_smooth(native, 0, *args, 0, rd.float_ptr(out.data_ptr()), rd.float_ptr(scratch.data_ptr()), n_fwd)
    with pytest.raises(RuntimeError, match='unknown weighting scheme 3'):
        rd.mesh_smooth(native, 3, *args, 1, rd.float_ptr(out.data_ptr()), rd.float_ptr(scratch.data_ptr()), n_fwd)
    with pytest.raises(RuntimeError, match='scratch of %d floats' % n_fwd):
        rd.mesh_smooth(native, 0, *args, 1, rd.float_ptr(out.data_ptr()), rd.float_ptr(scratch.data_ptr()), n_fwd - 1)
    with pytest.raises(RuntimeError, match='unknown weighting scheme -1'):
        rd.mesh_smooth_scratch(native, -1)
    from redner_amd import _capi
    lib = _capi.lib()
    assert lib.rdr_mesh_smooth(None, 0, None, None, 0.5, 1, None, None, 0) == 1
    assert lib.rdr_last_error().decode() == 'rdr_mesh_smooth: a topology is required'
    assert lib.rdr_mesh_boundary(None, None) == 1 and lib.rdr_mesh_laplacian(None, 0, None, None, None, None, None, 0) == 1
    assert lib.rdr_mesh_laplacian_backward(None, 0, None, None, None, None, None, None, 0) == 1
    assert lib.rdr_mesh_smooth_scratch(None, 0, None, None, ctypes.byref(ctypes.c_int64(0))) == 1
    # control = NULL at the C boundary is all ones
    rd.mesh_smooth(native, 0, *args, 1, rd.float_ptr(out.data_ptr()), rd.float_ptr(scratch.data_ptr()), n_fwd)
    ones = v.clone()
    sm.smooth(ones, idx, LMD, control=torch.ones(len(vertices), device=device), topology=topology)
    assert torch.equal(out, ones)
    # no faces at all: nothing moves, every vertex is interior
    nothing = torch.zeros(0, 3, dtype=torch.int32, device=device)
    assert bool((sm.mesh_laplacian(v, nothing, backend=backend) == 0).all())
    assert bool((sm.bound_vertices(v, nothing, backend=backend) == 1).all())


def test_errors_hostsim(hostsim_backend):
    _run_errors(hostsim_backend, CPU, torch.empty(6, 3, device='meta'))


@pytest.mark.gpu
def test_errors_gpu(gpu_backend):
    _run_errors(gpu_backend, GPU, mg.mesh('fan5')[0])


@pytest.mark.gpu
def test_product_library_refuses_host_tensors_gpu(gpu_backend):
    """No torch fall-back and no silent CPU path: CPU tensors are for the harness library only."""
    vertices, indices = mg.mesh('fan5')
    with pytest.raises(RuntimeError, match='harness'):
        _shape_module().smooth(vertices, indices, LMD, backend=gpu_backend)


def test_exports(hostsim_backend):
    import redner_amd
    sm = _shape_module()
    vertices, indices = mg.mesh('fan5')
    assert redner_amd.smooth is sm.smooth and redner_amd.mesh_laplacian is sm.mesh_laplacian
    assert redner_amd.bound_vertices is sm.bound_vertices and redner_amd.MeshLaplacian is sm.MeshLaplacian
    assert redner_amd.bound_vertices(vertices, indices, backend=hostsim_backend).tolist() == [1.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert int(hostsim_backend.SmoothWeighting.cotangent) == sm.SMOOTH_SCHEMES['cotangent'] == 2
