"""redner_amd.compute_vertex_normal (redner_amd.shape on rdr_mesh_topology_* / rdr_vertex_normal / rdr_vertex_normal_backward)
against fixtures made by the reference's own pyredner.compute_vertex_normal under torch autograd
(tests/golden/make_mesh_golden.py), against an independent fp64 definition written here, and through RenderFunction against the
oracle.

Bars
  * fixtures and the fp64 definition: parity_util.TOL = 1e-4 relative L2 of every whole tensor (normals, d_vertices, image).  The
    reference's own fp32 sits 2e-8 ... 1.3e-6 from its fp64 on these meshes; a wrong weight, sign, corner or a missing row entry
    is off by 1e-2 or more.
  * the degenerate mesh: the same bar for the forward pass and for the gradient against the definition (whose degenerate corners
    are masked out BEFORE any division, so its autograd is finite); (0, 0, 1) where specified; the gradient exactly 0 on the
    vertices that only degenerate faces touch.
  * the adjoint: native backward == autograd of the definition, same bar, under three upstream tensors (one nonzero on a single
    vertex).
  * reproducibility (GPU): two forward + backward runs are torch.equal.
  * the plan: rows read back == ascending corner ids per vertex, exactly.
The meshes are the smallest at which the code can still go wrong (make_mesh_golden.MESHES): both schemes with and without the
cotangent fallback, more than one workgroup, V not a multiple of 64, boundary rows of valence 1 - 3, a row longer than a wave
(and than the insertion-sort limit of the plan's row sort), degenerate faces.  'cotangent' runs on the closed meshes only: at an
open boundary the cotangent vector lies in the surface and the flip towards the 'max' normal is decided by rounding noise (the
reference's own fp32 and fp64 disagree there).
The harness cases run the same per-item bodies as the kernels, as plain loops; the GPU cases run on both builds of the library."""
import os

import numpy as np
import pytest
import torch

import parity_util
from golden import make_mesh_golden as mg

GOLD = parity_util.GOLD
CPU, GPU = torch.device('cpu'), torch.device('cuda:0')
CASES = [(name, scheme) for name, (_, _, schemes, _) in mg.MESHES.items() for scheme in schemes]
CASE_IDS = ['%s-%s' % c for c in CASES]
ADJOINT_CASES = [(name, scheme, which) for name, scheme in CASES for which in (1, 2)]       # (which = 0: with the forward bar)
ADJOINT_IDS = ['%s-%s-w%d' % c for c in ADJOINT_CASES]


def _shape_module():
    from redner_amd import shape
    return shape


def _check(name, out, gold, tag):
    rep = parity_util.compare(out, gold)
    print(name, tag, {k: '%.2e' % e['rel_l2'] for k, e in rep.items()})
    parity_util.record(name, rep, tag)
    parity_util.assert_parity(rep, name)


def _native(backend, device, name, scheme, weights):
    """normals and the gradient of sum(normals * weights), from a fresh MeshTopology."""
    sm = _shape_module()
    vertices, indices = mg.mesh(name)
    x = vertices.to(device).requires_grad_(True)
    topology = sm.MeshTopology(indices.to(device), len(vertices), backend=backend)
    normals = sm.compute_vertex_normal(x, indices.to(device), scheme, topology=topology)
    assert normals.dtype == torch.float32 and normals.is_contiguous() and normals.device == x.device
    assert tuple(normals.shape) == tuple(vertices.shape)
    (normals * weights.to(device)).sum().backward()
    return normals.detach().cpu(), x.grad.cpu()


# ---- 1. fixtures ----------------------------------------------------------------------------------------------------------------
def _assert_checksums(vertices, indices, gold):
    want = float(gold['vertices_sum'])
    assert abs(mg.checksum(vertices) - want) <= 1e-12 * abs(want), 'the regenerated mesh is not the fixture\'s'
    assert mg.checksum(indices) == float(gold['indices_sum'])


def _run_fixture_case(backend, device, name, scheme, tag):
    gold = dict(np.load(os.path.join(GOLD, 'vertex_normal_%s.npz' % name)))
    vertices, indices = mg.mesh(name)
    _assert_checksums(vertices, indices, gold)
    normals, grad = _native(backend, device, name, scheme, mg.upstream(len(vertices), 0))
    if scheme == 'cotangent':
        # both branches of the cotangent choice stay covered: exactly the planar vertices take the 'max' normal, bit for bit
        plain, _ = _native(backend, device, name, 'max', mg.upstream(len(vertices), 0))
        assert int((normals == plain).all(dim=1).sum()) == mg.COTANGENT_FALLBACKS[name]
    out, want = {'normals': normals.numpy()}, {'normals': gold['normals_' + scheme]}
    if mg.MESHES[name][3]:
        out['d_vertices'], want['d_vertices'] = grad.numpy(), gold['d_vertices_' + scheme]
    _check('vertex_normal_%s_%s' % (name, scheme), out, want, tag)


@pytest.mark.parametrize('name,scheme', CASES, ids=CASE_IDS)
def test_fixture_hostsim(hostsim_backend, name, scheme):
    _run_fixture_case(hostsim_backend, CPU, name, scheme, 'hostsim')


@pytest.mark.gpu
@pytest.mark.parametrize('name,scheme', CASES, ids=CASE_IDS)
def test_fixture_gpu(gpu_backend, name, scheme):
    _run_fixture_case(gpu_backend, GPU, name, scheme, 'gpu')


# ---- 2. an independent definition in fp64 ---------------------------------------------------------------------------------------
def _safe_sqrt(sq):
    """(sqrt(sq) where sq > 0 else 0, the mask), with a finite gradient everywhere"""
    live = sq > 0
    return torch.sqrt(torch.where(live, sq, torch.ones_like(sq))) * live, live


def _definition(v, idx, scheme):
    """The meaning of csrc/vertex_normal.h in torch double: angles by atan2(|a x b|, a . b), sums by index_add, every degenerate
    corner, face and vertex masked out before the division it would spoil."""
    def cross(a, b):
        # products rounded one by one: torch.linalg.cross fuses a multiply-add, and the cross product of two EQUAL vectors is
        # then rounding residue (1e-17) instead of 0 -- a coincident-sides corner would pass for a spread one with cot = 1e16
        return torch.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                            a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], dim=1)

    num_vertices = v.shape[0]
    p = [v[idx[:, k]] for k in range(3)]
    sum_max, sum_cot = torch.zeros_like(v), torch.zeros_like(v)
    normal = None
    for k in range(3):
        p0, p1, p2 = p[k], p[(k + 1) % 3], p[(k + 2) % 3]
        e1, e2 = p1 - p0, p2 - p0
        l1, live1 = _safe_sqrt((e1 * e1).sum(1))
        l2, live2 = _safe_sqrt((e2 * e2).sum(1))
        live = live1 & live2
        one = torch.ones_like(l1)
        a, b = e1 / torch.where(live, l1, one)[:, None], e2 / torch.where(live, l2, one)[:, None]
        c = cross(a, b)
        c_len, spread = _safe_sqrt((c * c).sum(1))
        spread = spread & live
        if k == 0:
            normal = c / torch.where(spread, c_len, one)[:, None] * spread[:, None]
        # a . b is +-1 where the sides are parallel
        angle = torch.where(spread, torch.atan2(torch.where(spread, c_len, one), (a * b).sum(1)), torch.zeros_like(c_len))
        weight = torch.where(live, torch.sin(angle) / torch.where(live, l1 * l2, one), torch.zeros_like(l1))
        sum_max = sum_max.index_add(0, idx[:, k], normal * weight[:, None])
        if scheme == 'cotangent':
            cot = torch.where(spread, 1.0 / torch.tan(torch.where(spread, angle, one)), torch.zeros_like(angle))
            w = (p2 - p1) * cot[:, None]
            sum_cot = sum_cot.index_add(0, idx[:, (k + 1) % 3], w).index_add(0, idx[:, (k + 2) % 3], -w)
    up = torch.zeros(num_vertices, 3, dtype=v.dtype, device=v.device)
    up[:, 2] = 1.0
    length, live = _safe_sqrt((sum_max * sum_max).sum(1))
    n_max = torch.where(live[:, None], sum_max / torch.where(live, length, torch.ones_like(length))[:, None], up)
    if scheme == 'max':
        return n_max
    s = torch.where(((sum_cot * n_max).sum(1) > 0)[:, None], sum_cot, -sum_cot)
    length, _ = _safe_sqrt((s * s).sum(1))
    kept = length > 0.05
    return torch.where(kept[:, None], s / torch.where(kept, length, torch.ones_like(length))[:, None], n_max)


_definition_cache = {}


def _definition_case(name, scheme, which):
    """Computed once per case and shared by the harness leg and the GPU legs of both builds."""
    key = (name, scheme, which)
    if key not in _definition_cache:
        vertices, indices = mg.mesh(name)
        x = vertices.double().requires_grad_(True)
        normals = _definition(x, indices.long(), scheme)
        grad, = torch.autograd.grad(normals, x, mg.upstream(len(vertices), which).double())
        assert bool(torch.isfinite(normals).all()) and bool(torch.isfinite(grad).all()), key
        _definition_cache[key] = (normals.detach().numpy(), grad.numpy())
    return _definition_cache[key]


def _run_definition_case(backend, device, name, scheme, which, tag):
    want_normals, want_grad = _definition_case(name, scheme, which)
    vertices, _ = mg.mesh(name)
    normals, grad = _native(backend, device, name, scheme, mg.upstream(len(vertices), which))
    assert bool(torch.isfinite(grad).all())
    _check('vertex_normal_definition_%s_%s_w%d' % (name, scheme, which), {'normals': normals.numpy(), 'd_vertices': grad.numpy()},
           {'normals': want_normals, 'd_vertices': want_grad}, tag)
    if name == 'degenerate':
        rows = mg.DEGENERATE_DEFAULT_NORMAL
        assert torch.equal(normals[rows], torch.tensor([[0.0, 0.0, 1.0]] * len(rows)))
        assert bool((grad[rows] == 0).all()) and bool((torch.from_numpy(want_grad)[rows] == 0).all())
        assert float(grad[:4].abs().sum()) > 0


@pytest.mark.parametrize('name,scheme', CASES, ids=CASE_IDS)
def test_definition_hostsim(hostsim_backend, name, scheme):
    _run_definition_case(hostsim_backend, CPU, name, scheme, 0, 'hostsim')


@pytest.mark.gpu
@pytest.mark.parametrize('name,scheme', CASES, ids=CASE_IDS)
def test_definition_gpu(gpu_backend, name, scheme):
    _run_definition_case(gpu_backend, GPU, name, scheme, 0, 'gpu')


def test_definition_is_the_reference_on_fixtures():
    """The definition written here and the reference agree (on the reference's fixtures): the two yardsticks are one."""
    for name, scheme in CASES:
        gold = np.load(os.path.join(GOLD, 'vertex_normal_%s.npz' % name))
        want_normals, want_grad = _definition_case(name, scheme, 0)
        out, want = {'normals': want_normals.astype(np.float32)}, {'normals': gold['normals_' + scheme]}
        if mg.MESHES[name][3]:
            out['d_vertices'], want['d_vertices'] = want_grad.astype(np.float32), gold['d_vertices_' + scheme]
        parity_util.assert_parity(parity_util.compare(out, want), name + scheme)


def _run_collapsed_edge(backend, device, tag):
    """The degenerate rule under BOTH schemes on a closed mesh (box4 with an edge collapsed: corners with a zero-length side, and
    with coincident sides): the forward pass and the gradient against the definition at the usual bar, the gradient finite."""
    sm = _shape_module()
    vertices, indices, (a, b) = mg.collapsed_box()
    assert torch.equal(vertices[a], vertices[b])
    weights = mg.upstream(len(vertices), 1)
    for scheme in ('max', 'cotangent'):
        x64 = vertices.double().requires_grad_(True)
        want = _definition(x64, indices.long(), scheme)
        want_grad, = torch.autograd.grad(want, x64, weights.double())
        assert bool(torch.isfinite(want).all()) and bool(torch.isfinite(want_grad).all())
        x = vertices.clone().to(device).requires_grad_(True)
        normals = sm.compute_vertex_normal(x, indices.to(device), scheme, backend=backend)
        (normals * weights.to(device)).sum().backward()
        assert bool(torch.isfinite(normals).all()) and bool(torch.isfinite(x.grad).all())
        _check('vertex_normal_collapsed_edge_' + scheme, {'normals': normals.detach().cpu().numpy(), 'd_vertices': x.grad.cpu().numpy()},
               {'normals': want.detach().numpy(), 'd_vertices': want_grad.numpy()}, tag)


def test_collapsed_edge_hostsim(hostsim_backend):
    _run_collapsed_edge(hostsim_backend, CPU, 'hostsim')


@pytest.mark.gpu
def test_collapsed_edge_gpu(gpu_backend):
    _run_collapsed_edge(gpu_backend, GPU, 'gpu')


# ---- 3. the adjoint under other upstream gradients ------------------------------------------------------------------------------
@pytest.mark.parametrize('name,scheme,which', ADJOINT_CASES, ids=ADJOINT_IDS)
def test_adjoint_hostsim(hostsim_backend, name, scheme, which):
    _run_definition_case(hostsim_backend, CPU, name, scheme, which, 'hostsim')


@pytest.mark.gpu
@pytest.mark.parametrize('name,scheme,which', ADJOINT_CASES, ids=ADJOINT_IDS)
def test_adjoint_gpu(gpu_backend, name, scheme, which):
    _run_definition_case(gpu_backend, GPU, name, scheme, which, 'gpu')


# ---- 4. bitwise reproducible ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('name,scheme', [('fan300', 'max'), ('sphere40x64', 'max'), ('box9', 'cotangent')])
def test_bitwise_reproducible_gpu(gpu_backend, name, scheme):
    weights = mg.upstream(mg.SIZES[name][0], 1)
    first = _native(gpu_backend, GPU, name, scheme, weights)
    second = _native(gpu_backend, GPU, name, scheme, weights)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])


def test_harness_runs_are_equal(hostsim_backend):
    weights = mg.upstream(mg.SIZES['box4'][0], 1)
    first = _native(hostsim_backend, CPU, 'box4', 'cotangent', weights)
    second = _native(hostsim_backend, CPU, 'box4', 'cotangent', weights)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])


# ---- 5. the plan ----------------------------------------------------------------------------------------------------------------
def _canonical_rows(indices, num_vertices):
    flat = indices.reshape(-1).tolist()
    rows = [[] for _ in range(num_vertices)]
    for c, v in enumerate(flat):
        rows[v].append(c)
    offsets = [0]
    for r in rows:
        offsets.append(offsets[-1] + len(r))
    return offsets, [c for r in rows for c in r]


def _run_plan_rows(backend, device):
    sm = _shape_module()
    for name in ('degenerate', 'fan5', 'grid7x9', 'fan300', 'box9'):
        vertices, indices = mg.mesh(name)
        want = _canonical_rows(indices, len(vertices))
        got = sm.MeshTopology(indices.to(device), len(vertices), backend=backend).rows()
        assert got[0] == want[0] and got[1] == want[1], name
        if name == 'fan300':
            assert want[0][1] - want[0][0] == 300           # the hub: a row beyond the insertion-sort limit
    # a permuted face list: the same mesh, another -- but fixed -- order
    vertices, indices = mg.mesh('grid7x9')
    perm = torch.randperm(len(indices), generator=torch.Generator().manual_seed(3))
    x = vertices.to(device)
    plain = sm.compute_vertex_normal(x, indices.to(device), 'max', backend=backend)
    shuffled_indices = indices[perm].contiguous().to(device)
    shuffled = sm.compute_vertex_normal(x, shuffled_indices, 'max', backend=backend)
    assert float((plain - shuffled).abs().max()) <= 1e-6
    rows = [sm.MeshTopology(shuffled_indices, len(vertices), backend=backend).rows() for _ in range(2)]
    assert rows[0] == rows[1] == _canonical_rows(indices[perm], len(vertices))
    assert rows[0][0] == _canonical_rows(indices, len(vertices))[0] and rows[0][1] != _canonical_rows(indices, len(vertices))[1]


def _run_plan_validation(backend, device):
    sm = _shape_module()
    vertices, indices = mg.mesh('fan5')
    x = vertices.to(device)
    want = sm.compute_vertex_normal(x, indices.to(device), backend=backend)
    assert torch.equal(sm.compute_vertex_normal(x, indices.long().to(device), backend=backend), want)       # int64: converted once
    for bad in (len(vertices), -1, 2 ** 31 + 1):
        broken = indices.long().clone()
        broken[2, 1] = bad
        for t in (broken, broken.to(torch.int32)) if bad < 2 ** 31 else (broken,):
            with pytest.raises(RuntimeError, match='outside'):
                sm.MeshTopology(t.to(device), len(vertices), backend=backend)
    with pytest.raises(RuntimeError, match='at least 1'):
        sm.MeshTopology(indices.to(device), 0, backend=backend)
    with pytest.raises(ValueError, match='Unknown weighting scheme'):
        sm.compute_vertex_normal(x, indices.to(device), 'uniform', backend=backend)
    with pytest.raises(RuntimeError):
        sm.compute_vertex_normal(x.double(), indices.to(device), backend=backend)
    with pytest.raises(RuntimeError, match='tensor'):
        sm.compute_vertex_normal(x, indices.tolist(), backend=backend)
    with pytest.raises(RuntimeError):
        sm.compute_vertex_normal(x[:4], indices.to(device), topology=sm.MeshTopology(indices.to(device), 6, backend=backend))
    # no faces at all: every vertex is isolated
    empty = sm.compute_vertex_normal(x, torch.zeros(0, 3, dtype=torch.int32, device=device), backend=backend)
    assert torch.equal(empty.cpu(), torch.tensor([[0.0, 0.0, 1.0]] * len(vertices)))


def _run_plan_cache(backend, device):
    sm = _shape_module()
    vertices, indices = mg.mesh('fan5')
    x, idx = vertices.to(device), indices.to(device)
    sm._plans.clear()
    first = sm.compute_vertex_normal(x, idx, backend=backend)
    plan = next(iter(sm._plans.values()))[1]
    assert len(sm._plans) == 1 and torch.equal(sm.compute_vertex_normal(x, idx, backend=backend), first)
    assert len(sm._plans) == 1 and next(iter(sm._plans.values()))[1] is plan                    # reused
    idx[0] = idx[0].roll(1)                                                                     # in place: _version moves on
    again = sm.compute_vertex_normal(x, idx, backend=backend)
    assert len(sm._plans) == 2 and list(sm._plans.values())[-1][1] is not plan
    assert list(sm._plans.values())[-1][1].rows() == _canonical_rows(idx.cpu(), len(vertices))
    assert float((again - first).abs().max()) <= 1e-6                                           # (the same triangle, rotated)
    for k in range(sm.PLAN_CACHE_SIZE + 2):
        sm.compute_vertex_normal(x, idx.clone(), backend=backend)
    assert len(sm._plans) == sm.PLAN_CACHE_SIZE
    sm._plans.clear()


def test_plan_rows_hostsim(hostsim_backend):
    _run_plan_rows(hostsim_backend, CPU)


def test_plan_validation_hostsim(hostsim_backend):
    _run_plan_validation(hostsim_backend, CPU)


def test_plan_cache_hostsim(hostsim_backend):
    _run_plan_cache(hostsim_backend, CPU)


@pytest.mark.gpu
def test_plan_rows_gpu(gpu_backend):
    _run_plan_rows(gpu_backend, GPU)


@pytest.mark.gpu
def test_plan_validation_gpu(gpu_backend):
    _run_plan_validation(gpu_backend, GPU)


@pytest.mark.gpu
def test_plan_cache_gpu(gpu_backend):
    _run_plan_cache(gpu_backend, GPU)


# ---- 6. autograd plumbing -------------------------------------------------------------------------------------------------------
def _run_autograd(backend, device):
    sm = _shape_module()
    vertices, indices = mg.mesh('box4')
    idx = indices.to(device)
    topology = sm.MeshTopology(idx, len(vertices), backend=backend)
    w = mg.upstream(len(vertices), 1).to(device)
    for scheme in ('max', 'cotangent'):
        x = vertices.clone().to(device).requires_grad_(True)
        normals = sm.compute_vertex_normal(x, idx, scheme, topology=topology)
        (normals * w).sum().backward(retain_graph=True)
        once = x.grad.clone()
        (normals * w).sum().backward()                                       # twice over one graph: the saved sums are still there
        assert float(once.abs().sum()) > 0 and torch.equal(x.grad, once + once)
        x.grad = None
        strided = torch.empty(3, len(vertices), device=device).t()           # a gradient that is not contiguous
        strided.copy_(w)
        assert not strided.is_contiguous()
        sm.compute_vertex_normal(x, idx, scheme, topology=topology).backward(strided)
        assert torch.equal(x.grad, once)
        # a non-contiguous input; an unused output
        wide = torch.zeros(len(vertices), 5, device=device)
        wide[:, 1:4] = vertices.to(device)
        assert torch.equal(sm.compute_vertex_normal(wide[:, 1:4], idx, scheme, topology=topology), normals.detach())
        y = vertices.clone().to(device).requires_grad_(True)
        unused = sm.compute_vertex_normal(y, idx, scheme, topology=topology)
        (unused.detach().sum() + (y * 2.0).sum()).backward()
        assert torch.equal(y.grad, torch.full_like(y, 2.0))


def test_autograd_hostsim(hostsim_backend):
    _run_autograd(hostsim_backend, CPU)


@pytest.mark.gpu
def test_autograd_gpu(gpu_backend):
    _run_autograd(gpu_backend, GPU)


@pytest.mark.gpu
def test_product_library_refuses_host_tensors_gpu(gpu_backend):
    """No torch fall-back and no silent CPU path: CPU tensors are for the harness library only."""
    vertices, indices = mg.mesh('fan5')
    with pytest.raises(RuntimeError, match='harness'):
        _shape_module().compute_vertex_normal(vertices, indices, backend=gpu_backend)


def test_exports(hostsim_backend):
    import redner_amd
    vertices, indices = mg.mesh('fan5')
    normals = redner_amd.compute_vertex_normal(vertices, indices, backend=hostsim_backend)
    assert isinstance(redner_amd.MeshTopology(indices, 6, backend=hostsim_backend), _shape_module().MeshTopology)
    assert float((normals.norm(dim=1) - 1).abs().max()) < 1e-6 and redner_amd.VertexNormals is _shape_module().VertexNormals


# ---- 7. end to end --------------------------------------------------------------------------------------------------------------
def _run_e2e(backend, device, tag):
    import redner_amd
    v, f = mg.e2e_mesh()
    vertices, indices = torch.from_numpy(v).to(device).requires_grad_(True), torch.from_numpy(f).to(device)
    normals = redner_amd.compute_vertex_normal(vertices, indices, backend=backend)
    assert not normals.is_leaf
    img = mg.render_e2e(mg.e2e_scene(device, vertices, indices, normals), device, backend)
    assert tuple(vertices.grad.shape) == tuple(v.shape)
    out = {'image': img.detach().cpu().numpy(), 'grad_vertices': vertices.grad.cpu().numpy()}
    gold = dict(np.load(os.path.join(GOLD, 'vertex_normal_e2e.npz')))
    _assert_checksums(torch.from_numpy(v), torch.from_numpy(f), gold)
    _check('vertex_normal_e2e', out, {k: gold[k] for k in out}, tag)


def test_e2e_hostsim(hostsim_backend):
    _run_e2e(hostsim_backend, CPU, 'hostsim')


@pytest.mark.gpu
def test_e2e_gpu(gpu_backend):
    _run_e2e(gpu_backend, GPU, 'gpu')
