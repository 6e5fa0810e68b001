"""Smooth vertex normals (pyredner/shape.py: compute_vertex_normal) on the native kernels, with a vertex gradient; and, further
down, Laplacian smoothing (smooth, bound_vertices, the differentiable mesh_laplacian) on the same plan.

    topology = MeshTopology(indices, num_vertices)                   # once per connectivity
    for it in range(steps):
        shape.normals = compute_vertex_normal(vertices, indices, 'max', topology=topology)
        loss(render(scene)).backward()                               # vertices.grad: the geometric part + the normals' part

The meaning is the reference's (csrc/vertex_normal.h restates it):

  * 'max': every corner adds  n * sin(angle) / (|e1| |e2|)  to its vertex (n: the face's unit normal, e1, e2: the corner's
    sides); the sum is normalised, or (0, 0, 1) where it is zero (an isolated vertex).
  * 'cotangent': corner i adds (v[i+2] - v[i+1]) * cot(angle_i) to vertex i + 1 and subtracts it from vertex i + 2; the sum is
    turned to the side of the 'max' normal and normalised if it is longer than 0.05, otherwise the 'max' normal is the result.
  * per-corner terms in fp32, per-vertex sums in fp64 in ascending corner id 3 f + k, rounded once: a function of `indices`
    only, so the normals AND the gradient are bitwise reproducible (the reference's scatter_add_ is fp32 atomics on a GPU).
  * the gradient of a degenerate corner or face, and of a vertex that takes (0, 0, 1), is 0 where the reference returns NaN.

What depends on `indices` only (validation, the rows of corners per vertex) is a `MeshTopology`, built once; without one,
compute_vertex_normal keeps the plans of the last 8 index tensors it saw.

There is no torch fall-back: the tensors' memory goes to the loaded native library.  CPU tensors are accepted by the CPU
debugging harness only (the test-suite loads it); the product library raises for them.
"""
import collections
import threading

import torch

from . import redner as _default_backend
from ._op import first_order_only, place, ptr, scratch, upstream

SCHEMES = {'max': 0, 'cotangent': 1}
PLAN_CACHE_SIZE = 8


class MeshTopology:
    """The plan of one connectivity: indices [T, 3] (int32, or int64: converted once here) validated against num_vertices and
    turned into the rows of corners per vertex, on the indices' device.  Raises RuntimeError for an index outside
    [0, num_vertices).  Owns the native plan and destroys it on collection."""

    def __init__(self, indices, num_vertices, backend=None):
        rd = backend or _default_backend
        if not isinstance(indices, torch.Tensor) or indices.dim() != 2 or indices.shape[1] != 3:
            raise RuntimeError('MeshTopology: indices must be a [T, 3] tensor, got %s' % (tuple(getattr(indices, 'shape', ())),))
        if indices.dtype == torch.int64:
            # (values beyond int32 stay out of range instead of wrapping into it)
            indices = indices.clamp(-1, 2 ** 31 - 1).to(torch.int32)
        if indices.dtype != torch.int32:
            raise RuntimeError('MeshTopology: int32 or int64 indices only')
        indices = indices.detach().contiguous()
        self.num_vertices, self.num_triangles, self.device = int(num_vertices), int(indices.shape[0]), indices.device
        self.native = rd.mesh_topology(rd.int_ptr(indices.data_ptr()), self.num_triangles, self.num_vertices, *place(indices))
        self.rd = rd

    def rows(self):
        """(offsets, corners): vertex v sums the corners corners[offsets[v]:offsets[v + 1]] in that order (corner 3 f + k)."""
        return self.native.read()


class VertexNormals(torch.autograd.Function):
    """vertices [V, 3] -> normals [V, 3].  One native call forward, one backward; the gradient goes to `vertices`, once: under
    create_graph=True the backward call raises."""

    @staticmethod
    def forward(ctx, vertices, topology, scheme):
        rd = topology.rd
        if vertices.dim() != 2 or tuple(vertices.shape) != (topology.num_vertices, 3):
            raise RuntimeError('compute_vertex_normal: vertices must be [%d, 3], got %s' % (topology.num_vertices, tuple(vertices.shape)))
        if vertices.dtype != torch.float32:
            raise RuntimeError('compute_vertex_normal: fp32 vertices only')
        if vertices.device != topology.device:
            raise RuntimeError('compute_vertex_normal: vertices are on %s, the topology on %s' % (vertices.device, topology.device))
        v = vertices.detach().contiguous()
        n_fwd, _, n_saved = topology.native.scratch(scheme)
        normals = torch.empty_like(v)
        saved = torch.empty(max(n_saved, 1), dtype=torch.float32, device=v.device)
        work = scratch(n_fwd, v.device)
        rd.vertex_normal(topology.native, scheme, ptr(rd, v), ptr(rd, normals), ptr(rd, saved), ptr(rd, work), n_fwd)
        ctx.topology, ctx.scheme = topology, scheme
        ctx.save_for_backward(v, saved)
        ctx.set_materialize_grads(False)
        return normals

    @staticmethod
    def backward(ctx, d_normals):
        first_order_only('VertexNormals')
        if d_normals is None:
            return None, None, None
        topology, rd = ctx.topology, ctx.topology.rd
        v, saved = ctx.saved_tensors
        g = upstream(d_normals, v.device)
        n_bwd = topology.native.scratch(ctx.scheme)[1]
        d_vertices = torch.empty_like(v)
        work = scratch(n_bwd, v.device)
        rd.vertex_normal_backward(topology.native, ctx.scheme, ptr(rd, v), ptr(rd, saved), ptr(rd, g), ptr(rd, d_vertices),
                                  ptr(rd, work), n_bwd)
        return d_vertices, None, None


# the plans compute_vertex_normal made itself: key -> (the indices tensor, MeshTopology).  The key names the tensor's memory and
# version; the entry keeps the tensor alive, so its address cannot be handed to another tensor while the entry exists.
_plans = collections.OrderedDict()
_plans_lock = threading.Lock()          # compute_vertex_normal may be called from several threads (one per device)


def _cached_topology(indices, num_vertices, rd):
    from . import _capi
    if not isinstance(indices, torch.Tensor):
        raise RuntimeError('compute_vertex_normal: indices must be a [T, 3] tensor')
    key = (indices.data_ptr(), indices._version, tuple(indices.shape), tuple(indices.stride()), indices.dtype, str(indices.device),
           int(num_vertices), id(rd), _capi.library_path())
    with _plans_lock:
        hit = _plans.get(key)
        if hit is not None:
            _plans.move_to_end(key)
            return hit[1]
    topology = MeshTopology(indices, num_vertices, backend=rd)          # (outside the lock: it synchronises a device)
    with _plans_lock:
        _plans[key] = (indices, topology)
        while len(_plans) > PLAN_CACHE_SIZE:
            _plans.popitem(last=False)
    return topology


def compute_vertex_normal(vertices, indices, weighting_scheme='max', topology=None, backend=None):
    """pyredner.compute_vertex_normal: the [V, 3] fp32 vertex normals of a mesh (contiguous, on the vertices' device),
    differentiable with respect to `vertices`.  weighting_scheme: 'max' or 'cotangent'.  topology: the MeshTopology of
    `indices` (then `indices` is not looked at); None = one is made and kept for the next call with the same index tensor."""
    if weighting_scheme not in SCHEMES:
        raise ValueError('Unknown weighting scheme: {}'.format(weighting_scheme))
    if not isinstance(vertices, torch.Tensor) or vertices.dim() != 2 or vertices.shape[1] != 3:
        raise RuntimeError('compute_vertex_normal: vertices must be a [V, 3] tensor')
    if topology is None:
        topology = _cached_topology(indices, int(vertices.shape[0]), backend or _default_backend)
    return VertexNormals.apply(vertices, topology, SCHEMES[weighting_scheme])


# ---- Laplacian smoothing (pyredner/shape.py: bound_vertices, smooth; csrc/mesh_smooth.h restates the meaning) ---------------------
#   * every vertex i gets a vector sum C_i and a weight sum W_i over its corners ('reciprocal': unit sides and 1 / |side|;
#     'uniform': sides and 2; 'cotangent': the opposite edges times cot of the opposite angles, and those cots);
#     shift_i = (C_i / W_i) * control_i, and smooth sets v_i = v_i + shift_i * lmd
#   * per-corner terms in fp32, per-vertex sums in fp64 in ascending corner id, rounded once: bitwise reproducible (the
#     reference's scatter_add_ is fp32 atomics on a GPU)
#   * a vertex with W == 0 (isolated, or of degenerate corners only) does not move and has a zero gradient, and a 'cotangent'
#     corner that is degenerate adds nothing, where the reference returns NaN
#   * mesh_laplacian is the displacement itself as a differentiable function (a regulariser |L v|^2 can go into a loss);
#     the reference's smooth only updates vertices.data
SMOOTH_SCHEMES = {'reciprocal': 0, 'uniform': 1, 'cotangent': 2}


def _smooth_arguments(who, vertices, indices, weighting_scheme, topology, backend):
    """The checks of compute_vertex_normal for the smoothing functions -> the topology"""
    if weighting_scheme not in SMOOTH_SCHEMES:
        raise ValueError('Unknown weighting_scheme: {}'.format(weighting_scheme))
    if not isinstance(vertices, torch.Tensor) or vertices.dim() != 2 or vertices.shape[1] != 3:
        raise RuntimeError('%s: vertices must be a [V, 3] tensor' % who)
    if topology is None:
        topology = _cached_topology(indices, int(vertices.shape[0]), backend or _default_backend)
    if tuple(vertices.shape) != (topology.num_vertices, 3):
        raise RuntimeError('%s: vertices must be [%d, 3], got %s' % (who, topology.num_vertices, tuple(vertices.shape)))
    if vertices.dtype != torch.float32:
        raise RuntimeError('%s: fp32 vertices only' % who)
    if vertices.device != topology.device:
        raise RuntimeError('%s: vertices are on %s, the topology on %s' % (who, vertices.device, topology.device))
    return topology


def _boundary(topology):
    rd = topology.rd
    bound = torch.empty(topology.num_vertices, dtype=torch.float32, device=topology.device)
    rd.mesh_boundary(topology.native, ptr(rd, bound))
    return bound


def _control(control, topology):
    """control [V] as the kernels read it: fp32, contiguous, on the topology's device, a constant; None = the boundary mask"""
    if control is None:
        return _boundary(topology)
    if not isinstance(control, torch.Tensor) or control.numel() != topology.num_vertices:
        raise ValueError('Size of control tensor inconsistent with number of vertices')
    return control.detach().to(device=topology.device, dtype=torch.float32).reshape(-1).contiguous()


def bound_vertices(vertices, indices, topology=None, backend=None):
    """pyredner.bound_vertices: [V] fp32 on the vertices' device, 0 for a vertex on an open rim of the mesh, otherwise 1 (the
    default `control` of smooth).  A function of the connectivity only, summed in integers.  topology: as compute_vertex_normal."""
    return _boundary(_smooth_arguments('bound_vertices', vertices, indices, 'reciprocal', topology, backend))


class MeshLaplacian(torch.autograd.Function):
    """vertices [V, 3] -> shift [V, 3] = (C / W) * control; control [V] is a constant.  One native call forward, one backward; the
    gradient goes to `vertices`, once: under create_graph=True the backward call raises."""

    @staticmethod
    def forward(ctx, vertices, topology, scheme, control):
        rd = topology.rd
        v = vertices.detach().contiguous()
        n_fwd, _, n_saved = rd.mesh_smooth_scratch(topology.native, scheme)
        shift = torch.empty_like(v)
        saved = torch.empty(max(n_saved, 1), dtype=torch.float32, device=v.device)
        work = scratch(n_fwd, v.device)
        rd.mesh_laplacian(topology.native, scheme, ptr(rd, v), ptr(rd, control), ptr(rd, shift), ptr(rd, saved), ptr(rd, work), n_fwd)
        ctx.topology, ctx.scheme = topology, scheme
        ctx.save_for_backward(v, control, saved)
        ctx.set_materialize_grads(False)
        return shift

    @staticmethod
    def backward(ctx, d_shift):
        first_order_only('MeshLaplacian')
        if d_shift is None:
            return None, None, None, None
        topology, rd = ctx.topology, ctx.topology.rd
        v, control, saved = ctx.saved_tensors
        g = upstream(d_shift, v.device)
        n_bwd = rd.mesh_smooth_scratch(topology.native, ctx.scheme)[1]
        d_vertices = torch.empty_like(v)
        work = scratch(n_bwd, v.device)
        rd.mesh_laplacian_backward(topology.native, ctx.scheme, ptr(rd, v), ptr(rd, control), ptr(rd, saved), ptr(rd, g),
                                   ptr(rd, d_vertices), ptr(rd, work), n_bwd)
        return d_vertices, None, None, None


def mesh_laplacian(vertices, indices, weighting_scheme='reciprocal', control=None, topology=None, backend=None):
    """The displacement of one smoothing step of unit length, [V, 3] fp32 (contiguous, on the vertices' device), differentiable
    with respect to `vertices`: smooth(vertices, ..., lmd) adds mesh_laplacian(vertices, ...) * lmd.  weighting_scheme:
    'reciprocal', 'uniform' or 'cotangent'.  control: [V] factors, a constant; None = bound_vertices (an open rim stays put).
    topology: as compute_vertex_normal."""
    topology = _smooth_arguments('mesh_laplacian', vertices, indices, weighting_scheme, topology, backend)
    return MeshLaplacian.apply(vertices, topology, SMOOTH_SCHEMES[weighting_scheme], _control(control, topology))


def smooth(vertices, indices, lmd, weighting_scheme='reciprocal', control=None, topology=None, iterations=1, backend=None):
    """pyredner.smooth: `iterations` steps of Laplacian smoothing, vertices += mesh_laplacian(vertices) * lmd, written into the
    tensor's own memory.  Returns None and leaves no autograd record (a leaf that requires grad is accepted and stays a leaf);
    vertices._version advances, so whatever is cached by version sees the change.  lmd: a Python number or a one-element tensor,
    rounded to fp32.  control: as mesh_laplacian, evaluated once for all iterations."""
    topology = _smooth_arguments('smooth', vertices, indices, weighting_scheme, topology, backend)
    if int(iterations) < 1:
        raise ValueError('smooth: iterations must be at least 1, got %s' % (iterations,))
    rd, scheme = topology.rd, SMOOTH_SCHEMES[weighting_scheme]
    control = _control(control, topology)
    v = vertices.detach().contiguous()
    n_fwd = rd.mesh_smooth_scratch(topology.native, scheme)[0]
    moved = torch.empty_like(v)
    work = scratch(n_fwd, v.device)
    rd.mesh_smooth(topology.native, scheme, ptr(rd, v), ptr(rd, control), float(lmd), int(iterations), ptr(rd, moved), ptr(rd, work),
                   n_fwd)
    with torch.no_grad():
        vertices.copy_(moved)              # (not a write through .data: that would leave vertices._version where it was)
