"""The rigid pose of the reference's pose-estimation scripts on the native kernels of csrc/pose.h.

    R = gen_rotate_matrix(angles)                                    # rdr_rotate_matrix: [3] fp32 -> [3, 3] fp32
    posed = pose_vertices([v0, v1], angles, translation)             # rdr_pose_vertices: every set in the same launches
    render(posed); loss.backward()                                   # rdr_pose_vertices_backward

What the scripts write in torch at every iteration (tests/test_bunny_box.py, tutorials 02 and 04):

    R = pyredner.gen_rotate_matrix(euler_angles)                     Rz(psi) (Ry(phi) Rx(theta)), filled element by element
    center = torch.mean(torch.cat(all vertex sets), 0)
    vertices_k = (vertices0_k - center) @ torch.t(R) + center + translation

About 200 torch operations forward and backward become at most two native launches each way.  csrc/pose.h pins the arithmetic:
R from glibc-exact fp64 sines and cosines, rounded once; the centre an fp64 mean; the sums of the angle and translation gradients
fp64 in a fixed order without atomics, so every output and gradient is bitwise reproducible from run to run.

There is no torch fall-back: the tensors' memory goes to the loaded native library.  CPU vertices are accepted by the CPU
debugging harness only (the test-suite loads it); the product library raises for them.  Nothing synchronises: angles,
translation and centre are read on the device.
"""
import torch

from . import redner as _default_backend
from ._op import first_order_only, named, place, ptr, scratch, upstream

MAX_SETS = 16


class RotateMatrix(torch.autograd.Function):
    """angles [3] fp32 -> R [3, 3] fp32 on the same device; the gradient goes to `angles`, once: under create_graph=True the backward
    call raises."""

    @staticmethod
    def forward(ctx, angles, backend=None):
        rd = backend or _default_backend
        a = angles.detach().contiguous()
        matrix = torch.empty(3, 3, dtype=torch.float32, device=a.device)
        rd.rotate_matrix(ptr(rd, a), ptr(rd, matrix), *place(a))
        ctx.rd = rd
        ctx.save_for_backward(a)
        return matrix

    @staticmethod
    def backward(ctx, d_matrix):
        first_order_only('RotateMatrix')
        rd = ctx.rd
        a, = ctx.saved_tensors
        g = upstream(d_matrix, a.device)
        d_angles = torch.empty(3, dtype=torch.float32, device=a.device)
        rd.rotate_matrix_backward(ptr(rd, a), ptr(rd, g), ptr(rd, d_angles), *place(a))
        return d_angles, None


def _forward(rd, sets, a, t, c):
    """sets, a, t, c (or None): detached contiguous fp32 on one device.  -> the posed sets, saved [12] (R, then the centre used)"""
    device = sets[0].device
    counts = [int(v.shape[0]) for v in sets]
    out = [torch.empty_like(v) for v in sets]
    saved = torch.empty(12, dtype=torch.float32, device=device)
    work, floats = None, 0
    if c is None:
        floats, _ = rd.pose_scratch(counts)
        work = scratch(floats, device)
    rd.pose_vertices([ptr(rd, v) for v in sets], counts, ptr(rd, a), ptr(rd, t), ptr(rd, c), [ptr(rd, o) for o in out],
                     ptr(rd, saved), ptr(rd, work), floats, *place(device))
    return out, saved


class PoseVertices(torch.autograd.Function):
    """(angles, translation, center or None, backend, *vertex sets) -> one posed tensor per set.  All tensors fp32 on one device.
    Gradients go to angles, translation, a given centre and every vertex set that asks for one; an output without an upstream
    gradient counts as zeros; under create_graph=True the backward call raises (the adjoint cannot be differentiated again).  The node of the outputs (`out.grad_fn`) keeps `saved`, the [12] fp32 tensor the forward call
    wrote and the backward call reads: R row by row, then the centre that was used."""

    @staticmethod
    def forward(ctx, angles, translation, center, backend, *vertices):
        rd = backend or _default_backend
        sets = [v.detach().contiguous() for v in vertices]
        a = angles.detach().contiguous()
        c = None if center is None else center.detach().contiguous()
        out, saved = _forward(rd, sets, a, translation.detach().contiguous(), c)
        ctx.rd, ctx.counts, ctx.saved, ctx.own = rd, [int(v.shape[0]) for v in sets], saved, c is None
        # what the backward call reads, and a given centre (its copy in `saved` is what is read): for a contiguous input that is
        # the caller's own memory, and saved this way an in-place edit before backward raises.  ctx.saved stays for readers.
        ctx.save_for_backward(a, saved, *sets, *(() if c is None else (c,)))
        ctx.set_materialize_grads(False)
        return tuple(out)

    @staticmethod
    def backward(ctx, *d_out):
        first_order_only('PoseVertices')
        rd, counts = ctx.rd, ctx.counts
        a, saved = ctx.saved_tensors[:2]
        sets = list(ctx.saved_tensors[2:2 + len(counts)])
        device = sets[0].device
        g = [upstream(d, device) for d in d_out]
        d_vertices = [torch.empty_like(v) if ctx.needs_input_grad[4 + k] else None for k, v in enumerate(sets)]
        d_angles, d_translation = (torch.empty(3, dtype=torch.float32, device=device) for _ in range(2))
        d_center = None if ctx.own else torch.empty(3, dtype=torch.float32, device=device)
        _, floats = rd.pose_scratch(counts)
        work = scratch(floats, device)
        rd.pose_vertices_backward([ptr(rd, v) for v in sets], counts, ptr(rd, a), ptr(rd, saved), ctx.own, [ptr(rd, d) for d in g],
                                  [ptr(rd, d) for d in d_vertices] if any(d is not None for d in d_vertices) else None,
                                  ptr(rd, d_angles), ptr(rd, d_translation), ptr(rd, d_center), ptr(rd, work), floats, *place(device))
        return (d_angles, d_translation, d_center, None) + tuple(d_vertices)


def _triple(who, name, t, device):
    """A [3] fp32 tensor on `device` or on the CPU, moved (differentiably) to `device`."""
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != (3,):
        raise ValueError('%s: %s must be a tensor of shape [3]' % (who, name))
    if t.dtype != torch.float32:
        raise ValueError('%s: fp32 only, %s is %s' % (who, name, t.dtype))
    if t.device != device and t.device.type != 'cpu':
        raise ValueError('%s: %s is on %s, the vertices on %s' % (who, name, t.device, device))
    return t if t.device == device else t.to(device)


def gen_rotate_matrix(angles, backend=None):
    """The reference's gen_rotate_matrix: the 3 x 3 rotation matrix Rz(angles[2]) (Ry(angles[1]) Rx(angles[0])) of a [3] fp32
    tensor of Euler angles, in its sign convention, on the angles' device; differentiable."""
    who = 'gen_rotate_matrix'
    if isinstance(angles, torch.Tensor):
        angles = _triple(who, 'angles', angles, angles.device)
    else:
        raise ValueError('%s: angles must be a tensor of shape [3]' % who)
    with named(who):
        return RotateMatrix.apply(angles, backend)


def _checked(who, vertices, angles, translation, center):
    single = isinstance(vertices, torch.Tensor)
    if not single and not isinstance(vertices, (list, tuple)):
        raise ValueError('%s: vertices must be a tensor [N, 3] or a list / tuple of them' % who)
    sets = [vertices] if single else list(vertices)
    if not 1 <= len(sets) <= MAX_SETS:
        raise ValueError('%s: between 1 and %d vertex sets in a call, got %d' % (who, MAX_SETS, len(sets)))
    for k, v in enumerate(sets):
        if not isinstance(v, torch.Tensor) or v.dim() != 2 or v.shape[1] != 3:
            raise ValueError('%s: vertex set %d must be a tensor [N, 3]' % (who, k))
        if v.dtype != torch.float32:
            raise ValueError('%s: fp32 only, vertex set %d is %s' % (who, k, v.dtype))
        if v.shape[0] < 1:
            raise ValueError('%s: vertex set %d is empty' % (who, k))
        if v.device != sets[0].device:
            raise ValueError('%s: vertex set %d is on %s, set 0 on %s' % (who, k, v.device, sets[0].device))
    device = sets[0].device
    angles = _triple(who, 'angles', angles, device)
    translation = _triple(who, 'translation', translation, device)
    if center is not None:
        center = _triple(who, 'center', center, device)
    return single, sets, angles, translation, center


def pose_vertices(vertices, angles, translation, center=None, backend=None):
    """(v - center) @ R^T + center + translation with R = gen_rotate_matrix(angles), for one [N, 3] fp32 tensor or a list / tuple
    of at most 16 of them on one device; the result has the same structure, in new contiguous tensors.  center=None: the mean
    over the concatenation of all the sets given (differentiable through the vertices), as the scripts do; otherwise a [3] fp32
    tensor.  angles, translation and center may live on the vertices' device or on the CPU (their gradients come back to where
    they live)."""
    who = 'pose_vertices'
    single, sets, angles, translation, center = _checked(who, vertices, angles, translation, center)
    with named(who):
        out = PoseVertices.apply(angles, translation, center, backend, *sets)
    return out[0] if single else (tuple(out) if isinstance(vertices, tuple) else list(out))

