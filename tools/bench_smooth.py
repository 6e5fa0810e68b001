#!/usr/bin/env python3
"""Laplacian smoothing: the native kernels (redner_amd.shape: smooth, mesh_laplacian) against the same formulas composed from
torch operations on the same device, as a user of this package had to before they existed.

    python tools/bench_smooth.py [--spheres 40x64 300x500 700x1000] [--iters 50] [--warmup 5] [--out FILE]

The baseline is written here: gathers, lengths, asin angles, torch.where and index_add in fp32 (float atomics on the GPU, so
unlike the native path it is not reproducible from run to run); its backward pass is torch autograd.  Meshes and protocol are
those of tools/bench_vertex_normals.py: jittered UV spheres of tests/golden/make_mesh_golden.py and the 300-spoke fan; baseline
and native alternate inside one process, both warmed up; every call sits in its own pair of device events; the median and the
10th / 90th percentiles are reported.  Per mesh and scheme: (a) one smoothing step in place, (b) 10 steps (the native path: one
call with iterations = 10), (c) mesh_laplacian forward + backward.  Both sides get the same precomputed `control` (the boundary
mask) and the native side a MeshTopology built once.  These are CALL times: launches, the allocation of outputs and scratch and
the Python around them included -- at the small sizes they measure those overheads, not the kernels.
"""
import argparse
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]

from golden import make_mesh_golden as mg          # noqa: E402
from redner_amd import shape                       # noqa: E402
from bench_vertex_normals import against_torch     # noqa: E402   (torch against native, with their speedup)
from op_bench import emit, require_gpu             # noqa: E402

SCHEMES = ('reciprocal', 'uniform', 'cotangent')
LMD = 0.1


def torch_laplacian(v, idx, scheme, control):
    """The baseline: the formulas of csrc/mesh_smooth.h composed from torch operations in fp32, differentiable by autograd.
    Corners that add nothing and vertices that do not move are masked out before the division they would spoil."""
    p = [v[idx[:, k]] for k in range(3)]
    C, W = torch.zeros_like(v), torch.zeros(v.shape[0], dtype=v.dtype, device=v.device)
    for k in range(3):
        p0, p1, p2 = p[k], p[(k + 1) % 3], p[(k + 2) % 3]
        e1, e2 = p1 - p0, p2 - p0
        q1, q2 = (e1 * e1).sum(1), (e2 * e2).sum(1)
        live = (q1 > 0) & (q2 > 0)
        one = torch.ones_like(q1)
        l1, l2 = torch.sqrt(torch.where(live, q1, one)), torch.sqrt(torch.where(live, q2, one))
        if scheme == 'reciprocal':
            C = C.index_add(0, idx[:, k], (e1 / l1[:, None] + e2 / l2[:, None]) * live[:, None])
            W = W.index_add(0, idx[:, k], (1.0 / l1 + 1.0 / l2) * live)
        elif scheme == 'uniform':
            C = C.index_add(0, idx[:, k], (e1 + e2) * live[:, None])
            W = W.index_add(0, idx[:, k], 2.0 * live)
        else:
            a, b = e1 / l1[:, None], e2 / l2[:, None]
            obtuse = (a * b).sum(1) < 0
            chord = torch.where(obtuse[:, None], a + b, b - a)
            x = 0.5 * torch.sqrt((chord * chord).sum(1).clamp_min(1e-30))
            spread = live & (obtuse | (x > 1e-15))
            half = torch.asin(x.clamp(0, 1 - 1e-6))
            angle = torch.where(obtuse, math.pi - 2.0 * half, 2.0 * half)
            cot = torch.where(spread, 1.0 / torch.tan(torch.where(spread, angle, one)), torch.zeros_like(one))
            w = (p2 - p1) * cot[:, None]
            C = C.index_add(0, idx[:, (k + 1) % 3], w).index_add(0, idx[:, (k + 2) % 3], -w)
            W = W.index_add(0, idx[:, (k + 1) % 3], cot).index_add(0, idx[:, (k + 2) % 3], cot)
    moves = W != 0
    return torch.where(moves[:, None], C / torch.where(moves, W, torch.ones_like(W))[:, None], torch.zeros_like(C)) * control[:, None]


def torch_smooth(v, idx, lmd, scheme, control, iterations=1):
    with torch.no_grad():
        for _ in range(iterations):
            v.add_(torch_laplacian(v, idx, scheme, control) * lmd)


def mesh_cases(name, vertices, indices, device, iters, warmup):
    v = vertices.to(device)
    idx32, idx64 = indices.to(device), indices.long().to(device)
    up = mg.upstream(len(vertices), 1).to(device)
    topology = shape.MeshTopology(idx32, len(vertices))
    control = shape.bound_vertices(v, idx32, topology=topology)
    res = {'mesh': name, 'vertices': len(vertices), 'triangles': len(indices), 'iters': iters,
           'interior_vertices': int(control.sum())}
    for scheme in SCHEMES:
        x = v.clone().requires_grad_(True)
        with torch.no_grad():
            diff = float((torch_laplacian(v, idx64, scheme, control) - shape.mesh_laplacian(v, idx32, scheme, control, topology=topology)).abs().max())
        # every timed step starts from the same vertices: a mesh smoothed a thousand times over is another (degenerate) mesh
        work_torch, work_native = v.clone(), v.clone()

        def step_torch(n=1):
            work_torch.copy_(v)
            torch_smooth(work_torch, idx64, LMD, scheme, control, n)

        def step_native(n=1):
            work_native.copy_(v)
            shape.smooth(work_native, idx32, LMD, scheme, control, topology=topology, iterations=n)

        def both_torch():
            x.grad = None
            torch_laplacian(x, idx64, scheme, control).backward(up)

        def both_native():
            x.grad = None
            shape.mesh_laplacian(x, idx32, scheme, control, topology=topology).backward(up)

        res[scheme] = {'max_abs_difference_of_shift': diff,
                       'a_one_step': against_torch(step_torch, step_native, iters, warmup),
                       'b_ten_steps': against_torch(lambda: step_torch(10), lambda: step_native(10), max(iters // 2, 5), warmup),
                       'c_laplacian_forward_backward': against_torch(both_torch, both_native, iters, warmup)}
        for key in ('a_one_step', 'b_ten_steps', 'c_laplacian_forward_backward'):
            r = res[scheme][key]
            print('%-16s V %8d T %8d %-10s %-28s torch %8.3f ms [%7.3f, %7.3f]   native %7.3f ms [%6.3f, %6.3f]   x%.1f'
                  % (name, len(vertices), len(indices), scheme, key, r['torch']['median_ms'], r['torch']['p10_ms'], r['torch']['p90_ms'],
                     r['native']['median_ms'], r['native']['p10_ms'], r['native']['p90_ms'], r['speedup']), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--spheres', nargs='+', default=['40x64', '300x500', '700x1000'])
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    device = require_gpu('bench_smooth')
    results = []
    for spec in a.spheres:
        rows, cols = (int(s) for s in spec.split('x'))
        v, f = mg.uv_sphere(rows, cols, 22)
        results.append(mesh_cases('sphere' + spec, torch.from_numpy(v), torch.from_numpy(f), device, a.iters, a.warmup))
    v, f = mg.mesh('fan300')
    results.append(mesh_cases('fan300', v, f, device, a.iters, a.warmup))
    emit(results, a.out)


if __name__ == '__main__':
    main()
