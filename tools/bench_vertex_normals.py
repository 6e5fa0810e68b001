#!/usr/bin/env python3
"""Vertex normals: the native kernels (redner_amd.shape) against the same formulas composed from torch operations on the same
device, as a user of this package had to before compute_vertex_normal existed.

    python tools/bench_vertex_normals.py [--spheres 40x64 300x500 700x1000] [--iters 50] [--warmup 5] [--out FILE]

The baseline is a copy of the definition of tests/test_vertex_normal.py (gathers, atan2 / sin / tan, index_add, torch.where)
run in fp32; its index_add is float atomics on the GPU, so unlike the native path it is not reproducible from run to run.
Per mesh (jittered UV spheres of tests/golden/make_mesh_golden.py, and the 300-spoke fan: one row far longer than a wave) and
scheme: (a) forward, (b) forward + backward, and once per mesh (c) building the MeshTopology (done once per connectivity, not per
iteration).  Baseline and native alternate inside one process, both warmed up; every call sits in its own pair of device
events; the median and the 10th / 90th percentiles are reported.  These are CALL times: they include the launches, the
allocation of outputs and scratch and the Python around them -- at the small sizes they measure those overheads, not the kernels.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]

from golden import make_mesh_golden as mg          # noqa: E402
from redner_amd import shape                       # noqa: E402
import op_bench                                    # noqa: E402


def _safe_sqrt(sq):
    """(sqrt(sq) where sq > 0 else 0, the mask), with a finite gradient everywhere"""
    live = sq > 0
    return torch.sqrt(torch.where(live, sq, torch.ones_like(sq))) * live, live


def torch_vertex_normals(v, idx, scheme):
    """The baseline: the formulas of csrc/vertex_normal.h composed from torch operations (a copy of the definition that
    tests/test_vertex_normal.py checks the kernels against, run here in fp32 on the device)."""
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


def against_torch(base, native, iters, warmup):
    out = op_bench.time_alternating({'torch': base, 'native': native}, iters, warmup)
    out['speedup'] = out['torch']['median_ms'] / out['native']['median_ms']
    return out


def time_plan(indices, num_vertices, iters):
    ts = []
    for _ in range(iters + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        shape.MeshTopology(indices, num_vertices)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return op_bench.summary(ts[2:])


def mesh_cases(name, vertices, indices, schemes, device, iters, warmup):
    v = vertices.to(device)
    idx32, idx64 = indices.to(device), indices.long().to(device)
    up = mg.upstream(len(vertices), 1).to(device)
    topology = shape.MeshTopology(idx32, len(vertices))
    res = {'mesh': name, 'vertices': len(vertices), 'triangles': len(indices), 'iters': iters,
           'longest_row': max(b - a for a, b in zip(topology.rows()[0], topology.rows()[0][1:])),
           'c_plan_build': time_plan(idx32, len(vertices), max(iters // 5, 5))}
    for scheme in schemes:
        x = v.clone().requires_grad_(True)
        with torch.no_grad():
            diff = float((torch_vertex_normals(v, idx64, scheme) - shape.compute_vertex_normal(v, idx32, scheme, topology=topology)).abs().max())

        def fwd_torch():
            with torch.no_grad():
                return torch_vertex_normals(v, idx64, scheme)

        def fwd_native():
            with torch.no_grad():
                return shape.compute_vertex_normal(v, idx32, scheme, topology=topology)

        def both_torch():
            x.grad = None
            torch_vertex_normals(x, idx64, scheme).backward(up)

        def both_native():
            x.grad = None
            shape.compute_vertex_normal(x, idx32, scheme, topology=topology).backward(up)

        res[scheme] = {'max_abs_difference_of_normals': diff,
                       'a_forward': against_torch(fwd_torch, fwd_native, iters, warmup),
                       'b_forward_backward': against_torch(both_torch, both_native, iters, warmup)}
        for key in ('a_forward', 'b_forward_backward'):
            r = res[scheme][key]
            print('%-16s V %8d T %8d %-9s %-18s torch %8.3f ms [%7.3f, %7.3f]   native %7.3f ms [%6.3f, %6.3f]   x%.1f'
                  % (name, len(vertices), len(indices), scheme, key, r['torch']['median_ms'], r['torch']['p10_ms'], r['torch']['p90_ms'],
                     r['native']['median_ms'], r['native']['p10_ms'], r['native']['p90_ms'], r['speedup']), flush=True)
    p = res['c_plan_build']
    print('%-16s plan build (once per connectivity) %8.3f ms [%7.3f, %7.3f], longest row %d'
          % (name, p['median_ms'], p['p10_ms'], p['p90_ms'], res['longest_row']), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--spheres', nargs='+', default=['40x64', '300x500', '700x1000'])
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    device = op_bench.require_gpu('bench_vertex_normals')
    results = []
    for spec in a.spheres:
        rows, cols = (int(s) for s in spec.split('x'))
        v, f = mg.uv_sphere(rows, cols, 22)
        # (cotangent on a sphere this fine falls back to 'max' everywhere: both sums are computed, which is what is timed)
        res = mesh_cases('sphere' + spec, torch.from_numpy(v), torch.from_numpy(f), ('max', 'cotangent'), device, a.iters, a.warmup)
        results.append(res)
    v, f = mg.mesh('fan300')
    results.append(mesh_cases('fan300', v, f, ('max',), device, a.iters, a.warmup))
    op_bench.emit(results, a.out)


if __name__ == '__main__':
    main()
