#!/usr/bin/env python3
"""Forward plus backward of the rigid pose alone: the native op (redner_amd.pose_vertices on rdr_pose_vertices /
rdr_pose_vertices_backward) against the torch formulation on the same device, which is what a user of this package ran before it
existed: a rotation matrix filled element by element from cos / sin of the three angles, two 3 x 3 products, the mean of the
concatenated vertices, one matmul per set, autograd.

    python tools/bench_pose.py [--cases 2503 35947 1000+8] [--iters 200] [--warmup 10] [--iteration] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_pose.py --kernels-only     (kernel times, a run of its own)

A step is "angles, translation (both require grad), fixed vertices -> posed vertices -> gradients from a fixed upstream".
Baseline and native alternate inside one process, both warmed up; every step sits in its own pair of device events on the
current stream; the median and the 10th / 90th percentiles are reported.  These are STEP times: launches, allocations, autograd
and the Python around them included.  Launches per step are counted by torch.profiler (device kernels and copies of one step);
the run fails if the profiler reports none.

--iteration: one 256 x 256, 4 spp bunny_box iteration (pose, Scene, render, loss, backward) with the bunny posed each way and
with a fixed pose, so that the share of the pose in an iteration is on record.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]

from redner_amd import pose_vertices        # noqa: E402
from op_bench import count_launches, emit, require_gpu, time_alternating          # noqa: E402


def torch_rotate_matrix(angles):
    """The three plane rotations filled one element at a time, then multiplied: what the scripts' helper does in torch"""
    c, s = [angles[k].cos() for k in range(3)], [angles[k].sin() for k in range(3)]
    mats = [torch.zeros(3, 3, device=angles.device, dtype=torch.float32) for _ in range(3)]
    fill = (((0, 0, 1), (0, 1, 0), (0, 2, 0), (1, 0, 0), (1, 1, c[0]), (1, 2, s[0]), (2, 0, 0), (2, 1, -s[0]), (2, 2, c[0])),
            ((0, 0, c[1]), (0, 1, 0), (0, 2, -s[1]), (1, 0, 0), (1, 1, 1), (1, 2, 0), (2, 0, s[1]), (2, 1, 0), (2, 2, c[1])),
            ((0, 0, c[2]), (0, 1, -s[2]), (0, 2, 0), (1, 0, s[2]), (1, 1, c[2]), (1, 2, 0), (2, 0, 0), (2, 1, 0), (2, 2, 1)))
    for m, entries in zip(mats, fill):
        for i, j, value in entries:
            m[i, j] = value
    return mats[2] @ (mats[1] @ mats[0])


def torch_pose(sets, angles, translation):
    rotation = torch_rotate_matrix(angles)
    center = torch.mean(torch.cat(sets), 0)
    return [(v - center) @ torch.t(rotation) + center + translation for v in sets]


def make_steps(spec, device):
    sizes = [int(s) for s in spec.split('+')]
    gen = torch.Generator().manual_seed(21)
    sets = [torch.randn(n, 3, generator=gen).to(device) for n in sizes]
    upstream = [torch.randn(n, 3, generator=gen).to(device) for n in sizes]
    params = {name: (torch.tensor([0.1, -0.1, 0.1], device=device, requires_grad=True),
                     torch.tensor([0.1, 0.4, 0.1], device=device, requires_grad=True)) for name in ('torch', 'native')}
    last = {}

    def step(name, pose):
        angles, translation = params[name]
        angles.grad = translation.grad = None
        last[name] = pose(sets, angles, translation)
        torch.autograd.backward(last[name], upstream)

    return sizes, params, last, (lambda: step('torch', torch_pose)), (lambda: step('native', pose_vertices))


def rel(a, b):
    return float(((a.double() - b.double()).norm() / b.double().norm()).detach())


def run_case(spec, device, iters, warmup):
    sizes, params, last, step_torch, step_native = make_steps(spec, device)
    res = {'case': spec, 'iters': iters}
    steps = {'torch': step_torch, 'native': step_native}
    for f in steps.values():
        f()
    torch.cuda.synchronize()
    res['out_rel_difference'] = max(rel(x, y) for x, y in zip(last['native'], last['torch']))
    res['d_angles_rel_difference'] = rel(params['native'][0].grad, params['torch'][0].grad)
    res['d_translation_rel_difference'] = rel(params['native'][1].grad, params['torch'][1].grad)
    res['step'] = time_alternating(steps, iters, warmup)
    res['launches'] = {name: count_launches(f, 'bench_pose', required=True) for name, f in steps.items()}
    r = res['step']
    res['ratio'] = r['torch']['median_ms'] / r['native']['median_ms']
    print('%-12s step  torch %8.3f ms [%7.3f, %7.3f] %s launches   native %7.3f ms [%6.3f, %6.3f] %s launches   x%.1f   '
          '(outputs differ by %.1e, d_angles by %.1e, d_translation by %.1e)'
          % (spec, r['torch']['median_ms'], r['torch']['p10_ms'], r['torch']['p90_ms'], res['launches']['torch'],
             r['native']['median_ms'], r['native']['p10_ms'], r['native']['p90_ms'], res['launches']['native'], res['ratio'],
             res['out_rel_difference'], res['d_angles_rel_difference'], res['d_translation_rel_difference']), flush=True)
    return res


def run_iteration(device, res=256, spp=4, rounds=12):
    """pose + Scene + render + loss + backward of bunny_box with the bunny posed natively, by torch and not at all (its vertices a
    leaf that requires a gradient), alternating; wall time per iteration around a synchronise"""
    import scenes
    from redner_amd import gaussian_pyramid_loss, redner as rd
    from redner_amd.render_pytorch import RenderFunction
    sc = scenes.bunny_box(device, resolution=(res, res))
    bunny = int(np.load(os.path.join(ROOT, 'tests', 'golden', 'bunny_box_scene.npz'))['bunny_shape_id'])
    rest = sc.shapes[bunny].vertices.detach().clone()
    for k, s in enumerate(sc.shapes):
        s.vertices = s.vertices.detach().requires_grad_(k != bunny)
    target = torch.rand(res, res, 3, generator=torch.Generator().manual_seed(3)).to(device)
    angles = torch.tensor([0.1, -0.1, 0.1], device=device, requires_grad=True)
    translation = torch.tensor([0.1, 0.4, 0.1], device=device, requires_grad=True)
    poses = {'fixed': None, 'native': lambda: pose_vertices(rest, angles, translation),
             'torch': lambda: torch_pose([rest], angles, translation)[0]}
    times = {name: [] for name in poses}
    for it in range(rounds):
        for j, (name, f) in enumerate(poses.items()):
            # every iteration has a pose of its own: no variant renders geometry that the one before it left in the Scene caches
            with torch.no_grad():
                angles[0] = 0.1 + 1e-3 * (it * len(poses) + j)
            fixed = pose_vertices(rest, angles, translation).detach().clone()
            torch.cuda.synchronize()
            t0 = time.time()
            angles.grad = translation.grad = None
            sc.shapes[bunny].vertices = fixed.requires_grad_(True) if f is None else f()
            args = RenderFunction.serialize_scene(sc, spp, 4, sampler_type=rd.SamplerType.sobol, device=device, backend=rd)
            gaussian_pyramid_loss(RenderFunction.apply(it + 1, *args), target, 5).backward()
            torch.cuda.synchronize()
            times[name].append(time.time() - t0)
    out = {'case': 'bunny_box %dx%d, %d spp, one iteration, %d bunny vertices' % (res, res, spp, rest.shape[0])}
    for name, ts in times.items():
        ts = sorted(ts[2:])
        out[name + '_median_ms'] = ts[len(ts) // 2] * 1e3
    print('bunny_box %dx%d %d spp iteration: %s' % (res, res, spp, '   '.join(
        '%s pose %.2f ms' % (name, out[name + '_median_ms']) for name in poses)), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', nargs='+', default=['2503', '35947', '1000+8'], help='vertices per set, sets joined by +')
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--out', default=None)
    ap.add_argument('--iteration', action='store_true', help='also one bunny_box iteration with each pose')
    ap.add_argument('--kernels-only', action='store_true', help='only the native steps, untimed: for a kernel trace')
    a = ap.parse_args()
    device = require_gpu('bench_pose')
    if a.kernels_only:
        for spec in a.cases:
            step_native = make_steps(spec, device)[4]
            for _ in range(a.iters):
                step_native()
            torch.cuda.synchronize()
        return
    results = [run_case(spec, device, a.iters, a.warmup) for spec in a.cases]
    if a.iteration:
        results.append(run_iteration(device))
    emit(results, a.out)


if __name__ == '__main__':
    main()
