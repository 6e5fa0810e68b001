#!/usr/bin/env python3
"""Forward plus backward of the Gaussian pyramid loss alone: the native op (redner_amd.gaussian_pyramid_loss on rdr_pyramid_loss /
rdr_pyramid_loss_backward) against the torch formulation on the same device, which is what a user of this package ran before it
existed (a permute to NCHW, per level a dense C x C x 7 x 7 conv2d and an AvgPool2d(2), a reduction per level, autograd).

    python tools/bench_pyramid_loss.py [--cases 256x256x3x5 1024x1024x3x5] [--iters 200] [--warmup 10] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_pyramid_loss.py --kernels-only     (kernel times, a run of its own)

A step is "image (requires grad), target -> loss -> image.grad".  Baseline and native alternate inside one process, both warmed
up; every step sits in its own pair of device events on the current stream; the median and the 10th / 90th percentiles are
reported.  These are STEP times: launches, allocations, autograd and the Python around them included.  Launches per step are
counted by torch.profiler (device kernels and copies of one step; `null` where the profiler reports none).  The native op's
time is also set against its traffic bound: the bytes of image, target, the levels written and read again, the level gradients
written and read, and d_image, over the 6.29 TB/s a float4 copy reaches on this chip.  If the convolution library cannot run
the baseline, that is recorded and the native figures stand alone.

--iteration: one 256 x 256, 4 spp bunny_box iteration (Scene, render, loss, backward) with each loss, so that the share of the
loss in an iteration is on record.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]

from redner_amd import gaussian_pyramid_loss        # noqa: E402
from op_bench import count_launches, emit, require_gpu, time_alternating          # noqa: E402

COPY_BYTES_PER_S = 6.29e12


def taps():
    k = np.arange(-4, 5, dtype=np.float64)
    w = np.exp(-0.5 * k * k)
    w /= w.sum()
    return np.array([w[1] + w[0], w[2], w[3], w[4], w[5], w[6], w[7] + w[8]]).astype(np.float32)


def torch_loss_factory(channels, num_levels, device):
    a = torch.from_numpy(taps())
    table = torch.outer(a, a)
    kernel = torch.zeros(channels, channels, 7, 7)
    for k in range(channels):
        kernel[k, k] = table
    kernel = kernel.to(device)
    pool = torch.nn.AvgPool2d(2)

    def loss(image, target):
        d = (image - target).unsqueeze(0).permute(0, 3, 1, 2)
        h, w = d.shape[2], d.shape[3]
        total = d.pow(2).sum() / (h * w)
        for l in range(1, num_levels):
            d = pool(torch.nn.functional.conv2d(d, kernel, padding=3))
            total = total + d.pow(2).sum() / ((h / 2 ** l) * (w / 2 ** l))
        return total
    return loss


def traffic_bytes(h, w, c, num_levels):
    sizes = [(h >> l) * (w >> l) * c for l in range(num_levels)]
    # forward: image + target read, levels 1.. written and (all but the last) read again; backward: image + target read, levels
    # 1.. read, their gradients written and read, d_image written
    return 4 * (2 * sizes[0] + sum(sizes[1:]) + sum(sizes[1:-1]) + 2 * sizes[0] + 3 * sum(sizes[1:]) + sizes[0])


def make_steps(spec, device):
    h, w, c, num_levels = (int(s) for s in spec.split('x'))
    gen = torch.Generator().manual_seed(11)
    target = torch.rand(h, w, c, generator=gen).to(device)
    images = {name: (torch.rand(h, w, c, generator=torch.Generator().manual_seed(12))).to(device).requires_grad_(True)
              for name in ('torch', 'native')}
    torch_loss = torch_loss_factory(c, num_levels, device)
    last = {}

    def step_torch():
        x = images['torch']
        x.grad = None
        last['torch'] = torch_loss(x, target)
        last['torch'].backward()

    def step_native():
        x = images['native']
        x.grad = None
        last['native'] = gaussian_pyramid_loss(x, target, num_levels)
        last['native'].backward()

    return (h, w, c, num_levels), images, last, step_torch, step_native


def run_case(spec, device, iters, warmup):
    (h, w, c, num_levels), images, last, step_torch, step_native = make_steps(spec, device)
    res = {'case': spec, 'iters': iters}
    steps = {'native': step_native}
    try:
        step_torch()
        torch.cuda.synchronize()
        steps = {'torch': step_torch, 'native': step_native}
    except Exception as e:
        res['torch_baseline_failed'] = '%s: %s' % (type(e).__name__, str(e).splitlines()[0] if str(e) else '')
        print('bench_pyramid_loss: the torch formulation does not run on this device: %s' % res['torch_baseline_failed'], flush=True)
    step_native()
    torch.cuda.synchronize()
    if 'torch' in steps:
        res['loss_rel_difference'] = abs(last['torch'].item() - last['native'].item()) / abs(last['torch'].item())
        res['grad_rel_difference'] = float((images['torch'].grad - images['native'].grad).norm() / images['torch'].grad.norm())
    res['step'] = time_alternating(steps, iters, warmup)
    res['launches'] = {name: count_launches(f, 'bench_pyramid_loss') for name, f in steps.items()}
    bound_ms = traffic_bytes(h, w, c, num_levels) / COPY_BYTES_PER_S * 1e3
    res['native_traffic_bytes'], res['native_traffic_bound_ms'] = traffic_bytes(h, w, c, num_levels), bound_ms
    r = res['step']
    if 'torch' in r:
        res['ratio'] = r['torch']['median_ms'] / r['native']['median_ms']
        print('%-16s step  torch %8.3f ms [%7.3f, %7.3f] %s launches   native %7.3f ms [%6.3f, %6.3f] %s launches   x%.1f   '
              '(loss differs by %.1e, gradient by %.1e; traffic bound of the native op %.4f ms)'
              % (spec, r['torch']['median_ms'], r['torch']['p10_ms'], r['torch']['p90_ms'], res['launches']['torch'],
                 r['native']['median_ms'], r['native']['p10_ms'], r['native']['p90_ms'], res['launches']['native'], res['ratio'],
                 res['loss_rel_difference'], res['grad_rel_difference'], bound_ms), flush=True)
    else:
        print('%-16s step  native %7.3f ms [%6.3f, %6.3f] %s launches   traffic bound %.4f ms'
              % (spec, r['native']['median_ms'], r['native']['p10_ms'], r['native']['p90_ms'], res['launches']['native'], bound_ms),
              flush=True)
    return res


def run_iteration(device, res=256, spp=4, rounds=12):
    """Scene + render + loss + backward of bunny_box with each loss, alternating; wall time per iteration around a synchronise"""
    import scenes
    from redner_amd import redner as rd
    from redner_amd.render_pytorch import RenderFunction
    sc = scenes.bunny_box(device, resolution=(res, res))
    for s in sc.shapes:
        s.vertices.requires_grad_(True)
    target = torch.rand(res, res, 3, generator=torch.Generator().manual_seed(3)).to(device)
    losses = {'sum': lambda img: img.sum(), 'native': lambda img: gaussian_pyramid_loss(img, target, 5)}
    try:
        torch_loss = torch_loss_factory(3, 5, device)
        torch_loss(target, target * 0.5)
        losses['torch'] = lambda img: torch_loss(img, target)
    except Exception as e:
        print('bench_pyramid_loss: the torch formulation does not run on this device: %s' % type(e).__name__, flush=True)
    times = {name: [] for name in losses}
    for it in range(rounds):
        for name, f in losses.items():
            torch.cuda.synchronize()
            t0 = time.time()
            args = RenderFunction.serialize_scene(sc, spp, 4, sampler_type=rd.SamplerType.sobol, device=device, backend=rd)
            f(RenderFunction.apply(it + 1, *args)).backward()
            torch.cuda.synchronize()
            times[name].append(time.time() - t0)
    out = {'case': 'bunny_box %dx%d, %d spp, one iteration' % (res, res, spp)}
    for name, ts in times.items():
        ts = sorted(ts[2:])
        out[name + '_median_ms'] = ts[len(ts) // 2] * 1e3
    print('bunny_box %dx%d %d spp iteration: %s' % (res, res, spp, '   '.join(
        '%s loss %.2f ms' % (name, out[name + '_median_ms']) for name in losses)), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', nargs='+', default=['256x256x3x5', '1024x1024x3x5'], help='HEIGHTxWIDTHxCHANNELSxLEVELS')
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--out', default=None)
    ap.add_argument('--iteration', action='store_true', help='also one bunny_box iteration with each loss')
    ap.add_argument('--kernels-only', action='store_true', help='only the native steps, untimed: for a kernel trace')
    a = ap.parse_args()
    device = require_gpu('bench_pyramid_loss')
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
