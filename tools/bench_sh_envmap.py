#!/usr/bin/env python3
"""One step of an environment-map fit from spherical-harmonic coefficients: the native kernels (redner_amd.SH_reconstruct,
redner_amd.EnvironmentMap on rdr_sh_reconstruct / rdr_envmap_tables) against the same step composed from torch operations on
the same device, as a user of this package had to before they existed.

    python tools/bench_sh_envmap.py [--cases 128x128x4 1024x2048x8] [--iters 50] [--warmup 5] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_sh_envmap.py --kernels-only      (kernel times, a run of its own)

A step is "coeffs [3, L^2] -> EnvironmentMap ready (image, mip pyramid, sampling tables) -> the gradient of a given gradient of
every pyramid level back in coeffs.grad".  The pyramid is the native one on both sides (redner_amd.Texture).  The baseline
composes the image from elementwise torch operations per basis function (the recurrence and the loop over (l, m) of the
definition in csrc/sh_envmap.h, the angles copied from the host on every call) and builds the tables with
render_pytorch.EnvironmentMap (torch.cumsum on the device).  Baseline and native alternate inside one process, both warmed up;
every step sits in its own pair of device events; the median and the 10th / 90th percentiles are reported.  These are STEP
times: launches, allocations, autograd and the Python around them included.  Launches per step are counted by torch.profiler
(device kernels and copies of one step; `null` where the profiler reports none).
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tools')]

import redner_amd                                   # noqa: E402
from redner_amd import render_pytorch               # noqa: E402
from op_bench import count_launches, emit, require_gpu, time_alternating          # noqa: E402


def _legendre(l, m, x):
    pmm = torch.ones_like(x)
    if m > 0:
        root = torch.sqrt((1 - x) * (1 + x))
        for k in range(1, m + 1):
            pmm = pmm * (-(2.0 * k - 1.0)) * root
    if l == m:
        return pmm
    upper = x * (2.0 * m + 1.0) * pmm
    for ll in range(m + 2, l + 1):
        pmm, upper = upper, ((2.0 * ll - 1.0) * x * upper - (ll + m - 1.0) * pmm) / (ll - m)
    return upper


def torch_sh_reconstruct(coeffs, res):
    """The baseline: csrc/sh_envmap.h's definition composed from torch operations, one basis function at a time."""
    rows, cols = np.mgrid[0:res[0], 0:res[1]].astype(np.float32)
    theta = torch.from_numpy((math.pi / res[0]) * (rows + 0.5)).to(coeffs.device)
    phi = torch.from_numpy((2 * math.pi / res[1]) * (cols + 0.5)).to(coeffs.device)
    x = torch.cos(theta)
    out = torch.zeros(res[0], res[1], coeffs.shape[0], device=coeffs.device)
    i = 0
    for l in range(int(math.sqrt(coeffs.shape[1]))):
        for m in range(-l, l + 1):
            a = abs(m)
            k = math.sqrt((2.0 * l + 1.0) * math.factorial(l - a) / (4 * math.pi * math.factorial(l + a)))
            if m == 0:
                y = k * _legendre(l, 0, x)
            elif m > 0:
                y = math.sqrt(2.0) * k * torch.cos(m * phi) * _legendre(l, a, x)
            else:
                y = math.sqrt(2.0) * k * torch.sin(a * phi) * _legendre(l, a, x)
            out = out + y[:, :, None] * coeffs[:, i]
            i += 1
    return torch.max(out, torch.zeros_like(out))


def make_steps(res, bands, device):
    gen = torch.Generator().manual_seed(5)
    start = 0.3 * torch.randn(3, bands * bands, generator=gen)
    start[:, 0] += 0.6
    coeffs = {name: start.clone().to(device).requires_grad_(True) for name in ('torch', 'native')}
    sizes = [tuple(l.shape) for l in redner_amd.Texture(torch.zeros(res[0], res[1], 3, device=device)).mipmap]
    grads = [torch.randn(*s, generator=gen).to(device) for s in sizes]

    def step_torch():
        c = coeffs['torch']
        c.grad = None
        env = render_pytorch.EnvironmentMap(redner_amd.Texture(torch_sh_reconstruct(c, res)))
        torch.autograd.backward(env.values.mipmap, grads)
        return env

    def step_native():
        c = coeffs['native']
        c.grad = None
        env = redner_amd.EnvironmentMap(redner_amd.SH_reconstruct(c, res))
        torch.autograd.backward(env.values.mipmap, grads)
        return env

    return coeffs, step_torch, step_native


def run_case(spec, device, iters, warmup):
    h, w, bands = (int(s) for s in spec.split('x'))
    coeffs, step_torch, step_native = make_steps((h, w), bands, device)
    a, b = step_torch(), step_native()
    torch.cuda.synchronize()
    res = {'case': spec, 'iters': iters,
           'image_max_abs_difference': float((a.values.mipmap[0] - b.values.mipmap[0]).abs().max()),
           'grad_rel_difference': float((coeffs['torch'].grad - coeffs['native'].grad).norm() / coeffs['torch'].grad.norm()),
           'tables_equal': bool(torch.equal(a.sample_cdf_xs, b.sample_cdf_xs) and torch.equal(a.sample_cdf_ys, b.sample_cdf_ys)),
           'step': time_alternating({'torch': step_torch, 'native': step_native}, iters, warmup),
           'launches': {'torch': count_launches(step_torch, 'bench_sh_envmap'), 'native': count_launches(step_native, 'bench_sh_envmap')}}
    r = res['step']
    r['ratio'] = r['torch']['median_ms'] / r['native']['median_ms']
    print('%-14s step  torch %8.3f ms [%7.3f, %7.3f] %s launches   native %7.3f ms [%6.3f, %6.3f] %s launches   x%.1f'
          % (spec, r['torch']['median_ms'], r['torch']['p10_ms'], r['torch']['p90_ms'], res['launches']['torch'],
             r['native']['median_ms'], r['native']['p10_ms'], r['native']['p90_ms'], res['launches']['native'], r['ratio']), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', nargs='+', default=['128x128x4', '1024x2048x8'], help='HEIGHTxWIDTHxBANDS')
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--kernels-only', action='store_true', help='only the native steps, untimed: for a kernel trace')
    a = ap.parse_args()
    device = require_gpu('bench_sh_envmap')
    if a.kernels_only:
        for spec in a.cases:
            h, w, bands = (int(s) for s in spec.split('x'))
            step_native = make_steps((h, w), bands, device)[2]
            for _ in range(a.iters):
                step_native()
            torch.cuda.synchronize()
        return
    emit([run_case(spec, device, a.iters, a.warmup) for spec in a.cases], a.out)


if __name__ == '__main__':
    main()
