#!/usr/bin/env python3
"""SHLight in deferred shading: what a spherical-harmonic environment light costs in the fused shade step, beside the four
existing lights, beside three directional lights (the same number of table rows) and beside the same formula composed from torch
operations on the G-buffer -- what a user wrote before the light existed.

    python tools/bench_deferred_sh.py [--sizes 256 1024] [--iters 30] [--warmup 3] [--out FILE] [--four-lights-only]

The G-buffer and the four lights are those of tools/bench_deferred.py (synthetic, alpha, aa_samples 2).  Per output size, forward
and forward + backward of the shade step alone:
    four_lights          ambient, point, directional, spot
    three_directional    three rows of the cheapest light with a cosine
    sh_light             one SHLight ([3, 9] coefficients: three rows)
    four_plus_sh         the four lights and the SHLight
    torch_sh             the SHLight's formula as whole-image torch operations and their autograd
The steps alternate inside one process (tools/op_bench.py); median and 10th / 90th percentiles.  --four-lights-only times the
first step alone and uses no SH row, so the same tool measures a library built before the light existed
(REDNER_AMD_LIB=<that library>).
"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]

from redner_amd import _capi, render_utils as ru          # noqa: E402
from bench_deferred import AA, clear_grads, make_lights, synthetic_g_buffer          # noqa: E402
from op_bench import emit, require_gpu, time_alternating          # noqa: E402

K0, K1, K2 = 0.5 * math.sqrt(1.0 / math.pi), math.sqrt(3.0 / (4.0 * math.pi)), 0.5 * math.sqrt(15.0 / math.pi)
K20, K22 = 0.25 * math.sqrt(5.0 / math.pi), 0.25 * math.sqrt(15.0 / math.pi)
LOBE = [math.pi] + [2.0 * math.pi / 3.0] * 3 + [math.pi / 4.0] * 5


def torch_sh(g, coeffs, aa):
    """g [Hg, Wg, 10], coeffs [3, 9] -> [H, W, 4]: the table of redner_amd/render_utils.py, one torch operation per step"""
    normal, albedo = g[:, :, 3:6], g[:, :, 6:9]
    x, y, z = -normal[:, :, 2], normal[:, :, 0], normal[:, :, 1]
    basis = torch.stack([torch.full_like(x, K0), -K1 * y, K1 * z, -K1 * x, K2 * x * y, -K2 * y * z, K20 * (3.0 * z * z - 1.0),
                         -K2 * x * z, K22 * (x * x - y * y)], dim=-1)
    irradiance = basis @ (coeffs * torch.tensor(LOBE, device=g.device)).t()
    img = torch.max(irradiance, torch.zeros_like(irradiance)) * (albedo / math.pi)
    img = torch.cat((img, g[:, :, 9:10]), dim=-1)
    img = img.permute(2, 0, 1).unsqueeze(0)
    img = torch.nn.functional.interpolate(img, size=(g.shape[0] // aa, g.shape[1] // aa), mode='area')
    return img.squeeze(0).permute(1, 2, 0)


def case(size, device, iters, warmup, four_only):
    spec, four = make_lights(device)
    g = synthetic_g_buffer(size, device).requires_grad_(True)
    up = torch.rand(size, size, 4, device=device)
    gen = torch.Generator().manual_seed(7)
    coeffs = ((torch.rand(3, 9, generator=gen) - 0.5) * torch.tensor([3.0] + [1.0] * 8)).to(device).requires_grad_(True)
    lists = {'four_lights': four}
    if not four_only:
        def d(v):
            return torch.tensor(v, dtype=torch.float32, device=device, requires_grad=True)
        lists['three_directional'] = [ru.DirectionalLight(d([0.3, -0.5, 1.0 + k]), d([0.8, 0.9, 1.1])) for k in range(3)]
        lists['sh_light'] = [ru.SHLight(coeffs)]
        lists['four_plus_sh'] = four + [ru.SHLight(coeffs)]

    def fwd(lights):
        def step():
            with torch.no_grad():
                return ru.deferred_shade(g.unsqueeze(0), lights, alpha=True, aa_samples=AA)
        return step

    def both(lights):
        def step():
            clear_grads(spec, g, coeffs)
            ru.deferred_shade(g.unsqueeze(0), lights, alpha=True, aa_samples=AA)[0].backward(up)
        return step

    forward = {name: fwd(lights) for name, lights in lists.items()}
    forward_backward = {name: both(lights) for name, lights in lists.items()}
    res = {'size': size, 'aa_samples': AA, 'alpha': True, 'iters': iters}
    if not four_only:
        def fwd_torch():
            with torch.no_grad():
                return torch_sh(g, coeffs, AA)

        def both_torch():
            clear_grads(spec, g, coeffs)
            torch_sh(g, coeffs, AA).backward(up)

        forward['torch_sh'], forward_backward['torch_sh'] = fwd_torch, both_torch
        with torch.no_grad():
            res['max_abs_difference_fused_torch_sh'] = float((fwd_torch() - forward['sh_light']()[0]).abs().max())
    res['a_shade_forward'] = time_alternating(forward, iters, warmup)
    res['b_shade_forward_backward'] = time_alternating(forward_backward, iters, warmup)
    res['library'] = _capi.library_path()                # (loaded by the first call)
    for key in ('a_shade_forward', 'b_shade_forward_backward'):
        for name, t in res[key].items():
            print('%4d^2 %-26s %-18s %8.3f ms [%7.3f, %7.3f]' % (size, key, name, t['median_ms'], t['p10_ms'], t['p90_ms']), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[256, 1024])
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('--four-lights-only', action='store_true')
    a = ap.parse_args()
    device = require_gpu('bench_deferred_sh')
    results = []
    for size in a.sizes:
        results.append(case(size, device, a.iters, a.warmup, a.four_lights_only))
        print(json.dumps(results[-1]), flush=True)
    emit(results, a.out, echo=False)


if __name__ == '__main__':
    main()
