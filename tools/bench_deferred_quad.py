#!/usr/bin/env python3
"""Quad lights in deferred shading: what the fused polygon irradiance (rdr_deferred_quad, csrc/deferred_quad.h) costs, beside the
same definition composed from torch operations on the same GPU -- the only route to an area light in the deferred pass before the
op existed -- and beside deferred_shade with as many point lights, for scale.

    python tools/bench_deferred_quad.py [--sizes 256 1024] [--aa 2 1] [--quads 1 4 8] [--iters 30] [--warmup 3] [--out FILE]

Per output size, aa and number of quads, forward and forward + backward of:
    quad             deferred_quad: one launch forward; the adjoint and its fold backward
    torch_quad       the definition of csrc/deferred_quad_abi.h as whole-image fp32 torch operations and their autograd
    deferred_shade   the diffuse pass with as many point lights as there are quads
The G-buffer is synthetic (alpha, a quarter of background) with the texels of tests/test_deferred_quad.py's generator; the quads
alternate between one high above the patch and one low and upright, which the horizon of many texels cuts.  The steps alternate
inside one process (tools/op_bench.py); median and 10th / 90th percentiles.  `hbm_fraction`: the bytes the fused call must move
(forward: 40 per texel read, 12 per pixel written; backward: the texels read once for their own gradients and once per quad, 40
per texel written) over its median time, as a share of 8 TB/s."""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]

from redner_amd import _capi, render_utils as ru          # noqa: E402
from bench_deferred import PEAK_BYTES_PER_S          # noqa: E402
from bench_deferred_specular import point_lights          # noqa: E402
from op_bench import emit, require_gpu, time_alternating          # noqa: E402


def inputs(size, aa, device):
    """g [1, size aa, size aa, 10]"""
    gen = torch.Generator().manual_seed(size * 10 + aa)
    n = size * aa
    pos = (torch.rand(n, n, 3, generator=gen) * 2.0 - 1.0) * torch.tensor([1.0, 1.0, 0.1])
    nrm = torch.tensor([0.0, 0.0, 1.0]) + 0.6 * (torch.rand(n, n, 3, generator=gen) * 2.0 - 1.0)
    nrm = nrm / nrm.norm(dim=-1, keepdim=True) * (0.5 + 1.5 * torch.rand(n, n, 1, generator=gen))
    g = torch.cat([pos, nrm, 0.1 + 0.8 * torch.rand(n, n, 3, generator=gen), torch.rand(n, n, 1, generator=gen)], dim=-1)
    g[n // 2:, : n // 2, :] = 0.0                  # a quarter of background
    return g.unsqueeze(0).to(device).contiguous()


def quad_lights(count, device):
    def t(v):
        return torch.tensor(v, dtype=torch.float32, device=device, requires_grad=True)
    lights = []
    for k in range(count):
        s = 0.1 * k
        if k % 2 == 0:                             # high above the patch, facing down
            corners = [[-1.0 + s, 0.0, 1.5], [-1.0 + s, 0.8, 1.6], [0.0 + s, 0.8, 1.7], [0.0 + s, 0.0, 1.6]]
        else:                                      # low and upright, facing +x
            corners = [[0.3 - s, -0.5, -0.15], [0.3 - s, 0.5, -0.15], [0.35 - s, 0.5, 0.65], [0.35 - s, -0.5, 0.65]]
        lights.append(ru.QuadLight(t(corners), t([1.0 + 0.1 * k, 0.9, 0.8]), two_sided=(k % 4 == 3)))
    return lights


def _dot(a, b):
    return (a * b).sum(-1)


def _edge(A, B, nh):
    c = torch.cross(B, A, dim=-1)
    cc = _dot(c, c)
    ok = cc > 0
    s = torch.sqrt(torch.where(ok, cc, torch.ones_like(cc)))
    value = torch.atan2(s, _dot(A, B)) * _dot(c, nh) / s
    return torch.where(ok, value, torch.zeros_like(value))


def torch_quad(g, lights, aa):
    """the definition, one torch operation per step (gated texels get a harmless divisor, so that no NaN meets a zero)"""
    p, nrm, alb = g[..., 0:3], g[..., 3:6], g[..., 6:9]
    nn = _dot(nrm, nrm)
    has = nn > 0
    nh = nrm / torch.sqrt(torch.where(has, nn, torch.ones_like(nn))).unsqueeze(-1)
    rgb = torch.zeros_like(p)
    for light in lights:
        r = [light.vertices[i] - p for i in range(4)]
        h = [_dot(nh, r[i]) for i in range(4)]
        S = torch.zeros_like(nn)
        leave, enter = torch.zeros_like(p), torch.zeros_like(p)
        crossed = torch.zeros_like(has)
        for i in range(4):
            j = (i + 1) % 4
            upA, upB = h[i] > 0, h[j] > 0
            exits, enters = upA & ~upB, ~upA & upB
            cut = exits | enters
            x = r[i] + (r[j] - r[i]) * (h[i] / torch.where(cut, h[i] - h[j], torch.ones_like(nn))).unsqueeze(-1)
            e = _edge(torch.where(enters.unsqueeze(-1), x, r[i]), torch.where(exits.unsqueeze(-1), x, r[j]), nh)
            S = S + torch.where(upA | upB, e, torch.zeros_like(e))
            leave, enter = torch.where(exits.unsqueeze(-1), x, leave), torch.where(enters.unsqueeze(-1), x, enter)
            crossed = crossed | cut
        arc = _edge(leave, enter, nh)
        S = S + torch.where(crossed, arc, torch.zeros_like(arc))
        F = (S.abs() if light.two_sided else torch.max(S, torch.zeros_like(S))) / 2.0
        value = light.intensity * (alb / math.pi) * F.unsqueeze(-1)
        rgb = rgb + torch.where(has.unsqueeze(-1), value, torch.zeros_like(value))
    img = torch.nn.functional.interpolate(rgb.permute(0, 3, 1, 2), size=(g.shape[1] // aa, g.shape[2] // aa), mode='area')
    return img.permute(0, 2, 3, 1)


def case(size, aa, count, device, iters, warmup):
    g = inputs(size, aa, device)
    g.requires_grad_(True)
    quads, points = quad_lights(count, device), point_lights(count, device)
    up3, up4 = torch.rand(1, size, size, 3, device=device), torch.rand(1, size, size, 4, device=device)
    calls = {'quad': (lambda: ru.deferred_quad(g, quads, alpha=True, aa_samples=aa), up3),
             'torch_quad': (lambda: torch_quad(g, quads, aa), up3),
             'deferred_shade': (lambda: ru.deferred_shade(g, points, alpha=True, aa_samples=aa), up4)}

    def clear():
        for t in [g] + [x for light in quads for x in (light.vertices, light.intensity)] + \
                [x for light in points for x in (light.position, light.intensity)]:
            t.grad = None

    def fwd(f):
        def step():
            with torch.no_grad():
                return f()
        return step

    def both(f, up):
        def step():
            clear()
            f().backward(up)
        return step

    res = {'size': size, 'aa_samples': aa, 'quads': count, 'alpha': True, 'iters': iters}
    with torch.no_grad():
        a, b = calls['quad'][0](), calls['torch_quad'][0]()
        res['max_abs_difference_fused_torch'] = float((a - b).abs().max())
        res['largest_value'] = float(b.abs().max())
    res['a_forward'] = time_alternating({name: fwd(f) for name, (f, _) in calls.items()}, iters, warmup)
    res['b_forward_backward'] = time_alternating({name: both(f, up) for name, (f, up) in calls.items()}, iters, warmup)
    texels, pixels = (size * aa) ** 2, size * size
    moved = {'a_forward': 40 * texels + 12 * pixels, 'b_forward_backward': 40 * texels + 12 * pixels + 40 * texels * (2 + count) + 12 * pixels}
    res['hbm_fraction'] = {key: moved[key] / (res[key]['quad']['median_ms'] * 1e-3) / PEAK_BYTES_PER_S for key in moved}
    res['library'] = _capi.library_path()
    for key in ('a_forward', 'b_forward_backward'):
        for name, t in res[key].items():
            print('%4d^2 aa %d quads %d %-20s %-15s %8.3f ms [%7.3f, %7.3f]' % (size, aa, count, key, name, t['median_ms'], t['p10_ms'],
                                                                            t['p90_ms']), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[256, 1024])
    ap.add_argument('--aa', type=int, nargs='+', default=[2, 1])
    ap.add_argument('--quads', type=int, nargs='+', default=[1, 4, 8])
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    device = require_gpu('bench_deferred_quad')
    results = []
    for size in a.sizes:
        for aa in a.aa:
            for count in a.quads:
                results.append(case(size, aa, count, device, a.iters, a.warmup))
                print(json.dumps(results[-1]), flush=True)
    emit(results, a.out, echo=False)


if __name__ == '__main__':
    main()
