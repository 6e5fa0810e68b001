#!/usr/bin/env python3
"""Specular highlights in deferred shading: what the fused lobe (rdr_deferred_specular, csrc/deferred_specular.h) costs, beside
the same definition composed from torch operations on the same GPU -- the only route to a specular term before the op existed --
and beside deferred_shade alone at the same size, for scale.

    python tools/bench_deferred_specular.py [--sizes 256 1024] [--aa 2 1] [--lights 1 4 8] [--iters 30] [--warmup 3] [--out FILE]

Per output size, aa and number of point lights, forward and forward + backward of:
    specular         deferred_specular: one launch forward; the adjoint and its fold backward
    torch_lobe       the definition of csrc/deferred_specular_abi.h as whole-image fp32 torch operations and their autograd
    deferred_shade   the diffuse pass with the same lights
The G-buffer is synthetic (alpha, a quarter of background), with the materials and the eye of tests/test_deferred_specular.py's
generator.  The steps alternate inside one process (tools/op_bench.py); median and 10th / 90th percentiles.  `hbm_fraction`: the
bytes the fused call must move (forward: 40 + 16 per texel read, 12 per pixel written; backward: the texels read once for their
own gradients and once per light, 56 per texel written) over its median time, as a share of 8 TB/s."""
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
from op_bench import emit, require_gpu, time_alternating          # noqa: E402


def inputs(size, aa, device):
    """g [1, size aa, size aa, 10], material [1, size aa, size aa, 4], eye [1, 3]"""
    gen = torch.Generator().manual_seed(size * 10 + aa)
    n = size * aa
    pos = (torch.rand(n, n, 3, generator=gen) * 2.0 - 1.0) * torch.tensor([1.0, 1.0, 0.1])
    nrm = torch.tensor([0.0, 0.0, 1.0]) + 0.6 * (torch.rand(n, n, 3, generator=gen) * 2.0 - 1.0)
    nrm = nrm / nrm.norm(dim=-1, keepdim=True) * (0.5 + 1.5 * torch.rand(n, n, 1, generator=gen))
    g = torch.cat([pos, nrm, 0.1 + 0.8 * torch.rand(n, n, 3, generator=gen), torch.rand(n, n, 1, generator=gen)], dim=-1)
    g[n // 2:, : n // 2, :] = 0.0                  # a quarter of background
    rough = torch.exp(math.log(0.02) + (math.log(1.5) - math.log(0.02)) * torch.rand(n, n, 1, generator=gen))
    mat = torch.cat([torch.rand(n, n, 3, generator=gen) * 1.1 - 0.1, rough], dim=-1)
    return g.unsqueeze(0).to(device).contiguous(), mat.unsqueeze(0).to(device).contiguous(), torch.tensor([[0.3, 0.2, 2.0]], device=device)


def point_lights(count, device):
    def t(v):
        return torch.tensor(v, dtype=torch.float32, device=device, requires_grad=True)
    return [ru.PointLight(t([-0.5 + 0.3 * k, 0.4 - 0.2 * k, 1.5 + 0.1 * k]), t([1.0 + 0.1 * k, 0.9, 0.8])) for k in range(count)]


def _g1(c, r):
    u = 1.0 / (c * c) - 1.0
    sloped = u > 0
    a = 1.0 / (torch.sqrt(r) * torch.sqrt(torch.where(sloped, u, torch.ones_like(u))))
    rational = (3.535 * a + 2.181 * a * a) / (1.0 + 2.276 * a + 2.577 * a * a)
    return torch.where(sloped & (a < 1.6), rational, torch.ones_like(a))


def torch_lobe(g, mat, eye, lights, aa):
    """the definition, one torch operation per step (gated texels get a harmless cosine, so that no NaN meets a zero)"""
    p, nrm, ks, rho = g[..., 0:3], g[..., 3:6], mat[..., 0:3], mat[..., 3]
    nn = (nrm * nrm).sum(-1)
    has_n = nn > 0
    nh = nrm / torch.sqrt(torch.where(has_n, nn, torch.ones_like(nn))).unsqueeze(-1)
    ev = eye[:, None, None, :] - p
    v = ev / ev.norm(dim=-1, keepdim=True)
    cv = (nh * v).sum(-1)
    r = torch.max(rho, torch.full_like(rho, 1e-3))
    e = torch.max(2.0 / r - 2.0, torch.zeros_like(r))
    k = torch.max(ks, torch.zeros_like(ks))
    rgb = torch.zeros_like(p)
    for light in lights:
        d = light.position - p
        r2 = (d * d).sum(-1, keepdim=True)
        l = d / torch.sqrt(r2)
        cl = (nh * l).sum(-1)
        hv = v + l
        m = hv / hv.norm(dim=-1, keepdim=True)
        cm = (nh * m).sum(-1)
        lit = has_n & (cv > 0) & (cl > 1e-3) & (cm > 0)
        half = torch.full_like(cv, 0.5)
        cvs, cls, cms = torch.where(lit, cv, half), torch.where(lit, cl, half), torch.where(lit, cm, half)
        D = torch.pow(cms, e) * (e + 2.0) / (2.0 * math.pi)
        q = torch.max(1.0 - (m * l).sum(-1).abs(), torch.zeros_like(cv))
        F = k + (1.0 - k) * (q ** 5).unsqueeze(-1)
        value = (light.intensity / r2) * F * (D * _g1(cvs, r) * _g1(cls, r) / (4.0 * cvs)).unsqueeze(-1)
        rgb = rgb + torch.where(lit.unsqueeze(-1), value, torch.zeros_like(value))
    img = torch.nn.functional.interpolate(rgb.permute(0, 3, 1, 2), size=(g.shape[1] // aa, g.shape[2] // aa), mode='area')
    return img.permute(0, 2, 3, 1)


def case(size, aa, count, device, iters, warmup):
    g, mat, eye = inputs(size, aa, device)
    g.requires_grad_(True), mat.requires_grad_(True), eye.requires_grad_(True)
    lights = point_lights(count, device)
    up3, up4 = torch.rand(1, size, size, 3, device=device), torch.rand(1, size, size, 4, device=device)
    calls = {'specular': (lambda: ru.deferred_specular(g, mat, lights, eye, alpha=True, aa_samples=aa), up3),
             'torch_lobe': (lambda: torch_lobe(g, mat, eye, lights, aa), up3),
             'deferred_shade': (lambda: ru.deferred_shade(g, lights, alpha=True, aa_samples=aa), up4)}

    def clear():
        for t in [g, mat, eye] + [x for light in lights for x in (light.position, light.intensity)]:
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

    res = {'size': size, 'aa_samples': aa, 'point_lights': count, 'alpha': True, 'iters': iters}
    with torch.no_grad():
        a, b = calls['specular'][0](), calls['torch_lobe'][0]()
        res['max_abs_difference_fused_torch'] = float((a - b).abs().max())
        res['largest_value'] = float(b.abs().max())
    res['a_forward'] = time_alternating({name: fwd(f) for name, (f, _) in calls.items()}, iters, warmup)
    res['b_forward_backward'] = time_alternating({name: both(f, up) for name, (f, up) in calls.items()}, iters, warmup)
    texels, pixels = (size * aa) ** 2, size * size
    moved = {'a_forward': 56 * texels + 12 * pixels, 'b_forward_backward': 56 * texels + 12 * pixels + 56 * texels * (2 + count) + 12 * pixels}
    res['hbm_fraction'] = {key: moved[key] / (res[key]['specular']['median_ms'] * 1e-3) / PEAK_BYTES_PER_S for key in moved}
    res['library'] = _capi.library_path()
    for key in ('a_forward', 'b_forward_backward'):
        for name, t in res[key].items():
            print('%4d^2 aa %d lights %d %-20s %-15s %8.3f ms [%7.3f, %7.3f]' % (size, aa, count, key, name, t['median_ms'], t['p10_ms'],
                                                                             t['p90_ms']), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[256, 1024])
    ap.add_argument('--aa', type=int, nargs='+', default=[2, 1])
    ap.add_argument('--lights', type=int, nargs='+', default=[1, 4, 8])
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    device = require_gpu('bench_deferred_specular')
    results = []
    for size in a.sizes:
        for aa in a.aa:
            for count in a.lights:
                results.append(case(size, aa, count, device, a.iters, a.warmup))
                print(json.dumps(results[-1]), flush=True)
    emit(results, a.out, echo=False)


if __name__ == '__main__':
    main()
