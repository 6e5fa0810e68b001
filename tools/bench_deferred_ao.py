#!/usr/bin/env python3
"""Deferred shading with ambient occlusion: what the K hemisphere rays per texel of `deferred_shade(ambient_occlusion=K)` cost on
top of the shade step.

    python tools/bench_deferred_ao.py [--sizes 256 1024] [--rays 4 16 32] [--radius-share 0.1] [--iters 30] [--warmup 3]
                                      [--out FILE] [--unoccluded-only]

The G-buffer is tests/scenes.py: bunny_box rendered at aa_samples 2 (position, shading normal, diffuse reflectance, alpha), the
occluders are the same scene (14 416 triangles), the lights an AmbientLight and an SHLight of nine coefficients (four rows of
the light table, all of them sky rows).  bunny_box is a CLOSED box, so the radius is finite: --radius-share of the diagonal of
the scene's bounding box (the file states the length).  Per output size:
  (a) the shade step alone, forward              plain / K = each of --rays
  (b) the shade step alone, forward + backward   plain / K = each of --rays
  (c) the backward call alone                    plain / occluded (largest K): one more word read per texel
The steps alternate inside one process (tools/op_bench.py); median and 10th / 90th percentiles.  Then the any-hit launches of
each occluded forward call, from the library's own trace statistics (tools/bench_deferred_shadows.py: any_hit_rate).
--unoccluded-only times the plain and the shadowed calls with the four lights of tools/bench_deferred.py and uses nothing that a
build without occlusion lacks, so the same tool measures such a build (REDNER_AMD_LIB=<its library>).
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]

from redner_amd import _capi, render_utils as ru                     # noqa: E402
from bench_deferred import AA, clear_grads, make_lights              # noqa: E402
from bench_deferred_shadows import any_hit_rate, bunny_g_buffer      # noqa: E402
from op_bench import emit, require_gpu, summary, time_alternating    # noqa: E402


def sky_lights(device):
    inten = torch.tensor([0.3, 0.35, 0.4], device=device, requires_grad=True)
    coeffs = (0.3 * torch.randn(3, 9, generator=torch.Generator().manual_seed(5)) + torch.tensor([1.0] + [0.0] * 8)).to(device)
    coeffs.requires_grad_(True)
    return [inten, coeffs], [ru.AmbientLight(inten), ru.SHLight(coeffs)]


def scene_diagonal(sc):
    lo = torch.stack([s.vertices.detach().min(dim=0).values for s in sc.shapes]).min(dim=0).values
    hi = torch.stack([s.vertices.detach().max(dim=0).values for s in sc.shapes]).max(dim=0).values
    return float((hi - lo).norm())


def unoccluded_case(size, device, iters, warmup):
    """the calls that exist without occlusion: plain and shadows-only, four lights"""
    spec, lights = make_lights(device)
    sc, g = bunny_g_buffer(size, device)
    g.requires_grad_(True)
    up = torch.rand(1, size, size, 4, device=device)
    occ = ru.occluder_scene(sc, device=device)

    def fwd(kw):
        def step():
            with torch.no_grad():
                return ru.deferred_shade(g, lights, alpha=True, aa_samples=AA, **kw)
        return step

    def both(kw):
        def step():
            clear_grads(spec, g)
            ru.deferred_shade(g, lights, alpha=True, aa_samples=AA, **kw).backward(up)
        return step

    kinds = {'plain': {}, 'shadowed': {'occluders': occ}}
    res = {'size': size, 'aa_samples': AA, 'alpha': True, 'lights': 4, 'iters': iters, 'scene': 'bunny_box',
           'library': _capi.library_path()}
    res['a_shade_forward'] = time_alternating({k: fwd(kw) for k, kw in kinds.items()}, iters, warmup)
    res['b_shade_forward_backward'] = time_alternating({k: both(kw) for k, kw in kinds.items()}, iters, warmup)
    return res


def case(size, device, iters, warmup, rays, radius_share):
    leaves, lights = sky_lights(device)
    sc, g = bunny_g_buffer(size, device)
    g.requires_grad_(True)
    up = torch.rand(1, size, size, 4, device=device)
    occ = ru.occluder_scene(sc, device=device)
    radius = radius_share * scene_diagonal(sc)

    def keywords(k):
        return {} if k == 0 else {'ambient_occlusion': k, 'ao_radius': radius, 'ao_occluders': occ}

    def fwd(k):
        def step():
            with torch.no_grad():
                return ru.deferred_shade(g, lights, alpha=True, aa_samples=AA, **keywords(k))
        return step

    def both(k):
        def step():
            clear_grads([], g, *leaves)
            ru.deferred_shade(g, lights, alpha=True, aa_samples=AA, **keywords(k)).backward(up)
        return step

    def backward_only(k):
        def step():
            clear_grads([], g, *leaves)
            img = ru.deferred_shade(g, lights, alpha=True, aa_samples=AA, **keywords(k))
            torch.cuda.synchronize()
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            img.backward(up)
            end.record()
            torch.cuda.synchronize()
            return start.elapsed_time(end)
        return step

    name = lambda k: 'plain' if k == 0 else 'K%d' % k
    res = {'size': size, 'aa_samples': AA, 'alpha': True, 'lights': 'ambient + SHLight (4 rows)', 'iters': iters, 'scene': 'bunny_box',
           'ao_radius': radius, 'scene_diagonal': scene_diagonal(sc), 'library': _capi.library_path(), 'texels': int(g.shape[1] * g.shape[2])}
    res['a_shade_forward'] = time_alternating({name(k): fwd(k) for k in [0] + rays}, iters, warmup)
    res['b_shade_forward_backward'] = time_alternating({name(k): both(k) for k in [0] + rays}, iters, warmup)
    steps = {name(k): backward_only(k) for k in (0, max(rays))}
    times = {n: [] for n in steps}
    for it in range(warmup + iters):
        for n, f in steps.items():
            t = f()
            if it >= warmup:
                times[n].append(t)
    res['c_backward_alone'] = {n: summary(ts) for n, ts in times.items()}
    res['any_hit_launches_of_the_forward_call'] = {}
    for k in rays:
        with torch.no_grad():
            _, words = ru.deferred_shade(g, lights, alpha=True, aa_samples=AA, return_occlusion=True, **keywords(k))
        bits = sum(((words >> b) & 1) for b in range(k))
        rate = any_hit_rate(fwd(k), 5)
        rate['rays_per_call'] = rate['any_rays'] // rate['calls']
        rate['mean_occlusion_factor'] = float(bits.double().mean()) / k
        res['any_hit_launches_of_the_forward_call'][name(k)] = rate
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[256, 1024])
    ap.add_argument('--rays', type=int, nargs='+', default=[4, 16, 32])
    ap.add_argument('--radius-share', type=float, default=0.1)
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('--unoccluded-only', action='store_true')
    a = ap.parse_args()
    device = require_gpu('bench_deferred_ao')
    results = []
    for size in a.sizes:
        res = unoccluded_case(size, device, a.iters, a.warmup) if a.unoccluded_only else \
            case(size, device, a.iters, a.warmup, a.rays, a.radius_share)
        for key in ('a_shade_forward', 'b_shade_forward_backward', 'c_backward_alone'):
            for name, t in res.get(key, {}).items():
                print('%4d^2 %-26s %-9s %8.3f ms [%7.3f, %7.3f]' % (size, key, name, t['median_ms'], t['p10_ms'], t['p90_ms']), flush=True)
        results.append(res)
        print(json.dumps(res), flush=True)
    emit(results, a.out, echo=False)


if __name__ == '__main__':
    main()
