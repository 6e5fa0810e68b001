#!/usr/bin/env python3
"""Soft shadows of the quad lights: what the K any-hit rays per texel and quad of `deferred_quad(occluders=..., shadow_rays=K)`
(rdr_deferred_quad_shadowed, csrc/deferred_quad_shadow.h) cost on top of the unshadowed call, beside ambient occlusion with the
same K, which casts as many rays per pass.

    python tools/bench_deferred_quad_shadows.py [--sizes 256 1024] [--aa 2 1] [--quads 1 4 8] [--rays 4 16 32] [--iters 30]
                                                [--warmup 3] [--out FILE] [--unshadowed-only]

The G-buffer is tests/scenes.py: bunny_box rendered at aa_samples times the size (position, shading normal, diffuse reflectance,
alpha); the occluders are the same scene (14 416 triangles); the quads hang under the ceiling of the box, facing down, side by
side.  Per size, aa and number of quads, alternating in one process (tools/op_bench.py), device events, median and 10th / 90th
percentiles:
  (a) forward              deferred_quad unshadowed / K = each of --rays
  (b) forward + backward   the same
  (c) deferred_shade of an AmbientLight, plain / ambient_occlusion = each of --rays (once per size and aa: no quads in it)
Then, per K, the any-hit launches of one shadowed forward call from the library's own trace statistics
(tools/bench_deferred_shadows.py: any_hit_rate) -- their share of the call is any_ms per call over the forward median -- and the
bytes of words and factors, 8 per (quad, texel).
--unshadowed-only times (a) and (b) of the unshadowed call alone and uses nothing a build without soft shadows lacks, so the
same tool measures such a build (REDNER_AMD_LIB=<its library>).
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]

from redner_amd import _capi, redner, render_utils as ru            # noqa: E402
from bench_deferred_ao import scene_diagonal                         # noqa: E402
from bench_deferred_shadows import any_hit_rate                      # noqa: E402
from op_bench import emit, require_gpu, time_alternating             # noqa: E402


def bunny_g_buffer(size, aa, device):
    import scenes
    sc = scenes.bunny_box(device, resolution=(size * aa, size * aa), vertex_grad=False)
    channels = [redner.channels.position, redner.channels.shading_normal, redner.channels.diffuse_reflectance, redner.channels.alpha]
    g = ru.render_g_buffer(sc, channels, seed=1, device=device).detach().unsqueeze(0).contiguous()
    return sc, g


def ceiling_quads(sc, count, device):
    """`count` quads side by side, 2 % of the box's height under its ceiling, facing down (cross(q1 - q0, q3 - q0) = -y)"""
    lo = torch.stack([s.vertices.detach().min(dim=0).values for s in sc.shapes]).min(dim=0).values.cpu()
    hi = torch.stack([s.vertices.detach().max(dim=0).values for s in sc.shapes]).max(dim=0).values.cpu()
    ext = hi - lo
    y = float(hi[1] - 0.02 * ext[1])
    z0, z1 = float(lo[2] + 0.35 * ext[2]), float(lo[2] + 0.65 * ext[2])
    lights = []
    for k in range(count):
        x0 = float(lo[0] + ext[0] * (0.1 + 0.8 * k / count))
        x1 = x0 + float(0.6 * 0.8 * ext[0] / count)
        corners = torch.tensor([[x0, y, z0], [x1, y, z0], [x1, y, z1], [x0, y, z1]], device=device, requires_grad=True)
        lights.append(ru.QuadLight(corners, torch.tensor([4.0 + 0.1 * k, 3.5, 3.0], device=device, requires_grad=True)))
    return lights


def case(size, aa, count, device, iters, warmup, rays, unshadowed_only, with_ao):
    sc, g = bunny_g_buffer(size, aa, device)
    g.requires_grad_(True)
    quads = ceiling_quads(sc, count, device)
    occ = ru.occluder_scene(sc, device=device)
    up3, up4 = torch.rand(1, size, size, 3, device=device), torch.rand(1, size, size, 4, device=device)
    texels = int(g.shape[1] * g.shape[2])

    def keywords(k):
        return {} if k == 0 else {'occluders': occ, 'shadow_rays': k}

    def clear():
        for t in [g] + [x for light in quads for x in (light.vertices, light.intensity)]:
            t.grad = None

    def fwd(k):
        def step():
            with torch.no_grad():
                return ru.deferred_quad(g, quads, alpha=True, aa_samples=aa, **keywords(k))
        return step

    def both(k):
        def step():
            clear()
            ru.deferred_quad(g, quads, alpha=True, aa_samples=aa, **keywords(k)).backward(up3)
        return step

    name = lambda k: 'unshadowed' if k == 0 else 'K%d' % k
    ks = [0] + ([] if unshadowed_only else rays)
    res = {'size': size, 'aa_samples': aa, 'quads': count, 'alpha': True, 'iters': iters, 'scene': 'bunny_box', 'texels': texels,
           'library': _capi.library_path(), 'bytes_of_words_and_factors': 8 * count * texels}
    res['a_forward'] = time_alternating({name(k): fwd(k) for k in ks}, iters, warmup)
    res['b_forward_backward'] = time_alternating({name(k): both(k) for k in ks}, iters, warmup)
    if not unshadowed_only:
        res['any_hit_launches_of_the_forward_call'] = {}
        for k in rays:
            with torch.no_grad():
                _, (words, factors) = ru.deferred_quad(g, quads, alpha=True, aa_samples=aa, return_visibility=True, **keywords(k))
            rate = any_hit_rate(fwd(k), 5)
            rate['rays_per_call'] = rate['any_rays'] // rate['calls']
            rate['mean_factor'] = float(factors.double().mean())
            rate['share_of_the_forward_call'] = (rate['any_ms'] / rate['calls']) / res['a_forward'][name(k)]['median_ms']
            res['any_hit_launches_of_the_forward_call'][name(k)] = rate
    if with_ao and not unshadowed_only:                # the same G-buffer under ambient occlusion: K rays per texel in one pass
        inten = torch.tensor([0.3, 0.35, 0.4], device=device, requires_grad=True)
        amb = [ru.AmbientLight(inten)]
        radius = 0.1 * scene_diagonal(sc)

        def ao_kw(k):
            return {} if k == 0 else {'ambient_occlusion': k, 'ao_radius': radius, 'ao_occluders': occ}

        def ao_fwd(k):
            def step():
                with torch.no_grad():
                    return ru.deferred_shade(g, amb, alpha=True, aa_samples=aa, **ao_kw(k))
            return step

        def ao_both(k):
            def step():
                g.grad, inten.grad = None, None
                ru.deferred_shade(g, amb, alpha=True, aa_samples=aa, **ao_kw(k)).backward(up4)
            return step

        ao_name = lambda k: 'plain' if k == 0 else 'ao_K%d' % k
        res['c_ambient_occlusion_forward'] = time_alternating({ao_name(k): ao_fwd(k) for k in [0] + rays}, iters, warmup)
        res['c_ambient_occlusion_forward_backward'] = time_alternating({ao_name(k): ao_both(k) for k in [0] + rays}, iters, warmup)
    for key in ('a_forward', 'b_forward_backward', 'c_ambient_occlusion_forward', 'c_ambient_occlusion_forward_backward'):
        for n, t in res.get(key, {}).items():
            print('%4d^2 aa %d quads %d %-36s %-11s %8.3f ms [%7.3f, %7.3f]' % (size, aa, count, key, n, t['median_ms'], t['p10_ms'],
                                                                           t['p90_ms']), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[256, 1024])
    ap.add_argument('--aa', type=int, nargs='+', default=[2, 1])
    ap.add_argument('--quads', type=int, nargs='+', default=[1, 4, 8])
    ap.add_argument('--rays', type=int, nargs='+', default=[4, 16, 32])
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('--unshadowed-only', action='store_true')
    a = ap.parse_args()
    device = require_gpu('bench_deferred_quad_shadows')
    results = []
    for size in a.sizes:
        for aa in a.aa:
            for n, count in enumerate(a.quads):
                results.append(case(size, aa, count, device, a.iters, a.warmup, a.rays, a.unshadowed_only, with_ao=(n == 0)))
                print(json.dumps(results[-1]), flush=True)
    emit(results, a.out, echo=False)


if __name__ == '__main__':
    main()
