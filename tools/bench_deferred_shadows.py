#!/usr/bin/env python3
"""Deferred shading with shadows: what the any-hit shadow rays of `deferred_shade(occluders=...)` cost on top of the shade step.

    python tools/bench_deferred_shadows.py [--sizes 256 1024] [--iters 30] [--warmup 3] [--out FILE] [--unshadowed-only]

The G-buffer is tests/scenes.py: bunny_box rendered at aa_samples 2 (position, shading normal, diffuse reflectance, alpha), the
occluders are the same scene (14 416 triangles), the lights are the four of tools/bench_deferred.py.  Per output size:
  (a) the shade step alone, forward              without / with occluders
  (b) the shade step alone, forward + backward   without / with occluders
The steps alternate inside one process (tools/op_bench.py); median and 10th / 90th percentiles.  Then the any-hit launches of the
shadowed forward call alone, from the library's own trace statistics (device events around every traversal launch, rays tallied
by the counting kernels in a run of their own): rays, time, rays/s.  --unshadowed-only times the calls without occluders only
and uses nothing that a build without shadows lacks, so the same tool measures such a build (REDNER_AMD_LIB=<its library>).
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]

from redner_amd import _capi, redner, render_utils as ru          # noqa: E402
from bench_deferred import AA, clear_grads, make_lights          # noqa: E402
from op_bench import emit, require_gpu, time_alternating          # noqa: E402


def bunny_g_buffer(size, device):
    import scenes
    sc = scenes.bunny_box(device, resolution=(size * AA, size * AA), vertex_grad=False)
    channels = [redner.channels.position, redner.channels.shading_normal, redner.channels.diffuse_reflectance, redner.channels.alpha]
    g = ru.render_g_buffer(sc, channels, seed=1, device=device).detach().unsqueeze(0).contiguous()
    return sc, g


def any_hit_rate(step, reps):
    """rays, milliseconds and launches of the any-hit traversal launches of `reps` calls of step(): the rays from a run with the
    counting kernels (exact tallies, slower kernels), the time from a run with device events only (the kernels every call runs)"""
    lib = _capi.lib()
    got = {}
    for counting in (1, 0):
        lib.rdr_trace_stats_enable(1, counting)
        lib.rdr_trace_stats_reset()
        for _ in range(reps):
            step()
        torch.cuda.synchronize()
        st = _capi.TraceStats()
        lib.rdr_trace_stats_get(C.byref(st))
        got[counting] = (int(st.any_launches), int(st.any_rays), float(st.any_ms))
    lib.rdr_trace_stats_enable(0, 0)
    lib.rdr_trace_stats_reset()
    rays, ms = got[1][1], got[0][2]
    return {'calls': reps, 'any_launches': got[0][0], 'any_rays': rays, 'queue_slots_launched': got[0][1], 'any_ms': ms,
            'any_ms_with_counting_kernels': got[1][2], 'any_rays_per_s': rays / (ms * 1e-3) if ms > 0 else None}


def case(size, device, iters, warmup, unshadowed_only):
    spec, lights = make_lights(device)
    sc, g = bunny_g_buffer(size, device)
    g.requires_grad_(True)
    up = torch.rand(1, size, size, 4, device=device)
    occ = None if unshadowed_only else ru.occluder_scene(sc, device=device)

    def fwd(occluders):
        def step():
            with torch.no_grad():
                if occluders is None:
                    return ru.deferred_shade(g, lights, alpha=True, aa_samples=AA)
                return ru.deferred_shade(g, lights, alpha=True, aa_samples=AA, occluders=occluders)
        return step

    def both(occluders):
        def step():
            clear_grads(spec, g)
            if occluders is None:
                ru.deferred_shade(g, lights, alpha=True, aa_samples=AA).backward(up)
            else:
                ru.deferred_shade(g, lights, alpha=True, aa_samples=AA, occluders=occluders).backward(up)
        return step

    forward, forward_backward = {'plain': fwd(None)}, {'plain': both(None)}
    res = {'size': size, 'aa_samples': AA, 'alpha': True, 'lights': 4, 'iters': iters, 'scene': 'bunny_box',
           'library': _capi.library_path()}
    if occ is not None:
        forward['shadowed'], forward_backward['shadowed'] = fwd(occ), both(occ)
        with torch.no_grad():
            _, vis = ru.deferred_shade(g, lights, alpha=True, aa_samples=AA, occluders=occ, return_visibility=True)
        words = vis.view(-1)
        res['texels'] = int(words.numel())
        res['texels_with_a_blocked_light'] = int((words != 15).sum())
    res['a_shade_forward'] = time_alternating(forward, iters, warmup)
    res['b_shade_forward_backward'] = time_alternating(forward_backward, iters, warmup)
    if occ is not None:
        res['any_hit_launches_of_the_forward_call'] = any_hit_rate(forward['shadowed'], 5)
    for key in ('a_shade_forward', 'b_shade_forward_backward'):
        for name, t in res[key].items():
            print('%4d^2 %-26s %-9s %8.3f ms [%7.3f, %7.3f]' % (size, key, name, t['median_ms'], t['p10_ms'], t['p90_ms']), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[256, 1024])
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('--unshadowed-only', action='store_true')
    a = ap.parse_args()
    device = require_gpu('bench_deferred_shadows')
    results = []
    for size in a.sizes:
        results.append(case(size, device, a.iters, a.warmup, a.unshadowed_only))
        print(json.dumps(results[-1]), flush=True)
    emit(results, a.out, echo=False)


if __name__ == '__main__':
    main()
