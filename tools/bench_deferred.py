#!/usr/bin/env python3
"""Deferred shading: the fused kernels (redner_amd.render_utils) against the same shading composed from torch operations, as the
reference composes it and as a user of this package had to before render_deferred existed.

    python tools/bench_deferred.py [--sizes 256 1024] [--iters 50] [--warmup 5] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_deferred.py --kernels-only     (kernel times, a run of its own)

Four lights (one of each type), alpha, aa_samples 2.  Per output size:
  (a) the shade step alone, forward            (b) the shade step alone, forward + backward
  (c) a whole render_deferred iteration, forward + backward, on tests/scenes.py: textured_sphere
Baseline and fused alternate inside one process, both warmed up; every call sits in its own pair of device events; the median
and the 10th / 90th percentiles are reported.  `algorithmic_bytes` is what the fused kernels must move (forward 40 B per texel
+ 16 B per pixel; backward 80 B per texel + 16 B per pixel + the slab of partial sums); over a KERNEL time (--kernels-only under
the profiler) it gives the share of the 8 TB/s roofline -- over the call times printed here it is an end-to-end rate that
includes the launch, the allocation of the outputs and the synchronisation.
"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]

from redner_amd import render_utils as ru          # noqa: E402
from op_bench import emit, require_gpu, time_alternating          # noqa: E402

AA = 2
PEAK_BYTES_PER_S = 8.0e12


def make_lights(device):
    """-> [(kind, {name: leaf tensor})] and the matching redner_amd light objects (sharing the tensors)"""
    def t(v):
        return torch.tensor(v, dtype=torch.float32, device=device, requires_grad=True)
    spec = [('ambient', {'intensity': t([0.2, 0.2, 0.25])}),
            ('point', {'position': t([1.0, 2.0, -3.0]), 'intensity': t([40.0, 35.0, 30.0])}),
            ('directional', {'direction': t([0.3, -0.5, 1.0]), 'intensity': t([0.8, 0.9, 1.1])}),
            ('spot', {'position': t([-2.0, 1.0, -4.0]), 'spot_direction': t([2.0, -1.0, 4.0]), 'spot_exponent': t([2.0]),
                      'intensity': t([6.0, 5.0, 4.0])})]
    cls = {'ambient': ru.AmbientLight, 'point': ru.PointLight, 'directional': ru.DirectionalLight, 'spot': ru.SpotLight}
    return spec, [cls[k](**p) for k, p in spec]


# ---- the baseline: one torch operation per step of the shading table (redner_amd/render_utils.py), whole-image tensors ----------
def torch_light(kind, p, pos, normal, albedo):
    inten = p['intensity']
    if kind == 'ambient':
        return inten * albedo
    if kind == 'directional':
        l = (-p['direction'] / torch.norm(p['direction'])).view(1, 1, 3)
        cos = torch.sum(l * normal, dim=-1, keepdim=True)
        cos = torch.max(cos, torch.zeros_like(cos))
        return inten * cos * (albedo / math.pi)
    d = p['position'] - pos
    if kind == 'point':
        dd = torch.sum(d * d, dim=-1, keepdim=True)
        l = d / torch.sqrt(dd)
        cos = torch.sum(l * normal, dim=-1, keepdim=True)
        cos = torch.max(cos, torch.zeros_like(cos))
        return inten * cos * (albedo / math.pi) / dd
    l = d / torch.norm(d, dim=-1, keepdim=True)
    s = -p['spot_direction'] / torch.norm(p['spot_direction'])
    spot = torch.sum(l * s, dim=-1, keepdim=True)
    spot = torch.pow(torch.max(spot, torch.zeros_like(spot)), p['spot_exponent'])
    cos = torch.sum(l * normal, dim=-1, keepdim=True)
    cos = torch.max(cos, torch.zeros_like(cos))
    return inten * spot * cos * (albedo / math.pi)


def torch_shade(g, spec, aa):
    """g [Hg, Wg, 10] -> [H, W, 4]"""
    pos, normal, albedo = g[:, :, :3], g[:, :, 3:6], g[:, :, 6:9]
    img = torch.zeros(g.shape[0], g.shape[1], 3, device=g.device)
    for kind, p in spec:
        img = img + torch_light(kind, p, pos, normal, albedo)
    img = torch.cat((img, g[:, :, 9:10]), dim=-1)
    img = img.permute(2, 0, 1).unsqueeze(0)
    img = torch.nn.functional.interpolate(img, size=(g.shape[0] // aa, g.shape[1] // aa), mode='area')
    return img.squeeze(0).permute(1, 2, 0)


def synthetic_g_buffer(size, device):
    gen = torch.Generator().manual_seed(size)
    n = size * AA
    pos = torch.rand(n, n, 3, generator=gen) * torch.tensor([4.0, 4.0, 1.5]) + torch.tensor([-2.0, -2.0, 0.5])
    nrm = torch.randn(n, n, 3, generator=gen)
    nrm = nrm / nrm.norm(dim=-1, keepdim=True)
    g = torch.cat([pos, nrm, 0.1 + 0.8 * torch.rand(n, n, 3, generator=gen), torch.rand(n, n, 1, generator=gen)], dim=-1)
    g[n // 2:, : n // 2, :] = 0.0                  # a quarter of background
    return g.to(device).contiguous()


def clear_grads(spec, *tensors):
    for _, p in spec:
        for t in p.values():
            t.grad = None
    for t in tensors:
        t.grad = None


def algorithmic_bytes(size, num_lights):
    texels, pixels = (size * AA) ** 2, size * size
    blocks = min((pixels + 255) // 256, 2048)
    return {'forward': 40 * texels + 16 * pixels, 'backward': 80 * texels + 16 * pixels + 2 * blocks * num_lights * 10 * 8}


def shade_cases(size, device, iters, warmup):
    spec, lights = make_lights(device)
    g = synthetic_g_buffer(size, device).requires_grad_(True)
    up = torch.rand(size, size, 4, device=device)
    with torch.no_grad():
        err = float((torch_shade(g, spec, AA) - ru.deferred_shade(g.unsqueeze(0), lights, alpha=True, aa_samples=AA)[0]).abs().max())

    def fwd_torch():
        with torch.no_grad():
            return torch_shade(g, spec, AA)

    def fwd_fused():
        with torch.no_grad():
            return ru.deferred_shade(g.unsqueeze(0), lights, alpha=True, aa_samples=AA)

    def both_torch():
        clear_grads(spec, g)
        torch_shade(g, spec, AA).backward(up)

    def both_fused():
        clear_grads(spec, g)
        ru.deferred_shade(g.unsqueeze(0), lights, alpha=True, aa_samples=AA)[0].backward(up)

    return {'max_abs_difference_of_images': err,
            'a_shade_forward': time_alternating({'torch': fwd_torch, 'fused': fwd_fused}, iters, warmup),
            'b_shade_forward_backward': time_alternating({'torch': both_torch, 'fused': both_fused}, iters, warmup)}


def whole_iteration_case(size, device, iters, warmup):
    import scenes
    from redner_amd import redner
    sc = scenes.textured_sphere(device, resolution=(size, size))
    spec, lights = make_lights(device)
    channels = [redner.channels.position, redner.channels.shading_normal, redner.channels.diffuse_reflectance, redner.channels.alpha]
    up = torch.rand(size, size, 4, device=device)
    leaves = [sh.vertices for sh in sc.shapes if sh.vertices.requires_grad]

    def it_torch():
        clear_grads(spec, *leaves)
        g = ru._render_g_buffer_for_deferred(sc, 1, channels, AA, False, True, device, redner)
        torch_shade(g, spec, AA).backward(up)

    def it_fused():
        clear_grads(spec, *leaves)
        ru.render_deferred(sc, lights, alpha=True, aa_samples=AA, seed=1, device=device).backward(up)

    return {'c_render_deferred_forward_backward': time_alternating({'torch': it_torch, 'fused': it_fused}, iters, warmup)}


def kernels_only(sizes, device, reps):
    """fused forward + backward only, for a kernel trace"""
    for size in sizes:
        spec, lights = make_lights(device)
        g = synthetic_g_buffer(size, device).requires_grad_(True)
        up = torch.rand(size, size, 4, device=device)
        for _ in range(reps):
            clear_grads(spec, g)
            ru.deferred_shade(g.unsqueeze(0), lights, alpha=True, aa_samples=AA)[0].backward(up)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[256, 1024])
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--skip-whole-iteration', action='store_true')
    a = ap.parse_args()
    device = require_gpu('bench_deferred')
    if a.kernels_only:
        kernels_only(a.sizes, device, 20)
        return
    results = []
    for size in a.sizes:
        res = {'size': size, 'aa_samples': AA, 'alpha': True, 'lights': 4, 'iters': a.iters,
               'algorithmic_bytes': algorithmic_bytes(size, 4)}
        res.update(shade_cases(size, device, a.iters, a.warmup))
        if not a.skip_whole_iteration:
            res.update(whole_iteration_case(size, device, a.iters, a.warmup))
        for key in ('a_shade_forward', 'b_shade_forward_backward', 'c_render_deferred_forward_backward'):
            if key not in res:
                continue
            t, f = res[key]['torch'], res[key]['fused']
            spread = max(t['p90_ms'] - t['p10_ms'], f['p90_ms'] - f['p10_ms'])
            res[key]['speedup'] = t['median_ms'] / f['median_ms']
            res[key]['fused_no_slower_beyond_spread'] = f['median_ms'] <= t['median_ms'] + spread
            print('%4d^2 %-36s torch %8.3f ms [%7.3f, %7.3f]   fused %8.3f ms [%7.3f, %7.3f]   x%.2f'
                  % (size, key, t['median_ms'], t['p10_ms'], t['p90_ms'], f['median_ms'], f['p10_ms'], f['p90_ms'], res[key]['speedup']),
                  flush=True)
        b = res['algorithmic_bytes']
        fa = res['a_shade_forward']['fused']['median_ms'] * 1e-3
        res['forward_call_rate_share_of_8TBps'] = b['forward'] / fa / PEAK_BYTES_PER_S
        results.append(res)
        print(json.dumps(res), flush=True)
    emit(results, a.out, echo=False)


if __name__ == '__main__':
    main()
