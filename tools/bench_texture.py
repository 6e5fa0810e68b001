#!/usr/bin/env python3
"""The mip pyramid: the native kernels (redner_amd.texture) against the same pyramid composed from torch operations, as the
reference composes it (per level: circular pad, grouped 2 x 2 conv2d, interpolate(area), permuted copy; under autograd) and as a
user of this package had to before redner_amd.Texture existed.

    python tools/bench_texture.py [--sizes 256 1024] [--iters 50] [--warmup 5] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_texture.py --kernels-only      (kernel times, a run of its own)

Per size (H = W, C = 3):
  (a) the pyramid forward                      (b) forward + backward with an upstream gradient on every level
and once:
  (c) one iteration of a three-texture fit (diffuse, specular, roughness at 512 x 512) of tests/scenes.py: textured_sphere at
      256 x 256 x 4 spp, the pyramids rebuilt in the iteration; next to it the three pyramids alone (forward + backward), whose
      share of the iteration is reported for either side.
Torch composition and native calls alternate inside one process, both warmed up; every call sits in its own pair of device
events; the median and the 10th / 90th percentiles are reported.  `algorithmic_bytes`: level 0 read once, the levels 1.. written
once (mirrored backward: every level's gradient read, d_texels written); over a KERNEL time (--kernels-only under the profiler)
it gives the share of the 8 TB/s roofline.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]

from redner_amd import texture as tx          # noqa: E402
import op_bench                                # noqa: E402

PEAK_BYTES_PER_S = 8.0e12


def torch_mipmap(texels):
    """The op list of the reference's Texture.generate_mipmap."""
    h, w, c = texels.shape
    num_levels = min((max(h, w) - 1).bit_length() + 1, 8)
    box = torch.ones(c, 1, 2, 2, device=texels.device) / 4.0
    mipmap = [texels.contiguous()]
    prev = texels.unsqueeze(0).permute(0, 3, 1, 2)
    for _ in range(1, num_levels):
        cur = torch.nn.functional.pad(prev, (0, 1, 0, 1), mode='circular')
        cur = torch.nn.functional.conv2d(cur, box, groups=c)
        cur = torch.nn.functional.interpolate(cur, size=(max(cur.shape[2] // 2, 1), max(cur.shape[3] // 2, 1)), mode='area')
        mipmap.append(cur.squeeze(0).permute(1, 2, 0).contiguous())
        prev = cur
    return mipmap


def against_torch(base, native, iters, warmup):
    out = op_bench.time_alternating({'torch': base, 'native': native}, iters, warmup)
    t, f = out['torch'], out['native']
    spread = max(t['p90_ms'] - t['p10_ms'], f['p90_ms'] - f['p10_ms'])
    out['speedup'] = t['median_ms'] / f['median_ms']
    out['native_faster_beyond_spread'] = f['median_ms'] + spread < t['median_ms']
    return out


def report(label, key, r):
    t, f = r['torch'], r['native']
    print('%-10s %-34s torch %8.3f ms [%7.3f, %7.3f]   native %8.3f ms [%7.3f, %7.3f]   x%.2f   beyond spread: %s'
          % (label, key, t['median_ms'], t['p10_ms'], t['p90_ms'], f['median_ms'], f['p10_ms'], f['p90_ms'], r['speedup'],
             r['native_faster_beyond_spread']), flush=True)


def algorithmic_bytes(size, channels=3):
    levels = [max(size >> l, 1) ** 2 * channels * 4 for l in range(min((size - 1).bit_length() + 1, 8))]
    return {'forward': sum(levels), 'backward': sum(levels[1:]) + levels[0]}


def upstreams(levels):
    return [torch.rand(l.shape, device=l.device) for l in levels]


def pyramid_cases(size, device, iters, warmup):
    texels = torch.rand(size, size, 3, device=device).requires_grad_(True)
    ups = upstreams(torch_mipmap(texels.detach()))
    with torch.no_grad():
        err = max(float((a - b).abs().max()) for a, b in zip(torch_mipmap(texels), tx.generate_mipmap(texels)))

    def fwd(build):
        def run():
            with torch.no_grad():
                return build(texels)
        return run

    def both(build):
        def run():
            texels.grad = None
            levels = build(texels)
            torch.autograd.backward(levels, ups)
        return run

    return {'max_abs_difference_of_levels': err,
            'a_forward': against_torch(fwd(torch_mipmap), fwd(tx.generate_mipmap), iters, warmup),
            'b_forward_backward': against_torch(both(torch_mipmap), both(tx.generate_mipmap), iters, warmup)}


def fit_case(device, iters, warmup):
    import scenes
    from redner_amd import redner
    from redner_amd.render_pytorch import Material, RenderFunction, Texture
    res, tex_size = 256, 512
    sc = scenes.textured_sphere(device, resolution=(res, res))
    for sh in sc.shapes:
        for name in ('vertices', 'uvs', 'normals', 'colors'):
            if getattr(sh, name) is not None:
                getattr(sh, name).requires_grad_(False)
    sc.materials[1] = Material(diffuse_reflectance=torch.tensor([0.6, 0.55, 0.5], device=device))
    leaves = [torch.from_numpy(scenes._procedural(tex_size, tex_size, c, ph, lo, hi)).to(device).requires_grad_(True)
              for c, ph, lo, hi in ((3, 0.0, 0.1, 0.9), (3, 0.5, 0.05, 0.3), (1, 1.0, 0.2, 0.7))]
    up = torch.rand(res, res, 3, device=device)
    ups = [upstreams(torch_mipmap(t.detach())) for t in leaves]

    def iteration(build):
        def run():
            for t in leaves:
                t.grad = None
            d, s, r = (Texture(build(t)) for t in leaves)
            sc.materials[0] = Material(diffuse_reflectance=d, specular_reflectance=s, roughness=r)
            args = RenderFunction.serialize_scene(sc, (4, 4), 1, sampler_type=redner.SamplerType.sobol, device=device)
            RenderFunction.apply(1, *args).backward(up)
        return run

    def pyramids(build):
        def run():
            for t, u in zip(leaves, ups):
                t.grad = None
                torch.autograd.backward(build(t), u)
        return run

    whole = against_torch(iteration(torch_mipmap), iteration(tx.generate_mipmap), iters, warmup)
    alone = against_torch(pyramids(torch_mipmap), pyramids(tx.generate_mipmap), iters, warmup)
    share = {k: alone[k]['median_ms'] / whole[k]['median_ms'] for k in ('torch', 'native')}
    return {'c_fit_iteration': whole, 'c_three_pyramids_forward_backward': alone, 'c_pyramid_share_of_iteration': share}


def kernels_only(sizes, device, reps):
    """native forward + backward only, for a kernel trace"""
    for size in sizes:
        texels = torch.rand(size, size, 3, device=device).requires_grad_(True)
        ups = upstreams(torch_mipmap(texels.detach()))
        for _ in range(reps):
            texels.grad = None
            torch.autograd.backward(tx.generate_mipmap(texels), ups)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[256, 1024])
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--skip-fit', action='store_true')
    a = ap.parse_args()
    device = op_bench.require_gpu('bench_texture')
    if a.kernels_only:
        kernels_only(a.sizes, device, 20)
        return
    results = []
    for size in a.sizes:
        res = {'size': size, 'channels': 3, 'iters': a.iters, 'algorithmic_bytes': algorithmic_bytes(size)}
        res.update(pyramid_cases(size, device, a.iters, a.warmup))
        for key in ('a_forward', 'b_forward_backward'):
            report('%d^2 x 3' % size, key, res[key])
        results.append(res)
        print(json.dumps(res), flush=True)
    if not a.skip_fit:
        res = fit_case(device, a.iters, a.warmup)
        for key in ('c_fit_iteration', 'c_three_pyramids_forward_backward'):
            report('fit', key, res[key])
        results.append(res)
        print(json.dumps(res), flush=True)
    op_bench.emit(results, a.out, echo=False)


if __name__ == '__main__':
    main()
