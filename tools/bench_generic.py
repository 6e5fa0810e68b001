#!/usr/bin/env python3
"""Forward plus backward of a G-buffer render whose only channel is a wide generic texture, on two builds of the library that
take turns inside one process.

    python tools/bench_generic.py --other variants/parent.so --label parent --widths 5 16 [--iters 60] [--warmup 5] [--out FILE]

A step is "64 x 64 x N texels (require grad) -> redner_amd.Texture (mip pyramid) -> render_g_buffer of tests/scenes.py's
textured_sphere at 256 x 256, channel generic_texture, one sample per pixel, first hits only -> gradient of the texels under a
fixed upstream image".  `--other` is a second build of the library (tools/build_variant.sh): the parent commit built into
variants/, or this tree with a -D switch.  Both builds are warmed up, every step sits in its own pair of device events
(op_bench.time_alternating); median and 10th / 90th percentiles are reported, and `other_spread_ms` = the other build's
p90 - p10 in that run is the measured noise a difference of medians has to be read against.  These are STEP times: the
Material and Texture objects, the pyramid and its adjoint, scene serialisation, launches and autograd are inside every step
beside the first-hit stages, so a difference in the texel scatter alone shows diluted.  A build that refuses the width
(the parent above 16 channels) is reported as such, not timed.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tests', 'golden'), os.path.join(ROOT, 'tools')]

from redner_amd import _capi                 # noqa: E402
from op_bench import emit, require_gpu, time_alternating          # noqa: E402

FRAME, TEXTURE = (256, 256), (64, 64)


def make_step(library, width, device):
    """-> (step, state): `library` = (ctypes handle, path) of the build the step runs on"""
    import redner_amd
    import scenes
    import make_deferred_golden as mk
    import make_texture_golden as mt
    from redner_amd import redner as rd, render_utils as ru
    from redner_amd.render_pytorch import Material
    texels = torch.rand(TEXTURE + (width,), generator=torch.Generator().manual_seed(width)).to(device).requires_grad_(True)
    sc = mt._freeze(scenes.textured_sphere(device, resolution=FRAME))
    upstream = mk.upstream(FRAME + (width,)).to(device)
    state = {}

    def step():
        _capi.use(*library)          # the build this step runs on (both were loaded by _capi.load)
        texels.grad = None
        sc.materials[0] = Material(diffuse_reflectance=torch.tensor([0.5, 0.5, 0.5], device=device),
                                   generic_texture=redner_amd.Texture(texels, backend=rd))
        img = ru.render_g_buffer(sc, [rd.channels.generic_texture], seed=1, device=device, backend=rd)
        (img * upstream).sum().backward()
        state['image'], state['grad'] = img.detach(), texels.grad
    return step, state


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def run_case(width, libs, label, device, iters, warmup):
    res = {'case': 'generic %dx%dx%d, textured_sphere %dx%d' % (TEXTURE + (width,) + FRAME), 'width': width, 'other': label, 'iters': iters}
    steps, states = {}, {}
    for name in (label, 'this'):
        step, state = make_step(libs[name], width, device)
        try:
            step()
        except RuntimeError as e:
            res[name + '_refuses'] = str(e)
            print('%-3d %s refuses: %s' % (width, name, e), flush=True)
            continue
        steps[name], states[name] = step, state
    torch.cuda.synchronize()
    if len(steps) == 2:
        res['image_equal'] = bool(torch.equal(states['this']['image'], states[label]['image']))
        res['grad_rel_difference'] = rel(states['this']['grad'], states[label]['grad'])
    res['step'] = time_alternating(steps, iters, warmup)
    r = res['step']
    if len(steps) == 2:
        res['other_spread_ms'] = r[label]['p90_ms'] - r[label]['p10_ms']
        res['this_minus_other_ms'] = r['this']['median_ms'] - r[label]['median_ms']
    print('%-3d ' % width + '   '.join('%s %.3f ms [%.3f, %.3f]' % (n, t['median_ms'], t['p10_ms'], t['p90_ms']) for n, t in r.items()) +
          ('   this - %s = %+.3f ms, spread of %s %.3f ms, images equal %s, gradients differ by %.1e'
           % (label, res['this_minus_other_ms'], label, res['other_spread_ms'], res['image_equal'], res['grad_rel_difference'])
           if len(steps) == 2 else ''), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--other', required=True, help='the second build of the library (a path)')
    ap.add_argument('--label', default='other')
    ap.add_argument('--widths', nargs='+', type=int, default=[5, 16, 32, 64])
    ap.add_argument('--iters', type=int, default=60)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    device = require_gpu('bench_generic')
    other = os.path.abspath(a.other)
    libs = {a.label: (_capi.load(other), other), 'this': (_capi.load(_capi.DEFAULT_LIBRARY), _capi.DEFAULT_LIBRARY)}
    emit([run_case(w, libs, a.label, device, a.iters, a.warmup) for w in a.widths], a.out, echo=True)


if __name__ == '__main__':
    main()
