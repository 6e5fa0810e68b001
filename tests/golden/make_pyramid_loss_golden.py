#!/usr/bin/env python3
"""Generate the Gaussian pyramid loss fixtures under tests/golden/ (run in the BUILD container only; needs scipy and the CPU
debugging harness, tests/hostsim).

The expected values come from the torch formulation the optimisation scripts write, stated here in this file's own words and run
by torch on the CPU in fp32: D_0 = image - target (clamped when the case says so); D_{l+1} = AvgPool2d(2)(conv2d(D_l, K,
padding=3)) with K the 7 x 7 table of scipy.ndimage.gaussian_filter(dirac, 1.0) on a per-channel diagonal; loss = sum_l w_l *
D_l.pow(2).sum() / ((H / 2 ** l) * (W / 2 ** l)); image.grad by autograd.

  pyramid_loss_gauss7x7.npy    the scipy table, fp32 (scipy need not be where the tests run)
  pyramid_loss_<case>.npz      loss (fp32), terms (fp64 [L], from the fp32 levels), grad (image.grad, fp32), `inputs_sum` (fp64,
                               guards the regenerated inputs: the inputs are a function of the case's seed, inputs(), and are
                               not stored -- two 256 x 256 x 3 images would not fit a committed file), and what this project's
                               CPU debugging harness computes: harness_loss (fp32), harness_terms (fp64) and harness_grad_sha256
                               (the digest of the gradient's bytes); the GPU kernels add in the same order and must give the
                               same bits.

The generator ASSERTS, per case, that the torch formulation's own fp32 levels and gradient lie within the per-element bars of
tests/test_pyramid_loss.py (K_DOWN, k_grad) of the fp64 separable definition below, so the bars are not tighter than what the
reference achieves; and that four mutations of that definition (a plain truncated 7-tap filter, wrapped padding, a pooled-size
divisor, the odd-side rule swapped) each fail a bar on at least one case.

The helpers at the top (cases, inputs, the fp64 definition) are also what tests/test_pyramid_loss.py uses; they need neither scipy
nor the harness.
"""
import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
U = 2.0 ** -24
K_DOWN = 20            # roundings on the longest path of one level step (tests/test_pyramid_loss.py derives it)

# name -> (shape, num_levels, clamp, weights)
CASES = {
    '1x1x1_L1': ((1, 1, 1), 1, None, None),
    '2x2x3_L2': ((2, 2, 3), 2, None, None),
    '7x7x3_L2': ((7, 7, 3), 2, None, None),
    '5x9x3_L3': ((5, 9, 3), 3, None, None),
    '13x6x1_L2': ((13, 6, 1), 2, None, None),
    '70x38x4_L4': ((70, 38, 4), 4, None, None),
    '100x100x3_L6': ((100, 100, 3), 6, None, None),
    '256x256x3_L5': ((256, 256, 3), 5, None, None),
    '256x256x3_L6': ((256, 256, 3), 6, None, None),
    '2x40x24x3_L3': ((2, 40, 24, 3), 3, None, None),
    '33x33x3_L3_clamp1': ((33, 33, 3), 3, 1.0, None),
    '256x256x3_L5_w00111': ((256, 256, 3), 5, None, (0.0, 0.0, 1.0, 1.0, 1.0)),
}


def fixture_path(name):
    return os.path.join(HERE, 'pyramid_loss_%s.npz' % name)


TABLE_PATH = os.path.join(HERE, 'pyramid_loss_gauss7x7.npy')


def inputs(name):
    """image, target fp32 of the case's shape: a smooth pattern plus noise against another one.  The clamp case has differences
    of up to 1.5 and, at every 7th element, a difference of exactly +1 or -1 (the target there is a multiple of 1/8)."""
    shape, _, clamp, _ = CASES[name]
    gen = torch.Generator().manual_seed(4100 + sum((i + 1) * 17 * s for i, s in enumerate(shape)) + (1 if clamp else 0))
    target = torch.rand(*shape, generator=gen)
    image = target + (1.5 if clamp else 0.5) * (torch.rand(*shape, generator=gen) - 0.5) * 2.0
    if clamp:
        t, a = target.reshape(-1), image.reshape(-1)
        t[::7] = torch.round(t[::7] * 8.0) / 8.0
        a[::7] = t[::7] + clamp
        a[::14] = t[::14] - clamp
    return image.contiguous(), target.contiguous()


def inputs_sum(name):
    image, target = inputs(name)
    return float(image.double().sum() + 3.0 * target.double().sum())


def taps(truncated=False):
    """The seven taps a, fp32: the unit Gaussian cut at 4 sigma with the ninth tap reflected into the ends (what a 7-wide dirac
    through scipy's gaussian_filter gives); truncated=True: the plain 7-tap Gaussian (a mutation)."""
    k = np.arange(-4, 5, dtype=np.float64)
    w = np.exp(-0.5 * k * k)
    if truncated:
        w = w[1:-1] / w[1:-1].sum()
        return w.astype(np.float32)
    w /= w.sum()
    return np.array([w[1] + w[0], w[2], w[3], w[4], w[5], w[6], w[7] + w[8]]).astype(np.float32)


# ---- the fp64 definition, separable, with its mutations -----------------------------------------------------------------------
def _filter(x, a, axis, wrap):
    n = x.shape[axis]
    pad = [(0, 0)] * x.ndim
    pad[axis] = (3, 3)
    p = np.pad(x, pad, mode='wrap' if wrap else 'constant')
    return sum(float(a[i]) * np.take(p, np.arange(i, i + n), axis=axis) for i in range(7))


def down64(d, a, mutate=None):
    """D_{l+1} [N, H // 2, W // 2, C] fp64 from D_l [N, H, W, C]"""
    wrap = mutate == 'wrap'
    g = _filter(_filter(d, a, 1, wrap), a, 2, wrap)
    h, w = d.shape[1] // 2, d.shape[2] // 2
    g = g[:, d.shape[1] - 2 * h:, d.shape[2] - 2 * w:] if mutate == 'odd' else g[:, :2 * h, :2 * w]
    return 0.25 * (g[:, 0::2, 0::2] + g[:, 0::2, 1::2] + g[:, 1::2, 0::2] + g[:, 1::2, 1::2])


def up64(acc, shape, a):
    """A^T acc: [N, H, W, C] fp64 from the coarse acc [N, H // 2, W // 2, C] (zero padding, last row / column of G dropped)"""
    g = np.zeros(shape, dtype=np.float64)
    h, w = acc.shape[1], acc.shape[2]
    for dy in (0, 1):
        for dx in (0, 1):
            g[:, dy:2 * h:2, dx:2 * w:2] = 0.25 * acc
    return _filter(_filter(g, a, 1, False), a, 2, False)           # a is symmetric: the filter is its own transpose


def batched(x):
    x = np.asarray(x, dtype=np.float64)
    return x if x.ndim == 4 else x[None]


def diff32(image, target, clamp):
    """D_0 as fp32 forms it (one IEEE subtraction, then the clamp) and the clamp's mask"""
    d = np.asarray(image, dtype=np.float32) - np.asarray(target, dtype=np.float32)
    mask = np.ones(d.shape, dtype=bool) if clamp is None else (d >= -clamp) & (d <= clamp)
    return (d if clamp is None else np.clip(d, np.float32(-clamp), np.float32(clamp))), mask


def counts(shape, num_levels, pooled=False):
    n, h, w, c = shape
    out = []
    for l in range(num_levels):
        out.append(float(h * w) if pooled else (shape[1] / 2 ** l) * (shape[2] / 2 ** l))
        h, w = h // 2, w // 2
    return out


def terms64(levels, weights, mutate=None):
    cnt = counts(levels[0].shape, len(levels), pooled=mutate == 'pooled')
    wts = weights or (1.0,) * len(levels)
    return np.array([wts[l] * float((levels[l] ** 2).sum()) / cnt[l] for l in range(len(levels))])


def grad64(levels, weights, a):
    """(acc_0, absacc_0) fp64 from the levels taken as exact: acc_l = c_l D_l + A^T acc_{l+1}, and the same with absolute values"""
    cnt = counts(levels[0].shape, len(levels))
    wts = weights or (1.0,) * len(levels)
    acc = absacc = None
    for l in range(len(levels) - 1, -1, -1):
        direct = (2.0 * wts[l] / cnt[l]) * levels[l]
        if acc is None:
            acc, absacc = direct, np.abs(direct)
        else:
            acc, absacc = direct + up64(acc, levels[l].shape, a), np.abs(direct) + up64(absacc, levels[l].shape, a)
    return acc, absacc


def k_grad(num_levels):
    return 14 * (num_levels - 1) + 5


def definition(name, mutate=None):
    """The whole op in fp64 from the case's inputs: levels, terms, loss, gradient"""
    shape, num_levels, clamp, weights = CASES[name]
    image, target = inputs(name)
    d0, mask = diff32(image.numpy(), target.numpy(), clamp)
    a = taps(truncated=mutate == 'truncated')
    levels = [batched(d0)]
    for _ in range(1, num_levels):
        levels.append(down64(levels[-1], a, mutate))
    terms = terms64(levels, weights, mutate)
    return levels, terms, float(terms.sum()), grad64(levels, weights, a)[0] * batched(mask)


# ---- everything below needs scipy and the harness ---------------------------------------------------------------------------
def scipy_table():
    import scipy.ndimage
    dirac = np.zeros((7, 7))
    dirac[3, 3] = 1.0
    return scipy.ndimage.gaussian_filter(dirac, 1.0).astype(np.float32)


def torch_formulation(image, target, num_levels, clamp, weights, table):
    """-> loss (0-dim fp32, attached), the fp32 levels [N, H_l, W_l, C] (detached numpy).  image may require grad."""
    c = image.shape[-1]
    kernel = torch.zeros(c, c, 7, 7)
    for k in range(c):
        kernel[k, k] = torch.from_numpy(table)
    d = image - target
    if clamp is not None:
        d = d.clamp(-clamp, clamp)
    if d.dim() == 3:
        d = d.unsqueeze(0)
    n, h, w, _ = d.shape
    d = d.permute(0, 3, 1, 2)
    pool = torch.nn.AvgPool2d(2)
    wts = weights or (1.0,) * num_levels
    loss, levels = 0.0, []
    for l in range(num_levels):
        levels.append(d.detach().permute(0, 2, 3, 1).numpy().copy())
        loss = loss + wts[l] * d.pow(2).sum() / ((h / 2 ** l) * (w / 2 ** l))
        if l + 1 < num_levels:
            d = pool(torch.nn.functional.conv2d(d, kernel, padding=3))
    return loss, levels


def violations(name, ref_levels, ref_terms, ref_grad, mutate=None):
    """How the reference's own fp32 results stand against the (possibly mutated) fp64 definition: the worst ratio to each bar"""
    shape, num_levels, clamp, weights = CASES[name]
    a = taps(truncated=mutate == 'truncated')
    worst = {'level': 0.0, 'term': 0.0, 'grad': 0.0}
    lv = [batched(x) for x in ref_levels]
    for l in range(1, num_levels):
        want, bar = down64(lv[l - 1], a, mutate), K_DOWN * U * down64(np.abs(lv[l - 1]), np.abs(a), mutate)
        worst['level'] = max(worst['level'], float(np.max(np.abs(lv[l] - want) / np.maximum(bar, 1e-300))))
    want = terms64(lv, weights, mutate)
    worst['term'] = float(np.max(np.abs(ref_terms - want) / np.maximum(1e-6 * np.abs(want), 1e-300)))
    image, target = inputs(name)
    mask = batched(diff32(image.numpy(), target.numpy(), clamp)[1])
    acc, absacc = grad64(lv, weights, a)
    bar = k_grad(num_levels) * U * absacc
    err = np.where(mask, np.abs(batched(ref_grad) - acc), np.abs(batched(ref_grad)))
    worst['grad'] = float(np.max(err / np.maximum(bar, 1e-300)))
    return worst


def main():
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
    import subprocess
    subprocess.check_call(['make', '-C', os.path.join(ROOT, 'tests', 'hostsim'), '-j8'], stdout=subprocess.DEVNULL)
    from redner_amd import _capi, redner
    from redner_amd.loss import gaussian_pyramid_loss
    _capi.load(os.path.join(ROOT, 'tests', 'hostsim', '_build', 'libredner_hostsim.so'))
    table = scipy_table()
    a = taps()
    # fp32(a_i) fp32(a_j) against scipy's fp64 product rounded to fp32: three roundings of numbers of at most table.max()
    assert np.max(np.abs(table.astype(np.float64) - np.outer(a.astype(np.float64), a.astype(np.float64)))) <= 3 * U * table.max(), \
        'the taps are not scipy\'s'
    np.save(TABLE_PATH, table)
    failed = {m: [] for m in ('truncated', 'wrap', 'pooled', 'odd')}
    for name, (shape, num_levels, clamp, weights) in CASES.items():
        image, target = inputs(name)
        x = image.clone().requires_grad_(True)
        loss, levels = torch_formulation(x, target, num_levels, clamp, weights, table)
        loss.backward()
        grad = x.grad.numpy()
        wts = weights or (1.0,) * num_levels
        cnt = counts(batched(levels[0]).shape, num_levels)
        terms = np.array([wts[l] * float((levels[l].astype(np.float64) ** 2).sum()) / cnt[l] for l in range(num_levels)])
        worst = violations(name, levels, terms, grad)
        print('%-24s loss %.9g   reference / bar: level %.3f grad %.3f' % (name, float(loss), worst['level'], worst['grad']))
        assert worst['level'] <= 1.0 and worst['grad'] <= 1.0 and worst['term'] <= 1.0, (name, worst)
        for m in failed:
            bad = violations(name, levels, terms, grad, m)
            if max(bad.values()) > 1.0:
                failed[m].append(name)
        y = image.clone().requires_grad_(True)
        h_loss, h_terms = gaussian_pyramid_loss(y, target, num_levels, clamp=clamp, weights=weights, return_terms=True, backend=redner)
        h_loss.backward()
        np.savez_compressed(fixture_path(name), loss=np.float32(loss.item()), terms=terms, grad=grad,
                            inputs_sum=np.float64(inputs_sum(name)), harness_loss=h_loss.detach().numpy(),
                            harness_terms=h_terms.numpy(),
                            harness_grad_sha256=np.frombuffer(hashlib.sha256(y.grad.numpy().tobytes()).digest(), dtype=np.uint8))
    for m, names in failed.items():
        print('mutation %-10s fails on %s' % (m, names))
        assert names, 'the mutation %s passes every case' % m


if __name__ == '__main__':
    main()
