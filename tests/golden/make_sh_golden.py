#!/usr/bin/env python3
"""Generate the spherical-harmonic and sampling-table fixtures under tests/golden/ (run in the BUILD container only).

The expected values come from the REFERENCE's own `pyredner.SH_reconstruct` and `pyredner.EnvironmentMap` executed by torch on
the CPU (gradients from torch autograd); nothing here restates their formulas.  Needs the reference checkout (its unmodified
Python package, imported like make_texture_golden does) and, for the end-to-end case, the oracle build (oracle/_ref).

  sh_tables_<H>x<W>.npz   per kind of input (table_texels): <kind>_cdf_ys, <kind>_cdf_xs, <kind>_pdf_norm (fp64 of the Python float)
                          of pyredner.EnvironmentMap(texels); `<kind>_sum` (fp64) guards the regenerated input
  sh_case_<name>.npz      image = pyredner.SH_reconstruct(coeffs, res) and d_coeffs under the fixed random upstream gradient of
                          sh_upstream(); `coeffs_sum` guards the input.  The generator ASSERTS that no pixel's unclamped value lies
                          within 1e-4 S of zero, S = sum_i |Y_i| |c_i| at that pixel in fp64 (the reference's own SH() on double
                          angles): a last-bit difference in cos cannot flip a clamp.  A seed that violates it is replaced (SH_CASES
                          holds the seeds that passed), pixels are never masked.  The case `ties` (all-zero coefficients) is
                          exempt: every pixel is a tie there, which is what it is about.
                          `harness_d_coeffs`, for the cases of BITWISE_CASES: what this project's CPU debugging harness computes
                          (recorded bytes; the GPU kernels add in the same order and must give the same bits).
  sh_e2e.npz              the envmap_sphere scene of make_texture_golden.envmap_scene lit by SH_reconstruct(coeffs, (16, 32)) at
                          order 3: image and d(coeffs), by the reference's SH_reconstruct + Texture + EnvironmentMap and the oracle

The helpers at the top (inputs, upstream gradients) are also what tests/test_sh_envmap.py builds its inputs from; they need
neither the reference nor the oracle.
"""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [p for p in (HERE,) if p not in sys.path]
import make_deferred_golden as mk          # noqa: E402
import make_texture_golden as mt           # noqa: E402

TABLE_SIZES = [(1, 1), (1, 7), (2, 2), (5, 3), (16, 32), (33, 65), (64, 129), (8, 4096)]
TABLE_KINDS = ('uniform', 'hdr', 'zero_rows')
# name -> (H, W), number of coefficient columns N, channels, seed, coeffs built as a slice of a wider tensor.  A tuple of seeds is
# one per channel (row of coeffs): at 64 x 129 x 3 and 64 basis functions a whole tensor that meets the clamp margin below is one in
# about a million draws, a single channel one in a hundred, and the channels are independent.
SH_CASES = {
    '1x1_o1': ((1, 1), 1, 3, 1, False),
    '1x7_o2': ((1, 7), 4, 3, 2, False),
    '5x3_o3': ((5, 3), 9, 3, 3, False),
    '16x32_o4': ((16, 32), 16, 3, 4, False),
    '33x17_o6': ((33, 17), 36, 3, 5, False),
    '64x129_o8': ((64, 129), 64, 3, (193, 302, 322), False),
    '16x32_o4_c1': ((16, 32), 16, 1, 7, False),
    '33x17_o3_c5': ((33, 17), 9, 5, 8, False),
    '16x32_n17': ((16, 32), 17, 3, 9, False),
    '16x32_o4_noncontig': ((16, 32), 16, 3, 50, True),
}
TIES = 'ties'                              # all-zero coefficients, (5, 3), order 2
BITWISE_CASES = ('16x32_o4', '64x129_o8')
E2E_RES, E2E_COEFFS, E2E_SEED = (16, 32), 9, 21
MARGIN = 1e-4


def size_tag(size):
    return '%dx%d' % tuple(size)


def table_texels(size, kind):
    """[H, W, 3] fp32: uniform values, an HDR-like image (rand**8 * 1000), or uniform with every second row all zero."""
    gen = torch.Generator().manual_seed(500 + 13 * size[0] + size[1] + 7 * TABLE_KINDS.index(kind))
    t = torch.rand(size[0], size[1], 3, generator=gen)
    if kind == 'hdr':
        t = t ** 8 * 1000.0
    elif kind == 'zero_rows':
        t[1::2] = 0.0
    return t.contiguous()


def case_shape(name):
    if name == TIES:
        return (5, 3), 4, 3
    return SH_CASES[name][:3]


def sh_coeffs(name):
    """[C, N] fp32: 0.3 * randn with + 0.6 on column 0 (about a third of the pixels clamped); a non-contiguous case is the same
    kind of values as every second column of a [C, 2 N] tensor."""
    res, n, c = case_shape(name)
    if name == TIES:
        return torch.zeros(c, n)
    seed, noncontig = SH_CASES[name][3:]
    if isinstance(seed, tuple):
        wide = torch.stack([0.3 * torch.randn(n, generator=torch.Generator().manual_seed(9000 + k)) for k in seed])
    else:
        gen = torch.Generator().manual_seed(9000 + seed)
        wide = 0.3 * torch.randn(c, 2 * n if noncontig else n, generator=gen)
    coeffs = wide[:, ::2] if noncontig else wide
    coeffs[:, 0] += 0.6
    assert coeffs.is_contiguous() != noncontig or coeffs.shape[1] == 1
    return coeffs


def sh_upstream(name):
    res, n, c = case_shape(name)
    gen = torch.Generator().manual_seed(77000 + res[0] * 131 + res[1] + c)
    return torch.randn(res[0], res[1], c, generator=gen)


def e2e_coeffs():
    gen = torch.Generator().manual_seed(9000 + E2E_SEED)
    coeffs = 0.3 * torch.randn(3, E2E_COEFFS, generator=gen)
    coeffs[:, 0] += 0.9
    return coeffs


# ---- everything below needs the reference -------------------------------------------------------------------------------------
def make_table_fixtures(pyredner):
    for size in TABLE_SIZES:
        out = {}
        for kind in TABLE_KINDS:
            texels = table_texels(size, kind)
            env = pyredner.EnvironmentMap(texels)
            out[kind + '_cdf_ys'] = env.sample_cdf_ys.numpy()
            out[kind + '_cdf_xs'] = env.sample_cdf_xs.numpy()
            out[kind + '_pdf_norm'] = np.asarray(env.pdf_norm, np.float64)
            out[kind + '_sum'] = np.asarray(texels.double().sum().item())
        np.savez_compressed(os.path.join(HERE, 'sh_tables_%s.npz' % size_tag(size)), **out)
        print('tables', size_tag(size))


def clamp_margin(pyredner, coeffs, res):
    """min over pixels and channels of |unclamped| / S in fp64, with the reference's own basis functions on double angles."""
    from pyredner import utils
    uv = np.mgrid[0:res[0], 0:res[1]].astype(np.float64)
    theta = torch.from_numpy((math.pi / res[0]) * (uv[0] + 0.5))
    phi = torch.from_numpy((2 * math.pi / res[1]) * (uv[1] + 0.5))
    c = coeffs.double()
    value = torch.zeros(res[0], res[1], c.shape[0], dtype=torch.float64)
    scale = torch.zeros_like(value)
    i = 0
    for l in range(int(math.sqrt(c.shape[1]))):
        for m in range(-l, l + 1):
            y = utils.SH(l, m, theta, phi)
            if not isinstance(y, torch.Tensor):
                y = torch.full_like(theta, float(y))
            value = value + y[:, :, None] * c[:, i]
            scale = scale + y.abs()[:, :, None] * c[:, i].abs()
            i += 1
    return float((value.abs() / scale).min()), float((value < 0).double().mean())


def make_sh_fixtures(pyredner, harness):
    for name in list(SH_CASES) + [TIES]:
        res, n, c = case_shape(name)
        coeffs = sh_coeffs(name).requires_grad_(True)
        image = pyredner.SH_reconstruct(coeffs, res)
        assert tuple(image.shape) == (res[0], res[1], c)
        (image * sh_upstream(name)).sum().backward()
        out = {'image': image.detach().numpy(), 'd_coeffs': coeffs.grad.numpy().copy(),
               'coeffs_sum': np.asarray(coeffs.detach().double().sum().item())}
        if name != TIES:
            margin, clamped = clamp_margin(pyredner, coeffs.detach(), res)
            print('sh', name, 'margin %.2e of S, %.0f %% of the pixels clamped' % (margin, 100 * clamped))
            assert margin > MARGIN, (name, margin, 'choose another seed')
        if name in BITWISE_CASES:
            from redner_amd import utils as native
            x = sh_coeffs(name).requires_grad_(True)
            (native.SH_reconstruct(x, res, backend=harness) * sh_upstream(name)).sum().backward()
            out['harness_d_coeffs'] = x.grad.numpy().copy()
        np.savez_compressed(os.path.join(HERE, 'sh_case_%s.npz' % name), **out)


def make_e2e_fixture(ref, pyredner):
    from redner_amd import render_pytorch as rp
    cpu = torch.device('cpu')
    coeffs = e2e_coeffs().requires_grad_(True)
    values = pyredner.SH_reconstruct(coeffs, E2E_RES)
    margin, clamped = clamp_margin(pyredner, coeffs.detach(), E2E_RES)
    print('e2e margin %.2e of S, %.0f %% of the pixels clamped' % (margin, 100 * clamped))
    assert margin > MARGIN, margin

    def ref_envmap(v, e2w):
        env = rp.EnvironmentMap(rp.Texture(pyredner.Texture(v).mipmap), env_to_world=e2w)
        theirs = pyredner.EnvironmentMap(v.detach(), env_to_world=e2w.contiguous())
        assert torch.equal(env.sample_cdf_xs, theirs.sample_cdf_xs) and torch.equal(env.sample_cdf_ys, theirs.sample_cdf_ys)
        assert env.pdf_norm == theirs.pdf_norm
        return env

    sc = mt.envmap_scene(cpu, ref_envmap, values)
    img = mt.render_e2e(sc, 'envmap', [ref.channels.radiance], cpu, ref)
    out = {'image': img.detach().numpy(), 'grad_coeffs': coeffs.grad.numpy().copy()}
    assert np.isfinite(out['image']).all() and np.abs(out['grad_coeffs']).sum() > 0
    np.savez_compressed(os.path.join(HERE, 'sh_e2e.npz'), **out)
    print('e2e', {k: v.shape for k, v in out.items()})


def main():
    # like make_golden.main: fresh zero pages for the reference's scratch buffers
    if os.environ.get('MALLOC_MMAP_THRESHOLD_') != '65536' or os.environ.get('MALLOC_PERTURB_') != '255':
        import subprocess
        env = dict(os.environ, MALLOC_MMAP_THRESHOLD_='65536', MALLOC_PERTURB_='255')
        sys.exit(subprocess.call([sys.executable] + sys.argv, env=env))
    ref, pyredner = mk.reference_package()
    make_table_fixtures(pyredner)
    make_e2e_fixture(ref, pyredner)
    # the harness last: loading it rebinds redner_amd's native library
    import subprocess
    subprocess.check_call(['make', '-C', os.path.join(ROOT, 'tests', 'hostsim'), '-j8'], stdout=subprocess.DEVNULL)
    from redner_amd import _capi, redner
    _capi.load(os.path.join(ROOT, 'tests', 'hostsim', '_build', 'libredner_hostsim.so'))
    make_sh_fixtures(pyredner, redner)


if __name__ == '__main__':
    main()
