"""The mip pyramid (redner_amd.texture on rdr_mip_pyramid / rdr_mip_pyramid_backward) against fixtures made by the reference's own
pyredner.Texture under torch autograd (tests/golden/make_texture_golden.py), against an independent fp64 definition written
here, and through redner_amd.Texture / redner_amd.EnvironmentMap and RenderFunction against the oracle.

Bars
  * fixtures: parity_util.TOL = 1e-4 relative L2 of every whole tensor (levels, d_texels, images, texel gradients); the expected
    error is fp32 rounding (the reference's own fp32 pyramid is within 2.4e-7, max relative per element, of fp64).  Level count
    and shapes must match exactly.
  * fp64 definition: per level, max abs error <= 84 * 2^-24 * max|texels|: a level costs at most 12 roundings (3 additions for
    the 2 x 2 box, up to 8 additions and one division for a 3 x 3 window; the scaling by 1/4 is exact), each at most 2^-24 of a
    value bounded by the input's maximum, averaging never amplifies an error, and at most 7 levels are built.  A wrong weight,
    window or wrap is off by 1e-2 or more.
  * launch plan (section 3b): the same forward bar, and d_texels element by element against the fp64 adjoint (autograd through
    a torch-double port of the definition) to 18 * (levels - 1) * 2^-24 * M_0, M_0 being that adjoint of |g| (_run_plan_case has
    the derivation), at shapes on both sides of every switch of the kernels' launch plan; each case asserts its stage count.
  * adjoint identity: <A x, y> == <x, A^T y> to 1e-5 relative in fp64 accumulation (the two sides differ by the fp32 rounding
    of A x and A^T y, about 1e-7; a wrong transpose is off by percents).
The harness cases run the same per-texel bodies as the kernels, as plain loops; the GPU cases run on both builds of the library.

"No level tensor is a leaf" is asserted for the levels 1..: level 0 of a pyramid IS `texels.contiguous()`, the user's own leaf
when it is contiguous (as in the reference), which is how its gradient g_0 reaches `texels.grad` without passing the Function."""
import os

import numpy as np
import pytest
import torch

import parity_util
from golden import make_deferred_golden as mk
from golden import make_texture_golden as mt

GOLD = parity_util.GOLD
CPU, GPU = torch.device('cpu'), torch.device('cuda:0')
DEFINITION_SIZES_GPU = [(2048, 1024, 3), (1023, 517, 1), (777, 1, 4)]
DEFINITION_SIZES_HOSTSIM = [(37, 90, 3), (130, 67, 2)]           # (the second is large enough for the tiled launches' shape rules)
ADJOINT_SIZES = [(1, 1, 3), (1, 7, 3), (2, 2, 1), (5, 3, 3), (13, 40, 5), (64, 64, 3), (100, 37, 1), (255, 129, 3), (300, 1, 2)]


def _texture_module():
    from redner_amd import texture
    return texture


def _check(name, out, gold, tag):
    rep = parity_util.compare(out, gold, name)
    print(name, tag, {k: '%.2e' % e['rel_l2'] for k, e in rep.items()})
    parity_util.record(name, rep, tag)
    parity_util.assert_parity(rep, name)


# ---- 1. kernel fixtures ---------------------------------------------------------------------------------------------------------
def _kernel_fixture(size):
    path = os.path.join(GOLD, 'texture_kernel_%s.npz' % mt.size_tag(size))
    gold = dict(np.load(path))
    if os.path.exists(path[:-4] + '_grad.npz'):
        gold.update(np.load(path[:-4] + '_grad.npz'))
    return gold


def _run_kernel_case(backend, device, size, tag):
    gold = _kernel_fixture(size)
    texels = mt.kernel_texels(size)
    assert abs(float(texels.double().sum()) - float(gold.pop('texels_sum'))) < 1e-9, 'the regenerated input is not the fixture\'s'
    texels = texels.to(device).requires_grad_(True)
    levels = _texture_module().generate_mipmap(texels, backend=backend)
    num_levels = int(gold.pop('num_levels'))
    assert len(levels) == num_levels == backend.mip_num_levels(size[0], size[1])
    for l in range(1, num_levels):
        assert tuple(levels[l].shape) == tuple(gold['level%d' % l].shape), (l, levels[l].shape)
        assert levels[l].device == texels.device and not levels[l].is_leaf
    assert levels[0].data_ptr() == texels.data_ptr()
    mt.pyramid_loss(levels).backward()
    assert tuple(texels.grad.shape) == tuple(size)
    out = {'level%d' % l: levels[l].detach().cpu().numpy() for l in range(1, num_levels)}
    out['d_texels'] = texels.grad.cpu().numpy()
    _check('texture_kernel_' + mt.size_tag(size), out, gold, tag)


@pytest.mark.parametrize('size', mt.KERNEL_SIZES, ids=mt.size_tag)
def test_pyramid_fixture_hostsim(hostsim_backend, size):
    _run_kernel_case(hostsim_backend, CPU, size, 'hostsim')


@pytest.mark.gpu
@pytest.mark.parametrize('size', mt.KERNEL_SIZES, ids=mt.size_tag)
def test_pyramid_fixture_gpu(gpu_backend, size):
    _run_kernel_case(gpu_backend, GPU, size, 'gpu')


# ---- 2. end to end --------------------------------------------------------------------------------------------------------------
def _assert_pyramid(tex, texels):
    assert len(tex.mipmap) > 1 and tex.mipmap[0].data_ptr() == texels.data_ptr()
    assert all(not l.is_leaf for l in tex.mipmap[1:])


def _run_sphere_case(backend, device, tag):
    import redner_amd
    diffuse, generic = (t.to(device).requires_grad_(True) for t in mt.sphere_texels())
    sc = mt.sphere_scene(device, lambda t, uv: redner_amd.Texture(t, uv, backend=backend), diffuse, generic)
    _assert_pyramid(sc.materials[0].diffuse_reflectance, diffuse)
    _assert_pyramid(sc.materials[0].generic_texture, generic)
    img = mt.render_e2e(sc, 'sphere', [backend.channels.radiance, backend.channels.generic_texture], device, backend)
    assert tuple(diffuse.grad.shape) == (32, 32, 3) and tuple(generic.grad.shape) == (8, 8, 5)
    out = {'image': img.detach().cpu().numpy(), 'grad_diffuse': diffuse.grad.cpu().numpy(), 'grad_generic': generic.grad.cpu().numpy()}
    _check('texture_sphere', out, np.load(os.path.join(GOLD, 'texture_sphere.npz')), tag)


def _run_envmap_case(backend, device, tag):
    import redner_amd
    values = mt.envmap_values().to(device).requires_grad_(True)
    sc = mt.envmap_scene(device, lambda v, e2w: redner_amd.EnvironmentMap(v, env_to_world=e2w, backend=backend), values)
    assert isinstance(sc.envmap.values, redner_amd.Texture)
    _assert_pyramid(sc.envmap.values, values)
    img = mt.render_e2e(sc, 'envmap', [backend.channels.radiance], device, backend)
    assert tuple(values.grad.shape) == (16, 32, 3)
    out = {'image': img.detach().cpu().numpy(), 'grad_values': values.grad.cpu().numpy()}
    _check('texture_envmap', out, np.load(os.path.join(GOLD, 'texture_envmap.npz')), tag)


def test_textured_sphere_hostsim(hostsim_backend):
    _run_sphere_case(hostsim_backend, CPU, 'hostsim')


def test_envmap_hostsim(hostsim_backend):
    _run_envmap_case(hostsim_backend, CPU, 'hostsim')


@pytest.mark.gpu
def test_textured_sphere_gpu(gpu_backend):
    _run_sphere_case(gpu_backend, GPU, 'gpu')


@pytest.mark.gpu
def test_envmap_gpu(gpu_backend):
    _run_envmap_case(gpu_backend, GPU, 'gpu')


# ---- 3. an independent definition in fp64 ---------------------------------------------------------------------------------------
def _definition_level(p):
    """One step of the pyramid for p [Hp, Wp, C] fp64: wrap by modulo, windows by floor / ceil, vectorised per window offset."""
    hp, wp = p.shape[0], p.shape[1]
    ho, wo = max(hp // 2, 1), max(wp // 2, 1)
    rows, cols = (np.arange(hp) + 1) % hp, (np.arange(wp) + 1) % wp
    b = (p + p[:, cols] + p[rows] + p[rows][:, cols]) / 4.0
    r0 = (np.arange(ho) * hp) // ho
    r1 = -((-(np.arange(ho) + 1) * hp) // ho)
    c0 = (np.arange(wo) * wp) // wo
    c1 = -((-(np.arange(wo) + 1) * wp) // wo)
    out = np.zeros((ho, wo, p.shape[2]))
    for dr in range(int((r1 - r0).max())):
        rsel = (r0 + dr < r1)[:, None, None]
        for dc in range(int((c1 - c0).max())):
            csel = (c0 + dc < c1)[None, :, None]
            out += b[np.minimum(r0 + dr, hp - 1)][:, np.minimum(c0 + dc, wp - 1)] * (rsel & csel)
    return out / ((r1 - r0)[:, None, None] * (c1 - c0)[None, :, None])


def _definition(texels):
    h, w = texels.shape[0], texels.shape[1]
    n = min((max(h, w) - 1).bit_length() + 1, 8)
    levels = [texels.astype(np.float64)]
    for _ in range(1, n):
        levels.append(_definition_level(levels[-1]))
    return levels


def _run_definition_case(backend, device, size):
    gen = torch.Generator().manual_seed(31 + size[0])
    texels = torch.rand(*size, generator=gen) * 2.0 - 0.5
    levels = _texture_module().generate_mipmap(texels.to(device), backend=backend)
    want = _definition(texels.numpy())
    assert [tuple(l.shape) for l in levels] == [tuple(l.shape) for l in want]
    bound = 84.0 * 2.0 ** -24 * float(texels.abs().max())
    for l, (got, ref) in enumerate(zip(levels, want)):
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max())
        print('definition', mt.size_tag(size), 'level', l, 'max abs error %.3e (bound %.3e)' % (err, bound))
        assert err <= bound, (size, l, err, bound)


@pytest.mark.parametrize('size', DEFINITION_SIZES_HOSTSIM, ids=mt.size_tag)
def test_pyramid_definition_hostsim(hostsim_backend, size):
    _run_definition_case(hostsim_backend, CPU, size)


@pytest.mark.gpu
@pytest.mark.parametrize('size', DEFINITION_SIZES_GPU, ids=mt.size_tag)
def test_pyramid_definition_gpu(gpu_backend, size):
    _run_definition_case(gpu_backend, GPU, size)


# ---- 3b. forward AND adjoint, element by element, on both sides of every switch of the launch plan ------------------------------
# (H, W, C) -> tiled launches each way.  The rule (csrc/mipmap.h, tiled_stages): a tiled launch does three levels while the level it
# starts from holds more than 64 * 64 * 3 floats and three more levels exist; one workgroup (the chain kernels) does the rest.
# The counts are written out, checked against the rule as restated in _stages_by_rule and against what the loaded library
# plans (rdr_mip_tiled_stages): moving kSmall cannot silently move a case to the other side of its switch.
PLAN_CASES = [
    # the kSmall switch: the last chain-only shape and the first tiled ones
    ((1, 12288, 1), 0), ((1, 12289, 1), 1), ((64, 65, 3), 1), ((65, 64, 3), 1),
    # sides of 1, 2, 3 inside a tiled launch (h[1..3] or w[1..3] = 1)
    ((1, 5000, 3), 1), ((13000, 1, 1), 1), ((2, 3000, 4), 1), ((3, 2100, 3), 1), ((5, 1000, 3), 1),
    # the chunked kernels (C not 1 or 3): one chunk, a full chunk, full + partial chunks
    ((129, 97, 2), 1), ((128, 32, 4), 1), ((257, 255, 5), 1), ((33, 1241, 6), 1), ((131, 259, 7), 1),
    # two tiled stages: the second adjoint stage reads `top` from scratch the first wrote
    ((520, 530, 3), 2), ((1100, 900, 1), 2), ((512, 768, 4), 2), ((521, 770, 5), 2),
]
# (size, stages, the only levels that carry an upstream gradient): d_levels[l] = NULL for the others
MISSING_CASES = [((520, 530, 3), 2, (2,)), ((520, 530, 3), 2, (5,)), ((257, 255, 5), 1, (2,)), ((257, 255, 5), 1, (5,))]
K_SMALL_FLOATS = 64 * 64 * 3
# Roundings of one level of the adjoint, counted from up_texel: a fine texel gathers from at most 3 x 3 coarse texels (the
# windows that hold row r or r - 1: two, three where the range wraps); each term is one division by the window's count (the
# weight 0.25 * m_r * m_c is a power of two: exact), the terms are added one by one (the first to 0.0: exact): 9 + 8, and one
# more for the addition of g_l (for level 0 that addition is autograd's).  18, not the 28 a count of every operation gives.
ADJOINT_ROUNDINGS_PER_LEVEL = 18
_plan_reference_cache = {}


def _stages_by_rule(size):
    h, w, c = size
    n = min((max(h, w) - 1).bit_length() + 1, 8)
    stages = 0
    while 3 * stages + 3 < n and h * w * c > K_SMALL_FLOATS:
        stages += 1
        for _ in range(3):
            h, w = max(h // 2, 1), max(w // 2, 1)
    return stages


def _definition_level_torch(p):
    """_definition_level in torch double, so that autograd transposes it: wrap by index, windows by floor / ceil, a SCATTER of
    every window offset under autograd -- not the kernels' gather with its m_r, m_c multiplicities."""
    hp, wp = p.shape[0], p.shape[1]
    ho, wo = max(hp // 2, 1), max(wp // 2, 1)
    rows, cols = (torch.arange(hp) + 1) % hp, (torch.arange(wp) + 1) % wp
    b = (p + p[:, cols] + p[rows] + p[rows][:, cols]) / 4.0
    r0 = (torch.arange(ho) * hp) // ho
    r1 = -((-(torch.arange(ho) + 1) * hp) // ho)
    c0 = (torch.arange(wo) * wp) // wo
    c1 = -((-(torch.arange(wo) + 1) * wp) // wo)
    out = torch.zeros(ho, wo, p.shape[2], dtype=torch.float64)
    for dr in range(int((r1 - r0).max())):
        rsel = (r0 + dr < r1)[:, None, None]
        for dc in range(int((c1 - c0).max())):
            csel = (c0 + dc < c1)[None, :, None]
            out = out + b[torch.clamp(r0 + dr, max=hp - 1)][:, torch.clamp(c0 + dc, max=wp - 1)] * (rsel & csel)
    return out / ((r1 - r0)[:, None, None] * (c1 - c0)[None, :, None])


def _plan_reference(size, present):
    """Computed once per case and shared by the harness leg and the GPU legs of both builds: the fp32 inputs, the fp64 levels
    (numpy definition), the fp64 adjoint of the upstream gradients (autograd through the torch definition) and M_0, the same
    adjoint applied to their absolute values."""
    key = (size, present)
    if key not in _plan_reference_cache:
        gen = torch.Generator().manual_seed(1000 * size[0] + size[1] + size[2])
        texels = torch.rand(*size, generator=gen) * 2.0 - 0.5
        want_levels = _definition(texels.numpy())
        x = texels.double().requires_grad_(True)
        ref = [x]
        for _ in range(1, len(want_levels)):
            ref.append(_definition_level_torch(ref[-1]))
        for a, b in zip(ref, want_levels):            # the two statements of the definition agree
            assert tuple(a.shape) == tuple(b.shape) and float(np.abs(a.detach().numpy() - b).max()) <= 1e-14
        ups = [(torch.rand(*l.shape, generator=gen) - 0.4) if present is None or k in present else None
               for k, l in enumerate(ref)]
        used = [k for k, u in enumerate(ups) if u is not None]
        want_grad, = torch.autograd.grad([ref[k] for k in used], x, [ups[k].double() for k in used], retain_graph=True)
        m0, = torch.autograd.grad([ref[k] for k in used], x, [ups[k].double().abs() for k in used])
        _plan_reference_cache[key] = (texels, want_levels, ups, want_grad.numpy(), m0.numpy())
    return _plan_reference_cache[key]


def _run_plan_case(backend, device, size, stages, present, tag):
    """Forward bar: the one of _run_definition_case.  Adjoint bar, derived the same way: with M_l = |g_l| + A^T M_{l+1} (the
    fp64 adjoint applied to |g|), every partial sum that up_texel forms for a texel of level l is bounded by M_l, each of its
    ADJOINT_ROUNDINGS_PER_LEVEL roundings is at most 2^-24 of such a sum, and A^T (non-negative weights) carries an error
    bounded by e M_{l+1} into one bounded by e A^T M_{l+1} <= e M_l.  So |acc_0 - exact| <= K 2^-24 M_0 element by element with
    K = 18 x the levels below the top (at most 7) <= 126, to first order (the second-order terms are 1e-6 of that).  A dropped
    term or a wrong weight is off by 1e-2 M_0 or more in the texels it touches: more than 1000 bars."""
    assert stages == _stages_by_rule(size) == backend.mip_tiled_stages(*size), (size, stages)
    texels, want_levels, ups, want_grad, m0 = _plan_reference(size, present)
    x = texels.clone().to(device).requires_grad_(True)                # (a copy: the shared inputs stay as they are)
    levels = _texture_module().generate_mipmap(x, backend=backend)
    assert [tuple(l.shape) for l in levels] == [tuple(l.shape) for l in want_levels]
    bound = 84.0 * 2.0 ** -24 * float(texels.abs().max())
    worst = 0.0
    for l, (got, ref) in enumerate(zip(levels, want_levels)):
        err = float(np.abs(got.detach().cpu().numpy().astype(np.float64) - ref).max())
        worst = max(worst, err)
        assert err <= bound, (size, 'level', l, err, bound)
    used = [k for k, u in enumerate(ups) if u is not None]
    torch.autograd.backward([levels[k] for k in used], [ups[k].to(device) for k in used])
    k_bar = ADJOINT_ROUNDINGS_PER_LEVEL * (len(levels) - 1)
    err = np.abs(x.grad.cpu().numpy().astype(np.float64) - want_grad)
    units = float(np.max(np.where(m0 > 0.0, err / np.where(m0 > 0.0, m0, 1.0), np.where(err > 0.0, np.inf, 0.0)))) * 2.0 ** 24
    name = 'texture_plan_%s%s' % (mt.size_tag(size), '' if present is None else '_only%d' % present[0])
    print(name, tag, 'stages %d: levels max abs error %.3e (bar %.3e); d_texels max error / M_0 = %.2f x 2^-24 (bar %d x 2^-24)'
          % (stages, worst, bound, units, k_bar))
    amax = float(texels.abs().max())
    parity_util.record(name, {'levels': {'rel_l2': worst / amax, 'tol': bound / amax, 'flipped_rows': 0,
                                         'measure': 'max |error| over all levels / max |texels|'},
                              'd_texels': {'rel_l2': units * 2.0 ** -24, 'tol': k_bar * 2.0 ** -24, 'flipped_rows': 0,
                                           'measure': 'max over the elements of |error| / M_0'}}, tag)
    assert float(m0.min()) >= 0.0 and units <= k_bar, (size, present, units, k_bar)


_plan_ids = [mt.size_tag(s) for s, _ in PLAN_CASES]
_missing_ids = ['%s_only%d' % (mt.size_tag(s), p[0]) for s, _, p in MISSING_CASES]


@pytest.mark.parametrize('size,stages', PLAN_CASES, ids=_plan_ids)
def test_launch_plan_values_hostsim(hostsim_backend, size, stages):
    """The per-texel bodies alone (the harness has no launch plan): proves the definitions and the bars before the GPU leg."""
    _run_plan_case(hostsim_backend, CPU, size, stages, None, 'hostsim')


@pytest.mark.gpu
@pytest.mark.parametrize('size,stages', PLAN_CASES, ids=_plan_ids)
def test_launch_plan_values_gpu(gpu_backend, size, stages):
    _run_plan_case(gpu_backend, GPU, size, stages, None, 'gpu')


@pytest.mark.parametrize('size,stages,present', MISSING_CASES, ids=_missing_ids)
def test_launch_plan_missing_level_gradients_hostsim(hostsim_backend, size, stages, present):
    _run_plan_case(hostsim_backend, CPU, size, stages, present, 'hostsim')


@pytest.mark.gpu
@pytest.mark.parametrize('size,stages,present', MISSING_CASES, ids=_missing_ids)
def test_launch_plan_missing_level_gradients_gpu(gpu_backend, size, stages, present):
    """d_levels[l] = NULL inside the tiled adjoint (G reads as zeros) and as the chain's start."""
    _run_plan_case(gpu_backend, GPU, size, stages, present, 'gpu')


# ---- 4. adjoint identity, constants ---------------------------------------------------------------------------------------------
def _run_adjoint_identity(backend, device, size):
    gen = torch.Generator().manual_seed(77 + size[1])
    x = (torch.rand(*size, generator=gen) - 0.3).to(device).requires_grad_(True)
    levels = _texture_module().generate_mipmap(x, backend=backend)
    ys = [(torch.rand(*l.shape, generator=gen) - 0.4).to(device) for l in levels]
    if len(levels) == 1:                              # a 1 x 1 image: no map to transpose
        assert levels[0].data_ptr() == x.data_ptr()
        return
    torch.autograd.backward(levels[1:], ys[1:])
    lhs = sum(float((l.detach().double() * y.double()).sum()) for l, y in zip(levels[1:], ys[1:]))
    rhs = float((x.detach().double() * x.grad.double()).sum())
    print('adjoint identity', mt.size_tag(size), lhs, rhs)
    assert lhs != 0.0 and abs(lhs - rhs) <= 1e-5 * abs(lhs), (size, lhs, rhs)


@pytest.mark.parametrize('size', ADJOINT_SIZES, ids=mt.size_tag)
def test_adjoint_identity_hostsim(hostsim_backend, size):
    _run_adjoint_identity(hostsim_backend, CPU, size)


@pytest.mark.gpu
@pytest.mark.parametrize('size', ADJOINT_SIZES + [(1023, 517, 1), (512, 768, 4)], ids=mt.size_tag)
def test_adjoint_identity_gpu(gpu_backend, size):
    _run_adjoint_identity(gpu_backend, GPU, size)


def _run_constant(backend, device):
    for size in [(64, 64, 3), (256, 128, 3), (8, 2, 1), (512, 512, 5)]:
        texels = torch.full(size, 0.3, device=device)
        for l in _texture_module().generate_mipmap(texels, backend=backend):
            assert bool((l == texels[0, 0, 0]).all()), (size, tuple(l.shape))


def test_constant_image_hostsim(hostsim_backend):
    _run_constant(hostsim_backend, CPU)


@pytest.mark.gpu
def test_constant_image_gpu(gpu_backend):
    _run_constant(gpu_backend, GPU)


def test_missing_level_gradients_hostsim(hostsim_backend):
    """Levels the loss does not touch reach the native call as NULL (= zeros): the gradient is that of the touched levels."""
    tx = _texture_module()
    x = torch.rand(40, 24, 3, generator=torch.Generator().manual_seed(3)).requires_grad_(True)
    levels = tx.generate_mipmap(x, backend=hostsim_backend)
    up = mk.upstream(levels[2].shape)
    (levels[2] * up).sum().backward()
    only2 = x.grad.clone()
    x.grad = None
    levels = tx.generate_mipmap(x, backend=hostsim_backend)
    (sum((l * 0.0).sum() for l in levels) + (levels[2] * up).sum()).backward()
    assert only2.abs().sum() > 0 and torch.equal(only2, x.grad)


# ---- 5. bitwise reproducible ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('size', [(1024, 1024, 3), (255, 129, 3)], ids=mt.size_tag)
def test_bitwise_reproducible_gpu(gpu_backend, size):
    tx = _texture_module()
    texels = torch.rand(*size, generator=torch.Generator().manual_seed(9)).to(GPU)
    runs = []
    for _ in range(2):
        x = texels.clone().requires_grad_(True)
        levels = tx.generate_mipmap(x, backend=gpu_backend)
        mt.pyramid_loss(levels[1:]).backward()
        runs.append([l.detach().cpu().numpy().tobytes() for l in levels[1:]] + [x.grad.cpu().numpy().tobytes()])
    assert runs[0] == runs[1]


# ---- 6. setters, a small optimisation -------------------------------------------------------------------------------------------
def test_setters_hostsim(hostsim_backend):
    import redner_amd
    gen = torch.Generator().manual_seed(1)
    a, b = torch.rand(16, 8, 3, generator=gen), torch.rand(16, 8, 3, generator=gen) + 0.5
    tex = redner_amd.Texture(a, backend=hostsim_backend)
    assert len(tex.mipmap) == 5 and not tex.constant and tex.device == a.device
    before = [l.clone() for l in tex.mipmap]
    tex.texels = b
    assert tex.texels is b and len(tex.mipmap) == 5
    assert all(not torch.equal(x, y) for x, y in zip(before, tex.mipmap))
    assert torch.equal(tex.mipmap[1], redner_amd.generate_mipmap(b, backend=hostsim_backend)[1])
    back = redner_amd.Texture.load_state_dict(tex.state_dict())
    assert isinstance(back, redner_amd.Texture) and all(torch.equal(x, y) for x, y in zip(back.mipmap, tex.mipmap))

    env = redner_amd.EnvironmentMap(mt.envmap_values(), backend=hostsim_backend)
    assert isinstance(env.values, redner_amd.Texture) and len(env.values.mipmap) == 6
    cdf_xs, cdf_ys, norm = env.sample_cdf_xs.clone(), env.sample_cdf_ys.clone(), env.pdf_norm
    env.values = redner_amd.Texture(mt.envmap_values().flip(1) * 2.0, backend=hostsim_backend)
    assert not torch.equal(cdf_xs, env.sample_cdf_xs) and env.pdf_norm != norm and env.sample_cdf_ys.shape == cdf_ys.shape
    e2w = torch.eye(4)
    e2w[0, 3] = 2.0
    env.env_to_world = e2w
    assert torch.equal(env.world_to_env, torch.inverse(e2w).contiguous())
    back = redner_amd.EnvironmentMap.load_state_dict(env.state_dict())
    assert back.pdf_norm == env.pdf_norm and torch.equal(back.sample_cdf_xs, env.sample_cdf_xs)
    assert torch.equal(back.values.mipmap[2], env.values.mipmap[2])


def test_texture_fit_lowers_loss_hostsim(hostsim_backend):
    """Three Adam steps on a 64 x 64 diffuse texture towards a target render (32 x 32 frame): the loss goes down."""
    import redner_amd
    import scenes
    from redner_amd.render_pytorch import Material, RenderFunction
    rd = hostsim_backend

    def render(tex):
        sc = scenes.textured_sphere(CPU, resolution=(32, 32))
        sc.materials[0] = Material(diffuse_reflectance=tex, specular_reflectance=torch.tensor([0.1, 0.1, 0.1]),
                                   roughness=torch.tensor([0.5]))
        sc.materials[1] = Material(diffuse_reflectance=torch.tensor([0.6, 0.55, 0.5]))
        for sh in sc.shapes:
            for name in ('vertices', 'uvs', 'normals', 'colors'):
                if getattr(sh, name) is not None:
                    getattr(sh, name).requires_grad_(False)
        args = RenderFunction.serialize_scene(sc, (2, 2), 1, sampler_type=rd.SamplerType.sobol, device=CPU, backend=rd)
        return RenderFunction.apply(5, *args)

    target_texels = torch.from_numpy(scenes._procedural(64, 64, 3, 0.4))
    target = render(redner_amd.Texture(target_texels, backend=rd)).detach()
    texels = torch.full((64, 64, 3), 0.5, requires_grad=True)
    tex = redner_amd.Texture(texels, backend=rd)
    opt = torch.optim.Adam([texels], lr=5e-2)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        tex.texels = texels                           # rebuilds the pyramid from the updated image
        loss = (render(tex) - target).pow(2).sum()
        loss.backward()
        assert tuple(texels.grad.shape) == (64, 64, 3) and float(texels.grad.abs().sum()) > 0
        opt.step()
        losses.append(float(loss.detach()))
    tex.texels = texels
    losses.append(float((render(tex) - target).pow(2).sum().detach()))
    print('texture fit losses', losses)
    assert losses[-1] < losses[0] and all(b < a for a, b in zip(losses, losses[1:]))


# ---- 7. unchanged behaviour, argument checks ------------------------------------------------------------------------------------
def test_one_level_classes_unchanged(hostsim_backend):
    import redner_amd
    from redner_amd import render_pytorch as rp
    image = torch.rand(8, 8, 3)
    assert len(rp.Texture(image).mipmap) == 1 and rp.Texture(image).mipmap[0] is image
    levels = [image, torch.rand(4, 4, 3)]
    assert rp.Texture(levels).mipmap == levels and not rp.Texture(levels).constant
    const = torch.tensor([0.2, 0.3, 0.4])
    for cls in (rp.Texture, lambda t: redner_amd.Texture(t, backend=hostsim_backend)):
        t = cls(const)
        assert t.constant and len(t.mipmap) == 1 and t.mipmap[0] is const
    kept = redner_amd.Texture(levels, backend=hostsim_backend)
    assert kept.mipmap == levels and not kept.constant
    env = rp.EnvironmentMap(mt.envmap_values())
    assert len(env.values.mipmap) == 1
    assert isinstance(redner_amd.Texture(image, backend=hostsim_backend), rp.Texture)
    assert isinstance(redner_amd.EnvironmentMap(mt.envmap_values(), backend=hostsim_backend), rp.EnvironmentMap)


def test_native_argument_checks_hostsim(hostsim_backend):
    import ctypes as C
    from redner_amd import _capi
    rd, lib = hostsim_backend, _capi.lib()
    assert [rd.mip_num_levels(h, w) for h, w in [(1, 1), (1, 2), (2, 2), (3, 1), (40, 7), (128, 128), (129, 1), (4096, 4096)]] == \
        [1, 2, 2, 3, 7, 8, 8, 8]
    assert all(rd.mip_num_levels(w, 1) == min((w - 1).bit_length() + 1, 8) for w in range(1, 3000))
    assert rd.mip_num_levels(0, 4) == 0
    a, b = torch.rand(4, 4, 1), torch.empty(2, 2, 1)
    table = (C.c_void_p * 2)(a.data_ptr(), b.data_ptr())
    assert lib.rdr_mip_pyramid(4, 4, 1, 2, table, -1) != 0 and 'num_levels' in _capi.last_error()
    assert lib.rdr_mip_pyramid(4, 0, 1, 3, table, -1) != 0 and 'positive' in _capi.last_error()
    with pytest.raises(RuntimeError):
        _texture_module().generate_mipmap(torch.rand(4, 4), backend=rd)
    with pytest.raises(RuntimeError):
        _texture_module().generate_mipmap(torch.rand(4, 4, 3).double(), backend=rd)


@pytest.mark.gpu
def test_product_library_refuses_host_tensors_gpu(gpu_backend):
    """No torch fall-back and no silent CPU path: CPU tensors are for the harness library only."""
    with pytest.raises(RuntimeError, match='harness'):
        _texture_module().generate_mipmap(torch.rand(8, 8, 3), backend=gpu_backend)


@pytest.mark.gpu
def test_readme_snippet_gpu(gpu_backend):
    from redner_amd import EnvironmentMap, Texture, generate_mipmap           # noqa: F401
    texels = torch.full((256, 256, 3), 0.5, device=GPU, requires_grad=True)
    tex = Texture(texels, backend=gpu_backend)
    assert [tuple(l.shape) for l in tex.mipmap] == [(256 >> l, 256 >> l, 3) for l in range(8)]
    sum(l.sum() for l in tex.mipmap).backward()
    # every level's texels average the image with total weight 1 per coarse texel: the gradient sums to the number of texels
    total = sum(l.numel() for l in tex.mipmap)
    assert tuple(texels.grad.shape) == (256, 256, 3) and abs(float(texels.grad.double().sum()) - total) < 1e-3 * total
