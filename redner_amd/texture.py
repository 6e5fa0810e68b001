"""Mip-mapped textures and environment maps (pyredner/texture.py, pyredner/envmap.py) on the native pyramid kernels.

    texels = torch.full((256, 256, 3), 0.5, device=dev, requires_grad=True)
    mat = Material(diffuse_reflectance=Texture(texels))        # the pyramid is built here: rdr_mip_pyramid
    loss(render(scene)).backward()                             # texels.grad holds the sum over ALL levels

The meaning is the reference's Texture.generate_mipmap (pyredner/texture.py:34-69).  For texels [H, W, C]:

  * num_levels = min(ceil(log2(max(H, W))) + 1, 8); level 0 is the image.  A side that is not a power of two reaches 1 early
    and the last levels repeat at 1 x 1 (40 wide: 40, 20, 10, 5, 2, 1, 1).
  * level l + 1 (Ho x Wo = max(Hp // 2, 1) x max(Wp // 2, 1)) from level l (P, Hp x Wp):
        B[r, c]   = (P[r, c] + P[r, c+1] + P[r+1, c] + P[r+1, c+1]) / 4          indices wrap
        out[i, j] = mean of B[floor(i Hp / Ho) : ceil((i + 1) Hp / Ho), floor(j Wp / Wo) : ceil((j + 1) Wp / Wo)]
    (an even side: the wrapping [1 2 1] / 4 filter at stride 2; an odd side: overlapping windows of 3; a side of 1: identity)
  * backward: d_texels = g_0 + A_1^T (g_1 + A_2^T (g_2 + ...)), with A_l the linear map from level l - 1 to level l and g_l the
    gradient the renderer wrote for level l (a level it did not touch counts as zero).

Gradient flow needs nothing from RenderFunction: the levels 1.. are non-leaf tensors made by `MipPyramid`, RenderFunction.backward
returns one gradient per level tensor as it does for hand-made levels, and autograd hands them to `MipPyramid.backward`, which
is one native call (rdr_mip_pyramid_backward: a gather, no atomics, bitwise reproducible).  Level 0 is `texels.contiguous()`,
handed back OUTSIDE the Function: autograd itself adds g_0 to what `MipPyramid.backward` returns, and the Function never
returns its own input.

There is no torch fall-back: the tensors' memory goes to the loaded native library.  CPU tensors are accepted by the CPU
debugging harness only (the test-suite loads it); the product library raises for them.

`render_pytorch.Texture` / `render_pytorch.EnvironmentMap` keep their one-level behaviour; the classes here derive from them
and are accepted wherever those are (Material, Scene, RenderFunction.serialize_scene).
"""
import math

import torch

from . import redner as _default_backend
from . import render_pytorch
from ._op import first_order_only, named, place, ptr, scratch, upstream


def _level_sizes(height, width, num_levels):
    sizes = [(height, width)]
    for _ in range(1, num_levels):
        height, width = max(height // 2, 1), max(width // 2, 1)
        sizes.append((height, width))
    return sizes


class MipPyramid(torch.autograd.Function):
    """texels [H, W, C] -> the levels 1 .. num_levels - 1 (fresh tensors on the texels' device).  One native call forward, one
    backward.  Needs an image of more than one level (generate_mipmap handles 1 x 1)."""

    @staticmethod
    def forward(ctx, texels, backend=None):
        rd = backend or _default_backend
        if texels.dim() != 3 or texels.numel() == 0:
            raise RuntimeError('MipPyramid: texels must be [H, W, C] with H, W, C >= 1, got %s' % (tuple(texels.shape),))
        if texels.dtype != torch.float32:
            raise RuntimeError('MipPyramid: fp32 texels only')
        base = texels.detach().contiguous()
        h, w, c = (int(v) for v in base.shape)
        sizes = _level_sizes(h, w, rd.mip_num_levels(h, w))
        if len(sizes) < 2:
            raise RuntimeError('MipPyramid: a 1 x 1 image has no further levels')
        levels = [base] + [torch.empty(hl, wl, c, dtype=torch.float32, device=base.device) for hl, wl in sizes[1:]]
        use_gpu, index = place(base)
        rd.mip_pyramid([ptr(rd, l) for l in levels], h, w, c, use_gpu, index)
        ctx.rd, ctx.geometry, ctx.device = rd, (h, w, c, use_gpu, index), base.device
        ctx.set_materialize_grads(False)
        return tuple(levels[1:])

    @staticmethod
    def backward(ctx, *d_levels):
        first_order_only('MipPyramid')
        rd = ctx.rd
        h, w, c, use_gpu, index = ctx.geometry
        d_texels = torch.empty(h, w, c, dtype=torch.float32, device=ctx.device)
        count = rd.mip_backward_scratch(h, w, c)
        work = scratch(count, ctx.device)
        grads = [None] + [upstream(g, ctx.device) for g in d_levels]                                     # g_0: autograd adds it
        rd.mip_pyramid_backward([ptr(rd, g) for g in grads], ptr(rd, d_texels), ptr(rd, work), count, h, w, c, use_gpu, index)
        return d_texels, None


def generate_mipmap(texels, backend=None):
    """The reference's pyramid of an [H, W, C] fp32 image: a list of [Hl, Wl, C] tensors, [0] being `texels.contiguous()`.
    Differentiable: the gradients of all levels reach `texels`.  Once: under create_graph=True the backward call raises."""
    if not isinstance(texels, torch.Tensor) or texels.dim() != 3:
        raise RuntimeError('generate_mipmap: texels must be an [H, W, C] tensor')
    base = texels.contiguous()
    if max(int(base.shape[0]), int(base.shape[1])) <= 1:
        if base.numel() == 0 or base.dtype != torch.float32:
            raise RuntimeError('generate_mipmap: texels must be fp32 with H, W, C >= 1')
        return [base]
    return [base] + list(MipPyramid.apply(texels, backend))


class Texture(render_pytorch.Texture):
    """pyredner.Texture: a constant (1-D tensor) or an [H, W, C] image whose mip pyramid is built at construction and again on
    every assignment to `.texels`.  (A list of levels is kept as it is, like render_pytorch.Texture does.)"""

    def __init__(self, texels, uv_scale=None, backend=None):
        self._backend = backend
        self.uv_scale = uv_scale if uv_scale is not None else torch.tensor([1.0, 1.0])
        assert self.uv_scale.dtype == torch.float32
        self._texels = texels
        self.generate_mipmap()

    def generate_mipmap(self):
        texels = self._texels
        if not isinstance(texels, torch.Tensor):
            self.mipmap, self.constant = list(texels), False
            return
        assert texels.dtype == torch.float32
        if texels.dim() >= 2:
            self.mipmap, self.constant = generate_mipmap(texels, self._backend), False
        else:
            self.mipmap, self.constant = [texels], True

    @property
    def texels(self):
        return self._texels

    @texels.setter
    def texels(self, value):
        self._texels = value
        self.generate_mipmap()

    @property
    def device(self):
        t = self._texels
        return (t if isinstance(t, torch.Tensor) else t[0]).device

    def state_dict(self):
        return {'texels': self.texels, 'mipmap': self.mipmap, 'uv_scale': self.uv_scale}

    @classmethod
    def load_state_dict(cls, state_dict):
        out = cls.__new__(cls)
        out._backend = None
        out._texels = state_dict['texels']
        out.mipmap = state_dict['mipmap']
        out.constant = isinstance(out._texels, torch.Tensor) and out._texels.dim() == 1
        out.uv_scale = state_dict['uv_scale'].to(torch.device('cpu'))
        return out


_y_weights = {}                 # (H, device) -> sin(pi (y + 0.5) / H), the weights of the rows of a latitude-longitude map, on that device


def _y_weight(height, device):
    key = (height, str(device))
    if key not in _y_weights:
        # the very expression of render_pytorch.EnvironmentMap.generate_envmap_pdf, evaluated ON THE CPU as the reference's tables
        # are and copied to the texels' device once: the device's own sin differs from the CPU's in the last bit of some rows
        # (seen at 16 rows on an MI355X), and with it sample_cdf_ys would not be the reference's table
        _y_weights[key] = torch.sin(math.pi * (torch.arange(height, dtype=torch.float32, device='cpu') + 0.5)
                                    / float(height)).contiguous().to(device)
    return _y_weights[key]


def envmap_sampling_tables(texels, backend=None):
    """(sample_cdf_ys [H], sample_cdf_xs [H, W], pdf_norm) of an environment map with level 0 `texels` [H, W, 3] fp32
    (pyredner/envmap.py:36-60), by one native call (rdr_envmap_tables, csrc/sh_envmap.h).  The running sums are taken as
    torch.cumsum takes them on the CPU -- a sequential fp64 accumulator rounded to fp32 at every output -- also on the device,
    where torch's scan associates differently: the tables of a map built on the device are the reference's.  For CPU tensors
    (the CPU debugging harness) all three results are bit for bit those of render_pytorch.EnvironmentMap.generate_envmap_pdf."""
    rd = backend or _default_backend
    if not isinstance(texels, torch.Tensor) or texels.dim() != 3 or int(texels.shape[2]) != 3 or texels.numel() == 0:
        raise RuntimeError('envmap_sampling_tables: texels must be an [H, W, 3] tensor with H, W >= 1, got %s'
                           % (tuple(texels.shape) if isinstance(texels, torch.Tensor) else type(texels),))
    if texels.dtype != torch.float32:
        raise RuntimeError('envmap_sampling_tables: fp32 texels only')
    base = texels.detach().contiguous()
    h, w = int(base.shape[0]), int(base.shape[1])
    use_gpu, index = place(base)
    y_weight = _y_weight(h, base.device)
    cdf_ys = torch.empty(h, dtype=torch.float32, device=base.device)
    cdf_xs = torch.empty(h, w, dtype=torch.float32, device=base.device)
    with named('envmap_sampling_tables'):
        total = rd.envmap_tables(ptr(rd, base), ptr(rd, y_weight), ptr(rd, cdf_ys), ptr(rd, cdf_xs), h, w, use_gpu, index)
    pdf_norm = (h * w) / (total * (2 * math.pi * math.pi))
    return cdf_ys, cdf_xs, pdf_norm


class EnvironmentMap(render_pytorch.EnvironmentMap):
    """pyredner.EnvironmentMap: a tensor becomes a mip-mapped Texture; assigning `.values` rebuilds the sampling tables
    (from level 0, by envmap_sampling_tables: one native call), assigning `.env_to_world` refreshes `world_to_env`."""

    def __init__(self, values, env_to_world=None, directly_visible=True, backend=None):
        if isinstance(values, torch.Tensor):
            values = Texture(values, backend=backend)
        env_to_world = env_to_world if env_to_world is not None else torch.eye(4, 4)
        assert env_to_world.dtype == torch.float32
        self._backend = backend
        self.directly_visible = directly_visible
        self.env_to_world = env_to_world
        self.values = values

    def generate_envmap_pdf(self):
        backend = getattr(self, '_backend', None) or getattr(self._values, '_backend', None)
        self.sample_cdf_ys, self.sample_cdf_xs, self.pdf_norm = envmap_sampling_tables(self._values.mipmap[0], backend)

    @property
    def values(self):
        return self._values

    @values.setter
    def values(self, value):
        self._values = value
        self.generate_envmap_pdf()

    @property
    def env_to_world(self):
        return self._env_to_world

    @env_to_world.setter
    def env_to_world(self, value):
        self._env_to_world = value
        self.world_to_env = torch.inverse(value).contiguous()

    def state_dict(self):
        return {'values': self.values.state_dict(), 'env_to_world': self.env_to_world, 'world_to_env': self.world_to_env,
                'sample_cdf_ys': self.sample_cdf_ys, 'sample_cdf_xs': self.sample_cdf_xs, 'pdf_norm': self.pdf_norm,
                'directly_visible': self.directly_visible}

    @classmethod
    def load_state_dict(cls, state_dict):
        out = cls.__new__(cls)
        out._values = Texture.load_state_dict(state_dict['values'])
        out._env_to_world = state_dict['env_to_world']
        out.world_to_env = state_dict['world_to_env']
        out.sample_cdf_ys = state_dict['sample_cdf_ys']
        out.sample_cdf_xs = state_dict['sample_cdf_xs']
        out.pdf_norm = state_dict['pdf_norm']
        out.directly_visible = state_dict['directly_visible']
        return out
