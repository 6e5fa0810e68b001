"""Spherical-harmonic utilities (pyredner/utils.py) on the native kernels of csrc/sh_envmap.h.

    coeffs = torch.zeros(3, 16, device=dev, requires_grad=True)        # [C, N]: int(sqrt(N)) bands, at most 8
    envmap = EnvironmentMap(SH_reconstruct(coeffs, (128, 128)))        # rdr_sh_reconstruct, then the pyramid and the tables
    loss(render(scene)).backward()                                     # coeffs.grad: rdr_sh_reconstruct_backward

The meaning is the reference's SH_reconstruct (pyredner/utils.py:10-60), restated in csrc/sh_envmap.h:

    out[r, c, ch] = max(sum_i Y_i(theta_r, phi_c) * coeffs[ch, i], 0),   theta_r = pi (r + 0.5) / H,  phi_c = 2 pi (c + 0.5) / W

in fp32 in the reference's order of operations; the columns of `coeffs` past int(sqrt(N))^2 are not read.  The gradient is a
reduction in a fixed order (fp64 partial sums per tile, no float atomics): bitwise reproducible.  At a pixel whose unclamped sum
is exactly 0 the clamp passes half of the upstream gradient, as torch.max(a, 0) does.

One native call forward and one backward.  There is no torch fall-back: the tensors' memory goes to the loaded native library.
CPU tensors are accepted by the CPU debugging harness only (the test-suite loads it); the product library raises for them.
"""
import torch

from . import redner as _default_backend
from ._op import first_order_only, named, place, ptr, scratch, upstream


class SHReconstruct(torch.autograd.Function):
    """coeffs [C, N] fp32 -> image [H, W, C] on the coefficients' device."""

    @staticmethod
    def forward(ctx, coeffs, height, width, backend=None):
        rd = backend or _default_backend
        base = coeffs.detach().contiguous()
        channels, num_coeffs = (int(v) for v in base.shape)
        use_gpu, index = place(base)
        image = torch.empty(height, width, channels, dtype=torch.float32, device=base.device)
        clamp = torch.empty(height, width, channels, dtype=torch.uint8, device=base.device) if ctx.needs_input_grad[0] else None
        rd.sh_reconstruct(ptr(rd, base), ptr(rd, image), None if clamp is None else clamp.data_ptr(), channels, num_coeffs, height,
                          width, use_gpu, index)
        ctx.rd, ctx.geometry, ctx.clamp = rd, (channels, num_coeffs, height, width, use_gpu, index), clamp
        return image

    @staticmethod
    def backward(ctx, d_image):
        first_order_only('SHReconstruct')
        rd = ctx.rd
        channels, num_coeffs, height, width, use_gpu, index = ctx.geometry
        clamp = ctx.clamp
        g = upstream(d_image, clamp.device)
        d_coeffs = torch.empty(channels, num_coeffs, dtype=torch.float32, device=clamp.device)
        count = rd.sh_backward_scratch(height, width, channels, num_coeffs)
        work = scratch(count, clamp.device)
        rd.sh_reconstruct_backward(clamp.data_ptr(), ptr(rd, g), ptr(rd, d_coeffs), ptr(rd, work), count, channels, num_coeffs, height,
                                   width, use_gpu, index)
        return d_coeffs, None, None, None


def SH_reconstruct(coeffs, res, backend=None):
    """pyredner.SH_reconstruct: the [res[0], res[1], C] fp32 image of the spherical-harmonic coefficients `coeffs` [C, N], clamped
    at 0, on the coefficients' device.  Differentiable with respect to `coeffs` (which need not be contiguous), once: under create_graph=True the backward call raises."""
    if not isinstance(coeffs, torch.Tensor) or coeffs.dim() != 2 or coeffs.numel() == 0:
        raise ValueError('SH_reconstruct: coeffs must be a [C, N] tensor with C, N >= 1')
    if coeffs.dtype != torch.float32:
        raise ValueError('SH_reconstruct: fp32 coeffs only, got %s' % (coeffs.dtype,))
    if len(res) != 2 or int(res[0]) <= 0 or int(res[1]) <= 0:
        raise ValueError('SH_reconstruct: res must be (height, width), both positive, got %s' % (tuple(res),))
    with named('SH_reconstruct'):
        return SHReconstruct.apply(coeffs, int(res[0]), int(res[1]), backend)
